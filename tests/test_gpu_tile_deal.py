"""k_chol_solve_lds<0> with its tile rows dealt to the owner waves by the window's tile skyline (pack_plan.hpp planTileDeal;
DESIGN.md: "the tile rows dealt by the skyline") against the same kernel on its closed-form deal (SVIN_NO_TILE_DEAL).  The deal says
which wave computes a tile row and nothing else: no tile's arithmetic or its order changes, so everything the solver produces must
be EQUAL between the two, bit for bit -- and a deal that left a flag without its writer would end in the solver's bounded spin and
cholFail bit 4, which every run here holds clear.

Every window is built twice, one handle packed with the planned deal and one with SVIN_NO_TILE_DEAL.  Compared: the word the handle
reports against the planner's own answer for the handle's skyline (tests/csrc/tile_deal_shim.cpp) or zero; one trust-region
iteration at three damping values; the states and the summary after optimize(3) and after seven iterations more; and the system the
handle has just solved through svin_ba_debug_solve_dense_profiled, which plans the deal from the profile it is given, with the switch
off and on.  The windows are tiny -- the solver sees d only: P = 6 (six tile rows: no row to move), P = 8 .. 11 (the quiet wave
holds no row at eight tile rows and rows 2 | 2, 3 | 2, 3, 4 at nine, ten, eleven), and a P = 10 window on the dense profile, where
the word must stay zero.  (The estimator cannot build a window whose prior covers every block -- a marginalisation prior reaches
the oldest speed / bias block only -- so that window is packed with SVIN_NO_TILE_SKYLINE; the profile of a prior over all blocks
itself goes through the planner in tests/test_tile_deal_host.py.)

A batch of two windows with different words keeps both words through the batched solve and gives each window the states it reaches
alone.  A system with one non-positive pivot reports the same cholFail on both deals: bit 2, a numerical event, with bits 4 | 8 clear."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import tile_deal_lib as td  # noqa: E402
import tile_skyline_lib as ts  # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402

pytestmark = pytest.mark.gpu
NO_DEAL, NO_SKYLINE = "SVIN_NO_TILE_DEAL", "SVIN_NO_TILE_SKYLINE"
SUMMARY = ("initial_cost", "final_cost", "iterations", "successful", "termination")
MUS = (1e-4, 1e-8, 1e-7)
# name -> (keyframes, packed on the dense profile, rows of the quiet wave in the closed form)
WINDOWS = {"P6": (6, False, []), "P8": (8, False, []), "P9": (9, False, [2]), "P10": (10, False, [2, 3]), "P11": (11, False, [2, 3, 4]),
           "P10_dense": (10, True, [2, 3])}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return td.build_shim(tmp_path_factory.mktemp("tile_deal_gpu"))


def build(P, seed=5, **kw):
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=P, L=40, n_obs=320, seed=seed, **kw)
    est = Estimator(0)
    fids, lids = syn.feed(est, spec)
    return est, fids, lids


def states_of(est, fids, lids):
    T = np.stack([est.get_T_WS(f) for f in fids])
    sb = np.stack([est.get_speed_and_bias(f) for f in fids])
    lms = est.get_landmarks()
    lm = np.stack([np.r_[lms[l]["point"], lms[l]["quality"]] for l in lids])
    return T, sb, lm


def run(P, dense, deal, debug_option):
    debug_option(NO_DEAL, 0 if deal else 1)
    debug_option(NO_SKYLINE, 1 if dense else 0)
    est, fids, lids = build(P)
    out = dict(steps=[])
    for mu in MUS:
        r = est.debug_trust_region_step(mu, 1e4, 0)
        assert (r["scalars"]["cholFail"] & 12) == 0 and r["scalars"]["failMax"] < 4
        out["steps"].append(r)
    out["cut"], out["word"] = est.debug_tile_skyline()[0], est.debug_tile_deal()
    est.optimize(3)
    out["after3"] = (states_of(est, fids, lids), {k: est.summary()[k] for k in SUMMARY})
    est.optimize(7)
    out["after10"] = (states_of(est, fids, lids), {k: est.summary()[k] for k in SUMMARY})
    assert est.debug_tile_deal() == out["word"]
    out["est"] = est
    return out


def assert_equal_runs(a, b, name):
    for mu, ra, rb in zip(MUS, a["steps"], b["steps"]):
        for key in ("y_C", "v_C", "y_L", "v_L"):
            assert np.array_equal(ra[key], rb[key]), "%s, mu %g: %s differs by %.3e" % (name, mu, key, float(np.max(np.abs(ra[key] - rb[key]))))
        for key, v in ra["scalars"].items():
            assert np.array_equal(np.asarray(v), np.asarray(rb["scalars"][key])), (name, mu, key, v, rb["scalars"][key])
    for stage in ("after3", "after10"):
        (sa, ma), (sb, mb) = a[stage], b[stage]
        assert ma == mb, (name, stage, ma, mb)
        for what, x, y in zip(("poses", "speed / bias", "landmarks"), sa, sb):
            assert np.array_equal(x, y), "%s, %s: %s differ by %.3e" % (name, stage, what, float(np.max(np.abs(x - y))))


def assert_same_system_solves(est, cut, name, debug_option):
    """the system the handle has just solved, through the direct solve inside its profile on both deals"""
    from svin_amd.estimator import Estimator
    for mu in MUS:
        est.debug_reduced_solve(mu, fused=False)
        S, g = est.debug_last_system()
        d = len(g)
        dpad = (d + 15) // 16 * 16
        buf = np.zeros((dpad, dpad))
        buf[:d, :d] = S
        debug_option(NO_DEAL, 0)
        dealt = Estimator.debug_solve_dense(buf, g, d, padded=True, ldS=dpad, tile_cut=cut)
        debug_option(NO_DEAL, 1)
        closed = Estimator.debug_solve_dense(buf, g, d, padded=True, ldS=dpad, tile_cut=cut)
        debug_option(NO_DEAL, 0)
        assert dealt["route"] == closed["route"] == 0, (name, dealt["route"])   # kRouteLdsWhole
        assert dealt["cholFail"] == closed["cholFail"] and (dealt["cholFail"] & 12) == 0, (name, mu, dealt["cholFail"], closed["cholFail"])
        assert np.array_equal(dealt["y"], closed["y"]), "%s, mu %g: y of one system differs by %.3e between the deals" % (
            name, mu, float(np.max(np.abs(dealt["y"] - closed["y"]))))


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_window_on_the_planned_deal_equals_the_closed_form(gpu_lib, debug_option, shim, name):
    P, dense, quiet_rows = WINDOWS[name]
    dealt = run(P, dense, True, debug_option)
    closed = run(P, dense, False, debug_option)
    d = dealt["steps"][0]["d"]
    nT = (d + 15) // 16
    assert d == 15 * P and dealt["cut"] == closed["cut"]
    hi = ts.unpack(dealt["cut"], nT)
    base = td.decode(shim, 0, nT)
    assert [I for I in sorted(base) if base[I] == td.QUIET] == quiet_rows
    want = int(shim.td_plan_cut(nT, dealt["cut"]))
    owner = td.decode(shim, dealt["word"], nT)
    print("%s: d %d, %d tile rows, skyline %s, deal %#x: %s" % (name, d, nT, hi, dealt["word"], owner))
    assert closed["word"] == 0, "SVIN_NO_TILE_DEAL left a deal"
    assert dealt["word"] == want, (name, hex(dealt["word"]), hex(want))
    td.check_deal(hi, owner)
    if dense or nT <= 7:
        assert dealt["word"] == 0
    if name == "P10":
        assert hi == [5, 7, 8, 9, 9, 9, 9, 9, 9, 9] and dealt["word"] == (2 << 8) | (1 << 12)
    if name in ("P9", "P10", "P11"):   # the quiet wave's rows have moved: these windows do exercise a planned deal
        assert dealt["word"] != 0 and all(owner[I] != td.QUIET for I in quiet_rows), (name, owner)
    assert_equal_runs(dealt, closed, name)
    assert_same_system_solves(dealt["est"], dealt["cut"], name, debug_option)


def test_batch_of_two_deals_equals_the_windows_alone(gpu_lib, debug_option):
    """two P = 10 windows of one batch group, the second PREPARED with SVIN_NO_TILE_DEAL on -- pack() reads the switch -- so that its
    slot carries the zero word next to the first window's deal"""
    from svin_amd import estimator
    debug_option(NO_SKYLINE, 0)
    debug_option(NO_DEAL, 0)
    seeds = [dict(seed=5), dict(seed=6, pose_noise=(0.2, 0.05))]
    alone = []
    for kw in seeds:
        est, fids, lids = build(10, **kw)
        est.optimize(6)
        alone.append((states_of(est, fids, lids), {k: est.summary()[k] for k in SUMMARY}))
    batch = []
    for k, kw in enumerate(seeds):
        debug_option(NO_DEAL, k)
        est, fids, lids = build(10, **kw)
        est.prepare()
        batch.append((est, fids, lids))
    debug_option(NO_DEAL, 0)
    words = [b[0].debug_tile_deal() for b in batch]
    assert words == [(2 << 8) | (1 << 12), 0], words
    assert estimator.solve_prepared_batch([b[0] for b in batch], 6) == 2
    assert [b[0].debug_tile_deal() for b in batch] == words   # (the batched solve packs nothing anew: each slot carried its own word)
    for k, (est, fids, lids) in enumerate(batch):
        est.finish()
        for what, x, y in zip(("poses", "speed / bias", "landmarks"), states_of(est, fids, lids), alone[k][0]):
            assert np.array_equal(x, y), "window %d: %s differ by %.3e" % (k, what, float(np.max(np.abs(x - y))))
        assert {s: est.summary()[s] for s in SUMMARY} == alone[k][1], k


def test_non_positive_pivot_reports_alike_on_both_deals(gpu_lib, debug_option):
    import dense_solve_reference as dr
    from svin_amd.estimator import Estimator
    debug_option(NO_SKYLINE, 0)
    debug_option(NO_DEAL, 0)
    est, _, _ = build(10)
    est.debug_reduced_solve(1e-4, fused=False)
    S, g = est.debug_last_system()
    cut = est.debug_tile_skyline()[0]
    assert est.debug_tile_deal() == (2 << 8) | (1 << 12)
    d = len(g)
    S = np.tril(S) + np.tril(S, -1).T
    buf = np.zeros((160, 160))
    buf[:d, :d] = dr.make_indefinite(S, 100)
    dealt = Estimator.debug_solve_dense(buf, g, d, padded=True, ldS=160, tile_cut=cut)
    debug_option(NO_DEAL, 1)
    closed = Estimator.debug_solve_dense(buf, g, d, padded=True, ldS=160, tile_cut=cut)
    print("pivot of row 100 non-positive: cholFail %d (planned deal) %d (closed form)" % (dealt["cholFail"], closed["cholFail"]))
    assert dealt["route"] == closed["route"] == 0
    assert dealt["cholFail"] == closed["cholFail"] and (dealt["cholFail"] & 2) and (dealt["cholFail"] & 12) == 0
