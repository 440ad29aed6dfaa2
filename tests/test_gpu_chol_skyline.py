"""k_chol_solve_lds<0> factoring inside the window's tile skyline (pack_plan.hpp planTileSkyline; DESIGN.md: "the reduced system
inside its tile skyline") against the same kernel on the dense profile (SVIN_NO_TILE_SKYLINE).  A product with a tile of exact
zeros changes no finite result, so every comparison is for equal values element by element (+0 == -0).

Every window is built twice.  One handle runs with the skyline and SVIN_CHECK_TILE_SKYLINE -- before each launch of the solver the
library copies S to the host and throws if a tile below the profile the BUILD may write (before the fill) holds anything but zeros
-- the other with SVIN_NO_TILE_SKYLINE.  Compared: one trust-region iteration at mu = 1e-4, at the ladder's start (1e-8) and at
its first retry (1e-7) -- y_C, v_C, the whole scalar record with cholFail -- then optimize(3) and seven more iterations: states,
landmarks, summary.  The window with variable extrinsics builds S with floating-point atomics in an order that changes from run to
run (include/svin_ba.h, svin_ba_debug_last_system), so two handles differ in their last bits whatever the solver does: it takes
part in everything below but not in the handle-to-handle comparison.
Every window then has the very system it solved (svin_ba_debug_last_system behind the unfused svin_ba_debug_reduced_solve, at
the three mu) solved twice through svin_ba_debug_solve_dense / _profiled -- dense and inside the reported skyline: y and cholFail
must be equal.  The profile the library reports (SVIN_LAST_TILE_SKYLINE_LO / _HI) is held against the numpy reference of
tests/helpers/tile_skyline_lib.py, built from the block lists of the handle's own graph (residuals_of / parameters_of over the
blocks of linearize()): never below it, equal to it on the windows without a prior, and 0 -- dense -- on the switched-off handle.
A bounded wait that gave up (cholFail bits 4 | 8) makes optimize() throw and is asserted absent in every scalar record.

Windows: P = 5 (dense), 6 (the first skipped tile), 10 (the bench's profile), 11 (eleven tile rows); a constant first pose; a
constant speed / bias block; the window right after its first marginalisation and after three of them; per-frame extrinsics of two
cameras (d = 162); a pose on the Pose4d manifold (k_lock_rows).  Then a batch of two P = 10 windows with different profiles
against the same windows alone.

A factorisation that fails: the P = 10 window's own system with one diagonal entry lowered (make_indefinite of
tests/helpers/dense_solve_reference.py, as tests/test_gpu_dense_solve.py uses it: exactly one negative pivot) through the direct
solve on both profiles -- the same cholFail, bit 2 set, bits 4 | 8 clear; and the window itself on two handles: a trust-region step
at mu = -0.5 (S - D / 2 is indefinite) fails, the retry at 1e-7 and optimize(10) behind it must give the same failMax / cholFail
sequence, step and end state.  Nothing is asked of y_C of the failed step: the skipped tiles stay zero where the dense profile
spreads non-finite values."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import tile_skyline_lib as ts  # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402

pytestmark = pytest.mark.gpu
NO, CHECK = "SVIN_NO_TILE_SKYLINE", "SVIN_CHECK_TILE_SKYLINE"
SUMMARY = ("initial_cost", "final_cost", "iterations", "successful", "termination")
MUS = (1e-4, 1e-8, 1e-7)


def blocks_of(est, kind):
    ids = [b for b in est.parameter_block_ids() if est.parameter_block(b)["type"] == kind]
    return sorted(ids)


def plain(P, seed=5, rig="euroc", **kw):
    def build():
        from svin_amd.estimator import Estimator
        spec = syn.make_window(P=P, L=48, n_obs=400, seed=seed, rig=rig, **kw)
        est = Estimator(0)
        fids, lids = syn.feed(est, spec)
        return est, fids, lids
    return build


def with_constant(P, kind, index):
    def build():
        est, fids, lids = plain(P)()
        assert est.set_parameter_block_constant(blocks_of(est, kind)[index])
        return est, fids, lids
    return build


def with_manifold(P, index):
    def build():
        est, fids, lids = plain(P)()
        assert est.reset_parameterization(blocks_of(est, 0)[index], est.POSE4D)
        return est, fids, lids
    return build


def slid(P, n_marg):
    """fed frame by frame; the last n_marg frames are each followed by optimize + marginalisation, so that the window carries a
    prior that went through n_marg marginalisations"""
    def build():
        from svin_amd.estimator import Estimator
        spec = syn.make_window(P=P, L=64, n_obs=640, seed=9, keyframe_every=2, frame_dt=0.3)
        est = Estimator(0)

        def on_frame(k, fid):
            if k >= spec.P - n_marg:
                est.optimize(4)
                est.apply_marginalization(3, 2)
        fids, lids = syn.feed(est, spec, on_frame=on_frame)
        est.wait_idle()
        assert est.marg() is not None
        return est, est.frame_ids(), [l for l in lids if l in est.get_landmarks()]
    return build


# name -> (builder, the reported profile must EQUAL the reference, two builds of the window give the same bits)
WINDOWS = {
    "P5": (plain(5), True, True), "P6": (plain(6), True, True), "P10": (plain(10), True, True), "P11": (plain(11), True, True),
    "constant_first_pose": (with_constant(10, 0, 0), True, True),
    "constant_speed_bias": (with_constant(10, 2, 4), True, True),
    "first_marginalisation": (slid(8, 1), False, True),
    "three_marginalisations": (slid(9, 3), False, True),
    "extrinsics_per_frame": (plain(6, rig="test4"), False, False),
    "pose4d_locked_rows": (with_manifold(10, 3), True, True),
}


def states_of(est, fids, lids):
    T = np.stack([est.get_T_WS(f) for f in fids])
    sb = np.stack([v if v is not None else np.full(9, np.nan) for v in (est.get_speed_and_bias(f) for f in fids)])   # (old keyframes keep their pose only)
    lms = est.get_landmarks()
    lm = np.stack([np.r_[lms[l]["point"], lms[l]["quality"]] for l in lids])
    return T, sb, lm


def reported(nT):
    from svin_amd.estimator import Estimator
    word = Estimator.debug_get_option("SVIN_LAST_TILE_SKYLINE_LO") | (Estimator.debug_get_option("SVIN_LAST_TILE_SKYLINE_HI") << 28)
    return word, ts.unpack(word, nT)


def graph_reference(est):
    """(d, nT, pre, hi) of the numpy reference from the handle's own graph"""
    lin = est.linearize(1e-4)
    off = {int(b): int(o) for b, o in zip(lin["block_ids"], lin["block_off"])}
    dim = {b: (9 if est.parameter_block(b)["type"] == 2 else 6) for b in off}
    d = lin["d"]
    dC = min([off[b] for b in off if dim[b] == 9] + [d])
    rids = sorted({r for b in off for r in est.residuals_of(b)})
    cliques = []
    for r in rids:
        blocks, _ = est.parameters_of(r)
        cl = [(off[b], dim[b]) for b in blocks if b in off]
        if cl and max(o + n for o, n in cl) > dC:   # (what lies inside the camera part is dense anyway)
            cliques.append(cl)
    pre, hi = ts.reference(d, dC, cliques)
    return d, (d + 15) // 16, pre, hi


def run(build, skyline, debug_option):
    debug_option(NO, 0 if skyline else 1)
    debug_option(CHECK, 1 if skyline else 0)
    est, fids, lids = build()
    out = dict(steps=[])
    for mu in MUS:
        r = est.debug_trust_region_step(mu, 1e4, 0)
        assert (r["scalars"]["cholFail"] & 12) == 0 and r["scalars"]["failMax"] < 4
        out["steps"].append(r)
    out["word"] = reported(11)[0]
    est.optimize(3)
    out["after3"] = (states_of(est, fids, lids), {k: est.summary()[k] for k in SUMMARY})
    est.optimize(7)
    out["after10"] = (states_of(est, fids, lids), {k: est.summary()[k] for k in SUMMARY})
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
            assert np.array_equal(x, y, equal_nan=True), "%s, %s: %s differ by %.3e" % (name, stage, what, float(np.nanmax(np.abs(x - y))))


def assert_same_system_solves(est, word, name):
    """the system the handle has just solved, through the direct solve on both profiles"""
    from svin_amd.estimator import Estimator
    for mu in MUS:
        est.debug_reduced_solve(mu, fused=False)
        S, g = est.debug_last_system()
        d = len(g)
        dpad = (d + 15) // 16 * 16
        buf = np.zeros((dpad, dpad))
        buf[:d, :d] = S
        dense = Estimator.debug_solve_dense(buf, g, d, padded=True, ldS=dpad)
        sky = Estimator.debug_solve_dense(buf, g, d, padded=True, ldS=dpad, tile_cut=word)
        assert dense["route"] == sky["route"] == 0, (name, dense["route"])   # kRouteLdsWhole
        assert dense["cholFail"] == sky["cholFail"] and (sky["cholFail"] & 12) == 0, (name, mu, dense["cholFail"], sky["cholFail"])
        assert np.array_equal(dense["y"], sky["y"]), "%s, mu %g: y of one system differs by %.3e between the profiles" % (
            name, mu, float(np.max(np.abs(dense["y"] - sky["y"]))))


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_window_inside_its_skyline_equals_the_dense_profile(gpu_lib, debug_option, name):
    build, exact, reproducible = WINDOWS[name]
    sky = run(build, True, debug_option)
    dense = run(build, False, debug_option)
    assert dense["word"] == 0, "SVIN_NO_TILE_SKYLINE left a profile"
    if reproducible:
        assert_equal_runs(sky, dense, name)
    debug_option(NO, 0)
    debug_option(CHECK, 1)
    assert_same_system_solves(sky["est"], sky["word"], name)
    d, nT, pre, hi = graph_reference(sky["est"])
    got = ts.unpack(sky["word"], nT)
    print("%s: d %d, %d tile rows, reported %s, reference %s (before the fill %s)" % (name, d, nT, got, hi, pre))
    assert d <= 176
    assert all(g >= h for g, h in zip(got, hi)), (name, got, hi)
    if exact:
        assert got == hi, (name, got, hi)
    if name == "P10":
        assert got == [5, 7, 8, 9, 9, 9, 9, 9, 9, 9]
    if name == "P6":
        assert got == [4, 5, 5, 5, 5, 5]
    if name == "P5":
        assert sky["word"] == 0


def test_batch_of_two_profiles_equals_the_windows_alone(gpu_lib, debug_option):
    """two P = 10 windows of one batch group with different profiles.  A window that differs in structure (P = 6; a constant block)
    differs in d and falls into another group, so the second window is PREPARED with SVIN_NO_TILE_SKYLINE on -- pack() reads the
    switch -- and carries the dense profile in its slot next to the first window's 5, 7, 8, 9, ..."""
    from svin_amd import estimator
    debug_option(NO, 0)
    debug_option(CHECK, 0)
    builders = [plain(10, seed=5), plain(10, seed=6, pose_noise=(0.2, 0.05))]
    alone = []
    for b in builders:
        est, fids, lids = b()
        est.optimize(6)
        alone.append((states_of(est, fids, lids), {k: est.summary()[k] for k in SUMMARY}))
    # the same two windows, the second on the dense profile (packed with the switch on), in ONE batch
    batch = []
    for k, b in enumerate(builders):
        debug_option(NO, k)
        est, fids, lids = b()
        est.prepare()
        batch.append((est, fids, lids))
    debug_option(NO, 0)
    words = [b[0].debug_tile_skyline()[0] for b in batch]
    assert ts.unpack(words[0], 10) == [5, 7, 8, 9, 9, 9, 9, 9, 9, 9] and words[1] == 0, words
    assert estimator.solve_prepared_batch([b[0] for b in batch], 6) == 2
    # the batched solve packs nothing anew: each slot carried the profile its window was prepared with.  (That the kernel reads
    # its OWN slot's word is not something results can show -- either profile is valid for either window: DESIGN.md section 26.)
    assert [b[0].debug_tile_skyline()[0] for b in batch] == words
    for k, (est, fids, lids) in enumerate(batch):
        est.finish()
        for what, x, y in zip(("poses", "speed / bias", "landmarks"), states_of(est, fids, lids), alone[k][0]):
            assert np.array_equal(x, y), "window %d: %s differ by %.3e" % (k, what, float(np.max(np.abs(x - y))))
        assert {s: est.summary()[s] for s in SUMMARY} == alone[k][1], k


def test_failing_factorisation_reports_and_recovers_alike(gpu_lib, debug_option):
    import dense_solve_reference as dr
    from svin_amd.estimator import Estimator
    # (a) one system, both profiles: a single negative pivot in the camera part, in the chain below a skipped tile, in the last row
    debug_option(NO, 0)
    debug_option(CHECK, 1)
    est, fids, lids = plain(10)()
    est.debug_reduced_solve(1e-4, fused=False)
    S, g = est.debug_last_system()
    word = est.debug_tile_skyline()[0]
    assert ts.unpack(word, 10) == [5, 7, 8, 9, 9, 9, 9, 9, 9, 9]
    d = len(g)
    S = np.tril(S) + np.tril(S, -1).T
    for row in (3, 100, 149):
        buf = np.zeros((160, 160))
        buf[:d, :d] = dr.make_indefinite(S, row)
        dense = Estimator.debug_solve_dense(buf, g, d, padded=True, ldS=160)
        sky = Estimator.debug_solve_dense(buf, g, d, padded=True, ldS=160, tile_cut=word)
        print("pivot of row %d negative: cholFail %d (dense) %d (skyline)" % (row, dense["cholFail"], sky["cholFail"]))
        assert dense["route"] == sky["route"] == 0
        assert dense["cholFail"] == sky["cholFail"] and (sky["cholFail"] & 2) and (sky["cholFail"] & 12) == 0 and (sky["cholFail"] & ~15) == 0, row

    # (b) the window: a step that fails, the retry, the solve behind it
    def history(skyline):
        debug_option(NO, 0 if skyline else 1)
        debug_option(CHECK, 1 if skyline else 0)
        est, fids, lids = plain(10)()
        failed = est.debug_trust_region_step(-0.5, 1e4, 0)
        retry = est.debug_trust_region_step(1e-7, 1e4, 0)
        seq = [(r["scalars"]["failMax"], r["scalars"]["cholFail"]) for r in (failed, retry)]
        est.optimize(10)
        return seq, retry, states_of(est, fids, lids), {k: est.summary()[k] for k in SUMMARY}

    a, b = history(True), history(False)
    print("failMax / cholFail of the failing step and of the retry: %s (skyline) %s (dense)" % (a[0], b[0]))
    assert a[0] == b[0], (a[0], b[0])
    # (failMax carries the cholFail bits of the step; the device's cholFail itself is cleared again by the time the record is read)
    assert 0 < a[0][0][0] < 4 and (a[0][0][1] & 12) == 0, a[0]   # bits 1 | 2: numerical; 4 | 8 clear: no wait gave up
    assert a[0][1][0] == 0 and a[0][1][1] == 0, a[0]             # the retry factorises
    for key in ("y_C", "v_C", "y_L", "v_L"):
        assert np.array_equal(a[1][key], b[1][key]), key
    for key, v in a[1]["scalars"].items():
        assert np.array_equal(np.asarray(v), np.asarray(b[1]["scalars"][key])), key
    assert a[3] == b[3], (a[3], b[3])
    for what, x, y in zip(("poses", "speed / bias", "landmarks"), a[2], b[2]):
        assert np.array_equal(x, y), "%s differ by %.3e" % (what, float(np.max(np.abs(x - y))))
