"""The factor blocks of the build (k_schur_dense) copy a factor's Jacobian and residual to LDS with one round of loads and form
J^T J and J^T r from the copy: the same products in the same order, so the reduced system is the one it was.  Checked on the windows
the long-track work on the build and the post-solve pass was planned for (that work itself was measured to gain nothing and is not in
the tree), which are also the smallest at which the build's landmark part, its slab sum and its factor blocks
take each of their paths:

  (d) S, g and one trust-region iteration in the form optimize() runs stay inside the a-priori bounds of schur_reference /
      step_reference at mu = 1e-4,
  (e) two consecutive linearize calls agree bit for bit (slab-count windows, whose IMU factors go into the same S as the slabs),
  and optimize(3) twice from the same state ends on the same bits (fixed extrinsics)

on tracks of 1, 2, 15 .. 18, 31 .. 34 observations (a lane short, every lane once, one or two lanes twice, every lane twice, one or
two lanes a third time); a 33-track in lane group 15 of a full chunk and alone in a last chunk; a constant pose under a lane's second
observation but not its first, and the reverse; a constant landmark with a track of 17; variable extrinsics with a track of 17;
1, 2, 15, 16, 17, 64 and 256 slabs (three observations per landmark).
Positions and track lengths are asserted on the device's own CSR (debug_csr), because pack() may re-sort."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obs_patterns as op          # noqa: E402
import schur_reference as sr       # noqa: E402
import step_reference as st        # noqa: E402
from test_gpu_schur_edges import DIM, KIND, gpu_records   # noqa: E402
from test_gpu_step_edges import state_of                  # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402

pytestmark = pytest.mark.gpu

MU = 1e-4
LENGTHS = (1, 2, 15, 16, 17, 18, 31, 32, 33, 34)
# the same lengths with the 33-track moved: to landmark 15 (lane group 15 of the first, full chunk) / to landmark 16 (alone in the last chunk)
LENGTHS_GROUP15 = (1, 2, 15, 16, 17, 18, 31, 32, 34, 3, 4, 5, 6, 3, 4, 33)
LENGTHS_ALONE = (1, 2, 15, 16, 17, 18, 31, 32, 34, 3, 4, 5, 6, 3, 4, 5, 33)
# observation i of a track is (frame i // 2, camera i % 2): lanes 4, 5 have frame 2 first and frame 10 second, lanes 6, 7 frame 3 first and frame 11 second
FIXED_FRAMES = (2, 11)


def ext_window():
    """per-frame variable extrinsics (rig test4), tracks of 17 and 18 among short ones"""
    P, lengths = 9, (17, 18, 3, 4, 5, 6, 3, 4, 5)
    spec = op.full_window(P, len(lengths), "test4", 1)
    every = sorted((f, c) for f in range(P) for c in (0, 1))
    tracks = {l: every[:n] if n > 6 else every[(5 * l) % (2 * P - 6):][:n] for l, n in enumerate(lengths)}
    op.keep_tracks(spec, tracks)
    assert set(spec.obs_frame.tolist()) == set(range(P))
    return op.Design(spec=spec, tracks=tracks)


# name -> (design, fixed frames, index of a landmark to hold constant, variable extrinsics, checks on the device CSR)
WINDOWS = {
    "lengths": (lambda: op.design_track_lengths(P=17, lengths=LENGTHS), (), None, False, dict(tracks=LENGTHS)),
    "group15": (lambda: op.design_track_lengths(P=17, lengths=LENGTHS_GROUP15, n_more=3), (), None, False, dict(at={15: 33}, L=19)),
    "alone": (lambda: op.design_track_lengths(P=17, lengths=LENGTHS_ALONE, n_more=0), (), None, False, dict(at={16: 33}, L=17)),
    "fixed_poses": (lambda: op.design_track_lengths(P=17, lengths=LENGTHS), FIXED_FRAMES, None, False, dict(tracks=LENGTHS, slots=True)),
    "const_landmark": (lambda: op.design_track_lengths(P=17, lengths=LENGTHS), (), 4, False, dict(tracks=LENGTHS, const=17)),
    "ext": (ext_window, (), None, True, dict(tracks=(17, 18))),
}
SLAB_L = (16, 32, 240, 256, 272, 1024, 4096)   # 1, 2, 15, 16, 17, 64, 256 slabs of sixteen landmarks


def make(design, fixed_frames=(), const_lm=None):
    from svin_amd.estimator import Estimator
    est = Estimator(0)
    fids, lids = syn.feed(est, design.spec)
    if fixed_frames:
        ev = est.eval_reprojection()
        pose_of = {est.describe_block(int(b))[0]: int(b) for b in np.unique(ev["pose_id"])}
        for f in fixed_frames:
            assert est.set_parameter_block_constant(pose_of[fids[f]])
    if const_lm is not None:
        assert est.set_parameter_block_constant(int(lids[const_lm]))
    return est


def check_csr(est, expect, fixed_frames):
    csr = est.debug_csr()
    n = np.diff(csr["lm_ptr"])
    if "L" in expect:
        assert csr["L"] == expect["L"]
    for l, k in expect.get("at", {}).items():
        assert n[l] == k, "device landmark %d has %d observations, %d wanted" % (l, n[l], k)
        if l % 16 == 15:
            assert l < csr["L"] - 1, "lane group 15 of a FULL chunk"
        else:
            assert l % 16 == 0 and l == csr["L"] - 1, "alone in the last chunk: device L = 16 k + 1"
    if "tracks" in expect:
        assert set(expect["tracks"]) <= set(n.tolist()), "track lengths on the device: %s" % sorted(set(n.tolist()))
    if expect.get("slots"):
        # the pose slots of the longest track run in frame order, so slot = frame
        l = int(np.argmax(n))
        slots = (csr["obs_idx"][csr["lm_ptr"][l]:csr["lm_ptr"][l + 1]] & 0xfff).astype(int)
        assert slots.tolist() == [i // 2 for i in range(n[l])]
        a, b = fixed_frames
        first, second = slots[:16], slots[16:32]
        assert any(first[g] == a and second[g] not in fixed_frames for g in range(16)), "no lane with only its first observation on a constant pose"
        assert any(second[g] == b and first[g] not in fixed_frames for g in range(16)), "no lane with only its second observation on a constant pose"
    if "const" in expect:
        neg = csr["w"] < 0
        assert neg.sum() == expect["const"] and len(set(csr["obs_lm"][neg].tolist())) == 1, "one constant landmark with a track of %d" % expect["const"]
    return csr


def solved_state(est):
    s = est.summary()
    blocks = [est.get_parameter_block(b) for b in est.parameter_block_ids()]
    lms = est.get_landmarks()
    return ([s[k] for k in ("initial_cost", "final_cost", "iterations", "successful", "termination")], blocks,
            np.array([lms[i]["point"] for i in sorted(lms)]))


def check_solve_repeats(make_est):
    """optimize(3) twice from the same state: the builds behind the first run with a loaded landmark scaling"""
    solved = []
    for _ in range(2):
        e = make_est()
        e.optimize(3)
        solved.append(solved_state(e))
    assert solved[0][0] == solved[1][0], "summaries differ: %s / %s" % (solved[0][0], solved[1][0])
    assert solved[0][0][2] >= 2, "optimize(3) stopped before a build with a loaded landmark scaling"
    assert all(np.array_equal(x, y) for x, y in zip(solved[0][1], solved[1][1])), "parameter blocks differ"
    assert np.array_equal(solved[0][2], solved[1][2]), "landmarks differ"


def check_bounds(name, est):
    """(d): the reduced system and one trust-region iteration against the long-double references"""
    recs, describe = gpu_records(est)
    lin = est.linearize(MU)
    kinds = [describe(int(b))[1] for b in lin["block_ids"]]
    blocks = [((KIND[k], int(b)), int(o), DIM[k]) for b, o, k in zip(lin["block_ids"], lin["block_off"], kinds)]
    rf = sr.assemble(recs, blocks, MU)
    assert rf["d"] == lin["d"]
    rS, rg = sr.worst_ratio(lin["S"], lin["g"], rf)
    print("%s: worst error / tol  S %.3g  g %.3g" % (name, rS, rg))
    assert rS <= 1.0 and rg <= 1.0, "the reduced system leaves its rounding bound"
    res = est.debug_trust_region_step(MU, 1e4, 0)
    res["radius"] = 1e4
    P = st.prepare(recs, blocks, lm_order=res["lm_ids"])
    x_blocks, lm_x = state_of(est, res)
    worst, _, _ = st.judge(P, MU, res, x_blocks, lm_x, None, {})
    print("%s: step, worst error / tol  %s" % (name, "  ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    assert res["scalars"]["failMax"] == 0 and res["scalars"]["cholFail"] == 0
    bad = {n: w for n, w in worst.items() if not w <= 1.0}
    assert not bad, "%s: outside the rounding bound: %s" % (name, bad)
    return lin


@pytest.mark.parametrize("name", list(WINDOWS))
def test_long_tracks(gpu_lib, name):
    if not sr.have_long_double():
        pytest.skip("np.longdouble is not wider than float64 on this machine")
    build, fixed_frames, const_lm, with_ext, expect = WINDOWS[name]
    design = build()
    make_est = lambda: make(design, fixed_frames, const_lm)   # noqa: E731
    est = make_est()
    check_csr(est, expect, fixed_frames)
    check_bounds(name, est)
    if not with_ext:
        check_solve_repeats(make_est)


@pytest.mark.parametrize("L", SLAB_L)
def test_slab_counts(gpu_lib, L):
    if not sr.have_long_double():
        pytest.skip("np.longdouble is not wider than float64 on this machine")
    design = op.design_three_observations(L)
    make_est = lambda: make(design)   # noqa: E731
    est = make_est()
    csr = est.debug_csr()
    assert csr["L"] == L and np.all(np.diff(csr["lm_ptr"]) == 3)
    lin = check_bounds("three_observations_L%d" % L, est)
    again = est.linearize(MU)
    assert np.array_equal(lin["S"], again["S"]) and np.array_equal(lin["g"], again["g"]), "(e) two builds of the same point differ"
    assert len(est.eval_factors()) > 0, "no small factor goes into S"
    check_solve_repeats(make_est)
