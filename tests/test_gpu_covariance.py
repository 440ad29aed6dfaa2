"""Marginal covariances on the GPU (svin_ba_get_covariance / _blocks; kernels in svin_amd/csrc/cov.hip) against high-precision
inverses of J^T J (tests/helpers/covariance_reference.py).

Sigma = (J^T J)^-1, J as the trust-region build sees it.  Error metric e(X) = max_ij |X_ij - ref_ij| / sqrt(ref_ii ref_jj).
Bar of every comparison: 8 x max(e(np.linalg.inv), e(block_replay)), both float64 on the same matrix against the same reference and
computed inside the test (the attainable error is cond x eps of each matrix, so no fixed tolerance exists); every test prints
the yardsticks and the device's e."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import covariance_reference as cr   # noqa: E402
import prior_reference as pr        # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402
from test_gpu_parity import drop_underdetermined_landmarks, log, snapshot_states   # noqa: E402

pytestmark = pytest.mark.gpu
LD = np.longdouble


def new_estimator():
    from svin_amd.estimator import Estimator
    return Estimator(0)


def small_window(rig, L=12, seed=5):
    kw = dict(sonar=True, depth=True, sonar_patch=(1, 2)) if rig == "rig_v2" else {}
    return drop_underdetermined_landmarks(syn.make_window(P=3, L=L, n_obs=None, seed=seed, rig=rig, **kw))


def stereo_pairs_only(spec):
    """keeps the observations that have their stereo partner in the same frame: whatever part of a landmark's track a sliding window
    holds, it is at least one stereo pair, so every landmark block stays positive definite without damping"""
    key = spec.obs_lm * spec.P + spec.obs_frame
    both = np.intersect1d(key[spec.obs_cam == 0], key[spec.obs_cam == 1])
    keep = np.isin(key, both)
    for name in ("obs_lm", "obs_frame", "obs_cam", "obs_uv", "obs_size"):
        setattr(spec, name, getattr(spec, name)[keep])
    return spec


def device_sigma(est, asm):
    """all of Sigma from one call, laid out as the assembled normal matrix"""
    ids = [(b, c, m) for b, c, m in asm["blocks"]] + [(l, asm["lm_col"][l], 3) for l in asm["lm_ids"]]
    n = asm["N"].shape[0]
    X = np.full((n, n), np.nan)
    pairs = [(a[0], b[0]) for a in ids for b in ids]
    out = est.get_covariance_blocks(pairs)
    k = 0
    for a in ids:
        for b in ids:
            assert out[k].shape == (a[2], b[2])
            X[a[1]:a[1] + a[2], b[1]:b[1] + b[2]] = out[k]
            k += 1
    assert not np.isnan(X).any()
    return X


def check_dense(est, tag):
    """the device's whole Sigma against mp_inverse of the dense J^T J assembled from eval_reprojection / eval_factors / the prior"""
    asm = cr.dense_normal_matrix(est, pr.moved)
    # (mpmath inverts n = 81 in 2.7 s and n = 150 in 19 s: beyond ~100 the block formulas with every inverse in mpmath)
    ref = cr.mp_inverse(asm["N"]) if asm["N"].shape[0] <= 100 else cr.mp_block_reference(asm["N"], asm["d"])
    bar, e_inv, e_blk = cr.bar(asm["N"], asm["d"], ref)
    n0 = est.covariance_pass_count()
    X = device_sigma(est, asm)
    assert est.covariance_pass_count() == n0 + 1
    e = cr.err(X, ref)
    d = asm["d"]
    sd = np.sqrt(np.diag(ref))
    parts = dict(cc=cr.err_block(X[:d, :d], ref, np.arange(d), np.arange(d), sd))
    if X.shape[0] > d:
        lm = np.arange(d, X.shape[0])
        parts["lc"] = cr.err_block(X[d:, :d], ref, lm, np.arange(d), sd)
        parts["ll"] = cr.err_block(X[d:, d:], ref, lm, lm, sd)
    log("%s: n %d d %d  e(np.linalg.inv) %.2e  e(block_replay) %.2e  bar %.2e  device e %.2e (ratio to the larger yardstick %.2f)  %s" %
        (tag, X.shape[0], d, e_inv, e_blk, bar, e, e / max(e_inv, e_blk), {k: "%.2e" % v for k, v in parts.items()}))
    assert np.array_equal(X, X.T), tag   # Sigma[b, a] == Sigma[a, b]^T bit for bit
    assert e <= bar, (tag, e, bar)
    return asm, X, ref


# ------------------------------------------------------------------------------------------ 1. dense definition, every block kind
@pytest.mark.parametrize("rig", ["euroc", "rig_v2"])
def test_dense_definition_every_block_kind(gpu_lib, rig):
    """P = 3, L = 12: camera blocks, every landmark's 3 x 3, landmark-pose and landmark-landmark cross blocks, at the initial states
    and after optimize(5) (rig_v2: sonar, depth, per-frame extrinsics with their relative-pose factors)"""
    est = new_estimator()
    syn.feed(est, small_window(rig))
    asm, X0, _ = check_dense(est, "%s initial" % rig)
    kinds = {est.describe_block(b)[1] for b, _, _ in asm["blocks"]}
    assert kinds == ({0, 1, 2} if rig == "rig_v2" else {0, 2}) and len(asm["lm_ids"]) >= 5
    est.optimize(5)
    _, X1, _ = check_dense(est, "%s after optimize(5)" % rig)
    assert not np.array_equal(X0, X1)


# ------------------------------------------------------------------------------------------ 2. inversion at the real sizes
def check_reduced(est, tag, want_d=None):
    lin = est.linearize(0.0)
    if want_d is not None:
        assert lin["d"] == want_d, (tag, lin["d"])
    S = np.tril(lin["S"]) + np.tril(lin["S"], -1).T   # as the solvers read it: lower triangle, mirrored
    ref = cr.refined_inverse(S)
    e_inv = cr.err(np.linalg.inv(S), ref)
    bar = cr.BAR_FACTOR * e_inv   # (no landmark part in S: block_replay of it IS np.linalg.inv)
    blocks = [(int(b), int(o)) for b, o in zip(lin["block_ids"], lin["block_off"])]
    dim = {b: (9 if est.describe_block(b)[1] == 2 else 6) for b, _ in blocks}
    out = est.get_covariance_blocks([(a, b) for a, _ in blocks for b, _ in blocks])
    X = np.zeros_like(S)
    k = 0
    for a, oa in blocks:
        for b, ob in blocks:
            X[oa:oa + dim[a], ob:ob + dim[b]] = out[k]
            k += 1
    e = cr.err(X, ref)
    log("%s: d %d  cond(scaled S) %.1e  e(np.linalg.inv) %.2e  bar %.2e  device e %.2e (ratio %.2f)" %
        (tag, lin["d"], np.linalg.cond(S / np.sqrt(np.outer(np.diag(S), np.diag(S)))), e_inv, bar, e, e / e_inv))
    assert np.array_equal(X, X.T)
    assert e <= bar, (tag, e, bar)
    return X, ref


@pytest.mark.parametrize("P,L,rig,d,hold", [(10, 300, "euroc", 150, 0), (8, 300, "rig_v2", 198, 1), (10, 300, "rig_v2", 258, 0),
                                           (18, 300, "euroc", 270, 0)])
def test_inversion_at_the_real_sizes(gpu_lib, P, L, rig, d, hold):
    """Sigma_cc against refined_inverse of the S svin_ba_linearize(h, 0) returns on the same handle and state: d = 150 (config #2's
    frame count); d = 198, the size of the stereo_rig_v2 sliding window, on a well-posed window of that rig (eight frames with
    per-frame extrinsics are 204 unknowns -- the generator holds the first frame's extrinsics constant -- and one more extrinsics
    block held constant leaves 198); config #3's shape (ten frames: 258 of the 270 unknowns for the same reason) and d = 270, the
    last tile row before the cap"""
    est = new_estimator()
    syn.feed(est, drop_underdetermined_landmarks(syn.make_window(P=P, L=L, n_obs=10 * L, seed=9, rig=rig)))
    if hold:
        lin = est.linearize(0.0)
        ext = [int(b) for b in lin["block_ids"] if est.describe_block(int(b))[1] == 1]
        assert est.set_parameter_block_constant(ext[-1])
    check_reduced(est, "%s P = %d" % (rig, P), d)


def test_steady_state_rig_v2_sliding_window_reports_its_rank_deficiency(gpu_lib):
    """A limitation, pinned so that it is seen when it goes away.  The stereo_rig_v2 sliding window (5 keyframes + 3 IMU frames,
    d = 198) in its steady state, prior included, has a reduced system that is NOT positive definite without damping: two
    eigenvalues of the unit-diagonal S are 1e-16 .. 1e-15 (the third is 9e-6), and both null vectors lie wholly in the three
    ROTATION rows of the oldest pose the prior holds -- the frame whose speed / bias block and landmarks have been marginalised and
    which the prior alone constrains; the prior's pseudo-inverse carries no information on two of its rotation directions next to
    the 2e16 of the extrinsics it now also holds.  (The window is well posed until the extrinsics enter the prior: at d = 186 the
    smallest eigenvalue is 4e-8 and the call answers.)  There is no inverse to hold the device against, so the call must say
    SINGULAR, as LAPACK's Cholesky does, and leave the handle usable; a caller who wants a covariance there has to constrain the
    orientation of that pose.  The inversion at d = 198 itself is test_inversion_at_the_real_sizes'."""
    from svin_amd import estimator
    est = new_estimator()
    frames = 12
    spec = stereo_pairs_only(syn.make_window(P=frames, L=18 * frames, n_obs=None, seed=3, rig="rig_v2", frame_dt=0.25, sonar=True,
                                             depth=True, sonar_patch=(2, 4)))
    hit = []

    def on_frame(k, fid):
        est.optimize(3)
        lin = est.linearize(0.0)
        if not hit and lin["d"] == 198:
            S = np.tril(lin["S"]) + np.tril(lin["S"], -1).T
            sd = np.sqrt(np.diag(S))
            w, V = np.linalg.eigh(S / np.outer(sd, sd))
            oldest = int(est.marg()["blocks"][0]["id"])
            off = dict(zip((int(b) for b in lin["block_ids"]), (int(o) for o in lin["block_off"])))[oldest]
            share = [float(np.sum(V[off + 3:off + 6, k] ** 2)) for k in range(2)]
            log("rig_v2 sliding window, d 198: eigenvalues of the unit-diagonal S %s; share of the two null vectors in the rotation "
                "rows of pose %d: %s" % (w[:3], oldest, share))
            assert w[1] < 1e-12 * w[-1] < w[2] and min(share) > 0.99
            n0 = est.covariance_pass_count()
            with pytest.raises(estimator.SingularError) as ei:
                est.get_covariance(fid, fid)
            assert "reduced system" in str(ei.value) and est.covariance_pass_count() == n0
            hit.append(k)
        est.apply_marginalization(5, 3)
    syn.feed(est, spec, on_frame=on_frame)
    assert hit, "the window never reached d = 198"
    est.optimize(2)


def test_wider_than_the_cap_is_unsupported(gpu_lib):
    """P = 19 euroc gives d = 285 > 272"""
    from svin_amd import estimator
    est = new_estimator()
    fids, _ = syn.feed(est, syn.make_window(P=19, L=200, n_obs=2000, seed=2))
    cov = np.zeros(36)
    assert est.L.svin_ba_get_covariance(est.h, fids[1], fids[1], cov.ctypes.data_as(C.POINTER(C.c_double)), 36) == estimator.SVIN_ERR_UNSUPPORTED
    assert b"285" in est.L.svin_ba_last_error()
    assert est.covariance_pass_count() == 0
    est.optimize(2)   # the handle stays usable


# ------------------------------------------------------------------------------------------ 3. landmark pass edges
@pytest.mark.parametrize("L", [1, 17, 65])
def test_landmark_pass_edges(gpu_lib, L):
    """L = 1, 17, 65 over P = 3 (one group, two workgroups' worth, a last workgroup with one landmark): landmark 0 is seen from every
    frame by both cameras, landmark 1 (L > 1) by exactly one stereo pair, one landmark is constant (zeros, while its observations
    still tighten the poses), one pose is constant through the Map API"""
    rng = np.random.default_rng(L)
    spec = syn.make_window(P=3, L=max(L, 4) + 6, n_obs=None, seed=40 + L)
    # landmarks seen from every frame by both cameras first, then cut to L
    seen = np.zeros((spec.L, 3, 2), bool)
    seen[spec.obs_lm, spec.obs_frame, spec.obs_cam] = True
    full = [l for l in range(spec.L) if seen[l].all()]
    assert len(full) >= 2, "the seeded window has no landmark seen from everywhere"
    order = full[:2] + [l for l in range(spec.L) if l not in full[:2]]
    order = order[:L]
    remap = -np.ones(spec.L, np.int64)
    remap[order] = np.arange(len(order))
    keep = remap[spec.obs_lm] >= 0
    if L > 1:   # landmark 1: the stereo pair of frame 1 only
        keep &= ~((remap[spec.obs_lm] == 1) & (spec.obs_frame != 1))
    for name in ("obs_frame", "obs_cam", "obs_uv", "obs_size"):
        setattr(spec, name, getattr(spec, name)[keep])
    spec.obs_lm = remap[spec.obs_lm[keep]]
    spec.lm_init, spec.lm_true = spec.lm_init[order], spec.lm_true[order]
    cnt = np.bincount(spec.obs_lm, minlength=L)
    ok = cnt >= 2
    ok[0] = True
    keep = ok[spec.obs_lm]
    for name in ("obs_lm", "obs_frame", "obs_cam", "obs_uv", "obs_size"):
        setattr(spec, name, getattr(spec, name)[keep])
    est = new_estimator()
    fids, lids = syn.feed(est, spec)
    observed = [lids[l] for l in range(L) if ok[l] and cnt[l] > 0]
    if L > 1:
        assert len(est.landmark_observations(lids[1])) == 2
    # (a stereo pair alone leaves the depth weakly observed but not unobserved: V_l is positive definite)
    asm, X, ref = check_dense(est, "L = %d" % L)
    assert len(asm["lm_ids"]) == len(observed)
    if L < 17:
        return
    # one constant landmark: zeros, and its observations still tighten the poses
    const = observed[2]
    pose = fids[2]
    P_with_free = est.get_covariance(pose, pose)
    assert est.set_parameter_block_constant(const)
    asm2, X2, _ = check_dense(est, "L = %d, landmark %d constant" % (L, const))
    assert const not in asm2["lm_ids"]
    assert not np.any(est.get_covariance(const, const)) and not np.any(est.get_covariance(const, pose))
    assert not np.any(est.get_covariance(pose, const)) and not np.any(est.get_covariance(const, observed[0]))
    P_const = est.get_covariance(pose, pose)
    # without it altogether the poses are looser than with it held constant
    for (f, c, kp, rid) in est.landmark_observations(const):
        assert est.remove_observation(const, f, c, kp)
    P_without = est.get_covariance(pose, pose)
    assert np.all(np.diag(P_const) <= np.diag(P_with_free) * (1 + 1e-9)) and np.all(np.diag(P_const) <= np.diag(P_without) * (1 + 1e-9))
    assert np.any(np.diag(P_const) < np.diag(P_without) * (1 - 1e-6))
    # one pose constant through the Map API
    assert est.set_parameter_block_constant(fids[1])
    asm3, _, _ = check_dense(est, "L = %d, pose %d constant" % (L, fids[1]))
    assert fids[1] not in [b for b, _, _ in asm3["blocks"]]
    assert not np.any(est.get_covariance(fids[1], fids[1])) and not np.any(est.get_covariance(fids[1], observed[0]))
    assert est.get_covariance(fids[1], fids[2]).shape == (6, 6) and not np.any(est.get_covariance(fids[2], fids[1]))


# ------------------------------------------------------------------------------------------ 4. after marginalisation
def states_differ(a, b):
    sa, sq = snapshot_states(a), snapshot_states(b)
    worst = 0.0
    for key in sa:
        assert sa[key].keys() == sq[key].keys()
        for k in sa[key]:
            worst = max(worst, float(np.max(np.abs(np.asarray(sa[key][k], float) - np.asarray(sq[key][k], float)))))
    return worst


def test_sliding_window_with_marginalisation(gpu_lib):
    """8 frames, applyMarginalizationStrategy each frame.  Every frame: Sigma_cc against the reference of test 2; the newest pose's
    block, 20 landmarks' 3 x 3 and their cross blocks with the newest pose against the block formulas in long double on the dense
    J^T J of that frame (prior included: ld_block_reference), so a landmark answered from another landmark's slot of the resident
    table fails; one pass per frame however many blocks are asked, a getLhs in between adds none and keeps the result; the window
    stays resident; and the final states are bit-identical to a handle that never asked."""
    spec = stereo_pairs_only(syn.make_window(P=8, L=160, n_obs=None, seed=12, keyframe_every=2, frame_dt=0.3, lm_noise=0.02))
    asked, quiet = new_estimator(), new_estimator()
    passes, worst = [], [0.0]

    def on_frame(est, k, fid):
        est.optimize(3)
        if est is asked and k >= 1:
            asm = cr.dense_normal_matrix(est, pr.moved)
            ref = cr.ld_block_reference(asm["N"], asm["d"])
            bar, e_inv, e_blk = cr.bar(asm["N"], asm["d"], ref)
            sd = np.sqrt(np.diag(ref))
            n0, l0 = est.covariance_pass_count(), est.lhs_pass_count()
            X, _ = check_reduced(est, "frame %d" % k)
            lms = [l for l in asm["lm_ids"]][-20:]
            assert len(lms) >= 10
            pairs = [(fid, fid)] + [(l, l) for l in lms] + [(l, fid) for l in lms]
            blocks = est.get_covariance_blocks(pairs)
            est.get_lhs(fid)
            again = est.get_covariance_blocks(pairs)
            assert all(np.array_equal(a, b) for a, b in zip(blocks, again))
            assert est.covariance_pass_count() == n0 + 1 and est.lhs_pass_count() == l0 + 1
            col = {b: (c, m) for b, c, m in asm["blocks"]}
            col.update({l: (asm["lm_col"][l], 3) for l in lms})
            e = 0.0
            for (a, b), B in zip(pairs, blocks):
                ra, rb = np.arange(col[a][0], col[a][0] + col[a][1]), np.arange(col[b][0], col[b][0] + col[b][1])
                e = max(e, cr.err_block(B, ref, ra, rb, sd))
            off = col[fid][0]
            assert np.array_equal(blocks[0], X[off:off + 6, off:off + 6])
            worst[0] = max(worst[0], e / max(e_inv, e_blk))
            log("frame %d: n %d  prior %s  e(np.linalg.inv) %.2e  e(block_replay) %.2e  bar %.2e  newest pose, %d landmarks and their cross "
                "blocks: device e %.2e (ratio %.2f)" % (k, asm["N"].shape[0], est.marg() is not None, e_inv, e_blk, bar, len(lms), e,
                                                      e / max(e_inv, e_blk)))
            assert e <= bar, (k, e, bar)
            passes.append(est.covariance_pass_count())
        est.apply_marginalization(3, 2)
    syn.feed(asked, spec, on_frame=lambda k, fid: on_frame(asked, k, fid))
    syn.feed(quiet, spec, on_frame=lambda k, fid: on_frame(quiet, k, fid))
    assert passes == list(range(1, 8)) and asked.marg() is not None
    ca, cq = asked.path_counters(), quiet.path_counters()
    assert ca["host_pack_solves"] == 0 and ca["resident_solves"] == cq["resident_solves"] >= 8
    assert states_differ(asked, quiet) == 0.0


# ------------------------------------------------------------------------------------------ 5. 2x2 information, Huber loss, host residual
@pytest.mark.parametrize("case", ["information", "huber", "host_residual"])
def test_general_information_loss_and_host_residual(gpu_lib, case):
    from svin_amd import estimator
    est = new_estimator()
    fids, lids = syn.feed(est, small_window("euroc", seed=8))
    ev = est.eval_reprojection(robust=True)
    if case == "information":   # every third residual gets a full 2 x 2 information matrix
        for k, rid in enumerate(ev["res_id"][::3]):
            a = 0.3 + 0.1 * (k % 5)
            assert est.map_set_reprojection_information(int(rid), np.array([[1.0 + a, 0.4 * a], [0.4 * a, 0.5 + a]])) == 1
    elif case == "huber":       # a scale that puts part of the residuals on the linear branch
        s = np.sort(np.hypot(ev["r"][:, 0], ev["r"][:, 1]))
        for rid in ev["res_id"][::2]:
            assert est.map_set_residual_loss(int(rid), estimator.SVIN_LOSS_HUBER, float(s[len(s) // 2])) == 1
    else:                       # a PoseError on the newest pose as a host cost function
        meas = est.get_T_WS(fids[2]) + np.r_[0.01, -0.02, 0.01, 0, 0, 0, 0]
        info6 = np.diag([50.0, 60, 70, 200, 300, 400]) + 5.0

        def pose_cost(ps):
            r, Jm, _ = estimator.host_pose_error(meas, info6, ps[0])
            return r, [Jm]
        assert est.map_add_host_residual([fids[2]], [7], 6, pose_cost) != 0
    base = new_estimator()
    syn.feed(base, small_window("euroc", seed=8))
    _, X, _ = check_dense(est, case)
    assert not np.array_equal(est.get_covariance(fids[2], fids[2]), base.get_covariance(fids[2], fids[2]))


# ------------------------------------------------------------------------------------------ 6. errors
def test_errors_and_bitwise_properties(gpu_lib):
    from svin_amd import distributed as sd
    from svin_amd import estimator
    spec = small_window("euroc", L=14, seed=6)
    est = new_estimator()
    fids, lids = syn.feed(est, spec)
    L, h = est.L, est.h
    pd = C.POINTER(C.c_double)
    cov = np.full(81, 7.0)
    lm = next(l for l in lids if len(est.landmark_observations(l)) >= 3)
    # unknown id, too small a cap (nothing written)
    assert L.svin_ba_get_covariance(h, 987654321, fids[0], cov.ctypes.data_as(pd), 81) == estimator.SVIN_ERR_NOT_FOUND
    assert L.svin_ba_get_covariance(h, fids[0], 987654321, cov.ctypes.data_as(pd), 81) == estimator.SVIN_ERR_NOT_FOUND
    assert L.svin_ba_get_covariance(h, fids[0], lm, cov.ctypes.data_as(pd), 17) == estimator.SVIN_ERR_INVALID_ARG
    assert np.all(cov == 7.0) and est.covariance_pass_count() == 0
    assert L.svin_ba_get_covariance(h, fids[0], lm, cov.ctypes.data_as(pd), 18) == 18 and np.all(cov[18:] == 7.0)
    with pytest.raises(RuntimeError):
        est.get_covariance(987654321, lm)
    # sizes only
    ia, ib = np.array([fids[0], lm], np.uint64), np.array([lm, lm], np.uint64)
    da, db = np.zeros(2, np.int32), np.zeros(2, np.int32)
    pu, pi = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    assert L.svin_ba_get_covariance_blocks(h, 2, ia.ctypes.data_as(pu), ib.ctypes.data_as(pu), da.ctypes.data_as(pi), db.ctypes.data_as(pi), None, 0) == 27
    assert list(da) == [6, 3] and list(db) == [3, 3]
    assert L.svin_ba_get_covariance_blocks(h, 2, ia.ctypes.data_as(pu), ib.ctypes.data_as(pu), None, None, cov.ctypes.data_as(pd), 26) == estimator.SVIN_ERR_INVALID_ARG
    # Sigma[b, a] == Sigma[a, b]^T and call-to-call equality, bitwise, across every kind of pair
    sbs = [b for b in est.parameter_block_ids() if (est.describe_block(b) or (0, -1))[1] == 2]
    lm2 = next(l for l in lids if l != lm and len(est.landmark_observations(l)) >= 3)
    ids = [fids[1], fids[2], sbs[0], lm, lm2]
    first = {(a, b): est.get_covariance(a, b) for a in ids for b in ids}
    for (a, b), X in first.items():
        assert np.array_equal(X, first[(b, a)].T), (a, b)
        assert np.any(X), (a, b)
    assert est.set_T_WS(fids[1], est.get_T_WS(fids[1]))   # drops the kept result: a fresh pass
    n0 = est.covariance_pass_count()
    for (a, b), X in first.items():
        assert np.array_equal(X, est.get_covariance(a, b)), (a, b)
    assert est.covariance_pass_count() == n0 + 1
    # a landmark with a single observation: SINGULAR naming its id; the same handle answers once the observation's landmark is gone
    single = est.new_id()
    assert est.add_landmark(single, np.r_[spec.lm_true[0][:3] + 0.3, 1.0])
    assert est.add_observation(single, fids[1], 0, 900, np.array([300.0, 200.0]), 8.0)
    with pytest.raises(estimator.SingularError) as ei:
        est.get_covariance(fids[1], fids[1])
    assert str(single) in str(ei.value)
    n1 = est.covariance_pass_count()
    assert L.svin_ba_get_covariance(h, fids[1], fids[1], cov.ctypes.data_as(pd), 81) == estimator.SVIN_ERR_SINGULAR
    assert est.covariance_pass_count() == n1   # nothing was kept: the call ran the pass again, and it does not count
    assert est.remove_observation(single, fids[1], 0, 900)
    again = est.get_covariance(fids[1], fids[2])   # (the window has one more landmark node than when `first` was taken)
    assert np.allclose(again, first[(fids[1], fids[2])], rtol=1e-9, atol=0.0)
    # no prior on the first pose: the gauge is free
    free = new_estimator()
    ffids, _ = syn.feed(free, spec)
    removed = 0
    for b in [ffids[0]] + [x for x in free.parameter_block_ids() if (free.describe_block(x) or (0, -1, 0))[0] == ffids[0]]:
        for rid in free.residuals_of(b):
            if free.parameters_of(rid)[0] == [b]:   # the unary factors of the first frame: PoseError, SpeedAndBiasError
                removed += free.map_remove_residual_block(rid) == 1
    assert removed >= 1
    with pytest.raises(estimator.SingularError) as ei:
        free.get_covariance(ffids[1], ffids[1])
    assert "reduced system" in str(ei.value)
    free.optimize(2)   # the handle stays usable
    # reduced manifold and sharded mode
    man = new_estimator()
    mf, _ = syn.feed(man, spec)
    assert man.reset_parameterization(mf[1], 3)
    assert man.L.svin_ba_get_covariance(man.h, mf[2], mf[2], cov.ctypes.data_as(pd), 81) == estimator.SVIN_ERR_UNSUPPORTED
    assert b"manifold" in man.L.svin_ba_last_error()
    world = 2
    ar = sd.ThreadAllReduce(world)
    e = new_estimator()
    syn.feed(e, sd.shard_spec(spec, 0, world))
    e.set_distributed(0, world, ar.callback(0))
    assert e.L.svin_ba_get_covariance(e.h, e.frame_ids()[1], e.frame_ids()[1], cov.ctypes.data_as(pd), 81) == estimator.SVIN_ERR_UNSUPPORTED

