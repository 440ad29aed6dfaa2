"""General 2x2 information matrices on reprojection residuals, on the device (svin_ba_map_add_reprojection_error with any symmetric
positive-definite matrix, svin_ba_map_set / get_reprojection_information).  The error is weighted by S = L^T of information =
L L^T (ReprojectionErrorBase::setInformation); the device keeps S = (s00, s01, s11) per observation in DeviceProblem::obsS whenever
the window holds at least one such matrix and the host packs it.  Pinned against the oracle's Map (evaluation, linearisation,
getLhs, solve), against numpy's restatement of S applied to what the window reported before (transform property, M1), and against
the one-weight path bit for bit (batch, resident window)."""
import os

import numpy as np
import pytest

from svin_amd import synthetic as syn

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE, CAUCHY = 0, 1
INTR, DIST = [350.0, 360.0, 378.0, 238.0], [-0.21, 0.14, 0.0006, 0.0003]


def quat_close(a, b):
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b))


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def rot(qv):
    x, y, z, w = qv
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_information(rng, isotropic=False, max_ratio=100.0):
    """a seeded symmetric positive-definite 2x2 matrix with eigenvalue ratio <= max_ratio (symmetric bit for bit)"""
    l0 = rng.uniform(0.2, 2.0)
    if isotropic:
        return np.array([[l0, 0.0], [0.0, l0]])
    l1 = l0 * rng.uniform(1.5, max_ratio)
    a = rng.uniform(0.0, np.pi)
    c, s = np.cos(a), np.sin(a)
    off = c * s * (l0 - l1)
    return np.array([[c * c * l0 + s * s * l1, off], [off, s * s * l0 + c * c * l1]])


def sqrt_information(info):
    """S = L^T, information = L L^T"""
    return np.linalg.cholesky(np.asarray(info)).T


def info_window(n, seed, priors, prior_variance=4.0):
    """One variable pose under a weak PoseError, one constant extrinsics block, n landmarks with one observation each under an
    equidistant camera; a seeded information matrix per observation (every third one isotropic), landmark 5 constant, landmark 7
    behind the camera.  priors: a weak HomogeneousPointError on every variable landmark (one view alone leaves its depth free).
    The same calls on the oracle's Map.  Returns est, oracle map, oracle lib, [(device rid, oracle rid, information)]."""
    from svin_amd.estimator import Estimator
    from oracle import orc
    rng = np.random.default_rng(seed)
    T_WS = np.r_[rng.uniform(-3, 3, 3), 0, 0, 0, 1.0]
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    T_WS[3:] = q
    T_SC = np.r_[0.1, -0.05, 0.02, 0.0, 0.0, 0.0, 1.0]
    est, m, L = Estimator(0), orc.OracleMap(), orc.lib()
    est.add_camera(syn.DIST_EQUIDISTANT, INTR, DIST, 752, 480, [0, 0, 0, 0])
    T_init = T_WS.copy(); T_init[:3] += 0.05 * rng.normal(size=3)
    for bid, T in ((1, T_init), (2, T_SC)):
        assert est.map_add_parameter_block(bid, est.BLOCK_POSE, T)
        m.add_param(bid, orc.BLOCK_POSE, T)
    assert est.set_parameter_block_constant(2)
    m.set_constant(2)
    info6 = np.diag([1e-2] * 3 + [1e-1] * 3)
    assert est.map_add_pose_error(1, T_init, info6) != 0
    L.orc_map_add_pose_error(m.h, orc.dptr(orc.arr(T_init)), orc.dptr(orc.arr(info6)), 1)
    Rws, Rsc = rot(T_WS[3:]), rot(T_SC[3:])
    rids = []
    for i in range(n):
        pc = np.r_[rng.uniform(-1.2, 1.2, 2), 1.0] * (3.0 * (i % 10) + 2.0)
        if i == 7:
            pc[2] = -pc[2]   # behind the camera: the weighted residual is kept, the Jacobians are zero
        pw = Rws @ (Rsc @ pc + T_SC[:3]) + T_WS[:3]
        hp = np.r_[pw + 0.05 * rng.normal(size=3), 1.0]
        assert est.map_add_parameter_block(10 + i, est.BLOCK_HOMOGENEOUS_POINT, hp)
        m.add_param(10 + i, orc.BLOCK_HPOINT, hp)
        r = np.hypot(pc[0], pc[1]); th = np.arctan2(r, abs(pc[2]))
        thd = th * (1 + DIST[0] * th ** 2 + DIST[1] * th ** 4 + DIST[2] * th ** 6 + DIST[3] * th ** 8)
        s = thd / r if r > 1e-8 else 1.0
        uv = np.array([INTR[0] * s * pc[0] + INTR[2], INTR[1] * s * pc[1] + INTR[3]]) + rng.uniform(-1, 1, 2)
        info = random_information(rng, isotropic=(i % 3 == 0))
        rid = est.map_add_reprojection_error(1, 10 + i, 2, 0, uv, info)
        assert rid != 0, est.L.svin_ba_last_error()
        ro = m.add_reproj(orc.DIST_EQUIDISTANT, INTR, DIST, uv, info, orc.LOSS_CAUCHY, 1, 10 + i, 2)
        rids.append((rid, ro, info))
        if i == 5:
            assert est.set_parameter_block_constant(10 + i)
            m.set_constant(10 + i)
        elif priors:
            assert est.add_homogeneous_point_error(10 + i, hp, variance=prior_variance) != 0
            m.add_hpoint_error(hp, prior_variance, 10 + i)
    return est, m, L, rids


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("n", [127, 128, 129, 257])
def test_evaluation_against_the_oracle_map(gpu_lib, debug_option, n, split):
    """eval_reprojection(robust = 0 / 1) per residual against orc_map_eval at the tolerance of
    test_gpu_parity.test_reprojection_residuals_and_jacobians (1e-9 on r, 1e-10 on the Jacobians relative to max(1, |J|)); the
    constant landmark's Jl is zero, the point behind the camera keeps its weighted residual and has zero Jacobians"""
    if split:
        debug_option("SVIN_SPLIT_EVAL", 1)
    est, m, L, rids = info_window(n, 40 + n, priors=False)
    pc = est.path_counters()
    for robust in (False, True):
        ev = est.eval_reprojection(robust=robust)
        assert len(ev["r"]) == n
        byrid = {int(r): k for k, r in enumerate(ev["res_id"])}
        worst = dict(r=0.0, Jp=0.0, Jl=0.0, Je=0.0)
        for i, (rid, ro, info) in enumerate(rids):
            k = byrid[rid]
            r, Js, Jm = m.eval(ro)
            sc = np.sqrt(1.0 / (1.0 + r @ r)) if robust else 1.0
            if i == 5:
                assert not ev["Jl"][k].any() and ev["Jp"][k].any()   # constant landmark
                Jm[1] = np.zeros((2, 3))
            if i == 7:
                assert ev["r"][k].any() and not ev["Jp"][k].any() and not ev["Jl"][k].any() and not ev["Je"][k].any()
            worst["r"] = max(worst["r"], np.max(np.abs(ev["r"][k] - sc * r)))
            worst["Jp"] = max(worst["Jp"], np.max(np.abs(ev["Jp"][k] - sc * Jm[0])) / max(1.0, np.max(np.abs(Jm[0]))))
            worst["Jl"] = max(worst["Jl"], np.max(np.abs(ev["Jl"][k] - sc * Jm[1])) / max(1.0, np.max(np.abs(Jm[1]))))
            worst["Je"] = max(worst["Je"], np.max(np.abs(ev["Je"][k] - sc * Jm[2])) / max(1.0, np.max(np.abs(Jm[2]))))
        print("general information, n", n, "split", split, "robust", robust, worst)
        assert worst["r"] < 1e-9 and worst["Jp"] < 1e-10 and worst["Jl"] < 1e-10 and worst["Je"] < 1e-10
    # the matrices come back as given, svin_ba_debug_csr reports +-s00
    for rid, _, info in rids[:9]:
        got = est.map_get_reprojection_information(rid)
        if info[0, 1] != 0.0:
            assert np.array_equal(got, info)
        else:
            assert np.allclose(got, info, rtol=5e-16, atol=0.0)
    csr = est.debug_csr()
    assert not csr["resident"] and csr["N"] == n
    s00 = sorted(abs(sqrt_information(info)[0, 0]) for _, _, info in rids)
    assert np.allclose(sorted(np.abs(csr["w"])), s00, rtol=5e-16, atol=0.0)
    assert int(np.sum(csr["w"] < 0)) == 1   # the constant landmark's observation keeps the sign convention


# 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("n", [129, 257])
def test_linearisation_and_lhs_against_the_oracle_map(gpu_lib, debug_option, n, split):
    """svin_ba_linearize's S, g and cost against orc_map_linearize at 1e-9 relative (the diagonally normalised system, as
    test_gpu_parity.test_reduced_system_parity compares), get_lhs of the pose and of two landmarks against orc_map_get_lhs at the
    1e-10 of tests/test_gpu_lhs.py"""
    if split:
        debug_option("SVIN_SPLIT_EVAL", 1)
    # (a landmark seen once has its depth from the prior alone; under a weak prior the reduced system S = A - sum W V^-1 W^T is the
    # difference of nearly equal numbers and both sides lose digits to the cancellation: variance 0.25 keeps the comparison about S)
    est, m, L, rids = info_window(n, 70 + n, priors=True, prior_variance=0.25)
    lin_c, lin_g = m.linearize(0.0), est.linearize(0.0)
    assert lin_g["d"] == lin_c["d"] == 6 and [int(b) for b in lin_g["block_ids"]] == [1] == [int(b) for b in lin_c["cam_ids"]]
    sd = np.sqrt(np.abs(np.diag(lin_c["S"])))
    dS = rel(lin_g["S"] / np.outer(sd, sd), lin_c["S"] / np.outer(sd, sd))
    dg = rel(lin_g["g"] / sd, lin_c["g"] / sd)
    dc = abs(lin_g["cost"] - lin_c["cost"]) / lin_c["cost"]
    print("general information linearisation n", n, "split", split, "dS", dS, "dg", dg, "dcost", dc)
    assert dc <= 1e-9 and dS < 1e-9 and dg < 1e-9
    ids, dims = [1, 10 + 1, 10 + 4], [6, 3, 3]
    for b, H, d in zip(ids, est.get_lhs_blocks(ids), dims):
        ref = m.get_lhs(b, d)
        dd = np.linalg.norm(H - ref) / np.linalg.norm(ref)
        print("  get_lhs block", b, dd)
        assert dd <= 1e-10, (b, dd)


# 3 ---------------------------------------------------------------------------------------------------------------------------
def test_tiny_window_solve_with_general_information_matches_the_oracle_map(gpu_lib):
    """tests/golden/tiny_window.npz's geometry (2 poses, one constant; 2 constant extrinsics; 12 landmarks; 48 Cauchy-robustified
    residuals) with a seeded general matrix per residual: the device solve against the oracle Map's -- same iteration count, cost
    within 1e-9 relative, pose within 1e-6 (the tolerances of test_tiny_window_fixed_point_matches_independent_minimiser)"""
    from svin_amd.estimator import Estimator
    from oracle import orc
    g = np.load(os.path.join(GOLD, "tiny_window.npz"))
    rng = np.random.default_rng(2024)
    est, m, L = Estimator(0), orc.OracleMap(), orc.lib()
    for c in range(2):
        est.add_camera(syn.DIST_RADTAN, g["intr"], g["dist"], 752, 480, [0.0, 0.0, 0.0, 0.0])
    size = float(g["size"])
    for bid, T, const in ((1, g["T0"], True), (2, g["T1_init"], False), (3, g["T_SC"][0], True), (4, g["T_SC"][1], True)):
        assert est.map_add_parameter_block(bid, est.BLOCK_POSE, T)
        m.add_param(bid, orc.BLOCK_POSE, T)
        if const:
            assert est.set_parameter_block_constant(bid)
            m.set_constant(bid)
    nL = len(g["lm_init"])
    for l in range(nL):
        hp = np.r_[g["lm_init"][l], 1.0]
        assert est.map_add_parameter_block(10 + l, est.BLOCK_HOMOGENEOUS_POINT, hp)
        m.add_param(10 + l, orc.BLOCK_HPOINT, hp)
        for f, pose in enumerate((1, 2)):
            for c in range(2):
                info = random_information(rng, max_ratio=25.0) * (64.0 / (size * size))
                assert est.map_add_reprojection_error(pose, 10 + l, 3 + c, c, g["uv"][f, c, l], info) != 0
                m.add_reproj(orc.DIST_RADTAN, g["intr"], g["dist"], g["uv"][f, c, l], info, orc.LOSS_CAUCHY, pose, 10 + l, 3 + c)
    est.set_solver_options(1e-14, 1e-14, 1e-14)
    L.orc_map_set_tolerances(m.h, 1e-14, 1e-14, 1e-14)
    est.optimize(100)
    so, s = m.solve(100), est.summary()
    T1, To = est.get_parameter_block(2), m.get_param(2)
    print("tiny window, general information: gpu", s["final_cost"], s["iterations"], "oracle", so["final_cost"], so["iterations"], "dT",
          np.linalg.norm(T1[:3] - To[:3]), quat_close(T1[3:], To[3:]), "path", est.path_counters())
    assert s["iterations"] == so["iterations"]
    assert abs(s["final_cost"] - so["final_cost"]) < 1e-9 * so["final_cost"]
    assert np.linalg.norm(T1[:3] - To[:3]) < 1e-6 and quat_close(T1[3:], To[3:]) < 1e-6
    assert est.path_counters()["host_pack_solves"] == 1 and est.path_counters()["resident_solves"] == 0


# 4 ---------------------------------------------------------------------------------------------------------------------------
def _transform_property(est, rng, tag):
    """eval_reprojection(robust=0), general matrices on a third of the residuals, eval_reprojection again: the changed residuals and
    every Jacobian equal S_j (old / w_j), formed here, to 1e-12 relative; the others are bit-identical"""
    ev0 = est.eval_reprojection(robust=False)
    n = len(ev0["res_id"])
    changed = {}
    for k in range(0, n, 3):
        rid = int(ev0["res_id"][k])
        w2 = est.map_get_reprojection_information(rid)
        assert w2[0, 1] == 0.0 and w2[0, 0] == w2[1, 1]
        info = random_information(rng) * w2[0, 0]
        assert est.map_set_reprojection_information(rid, info)
        changed[rid] = (np.sqrt(w2[0, 0]), sqrt_information(info))
    ev1 = est.eval_reprojection(robust=False)
    assert np.array_equal(ev0["res_id"], ev1["res_id"])   # (both from the host's landmark-major order)
    idx = np.arange(0, n, 3)
    keep = np.ones(n, bool)
    keep[idx] = False
    w = np.array([changed[int(r)][0] for r in ev0["res_id"][idx]])
    S = np.stack([changed[int(r)][1] for r in ev0["res_id"][idx]])
    worst, same = 0.0, int(keep.sum())
    for name in ("r", "Jp", "Jl", "Je"):
        old = ev0[name][idx].reshape(len(idx), 2, -1)
        want = np.einsum("mij,mjk->mik", S, old / w[:, None, None])
        got = ev1[name][idx].reshape(len(idx), 2, -1)
        scale = np.max(np.abs(want), axis=(1, 2))
        dev = np.max(np.abs(got - want), axis=(1, 2))
        assert not got[scale == 0.0].any(), (tag, name)   # (zero Jacobians stay zero: invalid points, constant extrinsics)
        if np.any(scale > 0.0):
            worst = max(worst, float(np.max(dev[scale > 0.0] / scale[scale > 0.0])))
        assert np.array_equal(ev0[name][keep], ev1[name][keep]), (tag, name)
    print(tag, "transform property: residuals", n, "changed", len(changed), "worst relative deviation %.3e" % worst)
    assert len(changed) >= n // 3 and same >= n // 2
    assert worst <= 1e-12
    return ev1, changed


def test_transform_property_on_an_estimator_built_window(gpu_lib):
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=6, L=400, n_obs=4000, seed=88)
    est = Estimator(0)
    syn.feed(est, spec)
    _transform_property(est, np.random.default_rng(3), "narrow window")
    est.optimize(3)
    s, pc = est.summary(), est.path_counters()
    assert np.isfinite(s["final_cost"]) and s["final_cost"] < s["initial_cost"] and pc["host_pack_solves"] == 1


def test_transform_property_on_a_window_that_takes_the_split_evaluation(gpu_lib):
    """The narrowest window whose fused evaluation has more than kEvalSplitBlocks = 512 blocks (launchEvalAll: small factors + one
    block per 256 observations + the prior's), so that the trust-region loop's evaluation is k_eval_reproj_split + k_eval_rest_split:
    517 reprojection blocks alone.  The per-residual property is read through eval_reprojection; what the split kernel itself
    computes is held through linearize()'s cost, which must be the sum over the residuals of rho(|S e|^2) / 2 with CauchyLoss(1)
    plus the small factors' |r|^2 / 2, formed here from the unrobustified values.  The two sums run over 132 168 terms in different
    orders: each term carries a relative error of a few 1e-16 (log1p against log(1 + s)), a sum of N positive terms at most
    N x 1.1e-16 = 1.5e-11 of itself and about sqrt(N) x 1.1e-16 = 4e-14 when the roundings are independent; the bar is 1e-11."""
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=32, L=12000, n_obs=132168, seed=5)
    est = Estimator(0)
    syn.feed(est, spec)
    ev1, changed = _transform_property(est, np.random.default_rng(4), "wide window")
    fac = est.eval_factors()
    n_blocks = len(fac) + (len(ev1["res_id"]) + 255) // 256
    assert n_blocks > 512, n_blocks
    s = np.sum(ev1["r"] * ev1["r"], axis=1)
    want = 0.5 * float(np.sum(np.log1p(s))) + 0.5 * sum(float(f["r"] @ f["r"]) for f in fac)
    lin_cost = est.linearize(1e-4, cap=8192)["cost"]
    print("wide window: evaluation blocks", n_blocks, "cost", lin_cost, "numpy", want, "relative", abs(lin_cost - want) / want)
    assert abs(lin_cost - want) <= 1e-11 * want


# 5 ---------------------------------------------------------------------------------------------------------------------------
def test_marginalisation_m1_takes_the_general_information(gpu_lib, debug_option):
    """The differential scheme of test_gpu_loss.test_marginalisation_m1_applies_each_residual_loss on the same window: two windows
    fed and optimised alike; at the first marginalisation one of them sets general matrices on the leaving frame's camera-0
    observations.  Its M1 system (SVIN_MARG_KEEP_PRE) must be the default window's plus, per changed residual that entered it,
    rho'(s') J'^T J' - rho'(s) J^T J and the matching right-hand side, with r' = S (r / w), J' = S (J / w) formed here from the
    unrobustified residuals and Jacobians the window reported before the change."""
    from svin_amd.estimator import Estimator
    from test_marginalization_m1_exact import scaled
    debug_option("SVIN_MARG_KEEP_PRE", 1)
    spec = syn.make_window(P=6, L=400, n_obs=4000, seed=61)
    runs = {}
    for general in (False, True):
        est = Estimator(0)
        fids, rec = [], {}
        rng = np.random.default_rng(9)

        def on_frame(k, fid):
            fids.append(fid)
            if k >= 1:
                est.optimize(4)
            if k == 5:
                ev = est.eval_reprojection()
                rec["S"] = {}
                for j in range(len(ev["res_id"])):
                    if int(ev["pose_id"][j]) == fids[0] and int(ev["cam"][j]) == 0:
                        rid = int(ev["res_id"][j])
                        w2 = est.map_get_reprojection_information(rid)[0, 0]
                        info = random_information(rng) * w2
                        rec["S"][rid] = (np.sqrt(w2), sqrt_information(info))
                        if general:
                            assert est.map_set_reprojection_information(rid, info)
                rec["ev"] = ev
                ok, removed = est.apply_marginalization(3, 2)
                assert ok
                rec["removed"], rec["pre"], rec["path"] = sorted(int(i) for i in removed), est.marg_pre(), est.path_counters()
        syn.feed(est, spec, on_frame=on_frame)
        runs[general] = (rec, list(fids))
    (d, fids), (r, _) = runs[False], runs[True]
    pd, pr = d["pre"], r["pre"]
    assert pd is not None and pr is not None and pd["rows_of"] == pr["rows_of"] and d["removed"] == r["removed"]
    assert np.array_equal(d["ev"]["r"], r["ev"]["r"]) and np.array_equal(d["ev"]["Jp"], r["ev"]["Jp"])   # the same point
    assert sorted(d["S"]) == sorted(r["S"])
    rows = pr["rows_of"]
    assert fids[0] in rows and rows[fids[0]][1] == 6   # the leaving pose is in the system
    H, b = pd["H"].copy(), pd["b0"].copy()
    ev, n_obs = r["ev"], 0
    for j in range(len(ev["res_id"])):
        p, lm, rid = int(ev["pose_id"][j]), int(ev["lm_id"][j]), int(ev["res_id"][j])
        if rid not in r["S"] or lm not in rows:   # (observations of kept landmarks do not enter M1)
            continue
        w, S = r["S"][rid]
        for sign, T in ((1.0, S / w), (-1.0, np.eye(2))):
            rv = T @ ev["r"][j]
            blocks = [(rows[p][0], T @ ev["Jp"][j]), (rows[lm][0], T @ ev["Jl"][j])]
            dw = sign / (1.0 + float(rv @ rv))   # rho' of CauchyLoss(1)
            for (oa, Ja) in blocks:
                b[oa:oa + Ja.shape[1]] -= dw * (Ja.T @ rv)
                for (ob, Jb) in blocks:
                    H[oa:oa + Ja.shape[1], ob:ob + Jb.shape[1]] += dw * (Ja.T @ Jb)
        n_obs += 1
    dH, db, bs = scaled(pr["H"], pr["b0"], H, b)
    moved, _, _ = scaled(pr["H"], pr["b0"], pd["H"], pd["b0"])
    print("m1 under general information: changed observations", n_obs, "| dH %.2e db %.2e (b scale %.2e), the matrices moved H by %.2e"
          % (dH, db, bs, moved), "paths", d["path"], r["path"])
    assert n_obs >= 10
    assert moved > 1e-3
    assert dH <= 1e-12 and db <= 1e-12 * max(1.0, bs)
    assert r["path"]["host_assembled_marginalisations"] >= 1
    assert r["path"]["host_assembled_marginalisations"] > d["path"]["host_assembled_marginalisations"]


# 6 ---------------------------------------------------------------------------------------------------------------------------
def _states(est, fids, lids):
    return (np.array([est.get_T_WS(f) for f in fids]), np.array([est.get_speed_and_bias(f) for f in fids]),
            np.array([est.get_landmark(l)["point"] for l in lids]))


def test_batch_with_general_information_ends_bit_for_bit_where_each_window_ends_alone(gpu_lib):
    from svin_amd import estimator
    from svin_amd.estimator import Estimator
    seeds = [311, 322, 333, 344]

    def build(k):
        est = Estimator(0)
        fids, lids = syn.feed(est, syn.make_window(P=5, L=300, n_obs=3000, seed=seeds[k]))
        if k % 2 == 1:   # two of the four: general matrices on a third of the observations
            rng = np.random.default_rng(seeds[k])
            for rid in est.eval_reprojection()["res_id"][::3]:
                w2 = est.map_get_reprojection_information(int(rid))[0, 0]
                assert est.map_set_reprojection_information(int(rid), random_information(rng) * w2)
        return est, fids, lids
    alone = []
    for k in range(4):
        est, fids, lids = build(k)
        est.optimize(8)
        alone.append((_states(est, fids, lids), est.summary(), est.path_counters()))
    batch = [build(k) for k in range(4)]
    assert estimator.optimize_batch([b[0] for b in batch], 8) == 4
    for k, (est, fids, lids) in enumerate(batch):
        s, (ref, s_ref, path) = est.summary(), alone[k]
        assert s["iterations"] == s_ref["iterations"] and s["final_cost"] == s_ref["final_cost"], k
        assert all(np.array_equal(x, y) for x, y in zip(_states(est, fids, lids), ref)), k
        assert path["host_pack_solves"] == (1 if k % 2 else 0)
    assert alone[1][1]["final_cost"] != alone[0][1]["final_cost"]


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_resident_window_falls_back_to_the_host_pack_and_returns(gpu_lib):
    """A sliding window of 8 frames.  While one observation carries a general matrix the window is packed by the host (counted in
    host_pack_solves, debug_csr says so); after set_reprojection_information(rid, s I) the resident path is taken again and the
    window ends bit for bit where a window that never left the one-weight form ends.  Then a general matrix during the slide:
    solved on the host pack, marginalised by a host-assembled job."""
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=8, L=300, n_obs=3000, seed=505, keyframe_every=2)
    ends = []
    for detour in (False, True):
        est = Estimator(0)
        seen = {}

        def on_frame(k, fid):
            est.optimize(3)
            if k == 4 and detour:
                rid = int(est.eval_reprojection()["res_id"][11])
                before = est.path_counters()
                w2 = est.map_get_reprojection_information(rid)
                assert est.map_set_reprojection_information(rid, np.array([[2.0, 0.3], [0.3, 1.0]]) * w2[0, 0])
                assert not est.debug_csr()["resident"]
                est.prepare()   # packs, solves nothing
                mid = est.path_counters()
                assert mid["host_pack_solves"] == before["host_pack_solves"] + 1 and mid["resident_solves"] == before["resident_solves"]
                assert est.map_set_reprojection_information(rid, w2)   # s I: back to the one-weight form
                assert np.array_equal(est.map_get_reprojection_information(rid), w2)
                assert est.debug_csr()["resident"]
                seen["mid"] = mid
            if k >= 5:
                est.apply_marginalization(3, 2)
        fids, lids = syn.feed(est, spec, on_frame=on_frame)
        est.optimize(3)
        ends.append((np.array([est.get_T_WS(f) for f in est.frame_ids()]), est.summary(), est.path_counters(), seen))
        last = est
    (Ta, sa, pa, _), (Tb, sb, pb, seen) = ends
    print("never left", pa, "detour", pb, sa["final_cost"], sb["final_cost"])
    assert pb["resident_solves"] > seen["mid"]["resident_solves"]          # resident again after the detour
    assert pb["host_pack_solves"] == 1 and pa["host_pack_solves"] == 0
    assert np.array_equal(Ta, Tb) and sa["final_cost"] == sb["final_cost"] and sa["iterations"] == sb["iterations"]
    # a general matrix that stays: host pack, finite and decreasing cost
    rid = int(last.eval_reprojection()["res_id"][5])
    w2 = last.map_get_reprojection_information(rid)[0, 0]
    assert last.map_set_reprojection_information(rid, np.array([[3.0, -0.5], [-0.5, 0.7]]) * w2)
    last.optimize(3)
    s, pc = last.summary(), last.path_counters()
    assert pc["host_pack_solves"] == pb["host_pack_solves"] + 1 and np.isfinite(s["final_cost"]) and s["final_cost"] <= s["initial_cost"]
    assert last.map_remove_residual_block(rid)   # the entry leaves with its observation: resident again
    last.optimize(1)
    assert last.path_counters()["resident_solves"] == pc["resident_solves"] + 1


# 8 ---------------------------------------------------------------------------------------------------------------------------
def test_return_codes_of_the_new_entry_points(gpu_lib):
    import ctypes as C
    est, m, _, rids = info_window(20, 3, priors=True)
    L, h = est.L, est.h
    pdbl = C.POINTER(C.c_double)

    def arr4(a):
        return np.ascontiguousarray(a, np.float64).reshape(4)
    good, out = arr4([[2.0, 0.5], [0.5, 1.0]]), np.zeros(4)
    rid = rids[1][0]
    setf, getf = L.svin_ba_map_set_reprojection_information, L.svin_ba_map_get_reprojection_information
    assert setf(h, 987654321, good.ctypes.data_as(pdbl)) == -2 and getf(h, 987654321, out.ctypes.data_as(pdbl)) == -2   # SVIN_ERR_NOT_FOUND
    for bad in ([[2.0, 0.3], [0.2, 1.0]], [[1.0, 2.0], [2.0, 1.0]], [[0.0, 0.0], [0.0, 0.0]], [[np.nan, 0.0], [0.0, 1.0]],
                [[1.0, np.nan], [np.nan, 1.0]], [[np.inf, 0.0], [0.0, 1.0]], [[-1.0, 0.0], [0.0, -1.0]]):
        b = arr4(bad)
        assert setf(h, rid, b.ctypes.data_as(pdbl)) == -1, bad                                   # SVIN_ERR_INVALID_ARG
        assert est.map_add_reprojection_error(1, 11, 2, 0, [300.0, 200.0], np.array(bad)) == 0   # refused with a text
        assert b"information" in L.svin_ba_last_error()
    assert np.array_equal(est.map_get_reprojection_information(rid), rids[1][2])   # the refused calls changed nothing
    factor = [f["res_id"] for f in est.eval_factors()][0]
    hpe = [r for r in est.residuals_of(11) if est.residual_info([r])[0][0] == 102]
    for other in (factor, hpe[0]):
        assert setf(h, other, good.ctypes.data_as(pdbl)) == -4 and getf(h, other, out.ctypes.data_as(pdbl)) == -4   # SVIN_ERR_UNSUPPORTED
    assert setf(h, rid, good.ctypes.data_as(pdbl)) == 1 and getf(h, rid, out.ctypes.data_as(pdbl)) == 1
    assert np.array_equal(out, good)
    with pytest.raises(RuntimeError):
        est.map_set_reprojection_information(rid, [[1.0, 2.0], [2.0, 1.0]])
    # s I returns the residual to the one-weight form; once every general matrix is gone the window qualifies for the resident path
    for r_, _, info in rids:
        assert est.map_set_reprojection_information(r_, np.eye(2) * 0.81)
        assert np.allclose(est.map_get_reprojection_information(r_), np.eye(2) * 0.81, rtol=5e-16, atol=0.0)
    assert np.allclose(np.abs(est.debug_csr()["w"][:1]), 0.9, rtol=5e-16)
    est.optimize(3)
    assert np.isfinite(est.summary()["final_cost"])


# 9 ---------------------------------------------------------------------------------------------------------------------------
def test_shim_reprojection_errors_with_general_information_on_the_gpu(gpu_lib, tmp_path):
    """tests/csrc/shim_reproj_information.cpp: ReprojectionErrors with a non-diagonal covariance_t through okvis::ceres::Map, solved;
    the final cost against the same problem (the program prints its points, measurements and matrices) built here through the C ABI"""
    import subprocess
    from svin_amd.estimator import Estimator
    from test_shim_compile import _compile
    exe = _compile(tmp_path, "shim_reproj_information")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    obs, tail = [], None
    for line in p.stdout.splitlines():
        t = line.split()
        if t and t[0] == "obs":
            obs.append((int(t[1]), np.array([float(t[2]), float(t[3])]), np.array([float(x) for x in t[4:8]]).reshape(2, 2),
                        np.array([float(x) for x in t[8:11]])))
        elif t and t[0] == "added":
            tail = {t[i]: t[i + 1] for i in range(0, len(t) - 1, 2)}
    print(p.stdout.splitlines()[-1])
    assert tail is not None and len(obs) == 90 and int(tail["added"]) == 90 and int(tail["refused"]) == 1 and int(tail["info_roundtrip"]) == 90
    assert sum(1 for _, _, i, _ in obs if i[0, 1] != 0.0) == 60
    est = Estimator(0)
    est.add_camera(syn.DIST_EQUIDISTANT, INTR, DIST, 752, 480, [0, 0, 0, 0])
    assert est.map_add_parameter_block(1, est.BLOCK_POSE, np.r_[1.1, -2.05, 0.45, 0, 0, 0, 1.0])
    assert est.map_add_parameter_block(2, est.BLOCK_POSE, np.r_[0.1, -0.05, 0.02, 0, 0, 0, 1.0]) and est.set_parameter_block_constant(2)
    for i, (pid, uv, info, pw) in enumerate(obs):
        assert pid == i + 3
        assert est.map_add_parameter_block(pid, est.BLOCK_HOMOGENEOUS_POINT, np.r_[pw, 1.0]) and est.set_parameter_block_constant(pid)
        rid = est.map_add_reprojection_error(1, pid, 2, 0, uv, info)
        assert rid != 0 and est.map_set_residual_loss(rid, NONE)
    est.set_solver_options(1e-6, 1e-10, 1e-8)   # okvis::ceres::Map::Options' defaults
    est.optimize(20)
    s = est.summary()
    print("shim", tail["final_cost"], tail["initial_cost"], tail["iterations"], "C ABI", s["final_cost"], s["initial_cost"], s["iterations"])
    assert float(tail["final_cost"]) < float(tail["initial_cost"])   # (the measurements carry half a pixel of noise: the cost does not go to zero)
    # the same calls with the same numbers (17 significant digits round-trip a double) on the same library
    assert int(tail["iterations"]) == s["iterations"]
    assert abs(float(tail["initial_cost"]) - s["initial_cost"]) <= 1e-12 * s["initial_cost"]
    assert abs(float(tail["final_cost"]) - s["final_cost"]) <= 1e-12 * s["final_cost"]
