"""Residual loss functions on the device (svin_ba_map_set_residual_loss): Ceres' TrivialLoss, CauchyLoss(a) and HuberLoss(a) on
reprojection residuals (a per-window loss table, the selector in bits 28-31 of the packed observation index) and on the small
factors, host residuals included (DevFactor::lossKind / lossScale, sqrt(rho') beside the factor's record).  Pinned against the
oracle's Map (the CPU restatement of Map.cpp and of Ceres' corrector), against the robust gradient formed in numpy from the
unrobustified residuals and Jacobians, and against the default path bit for bit."""
import numpy as np
import pytest

from svin_amd import synthetic as syn

pytestmark = pytest.mark.gpu
NONE, CAUCHY, HUBER = 0, 1, 2


def quat_close(a, b):
    return min(np.linalg.norm(a - b), np.linalg.norm(a + b))


def rho(kind, a, s):
    """rho, rho' of Ceres' loss_function.cc (the numbers the oracle uses, DBL_MIN floor on rho')"""
    if kind == CAUCHY:
        b = a * a
        return b * np.log1p(s / b), max(np.finfo(float).tiny, 1.0 / (1.0 + s / b))
    if kind == HUBER and s > a * a:
        r = np.sqrt(s)
        return 2.0 * a * r - a * a, max(np.finfo(float).tiny, a / r)
    return s, 1.0


def rot(qv):
    x, y, z, w = qv
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def map_window(losses, n=120, seed=5, with_oracle=True, constant_landmarks=False, outliers=(3, 17, 40), reference_geometry=False):
    """TestMap.cpp-shaped window through the Map interface: pose 1 variable under a weak PoseError, a constant pose 3 seen as
    well, constant extrinsics 2, n landmarks under an equidistant camera (variable under a weak HomogeneousPointError, or
    constant).  reference_geometry: the TestMarginalization.cpp shape instead -- three poses, two of them constant (3 and 4), and
    the extrinsics variable under PoseError(T_SC, 1e-4, 1e-4).  losses(i) -> (kind, a) of reprojection residual i.  The same calls
    on the oracle's Map when with_oracle."""
    from svin_amd.estimator import Estimator
    from oracle import orc
    rng = np.random.default_rng(seed)
    intr, dist = [350.0, 360.0, 378.0, 238.0], [-0.21, 0.14, 0.0006, 0.0003]
    T_WS = np.r_[rng.uniform(-3, 3, 3), 0, 0, 0, 1.0]
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    T_WS[3:] = q
    T_SC = np.r_[0.1, -0.05, 0.02, 0.0, 0.0, 0.0, 1.0]
    T_3 = T_WS.copy(); T_3[:3] += np.r_[0.3, -0.1, 0.05]
    T_4 = T_WS.copy(); T_4[:3] += np.r_[-0.2, 0.25, -0.1]
    views = ((1, T_WS), (3, T_3), (4, T_4)) if reference_geometry else ((1, T_WS), (3, T_3))
    est = Estimator(0)
    m = orc.OracleMap() if with_oracle else None
    L = orc.lib()
    est.add_camera(syn.DIST_EQUIDISTANT, intr, dist, 752, 480, [0, 0, 0, 0])
    T_init = T_WS.copy(); T_init[:3] += 0.05 * rng.normal(size=3)
    for bid, T in ((1, T_init), (2, T_SC), (3, T_3)) + (((4, T_4),) if reference_geometry else ()):
        assert est.map_add_parameter_block(bid, est.BLOCK_POSE, T)
        if m is not None:
            m.add_param(bid, orc.BLOCK_POSE, T)
    for bid in ((3, 4) if reference_geometry else (2, 3)):
        assert est.set_parameter_block_constant(bid)
        if m is not None:
            m.set_constant(bid)
    info6 = np.diag([1e-2] * 3 + [1e-1] * 3)
    pose_rid = est.map_add_pose_error(1, T_init, info6)
    assert pose_rid != 0
    if m is not None:
        L.orc_map_add_pose_error(m.h, orc.dptr(orc.arr(T_init)), orc.dptr(orc.arr(info6)), 1)
    if reference_geometry:   # PoseError(T_SC, 1e-4, 1e-4) on the extrinsics (TestMarginalization.cpp)
        infoE = np.eye(6) * 1e4
        assert est.map_add_pose_error(2, T_SC, infoE) != 0
        if m is not None:
            L.orc_map_add_pose_error(m.h, orc.dptr(orc.arr(T_SC)), orc.dptr(orc.arr(infoE)), 2)
    Rws, Rsc = rot(T_WS[3:]), rot(T_SC[3:])
    rids = []
    for i in range(n):
        pc = np.r_[rng.uniform(-1.2, 1.2, 2), 1.0] * (3.0 * (i % 10) + 2.0)
        pw = Rws @ (Rsc @ pc + T_SC[:3]) + T_WS[:3]
        hp = np.r_[pw + 0.05 * rng.normal(size=3), 1.0]
        assert est.map_add_parameter_block(10 + i, est.BLOCK_HOMOGENEOUS_POINT, hp)
        if m is not None:
            m.add_param(10 + i, orc.BLOCK_HPOINT, hp)
        for pose, Tp in views:
            pcam = Rsc.T @ (rot(Tp[3:]).T @ (pw - Tp[:3]) - T_SC[:3])
            r = np.hypot(pcam[0], pcam[1]); th = np.arctan2(r, pcam[2])
            thd = th * (1 + dist[0] * th ** 2 + dist[1] * th ** 4 + dist[2] * th ** 6 + dist[3] * th ** 8)
            s = thd / r if r > 1e-8 else 1.0
            uv = np.array([intr[0] * s * pcam[0] + intr[2], intr[1] * s * pcam[1] + intr[3]]) + rng.uniform(-1, 1, 2)
            if pose == 1 and i in outliers:
                uv += 25.0
            kind, a = losses(len(rids))
            rid = est.map_add_reprojection_error(pose, 10 + i, 2, 0, uv, np.eye(2))
            assert rid != 0 and est.map_set_residual_loss(rid, kind, a)
            if m is not None:
                assert a == 1.0
                m.add_reproj(orc.DIST_EQUIDISTANT, intr, dist, uv, np.eye(2), kind, pose, 10 + i, 2)
            rids.append(rid)
        if constant_landmarks:
            assert est.set_parameter_block_constant(10 + i)
            if m is not None:
                m.set_constant(10 + i)
        else:
            est.add_homogeneous_point_error(10 + i, hp, variance=4.0)
            if m is not None:
                m.add_hpoint_error(hp, 4.0, 10 + i)
    return est, m, L, rids, pose_rid, T_WS


@pytest.mark.parametrize("mode", ["none", "huber", "cauchy", "mixed"])
def test_reprojection_losses_match_the_oracle_map(gpu_lib, mode):
    pick = {"none": lambda i: (NONE, 1.0), "huber": lambda i: (HUBER, 1.0), "cauchy": lambda i: (CAUCHY, 1.0),
            "mixed": lambda i: ((NONE, HUBER, CAUCHY)[i % 3], 1.0)}[mode]
    # (no loss at all and 25-pixel outliers on weakly held landmarks is a badly conditioned problem: a landmark then travels metres
    # and back, and two implementations' paths part at rounding level long before they meet again at the fixed point -- the
    # outliers are for the robust modes)
    est, m, L, rids, _, T_WS = map_window(pick, n=100, reference_geometry=True, outliers=() if mode == "none" else (3, 17, 40))
    for i in (0, 1, 2, 5):
        assert est.map_get_residual_loss(rids[i]) == pick(i)
    # five iterations of the same trust-region algorithm on both sides, compared where they stand.  Near the fixed point the two
    # implementations' stopping tests, fed costs that agree to 1e-14, fire iterations apart (without a loss: 7 on the oracle, 12
    # on the device, final costs 1.5e-14 apart), so a comparison after convergence measures the stopping test, not the losses.
    est.set_solver_options(1e-14, 1e-14, 1e-14)
    L.orc_map_set_tolerances(m.h, 1e-14, 1e-14, 1e-14)
    est.optimize(5)
    so = m.solve(5)
    s = est.summary()
    dT = max(max(np.max(np.abs(est.get_parameter_block(b)[:3] - m.get_param(b)[:3])),
                 quat_close(est.get_parameter_block(b)[3:], m.get_param(b)[3:])) for b in (1, 2))
    dl = max(np.max(np.abs(est.get_parameter_block(10 + i) - m.get_param(10 + i))) for i in range(100))
    dc = abs(s["final_cost"] - so["final_cost"]) / so["final_cost"]
    print(mode, "gpu", s["final_cost"], s["iterations"], "oracle", so["final_cost"], so["iterations"], "dT", dT, "dlm", dl, "dcost", dc)
    assert s["iterations"] == so["iterations"] == 5
    assert dc <= 1e-12
    assert dT <= 1e-10 and dl <= 1e-10
    # eval_reprojection(robust) reports each residual under its own loss: the raw one scaled by sqrt(rho')
    ev = est.eval_reprojection(robust=False)
    byrid = {int(r): k for k, r in enumerate(ev["res_id"])}
    evr = est.eval_reprojection(robust=True)
    for i, rid in enumerate(rids[:12]):
        kind, a = pick(i)
        k = byrid[rid]
        sc = np.sqrt(rho(kind, a, float(ev["r"][k] @ ev["r"][k]))[1])
        assert np.allclose(evr["r"][k], sc * ev["r"][k], rtol=1e-13, atol=1e-15)
        assert np.allclose(evr["Jp"][k], sc * ev["Jp"][k], rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("a", [0.5, 2.0])
def test_scaled_losses_on_reprojections_and_factors_zero_the_robust_gradient(gpu_lib, a):
    """Cauchy(a) / Huber(a) on the reprojection residuals (outliers included), on a PoseError and on a RelativePoseError that pulls
    against it: at the device's fixed point the gradient sum_i rho'_i J_i^T r_i, formed here from the UNROBUSTIFIED residuals and
    minimal Jacobians and numpy's restatement of the loss, vanishes on the variable pose."""
    kinds = lambda i: ((CAUCHY, HUBER)[i % 2], a)
    est, _, _, rids, pose_rid, T_WS = map_window(kinds, n=80, seed=9, with_oracle=False, constant_landmarks=True)
    assert est.map_set_residual_loss(pose_rid, HUBER, a)
    assert est.set_parameter_block_constant(3, False)
    meas = est.get_parameter_block(3).copy(); meas[:3] += np.r_[1.0, 0.5, 0.0]   # an outlier prior on the second pose
    rel = est.map_add_relative_pose_error(1, 3, np.eye(6) * 4.0)
    pe3 = est.map_add_pose_error(3, meas, np.eye(6) * 10.0)
    assert rel and pe3
    assert est.map_set_residual_loss(rel, CAUCHY, a) and est.map_set_residual_loss(pe3, HUBER, a)
    assert est.map_get_residual_loss(rel) == (CAUCHY, a)
    est.set_solver_options(1e-16, 1e-16, 1e-16)
    est.optimize(60)
    g = {1: np.zeros(6), 3: np.zeros(6)}
    scale = {1: 0.0, 3: 0.0}
    ev = est.eval_reprojection(robust=False)
    loss_of = {rid: kinds(i) for i, rid in enumerate(rids)}
    for k in range(len(ev["res_id"])):
        rid, pose = int(ev["res_id"][k]), int(ev["pose_id"][k])
        r, J = ev["r"][k], ev["Jp"][k]
        w = rho(*loss_of[rid], float(r @ r))[1]
        g[pose] += w * J.T @ r
        scale[pose] += np.abs(w * J.T @ r).sum()
    n_out = 0
    flos = {pose_rid: (HUBER, a), rel: (CAUCHY, a), pe3: (HUBER, a)}
    for f in est.eval_factors():
        kind, sa = flos[f["res_id"]]
        s = float(f["r"] @ f["r"])
        w = rho(kind, sa, s)[1]
        n_out += w < 1.0
        for b, bid in enumerate(f["blocks"]):
            contrib = w * f["J"][:, 6 * b:6 * b + 6].T @ f["r"]
            g[bid] += contrib
            scale[bid] += np.abs(contrib).sum()
    print("a", a, "iterations", est.summary()["iterations"], "gradient", {k: float(np.max(np.abs(v))) for k, v in g.items()}, "scale", scale, "robust factors", n_out)
    assert n_out >= 1   # the outlier prior sits in the robust part of its loss
    # (a loss not applied, or applied twice, to any one outlier leaves a gradient of the order of `scale`)
    for bid in (1, 3):
        assert np.max(np.abs(g[bid])) < 1e-6 * scale[bid]


def test_host_residual_under_huber_ends_where_the_builtin_factor_ends(gpu_lib):
    from svin_amd import estimator
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=5, L=250, n_obs=2500, seed=31)
    ends = []
    for host in (False, True):
        est = Estimator(0)
        fids, lids = syn.feed(est, spec)
        meas = est.get_T_WS(fids[3]) + np.r_[0.4, -0.3, 0.2, 0, 0, 0, 0]
        info = np.eye(6) * 40.0
        if host:
            rid = est.map_add_host_residual([fids[3]], [7], 6, lambda ps: (lambda r, Jm, _: (r, [Jm]))(*estimator.host_pose_error(meas, info, ps[0])))
        else:
            rid = est.map_add_pose_error(fids[3], meas, info)
        assert rid and est.map_get_residual_loss(rid) == (NONE, 1.0)
        assert est.map_set_residual_loss(rid, HUBER, 0.5)
        est.set_solver_options(1e-14, 1e-14, 1e-14)
        est.optimize(15)
        ends.append((np.array([est.get_T_WS(f) for f in fids]), est.summary()))
    (Ta, sa), (Tb, sb) = ends
    print("built-in", sa["final_cost"], sa["iterations"], "host", sb["final_cost"], sb["iterations"], "dT", np.max(np.abs(Ta - Tb)))
    assert sa["iterations"] == sb["iterations"]
    assert abs(sa["final_cost"] - sb["final_cost"]) <= 1e-12 * sa["final_cost"]
    assert np.max(np.abs(Ta - Tb)) < 1e-12


def _states(est, fids, lids):
    return (np.array([est.get_T_WS(f) for f in fids]), np.array([est.get_speed_and_bias(f) for f in fids]),
            np.array([est.get_landmark(l)["point"] for l in lids]))


def test_explicit_default_losses_change_nothing(gpu_lib):
    """CauchyLoss(1) set on every observation and TrivialLoss on every factor of a config-#2 window: poses, summary and getLhs bit
    for bit as without the calls"""
    from svin_amd.estimator import Estimator
    spec = syn.make_window(seed=20250629)
    out = []
    for explicit in (False, True):
        est = Estimator(0)
        fids, lids = syn.feed(est, spec)
        if explicit:
            ev = est.eval_reprojection()
            for rid in ev["res_id"][:50]:
                assert est.map_get_residual_loss(int(rid)) == (CAUCHY, 1.0)
            for rid in ev["res_id"]:
                assert est.map_set_residual_loss(int(rid), CAUCHY, 1.0)
            for f in est.eval_factors():
                assert est.map_get_residual_loss(f["res_id"]) == (NONE, 1.0)
                assert est.map_set_residual_loss(f["res_id"], NONE)
        est.optimize(10)
        ids = est.parameter_block_ids()
        out.append((_states(est, fids, lids), est.summary(), est.get_lhs_blocks(ids)))
    (sa, ma, la), (sb, mb, lb) = out
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)
    for k in ("iterations", "successful", "initial_cost", "final_cost"):
        assert ma[k] == mb[k]
    assert len(la) == len(lb) and all(np.array_equal(x, y) for x, y in zip(la, lb))


def test_get_lhs_stays_loss_free(gpu_lib):
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=6, L=400, n_obs=4000, seed=77, pixel_noise=3.0)
    est0, est1 = Estimator(0), Estimator(0)
    syn.feed(est0, spec)
    syn.feed(est1, spec)
    ids = est0.parameter_block_ids()
    H0 = est0.get_lhs_blocks(ids)
    H1 = est1.get_lhs_blocks(ids)
    passes = est1.lhs_pass_count()
    for rid in est1.eval_reprojection()["res_id"]:
        assert est1.map_set_residual_loss(int(rid), HUBER, 0.5)
    for f in est1.eval_factors():
        assert est1.map_set_residual_loss(f["res_id"], HUBER, 0.5)
    H2 = est1.get_lhs_blocks(ids)
    assert est1.lhs_pass_count() == passes + 1
    assert all(np.array_equal(x, y) for x, y in zip(H0, H1)) and all(np.array_equal(x, y) for x, y in zip(H0, H2))


def _mixed_losses(est, seed):
    rng = np.random.default_rng(seed)
    for rid in est.eval_reprojection()["res_id"]:
        k = int(rng.integers(0, 4))
        if k:
            assert est.map_set_residual_loss(int(rid), (NONE, HUBER, CAUCHY)[k - 1], (0.5, 2.0, 1.0)[k - 1])
    for f in est.eval_factors():
        if f["kind"] == 0 and rng.integers(0, 2):
            assert est.map_set_residual_loss(f["res_id"], CAUCHY, 3.0)


def test_batch_of_windows_with_mixed_losses_ends_bit_for_bit_where_each_ends_alone(gpu_lib):
    from svin_amd import estimator
    from svin_amd.estimator import Estimator
    seeds = [20250629 + 7 * k for k in range(16)]

    def build(sd):
        est = Estimator(0)
        fids, lids = syn.feed(est, syn.make_window(seed=sd))
        _mixed_losses(est, sd)
        return est, fids, lids
    alone = []
    for sd in seeds:
        est, fids, lids = build(sd)
        est.optimize(10)
        alone.append((_states(est, fids, lids), est.summary()))
    batch = [build(sd) for sd in seeds]
    assert estimator.optimize_batch([b[0] for b in batch], 10) == 16
    for k, (est, fids, lids) in enumerate(batch):
        s, (ref, s_ref) = est.summary(), alone[k]
        assert s["iterations"] == s_ref["iterations"] and s["final_cost"] == s_ref["final_cost"]
        assert all(np.array_equal(x, y) for x, y in zip(_states(est, fids, lids), ref)), k


def test_resident_sliding_window_with_losses_equals_the_host_rebuild(gpu_lib):
    """30 frames, marginalising as it goes.  Every frame's new observations get a loss of their own BEFORE the frame is packed (the
    records still sit in the resident add log: setResidualLoss patches their packed handle there), and every fifth frame some
    observations already on the device change their loss (the resident table is rebuilt from the graph).  The device-resident
    path (pack mode 0) and the host rebuild (pack mode 1) end bit for bit alike, and the resident path was taken."""
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=30, L=900, n_obs=9000, seed=404, keyframe_every=2)
    ends = []
    for mode in (0, 1):
        est = Estimator(0)
        est.set_pack_mode(mode)
        rng = np.random.default_rng(1)
        patched = [0]

        def on_frame(k, fid):
            rids = est.residuals_of(fid)
            new = [int(r) for r, info in zip(rids, est.residual_info(rids)) if info[0] == 100]
            for rid in new:   # not packed yet: the pending add record is patched
                kind = int(rng.integers(0, 3))
                assert est.map_set_residual_loss(rid, kind, (1.0, 0.7, 1.5)[kind])
            patched[0] += len(new)
            est.optimize(3)
            if k % 5 == 4:   # already on the device: the resident table is rebuilt
                for rid in est.eval_reprojection()["res_id"][::37]:
                    assert est.map_set_residual_loss(int(rid), HUBER, 0.4)
                est.optimize(2)
            est.apply_marginalization(4, 3)
        syn.feed(est, spec, on_frame=on_frame)
        ends.append((np.array([est.get_T_WS(f) for f in est.frame_ids()]), est.summary(), est.path_counters(), patched[0]))
    (Ta, sa, pa, na), (Tb, sb, pb, nb) = ends
    print("resident", pa, "host", pb, sa["final_cost"], sb["final_cost"], "losses set before the pack", na)
    assert na == nb > 1000
    assert pa["resident_solves"] > 0 and pb["resident_solves"] == 0
    assert np.array_equal(Ta, Tb) and sa["final_cost"] == sb["final_cost"]


def test_marginalisation_m1_applies_each_residual_loss(gpu_lib, debug_option):
    """M1 (MarginalizationError.cpp:283-330) under losses other than the default.  Two windows are fed and optimised alike; at
    the first marginalisation, with identical states, one of them gives the leaving frame's camera-0 observations HuberLoss(2)
    (instead of CauchyLoss(1)) and a RelativePoseError between the leaving frame and the next CauchyLoss(0.5) (instead of none).
    The M1 system of that window (SVIN_MARG_KEEP_PRE) must be the default window's M1 system plus, per changed residual that
    entered it, (rho'_new - rho'_old) J^T J and -(rho'_new - rho'_old) J^T r, formed here from the UNROBUSTIFIED residuals and
    Jacobians the window reports and Ceres' corrector (tests/mp_m1.py restates it for the Cauchy loss)."""
    import mpmath as mp
    import mp_m1
    from svin_amd.estimator import Estimator
    from test_marginalization_m1_exact import scaled
    debug_option("SVIN_MARG_KEEP_PRE", 1)
    spec = syn.make_window(P=6, L=400, n_obs=4000, seed=61)
    runs = {}
    for robust in (False, True):
        est = Estimator(0)
        fids, rec = [], {}

        def on_frame(k, fid):
            fids.append(fid)
            if k == 2:
                rec["rel"] = est.map_add_relative_pose_error(fids[0], fids[1], np.eye(6) * 0.5)
                assert rec["rel"]
            if k >= 1:
                est.optimize(4)
            if k == 5:
                ev = est.eval_reprojection()
                if robust:
                    for j in range(len(ev["res_id"])):
                        if int(ev["pose_id"][j]) == fids[0] and int(ev["cam"][j]) == 0:
                            assert est.map_set_residual_loss(int(ev["res_id"][j]), HUBER, 2.0)
                    assert est.map_set_residual_loss(rec["rel"], CAUCHY, 0.5)
                rec["ev"], rec["fac"] = ev, est.eval_factors()
                ok, removed = est.apply_marginalization(3, 2)
                assert ok
                rec["removed"], rec["pre"] = sorted(int(i) for i in removed), est.marg_pre()
        syn.feed(est, spec, on_frame=on_frame)
        runs[robust] = (rec, list(fids))
    (d, fids), (r, _) = runs[False], runs[True]
    pd, pr = d["pre"], r["pre"]
    assert pd is not None and pr is not None and pd["rows_of"] == pr["rows_of"] and d["removed"] == r["removed"]
    assert np.array_equal(d["ev"]["r"], r["ev"]["r"]) and np.array_equal(d["ev"]["Jp"], r["ev"]["Jp"])   # the same point
    rows = pr["rows_of"]
    assert fids[0] in rows and rows[fids[0]][1] == 6   # the leaving pose is in the system
    H, b = pd["H"].copy(), pd["b0"].copy()

    def add(blocks, rv, dw):
        for (oa, Ja) in blocks:
            b[oa:oa + Ja.shape[1]] -= dw * (Ja.T @ rv)
            for (ob, Jb) in blocks:
                H[oa:oa + Ja.shape[1], ob:ob + Jb.shape[1]] += dw * (Ja.T @ Jb)
    ev, n_obs = r["ev"], 0
    for j in range(len(ev["res_id"])):
        p, lm = int(ev["pose_id"][j]), int(ev["lm_id"][j])
        if p != fids[0] or int(ev["cam"][j]) != 0 or lm not in rows:   # (observations of kept landmarks do not enter M1)
            continue
        rv = ev["r"][j]
        sq = float(rv @ rv)
        add([(rows[p][0], ev["Jp"][j]), (rows[lm][0], ev["Jl"][j])], rv, rho(HUBER, 2.0, sq)[1] - rho(CAUCHY, 1.0, sq)[1])
        n_obs += 1
    f = [x for x in r["fac"] if x["res_id"] == r["rel"]][0]
    assert f["blocks"] == [fids[0], fids[1]] and all(rows[i][1] == 6 for i in f["blocks"])
    rv, J = f["r"], f["J"]
    w = rho(CAUCHY, 0.5, float(rv @ rv))[1]
    # mp_m1's restatement of the corrector for this residual: J_c^T J_c = rho' J^T J
    _, (Jc,) = mp_m1.cauchy_corrector(mp_m1.mpv(rv), [mp.matrix(J.tolist())], mp.mpf(0.5))
    Jc = np.array(Jc.tolist(), dtype=float)
    assert np.max(np.abs(Jc.T @ Jc - w * (J.T @ J))) <= 1e-12 * np.max(np.abs(J.T @ J))
    add([(rows[fids[0]][0], J[:, :6]), (rows[fids[1]][0], J[:, 6:12])], rv, w - 1.0)
    dH, db, bs = scaled(pr["H"], pr["b0"], H, b)
    moved, _, _ = scaled(pr["H"], pr["b0"], pd["H"], pd["b0"])
    print("m1 under losses: changed observations", n_obs, "relative pose rho'", w, "| dH %.2e db %.2e (b scale %.2e), loss moved H by %.2e"
          % (dH, db, bs, moved))
    assert n_obs >= 10 and w < 0.9
    assert moved > 1e-3                              # the losses change the system ...
    assert dH <= 1e-12 and db <= 1e-12 * max(1.0, bs)   # ... exactly as the corrector says


def test_error_codes(gpu_lib):
    from svin_amd.estimator import Estimator
    est, _, _, rids, pose_rid, _ = map_window(lambda i: (CAUCHY, 1.0), n=20, with_oracle=False)
    L, h = est.L, est.h
    assert L.svin_ba_map_set_residual_loss(h, 987654321, CAUCHY, 1.0) == -2      # SVIN_ERR_NOT_FOUND
    assert L.svin_ba_map_set_residual_loss(h, rids[0], 3, 1.0) == -1             # unknown kind
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.svin_ba_map_set_residual_loss(h, rids[0], HUBER, bad) == -1
    hpe = [r for r in est.residuals_of(10) if est.residual_info([r])[0][0] == 102]
    assert hpe and L.svin_ba_map_set_residual_loss(h, hpe[0], HUBER, 1.0) == -4   # HomogeneousPointError: SVIN_ERR_UNSUPPORTED
    # the table holds 15 distinct losses (entry 0: CauchyLoss(1)); the 16th distinct one is refused, an existing one is not
    for k in range(14):
        assert L.svin_ba_map_set_residual_loss(h, rids[1 + k], HUBER, 1.0 + k) == 1
    assert L.svin_ba_map_set_residual_loss(h, rids[15], HUBER, 99.0) == -4
    assert L.svin_ba_map_set_residual_loss(h, rids[15], HUBER, 3.0) == 1
    assert L.svin_ba_map_set_residual_loss(h, pose_rid, HUBER, 99.0) == 1        # factors do not use the table
    assert est.map_get_residual_loss(pose_rid) == (HUBER, 99.0)
    with pytest.raises(RuntimeError):
        est.map_get_residual_loss(987654321)
    # a window with non-default losses is not taken into landmark-sharded mode (SVIN_ERR_UNSUPPORTED), the parameters are checked first
    import ctypes as C
    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p)(lambda *args: 1)
    assert L.svin_ba_set_distributed(h, 0, 2, C.cast(cb, C.c_void_p), None) == -4
    assert L.svin_ba_set_distributed(h, 0, 2, None, None) == -1
    assert L.svin_ba_set_distributed_rccl(h, 0, 2, bytes(128)) == -4
    est.optimize(5)
    assert np.isfinite(est.summary()["final_cost"])


def test_shim_losses_on_the_gpu(gpu_lib, tmp_path):
    """tests/csrc/shim_loss.cpp: NULL / HuberLoss(1) / CauchyLoss(2) reprojection residuals and a HuberLoss(0.5) PoseError through
    okvis::ceres::Map; lossFunctionPtr round-trips, an unsupported loss object throws, the solve converges"""
    import subprocess
    from test_shim_compile import _compile
    exe = _compile(tmp_path, "shim_loss")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-2000:])
    print(p.stdout)
    t = p.stdout.split()
    kv = {t[i]: t[i + 1] for i in range(0, len(t) - 1, 2) if t[i] in ("loss", "specs", "unsupported_throws", "final_cost", "initial_cost", "d_trans")}
    assert t[0] == "loss" and int(t[1]) == int(t[3]) == 90
    assert int(kv["specs"]) == 90 and int(kv["unsupported_throws"]) == 1
    assert float(kv["final_cost"]) < float(kv["initial_cost"]) and float(kv["d_trans"]) < 5e-2
