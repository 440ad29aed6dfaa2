"""Absolute keyframe measurements and the gauge (svin_pg_add_prior / remove_prior / num_priors / get_prior / set_gauge / get_gauge)
through the C ABI, on the case graphs of tests/helpers/pg_prior_cases.py, against the long-double reference
tests/helpers/pg_prior_reference.py (its host tests: tests/test_pg_prior_reference_host.py).

  stages         one debug_step per case and DoF: the local problem equals the restated construction (list order, ea = eb and eloop =
                 ekind = 3 on priors, eid, eprior, eloss; einfo to the rounding of an m x m Cholesky); the partition equals
                 pg_reference's restatement and the case's edge was reached; cholFail == 0; evaluation within the reference's bounds
                 (a prior's Jb zero exactly); node pass, solve and model by pg_reference's checks, the candidate's cost by the new
                 reference.
  determinism    a second step on a fresh handle returns the same bits, on every case.
  whole runs     (a) a rigidly moved noise-free trajectory is pulled onto the generating poses by position priors at a free gauge;
                 (b) a depth prior per keyframe takes a linear z drift out, to the helper Levenberg-Marquardt's optimum; (c) a gross
                 outlier fix under Cauchy ends nearer the truth than under no loss; (d) summary costs equal the numpy cost.
  covariances    whole columns under pg_cov_reference.check_columns on the extended problem; a prior shrinks Sigma_kk; no zero block
                 at a free gauge; SVIN_PG_ERR_SINGULAR with too few priors, the handle usable afterwards.
  removal        remove_prior and set_gauge(0) give back the bare graph's captures and results bit for bit.
  errors         every refusal leaves num_priors, the gauge and sentinel-filled outputs untouched.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pg_cases as pc  # noqa: E402
import pg_cov_reference as cr  # noqa: E402
import pg_prior_cases as qc  # noqa: E402
import pg_prior_reference as rr  # noqa: E402
import pg_reference as pr  # noqa: E402

from svin_amd import synthetic_pg as spg  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pr.have_long_double(), reason="np.longdouble is not an extended type on this platform")]

CASES = qc.build_cases()
BY_NAME = {c.name: c for c in CASES}
CASE_DOFS = [(c, six) for c in CASES for six in c.dofs]
IDS = ["%s-%ddof" % (c.name, 6 if six else 4) for c, six in CASE_DOFS]
_CAPTURES = {}
BITS = ("res", "Ja", "Jb", "g", "scale", "colsq", "nodeBlk", "y", "yS", "yawC", "tC", "qC")
SCALARS = ("cost", "costC", "gradmax", "model", "step2", "x2", "cholFail")
POSE, POSITION, DEPTH = rr.POSE, rr.POSITION, rr.DEPTH


def PoseGraph(*a, **kw):
    from svin_amd.posegraph import PoseGraph as P
    return P(*a, **kw)


def handle(case, six, **kw):
    g = PoseGraph(0, six_dof=six, **kw)
    case.configure(g)
    rr.feed(g, case.spec, case.callers, case.priors, case.gauge)
    return g


def _step(case, six):
    g = handle(case, six)
    before = g.poses()
    cap = g.debug_step(case.earliest, case.cur, case.radius)
    after = g.poses()
    assert cap is not None
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "debug_step moved the keyframes"
    g.close()
    return cap


def capture(case, six):
    key = (case.name, six)
    if key not in _CAPTURES:
        _CAPTURES[key] = _step(case, six)
    return _CAPTURES[key]


def same_bits(a, b):
    for key in BITS:
        assert np.array_equal(a[key].view(np.int64), b[key].view(np.int64)), key
    for key in SCALARS:
        assert np.float64(a[key]).tobytes() == np.float64(b[key]).tobytes(), key


# ---------------------------------------------------------------- 1. stages
@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_partition_and_problem(gpu_lib, case, six):
    cap = capture(case, six)
    P = case.problem(six)
    R = 6 if six else 4
    for key in rr.PROBLEM_KEYS:
        a, b = np.asarray(cap[key]), np.asarray(P[key])
        assert a.shape == b.shape, key
        if a.dtype.kind == "i" or key == "eloss":
            assert np.array_equal(a, b), key
        else:   # as tests/test_gpu_posegraph_stages.py: host float64 on both sides, other roundings
            assert np.max(np.abs(a - b), initial=0.0) <= 64 * pr.EPS64 * max(180.0, float(np.max(np.abs(b), initial=0.0))), key
    assert np.array_equal(cap["eloop"], cap["ekind"])
    prior_e = cap["ekind"] == 3
    assert np.array_equal(cap["ea"][prior_e], cap["eb"][prior_e]) and np.all(cap["eprior"][~prior_e] == -1)
    # the factor: the host's Cholesky of the m x m information against numpy's (tests/test_gpu_posegraph_edges.py's bound, on the block
    # the prior keeps); every entry outside that block is zero exactly
    Sa, Sb = cap["einfo"].reshape(-1, R, R), P["einfo"].reshape(-1, R, R)
    assert Sa.shape == Sb.shape
    for e in range(len(Sa)):
        assert np.all(np.tril(Sa[e], -1) == 0)
        if cap["ekind"][e] < 2:
            assert np.array_equal(Sa[e], Sb[e])
            continue
        m, first = (R, 0) if cap["ekind"][e] == 2 else rr.rows_of(cap["eprior"][e], six)
        keep = np.zeros((R, R), bool)
        keep[first:first + m, first:first + m] = True
        assert np.all(Sa[e][~keep] == 0.0)
        blk = Sb[e][first:first + m, first:first + m]
        assert np.max(np.abs(Sa[e] - Sb[e])) <= 4 * (m + 1) * pr.EPS64 * np.linalg.cond(blk) * np.max(np.abs(blk))
    ids = cap["eid"][prior_e]
    assert np.all(ids >= 1) and len(set(ids.tolist())) == len(ids)
    part = case.partition(cap, six)
    pr.check_partition(cap, part)
    assert cap["cholFail"] == 0
    case.reach(part, cap, six, ref=dict(yawC=cap["yawC"]))


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_evaluation(gpu_lib, case, six):
    rr.check_evaluation(capture(case, six), six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_node_pass(gpu_lib, case, six):
    rr.check_node_pass(capture(case, six), six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_solve(gpu_lib, case, six):
    pr.check_solve(capture(case, six), six, case.radius, verbose="eta %s %d-DoF" % (case.name, 6 if six else 4))


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_model_and_candidate(gpu_lib, case, six):
    rr.check_model_and_candidate(capture(case, six), six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_second_step_is_bit_identical(gpu_lib, case, six):
    same_bits(capture(case, six), _step(case, six))


# ---------------------------------------------------------------- 2. whole runs
def _error_to_truth(g, spec):
    T, _ = g.poses()
    return float(np.max(np.abs(T - spec.t_true)))


@pytest.mark.parametrize("six", [False, True])
def test_position_priors_pull_a_moved_trajectory_onto_the_truth(gpu_lib, six):
    """(a) the bars of tests/test_gpu_posegraph_edges.py::test_second_closure_and_outlier: the same situation"""
    spec, priors = qc.rigid_case(six)
    g = PoseGraph(0, six_dof=six, max_iterations=50)
    _, cur, _, _ = rr.feed(g, spec, [], priors, gauge=1)
    assert _error_to_truth(g, spec) > 1.0
    s = g.optimize(0, cur)
    print("%d-DoF rigid: %s, error to the generating poses %.3e" % (6 if six else 4, s, _error_to_truth(g, spec)))
    assert s["final_cost"] < 1e-9 * s["initial_cost"], s
    assert _error_to_truth(g, spec) < 1e-6
    g.close()


@pytest.mark.parametrize("six", [False, True])
def test_depth_priors_take_out_a_z_drift(gpu_lib, six):
    """(b) the final cost against the helper Levenberg-Marquardt's optimum to the solver's own function_tolerance; rms z error tenfold
    down (tests/test_pg_prior_reference_host.py shows that the optimum itself is)"""
    spec, priors = qc.depth_chain()
    g = PoseGraph(0, six_dof=six, max_iterations=50)
    _, cur, _, _ = rr.feed(g, spec, [], priors)
    P = rr.local_problem(spec, six, 0, cur, [], priors)
    _, opt, _ = rr.lm_solve(P, P, six)
    z0 = float(np.sqrt(np.mean((g.poses()[0][:, 2] - spec.t_true[:, 2]) ** 2)))
    s = g.optimize(0, cur)
    z1 = float(np.sqrt(np.mean((g.poses()[0][:, 2] - spec.t_true[:, 2]) ** 2)))
    print("%d-DoF depth chain: final cost %.12g, helper optimum %.12g, %d iterations, rms z error %.4g -> %.4g" %
          (6 if six else 4, s["final_cost"], opt, s["iterations"], z0, z1))
    assert spec.n <= 40
    assert abs(s["final_cost"] - opt) <= 1e-6 * opt
    assert z1 <= z0 / 10.0
    g.close()


@pytest.mark.parametrize("six", [False, True])
def test_outlier_fix_under_cauchy(gpu_lib, six):
    """(c) one fix two metres off among good ones: under Cauchy(0.5) the trajectory ends nearer the truth than under no loss"""
    spec, priors = qc.rigid_case(six)
    errs = {}
    for kind in (rr.LOSS_NONE, rr.LOSS_CAUCHY):
        bad = rr.prior(15, POSITION, spec.t_true[15] + np.array([2.0, -1.0, 0.5]), loss=kind, scale=0.5)
        g = PoseGraph(0, six_dof=six, max_iterations=50)
        _, cur, _, _ = rr.feed(g, spec, [], priors + [bad], gauge=1)
        g.optimize(0, cur)
        errs[kind] = _error_to_truth(g, spec)
        g.close()
    print("%d-DoF: error to the generating poses with the outlier fix under NONE %.3e, under Cauchy(0.5) %.3e" % (6 if six else 4, errs[0], errs[1]))
    assert errs[rr.LOSS_CAUCHY] < errs[rr.LOSS_NONE]


def _states_after(g, case, problem, six):
    T, Q = g.poses()
    lo, hi = case.earliest, case.cur + 1
    return cr.states_from_poses(problem, T[lo:hi], Q[lo:hi], six, pc._r2ypr)


@pytest.mark.parametrize("name,six", [("losses", False), ("losses", True), ("roles_4", False), ("roles_6", True), ("gauge_one_level_4", False),
                                      ("gauge_dense_6", True), ("mixed_shared4_sep_6", True)])
def test_summary_costs_equal_the_numpy_cost(gpu_lib, name, six):
    """(d) the bar of tests/test_gpu_posegraph_edges.py::test_summary_costs_equal_the_numpy_cost"""
    case = BY_NAME[name]
    g = handle(case, six)
    cap = g.debug_step(case.earliest, case.cur, case.radius)
    s = g.optimize(case.earliest, case.cur)
    c0 = rr.numpy_cost(cap, cap, six)
    c1 = rr.numpy_cost(cap, _states_after(g, case, cap, six), six)
    print("%s %d-DoF: initial %.12g (numpy %.12g) final %.12g (numpy %.12g)" % (name, 6 if six else 4, s["initial_cost"], c0, s["final_cost"], c1))
    assert abs(s["initial_cost"] - c0) <= 1e-10 * c0
    assert abs(s["final_cost"] - c1) <= 1e-10 * c1
    assert s["final_cost"] < s["initial_cost"]
    g.close()


@pytest.mark.parametrize("six", [False, True])
def test_free_gauge_without_priors_still_optimises(gpu_lib, six):
    spec = spg.make_pose_graph(n=60, laps=2, loop_every=7, seed=45)
    g = PoseGraph(0, six_dof=six)
    earliest, cur = spg.feed(g, spec)
    g.set_gauge(1)
    assert g.gauge() == 1
    from svin_amd.posegraph import _lib
    assert _lib().svin_pg_optimize(g.h, earliest, cur) == 1
    s = g.summary()
    assert np.isfinite(s["final_cost"]) and s["final_cost"] <= s["initial_cost"], s
    g.close()


# ---------------------------------------------------------------- 3. covariances
@pytest.mark.parametrize("name,six", [("losses", False), ("losses", True), ("roles_4", False), ("roles_6", True), ("left_out", True),
                                      ("mixed_shared3_band_4", False), ("gauge_dense_4", False), ("gauge_one_level_6", True),
                                      ("gauge_two_level_4", False), ("gauge_two_level_6", True)])
def test_covariance_columns(gpu_lib, name, six):
    case = BY_NAME[name]
    g = handle(case, six)
    cap = g.debug_step(case.earliest, case.cur, case.radius)
    A, _ = pr.system(cap["Ja"], cap["Jb"], cap["res"], cap["scale"], cap, six, np.inf)
    nn = len(cap["off"])
    cols = cr.role_columns(cap, cap)
    pairs = cr.column_pairs(nn, cols)
    e = case.earliest
    blocks = g.covariance_blocks(e, case.cur, [(e + a, e + b) for a, b in pairs])
    sigma = cr.columns_from_blocks(cap, six, cols, blocks)
    worst = cr.check_columns(A, cap["scale"], cap, six, cols, sigma)
    print("cov %s %d-DoF: worst eta ratio %.2f, forward / (kappa bar) %.3f" % (name, 6 if six else 4, worst["ratio"], worst["fwd"]))
    if case.gauge == 1:
        assert all(np.any(b != 0.0) for b in blocks), "a block is exactly zero at a free gauge"
    g.close()


@pytest.mark.parametrize("six", [False, True])
def test_a_prior_shrinks_the_keyframes_covariance(gpu_lib, six):
    spec = pc._graph(41, [(20, 0), (33, 6)], 291)
    D = 6 if six else 4
    sig = {}
    for with_prior in (False, True):
        g = PoseGraph(0, six_dof=six)
        rr.feed(g, spec, [], [qc.near(spec, 30, POSE, info=qc.pose_diag)] if with_prior else [])
        sig[with_prior] = g.covariance(0, 40, 30, 30)
        g.close()
    # information adds: Sigma_bare - Sigma_prior is positive semi-definite, and not zero
    diff = sig[False] - sig[True]
    w = np.linalg.eigvalsh((diff + diff.T) / 2)
    assert np.all(np.diag(sig[True]) < np.diag(sig[False])) and w.min() >= -1e-9 * np.max(np.abs(sig[False])) and w.max() > 0
    assert sig[True].shape == (D, D)


def test_too_few_priors_at_a_free_gauge_are_singular(gpu_lib):
    from svin_amd.posegraph import SingularError
    spec = pc._graph(41, [(20, 0), (33, 6)], 293)
    g = PoseGraph(0, six_dof=True)
    rr.feed(g, spec, [], [qc.near(spec, 10, POSITION, v=(0.1, 0.0, 0.0))], gauge=1)
    with pytest.raises(SingularError):
        g.covariance_blocks(0, 40, [(5, 5)])
    # the handle stays usable: the optimisation runs on the damped system, and two more fixes make the covariance regular
    s = g.optimize(0, 40)
    assert s["termination"] in (0, 1) and np.isfinite(s["final_cost"]) and s["final_cost"] <= s["initial_cost"]
    g.add_prior(25, POSITION, spec.t_svin[25])
    g.add_prior(38, POSITION, spec.t_svin[38])
    blk = g.covariance(0, 40, 5, 5)
    assert np.all(np.isfinite(blk)) and np.all(np.diag(blk) > 0)
    g.close()


def test_the_kept_covariance_factor_is_dropped(gpu_lib):
    spec = pc._graph(41, [(20, 0), (33, 6)], 295)
    g = PoseGraph(0, six_dof=False)
    spg.feed(g, spec)
    f0 = g.covariance_counters()["factorisations"]
    g.covariance(0, 40, 9, 9)
    g.covariance(0, 40, 9, 9)
    assert g.covariance_counters()["factorisations"] == f0 + 1
    pid = g.add_prior(9, DEPTH, spec.t_svin[9])
    g.covariance(0, 40, 9, 9)
    assert g.covariance_counters()["factorisations"] == f0 + 2, "add_prior kept the factor"
    g.remove_prior(pid)
    g.covariance(0, 40, 9, 9)
    assert g.covariance_counters()["factorisations"] == f0 + 3, "remove_prior kept the factor"
    g.set_gauge(0)
    g.covariance(0, 40, 9, 9)
    assert g.covariance_counters()["factorisations"] == f0 + 4, "set_gauge kept the factor"
    g.close()


# ---------------------------------------------------------------- 4. removal, get_prior
@pytest.mark.parametrize("six", [False, True])
def test_remove_prior_and_gauge_zero_restore_the_bare_graph(gpu_lib, six):
    base = pc.Case("bare", pc._graph(61, [(30, 0), (44, 9), (58, 21)], 203), piece=8, dense=0, levels=1)
    spec = base.spec
    bare, g = PoseGraph(0, six_dof=six), PoseGraph(0, six_dof=six)
    for h in (bare, g):
        base.configure(h)
        spg.feed(h, spec)
    priors = [qc.near(spec, 12, POSE, v=(0.1, 0.0, 0.2), info=qc.pose_info(80, 20.0)), qc.near(spec, 40, POSITION, v=(0.0, 0.1, 0.0)),
              qc.near(spec, 40, DEPTH, v=(0.0, 0.0, 0.3), loss=rr.LOSS_HUBER, scale=0.1)]
    ids = [g.add_prior(p["index"], p["kind"], p["t"], p["q"], p["yaw"], rr.info_of(p, six), p["loss"], p["scale"]) for p in priors]
    g.set_gauge(1)
    assert ids == [1, 2, 3] and g.num_priors() == 3 and g.gauge() == 1
    with_priors = g.debug_step(0, 60, 1e4)
    assert np.sum(with_priors["ekind"] == 3) == 3 and np.all(with_priors["off"] >= 0)
    g.remove_prior(ids[1])
    again = g.add_prior(5, DEPTH, [0.0, 0.0, 1.0])
    assert again == 4, "a prior id was reused"
    for i in (ids[0], ids[2], again):
        g.remove_prior(i)
    g.set_gauge(0)
    assert g.num_priors() == 0 and g.gauge() == 0
    a, b = bare.debug_step(0, 60, 1e4), g.debug_step(0, 60, 1e4)
    same_bits(a, b)
    for key in ("ea", "eb", "eloop", "ekind", "eid", "eprior", "off", "einfo", "eloss"):
        assert np.array_equal(a[key], b[key]), key
    assert np.all(b["ekind"] < 2) and np.all(b["eprior"] == -1)
    sa, sb = bare.optimize(0, 60), g.optimize(0, 60)
    assert all(sa[k] == sb[k] for k in ("initial_cost", "final_cost", "iterations", "termination", "successful"))
    assert np.array_equal(bare.poses()[0], g.poses()[0]) and np.array_equal(bare.poses()[1], g.poses()[1])
    bare.close(); g.close()


def test_get_prior_returns_what_was_given(gpu_lib):
    for six in (False, True):
        g = PoseGraph(0, six_dof=six)
        spg.feed(g, BY_NAME["losses"].spec)
        D = 6 if six else 4
        info = qc.spd(D, 90, 30.0)
        q = np.array([0.0, 0.0, np.sin(0.1), np.cos(0.1)])
        i = g.add_prior(7, POSE, [0.1, 0.2, 0.3], q, 11.5, info, rr.LOSS_CAUCHY, 0.7)
        p = g.get_prior(i)
        assert (p["index"], p["kind"], p["loss"], p["loss_scale"]) == (7, POSE, rr.LOSS_CAUCHY, 0.7)
        assert np.array_equal(p["t"], [0.1, 0.2, 0.3]) and np.array_equal(p["information"], info)
        assert np.array_equal(p["q"], q if six else [0.0, 0, 0, 1]) and p["yaw_deg"] == (0.0 if six else 11.5)
        j = g.add_prior(9, POSITION, [1.0, 2.0, 3.0], None, 0.0, None, rr.LOSS_NONE, -3.0)     # the scale of NONE is ignored
        p = g.get_prior(j)
        assert p["kind"] == POSITION and np.array_equal(p["information"], np.eye(3)) and np.array_equal(p["t"], [1.0, 2.0, 3.0])
        k = g.add_prior(9, DEPTH, [np.nan, np.inf, -4.5], None, np.nan, np.array([[16.0]]), rr.LOSS_HUBER, 0.2)   # t[2] alone is read
        p = g.get_prior(k)
        assert p["kind"] == DEPTH and np.array_equal(p["t"], [0.0, 0.0, -4.5]) and np.array_equal(p["information"], [[16.0]])
        assert (i, j, k) == (1, 2, 3) and g.num_priors() == 3
        g.close()


# ---------------------------------------------------------------- 5. errors
@pytest.mark.parametrize("six", [False, True])
def test_refusals_change_nothing(gpu_lib, six):
    from svin_amd.posegraph import _lib
    L = _lib()
    D = 6 if six else 4
    g = PoseGraph(0, six_dof=six)
    spg.feed(g, BY_NAME["losses"].spec)
    keep = g.add_prior(2, DEPTH, [0.0, 0.0, 1.0])
    pd = C.POINTER(C.c_double)
    t, q = np.array([0.1, 0.2, 0.3]), np.array([0.0, 0.0, 0.0, 1.0])
    good = {POSE: qc.spd(D, 91, 20.0), POSITION: qc.spd(3, 92, 20.0), DEPTH: np.array([[4.0]])}

    def add(h=None, index=3, kind=POSE, t_=t, q_=q, yaw=1.0, info="good", kl=rr.LOSS_HUBER, scale=0.5):
        p = lambda x: None if x is None else np.ascontiguousarray(x, np.float64).ctypes.data_as(pd)   # noqa: E731
        info = good.get(kind, good[POSE]) if isinstance(info, str) else info
        return L.svin_pg_add_prior(g.h if h is None else h, index, kind, p(t_), p(q_), yaw, p(info), kl, scale)
    refusals = [(dict(t_=None), -1), (dict(kind=3), -1), (dict(kind=-1), -1), (dict(t_=np.array([0.0, np.inf, 0.0])), -1),
                (dict(kind=DEPTH, t_=np.array([0.0, 0.0, np.nan])), -1), (dict(kl=3), -1), (dict(kl=-1), -1), (dict(scale=0.0), -1),
                (dict(scale=-1.0), -1), (dict(scale=np.nan), -1), (dict(scale=np.inf), -1), (dict(kl=rr.LOSS_CAUCHY, scale=0.0), -1),
                (dict(index=1000), -2), (dict(index=-4), -2), (dict(kind=DEPTH, info=np.array([[0.0]])), -1),
                (dict(kind=DEPTH, info=np.array([[-1.0]])), -1), (dict(kind=DEPTH, info=np.array([[np.nan]])), -1)]
    for kind in (POSE, POSITION):
        m = D if kind == POSE else 3
        asym = good[kind].copy(); asym[0, 1] = np.nextafter(asym[0, 1], np.inf)
        nan_info = good[kind].copy(); nan_info[1, 1] = np.nan
        semi = np.eye(m); semi[:2, :2] = 1.0
        indef = np.diag([1.0, -1.0] + [1.0] * (m - 2))
        refusals += [(dict(kind=kind, info=x), -1) for x in (asym, nan_info, semi, indef)]
    if six:
        refusals += [(dict(q_=None), -1), (dict(q_=np.array([0.0, np.nan, 0.0, 1.0])), -1)]
    else:
        refusals += [(dict(yaw=np.nan), -1)]
        assert add(q_=None) == keep + 1 and L.svin_pg_remove_prior(g.h, keep + 1) == 1        # q may be NULL in 4-DoF
    for kw, want in refusals:
        assert add(**kw) == want, (kw, want)
        assert L.svin_pg_last_error(), kw
        assert g.num_priors() == 1
    assert L.svin_pg_add_prior(None, 3, POSE, t.ctypes.data_as(pd), q.ctypes.data_as(pd), 0.0, None, 0, 1.0) == -1
    n0 = g.num_priors()
    assert add(kl=rr.LOSS_NONE, scale=np.nan) > keep and g.num_priors() == n0 + 1       # the scale of NONE is ignored
    assert add(kind=POSITION, q_=None, yaw=np.nan) > keep and g.num_priors() == n0 + 2   # q and yaw are POSE's alone
    # the gauge
    for bad in (2, -1):
        assert L.svin_pg_set_gauge(g.h, bad) == -1 and g.gauge() == 0
    assert L.svin_pg_set_gauge(None, 1) == -1 and L.svin_pg_get_gauge(None) == -1
    # remove / get: unknown ids, sentinel-filled outputs
    assert L.svin_pg_remove_prior(g.h, 999) == -2 and L.svin_pg_remove_prior(g.h, 0) == -2 and L.svin_pg_remove_prior(None, 1) == -1
    assert L.svin_pg_num_priors(None) == -1 and g.num_priors() == n0 + 2
    idx, kd, lk = C.c_int(-77), C.c_int(-77), C.c_int(-77)
    ot, oq, oy, oi, ol = np.full(3, -7.0), np.full(4, -7.0), np.full(1, -7.0), np.full(36, -7.0), np.full(1, -7.0)
    p = lambda x: x.ctypes.data_as(pd)   # noqa: E731
    for h, pid, want in ((g.h, 999, -2), (None, keep, -1)):
        assert L.svin_pg_get_prior(h, pid, C.byref(idx), C.byref(kd), p(ot), p(oq), p(oy), p(oi), C.byref(lk), p(ol)) == want
        assert (idx.value, kd.value, lk.value) == (-77, -77, -77)
        assert all(np.all(x == -7.0) for x in (ot, oq, oy, oi, ol))
    assert L.svin_pg_get_prior(g.h, keep, None, None, None, None, None, None, None, None) == 1
    # a DEPTH prior writes its 1 x 1 information and nothing behind it
    assert L.svin_pg_get_prior(g.h, keep, None, None, None, None, None, p(oi), None, None) == 1
    assert oi[0] == 1.0 and np.all(oi[1:] == -7.0)
    # the handle still optimises, and the first prior is still what it was
    assert g.get_prior(keep)["index"] == 2
    assert g.optimize(0, 60)["termination"] in (0, 1)
    g.close()
