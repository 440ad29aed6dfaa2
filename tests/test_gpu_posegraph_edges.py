"""Caller-given pose-graph edges (svin_pg_add_edge / remove_edge / num_edges / get_edge) through the C ABI, on the case graphs of
tests/helpers/pg_edge_cases.py, against the long-double reference tests/helpers/pg_edge_reference.py (its host tests:
tests/test_pg_edge_reference_host.py).

  stages         one debug_step per case and DoF: the local problem equals the restated construction (edge order, eloop = 2, ekind,
                 eid, eloss; einfo to the rounding of a D x D Cholesky); the partition equals pg_reference's restatement and the
                 case's edge was reached; cholFail == 0; evaluation within the new reference's bounds; node pass, solve and model by
                 pg_reference's checks (the candidate's cost by the new reference, which knows the caller edges).
  determinism    a second step on a fresh handle returns the same bits, on every case (the shared-destination cases are where
                 three and four terms meet in one block).
  both doors     loops given through add_keyframe against the same loops given as caller edges (information NULL + Huber(0.1),
                 and the squared weights written out): tests/test_gpu_posegraph.py's parity bars.
  whole run      summary costs equal the independent numpy cost; a second consistent closure brings a displaced session onto the
                 generating poses; a gross outlier under Cauchy ends nearer to them than under NONE.
  remove_edge    add then remove leaves captures and an optimisation bit for bit those of a handle that never had the edges.
  covariances    whole columns under pg_cov_reference.check_columns; a keyframe held only by a caller edge; SVIN_PG_ERR_SINGULAR
                 naming the keyframe once that edge is removed; the factor dropped by add_edge / remove_edge.
  errors         every refusal leaves num_edges and sentinel-filled outputs untouched.
"""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pg_cases as pc  # noqa: E402
import pg_cov_reference as cr  # noqa: E402
import pg_edge_cases as ec  # noqa: E402
import pg_edge_reference as er  # noqa: E402
import pg_reference as pr  # noqa: E402

from svin_amd import synthetic_pg as spg  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pr.have_long_double(), reason="np.longdouble is not an extended type on this platform")]

CASES = ec.build_cases()
BY_NAME = {c.name: c for c in CASES}
CASE_DOFS = [(c, six) for c in CASES for six in c.dofs]
IDS = ["%s-%ddof" % (c.name, 6 if six else 4) for c, six in CASE_DOFS]
_CAPTURES = {}
BITS = ("res", "Ja", "Jb", "g", "scale", "colsq", "nodeBlk", "y", "yS", "yawC", "tC", "qC")
SCALARS = ("cost", "costC", "gradmax", "model", "step2", "x2", "cholFail")


def PoseGraph(*a, **kw):
    from svin_amd.posegraph import PoseGraph as P
    return P(*a, **kw)


def handle(case, six, **kw):
    g = PoseGraph(0, six_dof=six, **kw)
    case.configure(g)
    er.feed(g, case.spec, case.callers)
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
    for key in er.PROBLEM_KEYS:
        a, b = np.asarray(cap[key]), np.asarray(P[key])
        assert a.shape == b.shape, key
        if a.dtype.kind == "i" or key == "eloss":
            assert np.array_equal(a, b), key
        else:   # as tests/test_gpu_posegraph_stages.py: host float64 on both sides, other roundings
            assert np.max(np.abs(a - b), initial=0.0) <= 64 * pr.EPS64 * max(180.0, float(np.max(np.abs(b), initial=0.0))), key
    assert np.array_equal(cap["eloop"], cap["ekind"])
    # the factor: the host's Cholesky against numpy's, both within gamma_(R+1) |S|^T |S| of the information (Higham 10.3): entries
    # of S differ by at most that backward error carried through the factorisation, cond(S) (R + 1) eps |S| to first order
    Sa, Sb = cap["einfo"].reshape(-1, R, R), P["einfo"].reshape(-1, R, R)
    assert Sa.shape == Sb.shape
    for e in range(len(Sa)):
        assert np.all(np.tril(Sa[e], -1) == 0)
        if cap["ekind"][e] != 2:
            assert np.array_equal(Sa[e], Sb[e])
        else:
            assert np.max(np.abs(Sa[e] - Sb[e])) <= 4 * (R + 1) * pr.EPS64 * np.linalg.cond(Sb[e]) * np.max(np.abs(Sb[e]))
    ids = cap["eid"][cap["ekind"] == 2]
    assert np.all(ids >= 1) and len(set(ids.tolist())) == len(ids) and np.all(cap["eid"][cap["ekind"] != 2] == 0)
    part = case.partition(cap, six)
    pr.check_partition(cap, part)
    assert cap["cholFail"] == 0
    case.reach(part, cap, six, ref=dict(yawC=cap["yawC"]))


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_evaluation(gpu_lib, case, six):
    er.check_evaluation(capture(case, six), six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_node_pass(gpu_lib, case, six):
    pr.check_node_pass(capture(case, six), six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_solve(gpu_lib, case, six):
    pr.check_solve(capture(case, six), six, case.radius, verbose="eta %s %d-DoF" % (case.name, 6 if six else 4))


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_model_and_candidate(gpu_lib, case, six):
    er.check_model_and_candidate(capture(case, six), six)


# ---------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_second_step_is_bit_identical(gpu_lib, case, six):
    same_bits(capture(case, six), _step(case, six))


# ---------------------------------------------------------------- 3. the same constraint through both doors
def _loops_as_callers(spec, info):
    return [dict(a=old, b=k, t=rt, q=rq, yaw=ry, info=info, loss=er.LOSS_HUBER, scale=0.1) for k, (old, rt, rq, ry) in sorted(spec.loops.items())]


def _without_loops(spec):
    bare = copy.deepcopy(spec)
    bare.loops = {}
    return bare


def _parity(ga, gb, sa, sb):
    assert sa["iterations"] == sb["iterations"] and sa["termination"] == sb["termination"] and sa["successful"] == sb["successful"], (sa, sb)
    assert abs(sa["initial_cost"] - sb["initial_cost"]) <= 1e-9 * max(1.0, sb["initial_cost"])
    assert abs(sa["final_cost"] - sb["final_cost"]) <= 1e-9 * max(1.0, sb["initial_cost"])
    (Ta, Qa), (Tb, Qb) = ga.poses(), gb.poses()
    sign = np.sign(np.sum(Qa * Qb, axis=1, keepdims=True))
    assert np.max(np.abs(Ta - Tb)) < 1e-7 and np.max(np.abs(Qa * sign - Qb)) < 1e-7


REGIMES = {"dense": dict(n=41, laps=2, loop_every=5, cfg=None), "one_level": dict(n=160, laps=4, loop_every=8, cfg=(8, 0, 1, 8)),
           "two_level": dict(n=190, laps=2, loop_every=19, cfg=(8, 0, 2, 8))}


@pytest.mark.parametrize("six", [False, True])
@pytest.mark.parametrize("info", [None, ec.loop_weights_squared], ids=["null", "written_out"])
@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_both_doors(gpu_lib, regime, info, six):
    r = REGIMES[regime]
    spec = spg.make_pose_graph(n=r["n"], laps=r["laps"], loop_every=r["loop_every"], seed=31)
    ga, gb = PoseGraph(0, six_dof=six), PoseGraph(0, six_dof=six)
    for g in (ga, gb):
        if r["cfg"]:
            g.set_partition(r["cfg"][0], r["cfg"][1])
            g.set_levels(r["cfg"][2], r["cfg"][3])
    earliest, cur = spg.feed(ga, spec)
    er.feed(gb, _without_loops(spec), _loops_as_callers(spec, info))
    sa, sb = ga.optimize(earliest, cur), gb.optimize(earliest, cur)
    pa, pb = ga.partition(), gb.partition()
    assert (pa["pieces"], pa["level2_pieces"], pa["separators"]) == (pb["pieces"], pb["level2_pieces"], pb["separators"])
    if regime == "dense":
        assert pa["pieces"] == 0
    elif regime == "one_level":
        assert pa["pieces"] >= 2 and pa["level2_pieces"] == 0
    else:
        assert pa["level2_pieces"] >= 2
    assert sa["iterations"] >= 2 and sa["final_cost"] < sa["initial_cost"]
    _parity(ga, gb, sa, sb)
    ga.close(); gb.close()


@pytest.mark.parametrize("six", [False, True])
def test_both_doors_incremental(gpu_lib, six):
    """three optimisations as the keyframes arrive, the drift handed over to the keyframes behind each"""
    spec = spg.make_pose_graph(n=120, laps=3, loop_every=13, seed=33)
    ga, gb = PoseGraph(0, six_dof=six), PoseGraph(0, six_dof=six)
    earliest, runs = None, 0
    for k in range(spec.n):
        ga.add_keyframe(k, 1, spec.t_svin[k], spec.q_svin[k], spec.loops.get(k))
        gb.add_keyframe(k, 1, spec.t_svin[k], spec.q_svin[k], None)
        if k in spec.loops:
            old, rt, rq, ry = spec.loops[k]
            gb.add_edge(old, k, rt, rq, ry, None, er.LOSS_HUBER, 0.1)
            earliest = old if earliest is None else min(earliest, old)
            if runs < 3 and k >= 60:
                sa, sb = ga.optimize(earliest, k), gb.optimize(earliest, k)
                _parity(ga, gb, sa, sb)
                ya, ra, ta = ga.drift()
                yb, rb, tb = gb.drift()
                assert abs(ya - yb) < 1e-6 and np.max(np.abs(ra - rb)) < 1e-8 and np.max(np.abs(ta - tb)) < 1e-6
                runs += 1
    assert runs == 3
    _parity(ga, gb, sa, sb)    # the keyframes behind the last optimisation carry the same drift
    ga.close(); gb.close()


# ---------------------------------------------------------------- 4. whole-run properties
def _states_after(g, case, problem, six):
    T, Q = g.poses()
    lo, hi = case.earliest, case.cur + 1
    return cr.states_from_poses(problem, T[lo:hi], Q[lo:hi], six, pc._r2ypr)


@pytest.mark.parametrize("name,six", [("losses", False), ("losses", True), ("cover5", False), ("level2_6", True), ("constants_6", True)])
def test_summary_costs_equal_the_numpy_cost(gpu_lib, name, six):
    case = BY_NAME[name]
    g = handle(case, six)
    cap = g.debug_step(case.earliest, case.cur, case.radius)
    s = g.optimize(case.earliest, case.cur)
    c0 = er.numpy_cost(cap, cap, six)
    c1 = er.numpy_cost(cap, _states_after(g, case, cap, six), six)
    print("%s %d-DoF: initial %.12g (numpy %.12g) final %.12g (numpy %.12g)" % (name, 6 if six else 4, s["initial_cost"], c0, s["final_cost"], c1))
    assert abs(s["initial_cost"] - c0) <= 1e-10 * c0
    assert abs(s["final_cost"] - c1) <= 1e-10 * c1
    assert s["final_cost"] < s["initial_cost"]
    g.close()


def _two_sessions(six):
    """session 2 (sequence 2) is the generating trajectory seen in another frame: turned about the vertical and shifted.  Its
    sequential edges hold in any frame, so a closure into session 1 decides where it lands; with noise-free closures the generating
    poses have zero cost."""
    spec = spg.make_pose_graph(n=60, laps=2, loop_every=10 ** 6, seed=35, drift_yaw_deg=0.0, drift_t=0.0)
    spec.sequence[30:] = 2
    Rz, sh = spg.ypr2R([8.0, 0.0, 0.0]), np.array([1.5, -1.0, 0.3])
    for k in range(30, 60):
        spec.t_svin[k] = Rz @ spec.t_true[k] + sh
        spec.q_svin[k] = spg.R2q(Rz @ spec.R_true[k])
    t, q, y = er.measure(spec, 10, 45, noise_t=0.0, noise_deg=0.0)
    spec.loops = {45: (10, t, q, y)}
    return spec


def _error_to_truth(g, spec):
    T, _ = g.poses()
    return float(np.max(np.abs(T - spec.t_true)))


@pytest.mark.parametrize("six", [False, True])
def test_second_closure_and_outlier(gpu_lib, six):
    spec = _two_sessions(six)
    second = er.caller_edge(spec, 20, 45, info=ec.dense_info, noise_t=0.0, noise_deg=0.0)
    g = PoseGraph(0, six_dof=six, max_iterations=50)
    earliest, cur, _ = er.feed(g, spec, [second])
    assert _error_to_truth(g, spec) > 1.0
    s = g.optimize(0, cur)
    assert s["final_cost"] < 1e-9 * s["initial_cost"], s
    assert _error_to_truth(g, spec) < 1e-6
    g.close()
    # a third closure that is grossly wrong: two metres and thirty degrees off
    errs = {}
    for kind in (er.LOSS_NONE, er.LOSS_CAUCHY):
        bad = er.caller_edge(spec, 25, 50, info=None, loss=kind, scale=0.5, noise_t=0.0, noise_deg=0.0, dt=(2.0, -1.0, 0.5), dyaw=30.0)
        bad["q"] = spg.R2q(spg.q2R(bad["q"]) @ spg.ypr2R([30.0, 0.0, 0.0]))
        g = PoseGraph(0, six_dof=six, max_iterations=50)
        er.feed(g, spec, [second, bad])
        g.optimize(0, cur)
        errs[kind] = _error_to_truth(g, spec)
        g.close()
    print("%d-DoF: error to the generating poses with the outlier under NONE %.3e, under Cauchy(0.5) %.3e" % (6 if six else 4, errs[0], errs[1]))
    assert errs[er.LOSS_CAUCHY] < errs[er.LOSS_NONE]


# ---------------------------------------------------------------- 5. remove_edge
@pytest.mark.parametrize("six", [False, True])
def test_remove_edge_restores_the_bare_graph(gpu_lib, six):
    base = pc.Case("bare", pc._graph(61, [(30, 0), (44, 9), (58, 21)], 103), piece=8, dense=0, levels=1)
    case = BY_NAME["cover5"]
    bare, g = PoseGraph(0, six_dof=six), PoseGraph(0, six_dof=six)
    for h in (bare, g):
        base.configure(h)
        spg.feed(h, base.spec)
    ids = [g.add_edge(ce["a"] % 61, ce["b"] % 61, ce["t"], ce["q"], ce["yaw"], er.info_of(ce, six), ce["loss"], ce["scale"]) for ce in case.callers]
    assert ids == list(range(1, len(ids) + 1)) and g.num_edges() == len(ids)
    with_edges = g.debug_step(0, 60, 1e4)
    assert np.sum(with_edges["ekind"] == 2) == len(ids)
    g.remove_edge(ids[1])
    again = g.add_edge(5, 50, np.zeros(3), np.array([0.0, 0, 0, 1]), 0.0, None, 0, 1.0)
    assert again == len(ids) + 1, "an edge id was reused"
    for i in ids[:1] + ids[2:] + [again]:
        g.remove_edge(i)
    assert g.num_edges() == 0
    a, b = bare.debug_step(0, 60, 1e4), g.debug_step(0, 60, 1e4)
    same_bits(a, b)
    assert np.array_equal(a["ea"], b["ea"]) and np.all(b["ekind"] < 2)
    sa, sb = bare.optimize(0, 60), g.optimize(0, 60)
    assert all(sa[k] == sb[k] for k in ("initial_cost", "final_cost", "iterations", "termination", "successful"))
    assert np.array_equal(bare.poses()[0], g.poses()[0]) and np.array_equal(bare.poses()[1], g.poses()[1])
    bare.close(); g.close()


def test_get_edge_returns_what_was_given(gpu_lib):
    for six in (False, True):
        g = PoseGraph(0, six_dof=six)
        spg.feed(g, BY_NAME["cover5"].spec)
        info = ec.dense_info(six)
        i = g.add_edge(7, 3, [0.1, 0.2, 0.3], [0.0, 0.0, np.sin(0.1), np.cos(0.1)], 11.5, info, er.LOSS_CAUCHY, 0.7)
        e = g.get_edge(i)
        assert (e["index_a"], e["index_b"], e["loss"], e["loss_scale"]) == (7, 3, er.LOSS_CAUCHY, 0.7)
        assert np.array_equal(e["rel_t"], [0.1, 0.2, 0.3]) and np.array_equal(e["information"], info)
        assert e["rel_yaw_deg"] == (0.0 if six else 11.5)
        j = g.add_edge(3, 9, [0.0, 0, 0], [0.0, 0, 0, 1], 0.0, None, er.LOSS_NONE, -3.0)      # the scale of NONE is ignored
        assert np.array_equal(g.get_edge(j)["information"], ec.loop_weights_squared(six))
        g.close()


# ---------------------------------------------------------------- 6. covariances
@pytest.mark.parametrize("name,six", [("losses", False), ("cover5", True), ("shared4_band_4", False), ("shared3_sep_6", True),
                                      ("level2_4", False), ("level2_6", True), ("constants_6", True), ("constants_4", False)])
def test_covariance_columns(gpu_lib, name, six):
    """(two_sequences is not here: its blocks of five are not all tied to the constant keyframe, J^T J is singular by construction)"""
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
    g.close()


@pytest.mark.parametrize("six", [False, True])
def test_keyframe_held_only_by_a_caller_edge(gpu_lib, six):
    """the last keyframe opens a sequence of its own: no sequential edge, no loop"""
    spec = pc._graph(41, [(20, 0), (33, 6)], 183)
    spec.sequence[40] = 3
    case = ec.EdgeCase(name="held", spec=spec, callers=[er.caller_edge(spec, 15, 40, info=ec.dense_info, seed=290)])
    g = handle(case, six)
    f0 = g.covariance_counters()["factorisations"]
    cap = g.debug_step(0, 40, 1e4)
    deg = np.bincount(np.concatenate([cap["ea"], cap["eb"]]), minlength=41)
    assert deg[40] == 1 and cap["ekind"][-1] == 2
    A, _ = pr.system(cap["Ja"], cap["Jb"], cap["res"], cap["scale"], cap, six, np.inf)
    blocks = g.covariance_blocks(0, 40, cr.column_pairs(41, [40]))
    cr.check_columns(A, cap["scale"], cap, six, [40], cr.columns_from_blocks(cap, six, [40], blocks))
    assert g.covariance_counters()["factorisations"] == f0 + 1
    g.covariance_blocks(0, 40, [(40, 40)])
    assert g.covariance_counters()["factorisations"] == f0 + 1, "the factor was not kept"
    extra = g.add_edge(3, 30, np.zeros(3), np.array([0.0, 0, 0, 1]), 0.0, None, 0, 1.0)
    g.covariance_blocks(0, 40, [(40, 40)])
    assert g.covariance_counters()["factorisations"] == f0 + 2, "add_edge kept the factor"
    g.remove_edge(extra)
    kept = g.covariance_blocks(0, 40, [(40, 40)])
    assert g.covariance_counters()["factorisations"] == f0 + 3, "remove_edge kept the factor"
    assert np.array_equal(kept[0], blocks[40])
    g.remove_edge(1)
    from svin_amd.posegraph import SingularError
    with pytest.raises(SingularError, match=r"keyframe 40\b"):
        g.covariance_blocks(0, 40, [(40, 40)])
    g.close()


# ---------------------------------------------------------------- 7. errors
@pytest.mark.parametrize("six", [False, True])
def test_refusals_change_nothing(gpu_lib, six):
    from svin_amd.posegraph import _lib
    L = _lib()
    D = 6 if six else 4
    g = PoseGraph(0, six_dof=six)
    spg.feed(g, BY_NAME["cover5"].spec)
    keep = g.add_edge(2, 9, np.zeros(3), np.array([0.0, 0, 0, 1]), 0.0, None, 0, 1.0)
    pd = C.POINTER(C.c_double)
    t, q = np.array([0.1, 0.2, 0.3]), np.array([0.0, 0.0, 0.0, 1.0])
    good = ec.dense_info(six)

    def add(h=None, a=3, b=8, t_=t, q_=q, yaw=1.0, info=good, kind=er.LOSS_HUBER, scale=0.5):
        p = lambda x: None if x is None else np.ascontiguousarray(x, np.float64).ctypes.data_as(pd)   # noqa: E731
        return L.svin_pg_add_edge(g.h if h is None else h, a, b, p(t_), p(q_), yaw, p(info), kind, scale)
    asym = good.copy(); asym[0, 1] = np.nextafter(asym[0, 1], np.inf)
    nan_info = good.copy(); nan_info[1, 1] = np.nan
    semi = np.zeros((D, D)); semi[:2, :2] = 1.0; semi[2:, 2:] = np.eye(D - 2)
    indef = np.diag([1.0, -1.0] + [1.0] * (D - 2))
    refusals = [(dict(t_=None), -1), (dict(a=5, b=5), -1), (dict(t_=np.array([0.0, np.inf, 0.0])), -1),
                (dict(kind=3), -1), (dict(kind=-1), -1), (dict(scale=0.0), -1), (dict(scale=-1.0), -1), (dict(scale=np.nan), -1),
                (dict(scale=np.inf), -1), (dict(kind=er.LOSS_CAUCHY, scale=0.0), -1), (dict(info=asym), -1), (dict(info=nan_info), -1),
                (dict(info=semi), -1), (dict(info=indef), -1), (dict(a=3, b=1000), -2), (dict(a=-4, b=3), -2)]
    if six:
        refusals += [(dict(q_=None), -1), (dict(q_=np.array([0.0, np.nan, 0.0, 1.0])), -1)]
    else:
        refusals += [(dict(yaw=np.nan), -1)]
        assert add(q_=None) == keep + 1 and L.svin_pg_remove_edge(g.h, keep + 1) == 1      # rel_q may be NULL in 4-DoF
    for kw, want in refusals:
        assert add(**kw) == want, (kw, want)
        assert L.svin_pg_last_error(), kw
        assert g.num_edges() == 1
    assert L.svin_pg_add_edge(None, 3, 8, t.ctypes.data_as(pd), q.ctypes.data_as(pd), 0.0, None, 0, 1.0) == -1
    assert add(kind=er.LOSS_NONE, scale=np.nan) > keep and g.num_edges() == 2      # the scale of NONE is ignored
    # remove / get: unknown ids, sentinel-filled outputs
    assert L.svin_pg_remove_edge(g.h, 999) == -2 and L.svin_pg_remove_edge(g.h, 0) == -2 and L.svin_pg_remove_edge(None, 1) == -1
    assert L.svin_pg_num_edges(None) == -1 and g.num_edges() == 2
    ia, ib, lk = C.c_int(-77), C.c_int(-77), C.c_int(-77)
    ot, oq, oy, oi, ol = np.full(3, -7.0), np.full(4, -7.0), np.full(1, -7.0), np.full(D * D, -7.0), np.full(1, -7.0)
    p = lambda x: x.ctypes.data_as(pd)   # noqa: E731
    for h, eid, want in ((g.h, 999, -2), (None, keep, -1)):
        assert L.svin_pg_get_edge(h, eid, C.byref(ia), C.byref(ib), p(ot), p(oq), p(oy), p(oi), C.byref(lk), p(ol)) == want
        assert (ia.value, ib.value, lk.value) == (-77, -77, -77)
        assert all(np.all(x == -7.0) for x in (ot, oq, oy, oi, ol))
    assert L.svin_pg_get_edge(g.h, keep, None, None, None, None, None, None, None, None) == 1
    # the handle still optimises, and the first edge is still what it was
    assert g.get_edge(keep)["index_b"] == 9
    assert g.optimize(0, 70)["termination"] in (0, 1)
    g.close()
