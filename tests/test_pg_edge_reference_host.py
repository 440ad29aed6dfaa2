"""CPU tests of the long-double reference of caller-given pose-graph edges (tests/helpers/pg_edge_reference.py), of the comparisons
tests/test_gpu_posegraph_edges.py judges the device with, and of its case graphs (tests/helpers/pg_edge_cases.py):

  * a plain float64 evaluation of the same expressions (class V in float64, and a numpy matrix product standing where the
    device's unrolled one stands) stays inside every bound on every case;
  * the reference's cost equals an independent plain-numpy restatement to 1e-10 relative;
  * the Jacobians after the factor agree with central differences through the manifold's Plus;
  * six planted defects are rejected, each by the assertion meant for it;
  * every case reaches the edge it was built for, by the restated construction and symbolic step.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pg_edge_cases as ec  # noqa: E402
import pg_edge_reference as er  # noqa: E402
import pg_reference as pr  # noqa: E402

pytestmark = pytest.mark.skipif(not pr.have_long_double(), reason="np.longdouble is not an extended type on this platform")

LD = pr.LD
CASES = ec.build_cases()
BY_NAME = {c.name: c for c in CASES}
CASE_DOFS = [(c, six) for c in CASES for six in c.dofs]
IDS = ["%s-%ddof" % (c.name, 6 if six else 4) for c, six in CASE_DOFS]


def f64(x):
    return np.asarray(x, np.float64)


@functools.lru_cache(maxsize=None)
def problem(name, six):
    return BY_NAME[name].problem(six)


def evaluate(P, six, defect=None):
    """a float64 implementation standing where the device stands: u, Ju from a float64 run of the unit-weight expressions, then
    numpy products for the factor and the loss written out.  defect plants one of the mistakes the comparison has to reject."""
    R = 6 if six else 4
    ne = len(P["ea"])
    unit, caller = er._unit_problem(P)
    with pr.evaluate_in(np.float64):
        E = pr.edges(unit, P, six)
    res, Ja, Jb = f64(E["res"].v).copy(), f64(E["Ja"].v).copy(), f64(E["Jb"].v).copy()
    cost = f64(E["cost_e"].v).copy()
    S = f64(P["einfo"]).reshape(ne, R, R)
    kl = f64(P["eloss"]).reshape(ne, 2)
    for e in np.where(caller)[0]:
        M = S[e].copy()
        u = res[e].copy()
        if defect == "lower":                 # L used where L^T belongs
            M = M.T.copy()
        elif defect == "information":         # the information itself used where its factor belongs
            M = M.T @ M
        elif defect == "drop":                # one off-diagonal entry of S dropped
            k, j = np.unravel_index(np.argmax(np.abs(np.triu(M, 1))), M.shape)
            M[k, j] = 0.0
        r, A, B = M @ u, M @ Ja[e], M @ Jb[e]
        s = float(u @ u) if defect == "loss_on_u" else float(r @ r)     # the loss taken on |u|^2 instead of |r|^2
        kind, a = int(kl[e, 0]), kl[e, 1]
        sc, c = 1.0, 0.5 * s
        if kind == er.LOSS_HUBER and s > a * a:
            c, sc = 0.5 * (2 * a * np.sqrt(s) - a * a), np.sqrt(a / np.sqrt(s))
        elif kind == er.LOSS_CAUCHY:
            b = a if defect == "cauchy_a" else a * a                    # rho' with a where a^2 belongs
            c, sc = 0.5 * (a * a) * np.log(1.0 + s / (a * a)), np.sqrt(1.0 / (1.0 + s / b))
        res[e], Ja[e], Jb[e], cost[e] = sc * r, sc * A, sc * B, c
    cap = dict(P)
    cap.update(res=res.reshape(-1), Ja=Ja.reshape(-1), Jb=Jb.reshape(-1), cost=float(np.sum(cost)))
    return cap


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_cases_reach_their_edges(case, six):
    P = problem(case.name, six)
    part = case.partition(P, six)
    case.reach(part, P, six)
    assert np.sum(P["eloop"] == 2) >= 1 and len(P["off"]) <= 190 and 6 * len(P["off"]) <= 1200


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_float64_evaluation_stays_inside_every_bound(case, six):
    P = problem(case.name, six)
    E = er.edges(P, P, six)
    with pr.evaluate_in(np.float64):
        F = er.edges(P, P, six)
    for key in ("res", "Ja", "Jb", "cost"):
        pr.assert_close(key, f64(F[key].v).reshape(-1), np.asarray(E[key].v).reshape(-1), np.asarray(E[key].tol()).reshape(-1))
    er.check_evaluation(evaluate(P, six), six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_cost_matches_the_numpy_restatement(case, six):
    P = problem(case.name, six)
    c_ref, c_np = float(er.edges(P, P, six)["cost"].v), er.numpy_cost(P, P, six)
    assert abs(c_ref - c_np) <= 1e-10 * c_np, (c_ref, c_np)


def _plus(P, node, comp, h, six):
    """states with the manifold's Plus applied to one tangent component of one keyframe"""
    st = dict(yaw=f64(P["yaw"]).copy(), t=f64(P["t"]).copy(), q=f64(P["q"]).copy())
    if not six:
        if comp == 0:
            st["yaw"][node] += h
        else:
            st["t"][3 * node + comp - 1] += h
    elif comp < 3:
        st["t"][3 * node + comp] += h
    else:
        d = np.zeros(3)
        d[comp - 3] = h
        dq = np.concatenate([np.sin(abs(h)) * d / abs(h), [np.cos(h)]])
        q = st["q"][4 * node:4 * node + 4]
        st["q"][4 * node:4 * node + 4] = [dq[3] * q[0] + dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1], dq[3] * q[1] + dq[1] * q[3] + dq[2] * q[0] - dq[0] * q[2],
                                          dq[3] * q[2] + dq[2] * q[3] + dq[0] * q[1] - dq[1] * q[0], dq[3] * q[3] - dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2]]
    return st


def _one_edge(P, e, six):
    """the problem of edge e alone (its two keyframes renumbered 0, 1)"""
    a, b = int(P["ea"][e]), int(P["eb"][e])
    R = 6 if six else 4
    Q = dict(ea=np.array([0]), eb=np.array([1]), eloop=P["eloop"][e:e + 1], off=np.array([0, R]), ekind=P["ekind"][e:e + 1])
    for k, w in (("et", 3), ("eyaw", 1), ("epitch", 1), ("eroll", 1), ("eq", 4), ("esq", 6), ("eloss", 2), ("einfo", R * R)):
        Q[k] = P[k][w * e:w * e + w]
    for k, w in (("yaw", 1), ("pitch", 1), ("roll", 1), ("t", 3), ("q", 4)):
        Q[k] = np.concatenate([P[k][w * a:w * a + w], P[k][w * b:w * b + w]])
    return Q


@pytest.mark.parametrize("name,six", [("losses", False), ("losses", True), ("positions_4", False), ("positions_6", True)])
def test_jacobians_match_central_differences(name, six):
    """r0 = S u against (r0(Plus(x, h e_c)) - r0(Plus(x, -h e_c))) / 2h, h = 1e-5, the states rounded to float64 after Plus: the
    rounding of a state of size |x| <= 10 (metres) / 180 (degrees) moves a residual by |S Ju| eps |x|, i.e. the quotient by up to
    |S Ju| 180 eps / h = 4e-9 |S Ju|; the truncation h^2 |r'''| / 6 is below 1e-10 |S|.  Bar: 1e-7 (max |J0| + max |S|)."""
    P = problem(name, six)
    D = 6 if six else 4
    h = 1e-5
    callers = np.where(P["eloop"] == 2)[0]
    for e in callers[:12]:
        Q = _one_edge(P, e, six)
        E = er.edges(Q, Q, six)
        bar = 1e-7 * (float(np.max(np.abs(E["Ja0"].v))) + float(np.max(np.abs(E["Jb0"].v))) + float(np.max(np.abs(Q["einfo"]))))
        for node, nm in ((0, "Ja0"), (1, "Jb0")):
            for c in range(D):
                rp = er.edges(Q, _plus(Q, node, c, h, six), six)["r0"].v[0]
                rm = er.edges(Q, _plus(Q, node, c, -h, six), six)["r0"].v[0]
                num = np.asarray((rp - rm) / (2 * LD(h)), np.float64)
                ana = f64(E[nm].v)[0, :, c]
                assert np.max(np.abs(num - ana)) <= bar, (int(e), nm, c, num, ana)


# ---------------------------------------------------------------- planted defects
def _ill_conditioned(six):
    """the `losses` case with a condition-1e6 information on its dense edges"""
    case = BY_NAME["losses"]
    callers = [dict(c) for c in case.callers]
    for c in callers:
        if c["info"] is ec.dense_info:
            c["info"] = lambda six_, f=ec.dense_info: f(six_, seed=9, cond=1e6)
    return er.local_problem(case.spec, six, case.earliest, case.cur, callers)


@pytest.mark.parametrize("six", [False, True])
@pytest.mark.parametrize("defect", ["lower", "information", "loss_on_u", "cauchy_a", "drop"])
def test_planted_evaluation_defects_are_rejected(defect, six):
    P = _ill_conditioned(six) if defect == "drop" else problem("losses", six)
    if defect == "drop":
        S = P["einfo"].reshape(-1, 6 if six else 4, 6 if six else 4)
        assert max(np.linalg.cond(x.T @ x) for x in S[P["eloop"] == 2]) > 1e5
    er.check_evaluation(evaluate(P, six), six)                      # the same evaluator without the defect passes
    with pytest.raises(AssertionError, match=r"^res: "):
        er.check_evaluation(evaluate(P, six, defect), six)
    # the cost alone sees the defects that touch it, when the stored arrays are the right ones
    if defect in ("loss_on_u", "information"):
        good, bad = evaluate(P, six), evaluate(P, six, defect)
        good["cost"] = bad["cost"]
        with pytest.raises(AssertionError, match=r"^cost: "):
            er.check_evaluation(good, six)


@pytest.mark.parametrize("name,six", [("shared3_band_4", False), ("shared3_sep_6", True), ("shared4_coupling_4", False)])
def test_a_shared_block_summing_too_few_edges_is_rejected(name, six):
    """stage 3 judges the assembly: a system whose three- (four-) edge block lacks one edge's term gives a y that the backward-error
    assertion of pg_reference.check_solve refuses"""
    case = BY_NAME[name]
    P = problem(name, six)
    D = 6 if six else 4
    cap = evaluate(P, six)
    with pr.evaluate_in(np.float64):
        N = pr.node_quantities(cap["res"], cap["Ja"], cap["Jb"], cap, six)
    cap["scale"] = f64(N["scale"][0])
    A, b = pr.system(cap["Ja"], cap["Jb"], cap["res"], cap["scale"], cap, six, case.radius)
    cap["y"] = pr.lapack_solve(A, b)
    pr.check_solve(cap, six, case.radius)
    (lo, hi), es = next(iter(er.shared_pairs(P).items()))
    assert len(es) >= 3
    e = es[-1]
    a, bb = int(P["ea"][e]), int(P["eb"][e])
    oa, ob = P["off"][a], P["off"][bb]
    s = np.asarray(cap["scale"], LD)
    blk = np.asarray(cap["Jb"], LD).reshape(-1, D, D)[e].T @ np.asarray(cap["Ja"], LD).reshape(-1, D, D)[e]
    blk = blk * s[ob:ob + D, None] * s[None, oa:oa + D]
    Abad = A.copy()
    Abad[ob:ob + D, oa:oa + D] -= blk
    Abad[oa:oa + D, ob:ob + D] -= blk.T
    cap["y"] = pr.lapack_solve(Abad, b)
    with pytest.raises(AssertionError, match="backward error"):
        pr.check_solve(cap, six, case.radius)
