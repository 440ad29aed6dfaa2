"""CPU tests of the long-double pose-graph reference (tests/helpers/pg_reference.py), of the comparison functions
tests/test_gpu_posegraph_stages.py judges the device with, and of the case graphs (tests/helpers/pg_cases.py):

  * the reference's edges against tests/golden/pg.npz, against 40-digit mpmath central differences through the same Plus and
    against the oracle's orc_pg_eval_edge; its normal equations against the oracle's linearisation;
  * the comparisons pass on the reference's own results rounded to float64 and reject seven planted defects, each by the
    assertion meant for it;
  * a correct float64 solver (LAPACK's LU, and a float64 Cholesky as a second one) meets the solve's bars on every case;
  * every case reaches the edge it was built for, by the restated symbolic step.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pg_cases as pc  # noqa: E402
import pg_reference as pr  # noqa: E402

from svin_amd import synthetic_pg as spg  # noqa: E402

pytestmark = pytest.mark.skipif(not pr.have_long_double(), reason="np.longdouble is not an extended type on this platform")

LD = pr.LD
CASES = pc.build_cases()
CASE_DOFS = [(c, six) for c in CASES for six in c.dofs]
IDS = ["%s-%ddof" % (c.name, 6 if six else 4) for c, six in CASE_DOFS]
BY_NAME = {c.name: c for c in CASES}


def f64(x):
    return np.asarray(x, np.float64)


@functools.lru_cache(maxsize=None)
def reference_capture(name, six):
    """what debug_step would return if the device computed every stage exactly and rounded once: the reference's own results
    in float64, each stage fed with the rounded records of the stage before (as the device's stages are)"""
    case = BY_NAME[name]
    D = 6 if six else 4
    cap = dict(case.problem(six))
    part = case.partition(cap, six)
    cap.update({k: part[k] for k in pr.PARTITION_KEYS})
    E = pr.edges(cap, cap, six)
    cap.update(res=f64(E["res"].v).reshape(-1), Ja=f64(E["Ja"].v).reshape(-1), Jb=f64(E["Jb"].v).reshape(-1), cost=float(E["cost"].v))
    N = pr.node_quantities(cap["res"], cap["Ja"], cap["Jb"], cap, six)
    cap.update(g=f64(N["g"][0]), colsq=f64(N["colsq"][0]), scale=f64(N["scale"][0]), nodeBlk=f64(N["blk"][0]).reshape(-1),
               gradmax=float(N["gradmax"][0]))
    A, b = pr.system(cap["Ja"], cap["Jb"], cap["res"], cap["scale"], cap, six, case.radius)
    cap["y"] = f64(pr.solve(A, b))
    cap["cholFail"] = 0
    M = pr.model_and_candidate(cap["y"], cap["scale"], cap["res"], cap["Ja"], cap["Jb"], cap, cap, six)
    nn = len(cap["off"])
    cap.update(model=float(M["model"].v), step2=float(M["step2"].v), x2=float(M["x2"].v), tC=f64(M["tC"].v).reshape(-1),
               yawC=f64(M["yawC"].v) if not six else f64(cap["yaw"]), qC=f64(M["qC"].v).reshape(-1) if six else f64(cap["q"]))
    cand = dict(yaw=cap["yawC"], t=cap["tC"], q=cap["qC"])
    cap["costC"] = float(pr.edges(cap, cand, six)["cost"].v)
    return dict(cap=cap, part=part, A=A, b=b, E=E, D=D, nn=nn)


def fresh(name, six):
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in reference_capture(name, six)["cap"].items()}


def float64_capture(name, six):
    """the same step by a plain float64 evaluation of the same expressions (numpy, this CPU's libm, a float64 Cholesky): a correct
    float64 implementation standing where the device will stand"""
    case = BY_NAME[name]
    cap = fresh(name, six)
    with pr.evaluate_in(np.float64):
        E = pr.edges(cap, cap, six)
        cap.update(res=f64(E["res"].v).reshape(-1), Ja=f64(E["Ja"].v).reshape(-1), Jb=f64(E["Jb"].v).reshape(-1), cost=float(E["cost"].v))
        N = pr.node_quantities(cap["res"], cap["Ja"], cap["Jb"], cap, six)
        cap.update(g=f64(N["g"][0]), colsq=f64(N["colsq"][0]), scale=f64(N["scale"][0]), nodeBlk=f64(N["blk"][0]).reshape(-1),
                   gradmax=float(N["gradmax"][0]))
    A, b = pr.system(cap["Ja"], cap["Jb"], cap["res"], cap["scale"], cap, six, case.radius)
    L = np.linalg.cholesky(f64(A))
    cap["y"] = np.linalg.solve(L.T, np.linalg.solve(L, f64(b)))
    with pr.evaluate_in(np.float64):
        M = pr.model_and_candidate(cap["y"], cap["scale"], cap["res"], cap["Ja"], cap["Jb"], cap, cap, six)
        cap.update(model=float(M["model"].v), step2=float(M["step2"].v), x2=float(M["x2"].v), tC=f64(M["tC"].v).reshape(-1))
        if six:
            cap["qC"] = f64(M["qC"].v).reshape(-1)
        else:
            cap["yawC"] = f64(M["yawC"].v)
        cap["costC"] = float(pr.edges(cap, dict(yaw=cap["yawC"], t=cap["tC"], q=cap["qC"]), six)["cost"].v)
    return cap


# ---------------------------------------------------------------- the reference against mpmath, the fixture and the oracle
def _golden_spec():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pg.npz"))
    loops = {int(k): (int(o), g["loop_t"][i], g["loop_q"][i], float(g["loop_yaw"][i])) for i, (k, o) in enumerate(zip(g["loop_cur"], g["loop_old"]))}
    n = len(g["t_svin"])
    return g, spg.PoseGraphSpec(n, None, None, g["t_svin"], g["q_svin"], loops, np.ones(n, int))


def test_edges_match_the_mpmath_fixture():
    """residual costs at the SVIn poses (both DoF) and at the fixture's perturbed 4-DoF state, and the pre-loss residuals and
    Jacobians of its three 4-DoF edges; the bound is the reference's own plus one float64 rounding of the stored number"""
    g, spec = _golden_spec()
    for six, key in ((False, "cost4_initial"), (True, "cost6_initial")):
        P = pc.local_problem(spec, six, 0, spec.n - 1)
        E = pr.edges(P, P, six)
        assert abs(float(E["cost"].v - LD(g[key]))) <= float(E["cost"].tol()) + pr.EPS64 * float(g[key])
    # the perturbed 4-DoF state through Plus (yaw wrapped, translation added).  The fixture's state is exact at 40 digits, this
    # one is rounded to float64 once more: a residual moves by at most |J| eps |x| (row sums of the Jacobian, |yaw| <= 180 degrees,
    # |t| <= 4 m), a Jacobian entry by the second derivative (pi / 180 per degree at most) times the same eps |x|
    P = pc.local_problem(spec, False, 0, spec.n - 1)
    d4 = g["d4"]
    st = dict(yaw=np.array([float(pr.wrap(pr.V(y + d)).v) for y, d in zip(P["yaw"], d4[:, 0])]), t=(P["t"].reshape(-1, 3) + d4[:, 1:]).reshape(-1))
    E = pr.edges(P, st, False)
    xmax = np.array([180.0, 4.0, 4.0, 4.0])
    found = 0
    for i in range(len(g["edge_a"])):
        for e in range(len(P["ea"])):
            if (P["ea"][e], P["eb"][e], P["eloop"][e]) == (int(g["edge_a"][i]), int(g["edge_b"][i]), int(g["edge_loop"][i])):
                found += 1
                Ja, Jb = np.abs(f64(E["Ja0"].v[e])), np.abs(f64(E["Jb0"].v[e]))
                moved_r = pr.EPS64 * ((Ja + Jb) @ xmax)
                moved_J = pr.EPS64 * float(pr.K_DEG) * np.max(Ja + Jb) * np.sum(xmax)
                pr.assert_close("fixture r", g["edge_r"][i], E["r0"].v[e], E["r0"].tol()[e] + moved_r + pr.EPS64 * np.abs(g["edge_r"][i]))
                pr.assert_close("fixture Ja", g["edge_Ja"][i], E["Ja0"].v[e], E["Ja0"].tol()[e] + moved_J + pr.EPS64 * Ja)
                pr.assert_close("fixture Jb", g["edge_Jb"][i], E["Jb0"].v[e], E["Jb0"].tol()[e] + moved_J + pr.EPS64 * Jb)
    assert found == len(g["edge_a"]) >= 3
    res = f64(E["res"].v)
    moved_cost = pr.EPS64 * float(np.sum(np.abs(res) * ((np.abs(f64(E["Ja"].v)) + np.abs(f64(E["Jb"].v))) @ xmax)))
    assert abs(float(E["cost"].v - LD(g["cost4_pert"]))) <= float(E["cost"].tol()) + moved_cost + pr.EPS64 * float(g["cost4_pert"])


def _mp_residual(mp, P, e, six, sa, sb):
    """pre-loss residual of edge e at mpmath states sa, sb = (yaw | q, t) of its two ends, straight from the functors"""
    m = mp.mpf
    d = [sb[1][i] - sa[1][i] for i in range(3)]
    et = [m(float(x)) for x in P["et"][3 * e:3 * e + 3]]
    if not six:
        y, p, r = [x / 180 * m(float(pr.PI64)) for x in (sa[0], m(float(P["epitch"][e])), m(float(P["eroll"][e])))]
        cy, sy, cp, sp, cr, sr = mp.cos(y), mp.sin(y), mp.cos(p), mp.sin(p), mp.cos(r), mp.sin(r)
        R = [[cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr], [sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr],
             [-sp, cp * sr, cp * cr]]
        out = [sum(R[j][k] * d[j] for j in range(3)) - et[k] for k in range(3)]
        a = sb[0] - sa[0] - m(float(P["eyaw"][e]))
        a = a - 360 if a > 180 else (a + 360 if a < -180 else a)
        return out + [a * (m(float(np.float64(0.1))) if P["eloop"][e] else 1)]

    def qm(a, b):
        return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]

    def cj(a):
        return [-a[0], -a[1], -a[2], a[3]]
    x, y, z, w = sa[0]
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    pab = [sum(R[j][k] * d[j] for j in range(3)) for k in range(3)]
    dq = qm([m(float(v)) for v in P["eq"][4 * e:4 * e + 4]], cj(qm(cj(sa[0]), sb[0])))
    si = [m(float(v)) for v in P["esq"][6 * e:6 * e + 6]]
    u = [pab[k] - et[k] for k in range(3)] + [2 * dq[k] for k in range(3)]
    return [si[k] * u[k] for k in range(6)]


def _mp_plus(mp, s, dv, six):
    if not six:
        a = s[0] + dv[0]
        a = a - 360 if a > 180 else (a + 360 if a < -180 else a)
        return (a, [s[1][i] + dv[1 + i] for i in range(3)])
    t = [s[1][i] + dv[i] for i in range(3)]
    nd = mp.sqrt(sum(v * v for v in dv[3:]))
    if nd == 0:
        return (s[0], t)
    k = mp.sin(nd) / nd
    a, b = [k * dv[3], k * dv[4], k * dv[5], mp.cos(nd)], s[0]
    q = [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
         a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]
    return (q, t)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_jacobians_match_mpmath_central_differences(case, six):
    """every loop edge (at most 6) and every 41st sequential edge of the case: the residual agrees with the 40-digit functor, the
    analytic Jacobian with central differences (h = 1e-12 at 40 digits: truncation h^2 |r'''| / 6 ~ 1e-22) through Plus"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    D = 6 if six else 4
    P = case.problem(six)
    E = reference_capture(case.name, six)["E"]
    loops = [e for e in range(len(P["ea"])) if P["eloop"][e]][:6]
    picked = loops + list(range(0, len(P["ea"]), 41))
    h = mp.mpf(10) ** -12

    def state(k):
        t = [mp.mpf(float(v)) for v in P["t"][3 * k:3 * k + 3]]
        return ([mp.mpf(float(v)) for v in P["q"][4 * k:4 * k + 4]], t) if six else (mp.mpf(float(P["yaw"][k])), t)
    for e in picked:
        a, b = int(P["ea"][e]), int(P["eb"][e])
        sa, sb = state(a), state(b)
        # 6-DoF: the analytic Jacobians are those of UNIT quaternions (a rotation R(q)); the stored ones are unit to a rounding,
        # and the true derivative of the functor differs by (|q|^2 - 1) times the entry's terms, at most 2 sqrt_info (|d|_1 + 1)
        unit = 0.0
        if six:
            nq = max(abs(float(np.sum(LD(1) * P[k][4 * i:4 * i + 4] ** 2) - 1)) for k, i in (("q", a), ("q", b), ("eq", e)))
            unit = 4 * (nq + pr.EPS64) * 2 * 100.0 * (float(np.sum(np.abs(P["t"][3 * b:3 * b + 3] - P["t"][3 * a:3 * a + 3]))) + 1)
        r = _mp_residual(mp, P, e, six, sa, sb)
        tol_r = E["r0"].tol()[e]
        assert all(abs(float(mp.mpf(float(E["r0"].v[e, k])) - r[k])) <= tol_r[k] + 1e-18 * (1 + abs(float(r[k]))) for k in range(D)), (e, "residual")
        for side, nm in ((0, "Ja0"), (1, "Jb0")):
            for c in range(D):
                dv = [mp.mpf(0)] * D
                dv[c] = h
                dm = [-v for v in dv]
                if side == 0:
                    rp, rm = _mp_residual(mp, P, e, six, _mp_plus(mp, sa, dv, six), sb), _mp_residual(mp, P, e, six, _mp_plus(mp, sa, dm, six), sb)
                else:
                    rp, rm = _mp_residual(mp, P, e, six, sa, _mp_plus(mp, sb, dv, six)), _mp_residual(mp, P, e, six, sa, _mp_plus(mp, sb, dm, six))
                for k in range(D):
                    num = float((rp[k] - rm[k]) / (2 * h))
                    ref, tol = float(E[nm].v[e, k, c]), E[nm].tol()[e, k, c]
                    # 1e-15 relative: the long double's own 64 bits against the 40 digits
                    assert abs(ref - num) <= tol + unit + 1e-15 * (1 + abs(num)), (e, nm, k, c, ref, num, tol)


def _oracle(case, six):
    from oracle import orc
    o = orc.OraclePoseGraph(six_dof=six)
    spg.feed(o, case.spec)
    nodes, nt, ne = o.build(case.earliest, case.cur)
    return o, nodes, nt, ne


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_edges_and_system_match_the_oracle(case, six):
    """orc_pg_eval_edge is one more float64 evaluation of the same expressions in another order: every entry of every edge has to
    sit inside the reference's bound (which thereby is tested on a float64 implementation before the device sees it); the
    oracle's J^T J and J^T r against the reference's, to the first-order bound |J|^T E + E^T |J| of the product"""
    rc = reference_capture(case.name, six)
    P, E, D = rc["cap"], rc["E"], rc["D"]
    o, nodes, nt, ne = _oracle(case, six)
    assert nodes == len(P["off"]) and ne == len(P["ea"]) and nt == D * int(np.sum(P["off"] >= 0))
    t = P["t"].reshape(-1, 3)
    for e in range(ne):
        a, b, lp, r, Ja, Jb = o.eval_edge(e)
        assert (a, b, int(lp)) == (P["ea"][e], P["eb"][e], P["eloop"][e])
        # The oracle builds its OWN measurements (R_a^T (t_b - t_a), yaw / pitch / roll by atan2, q_a^-1 q_b) in float64, as does
        # local_problem(): the two sets of data differ by roundings of quantities of size |t| (metres) and 180 (degrees, scaled
        # by pi / 180 in the rotation), weighted by sqrt_info.  32 eps of that is the allowance for the data; the expressions are
        # what this test compares (test_float64_evaluation_stays_inside_every_bound holds the bounds themselves)
        w = 100.0 if six else 1.0
        data = 32 * pr.EPS64 * w * (float(np.sum(np.abs(t[a])) + np.sum(np.abs(t[b]))) + 2.0 * np.pi)
        pr.assert_close("oracle r of edge %d" % e, r, E["r0"].v[e], E["r0"].tol()[e] + data)
        pr.assert_close("oracle Ja of edge %d" % e, Ja, E["Ja0"].v[e], E["Ja0"].tol()[e] + data)
        pr.assert_close("oracle Jb of edge %d" % e, Jb, E["Jb0"].v[e], E["Jb0"].tol()[e] + data)
    data_all = 32 * pr.EPS64 * (100.0 if six else 1.0) * (2 * float(np.max(np.sum(np.abs(t), axis=1))) + 2.0 * np.pi)
    assert abs(o.cost() - float(E["cost"].v)) <= float(E["cost"].tol()) + data_all * float(np.sum(np.abs(f64(E["res"].v))))
    r, J = o.linearize(ne * D, nt)
    H_ref, g_ref = pr.normal_matrix(P, E["Ja"].v, E["Jb"].v, E["res"].v, D)
    Je = f64(pr._dense_jacobian(P, E["Ja"].tol() + data_all, E["Jb"].tol() + data_all, D))
    aJ = f64(pr._dense_jacobian(P, E["Ja"].v, E["Jb"].v, D, absolute=True))
    rr, re = f64(np.abs(E["res"].v)).reshape(-1), E["res"].tol().reshape(-1) + data_all
    Jo, ro = f64(J), f64(r)
    tol_H = aJ.T @ Je + Je.T @ aJ + Je.T @ Je
    tol_g = aJ.T @ re + Je.T @ rr + Je.T @ re
    # (the oracle's products summed in float64 here: R * degree + 1 more roundings of the absolute sum)
    sum_H, sum_g = (6 * 12 + 1) * pr.EPS64 * (aJ.T @ aJ), (6 * 12 + 1) * pr.EPS64 * (aJ.T @ rr)
    pr.assert_close("J^T J", Jo.T @ Jo, H_ref, tol_H + sum_H)
    pr.assert_close("J^T r", Jo.T @ ro, g_ref, tol_g + sum_g)
    # and the reference's damped system is that J^T J scaled and damped (built from its rounded blocks: one more eps)
    s = np.asarray(P["scale"], LD)
    A = rc["A"]
    off_diag = ~np.eye(len(s), dtype=bool)
    pr.assert_close("A off the diagonal", f64(A)[off_diag], (H_ref * s[:, None] * s[None, :])[off_diag],
                    ((tol_H + 4 * pr.EPS64 * (aJ.T @ aJ)) * f64(s)[:, None] * f64(s)[None, :])[off_diag])


# ---------------------------------------------------------------- the comparisons: clean results pass, planted defects do not
@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_rounded_reference_passes_every_comparison(case, six):
    rc = reference_capture(case.name, six)
    cap = fresh(case.name, six)
    pr.check_partition(cap, rc["part"])
    pr.check_evaluation(cap, six)
    pr.check_node_pass(cap, six)
    eta_dev, eta_lap, kap, fwd = pr.check_solve(cap, six, case.radius, verbose=case.name)
    pr.check_model_and_candidate(cap, six)


@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_float64_evaluation_stays_inside_every_bound(case, six):
    """the derived bounds hold for a float64 implementation on this CPU, stage by stage, on every case"""
    cap = float64_capture(case.name, six)
    assert np.any(cap["res"] != reference_capture(case.name, six)["cap"]["res"])     # (it is not the rounded reference again)
    pr.check_evaluation(cap, six)
    pr.check_node_pass(cap, six)
    pr.check_solve(cap, six, case.radius)
    pr.check_model_and_candidate(cap, six)


def _rejected(fn, *args, match):
    with pytest.raises(AssertionError, match=match):
        fn(*args)


def test_defect_jacobian_sign_on_a_small_entry():
    """one entry of one edge's Jacobian, about 1e-6 of the largest entry of that edge, with its sign flipped"""
    best = None
    for c, six in CASE_DOFS:
        cap = reference_capture(c.name, six)["cap"]
        D = 6 if six else 4
        J = np.abs(cap["Ja"].reshape(-1, D * D))
        ratio = J / J.max(axis=1, keepdims=True)
        score = np.where(ratio > 0, np.abs(np.log10(np.where(ratio > 0, ratio, 1)) + 6), np.inf)
        i = np.unravel_index(np.argmin(score), score.shape)
        if best is None or score[i] < best[0]:
            best = (score[i], c.name, six, i, ratio[i])
    _, name, six, (e, k), ratio = best
    print("flipping Ja[%d][%d] of %s (%d-DoF): %.2e of its edge's largest entry" % (e, k, name, 6 if six else 4, ratio))
    assert 1e-7 < ratio < 1e-5
    cap = fresh(name, six)
    D = 6 if six else 4
    cap["Ja"][e * D * D + k] *= -1
    _rejected(pr.check_evaluation, cap, six, match="^Ja:")


def test_defect_huber_scaling_left_off_just_outside():
    for six in (False, True):
        name = "huber_%d" % (6 if six else 4)
        rc = reference_capture(name, six)
        D = rc["D"]
        s = f64(rc["E"]["s"].v)
        outside = np.where(rc["E"]["outside"] & (s < 0.0102))[0]
        assert len(outside) == 1
        e = int(outside[0])
        cap = fresh(name, six)
        cap["res"][e * D:(e + 1) * D] = f64(rc["E"]["r0"].v[e])
        cap["Ja"][e * D * D:(e + 1) * D * D] = f64(rc["E"]["Ja0"].v[e]).reshape(-1)
        cap["Jb"][e * D * D:(e + 1) * D * D] = f64(rc["E"]["Jb0"].v[e]).reshape(-1)
        _rejected(pr.check_evaluation, cap, six, match="^res:")
        cap["res"] = fresh(name, six)["res"]
        _rejected(pr.check_evaluation, cap, six, match="^Ja:")


def _solve_defect(name, six, mutate):
    rc = reference_capture(name, six)
    A = np.array(f64(rc["A"]))
    mutate(A, rc)
    cap = fresh(name, six)
    cap["y"] = np.linalg.solve(A, f64(rc["b"]))
    _rejected(pr.check_solve, cap, six, BY_NAME[name].radius, match="backward error .* above 8 x")


@pytest.mark.parametrize("name,six", [("pieces60", False), ("pieces60", True), ("level2_4", False), ("shared_coupling_6", True)])
def test_defect_missing_off_diagonal_block(name, six):
    def mutate(A, rc):
        P, D = rc["cap"], rc["D"]
        e = next(e for e in range(len(P["ea"])) if P["eloop"][e] and P["off"][P["ea"][e]] >= 0)
        oa, ob = P["off"][P["ea"][e]], P["off"][P["eb"][e]]
        J = pr._dense_jacobian(P, P["Ja"], P["Jb"], D)[e * D:(e + 1) * D]
        s = P["scale"]
        blk = f64(J[:, ob:ob + D].T @ J[:, oa:oa + D]) * s[ob:ob + D, None] * s[None, oa:oa + D]
        A[ob:ob + D, oa:oa + D] -= blk
        A[oa:oa + D, ob:ob + D] -= blk.T
    _solve_defect(name, six, mutate)


def _coupling_pair(rc):
    """(interior node, separator node) of the first edge between an interior keyframe and a separator"""
    P, part = rc["cap"], rc["part"]
    for a, b in zip(P["ea"], P["eb"]):
        if P["off"][a] >= 0 and P["off"][b] >= 0 and part["isSep"][a] != part["isSep"][b]:
            return (b, a) if part["isSep"][a] else (a, b)
    raise AssertionError("no coupling edge")


@pytest.mark.parametrize("name,six", [("pieces60", False), ("pieces60", True), ("heavy_hi_4", False)])
def test_defect_transposed_coupling_block(name, six):
    def mutate(A, rc):
        D, off = rc["D"], rc["cap"]["off"]
        i, s = _coupling_pair(rc)
        oi, os_ = off[i], off[s]
        blk = A[oi:oi + D, os_:os_ + D].copy()
        assert np.max(np.abs(blk - blk.T)) > 1e-3 * np.max(np.abs(blk))
        A[oi:oi + D, os_:os_ + D] = blk.T
        A[os_:os_ + D, oi:oi + D] = blk
    _solve_defect(name, six, mutate)


@pytest.mark.parametrize("name,six", [("heavy_hi_4", False), ("heavy_6", True), ("pieces60", False)])
def test_defect_zero_last_separator_column_of_the_fullest_piece(name, six):
    def mutate(A, rc):
        D, P, part = rc["D"], rc["cap"], rc["part"]
        p = int(np.argmax(part["cols"]))
        last = max(part["piece_adj"][p], key=lambda k: part["sepOff"][k])          # the separator of the last D columns
        col = P["off"][last] + D - 1
        rows = np.concatenate([P["off"][k] + np.arange(D) for k in range(len(P["off"])) if part["nodePiece"][k] == p])
        assert np.max(np.abs(A[rows, col])) > 0
        A[rows, col] = 0
        A[col, rows] = 0
    _solve_defect(name, six, mutate)


def test_defect_candidate_yaw_not_wrapped():
    rc = reference_capture("wrap_4", False)
    cap = fresh("wrap_4", False)
    crossed = np.where(np.abs(cap["yawC"] - cap["yaw"]) > 300)[0]
    assert len(crossed) > 0
    k = int(crossed[0])
    cap["yawC"][k] += 360.0 if cap["yawC"][k] < 0 else -360.0
    _rejected(pr.check_model_and_candidate, cap, False, match="^yawC:")


@pytest.mark.parametrize("name,six", [("pieces60", False), ("pieces60", True)])
def test_defect_model_without_half_mr_on_one_edge(name, six):
    rc = reference_capture(name, six)
    cap = fresh(name, six)
    M = pr.model_and_candidate(cap["y"], cap["scale"], cap["res"], cap["Ja"], cap["Jb"], cap, cap, six)
    mr2 = np.sum(f64(M["mr"].v) ** 2, axis=1)
    e = int(np.argsort(mr2)[len(mr2) // 2])     # a middling edge, not the one that dominates
    cap["model"] = float(M["model"].v - LD(0.5) * LD(mr2[e]))
    _rejected(pr.check_model_and_candidate, cap, six, match="^model:")


# ---------------------------------------------------------------- a correct float64 solver meets the solve's bars
@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_float64_solvers_meet_the_solve_bars(case, six):
    """LAPACK's LU (the yardstick itself) sits near eps and far below the ceiling; a float64 Cholesky with two triangular
    solves -- another correct solver, standing where the device will stand -- passes check_solve with room to spare"""
    rc = reference_capture(case.name, six)
    A, b, D = rc["A"], rc["b"], rc["D"]
    n = len(b)
    nA = pr.norm2(A)
    eta_lap = pr.eta(A, b, pr.lapack_solve(A, b), nA)
    assert eta_lap <= 2 * pr.EPS64 and eta_lap <= pr.eta_ceiling(n, D) / 100
    A64 = f64(A)
    L = np.linalg.cholesky(A64)
    cap = fresh(case.name, six)
    cap["y"] = np.linalg.solve(L.T, np.linalg.solve(L, f64(b)))
    eta_chol, _, kap, fwd = pr.check_solve(cap, six, case.radius)
    print("%s: n %d eta(LAPACK) %.2e eta(float64 Cholesky) %.2e kappa %.2e" % (case.name, n, eta_lap, eta_chol, kap))
    assert eta_chol <= pr.ETA_MARGIN / 2 * max(eta_lap, pr.EPS64)


# ---------------------------------------------------------------- the cases hit their edges
@pytest.mark.parametrize("case,six", CASE_DOFS, ids=IDS)
def test_case_reaches_its_edge(case, six):
    rc = reference_capture(case.name, six)
    case.reach(rc["part"], rc["cap"], six, ref=rc["cap"])
    part = rc["part"]
    assert np.all(part["cols"] <= pr.PIECE_THREADS) and np.all(part["cols2"] <= pr.PIECE_THREADS)
    assert len(rc["b"]) <= 1300


def test_cases_cover_the_planned_edges():
    names = {c.name for c in CASES}
    for need in ("dense40", "pieces60", "short_last_4", "short_last_6", "edges127_4", "edges128_4", "edges129_4", "edges127_6", "edges128_6",
                 "edges129_6", "nodes128", "nodes129", "level2_4", "level2_6", "level2_control_4", "level2_control_6", "level2_fallback_6",
                 "heavy_hi_4", "heavy_lo_4", "heavy_6", "shared_sep_4", "shared_band_4", "shared_coupling_4", "shared_sep_6", "shared_band_6",
                 "shared_coupling_6", "breaks", "constant_middle_6", "huber_4", "huber_6", "wrap_4", "radius_small"):
        assert need in names
    # the isolated keyframe: J^T J = 0, scale 1, damping at the 1e-6 floor, y = 0
    for six in (False, True):
        rc = reference_capture("breaks", six)
        D, cap = rc["D"], rc["cap"]
        o = cap["off"][-1]
        assert np.all(cap["colsq"][o:o + D] == 0) and np.all(cap["scale"][o:o + D] == 1) and np.all(cap["y"][o:o + D] == 0)
        assert np.allclose(f64(np.diag(rc["A"]))[o:o + D], 1e-6 / BY_NAME["breaks"].radius, rtol=1e-15)
