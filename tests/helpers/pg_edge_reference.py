"""Long-double reference of the pose graph's evaluation with caller-given edges (svin_pg_add_edge), with a bound per entry, and
the local problem / feeding helpers of the tests that use them.  Built on pg_reference.py's class V and its edges().

Arithmetic (read off svin_amd/csrc/posegraph.hip, k_pg_eval_edges)

  built-in edges    pg_reference.edges unchanged (weights, HuberLoss(0.1) on loops).
  caller edges      u, Ju_a, Ju_b: pgEdge at unit weights = pg_reference.edges with eloop = 0 and esq = 1 on these edges (the
                    multiplications by 1.0 are exact; the reference counts them as a rounding, which only widens the bound by
                    one unit).  Then, with S the upper-triangular factor of the edge (DATA: the host's Cholesky factor, captured
                    as `einfo`), r[k] = sum_{j >= k} S[k][j] u[j] and J[k][c] = sum_{j >= k} S[k][j] Ju[j][c]: a sum of at most R
                    products of a datum and a computed value, each product |S| e_u + |S u| (class V's product rule), the sum of
                    n <= R terms n M on top.  s = |r|^2 (R products, their sum).  The loss on s, parameters per edge (`eloss`):
                      NONE       cost = s / 2, nothing is scaled;
                      Huber(a)   b = a * a (the double product); s > b: cost = (2 a sqrt(s) - b) / 2, sc = sqrt(a / sqrt(s)),
                                 else cost = s / 2, sc = 1 -- counted as pg_reference counts it: one sqrt, one division, one
                                 sqrt, and the product with r or J (1);
                      Cauchy(a)  b = a * a, c = 1 / b (both IEEE double operations on data: the reference takes the double
                                 results), sum = 1 + s c (one product, one addition), inv = 1 / sum (U_DIV), cost = b log(sum) / 2
                                 (U_LOG, one product), sc = sqrt(inv) (U_SQRT), and the product with r or J (1).
                    Stored: sc r, sc Ja, sc Jb; the cost is the sum of the edges' costs.
U_LOG = 1: the HIP math API's table of double-precision device functions gives log 1 ulp (sin / cos 2, sqrt 1, as in
pg_reference.py).

numpy_cost() is an independent plain-numpy restatement of the cost (rotation matrices from the library's synthetic generator,
quaternion products as 4 x 4 matrices, the information matrix S^T S as a quadratic form, Ceres' rho written out with log1p) that
shares no expression with the above.
"""
import numpy as np

from svin_amd import synthetic_pg as spg

import pg_cases as pc
import pg_reference as pr

LD = pr.LD
V = pr.V
U_LOG = 1
LOSS_NONE, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2


# ---------------------------------------------------------------- caller edges on a spec, the local problem, feeding
def measure(spec, a, b, seed=0, noise_t=0.002, noise_deg=0.02, dt=(0, 0, 0), dyaw=0.0):
    """the pose of keyframe b in the frame of keyframe a from the true geometry (as pg_cases.set_loops measures a loop):
    (rel_t, rel_q, rel_yaw_deg)"""
    rng = np.random.default_rng(seed)
    Ra, Rb = spec.R_true[a], spec.R_true[b] @ spg.ypr2R(rng.normal(0, noise_deg, 3))
    rel_t = Ra.T @ (spec.t_true[b] - spec.t_true[a]) + rng.normal(0, noise_t, 3) + np.asarray(dt, float)
    yaw = spg.R2ypr(Rb)[0] - spg.R2ypr(Ra)[0] + dyaw
    yaw = yaw - 360.0 if yaw > 180.0 else (yaw + 360.0 if yaw < -180.0 else yaw)
    return rel_t, spg.R2q(Ra.T @ Rb), float(yaw)


def caller_edge(spec, a, b, info=None, loss=LOSS_NONE, scale=1.0, **kw):
    t, q, yaw = measure(spec, a, b, **kw)
    return dict(a=int(a), b=int(b), t=t, q=q, yaw=yaw, info=info, loss=int(loss), scale=float(scale))


def default_factor(six):
    return np.diag(np.array([20.0, 20, 20, 100, 100, 100] if six else [1.0, 1, 1, 0.1]))


def factor_of(info, six):
    """S = L^T of information = L L^T (numpy's Cholesky: the host's differs by roundings; tests take the captured einfo as data)"""
    if info is None:
        return default_factor(six)
    if callable(info):
        info = info(six)
    return np.linalg.cholesky(np.asarray(info, np.float64)).T


def info_of(edge, six):
    info = edge["info"]
    return info(six) if callable(info) else info


def local_problem(spec, six, earliest, cur, callers):
    """pg_cases.local_problem plus the caller-given edges (keyframe index = list position): each at the turn of its later
    keyframe, after that keyframe's built-in edges, in the order given; edges reaching outside [earliest, cur] are left out.
    Adds ekind, eid (1-based position in `callers`), einfo (ne x R x R), eloss (ne x 2); eloop = 2 and esq = 1 on caller edges."""
    P = pc.local_problem(spec, six, earliest, cur)
    R = 6 if six else 4
    ne0 = len(P["ea"])
    turn0 = np.maximum(P["ea"], P["eb"])
    nn = len(P["off"])
    rows = []   # (turn, order, builtin index or -1, caller index)
    for e in range(ne0):
        rows.append((int(turn0[e]), 0, e, e, -1))
    for c, ce in enumerate(callers):
        la, lb = ce["a"] - earliest, ce["b"] - earliest
        if min(la, lb) < 0 or max(la, lb) >= nn:
            continue
        rows.append((max(la, lb), 1, c, -1, c))
    rows.sort(key=lambda x: x[:3])
    keys3, keys1, keys4, keys6 = ("et",), ("eyaw", "epitch", "eroll"), ("eq",), ("esq",)
    out = {k: [] for k in ("ea", "eb", "eloop", "et", "eyaw", "epitch", "eroll", "eq", "esq", "ekind", "eid", "einfo", "eloss")}
    for _, _, _, e, c in rows:
        if e >= 0:
            for k in ("ea", "eb", "eloop"):
                out[k].append(int(P[k][e]))
            for ks, w in ((keys3, 3), (keys1, 1), (keys4, 4), (keys6, 6)):
                for k in ks:
                    out[k].append(P[k][w * e:w * e + w])
            lp = int(P["eloop"][e])
            out["ekind"].append(lp); out["eid"].append(0)
            out["einfo"].append(np.diag(P["esq"][6 * e:6 * e + 6]) if six else np.diag([1.0, 1, 1, 0.1 if lp else 1.0]))
            out["eloss"].append([LOSS_HUBER, 0.1] if lp else [LOSS_NONE, 0.0])
        else:
            ce = callers[c]
            la, lb = ce["a"] - earliest, ce["b"] - earliest
            out["ea"].append(la); out["eb"].append(lb); out["eloop"].append(2)
            out["et"].append(np.asarray(ce["t"], float)); out["eyaw"].append([0.0 if six else ce["yaw"]])
            out["epitch"].append([P["pitch"][la]]); out["eroll"].append([P["roll"][la]])
            out["eq"].append(np.asarray(ce["q"], float)); out["esq"].append(np.ones(6))
            out["ekind"].append(2); out["eid"].append(c + 1)
            out["einfo"].append(factor_of(ce["info"], six))
            out["eloss"].append([ce["loss"], 1.0 if ce["loss"] == LOSS_NONE else ce["scale"]])
    Q = dict(P)
    for k in ("ea", "eb", "eloop", "ekind", "eid"):
        Q[k] = np.array(out[k], int)
    for k in ("et", "eyaw", "epitch", "eroll", "eq", "esq", "eloss"):
        Q[k] = np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in out[k]]) if out[k] else np.zeros(0)
    Q["einfo"] = np.array(out["einfo"], np.float64).reshape(-1, R, R).reshape(-1)
    return Q


PROBLEM_KEYS = pc.PROBLEM_KEYS + ("ekind", "eid", "eloss")


def feed(g, spec, callers):
    """spg.feed, then the caller edges through add_edge; returns (earliest, cur, ids)"""
    earliest, cur = spg.feed(g, spec)
    ids = []
    for ce in callers:
        ids.append(g.add_edge(ce["a"], ce["b"], ce["t"], ce["q"], ce["yaw"], info_of(ce, g.six), ce["loss"], ce["scale"]))
    return earliest, cur, ids


# ---------------------------------------------------------------- the reference
def _unit_problem(problem):
    P = dict(problem)
    caller = np.asarray(problem["eloop"], int) == 2
    P["eloop"] = np.where(caller, 0, np.asarray(problem["eloop"], int))
    esq = np.array(problem["esq"], np.float64).reshape(-1, 6)
    esq[caller] = 1.0
    P["esq"] = esq.reshape(-1)
    return P, caller


def _log(x):
    return x.func(np.log, lambda v: LD(1) / np.abs(v), U_LOG)


def apply_factor(S, u, Ja, Jb):
    """r = S u, J = S Ju; S (ne x R x R float64 data, upper triangular), u (ne x R), Ja / Jb (ne x R x D) as V"""
    R = S.shape[1]
    r, A, B = [], [], []
    for k in range(R):
        Sk = [V(S[:, k, j]) for j in range(k, R)]
        r.append(pr.vsum([Sk[j - k] * u[:, j] for j in range(k, R)]))
        A.append(pr.vsum([Sk[j - k][:, None] * Ja[:, j, :] for j in range(k, R)]))
        B.append(pr.vsum([Sk[j - k][:, None] * Jb[:, j, :] for j in range(k, R)]))
    return pr.stack(r), pr.stack(A, axis=1), pr.stack(B, axis=1)


def loss(s, kind, a64):
    """(cost_e, sc, scaled) of s (V, n) under per-edge kind / scale (float64 data); scaled: where sc multiplies (elsewhere the
    stored values are r, J themselves)"""
    n = len(kind)
    one = V(np.ones(n))
    a = V(np.asarray(a64, np.float64))
    b64 = np.asarray(a64, np.float64) * np.asarray(a64, np.float64)          # `b = a * a` in double
    b = V(b64)
    # Huber
    hub_out = (kind == LOSS_HUBER) & (s.v > b.v)
    rt = s.where(hub_out, one).sqrt()
    cost_h = ((a * rt).exact(2) - b).exact(0.5)
    ratio = a * rt.recip()
    ratio = ratio.where(ratio.v > LD(pr.DBL_MIN), V(LD(pr.DBL_MIN)))
    sc_h = ratio.sqrt()
    # Cauchy
    cau = kind == LOSS_CAUCHY
    b_safe = np.where(cau, b64, 1.0)
    c = V(np.float64(1.0) / b_safe)                                          # `c = 1.0 / b` in double
    total = one + s * c
    inv = total.recip()
    cost_c = (V(b_safe) * _log(total)).exact(0.5)
    sc_c = inv.sqrt()
    cost = cost_c.where(cau, cost_h.where(hub_out, s.exact(0.5)))
    sc = sc_c.where(cau, sc_h.where(hub_out, one))
    return cost, sc, cau | hub_out


def edges(problem, states, six):
    """problem as local_problem() returns it (or a capture: the device's einfo / eloss / eloop): dict of V like
    pg_reference.edges -- r0 Ja0 Jb0 (before the loss, after the factor), s, sc, res Ja Jb, cost_e, cost"""
    R = 6 if six else 4
    P, caller = _unit_problem(problem)
    E = pr.edges(P, states, six)
    ne = len(caller)
    if not np.any(caller):
        return E
    S = np.asarray(problem["einfo"], np.float64).reshape(ne, R, R)
    kind = np.asarray(problem["eloss"], np.float64).reshape(ne, 2)[:, 0].astype(int)
    scale = np.asarray(problem["eloss"], np.float64).reshape(ne, 2)[:, 1]
    assert np.all(np.tril(S, -1) == 0), "einfo is not upper triangular"
    r, Ja, Jb = apply_factor(S, E["r0"], E["Ja0"], E["Jb0"])
    s = (r * r).sum(1)
    kind_c = np.where(caller, kind, LOSS_NONE)
    cost_e, sc, scaled = loss(s, kind_c, np.where(caller & (kind != LOSS_NONE), scale, 1.0))
    res = (r * sc[:, None]).where(scaled[:, None], r)
    JaR = (Ja * sc[:, None, None]).where(scaled[:, None, None], Ja)
    JbR = (Jb * sc[:, None, None]).where(scaled[:, None, None], Jb)
    c1, c2, c3 = caller, caller[:, None], caller[:, None, None]
    out = dict(r0=r.where(c2, E["r0"]), Ja0=Ja.where(c3, E["Ja0"]), Jb0=Jb.where(c3, E["Jb0"]), s=s.where(c1, E["s"]),
               sc=sc.where(c1, E["sc"]), outside=np.where(caller, scaled, E["outside"]), res=res.where(c2, E["res"]),
               Ja=JaR.where(c3, E["Ja"]), Jb=JbR.where(c3, E["Jb"]), cost_e=cost_e.where(c1, E["cost_e"]))
    out["cost"] = out["cost_e"].sum(0)
    return out


def _left(q):
    """q (x) p = _left(q) p for [x y z w] quaternions"""
    x, y, z, w = q
    return np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])


def numpy_cost(problem, states, six):
    """the cost in plain float64 numpy, written independently: sum over the edges of rho(u^T (S^T S) u) / 2"""
    R = 6 if six else 4
    ne = len(problem["ea"])
    t = np.asarray(states["t"], float).reshape(-1, 3)
    S = np.asarray(problem["einfo"], float).reshape(ne, R, R)
    lossp = np.asarray(problem["eloss"], float).reshape(ne, 2)
    total = 0.0
    for e in range(ne):
        a, b = int(problem["ea"][e]), int(problem["eb"][e])
        if six:
            q = np.asarray(states["q"], float).reshape(-1, 4)
            # the quaternions as they are stored: the sign of 2 vec(.) follows the hemispheres of rel_q and q_a^-1 q_b (include/svin_pg.h)
            Ra, conj = spg.q2R(q[a]), np.array([-1.0, -1.0, -1.0, 1.0])
            qab = _left(conj * q[a]) @ q[b]
            qd = _left(np.asarray(problem["eq"][4 * e:4 * e + 4], float)) @ (conj * qab)
            u = np.concatenate([Ra.T @ (t[b] - t[a]) - problem["et"][3 * e:3 * e + 3], 2 * qd[:3]])
        else:
            yaw = np.asarray(states["yaw"], float)
            Ra = spg.ypr2R([yaw[a], problem["epitch"][e], problem["eroll"][e]])
            dy = yaw[b] - yaw[a] - problem["eyaw"][e]
            dy = dy - 360 if dy > 180 else (dy + 360 if dy < -180 else dy)
            u = np.concatenate([Ra.T @ (t[b] - t[a]) - problem["et"][3 * e:3 * e + 3], [dy]])
        s = float(u @ (S[e].T @ S[e]) @ u)
        kind, a_ = int(lossp[e, 0]), lossp[e, 1]
        if kind == LOSS_HUBER:
            rho = s if s <= a_ * a_ else 2 * a_ * np.sqrt(s) - a_ * a_
        elif kind == LOSS_CAUCHY:
            rho = a_ * a_ * np.log1p(s / (a_ * a_))
        else:
            rho = s
        total += 0.5 * rho
    return total


# ---------------------------------------------------------------- the comparisons of tests/test_gpu_posegraph_edges.py
def check_evaluation(cap, six):
    """stage 1 with caller edges: the device's res, Ja, Jb and cost against edges() (pg_reference.check_evaluation's assertions)"""
    E = edges(cap, cap, six)
    pr.assert_close("res", cap["res"], E["res"].v.reshape(-1), E["res"].tol().reshape(-1))
    pr.assert_close("Ja", cap["Ja"], E["Ja"].v.reshape(-1), E["Ja"].tol().reshape(-1))
    pr.assert_close("Jb", cap["Jb"], E["Jb"].v.reshape(-1), E["Jb"].tol().reshape(-1))
    pr.assert_close("cost", cap["cost"], E["cost"].v, E["cost"].tol())
    return E


def check_model_and_candidate(cap, six):
    """stage 4: pg_reference.check_model_and_candidate's assertions; the candidate's cost comes from edges() here, because
    pg_reference.edges does not know the caller edges"""
    M = pr.model_and_candidate(cap["y"], cap["scale"], cap["res"], cap["Ja"], cap["Jb"], cap, cap, six)
    assert np.isfinite(cap["step2"]), "step^2 is not finite"
    pr.assert_close("model", cap["model"], M["model"].v, M["model"].tol())
    if six:
        pr.assert_close("qC", cap["qC"], M["qC"].v.reshape(-1), M["qC"].tol().reshape(-1))
    else:
        pr.assert_close("yawC", cap["yawC"], M["yawC"].v, M["yawC"].tol())
    pr.assert_close("tC", cap["tC"], M["tC"].v.reshape(-1), M["tC"].tol().reshape(-1))
    pr.assert_close("step2", cap["step2"], M["step2"].v, M["step2"].tol())
    pr.assert_close("x2", cap["x2"], M["x2"].v, M["x2"].tol())
    C = edges(cap, dict(yaw=cap["yawC"], t=cap["tC"], q=cap["qC"]), six)["cost"]
    pr.assert_close("costC", cap["costC"], C.v, C.tol())
    return M


def shared_pairs(problem, min_count=3):
    """{(lo, hi): [edges]} of the pairs of free keyframes that carry min_count or more edges"""
    off = np.asarray(problem["off"], int)
    pairs = {}
    for e, (a, b) in enumerate(zip(problem["ea"], problem["eb"])):
        if off[a] >= 0 and off[b] >= 0:
            pairs.setdefault((int(min(a, b)), int(max(a, b))), []).append(e)
    return {k: v for k, v in pairs.items() if len(v) >= min_count}
