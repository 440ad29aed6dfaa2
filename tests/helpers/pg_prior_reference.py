"""Long-double reference of the pose graph's evaluation with absolute keyframe measurements (svin_pg_add_prior), with a bound per
entry; the local problem / feeding helpers of the tests that use them; an independent float64 restatement of the cost; and a
small dense Levenberg-Marquardt on the same residuals for graphs of at most 40 keyframes.  Built on pg_edge_reference.py (caller
edges, factor, loss) and pg_reference.py's class V.

Arithmetic (read off svin_amd/csrc/posegraph.hip, pgPrior and k_pg_eval_terms)

  other entries     pg_edge_reference.edges unchanged.
  priors            one-ended: ea = eb = the keyframe k, eloop = 3, the measurement in et / eyaw / eq.
                    4-DoF  u[c] = t_k[c] - t_m[c] (one subtraction), u[3] = wrap(yaw_k - yaw_m) (pg_reference.wrap); Ju is made of
                           the constants 0 and 1 (tangent [yaw, t]: row c has its 1 at column 1 + c, row 3 at column 0).
                    6-DoF  u[c] = t_k[c] - t_m[c]; e = qmul(q_k, conj(q_m)) (dmath.hpp qmul: four products and their sum per
                           component), u[3 + c] = 2 e[c] (exact); Ju (tangent [t, dq]): identity on t, the rotation block
                           2 (e_w I - [e_v]x), entries +-2 e_i (exact doublings of computed values).
                    Then the factor S of the entry (DATA: the host's embedded factor, captured as `einfo`) as
                    pg_edge_reference.apply_factor does it -- rows the prior does not keep are sums of products with exact zeros:
                    value 0, bound 0 -- s = |r|^2, the loss of pg_edge_reference.loss, the scaling.  Jb is stored as zeros (sc * 0).
  incidences        a prior has ONE, on side a (incident()); node_quantities() below counts it once.

numpy_cost() restates the cost in plain float64 numpy and shares no expression with the above: rotations go through rotation
matrices or 4 x 4 quaternion matrices, the information is the quadratic form u_sel^T I u_sel with I = (S^T S) cut to the kept rows,
rho is written out with log1p.

DEFECTS are wrong versions of the evaluation the host tests plant and require the checks to reject.
"""
import numpy as np

from svin_amd import synthetic_pg as spg

import pg_edge_reference as er
import pg_reference as pr

LD = pr.LD
V = pr.V
POSE, POSITION, DEPTH = 0, 1, 2
LOSS_NONE, LOSS_CAUCHY, LOSS_HUBER = er.LOSS_NONE, er.LOSS_CAUCHY, er.LOSS_HUBER
DEFECTS = ("yaw_radians", "q_order", "L_not_LT", "depth_row0", "loss_on_u", "two_incidences")


def rows_of(kind, six):
    """(m, first row) of the rows of u a prior keeps"""
    return {POSE: (6 if six else 4, 0), POSITION: (3, 0), DEPTH: (1, 2)}[int(kind)]


# ---------------------------------------------------------------- priors on a spec, the local problem, feeding
def prior(index, kind, t, q=None, yaw=0.0, info=None, loss=LOSS_NONE, scale=1.0):
    """info: m x m, None (identity) or a callable (six) -> m x m"""
    return dict(index=int(index), kind=int(kind), t=np.asarray(t, np.float64), q=None if q is None else np.asarray(q, np.float64),
                yaw=float(yaw), info=info, loss=int(loss), scale=float(scale))


def truth_prior(spec, k, kind, six, info=None, loss=LOSS_NONE, scale=1.0, dt=(0, 0, 0), seed=None, noise_t=0.0):
    """a prior at the generating pose of keyframe k (plus dt, plus noise)"""
    rng = np.random.default_rng(seed)
    t = spec.t_true[k] + np.asarray(dt, float) + (rng.normal(0, noise_t, 3) if noise_t else 0.0)
    q = spg.R2q(spec.R_true[k])
    return prior(k, kind, t, q, spg.R2ypr(spec.R_true[k])[0], info, loss, scale)


def info_of(p, six):
    return p["info"](six) if callable(p["info"]) else p["info"]


def embedded_factor(p, six):
    """S = L^T of the m x m information (numpy's Cholesky) at the kept rows and columns of a D x D matrix of zeros"""
    D = 6 if six else 4
    m, first = rows_of(p["kind"], six)
    info = info_of(p, six)
    Sm = np.eye(m) if info is None else np.linalg.cholesky(np.asarray(info, np.float64)).T
    S = np.zeros((D, D))
    S[first:first + m, first:first + m] = Sm
    return S


def local_problem(spec, six, earliest, cur, callers, priors, gauge=0):
    """pg_edge_reference.local_problem plus the priors (keyframe index = list position): each at its keyframe's turn, after that
    keyframe's edges, in the order given; priors whose keyframe is outside [earliest, cur] are left out.  On a prior ea = eb, eloop =
    ekind = 3, eid = 1-based position in `priors`, epitch = eroll = 0, esq = 1, eprior = kind (-1 elsewhere).  gauge 1: every keyframe
    free."""
    P = er.local_problem(spec, six, earliest, cur, callers)
    R = 6 if six else 4
    nn = len(P["off"])
    ne0 = len(P["ea"])
    rows = [(int(max(P["ea"][e], P["eb"][e])), 0, e) for e in range(ne0)]
    for c, p in enumerate(priors):
        la = p["index"] - earliest
        if 0 <= la < nn:
            rows.append((la, 1, c))
    rows.sort()
    widths = dict(et=3, eyaw=1, epitch=1, eroll=1, eq=4, esq=6, eloss=2, einfo=R * R)
    out = {k: [] for k in ("ea", "eb", "eloop", "ekind", "eid", "eprior") + tuple(widths)}
    for turn, is_prior, i in rows:
        if not is_prior:
            for k in ("ea", "eb", "eloop", "ekind", "eid"):
                out[k].append(int(P[k][i]))
            out["eprior"].append(-1)
            for k, w in widths.items():
                out[k].append(np.asarray(P[k], np.float64)[w * i:w * i + w])
        else:
            p = priors[i]
            pose = p["kind"] == POSE
            out["ea"].append(turn); out["eb"].append(turn); out["eloop"].append(3); out["ekind"].append(3)
            out["eid"].append(i + 1); out["eprior"].append(p["kind"])
            out["et"].append(np.array([0.0, 0.0, p["t"][2]]) if p["kind"] == DEPTH else p["t"])
            out["eyaw"].append([p["yaw"] if pose and not six else 0.0])
            out["epitch"].append([0.0]); out["eroll"].append([0.0])
            out["eq"].append(p["q"] if pose and six else np.array([0.0, 0, 0, 1]))
            out["esq"].append(np.ones(6))
            out["einfo"].append(embedded_factor(p, six).reshape(-1))
            out["eloss"].append([p["loss"], 1.0 if p["loss"] == LOSS_NONE else p["scale"]])
    Q = dict(P)
    for k in ("ea", "eb", "eloop", "ekind", "eid", "eprior"):
        Q[k] = np.array(out[k], int)
    for k in widths:
        Q[k] = np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in out[k]]) if out[k] else np.zeros(0)
    if gauge == 1:
        Q["off"] = np.arange(nn) * R
    return Q


PROBLEM_KEYS = er.PROBLEM_KEYS + ("eprior",)


def feed(g, spec, callers, priors, gauge=0):
    """pg_edge_reference.feed, then the priors through add_prior and the gauge; returns (earliest, cur, edge ids, prior ids)"""
    earliest, cur, ids = er.feed(g, spec, callers)
    pids = [g.add_prior(p["index"], p["kind"], p["t"], p["q"], p["yaw"], info_of(p, g.six), p["loss"], p["scale"]) for p in priors]
    if gauge:
        g.set_gauge(gauge)
    return earliest, cur, ids, pids


# ---------------------------------------------------------------- the reference
def _is_prior(problem):
    return np.asarray(problem["eloop"], int) == 3


def prior_units(problem, states, six, defect=None):
    """u (ne x R) and Ju (ne x R x D) of the prior entries at unit weight as V; the other rows of the arrays are zero"""
    D = 6 if six else 4
    ea = np.asarray(problem["ea"], int)
    ne = len(ea)
    t = np.asarray(states["t"], np.float64).reshape(-1, 3)
    tk, tm = pr._cols(t[ea], 3), pr._cols(problem["et"], 3)
    zero, one = V(np.zeros(ne)), V(np.ones(ne))
    u = [None] * D
    Ju = [[zero] * D for _ in range(D)]
    for c in range(3):
        u[c] = tk[c] - tm[c]
    if not six:
        yaw = np.asarray(states["yaw"], np.float64)
        u[3] = pr.wrap(V(yaw[ea]) - V(np.asarray(problem["eyaw"], np.float64)))
        for c in range(3):
            Ju[c][1 + c] = one
        Ju[3][0] = one
        if defect == "yaw_radians":
            k = V(LD(pr.K_DEG))
            u[3], Ju[3][0] = u[3] * k, one * k
    else:
        q = np.asarray(states["q"], np.float64).reshape(-1, 4)
        qk, qm = tuple(pr._cols(q[ea], 4)), tuple(pr._cols(problem["eq"], 4))
        e = pr._qmul(pr._conj(qm), qk) if defect == "q_order" else pr._qmul(qk, pr._conj(qm))
        x, y, z, w = [c.exact(2) for c in e]
        for c in range(3):
            u[3 + c] = (x, y, z)[c]
            Ju[c][c] = one
        rot = [[w, z, -y], [-z, w, x], [y, -x, w]]
        for a in range(3):
            for b in range(3):
                Ju[3 + a][3 + b] = rot[a][b]
    return pr.stack(u), pr.stack([pr.stack(row) for row in Ju], axis=1)


def edges(problem, states, six, defect=None):
    """problem as local_problem() returns it (or a capture): dict of V like pg_edge_reference.edges.  The prior entries are
    evaluated here, everything else there."""
    R = 6 if six else 4
    prior_e = _is_prior(problem)
    ne = len(prior_e)
    P = dict(problem)
    P["eloop"] = np.where(prior_e, 2, np.asarray(problem["eloop"], int))   # (their rows of E are replaced below)
    if not np.any(prior_e):
        return er.edges(P, states, six)
    safe = dict(P)
    safe["einfo"] = np.where(np.repeat(prior_e, R * R), np.tile(np.eye(R).reshape(-1), ne), np.asarray(problem["einfo"], np.float64))
    E = er.edges(safe, states, six)
    S = np.asarray(problem["einfo"], np.float64).reshape(ne, R, R).copy()
    assert np.all(np.tril(S, -1) == 0), "einfo is not upper triangular"
    if defect == "L_not_LT":
        S = np.transpose(S, (0, 2, 1)).copy()
    if defect == "depth_row0":
        depth = prior_e & (np.asarray(problem["eprior"], int) == DEPTH)
        S[depth, 0, 0], S[depth, 2, 2] = S[depth, 2, 2], 0.0
    u, Ju = prior_units(problem, states, six, defect)
    zeroJ = V(np.zeros((ne, R, R)))
    if defect == "L_not_LT":   # a lower-triangular factor does not go through apply_factor's upper-triangular sums
        Sv = V(S)
        r = (Sv * u[:, None, :]).sum(2)
        Ja = pr.stack([(Sv[:, :, j][:, :, None] * Ju[:, j, :][:, None, :]) for j in range(R)], axis=0).sum(0)
        Jb = zeroJ
    else:
        r, Ja, Jb = er.apply_factor(S, u, Ju, zeroJ)
    s = (r * r).sum(1)
    s_loss = (u * u).sum(1) if defect == "loss_on_u" else s
    lossp = np.asarray(problem["eloss"], np.float64).reshape(ne, 2)
    kind = np.where(prior_e, lossp[:, 0].astype(int), LOSS_NONE)
    cost_e, sc, scaled = er.loss(s_loss, kind, np.where(prior_e & (kind != LOSS_NONE), lossp[:, 1], 1.0))
    res = (r * sc[:, None]).where(scaled[:, None], r)
    JaR = (Ja * sc[:, None, None]).where(scaled[:, None, None], Ja)
    JbR = V(np.zeros((ne, R, R)))
    if defect == "two_incidences":   # the block counted on both sides: what a second incidence amounts to downstream
        JbR = JaR
    p1, p2, p3 = prior_e, prior_e[:, None], prior_e[:, None, None]
    out = dict(r0=r.where(p2, E["r0"]), Ja0=Ja.where(p3, E["Ja0"]), Jb0=Jb.where(p3, E["Jb0"]), s=s.where(p1, E["s"]),
               sc=sc.where(p1, E["sc"]), outside=np.where(prior_e, scaled, E["outside"]), res=res.where(p2, E["res"]),
               Ja=JaR.where(p3, E["Ja"]), Jb=JbR.where(p3, E["Jb"]), cost_e=cost_e.where(p1, E["cost_e"]))
    out["cost"] = out["cost_e"].sum(0)
    return out


def incident(problem):
    """nodePtr / nodeEdge of optimize(): per node the incident (edge, side) in list order; a prior has one incidence, on side a"""
    ea, eb = np.asarray(problem["ea"], int), np.asarray(problem["eb"], int)
    prior_e = _is_prior(problem)
    inc = [[] for _ in range(len(problem["off"]))]
    for e in range(len(ea)):
        inc[ea[e]].append((e, 0))
        if not prior_e[e]:
            inc[eb[e]].append((e, 1))
    return inc


def node_blocks(res, Ja, Jb, problem, six, inc=None):
    """float64 gradient (n) and J^T J blocks (nn x D x D) over the incidences given (default: incident())"""
    D = 6 if six else 4
    off = np.asarray(problem["off"], int)
    res = np.asarray(res, np.float64).reshape(-1, D)
    Ja, Jb = np.asarray(Ja, np.float64).reshape(-1, D, D), np.asarray(Jb, np.float64).reshape(-1, D, D)
    g, blk = np.zeros(int(np.sum(off >= 0)) * D), np.zeros((len(off), D, D))
    for k, lst in enumerate(incident(problem) if inc is None else inc):
        if off[k] < 0:
            continue
        for e, side in lst:
            J = (Jb if side else Ja)[e]
            g[off[k]:off[k] + D] += J.T @ res[e]
            blk[k] += J.T @ J
    return g, blk


def _left(q):
    x, y, z, w = q
    return np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])


def numpy_cost(problem, states, six):
    """the cost in plain float64 numpy, written independently: pg_edge_reference.numpy_cost on the two-ended entries plus, per prior,
    rho(u_sel^T I u_sel) / 2"""
    R = 6 if six else 4
    prior_e = _is_prior(problem)
    ne = len(prior_e)
    keep = np.where(~prior_e)[0]
    sub = dict(problem)
    for k, w in (("ea", 1), ("eb", 1), ("eloop", 1), ("et", 3), ("eyaw", 1), ("epitch", 1), ("eroll", 1), ("eq", 4), ("esq", 6),
                 ("einfo", R * R), ("eloss", 2)):
        sub[k] = np.asarray(problem[k]).reshape(ne, w)[keep].reshape(-1)
    total = er.numpy_cost(sub, states, six) if len(keep) else 0.0
    t = np.asarray(states["t"], float).reshape(-1, 3)
    S = np.asarray(problem["einfo"], float).reshape(ne, R, R)
    lossp = np.asarray(problem["eloss"], float).reshape(ne, 2)
    for e in np.where(prior_e)[0]:
        k = int(problem["ea"][e])
        m, first = rows_of(problem["eprior"][e], six)
        dt = t[k] - np.asarray(problem["et"][3 * e:3 * e + 3], float)
        if six:
            qk = np.asarray(states["q"], float).reshape(-1, 4)[k]
            qm = np.asarray(problem["eq"][4 * e:4 * e + 4], float)
            qe = _left(qk) @ (qm * np.array([-1.0, -1.0, -1.0, 1.0]))
            u = np.concatenate([dt, 2 * qe[:3]])
        else:
            dy = float(np.asarray(states["yaw"], float)[k] - problem["eyaw"][e])
            dy = dy - 360 if dy > 180 else (dy + 360 if dy < -180 else dy)
            u = np.concatenate([dt, [dy]])
        info = (S[e].T @ S[e])[first:first + m, first:first + m]
        us = u[first:first + m]
        s = float(us @ info @ us)
        kind, a_ = int(lossp[e, 0]), lossp[e, 1]
        if kind == LOSS_HUBER:
            rho = s if s <= a_ * a_ else 2 * a_ * np.sqrt(s) - a_ * a_
        elif kind == LOSS_CAUCHY:
            rho = a_ * a_ * np.log1p(s / (a_ * a_))
        else:
            rho = s
        total += 0.5 * rho
    return total


# ---------------------------------------------------------------- float64 evaluation, Plus, central differences, a dense LM
def evaluate64(problem, states, six, defect=None):
    """edges() run in float64: dict of float64 arrays res (ne x R), Ja, Jb (ne x R x D), r0, Ja0, cost"""
    with pr.evaluate_in(np.float64):
        E = edges(problem, states, six, defect)
    return {k: np.asarray(E[k].v, np.float64) for k in ("res", "Ja", "Jb", "r0", "Ja0", "Jb0", "cost", "cost_e", "s")}


def plus(states, problem, delta, six):
    """Plus(x, delta) of the solver's tangent on the free keyframes (4-DoF [yaw, t] with one wrap, 6-DoF [t, dq] with
    q <- [sin|d| d/|d|, cos|d|] q)"""
    D = 6 if six else 4
    off = np.asarray(problem["off"], int)
    yaw = np.array(states["yaw"], np.float64)
    t = np.array(states["t"], np.float64).reshape(-1, 3)
    q = np.array(states["q"], np.float64).reshape(-1, 4)
    for k in np.where(off >= 0)[0]:
        d = delta[off[k]:off[k] + D]
        if six:
            t[k] += d[:3]
            nd = float(np.linalg.norm(d[3:]))
            if nd > 0:
                q[k] = _left(np.concatenate([np.sin(nd) / nd * d[3:], [np.cos(nd)]])) @ q[k]
        else:
            y = yaw[k] + d[0]
            yaw[k] = y - 360 if y > 180 else (y + 360 if y < -180 else y)
            t[k] += d[1:]
    return dict(yaw=yaw, t=t.reshape(-1), q=q.reshape(-1))


def central_difference_jacobian(problem, states, six, e, h=1e-6):
    """d r0[e] / d(tangent of keyframe ea[e]) by central differences of the float64 evaluation through plus(): R x D"""
    D = 6 if six else 4
    P = dict(problem)
    P["off"] = np.arange(len(problem["off"])) * D
    k = int(problem["ea"][e])
    J = np.zeros((D, D))
    for c in range(D):
        d = np.zeros(len(P["off"]) * D)
        d[k * D + c] = h
        hi = evaluate64(P, plus(states, P, d, six), six)["r0"][e]
        lo = evaluate64(P, plus(states, P, -d, six), six)["r0"][e]
        J[:, c] = (hi - lo) / (2 * h)
    return J


def lm_solve(problem, states, six, max_iterations=200, tol=1e-14):
    """a plain dense Levenberg-Marquardt on the float64 evaluation (robustified residuals and Jacobians as the device stores
    them; damping on the diagonal of J^T J; a step is kept when the cost falls): (states, cost, iterations).  For graphs of at
    most 40 keyframes."""
    D = 6 if six else 4
    assert len(problem["off"]) <= 40
    x = dict(yaw=np.array(states["yaw"], np.float64), t=np.array(states["t"], np.float64), q=np.array(states["q"], np.float64))
    E = evaluate64(problem, x, six)
    cost, mu = float(E["cost"]), 1e-4
    for it in range(max_iterations):
        J = np.asarray(pr._dense_jacobian(problem, E["Ja"], E["Jb"], D), np.float64)
        r = E["res"].reshape(-1)
        H, g = J.T @ J, J.T @ r
        if np.max(np.abs(g), initial=0.0) < 1e-13:
            break
        improved = False
        for _ in range(40):
            A = H + mu * np.diag(np.maximum(np.diag(H), 1e-9))
            try:
                d = -np.linalg.solve(A, g)
            except np.linalg.LinAlgError:
                mu *= 10
                continue
            xn = plus(x, problem, d, six)
            En = evaluate64(problem, xn, six)
            if float(En["cost"]) < cost:
                drop = cost - float(En["cost"])
                x, E, cost, mu, improved = xn, En, float(En["cost"]), max(mu / 10, 1e-15), True
                break
            mu *= 10
        if not improved or drop <= tol * cost:
            break
    return x, cost, it + 1


# ---------------------------------------------------------------- the comparisons of tests/test_gpu_posegraph_priors.py
def check_evaluation(cap, six):
    """stage 1: the device's res, Ja, Jb and cost against edges(); a prior's Jb is zero exactly"""
    E = edges(cap, cap, six)
    pr.assert_close("res", cap["res"], E["res"].v.reshape(-1), E["res"].tol().reshape(-1))
    pr.assert_close("Ja", cap["Ja"], E["Ja"].v.reshape(-1), E["Ja"].tol().reshape(-1))
    pr.assert_close("Jb", cap["Jb"], E["Jb"].v.reshape(-1), E["Jb"].tol().reshape(-1))
    pr.assert_close("cost", cap["cost"], E["cost"].v, E["cost"].tol())
    R = 6 if six else 4
    assert np.all(np.asarray(cap["Jb"]).reshape(-1, R * R)[_is_prior(cap)] == 0.0), "a prior's Jb is not zero"
    return E


def check_node_pass(cap, six):
    """stage 2: pg_reference.check_node_pass.  It walks both sides of every entry; a prior's side b holds the zeros
    check_evaluation has already required, so it adds exact zeros to value and bound alike (the count of terms in the bound grows
    by R per prior).  A prior's block counted twice is out by the block itself."""
    return pr.check_node_pass(cap, six)


def check_model_and_candidate(cap, six):
    """stage 4: pg_edge_reference.check_model_and_candidate with the candidate's cost from edges() here"""
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
