"""Long-double reference of one Levenberg-Marquardt step of the pose graph, stage by stage, with a bound for every entry.

Every stage is a pure function of the records that stage consumes (PoseGraph.debug_step() hands them over), recomputed in
np.longdouble (64-bit mantissa).  Next to each value the functions return the bound a float64 result has to meet.

Arithmetic (read off svin_amd/csrc/posegraph.hip)

  edges             pgEdge + k_pg_eval.  4-DoF (FourDOFError / FourDOFWeightError), tangent [yaw, t], angles in DEGREES:
                        R = ypr2R(yaw_a, pitch_e, roll_e) (angle / 180 * pi with pi the double 3.14159265358979323846),
                        r[0:3] = R^T (t_b - t_a) - t_e,   r[3] = wrap(yaw_b - yaw_a - yaw_e) * (0.1 on loop edges),
                        wrap(x) = x - 360 if x > 180, x + 360 if x < -180 (ONE wrap), dr/dyaw_a = (dR/dyaw)^T d with the
                        factor pi / 180 (a double), dr/dt_a = -R^T, dr/dt_b = R^T, dr3/dyaw = -+ weight.
                    6-DoF (PoseGraph3dErrorTerm), tangent [t, dq] with q <- [sin|d| d/|d|, cos|d|] q:
                        u = [R(q_a)^T (t_b - t_a) - t_e, 2 vec(q_e conj(conj(q_a) q_b))],  r = sqrt_info * u,
                        Jacobians as pgEdge writes them (2 R^T [d]x; 2 plus(q_e conj(q_b)) oplus(q_a) on the rotation rows).
                    Loop edges carry HuberLoss(0.1): s = |r|^2, b = 0.1 * 0.1 (the double product); s > b:
                        cost = 0.5 (2 * 0.1 sqrt(s) - b), sc = sqrt(0.1 / sqrt(s)); else cost = 0.5 s, sc = 1; what is
                        stored is sc r, sc Ja, sc Jb.
  node_quantities   k_pg_node from the DEVICE's stored res, Ja, Jb (data): g = sum J^T r, blk = lower(sum J^T J) over the
                    incident edges, colsq = diag(blk), scale = 1 / (1 + sqrt(colsq)), gradmax = max |g|.
  system / solve    A = diag(s) J^T J diag(s) + diag(clamp(diag(J^T J) s^2, 1e-6, 1e32)) / radius, b = diag(s) g in tangent
                    order (pgAssembleNode / pgAssembleEdge), solved by a long-double Cholesky.
  model_and_candidate   k_pg_model_plus: delta = -y * scale; model = sum_e sum_q mr (res + 0.5 mr), mr = Ja delta_a + Jb delta_b
                    (constant ends contribute nothing); pgPlus: yaw <- wrap(yaw + delta), t <- t + delta,
                    q <- [sin(nd) / nd * d, cos(nd)] q with nd = |d| and q unchanged when nd == 0;
                    step2 = sum |x_c - x|^2, x2 = sum |x|^2 over the free keyframes in ambient coordinates.

The bound.  Stages 1, 2 and 4 are short sums of products.  For a sum of n terms with M the sum of their absolute values, a
float64 evaluation in ANY order, with or without FMA, errs by at most gamma_(n + c0) M <= (n + c0) eps M (Higham, Accuracy and
Stability, 3.1 / 3.3), c0 the roundings inside a term; eps = 2^-52 = 2u leaves a factor two for the second-order terms.  Where
the terms are themselves computed (a rotation entry, a residual that is a difference of large numbers and is then squared)
each term carries the bound of its factors to first order, as step_reference.py does.  Class V is that rule as code: a value v
and its bound e in units of eps,
     data                      e = 0                (a zero or a weight the kernel stores as a literal must be exact)
     a + b, a - b              e = e_a + e_b + |v|                        (one rounding)
     a * b                     e = |a| e_b + |b| e_a + |v|                (c0 = 1 for a product of data; every computed factor
                                                                           brings its own bound)
     times 2, 0.5, -1          exact
     a / constant              e = e_a / |c| + |v|
     sum of n terms            e = sum e_i + n M,  M = sum |v_i|          (n - 1 additions in any order, one to spare)
     f(a), f in sin cos sqrt 1/x    e = |f'(v)| e_a + U_f |f(v)|          (the argument's error through f', plus U_f ulp)
Counted for the stages: a 4-DoF rotation entry is at most 3 products of sines / cosines (each 2 roundings for angle / 180 * pi
carried through f', plus U_f) and one addition; a translation residual row 3 products, the sum of 3, the difference t_b - t_a
before and the measurement after: c0 = 4 on top of the rotation's own bound; a 6-DoF row adds the scaling by sqrt_info (1);
the Huber corrector one sqrt, one division, one sqrt, and its product with r or J (1).  node_quantities: n = R * degree products
of DATA, c0 = 1: (n + 1) eps M.  model: per row 2 D products of data and delta (delta = -y scale: 1), mr (res + 0.5 mr): 2 more,
then the sum over ne R terms.  step2, x2: sums of squares over the free keyframes' ambient coordinates.
U_f: the HIP math API documentation (ROCm HIP "Math API" reference, table of double-precision device functions with their
maximum ULP error) gives sin and cos 2, sqrt 1; division is IEEE (taken as 1); tests/helpers/step_reference.py uses the same 2 ulp
for the device's sine and cosine.
The same bounds with the long-double eps hold for this reference itself (its libm's sinl / cosl / sqrtl are good to 1 ulp of
the long double): its error is at most (eps_ld / eps) tol = 2^-11 tol, which `check_precision` asserts to be below tol / 1000.

Stage 3 (the solve) is judged normwise.  The device eliminates the pieces, then the level-2 pieces, then the root: a Cholesky
factorisation A = R^T R in a nested-dissection order with Y = L^-1 C and S - Y^T Y formed block-wise, followed by the two
substitutions.  By Higham 10.3 / 10.4 the computed y solves (A + dA) y = b with |dA| <= gamma_(3n+1) |R^T| |R| whatever the
elimination and summation order, and || |R^T| |R| ||_2 <= n ||A||_2 (10.7), so
     eta(y) = |b - A y|_2 / (|A|_2 |y|_2 + |b|_2) <= n (3n + 1 + C_RSQ + C_ASM) eps =: ceiling(n, R)
     C_RSQ = 8: the reciprocal square roots (pgRsqrt: v_rsq_f64 plus two Newton steps, the dense solver's alike) are not
                correctly rounded; a diagonal entry and the D - 1 entries scaled by it each take up to 2 ulp more, which is a
                constant added to the row's gamma (4 for the factor, 4 for the substitutions that multiply by dinv);
     C_ASM = R + 4: A itself is formed in float64 from the stored Jacobians (R products per entry, two scalings, the clamp /
                radius term and its addition): |dA_asm| <= (R + 4) eps |Js|^T |Js|, and || |Js|^T |Js| ||_2 <= trace(Js^T Js)
                <= n ||A||_2.
The ceiling is of order n^2 eps; the measured bar of the GPU test is eta(device) <= ETA_MARGIN * max(eta(LAPACK), eps) with
numpy.linalg.solve in float64 on the same A, b as the yardstick, ETA_MARGIN = 8: up to three nested eliminations, each a
Cholesky solve with LAPACK's own bound, and twice that for the different summation order of the Gram products and the
iterated reciprocal square roots.  Forward error: |y - y_ld|_2 / |y_ld|_2 <= kappa_2(A) * (the bar in force for eta).

The symbolic step (cuts, vertex cover, level 2 and its fall-back) is restated in `partition()`.
"""
import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EPS_LD = float(np.finfo(LD).eps)
U_TRIG = 2
U_SQRT = 1
U_DIV = 1
C_RSQ = 8
ETA_MARGIN = 8
PI64 = np.float64(3.14159265358979323846)
K_DEG = PI64 / np.float64(180.0)          # `const double k = kPgPi / 180.0`
HUBER_A = np.float64(0.1)
HUBER_B = HUBER_A * HUBER_A                 # `b = a * a` in double
DBL_MIN = np.float64(2.2250738585072014e-308)
PIECE_THREADS = 256


def have_long_double():
    return EPS_LD < 1e-18


def check_precision():
    """the reference's own error is (eps_ld / eps) tol: below tol / 1000"""
    assert EPS_LD * 1000 <= EPS64, "np.longdouble is not an extended type here"


_DT = [LD]   # the type values are kept in: long double, or float64 for `evaluate_in(np.float64)` (the bounds stay long double)


class evaluate_in:
    """context: run edges / node_quantities / model_and_candidate in another floating-point type -- a plain float64 evaluation of
    the same expressions, which the host tests hold against the bounds before any device is"""
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        _DT.append(self.dtype)

    def __exit__(self, *a):
        _DT.pop()


class V:
    """(value, error bound in units of eps) of the module docstring; arrays broadcast"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, _DT[-1])
        self.e = np.zeros(self.v.shape, LD) if e is None else np.broadcast_to(np.asarray(e, LD), self.v.shape)

    @staticmethod
    def lift(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.lift(o)
        v = self.v + o.v
        return V(v, self.e + o.e + np.abs(v))

    def __sub__(self, o):
        o = V.lift(o)
        v = self.v - o.v
        return V(v, self.e + o.e + np.abs(v))

    def __mul__(self, o):
        o = V.lift(o)
        v = self.v * o.v
        return V(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e * LD(EPS64) + np.abs(v))

    def __neg__(self):
        return V(-self.v, self.e)

    def exact(self, c):
        """times a power of two (or -1): no rounding"""
        return V(self.v * LD(c), self.e * abs(LD(c)))

    def over(self, c):
        """divided by a constant: one rounding"""
        v = self.v / LD(c)
        return V(v, self.e / abs(LD(c)) + np.abs(v))

    def func(self, f, dfabs, ulps):
        fv = f(self.v)
        return V(fv, dfabs(self.v) * self.e + ulps * np.abs(fv))

    def sqrt(self):
        # (sqrt(0) of an exact zero -- an isolated keyframe's column norm -- is exact: e = 0 there)
        return self.func(np.sqrt, lambda x: LD(0.5) / np.sqrt(np.where(x > 0, x, LD(1))) * (x > 0), U_SQRT)

    def recip(self):
        return self.func(lambda x: LD(1) / x, lambda x: LD(1) / (x * x), U_DIV)

    def sin(self):
        return self.func(np.sin, lambda x: np.abs(np.cos(x)), U_TRIG)

    def cos(self):
        return self.func(np.cos, lambda x: np.abs(np.sin(x)), U_TRIG)

    def sum(self, axis):
        """n terms in ANY order: the terms' own bounds plus n eps M, M the sum of their absolute values"""
        n = self.v.shape[axis]
        return V(self.v.sum(axis=axis), self.e.sum(axis=axis) + n * np.abs(self.v).sum(axis=axis))

    def flat(self):
        return V(self.v.reshape(-1), self.e.reshape(-1))

    def reshape(self, *shape):
        return V(self.v.reshape(*shape), self.e.reshape(*shape))

    def where(self, cond, other):
        other = V.lift(other)
        return V(np.where(cond, self.v, other.v), np.where(cond, self.e, other.e))

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])

    def tol(self):
        return np.asarray(self.e * LD(EPS64), np.float64)


def vsum(terms):
    """sum of a short list of V (any order)"""
    return stack(terms, 0).sum(0)


def stack(vs, axis=-1):
    vs = [V.lift(x) for x in vs]
    shp = np.broadcast_shapes(*[x.v.shape for x in vs])
    return V(np.stack([np.broadcast_to(x.v, shp) for x in vs], axis), np.stack([np.broadcast_to(x.e, shp) for x in vs], axis))


def wrap(x):
    """pgNormalizeAngle: a single wrap; the +-360 is one more addition"""
    hi, lo = x.v > 180, x.v < -180
    w = x + V(np.where(hi, LD(-360), np.where(lo, LD(360), LD(0))))
    return w.where(hi | lo, x)


def _qmul(a, b):
    """dmath.hpp qmul on (x, y, z, w) tuples of V"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    w = vsum([aw * bw, -(ax * bx), -(ay * by), -(az * bz)])
    x = vsum([aw * bx, ax * bw, ay * bz, -(az * by)])
    y = vsum([aw * by, ay * bw, az * bx, -(ax * bz)])
    z = vsum([aw * bz, az * bw, ax * by, -(ay * bx)])
    return (x, y, z, w)


def _conj(q):
    return (-q[0], -q[1], -q[2], q[3])


def _quat_to_R(q):
    """dmath.hpp quatToR, row-major list of 9"""
    x, y, z, w = q
    tx, ty, tz = x.exact(2), y.exact(2), z.exact(2)
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = V(LD(1))
    return [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)]


def _ypr_to_R(yaw, pitch, roll):
    """pgYpr2R: R and dR / dyaw (per degree), row-major lists of 9"""
    def rad(a):
        return a.over(180) * V(LD(PI64))
    y, p, r = rad(yaw), rad(pitch), rad(roll)
    cy, sy, cp, sp, cr, sr = y.cos(), y.sin(), p.cos(), p.sin(), r.cos(), r.sin()
    R = [cy * cp, -(sy * cr) + cy * sp * sr, sy * sr + cy * sp * cr,
         sy * cp, cy * cr + sy * sp * sr, -(cy * sr) + sy * sp * cr,
         -sp, cp * sr, cp * cr]
    k = V(LD(K_DEG))
    zero = V(np.zeros_like(yaw.v))
    dR = [-(sy * cp) * k, (-(cy * cr) - sy * sp * sr) * k, (cy * sr - sy * sp * cr) * k,
          cy * cp * k, (-(sy * cr) + cy * sp * sr) * k, (sy * sr + cy * sp * cr) * k,
          zero, zero, zero]
    return R, dR


def _plus_mat(q):
    x, y, z, w = q
    return [[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]]


def _oplus_mat(q):
    x, y, z, w = q
    return [[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]]


def _cols(a, n):
    a = np.asarray(a, np.float64).reshape(-1, n)
    return [V(a[:, i]) for i in range(n)]


def edges(problem, states, six):
    """problem: ea eb eloop et eyaw epitch eroll eq esq; states: yaw t q (float64 data).  Returns a dict of V:
    r0 Ja0 Jb0 (before the loss; ne x R, ne x R x D), s, sc, res Ja Jb (as k_pg_eval stores them), cost_e, cost."""
    check_precision()
    ea, eb = np.asarray(problem["ea"], int), np.asarray(problem["eb"], int)
    loop = np.asarray(problem["eloop"], int) != 0
    ne = len(ea)
    D = 6 if six else 4
    t = np.asarray(states["t"], np.float64).reshape(-1, 3)
    ta, tb = _cols(t[ea], 3), _cols(t[eb], 3)
    d = [tb[i] - ta[i] for i in range(3)]
    et = _cols(problem["et"], 3)
    zero = V(np.zeros(ne))
    Ja = [[zero] * D for _ in range(D)]
    Jb = [[zero] * D for _ in range(D)]
    r = [None] * D
    if not six:
        yaw = np.asarray(states["yaw"], np.float64)
        R, dR = _ypr_to_R(V(yaw[ea]), V(np.asarray(problem["epitch"], np.float64)), V(np.asarray(problem["eroll"], np.float64)))
        wy = V(np.where(loop, np.float64(0.1), np.float64(1.0)))
        for k in range(3):   # the weight wt = 1.0 multiplies exactly
            r[k] = vsum([R[k] * d[0], R[3 + k] * d[1], R[6 + k] * d[2]]) - et[k]
            Ja[k][0] = vsum([dR[k] * d[0], dR[3 + k] * d[1], dR[6 + k] * d[2]])
            for c in range(3):
                Ja[k][1 + c] = -R[c * 3 + k]
                Jb[k][1 + c] = R[c * 3 + k]
        r[3] = wrap(V(yaw[eb]) - V(yaw[ea]) - V(np.asarray(problem["eyaw"], np.float64))) * wy
        Ja[3][0], Jb[3][0] = -wy, wy
    else:
        q = np.asarray(states["q"], np.float64).reshape(-1, 4)
        qa, qb, qm = tuple(_cols(q[ea], 4)), tuple(_cols(q[eb], 4)), tuple(_cols(problem["eq"], 4))
        si = _cols(problem["esq"], 6)
        Ra = _quat_to_R(qa)
        pab = [vsum([Ra[k] * d[0], Ra[3 + k] * d[1], Ra[6 + k] * d[2]]) for k in range(3)]
        dq = _qmul(qm, _conj(_qmul(_conj(qa), qb)))
        u = [pab[0] - et[0], pab[1] - et[1], pab[2] - et[2], dq[0].exact(2), dq[1].exact(2), dq[2].exact(2)]
        for k in range(6):
            r[k] = si[k] * u[k]
        dx = [[zero, -d[2], d[1]], [d[2], zero, -d[0]], [-d[1], d[0], zero]]
        for k in range(3):
            for c in range(3):
                rt = Ra[c * 3 + k]
                Ja[k][c] = -(rt * si[k])
                Jb[k][c] = rt * si[k]
                Ja[k][3 + c] = (vsum([Ra[j * 3 + k] * dx[j][c] for j in range(3)]) * si[k]).exact(2)
        PA, OB = _plus_mat(_qmul(qm, _conj(qb))), _oplus_mat(qa)
        for k in range(3):
            for c in range(3):
                s_ = vsum([PA[k][j] * OB[j][c] for j in range(4)]) * si[3 + k]
                Ja[3 + k][3 + c] = s_.exact(2)
                Jb[3 + k][3 + c] = s_.exact(-2)
    r0 = stack(r)
    Ja0 = stack([stack(row) for row in Ja], axis=1)
    Jb0 = stack([stack(row) for row in Jb], axis=1)
    s = (r0 * r0).sum(1)
    out = loop & (s.v > LD(HUBER_B))
    s_safe = s.where(out, V(np.ones(ne)))
    rt = s_safe.sqrt()
    a, b = V(LD(HUBER_A)), V(LD(HUBER_B))
    cost_out = ((a * rt).exact(2) - b).exact(0.5)
    ratio = a * rt.recip()
    ratio = ratio.where(ratio.v > LD(DBL_MIN), V(LD(DBL_MIN)))
    sc = ratio.sqrt().where(out, V(np.ones(ne)))
    cost_e = cost_out.where(out, s.exact(0.5))
    # sc = 1.0 multiplies exactly: no rounding where the corrector is off
    res = (r0 * sc[:, None]).where(out[:, None], r0)
    JaR = (Ja0 * sc[:, None, None]).where(out[:, None, None], Ja0)
    JbR = (Jb0 * sc[:, None, None]).where(out[:, None, None], Jb0)
    return dict(r0=r0, Ja0=Ja0, Jb0=Jb0, s=s, sc=sc, outside=out, res=res, Ja=JaR, Jb=JbR, cost_e=cost_e, cost=cost_e.sum(0))


def incident(problem):
    """nodePtr / nodeEdge of optimize(): per node the incident (edge, side) in edge order"""
    ea, eb = np.asarray(problem["ea"], int), np.asarray(problem["eb"], int)
    nn = len(problem["off"])
    inc = [[] for _ in range(nn)]
    for e in range(len(ea)):
        inc[ea[e]].append((e, 0))
        inc[eb[e]].append((e, 1))
    return inc


def _dense_jacobian(problem, Ja, Jb, D, absolute=False):
    """(ne R) x n Jacobian in tangent order from the per-edge blocks (long double)"""
    ea, eb, off = np.asarray(problem["ea"], int), np.asarray(problem["eb"], int), np.asarray(problem["off"], int)
    ne = len(ea)
    n = int(np.sum(off >= 0)) * D
    Ja = np.asarray(Ja, LD).reshape(ne, D, D)
    Jb = np.asarray(Jb, LD).reshape(ne, D, D)
    J = np.zeros((ne * D, n), LD)
    for e in range(ne):
        for node, blk in ((ea[e], Ja[e]), (eb[e], Jb[e])):
            if off[node] >= 0:
                J[e * D:(e + 1) * D, off[node]:off[node] + D] += np.abs(blk) if absolute else blk
    return J


def node_quantities(res, Ja, Jb, problem, six):
    """k_pg_node on the stored res, Ja, Jb (data).  Returns dict of (value, tol): g, colsq, scale (n), blk (nn x D x D, lower
    triangle, zero elsewhere and on constant nodes), gradmax.  A sum of n = R * degree products of data: k = n + 1."""
    check_precision()
    D = 6 if six else 4
    off = np.asarray(problem["off"], int)
    nn = len(off)
    n = int(np.sum(off >= 0)) * D
    DT = _DT[-1]
    res = np.asarray(res, DT).reshape(-1, D)
    Ja = np.asarray(Ja, DT).reshape(-1, D, D)
    Jb = np.asarray(Jb, DT).reshape(-1, D, D)
    g, gM = np.zeros(n, DT), np.zeros(n, LD)
    blk, blkM = np.zeros((nn, D, D), DT), np.zeros((nn, D, D), LD)
    kk = np.zeros(nn, np.int64)
    for k, inc in enumerate(incident(problem)):
        if off[k] < 0:
            continue
        o = off[k]
        for e, side in inc:
            J = (Jb if side else Ja)[e]
            g[o:o + D] += J.T @ res[e]
            gM[o:o + D] += np.abs(J.astype(LD)).T @ np.abs(res[e].astype(LD))
            blk[k] += J.T @ J
            blkM[k] += np.abs(J.astype(LD)).T @ np.abs(J.astype(LD))
        kk[k] = D * len(inc) + 1
    low = np.tril(np.ones((D, D), bool))
    blk, blkM = np.where(low, blk, 0), np.where(low, blkM, 0)
    kn = np.repeat(kk[off >= 0], D)
    tol_g = np.asarray(kn * LD(EPS64) * gM, np.float64)
    tol_blk = np.asarray(kk[:, None, None] * LD(EPS64) * blkM, np.float64)
    colsq = np.concatenate([np.diag(blk[k]) for k in range(nn) if off[k] >= 0]) if n else np.zeros(0, LD)
    tol_colsq = np.concatenate([np.diag(tol_blk[k]) for k in range(nn) if off[k] >= 0]) if n else np.zeros(0)
    c = V(colsq, kn * colsq)         # non-negative terms: M = the value
    scale = (V(LD(1)) + c.sqrt()).recip()
    gmax = np.max(np.abs(g)) if n else LD(0)
    return dict(g=(g, tol_g), blk=(blk, tol_blk), colsq=(colsq, tol_colsq), scale=(scale.v, scale.tol()),
                gradmax=(gmax, float(np.max(tol_g)) if n else 0.0))


def normal_matrix(problem, Ja, Jb, res, D, absolute=False):
    """J^T J (dense, tangent order) and J^T r accumulated block by block in long double"""
    ea, eb, off = np.asarray(problem["ea"], int), np.asarray(problem["eb"], int), np.asarray(problem["off"], int)
    ne = len(ea)
    n = int(np.sum(off >= 0)) * D
    Ja, Jb, res = np.asarray(Ja, LD).reshape(ne, D, D), np.asarray(Jb, LD).reshape(ne, D, D), np.asarray(res, LD).reshape(ne, D)
    if absolute:
        Ja, Jb, res = np.abs(Ja), np.abs(Jb), np.abs(res)
    H, g = np.zeros((n, n), LD), np.zeros(n, LD)
    for e in range(ne):
        oa, ob = off[ea[e]], off[eb[e]]
        if oa >= 0:
            H[oa:oa + D, oa:oa + D] += Ja[e].T @ Ja[e]
            g[oa:oa + D] += Ja[e].T @ res[e]
        if ob >= 0:
            H[ob:ob + D, ob:ob + D] += Jb[e].T @ Jb[e]
            g[ob:ob + D] += Jb[e].T @ res[e]
        if oa >= 0 and ob >= 0:
            blk = Jb[e].T @ Ja[e]
            H[ob:ob + D, oa:oa + D] += blk
            H[oa:oa + D, ob:ob + D] += blk.T
    return H, g


def system(Ja, Jb, res, scale, problem, six, radius):
    """dense damped scaled normal equations in tangent order from the stored (robustified) blocks and the scales (data)"""
    D = 6 if six else 4
    H, g = normal_matrix(problem, Ja, Jb, res, D)
    s = np.asarray(scale, LD)
    A = H * s[:, None] * s[None, :]
    damp = np.minimum(np.maximum(np.diag(H) * s * s, LD(1e-6)), LD(1e32)) / LD(radius)
    A[np.diag_indices_from(A)] += damp
    return A, g * s


def cholesky_ld(A):
    """lower Cholesky factor, left-looking, one column per step"""
    A = np.asarray(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not c[0] > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        L[j:, j] = c / np.sqrt(c[0])
    return L


def solve(A, b):
    L = cholesky_ld(A)
    n = len(b)
    z = np.zeros(n, LD)
    for i in range(n):
        z[i] = (b[i] - L[i, :i] @ z[:i]) / L[i, i]
    x = np.zeros(n, LD)
    for i in range(n - 1, -1, -1):
        x[i] = (z[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def norm2(A):
    return float(np.linalg.norm(np.asarray(A, np.float64), 2))


def eta(A, b, y, normA=None):
    """normwise backward error, residual in long double"""
    y = np.asarray(y, LD)
    r = np.asarray(b, LD) - np.asarray(A, LD) @ y
    normA = norm2(A) if normA is None else normA
    den = normA * float(np.sqrt(y @ y)) + float(np.sqrt(np.asarray(b, LD) @ np.asarray(b, LD)))
    return float(np.sqrt(r @ r)) / den if den > 0 else 0.0


def eta_ceiling(n, R):
    return n * (3 * n + 1 + C_RSQ + R + 4) * EPS64


def kappa2(A):
    w = np.linalg.eigvalsh(np.asarray(A, np.float64))
    return float(w[-1] / w[0]) if w[0] > 0 else float("inf")


def lapack_solve(A, b):
    return np.linalg.solve(np.asarray(A, np.float64), np.asarray(b, np.float64))


def model_and_candidate(y, scale, res, Ja, Jb, problem, states, six, cand_states=None):
    """k_pg_model_plus from the device's y, scale, res, Ja, Jb (data).  Returns dict of V: model, yawC, tC, qC, step2, x2 and,
    when cand_states (the candidate the evaluation consumed) is given, costC = edges(cand_states)['cost']."""
    check_precision()
    D = 6 if six else 4
    ea, eb, off = np.asarray(problem["ea"], int), np.asarray(problem["eb"], int), np.asarray(problem["off"], int)
    ne, nn = len(ea), len(off)
    free = off >= 0
    delta = -(V(np.asarray(y, np.float64)) * V(np.asarray(scale, np.float64)))       # n
    dn = V(np.zeros((nn, D)))                                                        # per node, zero on constant nodes
    idx = np.where(free, off, 0)[:, None] + np.arange(D)[None, :]
    dn = delta[idx].where(free[:, None], dn)
    Ja = V(np.asarray(Ja, np.float64).reshape(ne, D, D))
    Jb = V(np.asarray(Jb, np.float64).reshape(ne, D, D))
    r = V(np.asarray(res, np.float64).reshape(ne, D))
    da, db = dn[ea], dn[eb]
    prod = stack([Ja * da[:, None, :], Jb * db[:, None, :]], axis=-1)               # ne x R x D x 2
    mr = prod.reshape(ne, D, 2 * D).sum(2)
    term = mr * (r + mr.exact(0.5))
    model = term.flat().sum(0)
    out = dict(model=model, mr=mr, delta=delta)
    t0 = V(np.asarray(states["t"], np.float64).reshape(nn, 3))
    zero = V(np.zeros(nn))
    if not six:
        y0 = V(np.asarray(states["yaw"], np.float64))
        y1 = wrap(y0 + dn[:, 0]).where(free, y0)
        t1 = (t0 + dn[:, 1:4]).where(free[:, None], t0)
        diffs = stack([y1 - y0] + [t1[:, c] - t0[:, c] for c in range(3)])
        xs = stack([y0] + [t0[:, c] for c in range(3)])
        out.update(yawC=y1, tC=t1)
    else:
        t1 = (t0 + dn[:, 0:3]).where(free[:, None], t0)
        q0 = V(np.asarray(states["q"], np.float64).reshape(nn, 4))
        d3 = dn[:, 3:6]
        nd2 = (d3 * d3).sum(1)
        moved = free & (nd2.v > 0)
        nd = nd2.where(moved, V(np.ones(nn))).sqrt()
        s = nd.sin() * nd.recip()
        dq = (s * d3[:, 0], s * d3[:, 1], s * d3[:, 2], nd.cos())
        q1 = stack(list(_qmul(dq, (q0[:, 0], q0[:, 1], q0[:, 2], q0[:, 3])))).where(moved[:, None], q0)
        diffs = stack([t1[:, c] - t0[:, c] for c in range(3)] + [q1[:, c] - q0[:, c] for c in range(4)])
        xs = stack([t0[:, c] for c in range(3)] + [q0[:, c] for c in range(4)])
        out.update(tC=t1, qC=q1)
    sq, xq = diffs * diffs, xs * xs
    sq, xq = sq.where(free[:, None], zero[:, None]), xq.where(free[:, None], zero[:, None])
    out["step2"] = sq.flat().sum(0)
    out["x2"] = xq.flat().sum(0)
    if cand_states is not None:
        out["costC"] = edges(problem, cand_states, six)["cost"]
    return out


def partition(problem, six, piece_keyframes, dense_keyframes, levels, level2_piece_keyframes):
    """the host's symbolic step restated: separators = cuts of w keyframes + a vertex cover of the long edges, pieces closed by
    length or by the separators they touch, level 2 over the cut keyframes with its validation and fall-back.
    piece_keyframes / level2_piece_keyframes: the values in force (defaults 32 / 64 and 16 / 32 resolved by the caller)."""
    D = 6 if six else 4
    w = 4 if six else 2
    ea, eb, off = [int(x) for x in problem["ea"]], [int(x) for x in problem["eb"]], np.asarray(problem["off"], int)
    nn, ne = len(off), len(ea)
    inc = incident(problem)
    piece_len = max(8, min(piece_keyframes, 256 // D))
    l2_len = max(8, min(level2_piece_keyframes, 256 // D))
    max_adj = (PIECE_THREADS - 1) // D
    free_nodes = [k for k in range(nn) if off[k] >= 0]
    pos = {k: i for i, k in enumerate(free_nodes)}
    F = len(free_nodes)
    is_sep, is_cover, piece_of = np.zeros(nn, int), np.zeros(nn, int), -np.ones(nn, int)
    n_pieces = 0
    if F <= dense_keyframes:
        is_sep[free_nodes] = 1
    else:
        def is_long(e):
            return ea[e] in pos and eb[e] in pos and abs(pos[ea[e]] - pos[eb[e]]) > w
        long_deg = np.zeros(nn, int)
        for e in range(ne):
            if is_long(e):
                long_deg[ea[e]] += 1
                long_deg[eb[e]] += 1
        for e in range(ne):
            if is_long(e) and not is_sep[ea[e]] and not is_sep[eb[e]]:
                c = ea[e] if long_deg[ea[e]] >= long_deg[eb[e]] else eb[e]
                is_sep[c] = is_cover[c] = 1
        stamp = -np.ones(nn, int)
        cnt, adj, i = 0, 2 * w, 0
        while i < F:
            k = free_nodes[i]
            if is_sep[k]:
                if stamp[k] != n_pieces:
                    stamp[k] = n_pieces
                    adj += 1
                i += 1
                continue
            piece_of[k] = n_pieces
            cnt += 1
            for e, side in inc[k]:
                o = ea[e] if side else eb[e]
                if o in pos and is_sep[o] and stamp[o] != n_pieces:
                    stamp[o] = n_pieces
                    adj += 1
            if (cnt >= piece_len or adj + 1 >= max_adj) and i + w < F - 1:
                for j in range(1, w + 1):
                    is_sep[free_nodes[i + j]] = 1
                i += w
                n_pieces += 1
                cnt, adj = 0, 2 * w
            i += 1
        if cnt > 0 or any(piece_of[k] == n_pieces for k in free_nodes):
            n_pieces += 1
    W2 = 2 * w - 1
    piece_adj = [set() for _ in range(n_pieces)]
    for e in range(ne):
        a, b = ea[e], eb[e]
        if a not in pos or b not in pos:
            continue
        assert is_sep[a] or is_sep[b] or piece_of[a] == piece_of[b], "partition left an edge between two pieces"
        if not is_sep[a] and is_sep[b]:
            piece_adj[piece_of[a]].add(b)
        if not is_sep[b] and is_sep[a]:
            piece_adj[piece_of[b]].add(a)
    l2_piece_of, is_root = -np.ones(nn, int), np.zeros(nn, int)
    n_pieces2 = 0
    cut_list = [k for k in free_nodes if is_sep[k] and not is_cover[k]]
    use_l2 = levels == 2 and n_pieces >= 8 and len(cut_list) >= 3 * l2_len
    requested_l2 = use_l2
    sep_adj = [set() for _ in range(nn)]
    if use_l2:
        for A in piece_adj:
            for x in A:
                sep_adj[x] |= A - {x}
        for e in range(ne):
            a, b = ea[e], eb[e]
            if a in pos and b in pos and is_sep[a] and is_sep[b]:
                sep_adj[a].add(b)
                sep_adj[b].add(a)
        stamp = -np.ones(nn, int)
        is_l2_cut = np.zeros(nn, int)
        cnt, adj, C, i = 0, 2 * W2, len(cut_list), 0
        while i < C:
            k = cut_list[i]
            l2_piece_of[k] = n_pieces2
            cnt += 1
            for o in sorted(sep_adj[k]):
                if is_cover[o] and stamp[o] != n_pieces2:
                    stamp[o] = n_pieces2
                    adj += 1
            if (cnt >= l2_len or adj + 12 >= max_adj) and i + W2 < C - 1:
                for j in range(1, W2 + 1):
                    is_l2_cut[cut_list[i + j]] = 1
                i += W2
                n_pieces2 += 1
                cnt, adj = 0, 2 * W2
            i += 1
        if cnt > 0:
            n_pieces2 += 1
        for k in free_nodes:
            if is_sep[k] and (is_cover[k] or is_l2_cut[k]):
                is_root[k] = 1
                l2_piece_of[k] = -1
        rank, r = {}, 0
        for k in cut_list:
            if not is_root[k]:
                rank[k] = r
                r += 1
        a2 = [set() for _ in range(n_pieces2)]
        for k in cut_list:
            if is_root[k]:
                continue
            for o in sep_adj[k]:
                if is_root[o]:
                    a2[l2_piece_of[k]].add(o)
                elif l2_piece_of[o] != l2_piece_of[k] or abs(rank[o] - rank[k]) > W2:
                    use_l2 = False
        for A in a2:
            if len(A) * D + 1 > PIECE_THREADS:
                use_l2 = False
        if n_pieces2 < 2:
            use_l2 = False
    if not use_l2:
        n_pieces2 = 0
        l2_piece_of[:] = -1
        is_root = is_sep.copy()
    sep_off, node_row = -np.ones(nn, int), -np.ones(nn, int)
    nS = 0
    for k in free_nodes:
        if is_sep[k] and not is_root[k]:
            sep_off[k] = nS
            nS += D
    off_r = nS
    for k in free_nodes:
        if is_sep[k] and is_root[k]:
            sep_off[k] = nS
            nS += D
    rows = [0] * n_pieces
    for k in free_nodes:
        if not is_sep[k]:
            node_row[k] = rows[piece_of[k]]
            rows[piece_of[k]] += D
    cols = [len(A) * D + 1 for A in piece_adj]
    rows2, adj2 = [0] * n_pieces2, [set() for _ in range(n_pieces2)]
    for k in free_nodes:
        if l2_piece_of[k] >= 0:
            rows2[l2_piece_of[k]] += D
            adj2[l2_piece_of[k]] |= {o for o in sep_adj[k] if is_root[o]}
    cols2 = [len(A) * D + 1 for A in adj2]
    node_piece = np.where(is_sep == 1, -1, piece_of)
    return dict(rows=np.array(rows, int), cols=np.array(cols, int), rows2=np.array(rows2, int), cols2=np.array(cols2, int),
                sepOff=sep_off, nodePiece=node_piece, nodeRow=node_row, isCover=is_cover, isRoot=is_root, l2PieceOf=l2_piece_of,
                nS=nS, nR=nS - off_r, nPieces=n_pieces, nPieces2=n_pieces2, BW=w * D + D - 1, BW2=W2 * D + D - 1,
                isSep=is_sep, level2_requested=bool(requested_l2), piece_adj=[sorted(A) for A in piece_adj])


PARTITION_KEYS = ("rows", "cols", "rows2", "cols2", "sepOff", "nodePiece", "nodeRow", "isCover", "isRoot", "l2PieceOf",
                  "nS", "nR", "nPieces", "nPieces2", "BW", "BW2")


# ---------------------------------------------------------------- the comparisons of tests/test_gpu_posegraph_stages.py
def assert_close(name, got, ref, tol):
    """every entry of a float64 result within its own bound of the long-double value"""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, LD).reshape(got.shape)
    tol = np.broadcast_to(np.asarray(tol, np.float64), np.shape(ref)).reshape(got.shape)
    err = np.abs(np.asarray(got, LD) - ref)
    bad = ~(err <= tol)
    if np.any(bad):
        i = int(np.argmax(np.where(bad, err - tol, -np.inf)))
        raise AssertionError("%s: entry %d is %.17g, reference %.17g, off by %.3e > bound %.3e (%d of %d entries out)" %
                             (name, i, got.reshape(-1)[i], float(ref.reshape(-1)[i]), float(err.reshape(-1)[i]), tol.reshape(-1)[i],
                              int(bad.sum()), bad.size))


def check_evaluation(cap, six):
    """stage 1: the device's res, Ja, Jb and cost against edges()"""
    E = edges(cap, cap, six)
    assert_close("res", cap["res"], E["res"].v.reshape(-1), E["res"].tol().reshape(-1))
    assert_close("Ja", cap["Ja"], E["Ja"].v.reshape(-1), E["Ja"].tol().reshape(-1))
    assert_close("Jb", cap["Jb"], E["Jb"].v.reshape(-1), E["Jb"].tol().reshape(-1))
    assert_close("cost", cap["cost"], E["cost"].v, E["cost"].tol())
    return E


def check_node_pass(cap, six):
    """stage 2: g, colsq, nodeBlk, scale, gradmax against node_quantities() of the device's own res, Ja, Jb"""
    N = node_quantities(cap["res"], cap["Ja"], cap["Jb"], cap, six)
    assert_close("g", cap["g"], *N["g"])
    assert_close("colsq", cap["colsq"], *N["colsq"])
    assert_close("nodeBlk", cap["nodeBlk"], N["blk"][0].reshape(-1), N["blk"][1].reshape(-1))
    assert_close("scale", cap["scale"], *N["scale"])
    assert_close("gradmax", cap["gradmax"], *N["gradmax"])
    return N


def check_solve(cap, six, radius, verbose=None):
    """stage 3: backward error of the device's y under the derived ceiling and the measured bar, forward error under
    kappa times the bar.  Returns (eta_device, eta_lapack, kappa, forward error)."""
    D = 6 if six else 4
    A, b = system(cap["Ja"], cap["Jb"], cap["res"], cap["scale"], cap, six, radius)
    n = len(b)
    nA = norm2(A)
    y = np.asarray(cap["y"], np.float64)
    assert np.all(np.isfinite(y)), "y is not finite"
    eta_dev = eta(A, b, y, nA)
    eta_lap = eta(A, b, lapack_solve(A, b), nA)
    y_ld = solve(A, b)
    kap = kappa2(A)
    ny = float(np.sqrt(y_ld @ y_ld))
    fwd = float(np.sqrt(np.sum((np.asarray(y, LD) - y_ld) ** 2))) / ny if ny > 0 else float(np.max(np.abs(y)))
    bar = ETA_MARGIN * max(eta_lap, EPS64)
    if verbose is not None:
        print("%s: n %d eta(device) %.3e eta(LAPACK) %.3e ratio %.2f ceiling %.3e kappa %.3e forward %.3e" %
              (verbose, n, eta_dev, eta_lap, eta_dev / max(eta_lap, EPS64), eta_ceiling(n, D), kap, fwd))
    assert eta_dev <= bar, "backward error %.3e above %d x max(eta(LAPACK) = %.3e, eps)" % (eta_dev, ETA_MARGIN, eta_lap)
    assert eta_dev <= eta_ceiling(n, D), "backward error %.3e above the a-priori ceiling %.3e" % (eta_dev, eta_ceiling(n, D))
    assert fwd <= kap * bar, "forward error %.3e above kappa (%.3e) x bar (%.3e)" % (fwd, kap, bar)
    return eta_dev, eta_lap, kap, fwd


def check_model_and_candidate(cap, six):
    """stage 4: the scalars and the candidate against model_and_candidate() of the device's own y; the candidate's cost is
    evaluated at the device's candidate (what the candidate evaluation consumed)"""
    cand = dict(yaw=cap["yawC"], t=cap["tC"], q=cap["qC"])
    M = model_and_candidate(cap["y"], cap["scale"], cap["res"], cap["Ja"], cap["Jb"], cap, cap, six, cand_states=cand)
    assert np.isfinite(cap["step2"]), "step^2 is not finite"
    assert_close("model", cap["model"], M["model"].v, M["model"].tol())
    if six:
        assert_close("qC", cap["qC"], M["qC"].v.reshape(-1), M["qC"].tol().reshape(-1))
    else:
        assert_close("yawC", cap["yawC"], M["yawC"].v, M["yawC"].tol())
    assert_close("tC", cap["tC"], M["tC"].v.reshape(-1), M["tC"].tol().reshape(-1))
    assert_close("step2", cap["step2"], M["step2"].v, M["step2"].tol())
    assert_close("x2", cap["x2"], M["x2"].v, M["x2"].tol())
    assert_close("costC", cap["costC"], M["costC"].v, M["costC"].tol())
    return M


def check_partition(cap, part):
    """the captured partition against the restatement, array by array"""
    for key in PARTITION_KEYS:
        a, b = np.atleast_1d(np.asarray(cap[key])), np.atleast_1d(np.asarray(part[key]))
        assert a.shape == b.shape and np.array_equal(a, b), "partition array %s differs from the restatement" % key
