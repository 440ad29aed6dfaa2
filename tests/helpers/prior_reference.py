"""Long-double reference of the marginalisation prior AWAY from its linearisation point (K3: priorEvalBlock, priorAccumulateBlock,
the last block of k_post_solve), with an a-priori rounding bound for every quantity, built the way schur_reference builds its own:
the terms of every sum are counted and a float64 evaluation of a sum of n terms of absolute sum M in ANY order errs by at most
(n + C0) eps M (Higham 3.1 / 3.3; eps = 2^-52 = two unit roundoffs, C0 = schur_reference.C0 = 8 roundings to spare for what is done
inside a term).  Nothing is imported from the product and nothing is read off the kernel: the definitions are the reference's.

  PoseManifold::minus           dchi = [ r - r_lin ; 2 vec(q * q_lin^-1) ],  q_lin^-1 = conj(q_lin) / |q_lin|^2 (Eigen's inverse()),
                                no sign canonicalisation: a stored -q gives the vector part of -(q * q_lin^-1) as it comes.
  PoseManifold::liftJacobian    at the RAW linearisation quaternion: lift = blockdiag(I3, 2 [oplus(conj(q_lin))]_(3 x 4))
  Transformation::oplusJacobian at the NORMALISED current quaternion qn = q / |q|: plus = blockdiag(I3, 0.5 [oplus(qn)]_(4 x 3))
  MarginalizationError::EvaluateWithMinimalJacobians   e = e0 + J dchi, J_i = Jmin_i lift(x_lin), which Ceres multiplies by
                                PlusJacobian(x): the tangent map of a pose / extrinsics block is
                                    M = lift(x_lin) plus(x) = blockdiag(I3, M3),  M3 = [oplus(conj(q_lin))]_(3 x 4) [oplus(qn)]_(4 x 3)
  (oplus(q) p = p * q, operators.hpp; quaternions as x y z w.)  A speed / bias block: dchi = x - x_lin, M = I.  A block with mdim = 0
  has no rows.  With H = J^T J, b = J^T e0, c0 = e0 . e0 -- the form the solver holds -- the prior contributes
      grad = b + H dchi,   cost = 0.5 c0 + b . dchi + 0.5 dchi^T H dchi,   M^T H M to the normal equations,   M^T grad to the gradient,
  rows of constant blocks left out of the last two (their dchi still enters grad), and to the post-solve sums
      (Mv)^T H (Mv), (My)^T H (My), (Mv)^T H (My), (Mv)^T grad, (My)^T grad      with v, y the prior's rows of v_C, y_C (0 on constant blocks).

Inputs are data: H, b, c0 as the device holds them, the blocks' linearisation points (svin_ba_get_prior_lin) and current values.
Where the caller only has J and e0 (the oracle's prior; a device prior from the eigen-solve, whose H-space form is computed on the
device from them) it forms H, b, c0 in long double and hands over what a float64 evaluation of THEM may differ by,
dH = (m + C0) eps |J|^T |J|, db = (m + C0) eps |J|^T |e0|, dc0 = (m + C0) eps c0 (`from_factor`); they are propagated like any other
first-order perturbation of a datum.

The bound, quantity by quantity (first order in eps throughout)
  dchi      translation, speed / bias: one rounded subtraction, t_dchi = eps |dchi|.  Rotation: component k is
            2 sum_4 q_a (conj(q_lin) / |q_lin|^2)_b, four products of magnitude at most |q| |q_lin^-1|; inside a term the norm (7
            roundings), the division and the product: t_dchi = (4 + C0) eps 2 sum_4 |q_a| |q_lin^-1,b|.
  M3        entry (a, c) = sum_4 oplus(conj(q_lin))_ak oplus(qn)_kc, the first factor exact, the second carrying the normalisation of q
            (4 squares, 3 additions, a square root, a division: 9 roundings = 4.5 eps), then the product and the accumulation:
            t_M = (4 + C0) eps (|oplus(conj q_lin)| |oplus(qn)|)_ac.
  grad_i    m + 1 terms: (m + 1 + C0) eps (|b_i| + (|H| |dchi|)_i)  +  (|H| t_dchi)_i  [+ db_i + (dH |dchi|)_i]
  cost      m^2 + m + 1 terms of absolute sum Mc = 0.5 |c0| + |b| . |dchi| + 0.5 |dchi|^T |H| |dchi|:
            (m^2 + m + 1 + C0) eps Mc  +  t_dchi . |grad|   (d cost / d dchi = grad)   [+ 0.5 dc0 + |dchi| . db + 0.5 |dchi|^T dH |dchi|]
  M^T H M   entry (i, j): n_ij = c_i c_j terms (c = 3 for a rotation row, else 1; at most 9) of absolute sum (|M|^T |H| |M|)_ij:
            accumulated with everything else that lands on the entry (schur_reference.assemble adds n and M to its own), plus the
            propagated part P_S = t_M^T |H| |M| + |M|^T |H| t_M [+ |M|^T dH |M|]
  M^T grad  c_i terms of absolute sum (|M|^T |grad|)_i, propagated part P_g = t_M^T |grad| + |M|^T t_grad
  post-solve  Mv: c terms, t_Mv = (3 + C0) eps |M| |v| + t_M |v| + |M| t_v (y is data: no t_y); a quadratic sum has m^2 terms of absolute
            sum |Mv|^T |H| |My| and the propagated part t_Mv^T |H| |My| + |Mv|^T |H| t_My [+ |Mv|^T dH |My|]; a dot product with grad
            m terms of absolute sum |Mv| . |grad| and t_Mv . |grad| + |Mv| . t_grad.
The bounds are wide where the information is large (a row with H_ii ~ 1e16 tolerates an absolute error of about 1e16 eps |dchi|): that is
what float64 can deliver there, and tests/test_prior_reference_host.py shows that they are nevertheless tight enough to catch a
transposed, dropped, or wrongly normalised M3, a missing factor 2, a gradient without H dchi, a cost without its quadratic term and a
constant block's rows that were not skipped, on every moved case the GPU tests use.
The same bounds with the long-double eps hold for this reference itself (asserted below tol / 1000 by the callers' ref_ratio).
"""
import numpy as np

import schur_reference as sr

LD = sr.LD
EPS = sr.EPS64
C0 = sr.C0
KIND_OF = {0: "p", 1: "e", 2: "s"}


def oplus(q):
    """oplus(q) p = p * q for quaternions as (x, y, z, w) (operators.hpp)"""
    x, y, z, w = q
    return np.array([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]], dtype=np.asarray(q).dtype)


def from_factor(J, e0, dtype=LD):
    """H, b, c0 of a prior given as J, e0, in `dtype`, with what a float64 evaluation of them may differ by: (H, b, c0, dH, db, dc0)"""
    J, e0 = np.asarray(J, dtype), np.asarray(e0, dtype)
    m = len(e0)
    aJ = np.abs(J)
    c0 = e0 @ e0
    return J.T @ J, J.T @ e0, c0, EPS * (m + C0) * (aJ.T @ aJ), EPS * (m + C0) * (aJ.T @ np.abs(e0)), EPS * (m + C0) * c0


def moved(H, b, c0, blocks, columns, dH=None, db=None, dc0=0.0, dtype=LD):
    """H (m x m), b (m), c0: the prior's quadratic form (grad = b + H dchi, cost = 0.5 c0 + ...).
    blocks: [dict(kind "p" | "e" | "s", ordering, mdim, lin (the linearisation point), x (the current value))].
    columns[i]: the reduced system's row of the prior's row i, or -1 (a constant block).
    Returns a dict, everything over the prior's own m rows and in `dtype` unless it is a bound (float64):
    dchi, t_dchi, M (m x m), t_M, grad, t_grad, cost, tol_cost, S = M^T H M with n_S / M_S / P_S, g = M^T grad with n_g / M_g / P_g."""
    T = dtype
    H, b, c0 = np.asarray(H, T), np.asarray(b, T), T(c0)
    m = len(b)
    aH = np.abs(H)
    dH = np.zeros((m, m), T) if dH is None else np.asarray(dH, T)
    db = np.zeros(m, T) if db is None else np.asarray(db, T)
    dchi, t_dchi = np.zeros(m, T), np.zeros(m, T)
    M, t_M, cnt = np.eye(m, dtype=T), np.zeros((m, m), T), np.ones(m, np.int64)
    seen = np.zeros(m, bool)
    for blk in blocks:
        o, md = int(blk["ordering"]), int(blk["mdim"])
        if md == 0:
            continue
        assert md == (9 if blk["kind"] == "s" else 6) and not seen[o:o + md].any(), blk
        seen[o:o + md] = True
        x, lin = np.asarray(blk["x"], T), np.asarray(blk["lin"], T)
        if blk["kind"] == "s":
            dchi[o:o + 9] = x[:9] - lin[:9]
            t_dchi[o:o + 9] = EPS * np.abs(dchi[o:o + 9])
            continue
        dchi[o:o + 3] = x[:3] - lin[:3]
        t_dchi[o:o + 3] = EPS * np.abs(dchi[o:o + 3])
        q, ql = x[3:7], lin[3:7]
        conj = np.array([-ql[0], -ql[1], -ql[2], ql[3]], T)
        O = oplus(conj / (ql @ ql))            # q * q_lin^-1 = oplus(q_lin^-1) q
        dchi[o + 3:o + 6] = 2 * (O[:3] @ q)
        t_dchi[o + 3:o + 6] = EPS * (4 + C0) * 2 * (np.abs(O[:3]) @ np.abs(q))
        A, B = oplus(conj), oplus(q / np.sqrt(q @ q))
        M[o + 3:o + 6, o + 3:o + 6] = A[:3] @ B[:, :3]
        t_M[o + 3:o + 6, o + 3:o + 6] = EPS * (4 + C0) * (np.abs(A[:3]) @ np.abs(B[:, :3]))
        cnt[o + 3:o + 6] = 3
    assert seen.all(), "rows of the prior without a block"
    ad = np.abs(dchi)
    grad = b + H @ dchi
    t_grad = EPS * (m + 1 + C0) * (np.abs(b) + aH @ ad) + aH @ t_dchi + db + dH @ ad
    ag = np.abs(grad)
    cost = T(0.5) * c0 + dchi @ b + T(0.5) * (dchi @ (H @ dchi))
    Mc = T(0.5) * abs(c0) + ad @ np.abs(b) + T(0.5) * (ad @ (aH @ ad))
    tol_cost = EPS * (m * m + m + 1 + C0) * Mc + t_dchi @ ag + T(0.5) * T(dc0) + ad @ db + T(0.5) * (ad @ (dH @ ad))
    aM = np.abs(M)
    out = dict(m=m, columns=np.asarray(columns, np.int64), H=H, dH=dH, dchi=dchi, t_dchi=np.asarray(t_dchi, np.float64), M=M,
               t_M=np.asarray(t_M, np.float64), count=cnt, grad=grad, t_grad=np.asarray(t_grad, np.float64), cost=cost,
               tol_cost=float(tol_cost), M_cost=float(Mc),
               S=M.T @ H @ M, n_S=np.outer(cnt, cnt), M_S=aM.T @ aH @ aM, P_S=t_M.T @ aH @ aM + aM.T @ aH @ t_M + aM.T @ dH @ aM,
               g=M.T @ grad, n_g=cnt.copy(), M_g=aM.T @ ag, P_g=t_M.T @ ag + aM.T @ t_grad)
    assert len(out["columns"]) == m
    return out


def post_sums(pr, v_C, y_C, tol_vC):
    """the prior's part of the five post-solve sums at the reduced system's vectors v_C (with its bound) and y_C (data):
    {name: (value, propagated bound, absolute sum, number of terms)} and (Mv, My)"""
    T = pr["M"].dtype.type
    m, pc = pr["m"], pr["columns"]
    sel = pc >= 0
    v, y, tv = np.zeros(m, T), np.zeros(m, T), np.zeros(m, T)
    v[sel], y[sel], tv[sel] = np.asarray(v_C, T)[pc[sel]], np.asarray(y_C, T)[pc[sel]], np.asarray(tol_vC, T)[pc[sel]]
    M, aM, t_M, H, aH, dH = pr["M"], np.abs(pr["M"]), np.asarray(pr["t_M"], T), pr["H"], np.abs(pr["H"]), pr["dH"]
    Mv, My = M @ v, M @ y
    t_Mv = EPS * (3 + C0) * (aM @ np.abs(v)) + t_M @ np.abs(v) + aM @ tv
    t_My = EPS * (3 + C0) * (aM @ np.abs(y)) + t_M @ np.abs(y)
    aMv, aMy, grad, ag, tg = np.abs(Mv), np.abs(My), pr["grad"], np.abs(pr["grad"]), np.asarray(pr["t_grad"], T)

    def quad(a, b, aa, ab, ta, tb):
        return a @ (H @ b), ta @ (aH @ ab) + aa @ (aH @ tb) + aa @ (dH @ ab), aa @ (aH @ ab), m * m

    def dot(a, aa, ta):
        return a @ grad, ta @ ag + aa @ tg, aa @ ag, m
    return dict(jgSq=quad(Mv, Mv, aMv, aMv, t_Mv, t_Mv), jySq=quad(My, My, aMy, aMy, t_My, t_My), jvDotJy=quad(Mv, My, aMv, aMy, t_Mv, t_My),
                jvDotR=dot(Mv, aMv, t_Mv), jyDotR=dot(My, aMy, t_My)), (Mv, My)
