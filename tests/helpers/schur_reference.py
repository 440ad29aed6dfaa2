"""Long-double reference of the landmark elimination (K5) with an a-priori rounding bound for every entry.

The reduced system is a pure function of the per-residual records the kernels consume.  `assemble()` recomputes it from
those records in np.longdouble (64-bit mantissa) and returns, next to S, g and the cost, what is needed to judge a float64
result entry by entry without a tuned tolerance.

Arithmetic (read off svin_amd/csrc/kernels.hip: k_schur pass 1 / pass 2, factorsAccumulate, finalizeRow)

  per landmark l    V = sum Jl^T Jl,  b = sum Jl^T r,   sc_k = 1 / (1 + sqrt(V_kk)),
                    ht_k = clamp(V_kk sc_k^2, 1e-6, 1e32) / sc_k^2,   V_d = V + mu diag(ht),
                    W = sum Jc^T Jl  (Jc: the residual's columns of the variable camera-side blocks)
  camera side       A = sum Jc^T Jc over every record (a factor's loss corrector sqrt(rho') is applied to its r and J by
                    the caller), hC = diag(A), the same sc / clamp rule gives htC,
                    S = A - sum_l W V_d^-1 W^T + mu diag(htC),     g = sum Jc^T r - sum_l W V_d^-1 b.
  Blocks that are not in the block table (constant poses, fixed extrinsics) have no rows and no columns.  The scales are
  recomputed from the current V and hC (linearize() runs with initScale = true).

The bound.  Expanded into elementary products, an entry is a sum of terms
     A part       Jc[k,i] Jc[k,j]                                     one per residual row k that touches i and j
     Schur part   Jc[k,i] Jl[k,a] X[a,b] Jl[k',b] Jc[k',j]            X = V_d^-1; 9 per pair of rows (k, k') of a landmark
(g: r in place of the second Jc).  n is the number of terms, M the sum of their absolute values.  A float64 evaluation of
such a sum in ANY order and with any factoring (W first, G = W L^-T first, K = delta - Jl X Jl^T first), with or without
FMA, errs by at most gamma_(n + c0) M <= (n + c0) eps M (Higham, Accuracy and Stability, 3.1 / 3.3):
     c0 = 8 : at most four multiplications inside a term, the subtraction of the two parts, the product and the
              addition of the damping mu * ht (ht itself: sqrt, 2 products, a division: folded into the damping's own M),
              one to spare.
That treats X as data.  X is computed too: V is a sum of rows_l = 2 * (observations of l) products per entry
(|dV| <= gamma_rows |Jl|^T |Jl|, whose norm is at most 3 |V|), V_d adds two roundings, and its inverse goes through a
3 x 3 Cholesky factor, its inverse by substitution and the product L^-T L^-1: backward error gamma_4 |L| |L^T| <= 12 eps |V_d|
for the factor (Higham 10.4, n + 1 = 4, || |L||L^T| || <= n ||V_d||), 2 x 9 eps for the triangular inverse and the product
(n gamma_n each), together < 32 eps.  A relative perturbation delta of V_d moves V_d^-1 by kappa(V_d) delta |V_d^-1|
to first order, hence
     tol_ij = eps [ (n_ij + c0) M_ij + sum_l (c + 3 rows_l) kappa_l (|W_l| |X_l| |W_l|^T)_ij ],    c0 = 8,  c = 32,
the issue's formula with the sum that forms V_l written out (c alone is the inverse; 3 rows_l is V's own gamma).
The kappa term is the norm-wise statement of that perturbation.  Entry by entry and still to first order it reads
     d(W X W^T) = -(W X) dV (W X)^T + W dX_f W^T,
with |dV| <= (6 + rows_l) eps sqrt(V_d,aa V_d,bb) (the sum that forms V: |Jl|^T |Jl| <= sqrt(V_aa V_bb); the factor's backward
error 4 |L| |L^T| <= 4 sqrt(V_d,aa V_d,bb), both by Cauchy-Schwarz; two roundings for the damping) acting through the TRUE
product W X -- W has almost no component along the badly observed direction in which X is large, which |W| |X| forgets -- and
dX_f the forward error of L^-1 by substitution and of the product L^-T L^-1 (Higham 8.2 / 3.5 with n = 3):
|dX_f| <= eps [3 (D^T |L^-1| + |L^-1|^T D) + 3 |L^-1|^T |L^-1|], D = |L^-1| |L| |L^-1|.  Per landmark tol takes the SMALLER of
the kappa term and this one.
The first term is crude where one landmark has a nearly singular V_d (a single observation: X ~ 1 / (mu ht), its terms are
huge and cancel): n_ij counts the terms of ALL landmarks and multiplies them into that one landmark's M.  Every form computes a
landmark's contribution by itself and then accumulates contributions, so the sharper statement also holds:
     sum_l (n_l + c0) M'_l  +  (pieces_ij + c0) (M^A_ij + sum_l sqrt(t_l,ii t_l,jj)),    t_l = W_l X_l W_l^T,
with n_l and M'_l the terms of landmark l alone, M'_l taken with sqrt(X_aa X_bb) in place of |X_ab| (it bounds |L^-T| |L^-1| of
the Gram form too), three pieces per landmark (the columns of G) plus the terms of A, and sqrt(t_ii t_jj) >= (|G| |G|^T)_ij the
size of a landmark's pieces.  tol takes the SMALLER of the two first terms, so it is never wider than the formula above.
Two deviations from the plain formula, stated so that nobody takes them for more than they are.  (i) The sharper first term and
the entry-wise conditioning term assume STRUCTURE -- a landmark's contribution is formed by itself (through V_d's Cholesky factor)
and contributions are then added -- which holds for the four forms of kernels.hip but is not order-free: a future form that
accumulates differently may leave tol without being wrong, and is then to be judged by the plain formula (both first terms and
the kappa sums are returned: M_S, n_S, K_S).  (ii) The constant in front of kappa is not one small integer: it is 32 for the
inverse plus 3 rows_l for the sum that forms V_l, up to ~800 for a track of 2 P = 128 observations.
eps = 2^-52 (np.finfo(np.float64).eps).  The same bound with the long-double eps holds for this reference itself:
its error is at most (eps_ld / eps) tol = 2^-11 tol, which `assemble` asserts to be below tol / 1000.

Not covered by what is compared through this helper or through step_reference.py (the post-solve pass and the dogleg step, which
build on it): the batched Schur form (k_schur_dense_batch) and the sharded path.  (The marginalisation prior away from its
linearisation point: prior_reference.py, whose result `prior` below takes.)
"""
import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EPS_LD = float(np.finfo(LD).eps)
C0 = 8
C_INV = 32
KIND_LANDMARK = "l"


def have_long_double():
    return EPS_LD < 1e-18


def _metric(h):
    """ht of finalizeRow / k_schur for column norms h (sc recomputed: initScale = true)"""
    h = np.asarray(h, LD)
    sc = LD(1) / (LD(1) + np.sqrt(h))
    return np.minimum(np.maximum(h * sc * sc, LD(1e-6)), LD(1e32)) / (sc * sc)


def _inv3(V):
    """inverse of a symmetric 3 x 3 matrix by cofactors, in the precision of V"""
    a, b, c, d, e, f = V[0, 0], V[0, 1], V[0, 2], V[1, 1], V[1, 2], V[2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * c00 + b * c01 + c * c02
    c11, c12, c22 = a * f - c * c, b * c - a * e, a * d - b * b
    X = np.array([[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]], dtype=V.dtype)
    return X / det


def _chol3(V):
    """lower Cholesky factor of a symmetric positive definite 3 x 3 matrix, in the precision of V"""
    L = np.zeros((3, 3), V.dtype)
    for j in range(3):
        L[j, j] = np.sqrt(V[j, j] - L[j, :j] @ L[j, :j])
        for i in range(j + 1, 3):
            L[i, j] = (V[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def _inv3_lower(L):
    Li = np.zeros((3, 3), L.dtype)
    for j in range(3):
        Li[j, j] = 1 / L[j, j]
        for i in range(j + 1, 3):
            Li[i, j] = -(L[i, j:i] @ Li[j:i, j]) / L[i, i]
    return Li


def _kappa(Vd):
    w = np.linalg.eigvalsh(np.asarray(Vd, np.float64))
    return float("inf") if not w[0] > 0 else float(w[-1] / w[0])


def assemble(records, blocks, mu, dtype=LD, prior=None):
    """records: iterable of (r, [(key, J), ...]) or (r, [(key, J), ...], cost_term); key = (kind, id), kind one of "p" pose,
    "e" extrinsics, "s" speed / bias, "l" landmark (at most one landmark per record); J is len(r) x (6 | 6 | 9 | 3).  A record's
    cost term is 0.5 |r|^2 unless given (a robustified residual's is 0.5 rho).
    blocks: [(key, offset, dim)] of the variable camera-side blocks, in the order and at the offsets of the system to compare with.
    prior: None or (H, b0, c0, columns): the marginalisation prior as the quadratic form the device adds at the prior's linearisation
    point -- H into A (and its diagonal into hC), b0 into the gradient, c0 into the cost; columns[i] = the row of the system that
    row i of the prior belongs to, or -1 (a constant block).  One term per entry, M = |H|, |b0|.  Or the dict of
    prior_reference.moved(): the prior at the blocks' current values, away from its linearisation point (M3 != I, dchi != 0) -- M^T H M
    into A, M^T grad into the gradient, its cost into the cost, each with its number of terms and absolute sum; the first-order effect
    of the float64 dchi and M (P_S, P_g, the cost's own bound) is added to the tolerances as it stands.
    Returns a dict: S, g, cost (dtype), d, per landmark V / b / kappa (dicts by landmark id), M_S / n_S / M_g / n_g, the
    conditioning sums K_S / K_g, tol_S / tol_g / tol_cost (float64 arrays) and ref_ratio (the reference's own error / tol)."""
    T = dtype
    col = {key: (off, dim) for key, off, dim in blocks}
    d = max([off + dim for _, off, dim in blocks], default=0)
    mu = T(mu)
    A, MA = np.zeros((d, d), T), np.zeros((d, d), T)
    nS = np.zeros((d, d), np.int64)
    gA, Mg = np.zeros(d, T), np.zeros(d, T)
    ng = np.zeros(d, np.int64)
    cost, n_cost = T(0), 0
    by_lm = {}
    for rec in records:
        r = np.asarray(rec[0], T).reshape(-1)
        m = len(r)
        term = T(rec[2]) if len(rec) > 2 and rec[2] is not None else T(0.5) * (r @ r)
        cost += term
        n_cost += 1
        idx, Js, lm, Jl = [], [], None, None
        for key, J in rec[1]:
            J = np.asarray(J, T).reshape(m, -1)
            if key[0] == KIND_LANDMARK:
                assert lm is None, "one landmark per record"
                lm, Jl = key[1], J
            elif key in col:
                off, dim = col[key]
                assert J.shape[1] == dim, (key, J.shape, dim)
                idx.append(np.arange(off, off + dim))
                Js.append(J)
        idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
        Jc = np.concatenate(Js, 1) if Js else np.zeros((m, 0), T)
        if len(idx):
            ix = np.ix_(idx, idx)
            A[ix] += Jc.T @ Jc
            MA[ix] += np.abs(Jc).T @ np.abs(Jc)
            nS[ix] += m
            gA[idx] += Jc.T @ r
            Mg[idx] += np.abs(Jc).T @ np.abs(r)
            ng[idx] += m
        if lm is not None:
            by_lm.setdefault(lm, []).append((idx, Jc, Jl, r))
    PS, Pg, tol_prior_cost = np.zeros((d, d), T), np.zeros(d, T), 0.0   # first-order propagation of a moved prior's dchi and M
    if isinstance(prior, dict):
        pc = prior["columns"]
        sel = np.nonzero(pc >= 0)[0]
        ix, ixp = np.ix_(pc[sel], pc[sel]), np.ix_(sel, sel)
        A[ix] += np.asarray(prior["S"], T)[ixp]
        MA[ix] += np.asarray(prior["M_S"], T)[ixp]
        nS[ix] += prior["n_S"][ixp]
        PS[ix] += np.asarray(prior["P_S"], T)[ixp]
        gA[pc[sel]] += np.asarray(prior["g"], T)[sel]
        Mg[pc[sel]] += np.asarray(prior["M_g"], T)[sel]
        ng[pc[sel]] += prior["n_g"][sel]
        Pg[pc[sel]] += np.asarray(prior["P_g"], T)[sel]
        cost += T(prior["cost"])
        n_cost += 1
        tol_prior_cost = prior["tol_cost"]
    elif prior is not None:
        pc = np.asarray(prior[3])
        sel = np.nonzero(pc >= 0)[0]
        ix = np.ix_(pc[sel], pc[sel])
        Hp, bp = np.asarray(prior[0], T)[np.ix_(sel, sel)], np.asarray(prior[1], T)[sel]
        A[ix] += Hp
        MA[ix] += np.abs(Hp)
        nS[ix] += 1
        gA[pc[sel]] += bp
        Mg[pc[sel]] += np.abs(bp)
        ng[pc[sel]] += 1
        cost += T(prior[2])
        n_cost += 1
    S, g = A.copy(), gA.copy()
    MS = MA.copy()
    KS, Kg = np.zeros((d, d), T), np.zeros(d, T)
    RS, Rg = (nS + C0) * MA, (ng + C0) * Mg          # refined bound: the terms inside one piece ...
    accS, accg = MA.copy(), Mg.copy()                # ... and the magnitude of the pieces that are then accumulated
    npS, npg = nS.copy(), ng.copy()
    Vs, bs, kappas = {}, {}, {}
    for lm, rows in by_lm.items():
        Jl = np.concatenate([x[2] for x in rows], 0)
        r = np.concatenate([x[3] for x in rows], 0)
        R = len(r)
        V, b = Jl.T @ Jl, Jl.T @ r
        Vd = V + np.diag(mu * _metric(np.diag(V)))
        Vs[lm], bs[lm] = V, b
        kap = kappas[lm] = _kappa(Vd)
        cols = np.unique(np.concatenate([x[0] for x in rows])) if rows else np.zeros(0, np.int64)
        if not len(cols):
            continue
        assert np.isfinite(kap), "landmark %r: V + mu ht is singular" % (lm,)
        pos = {int(c): k for k, c in enumerate(cols)}
        Jc = np.zeros((R, len(cols)), T)
        present = np.zeros((R, len(cols)), bool)
        o = 0
        for idx, J, _, rr in rows:
            k = [pos[int(c)] for c in idx]
            Jc[o:o + len(rr), k] = J
            present[o:o + len(rr), k] = True
            o += len(rr)
        X = _inv3(Vd)
        aX = np.abs(X)
        W, Wabs = Jc.T @ Jl, np.abs(Jc).T @ np.abs(Jl)
        cnt = present.sum(0).astype(np.int64)
        ix = np.ix_(cols, cols)
        WX = W @ X
        S[ix] -= WX @ W.T
        g[cols] -= WX @ b
        MS[ix] += Wabs @ aX @ Wabs.T
        nS[ix] += 9 * np.outer(cnt, cnt)
        Mg[cols] += Wabs @ aX @ (np.abs(Jl).T @ np.abs(r))
        ng[cols] += 9 * cnt * R
        Xs = np.sqrt(np.outer(np.diag(X), np.diag(X)))        # >= |X| and >= |L^-T| |L^-1| entry by entry (Cauchy-Schwarz)
        t = WX @ W.T
        RS[ix] += (9 * np.outer(cnt, cnt) + C0) * (Wabs @ Xs @ Wabs.T)
        accS[ix] += np.sqrt(np.outer(np.abs(np.diag(t)), np.abs(np.diag(t))))
        npS[ix] += 3
        Rg[cols] += (9 * cnt * R + C0) * (Wabs @ Xs @ (np.abs(Jl).T @ np.abs(r)))
        accg[cols] += np.sqrt(np.abs(np.diag(t)) * np.abs(b @ X @ b))
        npg[cols] += 3
        c_l = T((C_INV + 3 * R) * kap)
        aW = np.abs(W)
        aWX = aW @ aX
        # the same perturbation without kappa (see the docstring): backward error of V_d and its factor through the TRUE W X,
        # forward error of L^-1 and of L^-T L^-1 through |W|
        Vsq = np.sqrt(np.outer(np.diag(Vd), np.diag(Vd)))
        Lc = _chol3(Vd)
        Li = _inv3_lower(Lc)
        aLi = np.abs(Li)
        Dl = aLi @ np.abs(Lc) @ aLi
        Ef = 3 * (Dl.T @ aLi + aLi.T @ Dl) + 3 * (aLi.T @ aLi)
        aWXt = np.abs(WX)
        KS[ix] += np.minimum(c_l * (aWX @ aW.T), (6 + R) * (aWXt @ Vsq @ aWXt.T) + aW @ Ef @ aW.T)
        Kg[cols] += np.minimum(c_l * (aWX @ np.abs(b)), (6 + R) * (aWXt @ Vsq @ np.abs(X @ b)) + aW @ Ef @ np.abs(b))
    damp = mu * _metric(np.diag(A))
    S[np.arange(d), np.arange(d)] += damp
    MS[np.arange(d), np.arange(d)] += np.abs(damp)
    accS[np.arange(d), np.arange(d)] += np.abs(damp)
    PS[np.arange(d), np.arange(d)] *= 1 + float(mu)   # (the damping follows hC: d ht / d h <= 1)
    tol_S = np.asarray(PS, np.float64) + EPS64 * np.minimum(np.asarray((nS + C0) * MS + KS, np.float64), np.asarray(RS + (npS + C0) * accS + KS, np.float64))
    tol_g = np.asarray(Pg, np.float64) + EPS64 * np.minimum(np.asarray((ng + C0) * Mg + Kg, np.float64), np.asarray(Rg + (npg + C0) * accg + Kg, np.float64))
    # every cost term is non-negative: M = cost; four roundings inside a term (two squares, their sum, the half / the logarithm)
    # (a moved prior's term carries its own bound, prior_reference.moved: its products are not all positive)
    tol_cost = EPS64 * (n_cost + 4) * float(cost) + tol_prior_cost
    ref_ratio = np.finfo(T).eps / EPS64
    if T is LD:
        assert ref_ratio < 1e-3, "long double is not wider than double here"
    return dict(S=S, g=g, cost=cost, d=d, V=Vs, b=bs, kappa=kappas, M_S=MS, n_S=nS, M_g=Mg, n_g=ng, K_S=KS, K_g=Kg,
                tol_S=tol_S, tol_g=tol_g, tol_cost=tol_cost, n_cost=n_cost, ref_ratio=float(ref_ratio))


def worst_ratio(S, g, ref):
    """(max |S - S_ref| / tol_S, max |g - g_ref| / tol_g); an entry with tol = 0 must be exact"""
    def ratio(x, x0, tol):
        err = np.abs(np.asarray(x, LD) - x0).astype(np.float64)
        out = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
        return float(out.max()) if out.size else 0.0
    return ratio(S, ref["S"], ref["tol_S"]), ratio(g, ref["g"], ref["tol_g"])
