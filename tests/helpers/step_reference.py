"""Long-double reference of what follows the reduced solve in an accepted trust-region iteration -- the post-solve pass
(k_post_solve: landmark back-substitution, the five J v / J y sums, the scaled-gradient norms) and the dogleg step with its
retraction (doglegCoefficients, k_step_retract / the fused tail of k_post_solve / evalReprojBlock with LmDefer) -- with an
a-priori rounding bound for every quantity, built the way schur_reference builds its own: the arithmetic is read off the kernel,
its terms are counted, and a float64 evaluation of a sum of n terms of absolute sum M in ANY order errs by at most
(n + c0) eps M (Higham 3.1 / 3.3; c0 = schur_reference.C0 = 8 roundings to spare for what is done to the sum afterwards).

The conditioning of the dense solve is judged in tests/test_gpu_reduced_solve.py and kept out of the bounds here: the reference
works in two stages, each taking the device's result of what went before as data.

Stage A (`stage_a`) takes the device's y_C.  Arithmetic (kernels.hip, k_post_solve_body; the solver's finalisation for v_C)
  camera side   g_i = sum Jc^T r over every record (n_i products, absolute sum Mg_i), h_i = sum Jc^2, ht_i = metric(h_i)
                (schur_reference._metric: sqrt, two products, a division, a clamp: 8 roundings), v_i = g_i / ht_i:
                    tol_vC = eps ((n_i + 2) Mg_i + (n_i + 8) |g_i|) / ht_i
  landmark l    (R = 2 * observations rows; observation i has k_i variable camera columns)
                u_i = Jc_i y_C (k_i products), t = sum_i Jl_i^T u_i (2 k_i products per component and observation), q = b - t,
                y_l = X (b - t), X = (V + mu diag(ht_l))^-1, v_l = b / ht_l.  With X as data y_l is a sum of
                n_y = sum_i 2 k_i + R + 3 terms of absolute sum |X| (|Jl|^T |r| + sum_i |Jl_i|^T |Jc_i| |y_C|); X itself is computed
                (schur_reference: |dX| <= (32 + 3 R) kappa_l eps |X| to first order), hence
                    tol_yl = eps [ (n_y + c0) |X| (Mb + T) + (32 + 3 R) kappa_l |X| |q| ],   tol_vl as tol_vC with n = R
  the five sums jgSq = sum |J v|^2, jySq = sum |J y|^2, jvDotJy, jvDotR, jyDotR over every row of every record, J v and J y
                formed per record from the FULL vectors (camera and landmark part; the reference does not use linearity anywhere).
                A row's J v is a sum of k + 3 products: |d(Jv)| <= E_v = eps (k + 4) (|Jc| |v_C| + |Jl| |v_l|) + |Jc| tol_vC + |Jl| tol_vl,
                |d(Jy)| <= E_y = eps (k + 4) (|Jc| |y_C| + |Jl| |y_l|) + |Jl| tol_yl  -- the first-order propagation of the landmark's
                own bound, kappa_l term included, through |J_l| (y_C is data).  A sum over n_rows rows of products of two such:
                    tol = sum_rows (|Jv| E_y + |Jy| E_v) + eps (n_rows + c0) sum_rows |Jv| |Jy|        (and alike for the others)
                The marginalisation prior enters as the quadratic form the device uses (k_post_solve's last block): with p the
                prior's rows in the reduced system, v_p^T H v_p, y_p^T H y_p, v_p^T H y_p, v_p^T b, y_p^T b with H = J^T J, b = J^T e0
                formed from est.marg()'s J and e0 ("what the solver consumes is J^T J, J^T e0 and e0 . e0", svin_ba.h): m more rows
                whose magnitude is |J| |v_p| (the products are summed over the rows first), 2 m products per term.
  norms         gHatSq = sum g^2 / ht, gnHatSq = sum ht y^2, gDotGn = -sum g y over camera rows and landmark coordinates, gradMax =
                max |g|: each term carries the bounds of its factors to first order (dg = eps (n + 1) Mg, d ht / ht = eps (n + 8),
                tol_yl), the accumulation (d + 3 L + c0) eps times the absolute sum.
Stage B (`stage_b`) takes the device's group-B scalars and its y, v as data: the dogleg coefficients, stepNorm, jdSq, jdDotR by
`dogleg_exact` (the expressions of doglegCoefficients at 50 digits, tolerance = condition number x N_OPS x eps exactly as in
tests/test_dogleg_host.py, the branch the one float64 selects); jdSq and jdDotR a second time DIRECTLY as sum |J delta|^2 and
sum (J delta) . r over the records with delta = cg v - cn y -- the check of the kernel's "by linearity"; its bound adds to the
dogleg tolerance the Stage A bounds of the three sums weighted by cg^2, 2 |cg cn|, cn^2 (cg, cn for the two dot products) --;
the candidates: delta_k = cg v_k - cn y_k has the bound |v_k| tol_cg + |y_k| tol_cn + 3 eps (|cg v_k| + |cn y_k|), speed / bias
and the first three landmark coordinates add it (one more rounding), the landmark's fourth coordinate is unchanged bit for bit,
a pose or extrinsics block is x [+] delta by the definition of poseOplus (dmath.hpp) in long double: translation as above; the
quaternion -- normalisation (10 operations), exponential (12, with a sine and a cosine of the device's own, 2 ulp each), product
(7), normalisation (10) on numbers of magnitude at most 1 -- 44 eps plus half the sum of the three rotation deltas' bounds.
stepNormSq and xNormSq (`norms`) are sums of squares in ambient coordinates over the variable blocks and every landmark (the
landmark's fourth coordinate is part of |x|^2) of the DEVICE's candidate: n non-negative terms, (n + 4) eps times the sum.

The prior is either the quadratic form J^T J, J^T e0 of est.marg() at its linearisation point -- straight after the FIRST
marginalisation of a window with nothing optimised in between (tests/test_gpu_lhs.py::test_lhs_with_marginalisation_prior_against_oracle
sets that up) -- or, away from that point (M3 != I, dchi != 0), the dict of prior_reference.moved(), whose docstring derives the
bounds of what it adds here.  NOT covered: the batched Schur form and the sharded path.

The same bounds with the long-double eps hold for this reference itself: its error is at most (eps_ld / eps) tol = 2^-11 tol,
asserted to be below tol / 1000.
"""
import numpy as np

import prior_reference as pref
import schur_reference as sr

LD = sr.LD
EPS = sr.EPS64
C0 = sr.C0
C_INV = sr.C_INV
N_OPS = (34, 31, 73, 72, 36)   # cg, cn, stepNorm, jdSq, jdDotR: counted in tests/test_dogleg_host.py
NEWTON, CAUCHY, INTERP = 0, 1, 2
GROUP_B = ("gHatSq", "jgSq", "gnHatSq", "gDotGn", "jySq", "jvDotJy", "jvDotR", "jyDotR")
Q_OPS = 44


class Problem:
    pass


def prepare(records, blocks, lm_order=None, dtype=LD):
    """records / blocks as schur_reference.assemble takes them; lm_order: landmark ids in the order of the arrays to compare with
    (default: first appearance).  Records with a landmark have two rows and at most twelve variable camera columns."""
    P = Problem()
    T = P.dtype = dtype
    col = {key: (off, dim) for key, off, dim in blocks}
    P.blocks = list(blocks)
    P.d = d = max([off + dim for _, off, dim in blocks], default=0)
    if lm_order is None:
        lm_order = []
        for rec in records:
            for key, _ in rec[1]:
                if key[0] == sr.KIND_LANDMARK and key[1] not in lm_order:
                    lm_order.append(key[1])
    P.lm_ids = [int(i) for i in lm_order]
    index = {i: k for k, i in enumerate(P.lm_ids)}
    P.L = len(P.lm_ids)
    n = sum(1 for rec in records if any(k[0] == sr.KIND_LANDMARK for k, _ in rec[1]))
    P.r, P.Jl, P.Jc = np.zeros((n, 2), T), np.zeros((n, 2, 3), T), np.zeros((n, 2, 12), T)
    P.cols, P.lm = np.full((n, 12), -1, np.int64), np.zeros(n, np.int64)
    P.facs = []
    o = 0
    for rec in records:
        r = np.asarray(rec[0], T).reshape(-1)
        m = len(r)
        lm, k = None, 0
        cc, Js = [], []
        for key, J in rec[1]:
            J = np.asarray(J, T).reshape(m, -1)
            if key[0] == sr.KIND_LANDMARK:
                assert lm is None, "one landmark per record"
                lm, Jlm = key[1], J
            elif key in col:
                off, dim = col[key]
                assert J.shape[1] == dim
                cc.append(np.arange(off, off + dim))
                Js.append(J)
        if lm is None:
            P.facs.append((r, np.concatenate(cc) if cc else np.zeros(0, np.int64), np.concatenate(Js, 1) if Js else np.zeros((m, 0), T)))
            continue
        assert m == 2
        P.r[o], P.Jl[o], P.lm[o] = r, Jlm, index[int(lm)]
        for c, J in zip(cc, Js):
            P.cols[o, k:k + len(c)] = c
            P.Jc[o, :, k:k + len(c)] = J
            k += len(c)
        o += 1
    assert o == n
    P.n_rows = 2 * n + sum(len(f[0]) for f in P.facs)
    return P


def _gather(x, cols):
    """x[cols] with 0 where cols < 0"""
    return np.concatenate([x, np.zeros(1, x.dtype)])[cols]


def prior_columns(prior, blocks):
    """reduced-system column of every row of est.marg()'s prior (-1: the block has no columns, it is constant)"""
    off = {key[1]: o for key, o, _ in blocks}
    pc = np.full(prior["n"], -1, np.int64)
    for b in prior["blocks"]:
        if b["mdim"] > 0 and b["id"] in off:
            pc[b["ordering"]:b["ordering"] + b["mdim"]] = off[b["id"]] + np.arange(b["mdim"])
    return pc


def stage_a(P, mu, y_C, prior=None):
    """prior: None, or (J, e0, columns) of est.marg() with `columns` from prior_columns() -- the prior AT its linearisation point --, or
    the dict of prior_reference.moved(): the prior at the blocks' current values (M^T grad into g, the diagonal of M^T H M into h, the
    five sums through Mv and My; the first-order effect of the float64 dchi and M is carried into every bound).
    Returns {name: value}, {name: tol} and the per-record products the second stage needs."""
    T = P.dtype
    mu = T(mu)
    d, L = P.d, P.L
    y = np.asarray(y_C, T)
    valid = P.cols >= 0
    k_i = valid.sum(1)
    aJc, aJl, ar = np.abs(P.Jc), np.abs(P.Jl), np.abs(P.r)
    g, Mg, h = np.zeros(d, T), np.zeros(d, T), np.zeros(d, T)
    ng = np.zeros(d, np.int64)
    np.add.at(g, P.cols[valid], np.einsum("nrk,nr->nk", P.Jc, P.r)[valid])
    np.add.at(Mg, P.cols[valid], np.einsum("nrk,nr->nk", aJc, ar)[valid])
    np.add.at(h, P.cols[valid], np.einsum("nrk,nrk->nk", P.Jc, P.Jc)[valid])
    np.add.at(ng, P.cols[valid], 2)
    for r, cols, J in P.facs:
        np.add.at(g, cols, J.T @ r)
        np.add.at(Mg, cols, np.abs(J).T @ np.abs(r))
        np.add.at(h, cols, np.einsum("rk,rk->k", J, J))
        np.add.at(ng, cols, len(r))
    Pg, Ph = np.zeros(d, T), np.zeros(d, T)   # a moved prior: what the float64 dchi and M do to g and h, to first order
    moved = prior if isinstance(prior, dict) else None
    if moved is not None:
        pcm = moved["columns"]
        selm = np.nonzero(pcm >= 0)[0]
        np.add.at(g, pcm[selm], np.asarray(moved["g"], T)[selm])
        np.add.at(Mg, pcm[selm], np.asarray(moved["M_g"], T)[selm])
        np.add.at(ng, pcm[selm], moved["n_g"][selm])
        np.add.at(Pg, pcm[selm], np.asarray(moved["P_g"], T)[selm])
        # h: the diagonal of M^T H M, at most nine terms that need not be positive: its own bound, relative to the sum h
        np.add.at(h, pcm[selm], np.diag(np.asarray(moved["S"], T))[selm])
        np.add.at(Ph, pcm[selm], (np.diag(np.asarray(moved["P_S"], T)) + EPS * (9 + C0) * np.diag(np.asarray(moved["M_S"], T)))[selm])
    elif prior is not None:
        Jp, e0, pc = np.asarray(prior[0], T), np.asarray(prior[1], T), np.asarray(prior[2])
        sel = pc >= 0
        Js, pcs = Jp[:, sel], pc[sel]
        m = len(e0)
        np.add.at(g, pcs, Js.T @ e0)
        np.add.at(Mg, pcs, np.abs(Js).T @ np.abs(e0))
        np.add.at(h, pcs, np.einsum("rk,rk->k", Js, Js))
        np.add.at(ng, pcs, m)
    ht = sr._metric(h)
    v = g / ht
    dg = EPS * (ng + 1) * Mg + Pg
    rel_ht = Ph / ht                                  # (d ht / d h <= 1: ht = h between the clamps)
    tol_vC = EPS * ((ng + 2) * Mg + (ng + 8) * np.abs(g)) / ht + Pg / ht + np.abs(g) / ht * rel_ht
    # landmarks
    V, b, Mb = np.zeros((L, 3, 3), T), np.zeros((L, 3), T), np.zeros((L, 3), T)
    R, nt = np.zeros(L, np.int64), np.zeros(L, np.int64)
    np.add.at(V, P.lm, np.einsum("nra,nrb->nab", P.Jl, P.Jl))
    np.add.at(b, P.lm, np.einsum("nra,nr->na", P.Jl, P.r))
    np.add.at(Mb, P.lm, np.einsum("nra,nr->na", aJl, ar))
    np.add.at(R, P.lm, 2)
    np.add.at(nt, P.lm, 2 * k_i)
    htL = sr._metric(np.einsum("laa->la", V))
    Vd = V.copy()
    for a in range(3):
        Vd[:, a, a] += mu * htL[:, a]
    w = np.linalg.eigvalsh(Vd.astype(np.float64)) if L else np.zeros((0, 3))
    assert np.all(w[:, 0] > 0), "a landmark's V + mu ht is singular"
    kappa = (w[:, 2] / w[:, 0]) if L else np.zeros(0)
    X = sr._inv3(Vd.transpose(1, 2, 0)).transpose(2, 0, 1) if L else np.zeros((0, 3, 3), T)
    aX = np.abs(X)
    uy = np.einsum("nrk,nk->nr", P.Jc, _gather(y, P.cols))
    auy = np.einsum("nrk,nk->nr", aJc, _gather(np.abs(y), P.cols))
    t, Tabs = np.zeros((L, 3), T), np.zeros((L, 3), T)
    np.add.at(t, P.lm, np.einsum("nra,nr->na", P.Jl, uy))
    np.add.at(Tabs, P.lm, np.einsum("nra,nr->na", aJl, auy))
    q = b - t
    yl = np.einsum("lab,lb->la", X, q)
    vl = b / htL
    n_y = nt + R + 3
    tol_yl = EPS * ((n_y + C0)[:, None] * np.einsum("lab,lb->la", aX, Mb + Tabs)
                    + ((C_INV + 3 * R) * kappa)[:, None] * np.einsum("lab,lb->la", aX, np.abs(q)))
    dbl = EPS * (R + 1)[:, None] * Mb
    tol_vl = EPS * ((R + 2)[:, None] * Mb + (R + 8)[:, None] * np.abs(b)) / htL
    # J v and J y per record, from the full vectors
    Jv = np.einsum("nrk,nk->nr", P.Jc, _gather(v, P.cols)) + np.einsum("nra,na->nr", P.Jl, vl[P.lm])
    Jy = uy + np.einsum("nra,na->nr", P.Jl, yl[P.lm])
    a_v = np.einsum("nrk,nk->nr", aJc, _gather(np.abs(v), P.cols)) + np.einsum("nra,na->nr", aJl, np.abs(vl)[P.lm])
    a_y = auy + np.einsum("nra,na->nr", aJl, np.abs(yl)[P.lm])
    E_v = EPS * (k_i + 4)[:, None] * a_v + np.einsum("nrk,nk->nr", aJc, _gather(tol_vC, P.cols)) + np.einsum("nra,na->nr", aJl, tol_vl[P.lm])
    E_y = EPS * (k_i + 4)[:, None] * a_y + np.einsum("nra,na->nr", aJl, tol_yl[P.lm])
    rows = [(Jv.reshape(-1), Jy.reshape(-1), P.r.reshape(-1), E_v.reshape(-1), E_y.reshape(-1), np.abs(Jv).reshape(-1), np.abs(Jy).reshape(-1))]
    for r, cols, J in P.facs:
        aJ = np.abs(J)
        jv, jy = J @ v[cols], J @ y[cols]
        rows.append((jv, jy, r, EPS * (len(cols) + 2) * (aJ @ np.abs(v[cols])) + aJ @ tol_vC[cols],
                     EPS * (len(cols) + 2) * (aJ @ np.abs(y[cols])), np.abs(jv), np.abs(jy)))
    if prior is not None and moved is None:
        # the device forms v^T (J^T J) v with J^T J and J^T e0 computed beforehand: the products of a row are summed over the rows
        # first, so a row's magnitude is |J| |v|, not |J v|, and every term passes through 2 m products
        aJ = np.abs(Js)
        mv, my = aJ @ np.abs(v[pcs]), aJ @ np.abs(y[pcs])
        rows.append((Js @ v[pcs], Js @ y[pcs], e0, EPS * (2 * m + 2) * mv + aJ @ tol_vC[pcs], EPS * (2 * m + 2) * my, mv, my))
    Jv_, Jy_, r_, Ev_, Ey_, aJv, aJy = [np.concatenate(x) for x in zip(*rows)]
    n_rows = len(r_)
    assert n_rows == P.n_rows + (len(e0) if prior is not None and moved is None else 0)
    val, tol = {}, {}

    def put(name, value, prop, M, n):
        val[name], tol[name] = value, float(prop + EPS * (n + C0) * M)
    ar_ = np.abs(r_)
    sums = dict(jgSq=(Jv_ @ Jv_, 2 * (aJv @ Ev_), aJv @ aJv), jySq=(Jy_ @ Jy_, 2 * (aJy @ Ey_), aJy @ aJy),
                jvDotJy=(Jv_ @ Jy_, aJv @ Ey_ + aJy @ Ev_, aJv @ aJy), jvDotR=(Jv_ @ r_, Ev_ @ ar_, aJv @ ar_),
                jyDotR=(Jy_ @ r_, Ey_ @ ar_, aJy @ ar_))
    n_sum = n_rows
    prior_aux = None if prior is None else (Js, e0, pcs) if moved is None else moved
    if moved is not None:
        # the prior's part of a sum is formed by itself (n_p terms of absolute sum M_p) and is then one more term of the sum
        extra, _ = pref.post_sums(moved, v, y, tol_vC)
        sums = {name: (value + extra[name][0], prop + extra[name][1] + EPS * (extra[name][3] + C0) * extra[name][2], M + extra[name][2])
                for name, (value, prop, M) in sums.items()}
        n_sum += 1
    for name, (value, prop, M) in sums.items():
        put(name, value, prop, M, n_sum)
    # scaled-gradient norms
    n_acc = d + 3 * L
    ag, ab, ay, ayl = np.abs(g), np.abs(b), np.abs(y), np.abs(yl)
    put("gHatSq", (g * g / ht).sum() + (b * b / htL).sum(),
        (2 * ag * dg / ht + (EPS * (ng + 10) + rel_ht) * g * g / ht).sum() + (2 * ab * dbl / htL + EPS * (R + 10)[:, None] * b * b / htL).sum(),
        (g * g / ht).sum() + (b * b / htL).sum(), n_acc)
    put("gnHatSq", (ht * y * y).sum() + (htL * yl * yl).sum(),
        ((EPS * (ng + 10) + rel_ht) * ht * y * y).sum() + (2 * htL * ayl * tol_yl + EPS * (R + 10)[:, None] * htL * yl * yl).sum(),
        (ht * y * y).sum() + (htL * yl * yl).sum(), n_acc)
    put("gDotGn", -((g * y).sum() + (b * yl).sum()),
        (ay * dg + EPS * ag * ay).sum() + (ayl * dbl + ab * tol_yl + 3 * EPS * ab * ayl).sum(), (ag * ay).sum() + (ab * ayl).sum(), n_acc)
    val["gradMax"] = max(ag.max() if d else T(0), ab.max() if L else T(0))
    tol["gradMax"] = max(float(dg.max()) if d else 0.0, float(dbl.max()) if L else 0.0)
    val.update(v_C=v, y_L=yl, v_L=vl)
    tol.update(v_C=np.asarray(tol_vC, np.float64), y_L=np.asarray(tol_yl, np.float64), v_L=np.asarray(tol_vl, np.float64))
    ref_ratio = float(np.finfo(T).eps / EPS)
    if T is LD:
        assert ref_ratio < 1e-3, "long double is not wider than double here"
    aux = dict(kappa=kappa, ht_C=ht, ht_L=htL, g=g, b=b, X=X, V=V, ref_ratio=ref_ratio, n_rows=n_sum,
               prior=prior_aux)
    return val, tol, aux


# ------------------------------------------------------------------------------------------------ dogleg
def code_branch(x):
    """the branch doglegCoefficients takes on nine doubles: its two comparisons with its own roundings"""
    x = [np.float64(v) for v in x]
    gnorm, gnnorm, alpha = np.sqrt(x[0]), np.sqrt(x[2]), x[0] / x[1]
    if gnnorm <= x[8]:
        return NEWTON
    if gnorm * alpha >= x[8]:
        return CAUCHY
    return INTERP


def dogleg_exact(x, branch):
    """the five outputs (cg, cn, stepNorm, jdSq, jdDotR) of the given branch's expressions in mpmath's working precision;
    x = gHatSq jgSq gnHatSq gDotGn jySq jvDotJy jvDotR jyDotR radius"""
    import mpmath as mp
    gHatSq, jgSq, gnHatSq, gDotGn, jySq, jvDotJy, jvDotR, jyDotR, radius = x
    gnorm, alpha = mp.sqrt(gHatSq), gHatSq / jgSq
    if branch == NEWTON:
        cg, cn, step = mp.mpf(0), mp.mpf(1), mp.sqrt(gnHatSq)
    elif branch == CAUCHY:
        cg, cn, step = -(radius / gnorm), mp.mpf(0), radius
    else:
        b_dot_a = -alpha * gDotGn
        a_sq = (alpha * gnorm) ** 2
        b_minus_a_sq = a_sq - 2 * b_dot_a + gnHatSq
        cc = b_dot_a - a_sq
        dd = mp.sqrt(cc * cc + b_minus_a_sq * (radius * radius - a_sq))
        beta = (dd - cc) / b_minus_a_sq
        cg, cn = -alpha * (1 - beta), beta
        step = mp.sqrt(cg * cg * gHatSq + 2 * cg * cn * gDotGn + cn * cn * gnHatSq)
    return [cg, cn, step, cg * cg * jgSq - 2 * cg * cn * jvDotJy + cn * cn * jySq, cg * jvDotR - cn * jyDotR]


def dogleg_reference(x, branch):
    """(values as mpf, tolerances as floats): tol_k = N_OPS[k] eps sum_i |x_i d f_k / d x_i| of the branch's expressions"""
    import mpmath as mp
    with mp.workdps(50):
        xm = [mp.mpf(float(v)) for v in x]
        val = dogleg_exact(xm, branch)
        tol = []
        for k in range(5):
            cond = mp.mpf(0)
            for i in range(9):
                cond += abs(xm[i] * mp.diff(lambda t, i=i, k=k: dogleg_exact(xm[:i] + [t] + xm[i + 1:], branch)[k], xm[i]))
            tol.append(float(N_OPS[k] * EPS * cond))
        return val, tol


def _to_ld(v):
    import mpmath as mp
    with mp.workdps(50):
        hi = float(v)
        return LD(hi) + LD(float(v - mp.mpf(hi)))


def pose_oplus(x, delta):
    """poseOplus of dmath.hpp (Transformation::oplus) in the precision of x"""
    T = x.dtype.type
    q = x[3:7] / np.sqrt(x[3:7] @ x[3:7])
    half = T(0.5) * np.sqrt(delta[3:6] @ delta[3:6])
    s = (np.sin(half) / half if half > 0 else T(1)) * T(0.5)
    dq = np.array([s * delta[3], s * delta[4], s * delta[5], np.cos(half)], x.dtype)
    a, b = dq, q   # (x, y, z, w)
    qn = np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                   a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                   a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                   a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], x.dtype)
    qn = qn / np.sqrt(qn @ qn)
    return np.concatenate([x[:3] + delta[:3], qn])


def stage_b(P, scal, radius, y_C, v_C, y_L, v_L, x_blocks, lm_x, tol_a, prior=None):
    """scal: the device's group B by field name; y / v: the device's vectors; x_blocks: [(key, values)] of every block of the
    window at the linearisation point (a key that is not in the block table is a constant block); lm_x: L x 4 in P.lm_ids order;
    tol_a: Stage A's tolerances (for the direct J delta sums); prior: what Stage A returned in aux["prior"]."""
    T = P.dtype
    x9 = [float(scal[k]) for k in GROUP_B] + [float(radius)]
    branch = code_branch(x9)
    dv, dt = dogleg_reference(x9, branch)
    names = ("cg", "cn", "stepNorm", "jdSq", "jdDotR")
    val = {n: _to_ld(v) for n, v in zip(names, dv)}
    tol = dict(zip(names, dt))
    val["branch"] = branch
    cg, cn = val["cg"], val["cn"]
    y, v, yl, vl = np.asarray(y_C, T), np.asarray(v_C, T), np.asarray(y_L, T).reshape(-1, 3), np.asarray(v_L, T).reshape(-1, 3)
    dC, dL = cg * v - cn * y, cg * vl - cn * yl
    tdC = np.asarray(np.abs(v) * tol["cg"] + np.abs(y) * tol["cn"] + 3 * EPS * (np.abs(cg * v) + np.abs(cn * y)), np.float64)
    tdL = np.asarray(np.abs(vl) * tol["cg"] + np.abs(yl) * tol["cn"] + 3 * EPS * (np.abs(cg * vl) + np.abs(cn * yl)), np.float64)
    # J delta directly, record by record
    Jd = np.einsum("nrk,nk->nr", P.Jc, _gather(dC, P.cols)) + np.einsum("nra,na->nr", P.Jl, dL[P.lm])
    parts = [(Jd.reshape(-1), P.r.reshape(-1))] + [(J @ dC[cols], r) for r, cols, J in P.facs]
    Jd_, r_ = [np.concatenate(x) for x in zip(*parts)]
    jd_sq, jd_r = Jd_ @ Jd_, Jd_ @ r_
    if isinstance(prior, dict):
        (sq, _, _, _), (dr, _, _, _) = [pref.post_sums(prior, dC, dC, np.zeros(P.d))[0][k] for k in ("jgSq", "jvDotR")]
        jd_sq += sq
        jd_r += dr
    elif prior is not None:
        Js, e0, pcs = prior
        jd_sq += (Js @ dC[pcs]) @ (Js @ dC[pcs])
        jd_r += (Js @ dC[pcs]) @ e0
    acg, acn = abs(float(cg)), abs(float(cn))
    val["jdSq_direct"], val["jdDotR_direct"] = jd_sq, jd_r
    tol["jdSq_direct"] = tol["jdSq"] + acg * acg * tol_a["jgSq"] + 2 * acg * acn * tol_a["jvDotJy"] + acn * acn * tol_a["jySq"]
    tol["jdDotR_direct"] = tol["jdDotR"] + acg * tol_a["jvDotR"] + acn * tol_a["jyDotR"]
    # candidates
    col = {key: (off, dim) for key, off, dim in P.blocks}
    cand, tcand = [], []
    for key, x in x_blocks:
        x = np.asarray(x, T)
        if key not in col:
            cand.append(x.copy())
            tcand.append(np.zeros(len(x)))
            continue
        off, dim = col[key]
        dl, td = dC[off:off + dim], tdC[off:off + dim]
        if dim == 9:
            xo = x + dl
            cand.append(xo)
            tcand.append(td + EPS * np.abs(xo).astype(np.float64))
        else:
            xo = pose_oplus(x, dl)
            cand.append(xo)
            tcand.append(np.concatenate([td[:3] + EPS * np.abs(xo[:3]).astype(np.float64), np.full(4, Q_OPS * EPS + 0.5 * td[3:6].sum())]))
    lm_x = np.asarray(lm_x, T).reshape(-1, 4)
    lm_c = lm_x.copy()
    lm_c[:, :3] += dL
    val.update(block_cand=cand, lm_cand=lm_c)
    tol.update(block_cand=tcand, lm_cand=tdL + EPS * np.abs(lm_c[:, :3]).astype(np.float64))
    return val, tol


def norms(P, x_blocks, cand_blocks, lm_x, lm_cand):
    """stepNormSq and xNormSq of a candidate (the DEVICE's) in ambient coordinates: variable blocks and every landmark"""
    T = P.dtype
    col = {key for key, _, _ in P.blocks}
    a = [np.asarray(x, T) for (key, x) in x_blocks if key in col] + [np.asarray(lm_x, T).reshape(-1)]
    b = [np.asarray(c, T) for (key, _), c in zip(x_blocks, cand_blocks) if key in col]
    step = sum(((x - c) @ (x - c) for x, c in zip(a[:-1], b)), T(0))
    dl = np.asarray(lm_x, T).reshape(-1, 4)[:, :3] - np.asarray(lm_cand, T).reshape(-1, 4)[:, :3]
    step += (dl * dl).sum()
    xsq = sum((x @ x for x in a), T(0))
    n = sum(len(x) for x in a)
    return dict(stepNormSq=step, xNormSq=xsq), dict(stepNormSq=float(EPS * (n + 4) * step), xNormSq=float(EPS * (n + 4) * xsq))


def ratio(x, ref, tol):
    """max |x - ref| / tol; where tol = 0 the two must be equal"""
    err = np.abs(np.asarray(x, LD) - np.asarray(ref, LD)).astype(np.float64)
    tol = np.broadcast_to(np.asarray(tol, np.float64), err.shape)
    out = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(out.max()) if out.size else 0.0


SCALARS_A = GROUP_B + ("gradMax",)
DEFERRED = 3


def judge(P, mu, res, x_blocks, lm_x, prior=None, cache=None):
    """error / tol of every Stage A and Stage B quantity of one result in the layout of Estimator.debug_trust_region_step
    (scalars by field name, y_C, v_C, y_L, v_L, block_cand, lm_cand, form, plus the radius): ({name: ratio}, dogleg branch, aux).
    inf where something that must be bit-identical is not.  cache: Stage A by the bits of y_C."""
    sc = res["scalars"]
    key = np.asarray(res["y_C"], np.float64).tobytes()
    cache = {} if cache is None else cache
    if key not in cache:
        cache[key] = stage_a(P, mu, res["y_C"], prior)
    va, ta, aux = cache[key]
    worst = {}
    for n in ("v_C", "y_L", "v_L"):
        worst[n] = ratio(res[n], va[n], ta[n])
    for n in SCALARS_A:
        worst[n] = ratio(sc[n], va[n], ta[n])
    vb, tb = stage_b(P, sc, res["radius"], res["y_C"], res["v_C"], res["y_L"], res["v_L"], x_blocks, lm_x, ta, aux["prior"])
    worst["stepNorm"] = ratio(sc["doglegStepNorm"], vb["stepNorm"], tb["stepNorm"])
    for n in ("jdSq", "jdDotR"):
        worst[n] = ratio(sc[n], vb[n], tb[n])
        worst[n + "_direct"] = ratio(sc[n], vb[n + "_direct"], tb[n + "_direct"])
    if res["form"] == DEFERRED:   # the coefficients travel to the candidate evaluation in the record
        worst["cg"], worst["cn"] = ratio(sc["spareA0"], vb["cg"], tb["cg"]), ratio(sc["spareA1"], vb["cn"], tb["cn"])
    worst["blocks"] = max(ratio(c, r, t) for c, r, t in zip(res["block_cand"], vb["block_cand"], tb["block_cand"]))
    worst["landmarks"] = ratio(res["lm_cand"][:, :3], vb["lm_cand"][:, :3], tb["lm_cand"])
    same = np.array_equal(np.asarray(res["lm_cand"], np.float64)[:, 3].view(np.uint64), np.asarray(lm_x, np.float64)[:, 3].view(np.uint64))
    worst["landmark_w"] = 0.0 if same else float("inf")
    vn, tn = norms(P, x_blocks, res["block_cand"], lm_x, res["lm_cand"])
    for n in ("stepNormSq", "xNormSq"):
        worst[n] = ratio(sc[n], vn[n], tn[n])
    return worst, vb["branch"], aux
