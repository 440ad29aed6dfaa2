"""References for the marginal covariances (svin_ba_get_covariance; svin_amd/csrc/cov.hip), Sigma = (J^T J)^-1.

  mp_inverse       mpmath, 50 digits: the reference everything else is held against.
  refined_inverse  numpy float64 inverse of the matrix scaled to a unit diagonal, then two Newton-Schulz steps X <- X + X (I - M X)
                   in np.longdouble.  NO symmetrisation: a matrix that is symmetric only to 3.5e-16 has an exact inverse that is not
                   symmetric either, and forcing symmetry spoils 8e-12 to 8e-9.
  block_replay     the block formulas the device uses, in float64 numpy: S = A - W V^-1 W^T, Sigma_cc = S^-1,
                   Sigma_lc = -Y_l Sigma_cc, Sigma_ll' = delta_ll' V_l^-1 + Y_l Sigma_cc Y_l'^T, Y_l = V_l^-1 W_l^T.
  mp_block_reference  the same formulas with V_l^-1, the Schur complement and S^-1 in mpmath: the reference where the dense
                   matrix is too large for mp_inverse inside a test (n > ~100).
  err              e(X) = max_ij |X_ij - ref_ij| / sqrt(ref_ii ref_jj): the standard deviations span 1e-8 .. 1e-1.
  dense_normal_matrix  J^T J of a product window from entry points that do not involve the covariance code: eval_reprojection
                   (robust), eval_factors and the prior (M^T H M, prior_reference.moved), in long double.
  bar              8 x max(e(np.linalg.inv), e(block_replay)), both float64 on the same matrix against the same reference.

Nothing here imports the product; dense_normal_matrix is handed an estimator object."""
import numpy as np

LD = np.longdouble
BAR_FACTOR = 8.0   # two honest float64 methods differ by up to 5 x from one another; the device adds its own summation order


def mp_inverse(A, dps=50):
    """inverse of A (float64 or long double) in mpmath at `dps` digits, returned as long double"""
    import mpmath as mp
    A = np.asarray(A, LD)
    n = A.shape[0]
    hi = A.astype(np.float64)
    lo = (A - hi.astype(LD)).astype(np.float64)
    with mp.workdps(dps):
        M = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                M[i, j] = mp.mpf(float(hi[i, j])) + mp.mpf(float(lo[i, j]))
        X = mp.inverse(M)
        out = np.zeros((n, n), LD)
        for i in range(n):
            for j in range(n):
                h = float(X[i, j])
                out[i, j] = LD(h) + LD(float(X[i, j] - mp.mpf(h)))
    return out


def refined_inverse(A, steps=2):
    """float64 inverse of the unit-diagonal scaling of A, refined by Newton-Schulz steps in long double; no symmetrisation"""
    A = np.asarray(A, np.float64)
    s = 1.0 / np.sqrt(np.diag(A))
    M = (A * s[:, None] * s[None, :])
    X = np.linalg.inv(M).astype(LD)
    sl = s.astype(LD)
    Ml, I = A.astype(LD) * sl[:, None] * sl[None, :], np.eye(len(A), dtype=LD)   # (the scaled matrix without float64's rounding of it)
    for _ in range(steps):
        X = X + X @ (I - Ml @ X)
    return X * sl[:, None] * sl[None, :]


def block_replay(N, d):
    """the block formulas on N = [[A, W], [W^T, V]] (A: d x d, V block diagonal in 3 x 3), float64 numpy throughout"""
    N = np.asarray(N, np.float64)
    n = N.shape[0]
    L = (n - d) // 3
    assert d + 3 * L == n
    A, W = N[:d, :d], N[:d, d:]
    Vinv, Y = np.zeros((L, 3, 3)), np.zeros((L, 3, d))
    S = A.copy()
    for l in range(L):
        Vinv[l] = np.linalg.inv(N[d + 3 * l:d + 3 * l + 3, d + 3 * l:d + 3 * l + 3])
        Wl = W[:, 3 * l:3 * l + 3]
        Y[l] = Vinv[l] @ Wl.T
        S = S - Wl @ Y[l]
    return _from_blocks(np.linalg.inv(S), Vinv, Y)


def _from_blocks(Scc, Vinv, Y):
    """Sigma from Sigma_cc, V_l^-1 and Y_l, in their dtype"""
    L, d = len(Y), Scc.shape[0]
    n = d + 3 * L
    out = np.zeros((n, n), Scc.dtype)
    out[:d, :d] = Scc
    Yf = np.asarray(Y).reshape(3 * L, d)
    YS = Yf @ Scc
    out[d:, :d] = -YS
    out[:d, d:] = -YS.T
    out[d:, d:] = YS @ Yf.T
    for l in range(L):
        a = slice(d + 3 * l, d + 3 * l + 3)
        out[a, a] += Vinv[l]
    return out


def mp_block_reference(N, d, dps=50):
    """the block formulas with everything that is inverted -- V_l, S -- and the Schur complement itself in mpmath at `dps` digits;
    the final products Y_l Sigma_cc Y_m^T in long double from those.  For n beyond what mp_inverse finishes in seconds."""
    import mpmath as mp
    N = np.asarray(N, LD)
    n = N.shape[0]
    L = (n - d) // 3
    assert d + 3 * L == n

    def to_mp(B):
        M = mp.matrix(B.shape[0], B.shape[1])
        hi = B.astype(np.float64)
        lo = (B - hi.astype(LD)).astype(np.float64)
        for i in range(B.shape[0]):
            for j in range(B.shape[1]):
                M[i, j] = mp.mpf(float(hi[i, j])) + mp.mpf(float(lo[i, j]))
        return M

    def to_ld(M):
        out = np.zeros((M.rows, M.cols), LD)
        for i in range(M.rows):
            for j in range(M.cols):
                h = float(M[i, j])
                out[i, j] = LD(h) + LD(float(M[i, j] - mp.mpf(h)))
        return out
    with mp.workdps(dps):
        S = to_mp(N[:d, :d])
        Vinv, Y = np.zeros((L, 3, 3), LD), np.zeros((L, 3, d), LD)
        for l in range(L):
            a = slice(d + 3 * l, d + 3 * l + 3)
            Vi = mp.inverse(to_mp(N[a, a]))
            Wl = to_mp(N[:d, a])
            Yl = Vi * Wl.T
            S = S - Wl * Yl
            Vinv[l], Y[l] = to_ld(Vi), to_ld(Yl)
        Scc = to_ld(mp.inverse(S)) if d > 0 else np.zeros((0, 0), LD)
    return _from_blocks(Scc, Vinv, Y)


def ld_block_reference(N, d):
    """the block formulas in long double throughout, for windows too large for mpmath inside a test: V_l^-1 by cofactors, the Schur
    complement, S^-1 by a float64 inverse of the unit-diagonal scaling and three Newton-Schulz steps.  Long double's rounding
    (1.1e-19) times the conditions met (S scaled: <= 1e9, V_l: <= 1e6) leaves 1e-10, two orders below the float64 yardsticks."""
    N = np.asarray(N, LD)
    n = N.shape[0]
    L = (n - d) // 3
    assert d + 3 * L == n
    S = N[:d, :d].copy()
    Vinv, Y = np.zeros((L, 3, 3), LD), np.zeros((L, 3, d), LD)
    for l in range(L):
        a = slice(d + 3 * l, d + 3 * l + 3)
        q = N[a, a]
        cof = np.array([[q[1, 1] * q[2, 2] - q[1, 2] * q[2, 1], q[0, 2] * q[2, 1] - q[0, 1] * q[2, 2], q[0, 1] * q[1, 2] - q[0, 2] * q[1, 1]],
                        [q[1, 2] * q[2, 0] - q[1, 0] * q[2, 2], q[0, 0] * q[2, 2] - q[0, 2] * q[2, 0], q[0, 2] * q[1, 0] - q[0, 0] * q[1, 2]],
                        [q[1, 0] * q[2, 1] - q[1, 1] * q[2, 0], q[0, 1] * q[2, 0] - q[0, 0] * q[2, 1], q[0, 0] * q[1, 1] - q[0, 1] * q[1, 0]]], LD)
        Vinv[l] = cof / (q[0, 0] * cof[0, 0] + q[0, 1] * cof[1, 0] + q[0, 2] * cof[2, 0])
        Y[l] = Vinv[l] @ N[:d, a].T
        S = S - N[:d, a] @ Y[l]
    s = 1 / np.sqrt(np.diag(S))
    M = S * s[:, None] * s[None, :]
    X = np.linalg.inv(M.astype(np.float64)).astype(LD)
    I = np.eye(d, dtype=LD)
    for _ in range(3):
        X = X + X @ (I - M @ X)
    return _from_blocks(X * s[:, None] * s[None, :], Vinv, Y)


def err(X, ref):
    """e(X) = max_ij |X_ij - ref_ij| / sqrt(ref_ii ref_jj), the scale from the reference's full diagonal"""
    ref = np.asarray(ref, LD)
    sd = np.sqrt(np.diag(ref))
    return float(np.max(np.abs(np.asarray(X, LD) - ref) / np.outer(sd, sd)))


def err_block(X, ref, rows, cols, sd):
    """the same for one block, sd = sqrt(diag) of the whole reference"""
    return float(np.max(np.abs(np.asarray(X, LD) - np.asarray(ref, LD)[np.ix_(rows, cols)]) / np.outer(sd[rows], sd[cols])))


def bar(N, d, ref):
    """(bar, e(np.linalg.inv), e(block_replay)) for the normal matrix N with d camera-side unknowns against `ref`"""
    N64 = np.asarray(N, np.float64)
    e_inv = err(np.linalg.inv(N64), ref)
    e_blk = err(block_replay(N64, d), ref)
    return BAR_FACTOR * max(e_inv, e_blk), e_inv, e_blk


def dense_normal_matrix(est, prior_moved=None):
    """J^T J (long double) of the window `est` holds, from est.linearize() (the order of the variable camera-side blocks),
    est.eval_reprojection(robust=True), est.eval_factors() and est.marg().  Constant blocks have no columns.  Landmarks follow
    the camera-side blocks in the order of their first observation.  prior_moved(H, b, c0, blocks, columns, dtype) is
    prior_reference.moved (handed in so that this module imports nothing of the test tree's).
    Returns dict(N, d, blocks: [(id, first column, dim)], lm_ids)."""
    lin = est.linearize(0.0)
    d = int(lin["d"])
    col, dim = {}, {}
    for bid, off in zip(lin["block_ids"], lin["block_off"]):
        kind = est.describe_block(int(bid))[1]
        col[int(bid)], dim[int(bid)] = int(off), 9 if kind == 2 else 6
    ev = est.eval_reprojection(robust=True)
    lm_col, lm_ids = {}, []
    for lid in ev["lm_id"]:
        lid = int(lid)
        if lid not in lm_col and not est.is_parameter_block_constant(lid):
            lm_col[lid] = d + 3 * len(lm_ids)
            lm_ids.append(lid)
    n = d + 3 * len(lm_ids)
    rows = []
    for k in range(len(ev["lm_id"])):
        pose, lid, ext = est.parameters_of(int(ev["res_id"][k]))[0][:3]
        R = np.zeros((2, n), LD)
        if int(pose) in col:
            R[:, col[int(pose)]:col[int(pose)] + 6] = ev["Jp"][k]
        if int(ext) in col:
            R[:, col[int(ext)]:col[int(ext)] + 6] = ev["Je"][k]
        if int(lid) in lm_col:
            R[:, lm_col[int(lid)]:lm_col[int(lid)] + 3] = ev["Jl"][k]
        rows.append(R)
    for f in est.eval_factors():
        R = np.zeros((f["m"], n), LD)
        c = 0
        for b in f["blocks"]:
            kind = est.describe_block(int(b))
            md = 9 if (kind is not None and kind[1] == 2) else _map_block_dim(est, b)
            if int(b) in col:
                R[:, col[int(b)]:col[int(b)] + md] = f["J"][:, c:c + md]
            c += md
        assert c == f["J"].shape[1], (f["kind"], c, f["J"].shape)
        rows.append(R)
    J = np.concatenate(rows) if rows else np.zeros((0, n), LD)
    N = J.T @ J
    mg = est.marg()
    if mg is not None:
        blocks, columns = [], -np.ones(mg["n"], np.int64)
        for b in mg["blocks"]:
            x = np.asarray(est.get_parameter_block(b["id"]), np.float64)
            blocks.append(dict(kind={0: "p", 1: "e", 2: "s"}[b["kind"]], ordering=b["ordering"], mdim=b["mdim"], lin=b["lin"], x=x))
            if b["id"] in col and b["mdim"] > 0:
                columns[b["ordering"]:b["ordering"] + b["mdim"]] = np.arange(col[b["id"]], col[b["id"]] + b["mdim"])
        pr = prior_moved(mg["H"], mg["b0"], 0.0, blocks, columns, dtype=LD)
        rows_in = np.nonzero(columns >= 0)[0]
        N[np.ix_(columns[rows_in], columns[rows_in])] += pr["S"][np.ix_(rows_in, rows_in)]
    return dict(N=N, d=d, blocks=[(b, col[b], dim[b]) for b in col], lm_ids=lm_ids, lm_col=lm_col)


def _map_block_dim(est, b):
    """minimal dimension of a block of a Map-built graph (no state describes it): 9 for speed / bias (ambient 9), else 6"""
    return 9 if len(est.get_parameter_block(int(b))) == 9 else 6
