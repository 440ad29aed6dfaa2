"""Long-double reference of the pose graph's marginal covariances (svin_pg_get_covariance_blocks) and a float64 restatement of
the device's recursion, on the records and case graphs of pg_reference.py / pg_cases.py.

Reference.  pr.edges at the given states (robustified Jacobians: square-root information and the Huber corrector applied),
pr.normal_matrix in long double, Jacobi-scaled with s = 1 / (1 + sqrt(diag J^T J)), pr.cholesky_ld, the requested columns by
two substitutions, unscaled: Sigma = S (S J^T J S)^-1 S.  Constant keyframes give zero blocks.  A pivot that is not positive
or below 1e-12 of its diagonal entry of the scaled matrix raises Singular (the rule of include/svin_pg.h).

Restatement (`device_blocks`).  What posegraph.hip does, in float64 on the CPU: the scaled normal equations assembled from a
float64 evaluation, factorised in the device's elimination order (level-1 pieces, level-2 pieces, root; pr.partition), the
block of a pair read off the column of the LATER keyframe, transposed when that is index_a, a diagonal block mirrored from
its lower triangle, unscaled by s on both sides.  `defect` plants one of the mistakes the host test must reject.

The bars (`check_columns`) are pg_reference.py's stage-3 rule unchanged: for column j of the result, y = Sigma[:, j] / (s s_j)
has to solve A y = e_j with eta <= eta_ceiling(n, R), eta <= 8 max(eta(LAPACK), eps), and a normalised forward error below
kappa_2(A) times that bar.
"""
import numpy as np
import scipy.linalg as sla

import pg_cases as pc
import pg_reference as pr

LD = pr.LD
PIVOT_TOL = 1e-12
DEFECTS = ("damping", "one_sided_scale", "transposed", "no_huber", "column_off", "constant_nonzero")


class Singular(Exception):
    """J^T J is not positive definite to working precision; .node is the local keyframe whose block met the pivot"""
    def __init__(self, node, msg):
        super().__init__(msg)
        self.node = node


def tangent(six):
    return 6 if six else 4


def node_of_unknown(problem, six):
    """tangent index -> local keyframe"""
    D = tangent(six)
    off = np.asarray(problem["off"], int)
    out = np.zeros(int(np.sum(off >= 0)) * D, int)
    for k, o in enumerate(off):
        if o >= 0:
            out[o:o + D] = k
    return out


def scaled_system(problem, states, six, dtype=LD, huber=True):
    """A = S J^T J S and s, J at `states` (robustified unless huber=False).  dtype float64: the Jacobians and the scales are float64
    data (a float64 evaluation, as the device's), their products still accumulated in long double -- what pr.system builds from
    a capture"""
    D = tangent(six)
    if dtype is LD:
        E = pr.edges(problem, states, six)
    else:
        with pr.evaluate_in(dtype):
            E = pr.edges(problem, states, six)
    Ja, Jb, res = (E["Ja"], E["Jb"], E["res"]) if huber else (E["Ja0"], E["Jb0"], E["r0"])
    Ja, Jb, res = np.asarray(Ja.v, dtype), np.asarray(Jb.v, dtype), np.asarray(res.v, dtype)
    H, _ = pr.normal_matrix(problem, Ja, Jb, res, D)      # long-double accumulation of `dtype` data: the matrix a result is judged on
    d = np.diag(H)
    s = LD(1) / (LD(1) + np.sqrt(d))
    if dtype is not LD:
        s = np.asarray(np.asarray(s, dtype), LD)
    return H * s[:, None] * s[None, :], s


def factor(A, problem, six):
    """pr.cholesky_ld with the pivot rule; raises Singular naming the keyframe"""
    nodes = node_of_unknown(problem, six)
    d = np.diag(A)
    for j in np.where(~(d > 0))[0]:
        raise Singular(int(nodes[j]), "zero diagonal at unknown %d (keyframe %d)" % (j, nodes[j]))
    try:
        L = pr.cholesky_ld(A)
    except np.linalg.LinAlgError as e:
        j = int(str(e).rsplit(" ", 1)[1])
        raise Singular(int(nodes[j]), str(e))
    piv = np.diag(L) ** 2
    bad = np.where(piv < LD(PIVOT_TOL) * d)[0]
    if len(bad):
        raise Singular(int(nodes[bad[0]]), "pivot %d is %.3e of its diagonal (keyframe %d)" % (bad[0], float(piv[bad[0]] / d[bad[0]]), nodes[bad[0]]))
    return L


def smallest_pivot_ratio(A):
    """min over the unknowns of pivot / diagonal of a long-double Cholesky that goes on past small pivots (0 when one is not positive)"""
    A = np.asarray(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    worst = np.inf
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not c[0] > 0:
            return 0.0
        worst = min(worst, float(c[0] / A[j, j]))
        L[j:, j] = c / np.sqrt(c[0])
    return worst


def _solve_columns(L, cols):
    """columns `cols` of (L L^T)^-1, long double"""
    n = L.shape[0]
    X = np.zeros((n, len(cols)), LD)
    for q, j in enumerate(cols):
        z = np.zeros(n, LD)
        z[j] = LD(1) / L[j, j]
        for i in range(j + 1, n):
            z[i] = -(L[i, j:i] @ z[j:i]) / L[i, i]
        x = np.zeros(n, LD)
        for i in range(n - 1, -1, -1):
            x[i] = (z[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
        X[:, q] = x
    return X


class Reference:
    """Sigma of one problem at one set of states: columns on demand, long double"""
    def __init__(self, problem, states, six):
        self.problem, self.six, self.D = problem, six, tangent(six)
        self.off = np.asarray(problem["off"], int)
        self.A, self.s = scaled_system(problem, states, six)
        self.L = factor(self.A, problem, six)
        self._cols = {}

    def column_block(self, node):
        """n x D: the columns of Sigma that belong to a free keyframe"""
        if node not in self._cols:
            o, D = self.off[node], self.D
            X = _solve_columns(self.L, list(range(o, o + D)))
            self._cols[node] = X * self.s[:, None] * self.s[None, o:o + D]
        return self._cols[node]

    def block(self, a, b):
        D = self.D
        if self.off[a] < 0 or self.off[b] < 0:
            return np.zeros((D, D), LD)
        return self.column_block(b)[self.off[a]:self.off[a] + D]

    def blocks(self, pairs):
        return np.stack([self.block(a, b) for a, b in pairs]) if len(pairs) else np.zeros((0, self.D, self.D), LD)

    def sigma_diag(self, node):
        o = self.off[node]
        return np.diag(self.column_block(node)[o:o + self.D])


def elimination_order(part, problem, six):
    """the unknowns in the order the device eliminates them: level-1 pieces (piece, row), then the separators in separator order
    (level-2 interiors first, the root last)"""
    D = tangent(six)
    off = np.asarray(problem["off"], int)
    free = [k for k in range(len(off)) if off[k] >= 0]
    inner = sorted((k for k in free if part["nodePiece"][k] >= 0), key=lambda k: (part["nodePiece"][k], part["nodeRow"][k]))
    seps = sorted((k for k in free if part["sepOff"][k] >= 0), key=lambda k: part["sepOff"][k])
    assert len(inner) + len(seps) == len(free)
    return np.concatenate([np.arange(off[k], off[k] + D) for k in inner + seps]).astype(int)


def device_blocks(problem, states, six, part, pairs, defect=None):
    """float64 restatement of the device's pass (module docstring); pairs in local keyframes"""
    assert defect is None or defect in DEFECTS
    D = tangent(six)
    off = np.asarray(problem["off"], int)
    A, s = scaled_system(problem, states, six, dtype=np.float64, huber=defect != "no_huber")
    A, s = np.asarray(A, np.float64), np.asarray(s, np.float64)
    if defect == "damping":
        A = A + np.diag(np.clip(np.diag(A), 1e-6, 1e32) / 1e4)
    perm = elimination_order(part, problem, six)
    inv = np.argsort(perm)
    if not np.all(np.diag(A) > 0):
        raise Singular(-1, "zero diagonal")
    c = sla.cho_factor(A[np.ix_(perm, perm)], lower=True)
    piv = np.diag(c[0]) ** 2
    if np.any(piv < PIVOT_TOL * np.diag(A)[perm]):
        raise Singular(-1, "small pivot")
    cache = {}

    def column(node):
        if node not in cache:
            E = np.zeros((len(s), D))
            E[inv[off[node]:off[node] + D], np.arange(D)] = 1.0
            cache[node] = sla.cho_solve(c, E)[inv]
        return cache[node]

    out = np.zeros((len(pairs), D, D))
    for i, (a, b) in enumerate(pairs):
        if off[a] < 0 or off[b] < 0:
            if defect == "constant_nonzero":
                out[i] = 1e-9 * np.eye(D)
            continue
        row, col = (a, b) if a <= b else (b, a)
        src = col - 1 if (defect == "column_off" and off[col - 1] >= 0) else col
        X = column(src)[off[row]:off[row] + D]
        if row == col:
            X = np.tril(X) + np.tril(X, -1).T
        sr, sc = s[off[row]:off[row] + D], s[off[col]:off[col] + D]
        B = X * ((np.ones(D)[:, None] if defect == "one_sided_scale" else sr[:, None]) * sc[None, :])   # x (s_i s_j): symmetric bit for bit
        if (a > b) != (defect == "transposed" and a != b):
            B = B.T
        out[i] = B
    return out


def column_pairs(nn, cols):
    """whole columns: every keyframe of the range as a row"""
    return [(a, b) for b in cols for a in range(nn)]


def check_columns(A, s, problem, six, cols, sigma_cols, ref_cols=None, forward_only=False, verbose=None):
    """pg_reference's stage-3 rule on every column of the given column keyframes.
    A, s: the scaled matrix the result is judged on and its scales; sigma_cols[node]: n x D float64 (free rows in tangent order);
    ref_cols[node]: the same from the long-double inverse of A (computed here when None).  Returns the worst ratios."""
    D = tangent(six)
    off = np.asarray(problem["off"], int)
    n = len(s)
    A = np.asarray(A, LD)
    s = np.asarray(s, LD)
    nA, kap = pr.norm2(A), pr.kappa2(A)
    L = None
    worst = dict(eta=0.0, ratio=0.0, fwd=0.0)
    units = [off[node] + j for node in cols for j in range(D)]
    E = np.zeros((n, len(units)))
    E[units, np.arange(len(units))] = 1.0
    Y_lap = pr.lapack_solve(A, E)          # LAPACK on the same A and e_j, every column in one call
    for qn, node in enumerate(cols):
        for j in range(D):
            u = off[node] + j
            e = np.zeros(n, LD)
            e[u] = 1
            y = np.asarray(sigma_cols[node][:, j], LD) / (s * s[u])
            assert np.all(np.isfinite(np.asarray(y, np.float64))), "column %d of keyframe %d is not finite" % (j, node)
            eta_lap = pr.eta(A, e, Y_lap[:, qn * D + j], nA)
            bar = pr.ETA_MARGIN * max(eta_lap, pr.EPS64)
            if ref_cols is not None:
                y_ld = np.asarray(ref_cols[node][:, j], LD) / (s * s[u])
            else:
                if L is None:
                    L = pr.cholesky_ld(A)
                y_ld = _solve_columns(L, [u])[:, 0]
            ny = float(np.sqrt(y_ld @ y_ld))
            fwd = float(np.sqrt(np.sum((y - y_ld) ** 2))) / ny
            eta_dev = pr.eta(A, e, y, nA)
            if verbose is not None:
                print("%s keyframe %d column %d: eta %.3e eta(LAPACK) %.3e ratio %.2f ceiling %.3e kappa %.3e forward %.3e" %
                      (verbose, node, j, eta_dev, eta_lap, eta_dev / max(eta_lap, pr.EPS64), pr.eta_ceiling(n, D), kap, fwd))
            if not forward_only:
                assert eta_dev <= bar, "keyframe %d column %d: backward error %.3e above %d x max(eta(LAPACK) = %.3e, eps)" % (
                    node, j, eta_dev, pr.ETA_MARGIN, eta_lap)
                assert eta_dev <= pr.eta_ceiling(n, D), "keyframe %d column %d: backward error %.3e above the ceiling" % (node, j, eta_dev)
            assert fwd <= kap * bar, "keyframe %d column %d: forward error %.3e above kappa (%.3e) x bar (%.3e)" % (node, j, fwd, kap, bar)
            worst["eta"] = max(worst["eta"], eta_dev)
            worst["ratio"] = max(worst["ratio"], eta_dev / max(eta_lap, pr.EPS64))
            worst["fwd"] = max(worst["fwd"], fwd / (kap * bar))
    return worst


def columns_from_blocks(problem, six, cols, blocks):
    """blocks of column_pairs(nn, cols) (n_pairs x D x D) -> {node: n x D over the free rows in tangent order}; also checks
    that the rows of constant keyframes are exactly zero"""
    D = tangent(six)
    off = np.asarray(problem["off"], int)
    nn = len(off)
    n = int(np.sum(off >= 0)) * D
    out = {}
    for q, node in enumerate(cols):
        X = np.zeros((n, D))
        for a in range(nn):
            blk = np.asarray(blocks[q * nn + a])
            if off[a] < 0 or off[node] < 0:
                assert np.all(blk == 0.0), "a constant keyframe has a non-zero covariance block"
            if off[a] >= 0:
                X[off[a]:off[a] + D] = blk
        out[node] = X
    return out


def role_columns(part, problem):
    """column keyframes by role in a (captured or restated) partition: an interior keyframe of the first and of the last piece, a
    level-1 cut keyframe (a level-2 interior where level 2 is active), a cover / root keyframe, the first free keyframe, the last
    keyframe"""
    off = np.asarray(problem["off"], int)
    free = [k for k in range(len(off)) if off[k] >= 0]
    picks = []
    if part["nPieces"] > 0:
        first = [k for k in free if part["nodePiece"][k] == 0]
        last = [k for k in free if part["nodePiece"][k] == part["nPieces"] - 1]
        picks += [first[len(first) // 2], last[len(last) // 2]]
        cuts = [k for k in free if part["sepOff"][k] >= 0 and not part["isCover"][k]]
        l2 = [k for k in cuts if part["l2PieceOf"][k] >= 0]
        if l2:
            picks.append(l2[len(l2) // 2])
        elif cuts:
            picks.append(cuts[len(cuts) // 2])
        roots = [k for k in free if part["sepOff"][k] >= 0 and part["isRoot"][k] and (part["isCover"][k] or part["nPieces2"] > 0)]
        if roots:
            picks.append(roots[len(roots) // 2])
    picks += [free[0], len(off) - 1]
    out = []
    for k in picks:
        if k not in out and off[k] >= 0:
            out.append(k)
    return out


def states_from_poses(problem, T, Q, six, r2ypr):
    """the states the device takes after an optimisation: positions and quaternions as svin_pg_get_poses returns them for the
    keyframes of the range (rows of T, Q), the yaw from the returned quaternion (r2ypr: pg_cases._r2ypr)"""
    T, Q = np.asarray(T, np.float64), np.asarray(Q, np.float64)
    return dict(yaw=np.array([r2ypr(q)[0] for q in Q]), t=T.reshape(-1), q=Q.reshape(-1))


def check_blocks(ref, pairs, blocks):
    """every requested block against the long-double reference, entry by entry.  The column rule bounds a column's error in the
    2-norm by kappa_2(A) bar |y_ld|_2 (y = Sigma[:, j] / (s s_j)), and no entry errs by more than its column does:
        |dSigma[a_i, b_j]| <= s_(a_i) s_(b_j) kappa_2(A) bar |y_ld(b_j)|_2,   bar = ETA_MARGIN eps (the bar's floor).
    This is the check that sees a block in the wrong orientation, from the wrong column or with the wrong scale."""
    D, off = ref.D, ref.off
    kap = pr.kappa2(ref.A)
    bar = pr.ETA_MARGIN * pr.EPS64
    worst = 0.0
    for (a, b), blk in zip(pairs, blocks):
        want = ref.block(a, b)
        if off[a] < 0 or off[b] < 0:
            assert np.all(np.asarray(blk) == 0.0), "block (%d, %d): a constant keyframe has a non-zero covariance block" % (a, b)
            continue
        sa, sb = ref.s[off[a]:off[a] + D], ref.s[off[b]:off[b] + D]
        Y = ref.column_block(b) / (ref.s[:, None] * sb[None, :])
        ny = np.sqrt(np.sum(Y * Y, axis=0))
        tol = np.asarray(sa[:, None] * sb[None, :] * ny[None, :] * LD(kap * bar), np.float64)
        err = np.abs(np.asarray(blk, LD) - want)
        worst = max(worst, float(np.max(err / tol)))
        assert np.all(err <= tol), "block (%d, %d): off by %.3e of its bound" % (a, b, float(np.max(err / tol)))
    return worst


def check_transposes(blocks_ab, blocks_ba):
    """Sigma[b, a] == Sigma[a, b]^T bit for bit"""
    for x, y in zip(blocks_ab, blocks_ba):
        assert np.array_equal(np.asarray(x), np.asarray(y).T), "Sigma[b, a] is not Sigma[a, b]^T bit for bit"


def second_sequence_case(**kw):
    """a singular input without a zero block: twenty keyframes, the last ten a sequence of their own with no loop to the first, so
    that they float as a whole (the exact pivot of their last keyframe is zero; rounding leaves about n eps of the diagonal)"""
    seq = np.ones(20, int)
    seq[10:] = 2
    return pc.Case(name="floating", spec=pc._graph(20, [(8, 0)], 171, sequence=seq), earliest=0, **kw)
