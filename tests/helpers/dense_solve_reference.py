"""Long-double reference of the reduced solve (S + mu D) y = g (kernels.hip launchSolveReduced), the systems its tests feed the
solver through svin_ba_debug_solve_dense, and the bars they hold it to.  Shared by tests/test_dense_solve_reference_host.py (CPU)
and tests/test_gpu_dense_solve.py.

Reference.  finalize() restates finalizeRow (kernels.hip) in long double: sc = 1 / (1 + sqrt(hC)) (or the supplied scale),
htil = clamp(hC sc^2, 1e-6, 1e32) / sc^2, and the diagonal gains mu htil.  Up to d = 600 the solution comes from a Cholesky factor
computed in np.longdouble (64-bit significand on x86); above, from a LAPACK factor refined with long-double residuals until the
correction is below 2^-60 of |x|.  chain_quantities() gives what the chain elimination must reproduce whatever its elimination
order: S_ks S_ss^-1 S_sk, S' = S_kk - S_ks S_ss^-1 S_sk and g' = g_k - S_ks S_ss^-1 g_s (kept rows first, as the solver orders them).

Systems.  The factor is drawn in the order (chain, kept), R = [[B, 0], [E, R_k]] with B 9x9-block lower bidiagonal, E dense and
R_k dense lower triangular; S = R R^T is permuted to kept-first and scaled D S D with D = 10^U(1, 5), so that the chain part is
exactly block tridiagonal and the entries span 1e2 .. 1e10 as in a window.  Family A: diagonals of R in [1, 2], off-diagonals
0.3 / sqrt(d) N(0, 1) -- Jacobi-scaled condition number of a few hundred at most.  Family B (the mu = 1e-9 regime): family A with a
few diagonals of R_k and B shrunk to 1e-4, one per affected 16-tile (first, a middle and the last tile row of the kept part, one
in a border row where there is one, one in the middle chain block) -- Jacobi-scaled condition number 1e7 .. 1e8.  The column of R
below a shrunk diagonal is cleared: R^-1 has 1e4 on that diagonal, and an entry R_ki between two shrunk rows k > i would put
R_ki / (R_kk R_ii) ~ 1e6 into R^-1 -- a condition number of 1e13 and more, at which LAPACK itself stops with a negative pivot
(measured at d = 750) -- where the regime to be tested is the 1e8 of a window at mu = 1e-9.

Bars (eps = 2^-53, s_i = sqrt(S_ii), H = S / (s s^T), gamma = (3 d + 1) eps):
  backward   |S y - g|_i <= gamma s_i sum_j s_j |y_j|.  Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.4: the
             computed solution of a Cholesky solve satisfies (S + dS) y = g with |dS| <= gamma_{3n+1} |R^T| |R|, and
             (|R^T| |R|)_ij <= |r_i| |r_j| = s_i s_j by Cauchy-Schwarz.  Independent of summation order and of the scaling D.
  forward    |s o (y - x)|_2 <= kappa_2(H) d gamma |s o x|_2: the backward bound in the 2-norm of the Jacobi-scaled system
             (|dH|_2 <= |dH|_F <= d gamma) times its condition number.
  family B   the device substitutes through explicit inverses of 16 x 16 diagonal tiles (9 x 9 blocks in the chain, the whole
             border block), whose error grows with the tile's condition number: backward bar times max(1, kappa_inf of the worst
             diagonal tile of the long-double factor of H taken in the device's elimination order).  Forward bar unchanged.
             (The device turned out not to need the allowance: the GPU test asserts the plain bar on family B too.)
  factor     |S - L L^T|_ij <= (d + 1) eps s_i s_j / (1 - (d + 1) eps)  (Demmel, Applied Numerical Linear Algebra, sec. 2.7.3 /
             Higham Theorem 10.3 with the same Cauchy-Schwarz step): the factorisation alone.
"""
import numpy as np
import scipy.linalg as sla

LD = np.longdouble
EPS = 2.0 ** -53
LD_FACTOR_MAX = 600


def gamma(d):
    return (3 * d + 1) * EPS


def sym_from_lower(S):
    S = np.asarray(S)
    return np.tril(S) + np.tril(S, -1).T


# ---------------------------------------------------------------- finalisation
def finalize(S, hC=None, mu=0.0, fused=False, init_scale=True, scaleC=None):
    """-> (S_fin, htil, scale) in long double; unfused: the bare system (htil = 1, what the hook hands the solver)"""
    Sf = np.array(S, dtype=LD)
    d = Sf.shape[0]
    if not fused:
        return Sf, np.ones(d, LD), np.ones(d, LD)
    h = np.asarray(hC, dtype=LD)
    sc = LD(1) / (LD(1) + np.sqrt(h)) if init_scale else np.asarray(scaleC, dtype=LD)
    htil = np.minimum(np.maximum(h * sc * sc, LD(1e-6)), LD(1e32)) / (sc * sc)
    Sf[np.arange(d), np.arange(d)] += LD(mu) * htil
    return Sf, htil, sc


# ---------------------------------------------------------------- long-double Cholesky and substitutions
def chol_ld(A):
    """lower Cholesky factor in long double (left-looking by columns); ValueError on a pivot that is not positive"""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise ValueError("pivot %d is not positive: %g" % (j, float(v[0])))
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def forward_ld(L, B):
    """L^-1 B, L lower triangular, long double; B a vector or a matrix of columns"""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def backward_ld(L, B):
    """L^-T B"""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def solve_factor(S_fin, g):
    L = chol_ld(S_fin)
    return backward_ld(L, forward_ld(L, g)), L


def solve_refined(S_fin, g, max_steps=10):
    """iterative refinement of a LAPACK factor with long-double residuals; raises if the correction does not fall below
    2^-60 |x| within max_steps"""
    S_fin = np.asarray(S_fin, dtype=LD)
    g = np.asarray(g, dtype=LD)
    c = sla.cho_factor(S_fin.astype(np.float64), lower=True)
    x = np.asarray(sla.cho_solve(c, g.astype(np.float64)), dtype=LD)
    for _ in range(max_steps):
        r = g - S_fin @ x
        dx = np.asarray(sla.cho_solve(c, r.astype(np.float64)), dtype=LD)
        x = x + dx
        if float(np.abs(dx).max()) <= 2.0 ** -60 * float(np.abs(x).max()):
            return x
    raise RuntimeError("refinement did not reach 2^-60 in %d steps" % max_steps)


def solve_reference(S_fin, g, factor_path=False):
    """-> (x, L or None): the factor path up to LD_FACTOR_MAX unknowns, refinement above.  factor_path: the factor path whatever
    the size -- family B's one system above 600 unknowns: with residuals of 64 bits a correction cannot fall below
    kappa 2^-64 ~ 1e-12 of |x| at its condition number, and refinement's criterion of 2^-60 is out of reach"""
    if S_fin.shape[0] <= LD_FACTOR_MAX or factor_path:
        return solve_factor(S_fin, g)
    return solve_refined(S_fin, g), None


def lapack_solve(S_fin, g):
    """what LAPACK in double makes of the finalised system rounded to double"""
    c = sla.cho_factor(np.asarray(S_fin, dtype=np.float64), lower=True)
    return sla.cho_solve(c, np.asarray(g, dtype=np.float64))


# ---------------------------------------------------------------- chain quantities (order-independent)
def chain_quantities(S_fin, g, dC, n):
    """kept rows [0, dC), chain rows [dC, dC + 9 n): P = S_ks S_ss^-1 S_sk, pg = S_ks S_ss^-1 g_s, S' = S_kk - P, g' = g_k - pg, and
    Z = S_ss^-1 [S_sk | g_s] (the bar of the Y region is built from it)"""
    S_fin = np.asarray(S_fin, dtype=LD)
    g = np.asarray(g, dtype=LD)
    d = dC + 9 * n
    Sss, Ssk = S_fin[dC:d, dC:d], S_fin[dC:d, :dC]
    W = np.concatenate([Ssk, g[dC:d, None]], axis=1)
    Ls = chol_ld(Sss)
    Yr = forward_ld(Ls, W)
    Z = backward_ld(Ls, Yr)
    G = Yr.T @ Yr                     # [S_ks S_ss^-1 S_sk | S_ks S_ss^-1 g_s ; ... | g_s^T S_ss^-1 g_s]
    return dict(gram=G, P=G[:dC, :dC], pg=G[:dC, dC], Sprime=S_fin[:dC, :dC] - G[:dC, :dC], gprime=g[:dC] - G[:dC, dC], Z=Z)


# ---------------------------------------------------------------- systems
def shrink_positions(d_solve, border, n):
    """family B: (kept-local rows whose diagonal of R_k shrinks, chain-local rows of B that shrink)"""
    main = d_solve - border
    nT = (main + 15) // 16
    rows = []
    for T in sorted({0, nT // 2, nT - 1}):
        lo, hi = 16 * T, min(16 * T + 16, main)
        rows.append(lo + min(5, hi - lo - 1))
    if border:
        rows.append(main + border // 2)
    chain = [9 * (n // 2) + 4] if n else []
    return rows, chain


def make_system(family, dC, n=0, seed=0, border=0):
    """-> dict(S (d x d float64, symmetric), g, hC, d, dC, n).  The solver's ordering: kept rows first, then n chain blocks of 9.
    border: rows of the dense solve beyond 176 that the LDS-resident solver eliminates first (family B places a small pivot there)"""
    d, m = dC + 9 * n, 9 * n
    rng = np.random.default_rng([seed, dC, n, 0 if family == "A" else 1])
    off = 0.3 / np.sqrt(d)
    R = np.zeros((d, d))
    for b in range(n):   # B: lower-triangular diagonal blocks, dense blocks below them
        R[9 * b:9 * b + 9, 9 * b:9 * b + 9] = np.tril(rng.standard_normal((9, 9)) * off, -1)
        if b:
            R[9 * b:9 * b + 9, 9 * b - 9:9 * b] = rng.standard_normal((9, 9)) * off
    R[m:, :m] = rng.standard_normal((dC, m)) * off
    R[m:, m:] = np.tril(rng.standard_normal((dC, dC)) * off, -1)
    R[np.arange(d), np.arange(d)] = rng.uniform(1.0, 2.0, d)
    if family == "B":
        kept, chain = shrink_positions(dC, border, n)
        for q in [m + r for r in kept] + chain:
            R[q, q] = 1e-4
            R[q + 1:, q] = 0.0   # (see the module's text: keeps the small pivots from multiplying each other)
    elif family != "A":
        raise ValueError(family)
    S = R @ R.T
    perm = np.concatenate([np.arange(m, d), np.arange(m)])   # kept first
    S = S[np.ix_(perm, perm)]
    D = 10.0 ** rng.uniform(1.0, 5.0, d)
    S = sym_from_lower((S * D[:, None]) * D[None, :])
    s = np.sqrt(np.diag(S))
    g = s * rng.standard_normal(d)
    return dict(S=S, g=g, hC=np.diag(S).copy(), d=d, dC=dC, n=n, family=family)


def make_indefinite(S, k):
    """S with S_kk lowered so that the pivot of row k, eliminated last, is -1/2 of what it was: exactly one negative eigenvalue
    (a change of one diagonal entry has rank one), hence exactly one negative pivot in any elimination order"""
    S = np.array(S, dtype=np.float64)
    s = np.sqrt(np.diag(S))
    e = np.zeros(S.shape[0])
    e[k] = 1.0
    pivot = 1.0 / np.linalg.solve(S, e)[k]
    assert pivot > 0
    S[k, k] -= 1.5 * pivot
    w = np.linalg.eigvalsh(S / np.outer(s, s))   # (a congruence: the same inertia, without the scaling's spread)
    assert w[0] < 0 < w[1]
    return S


# ---------------------------------------------------------------- bars
def scale_of(S_fin):
    return np.sqrt(np.diag(np.asarray(S_fin, dtype=LD)))


def backward_ratio(S_fin, g, y, tile_factor=1.0):
    """max_i |S y - g|_i / (gamma s_i sum_j s_j |y_j| tile_factor): <= 1 meets the bar; also the residual in units of eps"""
    S_fin = np.asarray(S_fin, dtype=LD)
    y = np.asarray(y, dtype=LD)
    s = scale_of(S_fin)
    r = np.abs(S_fin @ y - np.asarray(g, dtype=LD))
    unit = s * (s @ np.abs(y))
    in_eps = float((r / unit).max()) / EPS
    return in_eps * EPS / (gamma(S_fin.shape[0]) * tile_factor), in_eps


def jacobi_condition(S_fin):
    S = np.asarray(S_fin, dtype=np.float64)
    s = np.sqrt(np.diag(S))
    w = np.linalg.eigvalsh(S / np.outer(s, s))
    return float(w[-1] / w[0])


def forward_ratio(S_fin, x_ref, y, kappa):
    """|s o (y - x)|_2 / (kappa d gamma |s o x|_2), and the relative error itself"""
    s = scale_of(S_fin)
    d = len(s)
    err = np.sqrt(((s * (np.asarray(y, dtype=LD) - x_ref)) ** 2).sum()) / np.sqrt(((s * x_ref) ** 2).sum())
    return float(err) / (kappa * d * gamma(d)), float(err)


def factor_ratio(S_fin, L):
    """max_ij |S - L L^T|_ij / ((d + 1) eps s_i s_j / (1 - (d + 1) eps))"""
    S_fin = np.asarray(S_fin, dtype=LD)
    L = np.asarray(L, dtype=LD)
    d = S_fin.shape[0]
    s = scale_of(S_fin)
    bar = (d + 1) * EPS / (1.0 - (d + 1) * EPS)
    return float((np.abs(S_fin - L @ L.T) / np.outer(s, s)).max()) / bar


def kappa_inf_lower(T):
    T = np.asarray(T, dtype=LD)
    Ti = forward_ld(T, np.eye(T.shape[0], dtype=LD))
    return float(np.abs(T).sum(axis=1).max() * np.abs(Ti).sum(axis=1).max())


def elimination_blocks(d, dC, n, chain_engaged, border):
    """the device's elimination order as (permutation, [(start, size) of every diagonal block it inverts explicitly]): the chain's
    9 x 9 blocks first where it is eliminated (in chain order: cyclic reduction inverts blocks of the same size), then the border
    block of the LDS-resident solver, then 16 x 16 tiles"""
    order, blocks = [], []
    d_solve = dC if chain_engaged else d
    if chain_engaged:
        order += list(range(dC, d))
        blocks += [(9 * b, 9) for b in range(n)]
    main = d_solve - border
    if border:
        blocks.append((len(order), border))
        order += list(range(main, d_solve))
    blocks += [(len(order) + t, min(16, main - t)) for t in range(0, main, 16)]
    order += list(range(main))
    return np.array(order), blocks


def tile_condition(S_fin, dC, n, chain_engaged, border):
    """kappa_inf of the worst diagonal block of the long-double factor in the device's elimination order"""
    d = S_fin.shape[0]
    order, blocks = elimination_blocks(d, dC, n, chain_engaged, border)
    assert sorted(order.tolist()) == list(range(d))
    s = scale_of(S_fin)   # the factor of the Jacobi-scaled system: row scaling changes kappa_inf, not the substitutions' relative errors
    L = chol_ld((np.asarray(S_fin, dtype=LD) / np.outer(s, s))[np.ix_(order, order)])
    return max(kappa_inf_lower(L[a:a + k, a:a + k]) for a, k in blocks)


# ---------------------------------------------------------------- the factor as the device leaves it in its scratch
def assemble_ll_factor(scratch, d):
    """left-looking solver (k_chol_solve_ll): tile (I, j), j <= I, at (I (I + 1) / 2 + j) * 256, row-major 16 x 16; a diagonal tile
    holds L_kk^-1 (what the substitutions multiply with), inverted here in long double.  -> (L (d x d long double), 1 / L_ii)"""
    nT = (d + 15) // 16
    dpad = 16 * nT
    L = np.zeros((dpad, dpad), LD)
    for I in range(nT):
        for j in range(I + 1):
            T = np.asarray(scratch[(I * (I + 1) // 2 + j) * 256:][:256], dtype=LD).reshape(16, 16)
            if I == j:
                T = forward_ld(np.tril(T), np.eye(16, dtype=LD))
            L[16 * I:16 * I + 16, 16 * j:16 * j + 16] = T
    dinv = np.asarray(scratch[nT * (nT + 1) // 2 * 256:][:dpad])
    return L[:d, :d], dinv[:d]


def assemble_blocked_factor(scratch, plan, d):
    """blocked solver (launchFactorBlocked's comment): bigM = (dp + 64) x dp row-major with L in the 64 x 64 blocks below the
    diagonal; diagF = per panel the 64 x 64 diagonal block, L on and below the diagonal (L_tt^-T in the strict upper triangle of
    its 16 x 16 diagonal tiles); dinvG = 1 / L_ii"""
    dp = plan["dp"]
    M = np.asarray(scratch[plan["bigM_off"]:][:(dp + 64) * dp]).reshape(dp + 64, dp)
    F = np.asarray(scratch[plan["diagF_off"]:][:dp * 64]).reshape(dp // 64, 64, 64)
    L = np.zeros((dp, dp))
    for I in range(dp // 64):
        L[64 * I:64 * I + 64, :64 * I] = M[64 * I:64 * I + 64, :64 * I]
        L[64 * I:64 * I + 64, 64 * I:64 * I + 64] = np.tril(F[I])
    dinv = np.asarray(scratch[plan["dinvG_off"]:][:dp])
    return np.asarray(L[:d, :d], dtype=LD), dinv[:d]


# ---------------------------------------------------------------- the cases both test files run
# window form without a chain: (d, family B as well)
NO_CHAIN = {
    "lds_whole": [(1, 0), (15, 0), (16, 0), (17, 0), (33, 0), (160, 0), (175, 0), (176, 1)],
    "lds_border_load": [(177, 0), (180, 1)],
    "lds_border_prepared": [(181, 0), (192, 0), (199, 0), (200, 1)],
    "left_looking": [(201, 0), (209, 0), (257, 0), (272, 1)],
    "blocked": [(273, 0), (320, 0), (321, 0), (511, 0), (512, 0), (513, 1), (1024, 0), (1025, 0)],
}
# the same with a route switch: (d, switch, route)
SWITCHED = [(177, "SVIN_NO_LDS_BORDER", "left_looking"), (200, "SVIN_NO_LDS_BORDER", "left_looking"), (201, "SVIN_NO_LL", "blocked")]
WIDE_GRID_D = 1921          # 31 block rows, 523 helper tasks: k_big_chol_chain on a grid of 256
POSE_GRAPH = [(176, "lds_whole"), (177, "left_looking"), (272, "left_looking"), (273, "blocked")]   # sPadded = 0, ldS = d + 37
# with a chain: (chain mode, route of the kept rows, dC, n, family B as well)
CHAIN = [
    (2, "lds_whole", 132, 8, 0), (2, "lds_whole", 84, 14, 1), (2, "lds_whole", 16, 21, 0), (2, "lds_whole", 174, 29, 0), (2, "lds_whole", 96, 64, 0),
    (2, "lds_border_load", 180, 10, 1),
    (2, "lds_border_prepared", 192, 32, 0), (2, "lds_border_prepared", 198, 33, 0),
    (2, "left_looking", 201, 8, 0), (2, "left_looking", 240, 40, 0),
    (1, "blocked", 273, 8, 0), (1, "blocked", 288, 48, 0), (1, "blocked", 300, 50, 1),
]
# the planner declines the chain: (route of the whole system, dC, n)
DECLINED = [("lds_border_prepared", 132, 7), ("blocked", 96, 65), ("blocked", 15, 30)]
MU = {"A": 1e-4, "B": 1e-9}   # of the fused runs
STAGE_MAX_D = 600


def all_cases():
    """every (family, dC, n) the GPU test solves in the window form"""
    out = []
    for rows in NO_CHAIN.values():
        for d, b in rows:
            out.append(("A", d, 0))
            if b:
                out.append(("B", d, 0))
    out += [("A", d, 0) for d, _, _ in SWITCHED if ("A", d, 0) not in out]
    for _, _, dC, n, b in CHAIN:
        out.append(("A", dC, n))
        if b:
            out.append(("B", dC, n))
    out += [("A", dC, n) for _, dC, n in DECLINED]
    return out


def _clamped_rows(sy):
    sy["hC"][3], sy["hC"][100] = 0.0, 1e-9   # the lower clamp of htil engages in both


def _supplied_scale(sy):
    _clamped_rows(sy)
    rng = np.random.default_rng(176)
    sy["init_scale"], sy["scaleC"] = False, rng.uniform(0.5, 1.0, sy["d"]) / (1.0 + np.sqrt(sy["hC"]))


# the fused finalisation's edges at d = 176: `edit` arguments of reference()
EDGE_D = 176
EDGE_EDITS = [("clamped", _clamped_rows), ("scaleC", _supplied_scale)]

_CACHE = {}


def reference(family, dC, n, fused, border=0, seed=0, edit=None):
    """the system, its finalised form and the long-double quantities the bars need, computed once per session.
    border: the border rows of the route the planner gives the system without a switch (they place one of family B's small pivots);
    edit: optional (name, function(system dict)) applied to the drawn system before anything is derived (the finalisation edges)"""
    key = (family, dC, n, bool(fused), border, seed, edit[0] if edit else None)
    if key in _CACHE:
        return _CACHE[key]
    sy = dict(make_system(family, dC, n, seed, border))
    if edit:
        edit[1](sy)
    mu = MU[family] if fused else 0.0
    S_fin, htil, _ = finalize(sy["S"], sy["hC"], mu, fused, sy.get("init_scale", True), sy.get("scaleC"))
    x, L = solve_reference(S_fin, sy["g"], factor_path=family == "B")
    ref = dict(sy, mu=mu, fused=fused, S_fin=S_fin, htil=htil, x=x, L=L, kappa=jacobi_condition(S_fin), tile={})
    ref["y_lapack"] = lapack_solve(S_fin, sy["g"])
    _CACHE[key] = ref
    return ref


def tile_factor(ref, chain_engaged, border):
    """family B: the factor on the backward bar for a solve that eliminates in this order; 1 for family A"""
    if ref["family"] != "B":
        return 1.0
    key = (bool(chain_engaged), border)
    if key not in ref["tile"]:
        ref["tile"][key] = max(1.0, tile_condition(ref["S_fin"], ref["dC"], ref["n"], chain_engaged, border))
    return ref["tile"][key]


def judge(ref, y, factor=1.0):
    """-> dict(backward ratio to its bar, residual in eps, the bar in eps, forward ratio to its bar, forward error)"""
    b, b_eps = backward_ratio(ref["S_fin"], ref["g"], y, factor)
    f, f_err = forward_ratio(ref["S_fin"], ref["x"], y, ref["kappa"])
    return dict(backward=b, backward_eps=b_eps, forward=f, forward_err=f_err, bar_eps=gamma(ref["d"]) * factor / EPS)
