"""Designed systems for the marginalisation algebra M2 / M3 (svin_amd/csrc/marg.hip from k_marg_lm_prepare to k_marg_final), a
long-double reference of it that takes no rank decision and no eigen-decomposition, a float64 NumPy restatement of the kernels'
arithmetic, and the bars both are held to.  Shared by tests/test_marg_reference_host.py (CPU) and tests/test_gpu_marg_edges.py,
which hands the systems to the job's own launches through svin_ba_debug_marginalize.

Systems.  H = G^T G, b = -G^T r with G and r small integers (|entry| <= 3), so every entry of H and b is exact in double, scaled
D H D, D b with D powers of two (still exact; family D: 2^U{-20..14}, and 2^-22 on the first kept column, the first marginalised
column and one column of every third landmark, so that diagonals below 1e-9 -- the 1e-3 branch of the three preconditioners --
exist in every group whatever the number of rows).  Columns of G: m dense columns (nk kept, nm marginalised, where marg_rows says) and
3 Lm landmark columns; landmark l has rows of its own (two per observation), so V is block diagonal as after M1.  A group of
columns (kept / marginalised / one landmark) is built from `base` columns drawn at random, `dependent` columns +-base_i +- base_j
(designed nullity), zero columns (H_ii = 0) and, family C, one column a + 2^-k z next to its partner a (z integer).  The group's
range is spanned by its base columns and z -- a well-conditioned integer basis known by design.  make_design() asserts exactness
by forming every product in long double and in double and comparing them.

Reference.  Eliminating a group of columns C from the least-squares problem |G x - r| is the orthogonal projection of every other
column and of r off range(C): Hk = G_k^T (I - Pi) G_k, bk = -G_k^T (I - Pi) r, Pi = C (C^T C)^-1 C^T, per landmark (disjoint rows)
and then for the marginalised dense block, with C the designed basis and a long-double Cholesky factor of C^T C (chol_ld /
forward_ld / backward_ld of dense_solve_reference.py).  The pseudo-inverse with the reference's rank rule (eigenvalues
<= eps n lambda_max of the Jacobi-scaled block are dropped) gives the same matrix whenever the designed non-zero eigenvalues are
kept: W and b lie in the range by construction, so a null direction contributes O(eps) on whichever side of the threshold its
computed eigenvalue lands.  M3: J^T J = Hk, J^T e0 = -bk, c0 = |Pi_k r|^2 (= x^T Hk x with Hk x = -bk) through the kept group's
basis.

The condition every case meets (check_condition; a design that misses it is redrawn with the next seed): with float64 eigvalsh
of each eliminated block and of Hk, scaled by the reference's preconditioner p_i = sqrt(H_ii) if H_ii > 1e-9 else 1e-3, every
designed non-zero eigenvalue is above `margin` x the threshold eps n lambda_max and every designed null eigenvalue is below the
threshold in magnitude.  margin = 1e3 -- except the one case built to make the Cholesky certificate of k_marg_final_chol fail
without a dropped eigenvalue: the certificate asks 1 / |R^-1|_F^2 > eps n^2 and lambda_max < n, so that case has to sit in
(eps n lambda_max, eps n^2), a window of n / lambda_max ~ 6 at n = 17 (32 rows of {-1, 0, 1}: lambda_max ~ 2.8); it takes margin 2
on both sides (CERT_MARGIN), against a computed eigenvalue that moves by a few eps lambda_max (0.1 of the threshold) and a last
pivot of the factorisation that moves by n eps (0.15 of the eigenvalue).

Bars, in Jacobi-scaled units (|dX_ij| / (s_i s_j), s = sqrt(diag) of the reference, 1 where the diagonal is zero; vectors over s and
over max(1, |b / s|_inf); c0 over max(1, c0)), all against the long-double reference:
  identities   J^T J vs Hk, J^T e0 vs -bk (Hk | bk as M3 was given them), Ht vs J^T J, bp vs J^T e0: c1 n eps, n = nk.  Held
               twice: in the units above (c1) and with s replaced by the rule's own preconditioner p (c3).  The two differ only
               where a diagonal is below 1e-9 (family D), and there the algorithm -- the reference's as much as the kernels' --
               is backward stable in p's units only: in sqrt(diag) units the restatement itself is off by 87 n eps on
               a case of family D, which sets c1 for every case.  The second bar keeps the other cases tight.
  forward      Hk, bk, c0 and U, ba after the landmark part: c2 kappa n eps.  kappa (float64 eigvalsh, it only scales the bar) is
               the condition number of the designed non-zero part of the scaled eliminated block: the worst landmark (n = 3) for
               U | ba, the larger of that and the dense block's (n = max(3, nm)) for Hk | bk; for c0 the condition number of Hk
               (n = nk) times the elimination's when an elimination ran ahead of M3 in the same call (a relative perturbation
               delta of Hk moves x^T Hk x by kappa(Hk) delta).
  c1, c3, c2 = 8 x the largest error / (n eps), error / (kappa n eps) the float64 restatement reaches over all cases (constants()).
  The device sums in other orders than LAPACK and forms N from a Cholesky factor or a one-sided Jacobi instead of eigh, hence
  the factor 8 (tests/test_gpu_covariance.py uses the same margin for the same reason).  The GPU test recomputes both constants
  from the restatement, so they cannot be tuned to the device.
  On this CPU (tests/test_marg_reference_host.py prints them): HOST_CONSTANTS below, with the cases that set them.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_solve_reference as dr   # noqa: E402
import marg_plan_lib as mpl          # noqa: E402

LD = np.longdouble
EPS = 2.220446049250313e-16
STAGE_LM, STAGE_DENSE, STAGE_FINAL = 1, 2, 4
MARGIN, CERT_MARGIN = 1e3, 2.0
EIG_MODES = ("default", "direct", "cholesky", "jacobi")   # SVIN_MARG_EIG 0 .. 3
# what constants() gave on the CPU this was written on, {class: (value, the case and quantity that set it)}; nothing reads it
HOST_CONSTANTS = {1: (697.2, "whole-D-Lm129-nk33-nm17, JtJ vs Hk"), 3: (5.854, "final-A-n2, Jte0 vs -bk (rule units)"), 2: (7.526, "final-A-n1, c0")}


# ---------------------------------------------------------------- designs
def _group(rng, row_mask, c, nullity, zeros, pair_k, dense_rows):
    """one group of c columns -> (columns, a basis of their range, its rank, the role of each column: b base, d dependent,
    0 zero, p the near-dependent partner of base column 0).  row_mask(n_base): the 0 / 1 pattern (rows x n_base) the base columns
    may fill; z of the pair lives on the first dense_rows rows."""
    n_pair = 1 if pair_k else 0
    n_base = c - nullity - zeros - n_pair
    assert n_base >= 0 and (not n_pair or n_base >= 1)
    lo = 1 if (nullity or n_pair) else 3
    mask = row_mask(n_base)
    R = mask.shape[0]
    base = rng.integers(-lo, lo + 1, (R, n_base)).astype(np.float64) * mask
    roles = np.array(["b"] * n_base + ["d"] * nullity + ["0"] * zeros + ["p"] * n_pair)
    roles = roles[rng.permutation(c)] if c else roles
    cols = np.zeros((R, c))
    z = np.zeros((R, n_pair))
    nb = 0
    for j, role in enumerate(roles):
        if role == "b":
            cols[:, j] = base[:, nb]
            nb += 1
        elif role == "d" and n_base >= 2:
            i, k = rng.choice(n_base, 2, replace=False)
            cols[:, j] = rng.choice([-1.0, 1.0]) * base[:, i] + rng.choice([-1.0, 1.0]) * base[:, k]
        elif role == "d" and n_base == 1:
            cols[:, j] = rng.choice([-1.0, 1.0]) * base[:, 0]
        elif role == "p":
            z[:dense_rows, 0] = rng.integers(-1, 2, dense_rows)
            cols[:, j] = base[:, 0] + 2.0 ** -pair_k * z[:, 0]
    return cols, np.concatenate([base, z], axis=1), n_base + n_pair, roles


LM_PATTERN_B = ("one", "rank1", "zero", "full")


def _lm_kappa(g, rank):
    V = g.T @ g
    d = np.sqrt(np.diag(V))
    if not d.all():
        return np.inf
    w = np.linalg.eigvalsh(V / np.outer(d, d))
    return w[-1] / w[3 - rank] if w[3 - rank] > 0 else np.inf


def _landmark(rng, kind):
    """-> (G_l (rows x 3), basis (rows x rank)).  A block of full rank or of one observation is drawn again until the condition
    number of its scaled V (its non-zero part) is below 50: the worst of a few hundred random blocks would otherwise set kappa"""
    if kind == "full":
        while True:
            g = rng.integers(-3, 4, (4, 3)).astype(np.float64)
            if _lm_kappa(g, 3) < 50:
                return g, g
    if kind == "one":       # one observation: V of rank 2, its range all of the two rows
        while True:
            g = rng.integers(-3, 4, (2, 3)).astype(np.float64)
            if _lm_kappa(g, 2) < 50:
                return g, np.eye(2)
    if kind == "rank1":
        u = rng.integers(-1, 2, 4).astype(np.float64)
        u[rng.integers(4)] = 1.0
        v = rng.integers(-3, 4, 3).astype(np.float64)
        v[rng.integers(3)] = 3.0
        return np.outer(u, v), u[:, None]
    assert kind == "zero"   # a constant landmark: every landmark Jacobian is zero
    return np.zeros((2, 3)), np.zeros((2, 0))


def make_design(nk, nm, Lm, seed, interleaved=False, null_m=0, null_k=0, zero_k=0, pair_m=None, pair_k=None, lm_pattern=("full",),
                scale=False, rows_d=None, short=False):
    """-> dict: the system U | ba | W | V | bb | marg_rows in the hook's layout and what the reference needs of its construction"""
    rng = np.random.default_rng([seed, nk, nm, Lm, 7])
    m = nk + nm
    if interleaved and nm and nk:
        marg_pos = np.unique(np.floor((np.arange(nm) + 0.5) * m / nm).astype(int))
        assert len(marg_pos) == nm
    else:
        marg_pos = np.arange(nm)            # contiguous: the marginalised (oldest) blocks first
    marg_rows = np.zeros(m, np.int32)
    marg_rows[marg_pos] = 1
    keep = np.flatnonzero(marg_rows == 0)
    marg = np.flatnonzero(marg_rows == 1)
    if short:
        assert Lm == 0 and nm == 0 and rows_d is not None and rows_d < nk
    Rd = 0 if m == 0 else (rows_d if rows_d is not None else 2 * m + 8)
    kinds = [lm_pattern[l % len(lm_pattern)] for l in range(Lm)]
    lm = [_landmark(rng, k) for k in kinds]
    lm_rows, R = [], Rd
    for g, _ in lm:
        lm_rows.append((R, R + g.shape[0]))
        R += g.shape[0]
    p_touch = min(1.0, 6.0 / max(m, 1))

    def row_mask(n_base):
        mk = np.ones((R, n_base))
        mk[Rd:] = rng.random((R - Rd, n_base)) < p_touch
        if n_base >= 2:
            mk[Rd:, n_base - 1] = 0.0   # one base column per group no landmark touches: its row of W is zero
        return mk
    Gk, Bk, rk, roles_k = _group(rng, row_mask, nk, null_k, zero_k, pair_k, Rd)
    Gm, Bm, rm, roles_m = _group(rng, row_mask, nm, null_m, 0, pair_m, Rd)
    if short:
        Bk, rk = np.eye(Rd), Rd
    Gd = np.zeros((R, m))
    Gd[:, keep], Gd[:, marg] = Gk, Gm
    r = rng.integers(-3, 4, R).astype(np.float64)
    D = 2.0 ** rng.integers(-20, 15, m + 3 * Lm) if scale else np.ones(m + 3 * Lm)
    if scale:   # the 1e-3 branch of every preconditioner is reached by design: diagonals below 1e-9 in each group
        for j in ([keep[0]] if nk else []) + ([marg[0]] if nm else []) + [m + 9 * l for l in range((Lm + 2) // 3)]:
            D[j] = 2.0 ** -22
    Dd, Dl = D[:m], D[m:].reshape(Lm, 3)
    Gs = Gd * Dd
    U, ba = Gs.T @ Gs, -(Gs.T @ r)
    W, V, bb = np.zeros((m, 3 * Lm)), np.zeros((Lm, 9)), np.zeros(3 * Lm)
    Gls = []
    for l, ((a, b), (g, _)) in enumerate(zip(lm_rows, lm)):
        gs = g * Dl[l]
        Gls.append(gs)
        W[:, 3 * l:3 * l + 3] = Gs[a:b].T @ gs
        V[l] = (gs.T @ gs).ravel()
        bb[3 * l:3 * l + 3] = -(gs.T @ r[a:b])
    # exactness: the same products in long double
    GsL, rL = Gs.astype(LD), r.astype(LD)
    assert np.array_equal((GsL.T @ GsL).astype(np.float64), U) and np.array_equal(GsL.T @ GsL, U.astype(LD))
    assert np.array_equal(-(GsL.T @ rL), ba.astype(LD))
    for l, ((a, b), gs) in enumerate(zip(lm_rows, Gls)):
        gl = gs.astype(LD)
        assert np.array_equal(GsL[a:b].T @ gl, W[:, 3 * l:3 * l + 3].astype(LD))
        assert np.array_equal((gl.T @ gl).ravel(), V[l].astype(LD)) and np.array_equal(-(gl.T @ rL[a:b]), bb[3 * l:3 * l + 3].astype(LD))
    assert np.abs(Gd).max(initial=0) <= 3.0 + 1e-12 and np.abs(r).max(initial=0) <= 3
    return dict(m=m, nk=nk, nm=nm, Lm=Lm, marg_rows=marg_rows, keep=keep, marg=marg, U=U, ba=ba, W=W, V=V, bb=bb,
                Gs=Gs, r=r, Bk=Bk, Bm=Bm, rk=rk, rm=rm, lm_rows=lm_rows, lm_basis=[b for _, b in lm], lm_rank=[b.shape[1] for _, b in lm],
                kinds=kinds, zero_kept=int((roles_k == "0").sum()), Rd=Rd)


# ---------------------------------------------------------------- the long-double reference
def _project_off(X, C):
    """X - C (C^T C)^-1 C^T X in long double"""
    if C.shape[1] == 0:
        return X
    L = dr.chol_ld(C.T @ C)
    return X - C @ dr.backward_ld(L, dr.forward_ld(L, C.T @ X))


def reference(ds, stages):
    """-> dict(U, ba after the landmark part; Hk, bk; JtJ, Jte0, c0) in long double, None where the stage does not apply"""
    m, nk, nm = ds["m"], ds["nk"], ds["nm"]
    X = np.concatenate([ds["Gs"], ds["r"][:, None], ds["Bm"], ds["Bk"]], axis=1).astype(LD)
    if stages & STAGE_LM:
        for (a, b), C in zip(ds["lm_rows"], ds["lm_basis"]):
            X[a:b] = _project_off(X[a:b], C.astype(LD))
    else:
        assert ds["Lm"] == 0, "a system with landmarks whose landmark part does not run has no reduced form"
    Gp, rp = X[:, :m], X[:, m]
    out = dict(U=Gp.T @ Gp, ba=-(Gp.T @ rp), Hk=None, bk=None, JtJ=None, Jte0=None, c0=None)
    if not (stages & STAGE_DENSE) or nk == 0:
        return out
    Bm, Bk = X[:, m + 1:m + 1 + ds["rm"]], X[:, m + 1 + ds["rm"]:]
    Y = _project_off(np.concatenate([Gp[:, ds["keep"]], rp[:, None], Bk], axis=1), Bm)
    Xk, rr, Bk = Y[:, :nk], Y[:, nk], Y[:, nk + 1:]
    out.update(Hk=Xk.T @ Xk, bk=-(Xk.T @ rr))
    if stages & STAGE_FINAL:
        c0 = LD(0)
        if ds["rk"]:
            y = dr.forward_ld(dr.chol_ld(Bk.T @ Bk), Bk.T @ rr)
            c0 = y @ y
        out.update(JtJ=out["Hk"], Jte0=-out["bk"], c0=c0)
    return out


# ---------------------------------------------------------------- the condition on every case, and the condition numbers
def p_rule(d):
    d = np.asarray(d, dtype=np.float64)
    return np.where(d > 1.0e-9, np.sqrt(np.abs(d)), 1.0e-3)


def _block(A, rank, margin, cert=False):
    """eigenvalues of a block scaled by the rule's preconditioner -> (the condition holds, kappa of the designed non-zero part)"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    if n == 0:
        return True, 1.0
    p = p_rule(np.diag(A))
    w = np.linalg.eigvalsh(0.5 * (A + A.T) / np.outer(p, p))
    if w[-1] <= 0.0:
        return rank == 0, 1.0
    thr = EPS * n * w[-1]
    nz, null = w[n - rank:], w[:n - rank]
    ok = bool(np.all(nz > margin * thr)) and bool(np.all(np.abs(null) < thr))
    if cert and ok:   # the certificate of k_marg_final_chol has to fail with the same margin: 1 / trace(A^-1) <= lambda_min
        ok = margin * nz[0] < EPS * n * n
    return ok, (float(w[-1] / nz[0]) if rank and nz[0] > 0 else 1.0)


def check_condition(ds, ref, stages, margin=MARGIN, cert=False):
    """-> (holds, dict(kappa_L, kappa_M, kappa_K))"""
    ok, kL, kM, kK = True, 1.0, 1.0, 1.0
    if stages & STAGE_LM:
        for l in range(ds["Lm"]):
            if ds["kinds"][l] == "zero":
                continue
            o, k = _block(ds["V"][l].reshape(3, 3), ds["lm_rank"][l], margin)
            ok, kL = ok and o, max(kL, k)
    if ref["Hk"] is not None:
        if ds["nm"]:
            U1 = ref["U"].astype(np.float64)
            o, kM = _block(U1[np.ix_(ds["marg"], ds["marg"])], ds["rm"], margin)
            ok = ok and o
        o, kK = _block(ref["Hk"].astype(np.float64), ds["rk"], margin, cert)
        ok = ok and o
    return ok, dict(kappa_L=kL, kappa_M=kM, kappa_K=kK)


# ---------------------------------------------------------------- the float64 restatement of the kernels' arithmetic
def _pinv_factor(Vs, n_rule):
    """N with N N^T = Vs^+ by eigh and the rank rule -> (N, dropped)"""
    w, Q = np.linalg.eigh(Vs)
    tol = EPS * n_rule * w.max()
    keep = w > tol
    sc = np.zeros_like(w)
    sc[keep] = np.sqrt(1.0 / w[keep])
    return Q * sc, int((~keep).sum())


def restate(ds, stages):
    """what the kernels compute, in float64 NumPy with LAPACK's eigh: the same keys as Estimator.debug_marginalize, and `dropped`"""
    m, nk, Lm = ds["m"], ds["nk"], ds["Lm"]
    U, ba = ds["U"].copy(), ds["ba"].copy()
    out = dict(U=U, ba=ba, Hk=None, bk=None, J=None, e0=None, Ht=None, bp=None, c0=None, dropped=None)
    if (stages & STAGE_LM) and m > 0:
        for l in range(Lm):
            V = ds["V"][l].reshape(3, 3)
            if V[0, 0] == 0.0 and V[1, 1] == 0.0 and V[2, 2] == 0.0:
                continue
            pb = p_rule(np.diag(V))
            N, _ = _pinv_factor(V / np.outer(pb, pb), 3)
            N = N / pb[:, None]
            Wl = ds["W"][:, 3 * l:3 * l + 3]
            ba -= Wl @ (N @ (N.T @ ds["bb"][3 * l:3 * l + 3]))
            Mu = Wl @ N
            U -= Mu @ Mu.T
    if not (stages & STAGE_DENSE) or nk == 0:
        return out
    keep, marg = ds["keep"], ds["marg"]
    if ds["nm"]:
        Vm = U[np.ix_(marg, marg)]
        pm = p_rule(np.diag(Vm))
        N, _ = _pinv_factor(0.5 * (Vm + Vm.T) / np.outer(pm, pm), ds["nm"])
        N = N / pm[:, None]
        Mu = U[np.ix_(keep, marg)] @ N
        Hk = U[np.ix_(keep, keep)] - Mu @ Mu.T
        bk = ba[keep] - Mu @ (N.T @ ba[marg])
    else:
        Hk, bk = U.copy(), ba.copy()
    out.update(Hk=Hk, bk=bk)
    if stages & STAGE_FINAL:
        p = p_rule(np.diag(Hk))
        w, Q = np.linalg.eigh(0.5 * (Hk + Hk.T) / np.outer(p, p))
        kept = w > EPS * nk * w.max()
        sq = np.where(kept, np.sqrt(np.abs(w)), 0.0)
        J = (p[:, None] * Q * sq).T
        with np.errstate(divide="ignore"):
            e0 = np.where(kept, -(Q.T @ (bk / p)) / np.where(kept, sq, 1.0), 0.0)
        out.update(J=J, e0=e0, Ht=J.T @ J, bp=J.T @ e0, c0=float(e0 @ e0), dropped=int((~kept).sum()))
    return out


# ---------------------------------------------------------------- errors in scaled units and the bars
def _scale(diag):
    d = np.asarray(diag, dtype=LD)
    return np.where(d > 0, np.sqrt(np.abs(d)), LD(1))


def _mat_err(X, ref, s):
    return float((np.abs(np.asarray(X, dtype=LD) - ref) / np.outer(s, s)).max(initial=0))


def _vec_err(v, ref, s):
    return float((np.abs(np.asarray(v, dtype=LD) - ref) / s).max(initial=0) / max(LD(1), (np.abs(ref) / s).max(initial=0)))


def errors(case, res):
    """-> {quantity: (error in scaled units, the bar without its constant, class 1 (identity) | 2 (forward))} for a result `res` of
    the hook or of restate() on this case"""
    ds, ref, stages, kp = case["ds"], case["ref"], case["stages"], case["kappa"]
    out = {}
    lm_ran = bool(stages & STAGE_LM) and ds["Lm"] > 0 and ds["m"] > 0
    if lm_ran:
        s = _scale(np.diag(ref["U"]))
        bar = kp["kappa_L"] * 3 * EPS
        out["U"] = (_mat_err(res["U"], ref["U"], s), bar, 2)
        out["ba"] = (_vec_err(res["ba"], ref["ba"], s), bar, 2)
        out["U symmetry"] = (_mat_err(res["U"], np.asarray(res["U"], dtype=LD).T, s), bar, 2)
    if ref["Hk"] is None:
        return out
    s = _scale(np.diag(ref["Hk"]))
    k_elim = max(kp["kappa_L"] if lm_ran else 1.0, kp["kappa_M"])
    eliminated = lm_ran or ds["nm"] > 0
    bar = k_elim * max(3 if lm_ran else 1, ds["nm"]) * EPS
    out["Hk"] = (_mat_err(res["Hk"], ref["Hk"], s), bar, 2)
    out["bk"] = (_vec_err(res["bk"], ref["bk"], s), bar, 2)
    if ref["JtJ"] is None:
        return out
    n = ds["nk"]
    J, e0 = np.asarray(res["J"], dtype=LD), np.asarray(res["e0"], dtype=LD)
    JtJ, Jte0 = J.T @ J, J.T @ e0
    Hin, bin_ = np.asarray(res["Hk"], dtype=LD), np.asarray(res["bk"], dtype=LD)
    Hs = 0.5 * (Hin + Hin.T)
    # (the literal units s = sqrt(diag), class 1, and the units of the rule's own preconditioner, class 3: they differ where a
    # diagonal is below 1e-9, and there the algorithm is backward stable in the rule's units only)
    for units, sc, cls in (("", s, 1), (" (rule units)", np.asarray(p_rule(np.diag(ref["Hk"]).astype(np.float64)), dtype=LD), 3)):
        out["JtJ vs Hk" + units] = (_mat_err(JtJ, Hs, sc), n * EPS, cls)
        out["Jte0 vs -bk" + units] = (_vec_err(Jte0, -bin_, sc), n * EPS, cls)
        out["Ht vs JtJ" + units] = (_mat_err(res["Ht"], JtJ, sc), n * EPS, cls)
        out["bp vs Jte0" + units] = (_vec_err(res["bp"], Jte0, sc), n * EPS, cls)
    c0 = float(ref["c0"])
    out["c0"] = (abs(float(LD(res["c0"]) - ref["c0"])) / max(1.0, c0), kp["kappa_K"] * (k_elim if eliminated else 1.0) * n * EPS, 2)
    return out


def constants(cases):
    """-> {class: (constant, the case and quantity that set it)}: 8 x the restatement's largest error / bar over the cases"""
    worst = {1: (0.0, ""), 2: (0.0, ""), 3: (0.0, "")}
    for case in cases:
        for q, (err, bar, cls) in errors(case, case["restated"]).items():
            if err / bar > worst[cls][0]:
                worst[cls] = (err / bar, "%s, %s" % (case["name"], q))
    return {cls: (8.0 * w, who) for cls, (w, who) in worst.items()}


def ratios(case, res, consts):
    """-> {quantity: error / (constant x bar)}: <= 1 meets the bar"""
    return {q: err / (consts[cls][0] * bar) for q, (err, bar, cls) in errors(case, res).items()}


# ---------------------------------------------------------------- cases
_CACHE = {}


def build(spec):
    """the design (redrawn until the condition holds), its reference, condition numbers and restatement, once per session"""
    if spec["name"] in _CACHE:
        return _CACHE[spec["name"]]
    kw = {k: v for k, v in spec.items() if k not in ("name", "family", "stages", "margin", "cert", "group")}
    for seed in range(spec.get("seed", 0), spec.get("seed", 0) + 200):
        kw["seed"] = seed
        ds = make_design(**kw)
        try:
            ref = reference(ds, spec["stages"])
        except ValueError:      # a designed basis came out dependent
            continue
        ok, kappa = check_condition(ds, ref, spec["stages"], spec.get("margin", MARGIN), spec.get("cert", False))
        if ok:
            break
    else:
        raise AssertionError("%s: no seed meets the eigenvalue condition" % spec["name"])
    case = dict(spec, ds=ds, ref=ref, kappa=kappa, seed_used=seed)
    case["restated"] = restate(ds, spec["stages"])
    _CACHE[spec["name"]] = case
    return case


def plan_of(lib, m, Lm, nk, nm, eig=0):
    q = mpl.plan(lib, [(m, Lm, 0, 0, nk, nm, 0, 0, 0, 0, 0, eig, mpl.JACOBI_SHARED)])
    return {k: int(v[0]) for k, v in q.items()}


PLAN_FIELDS = ("lmPrepare_grid", "lmApply_grid", "lmUpdate_grid", "dense_grid", "denseUseLds", "denseProdLds", "denseTileChol", "copyPair",
               "finalChol_grid", "finalDc_grid", "final_grid", "finalMode", "finalFallbackLds", "finalSkipIfDone")


def masked_plan(lib, case, eig=0):
    """the plan fields the hook reports for this case: planMargJob's with the stages the mask leaves out taken out"""
    ds, st = case["ds"], case["stages"]
    q = plan_of(lib, ds["m"], ds["Lm"], ds["nk"], ds["nm"], eig)
    out = {k: q[k] for k in PLAN_FIELDS}
    if not st & STAGE_LM:
        out.update(lmPrepare_grid=0, lmApply_grid=0, lmUpdate_grid=0)
    if not st & STAGE_DENSE:
        out.update(dense_grid=0, copyPair=0)
    if not st & STAGE_FINAL:
        out.update(finalChol_grid=0, finalDc_grid=0, final_grid=0)
    return out


def final_modes(lib, n):
    """the SVIN_MARG_EIG settings whose plans of M3 differ at this size, the first of each"""
    seen, out = set(), []
    for eig, name in enumerate(EIG_MODES):
        q = plan_of(lib, n, 0, n, 0, eig)
        key = tuple(q[k] for k in PLAN_FIELDS[8:])
        if key not in seen:
            seen.add(key)
            out.append(name)
    return out


def last_where(lib, field, value, fixed, lo=1, hi=1024):
    """the largest size n in [lo, hi] for which the plan of fixed(n) = (m, Lm, nk, nm) has field == value (and n + 1 has not)"""
    best = None
    for n in range(lo, hi + 1):
        if plan_of(lib, *fixed(n))[field] == value:
            best = n
    assert best is not None and best < hi, (field, value)
    return best


LM_SIZES = (0, 1, 2, 4, 127, 128, 129, 255, 256, 257)
M_SIZES = (1, 15, 16, 17, 33)
NM_SIZES = (1, 6, 15, 16, 17, 27, 33)
FAMILY_KW = dict(A={}, D=dict(scale=True))


def landmark_specs():
    out = []
    for Lm in LM_SIZES:
        for m in M_SIZES:
            nm = m // 3
            for fam in "ABD":
                kw = dict(lm_pattern=LM_PATTERN_B) if fam == "B" else FAMILY_KW[fam]
                out.append(dict(name="lm-%s-Lm%d-m%d" % (fam, Lm, m), group="landmark", family=fam, stages=STAGE_LM, nk=m - nm, nm=nm, Lm=Lm,
                                interleaved=bool((Lm + m) & 1), **kw))
    return out


def dense_specs(lib):
    out = []

    def add(fam, nk, nm, tag="", stages=STAGE_DENSE, Lm=0, **kw):
        out.append(dict(name="dense-%s-nk%d-nm%d%s" % (fam, nk, nm, tag), group="dense", family=fam, stages=stages, nk=nk, nm=nm, Lm=Lm, **kw))
    for nm in NM_SIZES:
        add("A", 17, nm)
    for nm in (6, 17, 27):
        add("A", 17, nm, "-interleaved", interleaved=True)
    for nk in (1, 16, 117):
        add("A", nk, 27)
    add("A", 117, 27, "-interleaved", interleaved=True)
    edge = last_where(lib, "denseProdLds", 1, lambda n: (n + 27, 0, n, 27))
    add("A", edge, 27, "-prodLds-last")
    add("A", edge + 1, 27, "-prodLds-first-global")
    for nm, nul in ((1, 1), (17, 1), (27, 6), (33, 11)):
        add("B", 17, nm, "-null%d" % nul, null_m=nul)
    add("B", 17, 27, "-null6-interleaved", null_m=6, interleaved=True)
    for k in (7, 13):
        for nm in (17, 33):
            add("C", 17, nm, "-k%d" % k, pair_m=k)
    add("D", 17, 17, scale=True)
    add("D", 16, 27, scale=True)
    add("A", 17, 0, "-copy")
    add("A", 17, 0, "-copy-Lm4", stages=STAGE_LM | STAGE_DENSE, Lm=4)
    add("A", 0, 17, "-nothing-kept")
    return out


def final_sizes(lib):
    edge = last_where(lib, "finalMode", 4, lambda n: (n, 0, n, 0), hi=400)
    return (1, 2, 15, 16, 17, 33, 96, 97, 127, 128, 129, edge, edge + 1), edge + 1


def final_specs(lib):
    sizes, first6 = final_sizes(lib)
    st = STAGE_DENSE | STAGE_FINAL
    out = []

    def add(fam, n, tag="", **kw):
        out.append(dict(name="final-%s-n%d%s" % (fam, n, tag), group="final", family=fam, stages=st, nk=n, nm=0, Lm=0, **kw))
    for n in sizes:
        add("A", n)
    for n in (17, 33, 128, first6):
        add("B", n, "-null", null_k=max(1, n // 3), zero_k=1)
        for k in (7, 13):
            add("C", n, "-k%d" % k, pair_k=k)
    add("B", 33, "-short", rows_d=22, short=True)
    for n in (17, 128):
        add("D", n, scale=True)
    # the certificate of k_marg_final_chol fails, nothing is dropped: 32 rows of {-1, 0, 1}
    add("C", 17, "-cert", pair_k=21, rows_d=32, margin=CERT_MARGIN, cert=True)
    return out


WHOLE_SIZES = ((129, 33, 17), (257, 117, 27))


def whole_specs():
    st = STAGE_LM | STAGE_DENSE | STAGE_FINAL
    out = []
    for Lm, nk, nm in WHOLE_SIZES:
        fam_kw = dict(A={}, B=dict(lm_pattern=LM_PATTERN_B, null_m=nm // 3, null_k=nk // 3, zero_k=1), C=dict(pair_m=7), D=dict(scale=True))
        for fam in "ABCD":
            out.append(dict(name="whole-%s-Lm%d-nk%d-nm%d" % (fam, Lm, nk, nm), group="whole", family=fam, stages=st, nk=nk, nm=nm, Lm=Lm,
                            interleaved=fam in "BD", **fam_kw[fam]))
    out.append(dict(name="whole-A-nothing-kept", group="whole", family="A", stages=st, nk=0, nm=6, Lm=4))
    out.append(dict(name="whole-A-no-dense-rows", group="whole", family="A", stages=st, nk=0, nm=0, Lm=4))
    return out


def all_specs(lib):
    return landmark_specs() + dense_specs(lib) + final_specs(lib) + whole_specs()


def expected_final_route(case, mode, plan):
    """flag[3] the design and the plan predict: -8 certified Cholesky, -7 direct eigen-solve, -4 / -6 the Cholesky-preconditioned
    Jacobi in LDS / in global memory, 0 the Jacobi fall-back"""
    deficient = case["ds"]["rk"] < case["ds"]["nk"] or case.get("cert", False)
    if plan["finalChol_grid"] and not deficient:
        return -8
    if plan["finalDc_grid"]:
        return -7
    return {4: -4, 6: -6, 1: 0, 0: 0}[plan["finalMode"]]
