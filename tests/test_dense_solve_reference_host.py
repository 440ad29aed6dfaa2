"""The long-double reference of the reduced solve (tests/helpers/dense_solve_reference.py) on the CPU: held to mpmath on a small
system with a chain, its two solution paths held to each other, the routes its case tables name held to the planner
(svin_amd/csrc/solve_plan.hpp), and LAPACK in double held to every bar on every (family, shape) tests/test_gpu_dense_solve.py
runs -- a bar LAPACK missed would fail the reference, not the kernels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dense_solve_reference as dr     # noqa: E402
import solve_plan_lib as spl           # noqa: E402

LD = dr.LD


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return spl.build_shim(tmp_path_factory.mktemp("sp_dense"))


def weighted_rel(s, a, b):
    s, a, b = (np.asarray(v, dtype=LD) for v in (s, a, b))
    return float(np.sqrt(((s * (a - b)) ** 2).sum()) / np.sqrt(((s * b) ** 2).sum()))


# ------------------------------------------------------------------------------------------------ 1. against mpmath
def test_helper_equals_mpmath_at_d40_with_a_chain_of_two():
    """d = 40 = 22 kept rows + a chain of 2, fused with a clamped row: finalisation, solution and the chain quantities in 50
    digits.  Long double carries 64 bits: the solve's forward bound with u = 2^-64 (the bar of the GPU test's forward check, one
    precision up), the element-wise products to a few units of 2^-64."""
    import mpmath as mp
    mp.mp.dps = 50
    dC, n, mu = 22, 2, 1e-4
    sy = dr.make_system("A", dC, n, seed=3)
    d = sy["d"]
    hC = sy["hC"].copy()
    hC[4], hC[30] = 0.0, 1e-9
    S_fin, htil, sc = dr.finalize(sy["S"], hC, mu, fused=True)

    def to_ld(v):   # an mpf to long double through two doubles
        hi = float(v)
        return LD(hi) + LD(float(v - mp.mpf(hi)))
    # finalizeRow by hand
    ht_mp = []
    for i in range(d):
        h = mp.mpf(float(hC[i]))
        c = 1 / (1 + mp.sqrt(h))
        ht_mp.append(min(max(h * c * c, mp.mpf(1e-6)), mp.mpf(1e32)) / (c * c))
    assert ht_mp[4] == mp.mpf(1e-6) and abs(ht_mp[30] - mp.mpf(1e-6) * (1 + mp.sqrt(mp.mpf(1e-9))) ** 2) < mp.mpf(10) ** -40   # the lower clamp engages
    ht_ref = np.array([to_ld(v) for v in ht_mp])
    assert float((np.abs(htil - ht_ref) / ht_ref).max()) <= 8 * 2.0 ** -64   # (a square root, two divisions, three products)
    A = mp.matrix(d, d)
    for i in range(d):
        for j in range(d):
            A[i, j] = mp.mpf(float(sy["S"][i, j]))
        A[i, i] += mp.mpf(mu) * ht_mp[i]
    gm = mp.matrix([mp.mpf(float(v)) for v in sy["g"]])
    x_mp = mp.lu_solve(A, gm)
    x_ref = np.array([to_ld(x_mp[i]) for i in range(d)])
    s = dr.scale_of(S_fin)
    kappa = dr.jacobi_condition(S_fin)
    u = 2.0 ** -64
    x, L = dr.solve_factor(S_fin, sy["g"])
    assert weighted_rel(s, x, x_ref) <= kappa * d * (3 * d + 1) * u
    assert weighted_rel(s, dr.solve_refined(S_fin, sy["g"]), x_ref) <= 2.0 ** -58
    # chain quantities
    ks, ss = list(range(dC)), list(range(dC, d))
    Ass, Ask = A[dC:d, dC:d], A[dC:d, 0:dC]
    Zs = mp.inverse(Ass) * Ask                 # S_ss^-1 S_sk
    P_mp = Ask.T * Zs
    pg_mp = Ask.T * mp.lu_solve(Ass, mp.matrix([gm[i] for i in ss]))
    q = dr.chain_quantities(S_fin, sy["g"], dC, n)
    P_ref = np.array([[to_ld(P_mp[i, j]) for j in ks] for i in ks])
    Sp_ref = np.array([[to_ld(A[i, j] - P_mp[i, j]) for j in ks] for i in ks])
    gp_ref = np.array([to_ld(gm[i] - pg_mp[i]) for i in ks])
    sk = s[:dC]
    bar = 9 * n * (3 * 9 * n + 1) * u * dr.jacobi_condition(np.asarray(S_fin[dC:, dC:], dtype=np.float64))
    assert float((np.abs(q["P"] - P_ref) / np.outer(sk, sk)).max()) <= bar
    assert float((np.abs(q["Sprime"] - Sp_ref) / np.outer(sk, sk)).max()) <= bar
    assert float((np.abs(q["gprime"] - gp_ref) / (sk * np.abs(s * x_ref).sum())).max()) <= bar
    assert len(ss) == 9 * n and q["Z"].shape == (9 * n, dC + 1)
    # ... and the kept system solves to the kept part of x
    xk = dr.solve_factor(q["Sprime"], q["gprime"])[0]
    assert weighted_rel(sk, xk, x_ref[:dC]) <= kappa * d * (3 * d + 1) * u


def test_refinement_path_equals_factor_path_at_d600():
    sy = dr.make_system("A", 600, 0, seed=1)
    S_fin, _, _ = dr.finalize(sy["S"], sy["hC"], 1e-4, fused=True)
    s, kappa, d = dr.scale_of(S_fin), dr.jacobi_condition(S_fin), 600
    xf, _ = dr.solve_factor(S_fin, sy["g"])
    xr = dr.solve_refined(S_fin, sy["g"])
    assert weighted_rel(s, xf, xr) <= kappa * d * (3 * d + 1) * 2.0 ** -64 + 2.0 ** -58
    assert dr.LD_FACTOR_MAX == d   # (the largest system the factor path takes of its own accord)


def test_refinement_raises_when_it_cannot_converge():
    sy = dr.make_system("B", 40, 0)
    with pytest.raises(RuntimeError):
        dr.solve_refined(np.asarray(sy["S"], dtype=LD), sy["g"], max_steps=1)


def test_indefinite_system_has_exactly_one_negative_pivot():
    sy = dr.make_system("A", 84, 14)
    S = dr.make_indefinite(sy["S"], 84 + 9 * 3 + 8)
    s = np.sqrt(np.diag(sy["S"]))
    w = np.linalg.eigvalsh(S / np.outer(s, s))
    assert (w < 0).sum() == 1 and w[1] > 0.1
    with pytest.raises(ValueError):
        dr.chol_ld(S)


# ------------------------------------------------------------------------------------------------ 2. the tables' routes are the planner's
def test_case_tables_name_the_routes_the_planner_takes(lib):
    for route, rows in dr.NO_CHAIN.items():
        for d, _ in rows:
            q = spl.plan_one(lib, d)
            assert (q["chainMode"], spl.ROUTES[q["route"]]) == (0, route), d
    bits = {"SVIN_NO_LL": spl.NO_LL, "SVIN_NO_SB_ELIM": spl.NO_SB_ELIM, "SVIN_NO_LDS_BORDER": spl.NO_LDS_BORDER}
    for d, switch, route in dr.SWITCHED:
        assert spl.ROUTES[spl.plan_one(lib, d, switches=bits[switch])["route"]] == route
    q = spl.plan_one(lib, dr.WIDE_GRID_D)
    assert (spl.ROUTES[q["route"]], q["nb"], q["helperTasks"], q["bigChain_grid"]) == ("blocked", 31, 523, 256)
    assert spl.plan_one(lib, 1728)["bigChain_grid"] == 120   # (the largest system the window tests build)
    assert [spl.plan_one(lib, d)["nBackPanels"] for d in (512, 513, 1024, 1025)] == [1, 2, 2, 3]
    for d, route in dr.POSE_GRAPH:
        q = spl.plan_one(lib, d, padded=0)
        assert (spl.ROUTES[q["route"]], q["border"]) == (route, 0)
    for mode, route, dC, n, _ in dr.CHAIN:
        q = spl.plan_one(lib, dC + 9 * n, dC=dC, n=n)
        assert (q["chainMode"], spl.ROUTES[q["route"]], q["dSolve"]) == (mode, route, dC), (dC, n)
        assert spl.plan_one(lib, dC + 9 * n, dC=dC, n=n, switches=spl.NO_SB_ELIM)["chainMode"] == 0
    for route, dC, n in dr.DECLINED:
        q = spl.plan_one(lib, dC + 9 * n, dC=dC, n=n)
        assert (q["chainMode"], spl.ROUTES[q["route"]], q["dSolve"]) == (0, route, dC + 9 * n), (dC, n)


# ------------------------------------------------------------------------------------------------ 3. LAPACK meets every bar
def test_lapack_meets_every_bar_on_every_case(lib):
    worst = {}
    for family, dC, n in dr.all_cases() + [("A", dr.WIDE_GRID_D, 0)]:
        q = spl.plan_one(lib, dC + 9 * n, dC=dC, n=n)
        for fused in (False, True):
            if dC == dr.WIDE_GRID_D and fused:
                continue
            ref = dr.reference(family, dC, n, fused, border=q["border"])
            assert ref["kappa"] < (3e2 if family == "A" else 3e8)
            if family == "B":
                assert ref["kappa"] > 1e7
            # the plain bar: LAPACK substitutes with the factor itself, so it owes family B's tile factor nothing
            j = dr.judge(ref, ref["y_lapack"])
            assert j["backward"] <= 1.0 and j["forward"] <= 1.0, (family, dC, n, fused, j)
            key = (family, "backward")
            worst[key] = max(worst.get(key, 0.0), j["backward"])
            worst[family, "forward"] = max(worst.get((family, "forward"), 0.0), j["forward"])
            if family == "B":   # the factor the GPU test multiplies the bar with is finite and at least 1, for either elimination order
                for engaged in {False, q["chainMode"] != 0}:
                    f = dr.tile_factor(ref, engaged, q["border"] if engaged == (q["chainMode"] != 0) else 0)
                    assert 1.0 <= f < 1e6
    for edit in dr.EDGE_EDITS:   # the fused finalisation's edges: the shape of a case above, another S_fin
        ref = dr.reference("A", dr.EDGE_D, 0, True, edit=edit)
        j = dr.judge(ref, ref["y_lapack"])
        assert ref["kappa"] < 3e2 and j["backward"] <= 1.0 and j["forward"] <= 1.0, (edit[0], j)
        worst["A", "backward"] = max(worst["A", "backward"], j["backward"])
    print("LAPACK's largest ratio to a bar:", {k: "%.2e" % v for k, v in worst.items()})


def test_scratch_assemblers_read_back_a_known_factor():
    """the layouts the GPU test reads the factor from (kernels.hip k_chol_solve_ll, launchFactorBlocked), written here from a known L"""
    d = 209
    sy = dr.make_system("A", d, 0)
    L = np.asarray(dr.chol_ld(sy["S"]), dtype=np.float64)
    nT = (d + 15) // 16
    dpad = 16 * nT
    Lp = np.eye(dpad)
    Lp[:d, :d] = L
    scr = np.zeros(dpad * dpad)
    for I in range(nT):
        for j in range(I + 1):
            T = Lp[16 * I:16 * I + 16, 16 * j:16 * j + 16]
            if I == j:
                T = np.linalg.inv(T)
            scr[(I * (I + 1) // 2 + j) * 256:][:256] = T.ravel()
    scr[nT * (nT + 1) // 2 * 256:][:dpad] = 1.0 / np.diag(Lp)
    La, dinv = dr.assemble_ll_factor(scr, d)
    assert np.abs(np.asarray(La, dtype=np.float64) - L).max() <= 1e-13 * np.abs(L).max() and np.allclose(dinv * np.diag(L), 1.0, rtol=1e-15)
    dp = 256
    plan = dict(dp=dp, bigM_off=0, dinvG_off=(dp + 64) * dp, diagF_off=(dp + 64) * dp + dp)
    Lb = np.eye(dp)
    Lb[:d, :d] = L
    scr = np.full((dp + 64) * dp + dp + 64 * dp, 7.0)
    M = scr[:(dp + 64) * dp].reshape(dp + 64, dp)
    F = scr[plan["diagF_off"]:].reshape(dp // 64, 64, 64)
    for I in range(dp // 64):
        M[64 * I:64 * I + 64, :64 * I] = Lb[64 * I:64 * I + 64, :64 * I]
        F[I] = np.tril(Lb[64 * I:64 * I + 64, 64 * I:64 * I + 64]) + np.triu(np.full((64, 64), 7.0), 1)
    scr[plan["dinvG_off"]:][:dp] = 1.0 / np.diag(Lb)
    La, dinv = dr.assemble_blocked_factor(scr, plan, d)
    assert np.array_equal(np.asarray(La, dtype=np.float64), L) and np.array_equal(dinv, 1.0 / np.diag(L))
    assert dr.factor_ratio(np.asarray(sy["S"], dtype=LD), La) <= 1.0


# ------------------------------------------------------------------------------------------------ 4. the bars reject planted defects
def _tile_cholesky_solve(S_fin, g, drop=None, rsqrt_error=0.0):
    """a right-looking Cholesky over 16 x 16 tiles in double, as the device organises it, with a defect to order: `drop` = (I, J, K)
    leaves the update of tile (I, J) by tile column K out, rsqrt_error = relative error of every 1 / L_ii"""
    A = np.array(S_fin, dtype=np.float64)
    d = A.shape[0]
    nT = (d + 15) // 16
    t = lambda I: slice(16 * I, min(16 * I + 16, d))
    L = np.zeros_like(A)
    for K in range(nT):
        D = A[t(K), t(K)].copy()
        m = D.shape[0]
        Lk = np.zeros((m, m))
        for j in range(m):
            r = (1.0 + rsqrt_error) / np.sqrt(D[j, j] - Lk[j, :j] @ Lk[j, :j])
            Lk[j, j] = 1.0 / r
            Lk[j + 1:, j] = (D[j + 1:, j] - Lk[j + 1:, :j] @ Lk[j, :j]) * r
        L[t(K), t(K)] = Lk
        for I in range(K + 1, nT):
            L[t(I), t(K)] = np.linalg.solve(Lk, A[t(I), t(K)].T).T
        for I in range(K + 1, nT):
            for J in range(K + 1, I + 1):
                if (I, J, K) != drop:
                    A[t(I), t(J)] -= L[t(I), t(K)] @ L[t(J), t(K)].T
    import scipy.linalg as sla
    return sla.solve_triangular(L.T, sla.solve_triangular(L, np.asarray(g, dtype=np.float64), lower=True), lower=False)


def test_bars_reject_planted_defects():
    """the defects the bar of 1e-10 of max |y| let through (tests/test_gpu_reduced_solve.py): a tile update dropped in the row of
    the smallest weight, a row that misses its damping, reciprocal square roots at the hardware's 2^-26 -- each on d = 209 (the
    left-looking route's second size), fused with mu = 1e-4; the sound solve passes with the headroom LAPACK has"""
    ref = dr.reference("A", 209, 0, True)
    sound = dr.judge(ref, _tile_cholesky_solve(ref["S_fin"], ref["g"]))
    assert sound["backward"] <= 0.01 and sound["forward"] <= 0.01
    low = int(np.argmin(np.diag(ref["S"])[32:])) + 32   # (behind the first two tile rows, so that an update reaches it)
    dropped = dr.judge(ref, _tile_cholesky_solve(ref["S_fin"], ref["g"], drop=(low // 16, low // 16, 0)))
    assert dropped["backward"] > 1.0 and dropped["forward"] > 1.0
    undamped = np.array(ref["S_fin"])
    undamped[208, 208] = ref["S"][208, 208]   # the last row of the last tile keeps its diagonal as the build left it
    assert dr.judge(ref, _tile_cholesky_solve(undamped, ref["g"]))["backward"] > 1.0
    coarse = dr.judge(ref, _tile_cholesky_solve(ref["S_fin"], ref["g"], rsqrt_error=2.0 ** -26))
    assert coarse["backward"] > 1.0 and coarse["forward"] > 1.0
    # ... and the factor's own bar sees the dropped update where y is not looked at
    Lgood = np.linalg.cholesky(np.asarray(ref["S_fin"], dtype=np.float64))
    assert dr.factor_ratio(ref["S_fin"], Lgood) <= 1.0
    Lbad = Lgood.copy()
    Lbad[low, 3] = 0.0
    assert dr.factor_ratio(ref["S_fin"], Lbad) > 1.0
