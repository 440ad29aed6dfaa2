"""The reduced-system solver (kernels.hip launchSolveReduced) on systems handed to it directly, at the edges of every route
solve_plan.hpp knows: through svin_ba_debug_solve_dense, which runs launchSolveReduced itself on a minimal problem view, against
the long-double reference and the derived bars of tests/helpers/dense_solve_reference.py (read its text for where each bar
comes from; tests/test_dense_solve_reference_host.py shows on the CPU that LAPACK meets every one of them on every case here).

Per case: the plan the library took is the plan the planner gives (route, chain mode, border rows, grid: a test that silently
ran another route would prove nothing), cholFail == 0, the backward bar on S y - g row by row, the forward bar on y - x_ref.
Family A also reads the solver's scratch, which is filled with NaN beforehand (a window's scratch is not cleared either: nothing
may depend on what it held): the factor the left-looking and the blocked route leave behind (Demmel's bound for the factorisation
alone; 1 / L_ii), the chain's Y region (Y^T Y against S_ks S_ss^-1 [S_sk | g_s]) and the compact kept system S' | g'.
Every line printed is `route; d; device residual / bar; LAPACK residual / bar; forward error` (residuals and bars in eps)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dense_solve_reference as dr     # noqa: E402
import solve_plan_lib as spl           # noqa: E402

pytestmark = pytest.mark.gpu
LD = dr.LD
SWITCH_BITS = {"SVIN_NO_LL": spl.NO_LL, "SVIN_NO_SB_ELIM": spl.NO_SB_ELIM, "SVIN_NO_LDS_BORDER": spl.NO_LDS_BORDER}
NAN_FILL = 0xFF


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return spl.build_shim(tmp_path_factory.mktemp("sp_gpu_dense"))


def window_buffer(S):
    """the window's form: d rounded up to 16 rows of as many doubles, zero beyond row / column d"""
    d = S.shape[0]
    dpad = (d + 15) // 16 * 16
    buf = np.zeros((dpad, dpad))
    buf[:d, :d] = S
    return buf, dpad


def solve(planner, ref, switches=(), set_option=None, S=None, scratch=False, fill=0, form="window"):
    """one call of the hook on the reference's system (or on S in its place) -> (result, the planner's plan, the buffer handed over)"""
    from svin_amd.estimator import Estimator
    for name in switches:
        set_option(name, 1)
    S = ref["S"] if S is None else S
    d, dC, n = ref["d"], ref["dC"], ref["n"]
    bits = sum(SWITCH_BITS[name] for name in switches)
    kw = dict(mu=ref["mu"], fused=ref["fused"], init_scale=ref.get("init_scale", True), hC=ref["hC"], scaleC=ref.get("scaleC"),
              want_scratch=scratch, scratch_fill=fill)
    if form == "window":
        buf, dpad = window_buffer(S)
        plan = spl.plan_one(planner, d, dC=dC, n=n, padded=1, switches=bits)
        res = Estimator.debug_solve_dense(buf, ref["g"], d, dC=dC, sb_chain=n, padded=True, ldS=dpad, **kw)
    else:   # the pose graph's: the trailing principal block of a larger matrix, NaN around it
        N = d + 37
        buf = np.full((N, N), np.nan)
        buf[37:, 37:] = S
        plan = spl.plan_one(planner, d, padded=0, switches=bits)
        res = Estimator.debug_solve_dense(buf, ref["g"], d, padded=False, ldS=N, offset=37 * N + 37, **kw)
    return res, plan, buf


def assert_plan_taken(res, plan, what):
    got = tuple(res[k] for k in ("chainMode", "route", "dSolve", "border", "bigChainGrid", "helperTasks", "nBackPanels", "chainOverflow", "end"))
    want = tuple(plan[k] for k in ("chainMode", "route", "dSolve", "border", "bigChain_grid", "helperTasks", "nBackPanels", "chainOverflow", "end"))
    assert got == want, "%s: the library planned %s, the planner %s" % (what, got, want)


def route_name(plan):
    chain = {0: "", 1: "chain (blocked matrix) + ", 2: "chain (compact) + "}[plan["chainMode"]]
    return chain + spl.ROUTES[plan["route"]]


def check_solution(res, plan, ref, what):
    """the plan, cholFail and the two bars; prints the case's line"""
    assert_plan_taken(res, plan, what)
    assert res["cholFail"] == 0, what
    factor = dr.tile_factor(ref, plan["chainMode"] != 0, plan["border"])
    dev, lap = dr.judge(ref, res["y"], factor), dr.judge(ref, ref["y_lapack"], factor)
    print("%s; family %s %s; d %d; device %.3g / %.4g; LAPACK %.3g / %.4g; forward %.3g (bar %.3g)" %
          (route_name(plan), ref["family"], "fused mu %g" % ref["mu"] if ref["fused"] else "unfused", ref["d"], dev["backward_eps"], dev["bar_eps"],
           lap["backward_eps"], lap["bar_eps"], dev["forward_err"], dev["forward_err"] / max(dev["forward"], 1e-300)))
    assert np.all(np.isfinite(res["y"])), what
    assert dev["backward"] <= 1.0, "%s: backward residual %.3g eps over the bar of %.4g eps" % (what, dev["backward_eps"], dev["bar_eps"])
    # family B: the tile factor is an allowance the device does not need -- the plain bar gamma, which LAPACK is shown to meet on
    # these systems too, is asserted as well (the line above then follows from it, and stays as the bar the reference states)
    assert dev["backward_eps"] * dr.EPS <= dr.gamma(ref["d"]), "%s: backward residual %.3g eps over the plain bar" % (what, dev["backward_eps"])
    assert dev["forward"] <= 1.0, "%s: forward error %.3g is %.3g of its bar" % (what, dev["forward_err"], dev["forward"])
    if ref["fused"]:   # the metric the solver leaves for the post-solve pass: three roundings on top of the reference's
        assert np.abs(res["htil"] / np.asarray(ref["htil"], dtype=np.float64) - 1.0).max() <= 8 * dr.EPS, what


def check_stages(res, plan, ref, what):
    """what the launches of the plan leave in the solver's scratch (family A, d <= 600)"""
    d, dC, n, scr = ref["d"], ref["dC"], ref["n"], res["scratch"]
    S_fin = ref["S_fin"]
    s = dr.scale_of(S_fin)
    if plan["chainMode"] == 0 and plan["route"] in (spl.LEFT_LOOKING, spl.BLOCKED):
        if plan["route"] == spl.LEFT_LOOKING:
            assert plan["factor_off"] == 0
            L, dinv = dr.assemble_ll_factor(scr, d)
        else:
            L, dinv = dr.assemble_blocked_factor(scr, plan, d)
        ratio = dr.factor_ratio(S_fin, L)
        print("    factor: |S - L L^T| at %.3g of Demmel's bound" % ratio)
        assert ratio <= 1.0, what
        assert np.abs(dinv * np.asarray(np.diag(L), dtype=np.float64) - 1.0).max() <= 4 * dr.EPS, what
    if plan["chainMode"] != 0:
        q = dr.chain_quantities(S_fin, ref["g"], dC, n)
        rowsY, ldY = plan["rowsY"], plan["ldY"]
        Y = np.asarray(scr[plan["Y_off"]:][:rowsY * ldY], dtype=LD).reshape(rowsY, ldY)
        assert np.all(Y[9 * n:, :dC + 1] == 0), what
        gram = Y[:, :dC + 1].T @ Y[:, :dC + 1]
        t = (s[dC:, None] * np.abs(q["Z"])).sum(axis=0)   # sum_a s_a |S_ss^-1 [S_sk | g_s]|_a: the backward bar of the chain's own solve, column by column
        ratio = float((np.abs(gram - q["gram"]) / np.outer(t, t)).max()) / dr.gamma(9 * n)
        print("    chain: Y^T Y at %.3g of its bar" % ratio)
        assert ratio <= 1.0, what
    if plan["chainMode"] == 2:
        ld = plan["ldOut"]
        M = np.asarray(scr[plan["compactS_off"]:][:ld * ld]).reshape(ld, ld)
        gk = np.asarray(scr[plan["compactG_off"]:][:ld])
        low = np.tril(np.ones((dC, dC), bool))
        rS = float((np.abs(np.asarray(M[:dC, :dC], dtype=LD) - q["Sprime"]) / np.outer(s[:dC], s[:dC]))[low].max()) / dr.gamma(d)
        rg = float((np.abs(np.asarray(gk[:dC], dtype=LD) - q["gprime"]) / (s[:dC] * (s * np.abs(ref["x"])).sum())).max()) / dr.gamma(d)
        print("    compact kept system: S' at %.3g, g' at %.3g of their bars" % (rS, rg))
        assert rS <= 1.0 and rg <= 1.0, what
        # zero beyond dK, in the tiles the solver loads (the lower ones)
        tiles_low = np.kron(np.tril(np.ones((ld // 16, ld // 16), bool)), np.ones((16, 16), bool))
        beyond = np.zeros((ld, ld), bool)
        beyond[dC:, :] = True
        beyond[:, dC:] = True
        off_diag_tiles = tiles_low & ~np.kron(np.eye(ld // 16, dtype=bool), np.ones((16, 16), bool))
        assert np.all(M[beyond & off_diag_tiles] == 0), what
        # (g' beyond dK is left as it was: k_sb_load writes dK entries and no kept solver reads more -- every load of the right-hand
        #  side is guarded by the row count, `t < d ? p.gRed[t] : 0.0` in k_chol_solve_lds and k_chol_solve_ll, `valid` / `t < m` in
        #  k_chol_border_prepare, `a < border` in the border prologue; with the NaN fill a read of it would show in y)


def run_family(planner, debug_option, family, dC, n, switches=(), stages=True):
    """unfused with mu = 0 and fused with the family's mu, init_scale = 1 -> {fused: y}"""
    out = {}
    border = spl.plan_one(planner, dC + 9 * n, dC=dC, n=n)["border"]
    for fused in (False, True):
        ref = dr.reference(family, dC, n, fused, border=border)
        with_scratch = stages and family == "A" and ref["d"] <= dr.STAGE_MAX_D
        res, plan, _ = solve(planner, ref, switches, debug_option, scratch=with_scratch, fill=NAN_FILL)
        what = "%s d %d (dC %d, chain %d) %s %s" % (family, ref["d"], dC, n, "fused" if fused else "unfused", "+".join(switches))
        check_solution(res, plan, ref, what)
        if with_scratch:
            check_stages(res, plan, ref, what)
        out[fused] = res["y"]
    return out


# ------------------------------------------------------------------------------------------------ window form, no chain
@pytest.mark.parametrize("route,d,family", [(route, d, fam) for route, rows in dr.NO_CHAIN.items() for d, b in rows for fam in ("A", "B")[:1 + b]])
def test_window_form_without_a_chain(gpu_lib, planner, debug_option, route, d, family):
    assert spl.ROUTES[spl.plan_one(planner, d)["route"]] == route
    run_family(planner, debug_option, family, d, 0)


@pytest.mark.parametrize("d,switch,route", dr.SWITCHED)
def test_window_form_with_a_route_switch(gpu_lib, planner, debug_option, d, switch, route):
    assert spl.ROUTES[spl.plan_one(planner, d, switches=SWITCH_BITS[switch])["route"]] == route
    run_family(planner, debug_option, "A", d, 0, switches=(switch,))


def test_blocked_route_on_the_wide_grid(gpu_lib, planner, debug_option):
    """d = 1921: 31 block rows, 523 helper tasks > kPersistWideTasks, so k_big_chol_chain takes a grid of 256 instead of 120"""
    ref = dr.reference("A", dr.WIDE_GRID_D, 0, False)
    res, plan, _ = solve(planner, ref, fill=NAN_FILL)
    assert (plan["nb"], plan["helperTasks"], plan["bigChain_grid"]) == (31, 523, 256)
    assert res["bigChainGrid"] == 256 and res["helperTasks"] == 523
    check_solution(res, plan, ref, "d 1921")


# ------------------------------------------------------------------------------------------------ pose-graph form
@pytest.mark.parametrize("d,route", dr.POSE_GRAPH)
def test_pose_graph_form(gpu_lib, planner, debug_option, d, route):
    """sPadded = 0: S is the trailing principal block of a (d + 37)^2 matrix that holds NaN everywhere else"""
    ref = dr.reference("A", d, 0, False)
    res, plan, buf = solve(planner, ref, form="pose_graph", fill=NAN_FILL)
    assert spl.ROUTES[plan["route"]] == route and plan["border"] == 0
    check_solution(res, plan, ref, "pose-graph form d %d" % d)
    assert np.array_equal(res["S_after"].reshape(buf.shape), buf, equal_nan=True), "the solve wrote to the caller's matrix"


# ------------------------------------------------------------------------------------------------ fused finalisation edges
@pytest.mark.parametrize("edit", dr.EDGE_EDITS, ids=["clamped_rows", "supplied_scale"])
def test_fused_finalisation_edges(gpu_lib, planner, debug_option, edit):
    ref = dr.reference("A", dr.EDGE_D, 0, True, edit=edit)
    if edit[0] == "clamped":   # hC = 0: scale 1 and htil the clamp itself; hC = 1e-9: the clamp over the scale squared
        assert float(ref["htil"][3]) == 1e-6 and float(ref["htil"][100]) == pytest.approx(1e-6 * (1.0 + np.sqrt(1e-9)) ** 2, rel=1e-15)
    else:
        assert not ref["init_scale"] and float(ref["htil"][3]) == pytest.approx(1e-6 / ref["scaleC"][3] ** 2, rel=1e-15)
    res, plan, _ = solve(planner, ref, fill=NAN_FILL)
    check_solution(res, plan, ref, "d 176 fused, " + edit[0])


# ------------------------------------------------------------------------------------------------ with a chain
@pytest.mark.parametrize("mode,route,dC,n,family", [(m, r, dC, n, fam) for m, r, dC, n, b in dr.CHAIN for fam in ("A", "B")[:1 + b]])
def test_window_form_with_a_chain(gpu_lib, planner, debug_option, mode, route, dC, n, family):
    """each shape with the chain eliminated and again with SVIN_NO_SB_ELIM: both meet the bars, and their y differ in bits (the
    switch really selects code)"""
    plan = spl.plan_one(planner, dC + 9 * n, dC=dC, n=n)
    assert (plan["chainMode"], spl.ROUTES[plan["route"]]) == (mode, route)
    y_on = run_family(planner, debug_option, family, dC, n)
    y_off = run_family(planner, debug_option, family, dC, n, switches=("SVIN_NO_SB_ELIM",))
    for fused in (False, True):
        assert np.any(y_on[fused] != y_off[fused])


@pytest.mark.parametrize("route,dC,n", dr.DECLINED)
def test_chain_the_planner_declines(gpu_lib, planner, debug_option, route, dC, n):
    plan = spl.plan_one(planner, dC + 9 * n, dC=dC, n=n)
    assert (plan["chainMode"], spl.ROUTES[plan["route"]], plan["dSolve"]) == (0, route, dC + 9 * n)
    run_family(planner, debug_option, "A", dC, n)


# ------------------------------------------------------------------------------------------------ not positive definite
# (what, dC, n, row whose pivot turns negative, the bit of cholFail its reporter raises)
TILE_PIVOT, BLOCK_PIVOT = 2, 1   # cholDiag16Acc (tile16.hpp) | the border block's factorisation and cholPacked9 of a chain block (kernels.hip)
NOT_PD = [
    ("lds_whole, last tile row", 176, 0, 170, TILE_PIVOT),
    ("lds_border_load, last tile row of the main block", 180, 0, 170, TILE_PIVOT),
    ("lds_border_prepared, last tile row of the main block", 200, 0, 170, TILE_PIVOT),
    ("left_looking, last tile row", 272, 0, 268, TILE_PIVOT),
    ("blocked, last tile row", 513, 0, 512, TILE_PIVOT),
    ("chain (compact), last tile row of the kept rows", 84, 14, 82, TILE_PIVOT),
    ("chain (blocked matrix), last tile row of the kept rows", 273, 8, 272, TILE_PIVOT),
    ("border row at d = 190", 190, 0, 183, BLOCK_PIVOT),
    ("chain block 3 of (84, 14)", 84, 14, 84 + 9 * 3 + 4, BLOCK_PIVOT),
]


@pytest.mark.parametrize("what,dC,n,row,bit", NOT_PD, ids=[c[0].replace(" ", "_") for c in NOT_PD])
def test_not_positive_definite_is_reported(gpu_lib, planner, debug_option, what, dC, n, row, bit):
    """family A with one diagonal entry lowered so that exactly one pivot turns negative: a numerical event the solvers report in
    cholFail, not a fault -- the call returns, no bounded wait gives up; nothing is asked of y.
    The report is SolverScalars::cholFail's pair of bits 1 | 2 ("S or a landmark block is not positive definite", kernels.hpp; the
    host acts on failMax != 0 and tells only 4 | 8 apart), and each case asks for the bit of the reporter its pivot belongs to:
    bit 1 from the border block's factorisation (k_chol_solve_lds<1>'s prologue, k_chol_border_prepare) and from a chain block's
    (cholPacked9 in k_sb_factor) -- the two cases that exist for them: the tiles behind such a block fail as well and raise 2
    (measured: 3), so a mask of 3 would not notice if the block's own check fell silent; bit 2 from a pivot of a 16 x 16 tile
    (cholDiag16Acc, tile16.hpp, which cov.hip shares; measured: 2 on the five dense routes and on the kept rows behind either
    chain mode), the one bit the tile kernels raise."""
    ref = dr.reference("A", dC, n, False)
    S = dr.make_indefinite(ref["S"], row)
    res, plan, _ = solve(planner, ref, S=S, fill=NAN_FILL)
    assert_plan_taken(res, plan, what)
    print("%s: %s, cholFail %d" % (what, route_name(plan), res["cholFail"]))
    assert res["cholFail"] & bit, what
    assert (res["cholFail"] & 12) == 0, what
    assert (res["cholFail"] & ~15) == 0, what
