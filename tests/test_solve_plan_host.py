"""The host planning of the reduced solve (svin_amd/csrc/solve_plan.hpp) on the CPU.

launchSolveReduced walks the plan without checking it: a wrong route launches a kernel on a system it was not written for, a wrong
offset lets two launches of one sequence share doubles of DeviceProblem::cholL, a wrong LDS size is a refused launch.  The routes are
held to tests/golden/solve_plan.npz, which was recorded from the functions that decided them before the planner existed
(tests/golden/make_golden_solve_plan.py); the layout and the launch sizes are checked as properties over the same sweep."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import solve_plan_lib as spl          # noqa: E402

ROOT = spl.ROOT
LDS_BYTES = 163840   # of a gfx950 workgroup


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return spl.build_shim(tmp_path_factory.mktemp("sp"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "solve_plan.npz"))


@pytest.fixture(scope="module")
def swept(lib, golden):
    """the sweep and the fixture's extra rows, planned once, shared: (inputs, {field: array})"""
    rows = np.concatenate([spl.sweep(), golden["extra_in"]])
    return rows, spl.plan(lib, rows)


def recorded_view(q):
    """a plan's fields as the fixture records them: dp of the blocked route only, offsets of the regions in use, -1 otherwise"""
    chain, compact = q["chainMode"] != 0, q["chainMode"] == 2
    cols = [q["chainMode"], q["route"], q["border"], q["dp"]]
    cols += [np.where(chain, q[r + "_off"], -1) for r in ("Lf", "Y", "tvec")]
    cols += [np.where(compact, q[r + "_off"], -1) for r in ("compactS", "compactG")]
    return np.stack(cols, axis=1)


# ------------------------------------------------------------------------------------------------ 1. the routes are the recorded ones
def test_routes_and_chain_offsets_are_the_recorded_ones(swept, golden):
    rows, q = swept
    ref = np.concatenate([golden["sweep_out"].T, golden["extra_out"]]).astype(np.int64)
    got = recorded_view(q)
    assert got.shape == ref.shape
    bad = np.nonzero(np.any(got != ref, axis=1))[0]
    assert len(bad) == 0, "first of %d: input %s planned %s recorded %s" % (len(bad), rows[bad[0]].tolist(), got[bad[0]].tolist(), ref[bad[0]].tolist())


def test_fixture_holds_the_spot_values(golden):
    """read off the functions the fixture was recorded from; d alone decides without a chain, so these are among the extra rows"""
    extra = {tuple(i): tuple(o) for i, o in zip(golden["extra_in"].tolist(), golden["extra_out"].tolist())}
    route = lambda d: extra[(d, d, 0, 1, 0)][:3]
    assert route(150) == (0, spl.LDS_WHOLE, 0) and route(176) == (0, spl.LDS_WHOLE, 0)
    assert route(177) == (0, spl.LDS_BORDER_LOAD, 1) and route(200) == (0, spl.LDS_BORDER_PREPARED, 24)
    assert route(201) == (0, spl.LEFT_LOOKING, 0) and route(272) == (0, spl.LEFT_LOOKING, 0)
    assert route(273) == (0, spl.BLOCKED, 0)
    sw = spl.sweep()
    k = int(np.nonzero(np.all(sw == [270, 180, 10, 1, 0], axis=1))[0][0])   # config #3: compact, border rows in the load
    assert golden["sweep_out"][:, k].tolist()[:5] == [2, spl.LDS_BORDER_LOAD, 4, 0, 73920]
    assert len(sw) == 140000 and golden["sweep_out"].shape == (len(spl.RECORDED), len(sw))
    assert np.any(golden["extra_in"][:, 0] != golden["extra_in"][:, 1] + 9 * golden["extra_in"][:, 2])


# ------------------------------------------------------------------------------------------------ 2. the layout is sound
def test_regions_in_use_are_disjoint_aligned_and_inside_the_buffer(lib, swept):
    rows, q = swept
    off = np.stack([q[r + "_off"] for r in spl.REGIONS], axis=1)
    length = np.stack([q[r + "_len"] for r in spl.REGIONS], axis=1)
    used = length > 0
    assert np.all(off[used] % 2 == 0), "16-byte aligned starts"
    assert np.all(off >= 0) and np.all(length >= 0)
    # every region a sequence uses is live until its last launch (the chain's records are read by k_sb_back, S' by the kept
    # solver that writes the factor / the border scratch), so all of a plan's regions must be pairwise disjoint
    for a in range(len(spl.REGIONS)):
        for b in range(a + 1, len(spl.REGIONS)):
            both = used[:, a] & used[:, b]
            apart = (off[:, a] + length[:, a] <= off[:, b]) | (off[:, b] + length[:, b] <= off[:, a])
            assert np.all(apart[both]), (spl.REGIONS[a], spl.REGIONS[b], rows[np.nonzero(both & ~apart)[0][0]].tolist())
    assert np.all(q["end"] == np.max(np.where(used, off + length, 0), axis=1)), "the plan's end is its last region's"
    d = rows[:, 0]
    size = {w: np.array([spl.scratch_doubles(lib, x, w) for x in range(int(d.max()) + 1)], np.int64) for w in (False, True)}
    assert np.all(q["end"] <= size[True][d]), "a window's buffer"
    chainless = q["chainMode"] == 0
    assert np.all(q["end"][chainless] <= size[False][d[chainless]]), "a buffer without room for the chain (the pose graph's root solve)"
    # the chain's regions fit wherever the chain is eliminated at all: the fall-back to chain mode 0 never fires
    assert not np.any(q["chainOverflow"])
    fill = q["end"] / size[True][d]
    assert 0.3 < fill[q["chainMode"] != 0].max() < 0.32   # (the fullest chain plan: 0.316 of the buffer)


def test_which_regions_a_route_uses(swept):
    _, q = swept
    used = {r: q[r + "_len"] > 0 for r in spl.REGIONS}
    route, mode = q["route"], q["chainMode"]
    assert np.array_equal(used["factor"], route == spl.LEFT_LOOKING)
    assert np.array_equal(used["borderScr"], route == spl.LDS_BORDER_PREPARED)
    for r in ("bigM", "dinvG", "diagF", "ready"):
        assert np.array_equal(used[r], (route == spl.BLOCKED) & (q["dSolve"] > 0)), r
    for r in ("compactS", "compactG"):
        assert np.array_equal(used[r], mode == 2), r
    for r in ("Lf", "Y", "tvec", "counter"):
        assert np.array_equal(used[r], mode != 0), r
    # the kernels' own extents: the left-looking solver writes nT (nT + 1) / 2 tiles of 256, k_sb_load dpadK x dpadK and dK,
    # the chain n records, rowsY x ldY and 9 n entries, the blocked solver (dp + 64) x dp, dp, dp x 64 and (nb + 3) nb ints
    nT = q["dpad"] // 16
    ll = route == spl.LEFT_LOOKING
    assert np.all(q["factor_len"][ll] >= (nT * (nT + 1) // 2 * 256)[ll])
    big = route == spl.BLOCKED
    dp, nb = q["dp"], q["nb"]
    assert np.all((dp == (q["dSolve"] + 63) // 64 * 64)[big]) and np.all((nb == dp // 64)[big]) and np.all(dp[~big] == 0)
    assert np.all((q["bigM_len"] == (dp + 64) * dp)[big]) and np.all((q["dinvG_len"] == dp)[big]) and np.all((q["diagF_len"] == 64 * dp)[big])
    assert np.all((2 * q["ready_len"] >= (nb + 3) * nb)[big])
    ch = mode != 0
    assert np.all((q["Lf_len"] == 264 * q["n"])[ch]) and np.all((q["Y_len"] == q["rowsY"] * q["ldY"])[ch]) and np.all((q["tvec_len"] >= 9 * q["n"])[ch])
    assert np.all((q["ldY"] >= q["dK"] + 1)[ch]) and np.all((q["ldY"] % 16 == 0)[ch]) and np.all((q["rowsY"] % 4 == 0)[ch]) and np.all((q["rowsY"] >= 9 * q["n"])[ch])
    cp = mode == 2
    assert np.all((q["ldOut"] == (q["dK"] + 15) // 16 * 16)[cp]) and np.all((q["compactS_len"] == q["ldOut"] ** 2)[cp]) and np.all((q["compactG_len"] >= q["dK"])[cp])


# ------------------------------------------------------------------------------------------------ 3. every launch fits the machine
def test_every_planned_launch_fits_the_machine(swept):
    _, q = swept
    route, mode = q["route"], q["chainMode"]
    lds_route = route <= spl.LDS_BORDER_PREPARED
    planned = {"sbFactor": mode != 0, "sbForward": mode != 0, "sbLoad": mode != 0, "sbBack": mode != 0,
               "borderPrepare": route == spl.LDS_BORDER_PREPARED, "cholLds": lds_route, "cholLL": route == spl.LEFT_LOOKING,
               "bigLoad": (route == spl.BLOCKED) & (mode == 0), "bigChain": route == spl.BLOCKED}
    assert set(planned) == set(spl.LAUNCHES)
    for name, want in planned.items():
        grid, lds = q[name + "_grid"], q[name + "_lds"]
        assert np.all(grid[want] >= 1) and np.all(grid[~want] == 0), name
        assert np.all(lds >= 0) and np.all(lds <= LDS_BYTES), (name, int(lds.max()))
    big = route == spl.BLOCKED
    assert np.all(q["bigBackLds"] <= LDS_BYTES) and np.all(q["bigBackLds"][big] > 0)
    assert np.all(q["nBackPanels"][big & (q["dp"] > 0)] >= 1) and np.all(q["nBackPanels"][~big] == 0)
    assert np.all(q["nBackPanels"] - 1 <= 63), "k_big_back's nChunks: the spare rows of the right-hand-side block"
    # one-workgroup kernels are launched as one workgroup; k_big_chol_chain's workgroups must be co-resident
    for name in ("sbFactor", "borderPrepare", "cholLds", "cholLL"):
        assert np.all(q[name + "_grid"] <= 1), name
    assert np.all(q["bigChain_grid"] <= 256) and np.all(q["bigChain_grid"][big] >= 2)


def test_launch_sizes_are_the_expressions_the_launchers_held(swept):
    """grid and dynamic LDS of every launch against the expressions as launchSolveDense, launchSbChainFactor and
    launchSolveReduced wrote them out before the planner existed (restated here once, on purpose)"""
    _, q = swept
    route, mode, n, dK = q["route"], q["chainMode"], q["n"], q["dK"]
    nT = np.where(q["border"] > 0, 11, (q["dSolve"] + 15) // 16)
    lds = route <= spl.LDS_BORDER_PREPARED
    chol = (nT * (nT + 1) // 2 * 16 * 17 + 3 * 16 * nT) * 8 + 48 * 4 + 32 * 8
    assert np.all((q["cholLds_lds"] == chol)[lds]) and np.all((q["dpad"] == 16 * nT)[lds])
    ll = route == spl.LEFT_LOOKING
    half = (nT + 1) // 2
    assert np.all((q["cholLL_lds"] == ((nT - half) * half * 256 + 2 * 256 + 16 * 17 + 16 + 2 * 16 * nT) * 8)[ll]) and np.all((q["dpad"] == 16 * nT)[ll])
    big = route == spl.BLOCKED
    nb = q["nb"]
    helpers = np.zeros_like(nb)
    for k in np.unique(nb[big]):
        helpers[nb == k] = sum(max(k - st - 1, 0) + (2 if st + 2 <= k - 1 else 0) for st in range(k))
    assert np.all((q["helperTasks"] == helpers)[big])
    grid = 1 + np.maximum(1, np.minimum(helpers, np.where(helpers > 512, 256, 120) - 1))
    assert np.all((q["bigChain_grid"] == grid)[big]) and np.all((q["bigChain_lds"] == (3 * 16 * 16 * 17 + 64 + 2) * 8)[big])
    assert np.all((q["bigLoad_grid"] == 256)[big & (mode == 0)]) and np.all((q["bigBackLds"] == (512 + 8 * 64 + 64 * 65 + 64) * 8)[big])
    ch = mode != 0
    nTk = (dK + 15) // 16
    assert np.all((q["sbFactor_lds"] == (n * 162 + (n + 1) // 2 * 243) * 8)[ch]) and np.all((q["sbFactor_grid"] == 1)[ch])
    assert np.all((q["sbForward_lds"] == (q["rowsY"] * 8 + n * 243) * 8)[ch]) and np.all((q["sbForward_grid"] == q["ldY"] // 8)[ch])
    assert np.all((q["sbLoad_grid"] == nTk * (nTk + 1) // 2 + nTk)[ch]) and np.all(q["sbLoad_lds"] == 0)
    assert np.all((q["sbBack_lds"] == (n * 264 + 18 * n) * 8)[ch]) and np.all((q["sbBack_grid"] == (9 * n + 15) // 16)[ch])
    assert np.all((q["dpK"] == (dK + 63) // 64 * 64)[ch]) and np.all((q["dpK"] == q["dp"])[mode == 1])   # (SbElimArgs::dp)
    assert np.all((q["ldY"] == (dK + 1 + 15) // 16 * 16)[ch]) and np.all((q["rowsY"] == (9 * n + 3) // 4 * 4)[ch])
    # the regions the launchers derived themselves: the blocked solver's vectors and flags behind its matrix
    dp = q["dp"]
    assert np.all((q["dinvG_off"] == (dp + 64) * dp)[big]) and np.all((q["diagF_off"] == (dp + 64) * dp + dp)[big])
    assert np.all((q["ready_off"] == (dp + 64) * dp + dp + 64 * dp)[big]) and np.all((q["borderScr_off"] == 0) & (q["factor_off"] == 0) & (q["bigM_off"] == 0))


@pytest.mark.parametrize("dp", [320, 512, 576, 1024, 3072])
def test_back_panels_tile_the_columns_from_the_right(lib, dp):
    c = spl.constants(lib)
    span, panels, c1 = c["kBackSpan"], [], dp
    while c1 > 0:   # the loop of the backward substitution as it was written in the launcher
        c0 = max(0, c1 - span)
        panels.append(dict(c0=c0, c1=c1, blocks=(c1 - c0) // c["kNB"], nChunks=(dp - c1 + span - 1) // span))
        c1 -= span
    q = spl.plan_one(lib, dp)
    assert q["route"] == spl.BLOCKED and q["dp"] == dp and q["nBackPanels"] == len(panels)
    assert [spl.back_panel(lib, dp, k) for k in range(len(panels))] == panels


# ------------------------------------------------------------------------------------------------ 4. boundaries
W, BL, BP, LL, BIG = spl.LDS_WHOLE, spl.LDS_BORDER_LOAD, spl.LDS_BORDER_PREPARED, spl.LEFT_LOOKING, spl.BLOCKED
# name: (d, dC, chain, sPadded, switches) -> (chain mode, route, border rows)
BOUNDARIES = {
    "d176_lds_whole": ((176, 176, 0, 1, 0), (0, W, 0)),
    "d177_one_border_row": ((177, 177, 0, 1, 0), (0, BL, 1)),
    "d180_four_border_rows_in_the_load": ((180, 180, 0, 1, 0), (0, BL, 4)),
    "d181_five_border_rows_prepared": ((181, 181, 0, 1, 0), (0, BP, 5)),
    "d200_24_border_rows": ((200, 200, 0, 1, 0), (0, BP, 24)),
    "d201_left_looking": ((201, 201, 0, 1, 0), (0, LL, 0)),
    "d272_left_looking": ((272, 272, 0, 1, 0), (0, LL, 0)),
    "d273_blocked": ((273, 273, 0, 1, 0), (0, BIG, 0)),
    "d180_unpadded_has_no_border": ((180, 180, 0, 0, 0), (0, LL, 0)),
    "d176_unpadded_lds_whole": ((176, 176, 0, 0, 0), (0, W, 0)),
    "chain1_stays": ((249, 240, 1, 1, 0), (0, LL, 0)),
    "chain2_stays": ((258, 240, 2, 1, 0), (0, LL, 0)),
    "chain7_stays": ((303, 240, 7, 1, 0), (0, BIG, 0)),
    "chain8_eliminated": ((312, 240, 8, 1, 0), (2, LL, 0)),
    "chain64_eliminated": ((816, 240, 64, 1, 0), (2, LL, 0)),
    "chain65_stays": ((825, 240, 65, 1, 0), (0, BIG, 0)),
    "dC12_chain_stays": ((282, 12, 30, 1, 0), (0, BIG, 0)),
    "dC18_chain_eliminated": ((288, 18, 30, 1, 0), (2, W, 0)),
    "chain_behind_an_lds_system_stays": ((177, 60, 13, 1, 0), (0, BL, 1)),
    "chain_with_rows_behind_it_stays": ((271, 180, 10, 1, 0), (0, LL, 0)),
    "kept176_lds_whole": ((266, 176, 10, 1, 0), (2, W, 0)),
    "kept180_border_in_the_load": ((270, 180, 10, 1, 0), (2, BL, 4)),
    "kept182_border_prepared": ((272, 182, 10, 1, 0), (2, BP, 6)),
    "kept200_border_prepared": ((290, 200, 10, 1, 0), (2, BP, 24)),
    "kept206_left_looking": ((296, 206, 10, 1, 0), (2, LL, 0)),
    "kept272_left_looking": ((362, 272, 10, 1, 0), (2, LL, 0)),
    "kept278_blocked": ((368, 278, 10, 1, 0), (1, BIG, 0)),
    "kept180_of_an_unpadded_system_still_has_its_border": ((270, 180, 10, 0, 0), (2, BL, 4)),   # (S' is padded whatever S is)
    "no_ll_d250_blocked": ((250, 250, 0, 1, spl.NO_LL), (0, BIG, 0)),
    "no_ll_kept180_goes_to_the_blocked_matrix": ((270, 180, 10, 1, spl.NO_LL), (1, BIG, 0)),   # (the mode is chosen without the border rows)
    "no_sb_elim_keeps_the_chain": ((270, 180, 10, 1, spl.NO_SB_ELIM), (0, LL, 0)),
    "no_lds_border_d180_left_looking": ((180, 180, 0, 1, spl.NO_LDS_BORDER), (0, LL, 0)),
    "no_lds_border_kept180_left_looking": ((270, 180, 10, 1, spl.NO_LDS_BORDER), (2, LL, 0)),
}


@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_boundary(lib, name):
    row, want = BOUNDARIES[name]
    q = spl.plan(lib, [row])
    assert (int(q["chainMode"][0]), int(q["route"][0]), int(q["border"][0])) == want
    assert int(q["dSolve"][0]) == (row[1] if want[0] else row[0])


def test_kernel_arguments_of_the_routes(lib):
    """dpad as the one-workgroup kernels are launched with it, and config #3's chain layout"""
    assert spl.plan_one(lib, 150)["dpad"] == 160 and spl.plan_one(lib, 176)["dpad"] == 176
    assert spl.plan_one(lib, 180)["dpad"] == 176 and spl.plan_one(lib, 198)["dpad"] == 176   # border rows: the eleven tile rows
    assert spl.plan_one(lib, 201)["dpad"] == 208 and spl.plan_one(lib, 273)["dp"] == 320
    q = spl.plan_one(lib, 270, n=10)
    assert (q["dK"], q["n"], q["ldY"], q["rowsY"], q["ldOut"]) == (180, 10, 192, 92, 192)
    assert (q["compactS_off"], q["compactG_off"], q["Lf_off"], q["Y_off"]) == (192 * 192, 2 * 192 * 192, 73920, 73920 + 2640)
    assert (q["sbForward_grid"], q["sbLoad_grid"], q["sbBack_grid"]) == (24, 12 * 13 // 2 + 12, 6)
    q = spl.plan_one(lib, 960, n=64)   # config #4: the kept rows in the blocked matrix, the chain behind everything it keeps
    assert (q["chainMode"], q["dp"], q["nb"], q["bigLoad_grid"]) == (1, 384, 6, 0)
    assert q["Lf_off"] >= q["ready_off"] + q["ready_len"] and q["Lf_off"] % 2 == 0


def test_buffer_size_is_unchanged(lib):
    """solveReducedScratchDoubles against its expression as it stood in kernels.hpp"""
    def size(d, chain):
        dpad, d64 = (d + 15) // 16 * 16, (d + 63) // 64 * 64
        nb = d64 // 64
        big = (d64 + 64) * d64 + d64 + d64 * 64 + ((nb + 3) * nb + 1) // 2 + 2
        return max(dpad * dpad, big) + ((2 * dpad * dpad + (dpad + 8) * (dpad + 32) + 64 * 264 + 64) if chain else 0)
    for d in list(range(0, 400)) + [960, 2394, 3015, 6000]:
        for chain in (False, True):
            assert spl.scratch_doubles(lib, d, chain) == size(d, chain), (d, chain)


def test_batched_solver_takes_only_whole_unchained_lds_systems(lib, swept):
    """batchSupported's condition on the solver, against the expression it held before the planner: the WHOLE system (d, not the
    rows a chain elimination keeps) fits the LDS-resident solver -- its LDS bytes within 156 KB -- and has no border rows"""
    rows, q = swept
    d, padded, no_border = rows[:, 0], rows[:, 3] != 0, (rows[:, 4] & spl.NO_LDS_BORDER) != 0
    nT = (d + 15) // 16
    fits = (nT * (nT + 1) // 2 * 16 * 17 + 3 * 16 * nT) * 8 + 48 * 4 + 32 * 8 <= 156 * 1024
    border = np.where(padded & (d - 176 >= 1) & (d - 176 <= 24) & ~no_border, d - 176, 0)
    solver_class_0 = fits | (border > 0)
    assert np.array_equal(q["batched"] != 0, solver_class_0 & (border == 0))
    assert np.array_equal(q["batched"] != 0, d <= 176)
    # the kept rows of a chain elimination on the LDS-resident solver are NOT such a system: the batched kernel has no chain form
    kept_whole = (q["chainMode"] == 2) & (q["route"] == spl.LDS_WHOLE)
    assert kept_whole.sum() > 1000 and not np.any(q["batched"][kept_whole])
    for d1, dC, n in ((225, 90, 15), (210, 84, 14), (266, 176, 10), (435, 174, 29)):
        p = spl.plan_one(lib, d1, dC=dC, n=n)
        assert (p["chainMode"], p["route"], p["batched"]) == (2, spl.LDS_WHOLE, 0), (d1, dC, n)
    assert spl.plan_one(lib, 150, n=10)["batched"] == 1 and spl.plan_one(lib, 176)["batched"] == 1
    assert spl.plan_one(lib, 177)["batched"] == 0 and spl.plan_one(lib, 180, padded=0)["batched"] == 0


# ------------------------------------------------------------------------------------------------ 5. under a sanitizer
def test_planner_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program (its own main, the whole sweep), run as a child"""
    exe = str(tmp_path / "solve_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "solve_plan_sanitize.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout[-4000:]
