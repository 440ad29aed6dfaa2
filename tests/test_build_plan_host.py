"""The host planning of the build, the evaluation and the step (svin_amd/csrc/build_plan.hpp) on the CPU.

The launchers walk these plans without checking them: a wrong variant runs a kernel on a geometry it was not written for, a wrong
LDS size is a refused launch, and a slab count that disagrees with the build's grid lets k_reduce_slabs sum slabs nobody wrote.
The decisions are held to tests/golden/build_plan.npz, which was recorded from the code that took them before the planner existed
(tests/golden/make_golden_build_plan.py); launch sizes that existed there only as arguments of a launch are held against their
expressions, restated here once; the rest are properties over the same sweep."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import build_plan_lib as bpl          # noqa: E402

ROOT = bpl.ROOT
LDS_BYTES = 163840   # of a gfx950 workgroup


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return bpl.build_shim(tmp_path_factory.mktemp("bp"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "build_plan.npz"))


@pytest.fixture(scope="module")
def sizes(golden):
    """sizeof(CameraModel), sizeof(FactorShared) of the kernels the fixture was recorded from, and its small compute-unit count"""
    cm, fs, small = (int(x) for x in golden["sizes"])
    assert small == bpl.SMALL_CUS
    return cm, fs


@pytest.fixture(scope="module")
def swept(lib, sizes):
    """the sweep and the extra rows, planned once, shared: ({input: array}, {field: array})"""
    rows = np.concatenate([bpl.sweep(), bpl.extra_rows()])
    return {name: rows[:, k].astype(np.int64) for k, name in enumerate(bpl.INPUTS)}, bpl.plan(lib, rows, *sizes)


def plan_one(lib, sizes, *a, **k):
    return {name: int(v[0]) for name, v in bpl.plan(lib, [bpl.row(*a, **k)], *sizes).items()}


# ------------------------------------------------------------------------------------------------ 1. the decisions are the recorded ones
def test_decisions_are_the_recorded_ones(swept, golden):
    r, q = swept
    for name in bpl.RECORDED:
        ref = golden[name].astype(np.int64)
        assert ref.shape == q[name].shape, name
        bad = np.nonzero(ref != q[name])[0]
        assert len(bad) == 0, "%s, first of %d: input %s planned %d recorded %d" % (
            name, len(bad), {k: int(v[bad[0]]) for k, v in r.items()}, q[name][bad[0]], ref[bad[0]])


def test_fixture_holds_the_spot_values(golden, sizes):
    """read off the launchers the fixture was recorded from"""
    rows = np.concatenate([bpl.sweep(), bpl.extra_rows()])
    assert len(rows) == len(golden["formCode"]) == 721464 and sizes == (120, 133584)

    def at(**want):
        sel = np.ones(len(rows), bool)
        for k, v in want.items():
            sel &= rows[:, bpl.INPUTS.index(k)] == v
        k = np.nonzero(sel)[0]
        assert len(k) >= 1, want
        return {name: int(golden[name][k[0]]) for name in bpl.RECORDED}
    base = dict(L=2048, N=6000, F=9, priorM=30, ownsCamera=1)
    g = at(dC=60, anyExtVariable=0, switches=0, **base)      # ten poses: the bench's narrow window
    assert (g["formCode"], g["variant"], g["aMfma"], g["aBlocks"], g["nSlabs"], g["reduceSlabCount"]) == (1090, 3, 0, 0, 128, 128)
    assert g["schurDense_lds"] == (16 * 4 * 49 + 4 * 10 * 28) * 8 and g["evalBuild256"] == 1 and g["evalBuildSmall"] == 0 and g["fusable"] == 1
    assert g["reprojSplit_lds"] == 48 * 8 + (11 + 2) * 56 + 2 * 120 + 240 + 64
    g = at(dC=180, anyExtVariable=0, switches=0, **base)     # 30 pose blocks, twelve tile rows: <10, true, 8>, A block-wise
    assert (g["formCode"], g["variant"], g["aMfma"], g["aBlocks"], g["evalBuild256"]) == (1101, 1, 1, 1, 0)
    assert at(dC=180, anyExtVariable=0, switches=bpl.A_MFMA, **base)["formCode"] == 1102
    assert at(dC=252, anyExtVariable=0, switches=0, **base)["formCode"] == 1171
    assert at(dC=960, anyExtVariable=0, switches=0, **base)["formCode"] == 2000          # config #4
    assert at(dC=960, anyExtVariable=0, switches=bpl.PANELS_OLD, **base)["formCode"] == 3000
    g = at(dC=960, anyExtVariable=1, switches=0, **base)
    assert (g["formCode"], g["useLdsOfForm"], g["nSlabs"], g["reduceSlabCount"]) == (4001, 0, 1, 1)
    g = at(dC=60, anyExtVariable=0, switches=bpl.PAIRWISE, **base)
    assert (g["formCode"], g["useLdsOfForm"], g["nSlabs"], g["reduceSlabCount"]) == (4000, 1, 256, 256)
    g = at(dC=60, anyExtVariable=0, switches=0, L=0, N=5, F=9, priorM=30, ownsCamera=1)
    assert (g["formCode"], g["variant"], g["reduceSlabCount"]) == (5000, -1, 0)


# ------------------------------------------------------------------------------------------------ 2. properties over the sweep
def producible(r, q):
    """rows Window::pack() can produce: the dense form's pose -> row map holds kDensePoseCap poses, a pose block is six rows"""
    return (r["dC"] % 6 == 0) & (r["dCPose"] <= r["dC"])


def test_every_planned_launch_fits_the_machine(swept):
    r, q = swept
    ok = producible(r, q)
    assert int((~ok).sum()) == 28, "rows chooseSchurForm cannot produce (dC no multiple of 6): left out"
    for name in bpl.LAUNCHES:
        lds = q[name + "_lds"]
        assert np.all(lds >= 0) and np.all(lds[ok] <= LDS_BYTES), (name, int(lds[ok].max()))
    for name in ("reprojSplit_lds", "reprojAlone_lds"):
        fits = q["fusable"] != 0   # (a staging area beyond the factor blocks' LDS is refused by the launch, as it was)
        assert np.all(q[name][ok & fits] <= LDS_BYTES), name
    assert np.all(np.isin(q["denseThreads"][q["form"] == bpl.DENSE], (256, 512))) and np.all(q["denseThreads"][q["form"] != bpl.DENSE] == 0)


def test_exactly_the_launches_of_the_chosen_form_have_a_grid(swept):
    r, q = swept
    of_form = {bpl.DENSE: ("schurDense", "reduceSlabs"),
               bpl.BLOCK_PAIRS: ("panelsLandmarks", "blocksSlots", "schurRows", "blocksPoseReduce", "factorsOnly", "reducePanelSlabs"),
               bpl.PANELS: ("panelsLandmarks", "schurPanels", "factorsOnly", "reducePanelSlabs"),
               bpl.PAIRWISE_FORM: ("pairwise", "reduceSlabs"),
               bpl.FACTORS_ONLY: ("factorsOnly",)}
    ride = q["nFac"] + q["nPri"]
    # the launches whose grid is a count that may be zero (no factors and no prior; a wide window whose landmarks have no slots)
    may_be_empty = {"factorsOnly": ride == 0, "blocksSlots": r["nSlots"] == 0, "blocksPoseReduce": r["nSlots"] == 0,
                    "schurRows": r["nPanelBlocks"] == 0, "schurPanels": r["nPanelBlocks"] == 0}
    for form, mine in of_form.items():
        rows = q["form"] == form
        assert rows.sum() > 100, bpl.FORMS[form]
        for name in bpl.LAUNCHES:
            grid = q[name + "_grid"][rows]
            if name in mine:
                empty = may_be_empty.get(name, np.zeros(len(rows), bool))[rows]
                assert np.all((grid > 0) == ~empty), (bpl.FORMS[form], name)
            else:
                assert np.all(grid == 0), (bpl.FORMS[form], name)
    landmarks = (r["L"] > 0) & (r["N"] > 0) & (r["dC"] > 0)
    assert np.array_equal(q["form"] == bpl.FACTORS_ONLY, ~landmarks)
    assert np.array_equal(q["form"] == bpl.DENSE, landmarks & (q["schurDenseFlag"] != 0))
    assert np.array_equal(q["form"] == bpl.BLOCK_PAIRS, landmarks & (q["schurBlocksFlag"] != 0))
    assert np.array_equal(q["form"] == bpl.PANELS, landmarks & (q["schurPanelsFlag"] != 0) & (q["schurBlocksFlag"] == 0))
    assert np.array_equal(q["formCode"] // 1000 - 1, q["form"])


def test_the_slab_sum_takes_the_slabs_the_build_wrote(swept):
    """what the three copies of the "a slab fits LDS" test protected"""
    r, q = swept
    dense, pw = q["form"] == bpl.DENSE, q["form"] == bpl.PAIRWISE_FORM
    # dense: one private slab per chunk block, the blocks behind them are the factors' and the prior's
    assert np.all((q["reduceSlabCount"] == q["schurDense_grid"] - q["nFac"] - q["nPri"])[dense])
    # pairwise with LDS slabs: one per landmark block; without: the blocks add to ONE global slab, which the launcher cleared
    lds = pw & (q["useLds"] != 0)
    assert np.all((q["reduceSlabCount"] == q["pairwise_grid"] - q["nFac"] - q["nPri"])[lds]) and np.all((q["reduceSlabCount"] == q["pairwiseChunkBlocks"])[lds])
    glob = pw & (q["useLds"] == 0)
    assert lds.sum() > 1000 and glob.sum() > 1000
    assert np.all(q["reduceSlabCount"][glob] == 1) and np.all((q["slabBytes"] == (r["dC"] ** 2 + 3 * r["dC"]) * 8)[glob])
    # ... and pack() allocated that many: DeviceProblem::nSlabs (chooseSchurForm) is what the launch is told to sum, or more
    assert np.all((q["reduceSlabCount"] == q["nSlabs"])[dense | pw])
    assert np.all((q["useLds"] == q["useLdsOfForm"])[pw]), "pack()'s useLds and the launcher's"
    # the panel forms and a window without a landmark part do not launch k_reduce_slabs at all
    rest = ~(dense | pw)
    assert np.all(q["reduceSlabCount"][rest] == 0) and np.all(q["reduceSlabs_grid"][rest] == 0)
    assert np.all((q["reduceSlabs_grid"] == (r["dC"] ** 2 + 3 * r["dC"] + 15) // 16)[~rest])
    # the slab buffer holds what is summed: nSlabs slabs of dC^2 + 3 dC doubles (window.cpp reserves exactly that)
    assert np.all(q["reduceSlabCount"] <= np.maximum(q["nSlabs"], 1))


def test_what_a_batch_shares_is_a_function_of_the_group_fields(swept):
    """the batched path's premise: the dense variant, its LDS bytes, aBlocks, the slab sum's grid and the evaluation's stage bytes
    are equal for any two windows that agree in the integers of BatchGroupFields, whatever their L and N"""
    r, q = swept
    rows = (q["form"] == bpl.DENSE) & ((r["switches"] & (bpl.PAIRWISE | bpl.PANELS_OLD | bpl.SLAB_CHUNKS_2)) == 0)
    group = ("dC", "dCPose", "F", "nPose", "nExt", "priorM", "anyExtVariable", "nCam", "switches")   # (the fields of the group key a row has; SVIN_SCHUR_A_MFMA is process-wide)
    shared = ("variant", "denseThreads", "schurDense_lds", "aMfma", "aBlocks", "reduceSlabs_grid", "reprojSplit_lds")
    # (EvalPlan::fusable is NOT among them -- the partial slots bound N -- and batchSupported asks it of every window itself)
    key = np.stack([r[k][rows] for k in group], axis=1)
    val = np.stack([q[k][rows] for k in shared], axis=1)
    order = np.lexsort(key.T[::-1])
    key, val, L = key[order], val[order], r["L"][rows][order]
    same = np.all(key[1:] == key[:-1], axis=1)
    assert same.sum() > 10000 and len(np.unique(L)) >= 9
    assert np.all(val[1:][same] == val[:-1][same])
    # ... while the extents do differ inside a group
    assert np.any((q["schurDense_grid"][rows][order][1:] != q["schurDense_grid"][rows][order][:-1]) & same)


def test_launch_sizes_are_the_expressions_the_launchers_held(swept, sizes, lib):
    """grid and dynamic LDS of every launch against the expressions as launchAccumulateNormalEquations, launchEvalAll,
    launchEvalReproj, launchEvalBuild and launchDoglegPrepare wrote them out before the planner existed (restated here once, on purpose)"""
    r, q = swept
    c = bpl.constants(lib)
    cm, fs = sizes
    dC, L, N, F = r["dC"], r["L"], r["N"], r["F"]
    nPri = np.where((r["priorM"] > 0) & (r["ownsCamera"] != 0), (r["priorM"] ** 2 + 255) // 256, 0)
    assert np.array_equal(q["nFac"], F) and np.array_equal(q["nPri"], nPri)
    dense = q["form"] == bpl.DENSE
    assert np.all((q["schurDense_grid"] == q["nSlabs"] + F + nPri)[dense])
    nTr = (dC + 2 + 15) // 16
    ladder = np.where(nTr > 12, 0, np.where(nTr > 8, 1, np.where((r["anyExtVariable"] != 0) | (nTr > 8), 2, 3)))
    assert np.all((q["variant"] == ladder)[dense]) and np.all(q["variant"][~dense] == -1)
    assert np.all((q["denseThreads"] == np.where(ladder <= 1, 512, 256))[dense])
    bp = q["form"] == bpl.BLOCK_PAIRS
    nCopies = np.full(len(dC), 4)
    for _ in range(2):
        nCopies = np.where((nCopies > 1) & (nCopies * (dC // 6) * 35 * 8 > 76 * 1024), nCopies // 2, nCopies)
    nSlotBlocks = (r["nSlots"] + 1023) // 1024
    assert np.all((q["nCopies"] == nCopies)[bp]) and np.all((q["blocksSlots_lds"] == nCopies * (dC // 6) * 35 * 8)[bp])
    assert np.all((q["nSlotBlocks"] == nSlotBlocks)[bp]) and np.all((q["blocksSlots_grid"] == nSlotBlocks)[bp])
    assert np.all((q["schurRows_grid"] == r["nPanelBlocks"])[bp]) and np.all((q["schurRows_lds"] == max(2 * 230 * 20, 16 * 16 * 36) * 8)[bp])
    assert np.all((q["blocksPoseReduce_grid"] == np.where(nSlotBlocks > 0, dC // 6, 0))[bp])
    pn = q["form"] == bpl.PANELS
    assert np.all((q["schurPanels_grid"] == r["nPanelBlocks"])[pn]) and np.all((q["schurPanels_lds"] == (2 * 96 * 49 + 48) * 8)[pn])
    wide = bp | pn
    assert np.all((q["panelsLandmarks_grid"] == (L + 15) // 16)[wide]) and np.all((q["factorsOnly_grid"] == F + nPri)[wide | (q["form"] == bpl.FACTORS_ONLY)])
    assert np.all((q["reducePanelSlabs_grid"] == (96 * 96 + 3 * 96 + 15) // 16)[wide]) and np.all((q["reducePanelPairs"] == r["nPanelPairs"])[wide])
    pw = q["form"] == bpl.PAIRWISE_FORM
    acc, stage = (dC * dC + 3 * dC) * 8, 4 * 64 * 34 * 8
    use_lds = acc + stage <= 150 * 1024
    assert np.all((q["useLds"] != 0)[pw] == use_lds[pw])
    assert np.all((q["pairwise_lds"] == np.where(use_lds, acc + stage, stage))[pw])
    assert np.all((q["pairwise_grid"] == np.where(use_lds, q["nSlabs"], np.minimum((L + 3) // 4, 2048)) + F + nPri)[pw])
    assert (c["kStage"], c["kBlkPoseLd"], c["kSlotCopiesKB"], c["kBlkBatchRecs"], c["kBlkStride"], c["kBlkSlotsPerWorkgroup"]) == (34, 35, 76, 230, 20, 1024)
    assert (c["kDenseLd"], c["kDenseK"], c["kPoseAcc"], c["kPanelRows"], c["kPanelSlab"], c["kBlkPanelPoses"]) == (49, 48, 28, 96, 96 * 96 + 288, 16)
    # the evaluation: the four sums of the staging area
    tables = (r["nPose"] + r["nExt"]) * 7 * 8 + r["nCam"] * cm + 2 * 15 * 8
    nR, pri = (N + 255) // 256, (r["priorM"] > 0).astype(np.int64)
    assert np.array_equal(q["reprojAlone_lds"], tables) and np.array_equal(q["reprojAlone_grid"], (N + 127) // 128)   # launchEvalReproj
    assert np.array_equal(q["fusable"] != 0, (F > 0) & (N > 0) & (tables + 64 <= fs) & (nR + F <= 4096))              # canFuseEvaluation
    assert np.array_equal(q["reprojSplit_lds"], 48 * 8 + tables + 64)                                                  # evalSplitStageBytes
    assert np.array_equal(q["stageBytes"], tables)                                                                     # launchEvalBuild
    assert np.array_equal(q["nR"], nR) and np.array_equal(q["pri"], pri)
    assert np.array_equal(q["evalAll_grid"], F + nR + pri) and np.array_equal(q["reprojSplit_grid"], nR) and np.array_equal(q["restSplit_grid"], F + pri)
    assert np.array_equal(q["split"] != 0, F + nR + pri > 512)
    # the post-solve pass
    nLm = np.where((L > 0) & (N > 0), np.minimum((L + 15) // 16, 1024), 0)
    nFacB = np.where(F > 0, np.minimum((F + 3) // 4, 1024), 0)
    assert np.array_equal(q["postLm"], nLm) and np.array_equal(q["postFac"], nFacB) and np.array_equal(q["post_grid"], nLm + nFacB + 1)
    assert np.array_equal(q["postSplit"] != 0, nLm + nFacB + 1 > 512)
    # k_eval_build: the condition of launchEvalBuild (one GPU) with evalBuildFits written out
    plain = dense & (q["aMfma"] == 0) & (r["anyExtVariable"] == 0) & (q["fusable"] != 0)
    room = ((q["schurDense_lds"] + 15) // 16 * 16 + tables <= fs) & (F + nR + pri > 0) & (q["nSlabs"] > 0)
    for name, cus in (("evalBuild256", 256), ("evalBuildSmall", bpl.SMALL_CUS)):
        assert np.array_equal(q[name] != 0, plain & room & (F + nR + pri + q["nSlabs"] <= cus)), name


def test_no_eval_split_keeps_the_one_launch_forms(lib, sizes):
    big = bpl.row(60, 20000, 200000, F=9)
    on, off = bpl.plan(lib, [big], *sizes), bpl.plan(lib, [big[:-1] + [bpl.NO_EVAL_SPLIT]], *sizes)
    assert (int(on["split"][0]), int(on["postSplit"][0])) == (1, 1) and (int(off["split"][0]), int(off["postSplit"][0])) == (0, 0)
    for k in ("evalAll_grid", "reprojSplit_grid", "restSplit_grid", "post_grid", "reprojSplit_lds"):
        assert on[k][0] == off[k][0]


# ------------------------------------------------------------------------------------------------ 3. the step mode
def step_rows():
    rows = []
    for blocks in (0, 40, 16383, 16384, 16385, 40000):   # nPose + nExt + nSb + L
        for L, N in ((0, 0), (0, 5), (min(blocks, 7), 0), (min(blocks, 7), 50), (blocks, 3 * blocks + 1)):
            rest = blocks - L
            for fusable in (0, 1):
                for sw in range(8):
                    for sharded in (0, 1):
                        rows.append([rest // 3, rest // 3, rest - 2 * (rest // 3), L, N, fusable, sw, sharded])
    return np.array(rows, np.int64)


def test_step_mode_is_the_three_expressions_it_replaces(lib):
    """Window::solve, Window::debugTrustRegionStep and batchSupported as they decided the step before the planner existed"""
    rows = step_rows()
    q = bpl.step_mode(lib, rows)
    nPose, nExt, nSb, L, N = (rows[:, k] for k in range(5))
    fusable, sharded = rows[:, 5] != 0, rows[:, 7] != 0
    split_eval, no_fuse_step, no_defer_lm = ((rows[:, 6] & b) != 0 for b in (1, 2, 4))
    assert len(rows) == 6 * 5 * 2 * 8 * 2 and np.any(nPose + nExt + nSb + L == 16384) and np.any(nPose + nExt + nSb + L == 16385)
    # Window::solve (dist = sharded)
    defer_possible = fusable & ~split_eval & ~no_defer_lm & (L > 0) & (N > 0)
    fuse_step = ~no_fuse_step & ~sharded & ((nPose + nExt + nSb + L <= 16384) | defer_possible)
    defer_lm = fuse_step & defer_possible
    assert np.array_equal(q["fuseStep"] != 0, fuse_step) and np.array_equal(q["deferLm"] != 0, defer_lm)
    assert not np.any(sharded & ((q["fuseStep"] != 0) | (q["deferLm"] != 0))), "a sharded solve takes neither (solve() throws otherwise)"
    # Window::debugTrustRegionStep (one GPU only)
    one = ~sharded
    small = nPose + nExt + nSb + L <= 16384
    fuse_dbg = ~no_fuse_step & (small | defer_possible)
    chosen = np.where(fuse_dbg, np.where(defer_possible, 3, 1), 2)
    assert np.array_equal(q["chosenForm"][one], chosen[one]) and np.array_equal(q["deferPossible"] != 0, defer_possible) and np.array_equal(q["small"] != 0, small)
    # batchSupported, on the windows that reach its step condition (L > 0 and N > 0 were asked before it): refused when
    # !canFuseEvaluation || SVIN_SPLIT_EVAL || SVIN_NO_FUSE_STEP || SVIN_NO_DEFER_LM, or with more than 16384 blocks
    reach = one & (L > 0) & (N > 0)
    refused = ~fusable | split_eval | no_fuse_step | no_defer_lm | (nPose + nExt + nSb + L > 16384)
    assert np.array_equal(q["batched"][reach] != 0, ~refused[reach]) and 0 < (q["batched"][reach] != 0).sum() < reach.sum()
    assert np.all(q["chosenForm"][q["batched"] != 0] == 3)


# ------------------------------------------------------------------------------------------------ 4. boundaries
# Values read off kernels.hip and pack_plan.hpp as they stood before the planner.  name: (row arguments) -> {field: value}
B = dict(L=1000, N=9000)
BOUNDARIES = {
    # nTr = (dC + 2 + 15) / 16: 8 tile rows up to dC = 126, 12 up to 190
    "dC126_eight_tile_rows": (dict(dC=126, **B), dict(variant=3, formCode=1090, aMfma=0, denseThreads=256)),
    "dC132_nine_tile_rows": (dict(dC=132, **B), dict(variant=1, formCode=1101, aMfma=1, denseThreads=512)),
    "dC186_twelve_tile_rows": (dict(dC=186, **B), dict(variant=1, formCode=1101)),
    "dC192_thirteen_tile_rows": (dict(dC=192, **B), dict(variant=0, formCode=1171, denseThreads=512)),
    "dC126_variable_extrinsics": (dict(dC=126, dCPose=60, any_ext=1, **B), dict(variant=2, formCode=1091, aMfma=1, denseThreads=256)),
    # dC + 2 <= 256 and at most kDensePoseCap pose slots
    "dC252_last_dense": (dict(dC=252, **B), dict(form=bpl.DENSE, variant=0, formCode=1171)),
    "dC258_first_wide": (dict(dC=258, **B), dict(form=bpl.BLOCK_PAIRS, formCode=2000, variant=-1)),
    "dC258_variable_extrinsics_pairwise_global": (dict(dC=258, dCPose=120, any_ext=1, **B), dict(form=bpl.PAIRWISE_FORM, formCode=4001, useLds=0, reduceSlabCount=1)),
    "pose_slots_256_dense": (dict(dC=60, nPose=256, **B), dict(form=bpl.DENSE)),
    "pose_slots_257_panels": (dict(dC=60, nPose=257, **B), dict(form=bpl.BLOCK_PAIRS)),
    # aBlocks: (rows * 49 + (dC / 6) * 28 + nEB * nPB * 36) * 8 <= 150 * 1024; dC = 252, rows = 256: 12544 + 1176 + 36 nEB nPB <= 19200
    # <=> nEB nPB <= 152: 4 x 38 fits, 5 x 37 does not
    "aBlocks_last_that_fits": (dict(dC=252, dCPose=228, any_ext=1, **B), dict(aBlocks=1, formCode=1171, schurDense_lds=(256 * 49 + 42 * 28 + 4 * 38 * 36) * 8)),
    "aBlocks_first_that_does_not": (dict(dC=252, dCPose=222, any_ext=1, **B), dict(aBlocks=0, formCode=1172, schurDense_lds=(256 * 49 + 256 * 17) * 8)),
    "aBlocks_switched_off": (dict(dC=252, dCPose=228, any_ext=1, switches=bpl.A_MFMA, **B), dict(aBlocks=0, formCode=1172)),
    # pairwise: (dC^2 + 3 dC) * 8 + 4 * 64 * 34 * 8 <= 150 * 1024  <=>  dC <= 100
    "pairwise_dC96_lds_slabs": (dict(dC=96, switches=bpl.PAIRWISE, **B), dict(formCode=4000, useLds=1, reduceSlabCount=125, pairwise_lds=(96 * 96 + 288) * 8 + 69632)),
    "pairwise_dC100_lds_slabs": (dict(dC=100, switches=bpl.PAIRWISE, **B), dict(formCode=4000, useLds=1, useLdsOfForm=1)),
    "pairwise_dC101_global_slab": (dict(dC=101, switches=bpl.PAIRWISE, **B), dict(formCode=4001, useLds=0, useLdsOfForm=0, reduceSlabCount=1, nSlabs=1)),
    "pairwise_dC102_global_slab": (dict(dC=102, switches=bpl.PAIRWISE, **B), dict(formCode=4001, useLds=0, reduceSlabCount=1, pairwise_lds=69632, pairwise_grid=250 + 9 + 4)),
    "pairwise_grid_cap": (dict(dC=102, L=8193, N=20001, switches=bpl.PAIRWISE), dict(pairwiseChunkBlocks=2048)),
    # block pairs: nCopies * (dC / 6) * 35 * 8 > 76 * 1024 halves nCopies: 69 | 70 and 138 | 139 pose blocks
    "blocks_69_four_copies": (dict(dC=414, **B), dict(nCopies=4, blocksSlots_lds=4 * 69 * 280)),
    "blocks_70_two_copies": (dict(dC=420, **B), dict(nCopies=2, blocksSlots_lds=2 * 70 * 280)),
    "blocks_138_two_copies": (dict(dC=828, **B), dict(nCopies=2)),
    "blocks_139_one_copy": (dict(dC=834, **B), dict(nCopies=1, blocksSlots_lds=139 * 280)),
    "blocks_512_pose_blocks": (dict(dC=3072, **B), dict(form=bpl.BLOCK_PAIRS, nCopies=1, blocksSlots_lds=512 * 280)),
    "blocks_513_tile_form": (dict(dC=3078, **B), dict(form=bpl.PANELS, formCode=3000)),
    # evaluation: more than kEvalSplitBlocks = 512 blocks (F + nR + pri; nLm + nFac + 1), kMaxPartials = 4096 partial slots
    "eval_512_blocks_one_launch": (dict(dC=60, L=1000, N=502 * 256, F=9, priorM=30), dict(split=0, evalAll_grid=512)),
    "eval_513_blocks_split": (dict(dC=60, L=1000, N=502 * 256 + 1, F=9, priorM=30), dict(split=1, reprojSplit_grid=503, restSplit_grid=10)),
    "post_512_blocks": (dict(dC=60, L=16 * 508, N=30000, F=9), dict(postSplit=0, post_grid=512)),
    "post_513_blocks_wide_kernel": (dict(dC=60, L=16 * 508 + 1, N=30000, F=9), dict(postSplit=1, post_grid=513)),
    "partials_4096_fusable": (dict(dC=60, L=1000, N=4087 * 256, F=9), dict(fusable=1)),
    "partials_4097_not_fusable": (dict(dC=60, L=1000, N=4087 * 256 + 1, F=9), dict(fusable=0, evalBuild256=0)),
}


@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_boundary(lib, sizes, name):
    args, want = BOUNDARIES[name]
    args = dict(args)
    q = plan_one(lib, sizes, args.pop("dC"), args.pop("L"), args.pop("N"), **args)
    assert {k: q[k] for k in want} == want


@pytest.mark.parametrize("cus, taken", [(256, True), (255, False)])
def test_eval_build_with_exactly_as_many_workgroups_as_compute_units(lib, sizes, cus, taken):
    """evalBuildFits: F + nR + pri evaluation blocks and nSlabs chunk blocks, one workgroup per compute unit"""
    row = bpl.row(60, 16 * 240, 900, F=11, priorM=30)   # 11 + 4 + 1 evaluation blocks, 240 slabs: 256 workgroups
    q = {k: int(v[0]) for k, v in bpl.plan(lib, [row], *sizes).items()}
    assert q["evalAll_grid"] + q["nSlabs"] == 256 and q["variant"] == 3
    assert bpl.eval_build(lib, row, *sizes, compute_units=cus) == taken
    assert not bpl.eval_build(lib, row, *sizes, compute_units=cus, sharded=True)
    more = bpl.row(60, 16 * 241, 900, F=11, priorM=30)    # one more chunk block
    assert not bpl.eval_build(lib, more, *sizes, compute_units=256) and bpl.eval_build(lib, more, *sizes, compute_units=257)


# ------------------------------------------------------------------------------------------------ 5. under a sanitizer
def test_planner_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program (its own main, the whole sweep), run as a child"""
    exe = str(tmp_path / "build_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "build_plan_sanitize.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout[-4000:]
