"""ctypes access to the host planning of the build, the evaluation and the step (svin_amd/csrc/build_plan.hpp through
tests/csrc/build_plan_shim.cpp) and the sweep of window geometries its tests run over.  Shared by tests/test_build_plan_host.py,
tests/golden/make_golden_build_plan.py and tests/test_gpu_schur_edges.py.

An input row is the integers of DeviceProblem the launchers read, in the order of INPUTS, and the switches as bits.  pack() is
part of a row's meaning: schurDense / schurPanels / schurBlocks / nSlabs are what chooseSchurForm (pack_plan.hpp) gives for the
row, exactly as Window::pack() fills DeviceProblem from it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
INPUTS = ("dC", "dCPose", "anyExtVariable", "L", "N", "F", "priorM", "ownsCamera", "nPose", "nExt", "nCam", "nSlots", "nPanelBlocks",
          "nPanelPairs", "switches")
PAIRWISE, PANELS_OLD, A_MFMA, SLAB_CHUNKS_2, NO_EVAL_SPLIT = 1, 2, 4, 8, 16   # bits of `switches` (SVIN_SLAB_CHUNKS: 0 or 2)
FORMS = ("dense", "block_pairs", "panels", "pairwise", "factors_only")
DENSE, BLOCK_PAIRS, PANELS, PAIRWISE_FORM, FACTORS_ONLY = range(5)
VARIANTS = ("17_mfma_8", "10_mfma_8", "9_mfma_4", "9_copies_4")   # k_schur_dense<17, true, 8> ... <9, false, 4>
LAUNCHES = ("schurDense", "panelsLandmarks", "blocksSlots", "schurRows", "blocksPoseReduce", "schurPanels", "factorsOnly",
            "reducePanelSlabs", "pairwise", "reduceSlabs")
FIELDS = (("schurDenseFlag", "schurPanelsFlag", "schurBlocksFlag", "nSlabs", "useLdsOfForm",   # chooseSchurForm, as pack() takes it
           "form", "formCode", "nFac", "nPri", "variant", "aMfma", "aBlocks", "denseThreads", "nCopies", "nSlotBlocks", "useLds",
           "pairwiseChunkBlocks", "slabBytes", "reducePanelPairs", "reduceSlabCount")
          + tuple(l + s for l in LAUNCHES for s in ("_grid", "_lds"))
          + ("fusable", "split", "nR", "pri", "stageBytes", "evalAll_grid", "reprojSplit_grid", "reprojSplit_lds", "restSplit_grid",
             "reprojAlone_grid", "reprojAlone_lds", "postSplit", "postLm", "postFac", "post_grid", "evalBuild256", "evalBuildSmall"))
CONSTANTS = ("kDenseLm", "kDenseK", "kDenseLd", "kPoseAcc", "kStage", "kPanelRows", "kPanelSlab", "kBlkPanelPoses", "kBlkStride",
             "kBlkPoseLd", "kSlotCopiesKB", "kEvalSplitBlocks", "kMaxPartials", "kBlkMaxPoseBlocks", "kDensePoseCap", "kLossTabBytes",
             "kBlkBatchRecs", "kBlkSlotsPerWorkgroup", "kBlkWaves")
# what the fixture records of a row (tests/golden/build_plan.npz)
RECORDED = ("formCode", "variant", "aMfma", "aBlocks", "schurDense_lds", "useLdsOfForm", "nSlabs", "reduceSlabCount", "evalBuild256",
            "evalBuildSmall", "fusable", "reprojSplit_lds")
SMALL_CUS = 40          # the "small" compute-unit count of the evalBuild columns
STEP_SWITCHES = ("splitEval", "noFuseStep", "noDeferLm")


def dC_values():
    """every whole number of pose blocks through the dense / wide boundary (dC + 2 <= 256), the halvings of nCopies (70 / 139 pose
    blocks) and config #4 (960) up to 1002, then every eighth, and every one again around 6 * kBlkMaxPoseBlocks = 3072"""
    v = set(range(0, 1008, 6)) | set(range(1008, 3100, 48)) | set(range(3054, 3096, 6))
    return np.array(sorted(v), np.int32)


# (L, N): around nothing, one chunk of 16, the 256-slab caps (8 landmarks per pairwise slab, 16 per dense one) and the pairwise
# form's grid cap of 2048 blocks of four landmarks
LN = ((0, 0), (0, 5), (1, 0), (1, 3), (15, 40), (16, 50), (17, 60), (2048, 6000), (2049, 6001), (4096, 12000), (4097, 12001),
      (8192, 20000), (8193, 20001))
FPO = ((0, 0, 1), (9, 0, 1), (9, 30, 1), (9, 30, 0))   # (F, priorM, ownsCamera)


def panel_counts(dC, L):
    """stand-ins for the wide form's counts (pack() takes them from its work lists): plain functions of the row"""
    nPan = (dC + 95) // 96
    pairs = nPan * (nPan + 1) // 2
    return 7 * L, np.where(L > 0, 3 * pairs + 1, 0), pairs   # nSlots, nPanelBlocks, nPanelPairs


def sweep():
    """dC x (fixed extrinsics | variable ones with the reduced rows split three ways) x the sixteen switch combinations x (F, prior,
    ownsCamera) x (L, N), the last fastest"""
    parts = []
    ln = np.array(LN, np.int32)
    for dC in dC_values().tolist():
        nB = dC // 6
        splits = [(0, dC)] + [(1, 6 * k) for k in sorted({nB // 2, max(nB - 1, 0), nB // 5})]
        for any_ext, dCPose in splits:
            for sw in range(16):
                for F, priorM, owns in FPO:
                    n = len(ln)
                    L, N = ln[:, 0], ln[:, 1]
                    nSlots, nPanelBlocks, nPanelPairs = panel_counts(dC, L)
                    full = lambda x: np.full(n, x, np.int32)
                    parts.append(np.stack([full(dC), full(dCPose), full(any_ext), L, N, full(F), full(priorM), full(owns),
                                           full(dCPose // 6 + 1), full(2 + (dC - dCPose) // 6), full(2), nSlots, nPanelBlocks,
                                           full(nPanelPairs), full(sw)], axis=1))
    return np.ascontiguousarray(np.concatenate(parts), np.int32)


def row(dC, L, N, dCPose=None, any_ext=0, F=9, priorM=30, owns=1, nPose=None, nExt=None, nCam=2, switches=0):
    dCPose = dC if dCPose is None else dCPose
    nSlots, nPanelBlocks, nPanelPairs = panel_counts(dC, np.int32(L))
    return [dC, dCPose, any_ext, L, N, F, priorM, owns, dCPose // 6 + 1 if nPose is None else nPose,
            2 + (dC - dCPose) // 6 if nExt is None else nExt, nCam, int(nSlots), int(nPanelBlocks), int(nPanelPairs), switches]


def extra_rows():
    """rows off the sweep's grid: 256 / 257 pose slots, the evaluation's staging area at the size of the factor blocks' LDS, the
    partial slots of the fused evaluation, compute-unit counts met exactly, and dC that is no multiple of 6"""
    rows = [row(60, 100, 900, nPose=256), row(60, 100, 900, nPose=257), row(60, 100, 900, nPose=257, any_ext=1, dCPose=30)]
    for n in range(2280, 2380, 2):
        rows.append(row(60, 100, 900, nPose=n))
    for dN in (-1, 0, 1):
        rows.append(row(60, 100, (4096 - 9) * 256 + dN, F=9))
    for L in (16 * 240, 16 * 245, 16 * 246, 16 * 247, 16 * 26, 16 * 27, 16 * 28, 16 * 29, 16 * 30):   # slabs + evaluation blocks around 256 / 40
        rows += [row(60, L, 900, F=5), row(60, L, 900, F=5, priorM=0), row(126, L, 900, F=5), row(132, L, 900, F=5)]
    for dC in (1, 5, 7, 97, 100, 101, 127, 191, 193, 253, 254, 255, 256, 257):
        rows += [row(dC, 100, 900, dCPose=dC // 6 * 6), row(dC, 100, 900, switches=PAIRWISE)]
    return np.ascontiguousarray(np.array(rows, np.int32))


def build_shim(directory):
    so = os.path.join(str(directory), "libbp.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "build_plan_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.bp_plan.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    lib.bp_plan.restype = None
    lib.bp_step_mode.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.bp_step_mode.restype = None
    lib.bp_eval_build.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int]
    assert lib.bp_fields() == len(FIELDS) and lib.bp_inputs() == len(INPUTS)
    return lib


def plan(lib, rows, camera_model_bytes, factor_shared_bytes, small_cus=SMALL_CUS):
    """rows: (k, len(INPUTS)) integers -> {field: int64 array of k}; the two sizes are the kernels' sizeof(CameraModel) and
    sizeof(FactorShared), which the planner takes as arguments"""
    rows = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, len(INPUTS)))
    out = np.zeros((len(rows), len(FIELDS)), np.int64)
    lib.bp_plan(len(rows), rows.ctypes.data_as(C.c_void_p), int(camera_model_bytes), int(factor_shared_bytes), int(small_cus),
                out.ctypes.data_as(C.c_void_p))
    return {name: out[:, k] for k, name in enumerate(FIELDS)}


def step_mode(lib, rows):
    """rows: (k, 8) = nPose, nExt, nSb, L, N, fusable, switches (bits of STEP_SWITCHES), sharded -> {field: array}"""
    rows = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 8))
    out = np.zeros((len(rows), 6), np.int32)
    lib.bp_step_mode(len(rows), rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return {name: out[:, k] for k, name in enumerate(("fuseStep", "deferLm", "chosenForm", "deferPossible", "small", "batched"))}


def constants(lib):
    return {name: lib.bp_constant(k) for k, name in enumerate(CONSTANTS)}


def eval_build(lib, one_row, camera_model_bytes, factor_shared_bytes, compute_units, sharded=False):
    a = np.ascontiguousarray(np.asarray(one_row, np.int32).reshape(len(INPUTS)))
    return bool(lib.bp_eval_build(a.ctypes.data_as(C.c_void_p), int(camera_model_bytes), int(factor_shared_bytes), int(compute_units), int(sharded)))
