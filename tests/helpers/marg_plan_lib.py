"""ctypes access to the host planning of the marginalisation (svin_amd/csrc/marg_plan.hpp through tests/csrc/marg_plan_shim.cpp)
and the sweep of job sizes its test runs over.  Used by tests/test_marg_plan_host.py.

An input row is MargDims' fields in their order, then margEig (SVIN_MARG_EIG, 0-3) and jacobiShared (sizeof(JacobiShared))."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
INPUTS = ("m", "Lm", "N", "F", "nk", "nm", "nPose", "nExt", "nCam", "anyExtVar", "oldPriorM", "margEig", "jacobiShared")
JACOBI_SHARED = 16   # sizeof(JacobiShared): a double and two ints (marg.hip)
LAUNCHES_M1 = ("accumLm", "accumFactors")
LAUNCHES_LM = ("lmPrepare", "lmApply", "lmUpdate")
LAUNCHES_M3 = ("finalChol", "finalDc", "final")
SIZES = ("bU", "bW2", "bV", "bVec", "bScratch", "bHk", "bOut", "bLin", "bFacLin", "bPartial", "bFlag", "bScal", "gLm", "gUv", "gW",
         "gLmPtr", "gObsLm", "gIdx")
CLEARS = ("clearU", "clearW2", "clearV", "clearVec")
REGIONS = ("ba", "bb", "vb", "linR", "linJp", "linJl", "linJe", "Vm", "Qm", "denseTmp", "Hk", "bk", "oldH", "oldB0", "G", "Q", "J", "Ht",
           "e0", "bp", "scal", "finalTmp")
# the buffer each region lies in
BUFFER_OF = dict(ba="bVec", bb="bVec", vb="bVec", linR="bLin", linJp="bLin", linJl="bLin", linJe="bLin", Vm="bScratch", Qm="bScratch",
                 denseTmp="bScratch", Hk="bHk", bk="bHk", G="bOut", Q="bOut", J="bOut", Ht="bOut", e0="bOut", bp="bOut", scal="bOut",
                 finalTmp="bOut")


def _pairs(names):
    return tuple(n + s for n in names for s in ("_grid", "_lds"))


FIELDS = (("reproj", "factors") + _pairs(LAUNCHES_M1) + ("accumCamX", "accumCamY") + _pairs(LAUNCHES_LM) + _pairs(("dense",))
          + ("denseUseLds", "denseProdLds", "denseTileChol", "copyPair") + _pairs(LAUNCHES_M3)
          + ("finalDcAfterChol", "finalMode", "finalFallbackLds", "finalSkipIfDone") + SIZES + CLEARS
          + tuple(r + s for r in REGIONS for s in ("_off", "_len")))
LDS_FUNCTIONS = ("jacobiLdsBytes", "jacobiLdsBytesGOnly", "margCholLdsBytes", "symEigLdsBytes", "jacobiLdsLimit", "jacobiLd",
                 "margGatherScratchInts")
CONSTANTS = ("kJacobiRegLen", "kPanelLd", "kSymEigMaxN", "kMargLdsPerWorkgroup")

# sizes of the dense part: 0 ... 4, every multiple of 16 up to 320 with its neighbours, and the sizes at which jacobiLdsBytes (96 | 97),
# jacobiLdsBytesGOnly (139 | 140, and its register limit 144 | 145), margCholLdsBytes and the direct solver (128 | 129) and the LDS
# image of mode 4 (136 | 137) change their answer
M_VALUES = sorted(set([0, 1, 2, 3, 4, 96, 97, 98, 128, 129, 136, 137, 139, 140, 141, 144, 145, 320]
                      + [16 * k + e for k in range(1, 21) for e in (-1, 0, 1) if 16 * k + e <= 320]))
LM_VALUES = (0, 1, 63, 64, 65, 127, 128, 129, 2000)


def sweep():
    """Two families, as rows of INPUTS.  (a) every split nk + nm = m of every m of M_VALUES x margEig 0-3, the M1 / landmark inputs
    rotating through their values; (b) every m x every Lm x N, F zero and not x anyExtVar 0, 1 with the splits nk = 0, nm = 0 and
    the halves, margEig 0.  oldPriorM rotates through 0 and sizes up to nk."""
    rows = []
    i = 0
    for m in M_VALUES:
        for nk in range(m + 1):
            for eig in range(4):
                Lm = LM_VALUES[i % len(LM_VALUES)]
                N = (0, 1, 37, 1500)[(i // 3) % 4]
                F = (0, 1, 5)[(i // 5) % 3]
                ext = (i // 7) % 2
                old = (0, nk, nk // 2, max(nk - 9, 0))[(i // 2) % 4]
                rows.append((m, Lm, N, F, nk, m - nk, 1 + i % 9, 1 + i % 4, 1 + i % 3, ext, old, eig, JACOBI_SHARED))
                i += 1
    for m in M_VALUES:
        for Lm in LM_VALUES:
            for N in (0, 3 * Lm + 1):
                for F in (0, 4):
                    for ext in (0, 1):
                        for nk in sorted(set((0, m, m // 2, (m + 1) // 2))):
                            rows.append((m, Lm, N, F, nk, m - nk, 7, 2, 2, ext, min(nk, 15), 0, JACOBI_SHARED))
    return np.ascontiguousarray(np.array(rows, np.int32))


def build_shim(directory):
    so = os.path.join(str(directory), "libmp.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "marg_plan_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.mp_plan.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.mp_plan.restype = None
    lib.mp_lds.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.mp_lds.restype = C.c_int64
    lib.mp_constant.restype = C.c_int64
    lib.mp_select_frames.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.mp_select_frames.restype = None
    assert lib.mp_fields() == len(FIELDS)
    return lib


def plan(lib, rows):
    """rows: (k, 13) integers -> {field: int64 array of k}"""
    rows = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, len(INPUTS)))
    out = np.zeros((len(rows), len(FIELDS)), np.int64)
    lib.mp_plan(len(rows), rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert out[0, 0] in (0, 1), "the shim wrote another number of fields than it announces"
    return {name: out[:, k] for k, name in enumerate(FIELDS)}


def lds(lib, name, n, jacobi_shared=JACOBI_SHARED):
    return int(lib.mp_lds(LDS_FUNCTIONS.index(name), int(n), int(jacobi_shared)))


def constants(lib):
    return {name: int(lib.mp_constant(k)) for k, name in enumerate(CONSTANTS)}


def select_frames(lib, ids, is_keyframe, num_keyframes, num_imu_frames):
    """-> None (fewer states than the IMU window) or (removeFrames, removeAllButPose, allLinearizedFrames)"""
    ids = np.ascontiguousarray(ids, np.uint64)
    kf = np.ascontiguousarray(is_keyframe, np.uint8)
    out = np.zeros(4 + 3 * len(ids), np.int64)
    lib.mp_select_frames(len(ids), ids.ctypes.data_as(C.c_void_p), kf.ctypes.data_as(C.c_void_p), num_keyframes, num_imu_frames,
                         out.ctypes.data_as(C.c_void_p))
    if not out[0]:
        return None
    lists, k = [], 1
    for _ in range(3):
        n = int(out[k])
        lists.append([int(v) for v in out[k + 1:k + 1 + n]])
        k += 1 + n
    return tuple(lists)
