"""ctypes access to the host planning of the reduced solve (svin_amd/csrc/solve_plan.hpp through tests/csrc/solve_plan_shim.cpp)
and the sweep of system sizes its tests run over.  Shared by tests/test_solve_plan_host.py, tests/golden/make_golden_solve_plan.py
and tools/dbg/sb_elim_dbg.py.

An input row is (d, dC, sbChain, sPadded, switches): DeviceProblem's fields of these names and the three switches the planner
takes as bits (NO_LL, NO_SB_ELIM, NO_LDS_BORDER)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NO_LL, NO_SB_ELIM, NO_LDS_BORDER = 1, 2, 4
ROUTES = ("lds_whole", "lds_border_load", "lds_border_prepared", "left_looking", "blocked")
LDS_WHOLE, LDS_BORDER_LOAD, LDS_BORDER_PREPARED, LEFT_LOOKING, BLOCKED = range(5)
REGIONS = ("factor", "borderScr", "bigM", "dinvG", "diagF", "ready", "compactS", "compactG", "Lf", "Y", "tvec", "counter")
LAUNCHES = ("sbFactor", "sbForward", "sbLoad", "borderPrepare", "cholLds", "cholLL", "bigLoad", "bigChain", "sbBack")
FIELDS = (("chainMode", "chainOverflow", "route", "dSolve", "dpad", "border", "dp", "nb", "n", "dK", "ldY", "rowsY", "ldOut", "dpK", "batched")
          + tuple(r + s for r in REGIONS for s in ("_off", "_len")) + ("end",)
          + tuple(l + s for l in LAUNCHES for s in ("_grid", "_lds")) + ("helperTasks", "nBackPanels", "bigBackLds"))
CONSTANTS = ("kNB", "kBackSpan", "kCholLdsMaxTiles", "kBorderMaxRows", "kBorderScratchDoubles", "kSbRec", "kSbFlo", "kSbFhi",
             "kSbMaxChain", "kSbCols")
# what the fixture records of a row (tests/golden/solve_plan.npz)
RECORDED = ("chainMode", "route", "border", "dp", "Lf_off", "Y_off", "tvec_off", "compactS_off", "compactG_off")


def sweep():
    """dC = 0, 6, ..., 2394 x chain length 0 ... 69 with d = dC + 9 n: unpadded and padded S without a switch, then each switch
    alone on the padded S -- 140 000 rows"""
    dC, n = np.meshgrid(np.arange(0, 2400, 6), np.arange(70), indexing="ij")
    dC, n = dC.ravel(), n.ravel()
    parts = []
    for padded, switches in ((0, 0), (1, 0), (1, NO_LL), (1, NO_SB_ELIM), (1, NO_LDS_BORDER)):
        parts.append(np.stack([dC + 9 * n, dC, n, np.full_like(n, padded), np.full_like(n, switches)], axis=1))
    return np.ascontiguousarray(np.concatenate(parts), np.int32)


def build_shim(directory):
    so = os.path.join(str(directory), "libsp.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "solve_plan_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.sp_plan.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.sp_plan.restype = None
    lib.sp_scratch_doubles.restype = C.c_int64
    lib.sp_back_panel.argtypes = [C.c_int, C.c_int, C.c_void_p]
    assert lib.sp_fields() == len(FIELDS)
    return lib


def plan(lib, rows):
    """rows: (k, 5) integers -> {field: int64 array of k}"""
    rows = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 5))
    out = np.zeros((len(rows), len(FIELDS)), np.int64)
    lib.sp_plan(len(rows), rows.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return {name: out[:, k] for k, name in enumerate(FIELDS)}


def plan_one(lib, d, dC=None, n=0, padded=1, switches=0):
    q = plan(lib, [[d, d - 9 * n if dC is None else dC, n, padded, switches]])
    return {k: int(v[0]) for k, v in q.items()}


def scratch_doubles(lib, d, with_chain):
    return int(lib.sp_scratch_doubles(int(d), 1 if with_chain else 0))


def back_panel(lib, dp, k):
    out = (C.c_int * 4)()
    lib.sp_back_panel(dp, k, out)
    return dict(zip(("c0", "c1", "blocks", "nChunks"), list(out)))


def constants(lib):
    return {name: lib.sp_constant(k) for k, name in enumerate(CONSTANTS)}
