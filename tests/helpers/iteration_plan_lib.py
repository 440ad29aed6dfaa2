"""ctypes access to the accumulator ledger and the plan of a pass of Window::solve (svin_amd/csrc/iteration_plan.hpp through
tests/csrc/iteration_plan_shim.cpp).  Shared by tests/test_iteration_plan_host.py and tests/test_gpu_solve_loop.py."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIELDS = ("alive", "reuse", "mu", "initScale", "iteration", "solve", "launch", "zeroFirst", "allReduceSystem", "prepareRadius", "stepInEval",
          "lmDeferredPost", "doglegStep", "lmDeferredEval", "specWanted", "specMu", "specInEval", "specFused", "end", "hitsIfClosed",
          "missesIfClosed", "stepRadius", "batchStages")
RETRY, TERMINATED, ACCEPTED, REJECTED, INVALID = range(5)   # PassEnd
ZERO, BUILD, STALE = range(3)                               # AccumulatorLedger::Contents
ONE_GPU, NATIVE, CALLBACK, BATCHED = range(4)               # mode; BATCHED: a window of a batched solve
BATCH_FULL, BATCH_REUSE, BATCH_EVAL = 1, 2, 4               # batch_plan.hpp: stages of a round


def build_shim(directory):
    so = os.path.join(str(directory), "libip.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "iteration_plan_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.ip_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.ip_run_all.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.ip_run_all.restype = None
    lib.ip_need.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p]
    lib.ip_need.restype = None
    lib.ip_replay.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.ip_replay.restype = None
    lib.ip_batch_stages.argtypes = [C.c_void_p, C.c_double, C.c_int]
    assert lib.ip_fields() == len(FIELDS)
    return lib


def replay(lib, log, strategy, no_speculation, num_iter, initial_radius=1e4, max_radius=1e16, terminated_pass=False):
    """(hits, misses, passes) of the solve on one GPU that wrote the iteration log"""
    cfg = np.array([1 if strategy == "lm" else 0, int(no_speculation), 0, ONE_GPU, num_iter, 0], np.int32)
    log = np.ascontiguousarray(np.asarray(log, float).reshape(-1, 6))
    out = np.zeros(3, np.int32)
    lib.ip_replay(cfg.ctypes.data_as(C.c_void_p), initial_radius, max_radius, len(log), log.ctypes.data_as(C.c_void_p), int(terminated_pass),
                  out.ctypes.data_as(C.c_void_p))
    return int(out[0]), int(out[1]), int(out[2])
