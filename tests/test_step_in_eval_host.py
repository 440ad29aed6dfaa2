"""stepInEvalTaken (svin_amd/csrc/build_plan.hpp) on the CPU: when the dogleg step of an iteration leaves the tail of k_post_solve
for the head of k_eval_build's blocks.

A wrong "yes" is a post-solve pass that ends at its partials with nothing behind it to take the step (Window::solve throws), or a
head whose scratch runs over a block's LDS; a wrong "no" only keeps the old pair of launches.  Starting from the benchmark's narrow
window, where the pair is taken, every input that flips the decision is flipped alone -- the last iteration of a solve and a
re-used linearisation among them, the two situations in which Window::solve keeps the tail."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMERA_MODEL_BYTES, FACTOR_SHARED_BYTES = 120, 133584   # sizeof(CameraModel), sizeof(FactorShared) (tests/golden/build_plan.npz "sizes")

NAMES = ("dC", "dCPose", "anyExtVariable", "L", "N", "F", "priorM", "ownsCamera", "nPose", "nExt", "nCam", "nSb", "d", "stepSwitches",
         "sharded", "noSpeculation", "iteration", "numIter", "reuse", "hostFactors", "noStepInEval", "noEvalBuild", "computeUnits", "slabChunks")
# ten keyframes, 2 000 landmarks, 20 000 observations, nine IMU factors, the third of ten iterations, 256 compute units
BENCH = dict(dC=60, dCPose=60, anyExtVariable=0, L=2000, N=20000, F=9, priorM=0, ownsCamera=1, nPose=10, nExt=2, nCam=2, nSb=10, d=150,
             stepSwitches=0, sharded=0, noSpeculation=0, iteration=3, numIter=10, reuse=0, hostFactors=0, noStepInEval=0, noEvalBuild=0,
             computeUnits=256, slabChunks=0)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sie")), "libsie.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "step_in_eval_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.sie_decide.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    lib.sie_raw.argtypes = [C.c_void_p, C.c_void_p]
    return lib


def decide(lib, **change):
    unknown = set(change) - set(NAMES)
    assert not unknown, unknown
    row = np.array([dict(BENCH, **change)[n] for n in NAMES], np.int32)
    return lib.sie_decide(row.ctypes.data_as(C.c_void_p), CAMERA_MODEL_BYTES, FACTOR_SHARED_BYTES)


RAW = ("chosenForm", "sharded", "buildWanted", "evalBuildTaken", "reuse", "hostFactors", "noStepInEval", "d", "items", "nPost", "postSplit")
RAW_YES = dict(chosenForm=3, sharded=0, buildWanted=1, evalBuildTaken=1, reuse=0, hostFactors=0, noStepInEval=0, d=150, items=22, nPost=129, postSplit=0)
RAW_LDS = dict(evalStageBytes=1800, chunkLdsBytes=34048, stageBytes=1152, factorSharedBytes=FACTOR_SHARED_BYTES)


def raw(lib, **change):
    unknown = set(change) - set(RAW) - set(RAW_LDS)
    assert not unknown, unknown
    a = np.array([dict(RAW_YES, **change)[n] for n in RAW], np.int32)
    b = np.array([dict(RAW_LDS, **change)[n] for n in RAW_LDS], np.int64)
    return lib.sie_raw(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))


def test_the_benchmark_window_takes_the_pair(lib):
    assert decide(lib) == 1
    assert decide(lib, iteration=1) == 1 and decide(lib, iteration=9) == 1
    assert decide(lib, priorM=30) == 1     # (the prior's block takes the head as well)


@pytest.mark.parametrize("change", [
    dict(iteration=10),                    # the last iteration of a solve: no build behind it, k_eval_all follows
    dict(numIter=3),                       # the same, seen from the other side
    dict(reuse=1),                         # a re-used linearisation: k_step_retract takes the step
    dict(sharded=1),
    dict(noSpeculation=1),                 # SVIN_NO_SPECULATION: no build behind the candidate evaluation
    dict(noEvalBuild=1),                   # SVIN_NO_EVAL_BUILD
    dict(noStepInEval=1),                  # SVIN_NO_STEP_IN_EVAL
    dict(hostFactors=1),                   # the host reads the candidate blocks in front of the evaluation's launch
    dict(stepSwitches=1),                  # SVIN_SPLIT_EVAL: form 1
    dict(stepSwitches=2),                  # SVIN_NO_FUSE_STEP: form 2
    dict(stepSwitches=4),                  # SVIN_NO_DEFER_LM: form 1
    dict(computeUnits=64),                 # k_eval_build declines: more workgroups than compute units
    dict(anyExtVariable=1, dC=72),         # variable extrinsics: not k_eval_build's form
    dict(F=0),                             # nothing to fuse the evaluation with
    dict(nSb=90, d=870),                   # more parameter blocks than one pass of a workgroup retracts
    dict(d=1025),                          # y_C and v_C no longer staged
], ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_each_input_alone_keeps_the_tail(lib, change):
    assert decide(lib) == 1
    assert decide(lib, **change) == 0


def test_a_pass_of_more_than_512_blocks_keeps_its_tail(lib):
    """SVIN_SLAB_CHUNKS=3 brings a window of 511 landmark blocks to k_eval_build (171 chunk blocks beside 72 evaluation blocks);
    its post-solve pass is k_post_solve_wide, which has no form without a tail"""
    wide = dict(L=8176, N=16000, slabChunks=3)
    assert decide(lib, L=8000, N=16000, slabChunks=3) == 1     # 500 landmark blocks: the narrow pass
    assert decide(lib, **wide) == 0
    assert decide(lib, L=4080, N=8200, slabChunks=2) == 1      # 255 landmark blocks, 128 chunk blocks: the partials' second trip


def test_the_predicate_input_by_input(lib):
    assert raw(lib) == 1
    for change in (dict(chosenForm=1), dict(chosenForm=2), dict(sharded=1), dict(buildWanted=0), dict(evalBuildTaken=0), dict(reuse=1),
                   dict(hostFactors=1), dict(noStepInEval=1), dict(d=0), dict(items=0), dict(nPost=0), dict(postSplit=1)):
        assert raw(lib, **change) == 0, change


def test_the_staging_limits_are_the_tails(lib):
    max_d, max_items, max_partials, red, head150 = (lib.sie_constant(k) for k in range(5))
    assert (max_d, max_items, max_partials, red) == (1024, 96, 4096, 16 * 9 + 8) and head150 == (red + 300) * 8
    assert raw(lib, d=max_d) == 1 and raw(lib, d=max_d + 1) == 0
    assert raw(lib, items=max_items) == 1 and raw(lib, items=max_items + 1) == 0
    assert raw(lib, nPost=max_partials) == 1 and raw(lib, nPost=max_partials + 1) == 0


def test_the_heads_scratch_fits_behind_the_tables(lib):
    head = (16 * 9 + 8 + 2 * 150) * 8
    room = FACTOR_SHARED_BYTES - head
    # a reprojection block: reduction scratch, tables, then the head
    assert raw(lib, evalStageBytes=room) == 1 and raw(lib, evalStageBytes=room + 8) == 0
    # a chunk block: tiles (rounded up to 16 bytes), tables, then the head
    assert raw(lib, chunkLdsBytes=room - 1152) == 1 and raw(lib, chunkLdsBytes=room - 1152 + 8) == 0
    assert raw(lib, chunkLdsBytes=room - 1152 - 8) == 1
    assert raw(lib, chunkLdsBytes=0, stageBytes=room) == 1 and raw(lib, chunkLdsBytes=0, stageBytes=room + 8) == 0
