"""The host planning of a batched solve (svin_amd/csrc/batch_plan.hpp, driven by Window::solvePreparedBatch) on the CPU.

Windows share a launch sequence when they agree in what the launcher computes once per launch (reduced system, factors, prior,
cameras); the landmark and observation counts only decide how many blocks of each launch a window owns.  Checked here: the
group key ignores exactly those counts, the lane cut is a partition of the size-sorted group into contiguous non-empty runs, a
lane's grid is the largest extent among its windows, and a window's extents are the grids the single-window launchers take
(launchAccumulateNormalEquations, launchDoglegPrepare, launchDoglegStep, launchEvalAll -- restated below from their definitions)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL, REUSE, EVAL = 1, 2, 4
KEY = ("d", "dC", "dCPose", "F", "nPose", "nExt", "nSb", "priorM", "anyExtVariable", "ldS", "sPadded", "priorBlocks", "nCam", "schurDense")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bp") / "libbp.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "batch_plan_shim.cpp"), "-o", so])
    return C.CDLL(so)


def ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def dims(L, N, F=11, nPose=6, nExt=2, nSb=6, priorM=0, owns=1, nSlabs=None):
    return [L, N, F, nPose, nExt, nSb, priorM, owns, max(1, min(256, -(-L // 16))) if nSlabs is None else nSlabs]


def extents(lib, d):
    out = (C.c_int * 12)()
    lib.bp_extents(ints(d), out)
    return dict(zip(("buildSlabs", "buildFac", "buildPri", "postLm", "postFac", "step", "evalR", "evalF", "evalPri", "build", "post", "evalRest"), list(out)))


def single_window_grids(L, N, F, nPose, nExt, nSb, priorM):
    """gridDim.x of the launches of ONE window (dense Schur form, prior on this rank), as the launchers compute them"""
    ceil = lambda a, b: -(-a // b)
    n_slabs = max(1, min(256, ceil(L, 16)))                      # Window::pack, dense form
    n_pri = ceil(priorM * priorM, 256) if priorM > 0 else 0      # priorAccBlocks
    n_lm = min(ceil(L, 16), 1024) if (L > 0 and N > 0) else 0    # launchDoglegPrepare
    n_fac_p = min(ceil(F, 4), 1024) if F > 0 else 0
    return dict(buildSlabs=n_slabs, build=n_slabs + F + n_pri, postLm=n_lm, postFac=n_fac_p, post=n_lm + n_fac_p + 1,
                step=ceil(nPose + nExt + nSb + L, 256),          # launchDoglegStep
                evalR=ceil(N, 256), evalRest=F + (1 if priorM > 0 else 0))   # launchEvalAll (split form)


def test_group_key_ignores_the_counts_and_nothing_else(lib):
    assert lib.bp_key_fields() == len(KEY)
    base = [105, 60, 48, 11, 10, 2, 5, 24, 1, 112, 1, 3, 2, 1]
    # the key holds no landmark or observation count at all: two windows of one fleet are one group whatever the front end found
    assert lib.bp_same_group(ints(base), ints(list(base))) == 1
    for k, name in enumerate(KEY):
        for delta in (1, -1):
            other = list(base)
            other[k] += delta
            assert lib.bp_same_group(ints(base), ints(other)) == 0, name
            assert lib.bp_same_group(ints(other), ints(base)) == 0, name


L_EDGES = [1, 15, 16, 17, 90, 120, 250, 330, 399, 400, 401, 1990, 2010, 4096, 4097, 16368]
N_EDGES = [1, 128, 129, 255, 256, 257, 2560, 2561, 20000, 163840]


@pytest.mark.parametrize("F,priorM", [(11, 0), (9, 15), (1, 16), (12, 17), (4097, 96), (5000, 0)])
def test_extents_are_the_single_window_grids(lib, F, priorM):
    for L, N in itertools.product(L_EDGES, N_EDGES):
        for nPose, nExt, nSb in ((6, 2, 6), (10, 0, 5), (3, 1, 1)):
            got = extents(lib, dims(L, N, F, nPose, nExt, nSb, priorM))
            ref = single_window_grids(L, N, F, nPose, nExt, nSb, priorM)
            assert {k: got[k] for k in ref} == ref, (L, N, F, priorM, nPose, nExt, nSb)
            assert lib.bp_slab_count(L) == ref["buildSlabs"]
            # the parts add up to the grids, the factor blocks are one per factor, the tail block is the post-solve pass's last
            assert got["build"] == got["buildSlabs"] + got["buildFac"] + got["buildPri"] and got["buildFac"] == F
            assert got["post"] == got["postLm"] + got["postFac"] + 1
            assert got["evalRest"] == got["evalF"] + got["evalPri"] and got["evalF"] == F
    # the table block crosses a multiple of 256 with the landmark count alone
    assert extents(lib, dims(242, 2420))["step"] == 1 and extents(lib, dims(243, 2430))["step"] == 2
    # a rank that does not own the prior accumulates none of it; a window without observations has no landmark blocks
    assert extents(lib, dims(100, 1000, priorM=24, owns=0))["buildPri"] == 0
    assert extents(lib, dims(100, 0))["postLm"] == 0
    # SVIN_SLAB_CHUNKS: the slab count is the window's own field, not recomputed
    assert extents(lib, dims(1000, 10000, nSlabs=16))["buildSlabs"] == 16


def plan(lib, L, N, max_lanes):
    n = len(L)
    order, first, count = (C.c_int * n)(), (C.c_int * max(1, max_lanes))(), (C.c_int * max(1, max_lanes))()
    k = lib.bp_plan_lanes(n, ints(L), ints(N), max_lanes, order, first, count)
    return list(order), [(first[i], count[i]) for i in range(k)]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 16, 33, 64])
@pytest.mark.parametrize("max_lanes", [1, 2, 4])
def test_lane_cut_is_a_contiguous_partition_of_the_sorted_group(lib, n, max_lanes):
    rng = np.random.default_rng(100 * n + max_lanes)
    L = rng.integers(1600, 2401, n)
    N = 10 * L + rng.integers(-300, 300, n)
    order, lanes = plan(lib, L, N, max_lanes)
    assert sorted(order) == list(range(n))                                     # every window once
    keys = [(-(-int(L[i]) // 16), -(-int(N[i]) // 256)) for i in order]
    assert keys == sorted(keys)                                                # (landmark chunks, observation blocks) ascending
    assert len(lanes) == max(1, min(max_lanes, n // 2))                        # a lane has partners: at least two windows
    assert lanes[0][0] == 0 and all(c >= 1 for _, c in lanes)                  # never an empty lane
    assert all(lanes[k][0] + lanes[k][1] == lanes[k + 1][0] for k in range(len(lanes) - 1)) and lanes[-1][0] + lanes[-1][1] == n
    assert max(c for _, c in lanes) - min(c for _, c in lanes) <= 1            # dealt evenly


def test_equal_sizes_keep_the_order_of_the_call(lib):
    """windows of one size are dealt exactly as before there were sizes: lane k takes positions [B k / n, B (k + 1) / n)"""
    order, lanes = plan(lib, [2000] * 16, [20000] * 16, 4)
    assert order == list(range(16)) and lanes == [(0, 4), (4, 4), (8, 4), (12, 4)]
    # same chunk and block counts, different raw counts: still equal for the sort (the grids are equal)
    order, _ = plan(lib, [2000, 1999, 1998, 1997], [20000, 19990, 19980, 19970], 2)
    assert order == [0, 1, 2, 3]
    order, lanes = plan(lib, [2400, 1600, 2000, 1700, 2300], [24000, 16000, 20000, 17000, 23000], 4)
    assert order == [1, 3, 2, 4, 0] and lanes == [(0, 2), (2, 3)]


def test_a_lane_grid_is_the_largest_extent_of_the_windows_taking_part(lib):
    ws = [dims(90, 900), dims(2400, 24000), dims(400, 5000), dims(401, 2561)]
    ex = [extents(lib, w) for w in ws]

    def grid(stages):
        out = (C.c_longlong * 7)()
        lib.bp_lane_grid(len(ws), ints([x for w in ws for x in w]), ints(stages), out)
        return list(out)

    g = grid([FULL | EVAL] * 4)
    assert g[:5] == [max(e["build"] for e in ex), max(e["post"] for e in ex), 0, max(e["evalR"] for e in ex), max(e["evalRest"] for e in ex)]
    assert g[5] == g[0] + g[1] + g[3] + g[4]
    assert g[6] == sum(e["build"] + e["post"] + e["evalR"] + e["evalRest"] for e in ex) and g[6] < 4 * g[5]
    # the largest window sits the build out (rejected step: k_step_retract) and one has terminated: they do not size the build
    g = grid([FULL | EVAL, REUSE | EVAL, 0, FULL | EVAL])
    assert g[0] == max(ex[0]["build"], ex[3]["build"]) and g[1] == max(ex[0]["post"], ex[3]["post"])
    assert g[2] == ex[1]["step"] and g[3] == ex[1]["evalR"]
    assert g[6] == ex[0]["build"] + ex[0]["post"] + ex[3]["build"] + ex[3]["post"] + ex[1]["step"] + sum(ex[i]["evalR"] + ex[i]["evalRest"] for i in (0, 1, 3))
    # the initial evaluation: nothing but the two evaluation launches
    g = grid([EVAL] * 4)
    assert g[:3] == [0, 0, 0] and g[5] == g[3] + g[4]
    # windows of one size: no block is idle
    same = [dims(2000, 20000)] * 4
    out = (C.c_longlong * 7)()
    lib.bp_lane_grid(4, ints([x for w in same for x in w]), ints([FULL | EVAL] * 4), out)
    assert out[6] == 4 * out[5]
