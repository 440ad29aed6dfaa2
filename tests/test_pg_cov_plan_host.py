"""The host planning of the pose graph's covariance pass (svin_amd/csrc/pg_cov_plan.hpp through tests/csrc/pg_cov_plan_shim.cpp) on
the CPU: the column keyframe of a pair is the later one whichever way the pair is asked, constant keyframes give zero pairs and no
column, B - 1 / B / B + 1 / 2B + 1 column keyframes make 1 / 1 / 2 / 3 batches with every pair in exactly one of them, a batch's
forward pieces are those of its column keyframes and its backward pieces those of its row keyframes, and the piece kernels' LDS
stays within a workgroup's 160 KiB at the widest bands the solver builds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("pgcovplan")), "libpgcp.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "pg_cov_plan_shim.cpp"), "-o", so])
    L = C.CDLL(so)
    L.pgcp_constant.restype = C.c_int64
    L.pgcp_piece_lds.restype = C.c_int64
    L.pgcp_plan.restype = C.c_int64
    ip = C.POINTER(C.c_int)
    L.pgcp_plan.argtypes = [C.c_int, ip, ip, ip, ip, C.c_int, C.c_void_p, C.c_int64]
    return L


def plan(lib, pairs, off, node_piece, n_pieces):
    ip = C.POINTER(C.c_int)
    la = np.ascontiguousarray([a for a, _ in pairs], np.int32)
    lb = np.ascontiguousarray([b for _, b in pairs], np.int32)
    off = np.ascontiguousarray(off, np.int32)
    npc = np.ascontiguousarray(node_piece, np.int32)
    args = (len(pairs), la.ctypes.data_as(ip), lb.ctypes.data_as(ip), off.ctypes.data_as(ip), npc.ctypes.data_as(ip), n_pieces)
    need = lib.pgcp_plan(*args, None, 0)
    o = np.zeros(need, np.int64)
    assert lib.pgcp_plan(*args, o.ctypes.data_as(C.c_void_p), need) == need
    it = iter(o.tolist())

    def lst():
        return [next(it) for _ in range(next(it))]
    out = dict(zero=lst(), columns=lst(), batches=[])
    for _ in range(next(it)):
        b = dict(slots=lst())
        b["pairs"] = [tuple(next(it) for _ in range(4)) for _ in range(next(it))]
        b["fwd"], b["active"], b["back"] = lst(), lst(), lst()
        out["batches"].append(b)
    assert next(it, None) is None
    return out


def chain(nn=60, piece=10):
    """node 0 constant; every `piece`-th free keyframe a separator, the others interior keyframes of the piece before it"""
    off = [-1] + [4 * k for k in range(nn - 1)]
    node_piece = [-1] + [(-1 if k % piece == 0 else k // piece) for k in range(1, nn)]
    return off, node_piece, max(node_piece) + 1


def test_constants(lib):
    assert lib.pgcp_constant(0) >= 8 and lib.pgcp_constant(1) % 64 == 0 and lib.pgcp_constant(2) == 160 * 1024


def test_later_keyframe_is_the_column(lib):
    off, npc, np_ = chain()
    q = plan(lib, [(5, 17), (17, 5), (9, 9), (0, 9), (9, 0)], off, npc, np_)
    assert q["zero"] == [3, 4] and q["columns"] == [9, 17] and len(q["batches"]) == 1
    b = q["batches"][0]
    assert b["slots"] == [9, 17]
    assert sorted(b["pairs"]) == [(0, 5, 1, 0), (1, 5, 1, 1), (2, 9, 0, 0)]      # (pair, row keyframe, slot, transposed)
    assert b["fwd"] == sorted({npc[9], npc[17]}) and b["back"] == sorted({npc[5], npc[9]})
    assert [i for i, a in enumerate(b["active"]) if a] == b["fwd"]


def test_separator_columns_touch_no_piece(lib):
    off, npc, np_ = chain()
    q = plan(lib, [(10, 20)], off, npc, np_)
    assert q["batches"][0]["fwd"] == [] and q["batches"][0]["back"] == [] and not any(q["batches"][0]["active"])


def test_dense_regime(lib):
    off = [-1] + [6 * k for k in range(20)]
    q = plan(lib, [(a, 20) for a in range(21)], off, [-1] * 21, 0)
    assert q["zero"] == [0] and q["columns"] == [20] and q["batches"][0]["fwd"] == [] and q["batches"][0]["back"] == []
    assert len(q["batches"][0]["pairs"]) == 20


@pytest.mark.parametrize("extra", [-1, 0, 1, None])
def test_batch_edges(lib, extra):
    B = lib.pgcp_constant(0)
    ncol = 2 * B + 1 if extra is None else B + extra
    off, npc, np_ = chain(nn=4 * B + 8)
    cols = list(range(3, 3 + ncol))
    pairs = [(1, c) for c in cols] + [(c, c) for c in cols]
    q = plan(lib, pairs, off, npc, np_)
    assert q["columns"] == cols and len(q["batches"]) == -(-ncol // B)
    seen = []
    for k, b in enumerate(q["batches"]):
        assert b["slots"] == cols[k * B:(k + 1) * B] and 1 <= len(b["slots"]) <= B
        for pair, row, slot, tr in b["pairs"]:
            assert b["slots"][slot] == pairs[pair][1] and row == pairs[pair][0] and tr == 0
            seen.append(pair)
        assert b["fwd"] == sorted({npc[c] for c in b["slots"] if npc[c] >= 0})
    assert sorted(seen) == list(range(len(pairs)))


def test_lds_of_the_piece_kernels(lib):
    B, cap = lib.pgcp_constant(0), lib.pgcp_constant(2)
    # (D, w): level 1 reaches w keyframes, level 2 2w - 1; a piece has at most 256 rows
    for D, w in ((4, 2), (6, 4)):
        for reach in (w, 2 * w - 1):
            BW = reach * D + D - 1
            lds = lib.pgcp_piece_lds(256, BW, B * D)
            assert lds == (256 + B * D) * (BW + 1) * 8 and lds <= cap and lib.pgcp_piece_fits(256, BW, B * D) == 1
    assert lib.pgcp_piece_fits(256, 80, 6 * B) == 0
