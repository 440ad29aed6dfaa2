"""The tile skyline of the reduced system (svin_amd/csrc/pack_plan.hpp planTileSkyline through tests/csrc/tile_skyline_shim.cpp),
a numpy reference for it -- the boolean entry pattern of S from the same block lists, a dense symbolic Cholesky entry by entry,
then each tile column's last non-zero tile row -- and the block lists of the windows the tests run over.  Shared by
tests/test_tile_skyline_host.py (CPU) and tests/test_gpu_chol_skyline.py.

A system is (d, dC, cliques): rows < dC are the camera part (dense), a clique is the list of (row offset, rows) of the variable
blocks one factor -- or the prior -- couples pairwise."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MAX_TILES = 11


def build_shim(directory):
    so = os.path.join(str(directory), "libts.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "tile_skyline_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.ts_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ts_hi_of.argtypes = [C.c_uint64, C.c_int, C.c_int]
    assert lib.ts_max_tiles() == MAX_TILES
    return lib


def _flat(cliques):
    ptr, off, length = [0], [], []
    for cl in cliques:
        for o, n in cl:
            off.append(o)
            length.append(n)
        ptr.append(len(off))
    return (np.asarray(ptr, np.int32), np.asarray(off + [0], np.int32), np.asarray(length + [0], np.int32))


def plan(lib, d, dC, cliques, recognised=True):
    """-> dict(nT, hi, pre, cut, cutPre): the profile the factorisation keeps, the one the build may write, and both as the
    words DeviceProblem carries"""
    ptr, off, length = _flat(cliques)
    hi, pre, cut = np.zeros(MAX_TILES, np.int32), np.zeros(MAX_TILES, np.int32), np.zeros(2, np.uint64)
    nT = lib.ts_plan(d, dC, len(cliques), ptr.ctypes.data, off.ctypes.data, length.ctypes.data, 1 if recognised else 0,
                     hi.ctypes.data, pre.ctypes.data, cut.ctypes.data)
    n = nT if nT <= MAX_TILES else 0
    return dict(nT=nT, hi=[int(v) for v in hi[:n]], pre=[int(v) for v in pre[:n]], cut=int(cut[0]), cutPre=int(cut[1]))


def unpack(cut, nT):
    """hi[k] from the packed word (four bits per tile column: nT - 1 - hi[k])"""
    return [nT - 1 - ((int(cut) >> (4 * k)) & 15) for k in range(nT)]


def case_text(d, dC, cliques, recognised=True):
    """one line of the sanitizer program's input (tests/csrc/tile_skyline_sanitize.cpp)"""
    words = [d, dC, 1 if recognised else 0, len(cliques)]
    for cl in cliques:
        words.append(len(cl))
        for o, n in cl:
            words += [o, n]
    return " ".join(str(w) for w in words)


def pattern(d, dC, cliques):
    """boolean entry pattern (dpad x dpad, symmetric) of S: the camera part, every clique, the diagonal (identity padding)"""
    n = (d + 15) // 16 * 16
    A = np.eye(n, dtype=bool)
    A[:dC, :dC] = True
    for cl in cliques:
        rows = np.concatenate([np.arange(o, o + m) for o, m in cl]) if cl else np.zeros(0, int)
        A[np.ix_(rows, rows)] = True
    return A


def tile_profile(A):
    """last non-zero tile row of every tile column of the lower triangle"""
    n = A.shape[0]
    low = np.tril(A)
    hi = []
    for J in range(n // 16):
        rows = np.nonzero(low[:, 16 * J:16 * J + 16].any(axis=1))[0]
        hi.append(int(rows.max()) // 16)
    return hi


def reference(d, dC, cliques):
    """-> (pre, hi): tile profiles of the pattern of S and of its Cholesky factor (dense symbolic factorisation, entry by entry)"""
    A = pattern(d, dC, cliques)
    pre = tile_profile(A)
    Lp = np.tril(A).copy()
    for k in range(A.shape[0]):
        rows = np.nonzero(Lp[k + 1:, k])[0] + k + 1
        if len(rows):
            Lp[np.ix_(rows, rows)] |= np.tril(np.ones((len(rows), len(rows)), bool))
    return pre, tile_profile(Lp)


def window(P, fixed_poses=(), fixed_sb=(), ext_per_frame=False, prior_first=0, prior_all=False, extra=()):
    """Block lists of a window of P frames as the estimator builds it: variable poses (6 rows) first, then per-frame extrinsics
    (6, when asked for), then speed / bias blocks (9), each in frame order; IMU factor b couples pose b, speed / bias b, pose b + 1,
    speed / bias b + 1; the first frame carries a pose and a speed / bias prior; consecutive extrinsics are tied pairwise.
    prior_first = k: a marginalisation prior over the first k blocks in row order; prior_all: over every block.
    extra: further cliques of block names ("p3", "s7", "e0").  -> (d, dC, cliques, offsets by name)"""
    off, d = {}, 0
    for b in range(P):
        if b not in fixed_poses:
            off["p%d" % b] = (d, 6)
            d += 6
    if ext_per_frame:
        for b in range(P):
            off["e%d" % b] = (d, 6)
            d += 6
    dC = d
    for b in range(P):
        if b not in fixed_sb:
            off["s%d" % b] = (d, 9)
            d += 9
    names = []
    for b in range(P - 1):
        names.append(["p%d" % b, "s%d" % b, "p%d" % (b + 1), "s%d" % (b + 1)])
    names += [["p0"], ["s0"]]
    if ext_per_frame:
        names += [["e%d" % b, "e%d" % (b + 1)] for b in range(P - 1)] + [["e0"]]
    names += [list(e) for e in extra]
    order = sorted(off, key=lambda k: off[k][0])
    if prior_all:
        names.append(order)
    elif prior_first:
        names.append(order[:prior_first])
    cliques = [[off[n] for n in cl if n in off] for cl in names]
    return d, dC, cliques, off
