"""Inputs for, and ctypes access to, the host planning of Window::pack (svin_amd/csrc/pack_plan.hpp through
tests/csrc/pack_plan_shim.cpp).  Shared by tests/test_pack_plan_host.py and tests/golden/make_golden_pack_plan.py.

An input is what pack() hands the planner: the landmark-major CSR (lmPtr), the packed observation indices (pose slot in bits
0-11, extrinsics slot << 12, camera << 24) and the pose slot -> reduced-row table (poseOff, -1 for a fixed pose)."""
import ctypes as C
import os
import subprocess
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CONSTANTS = ("kBlkMinWordsPerBlock", "kBlkWaves", "kBlkBatchRecs", "kBlkBatchWords", "kBlkRec", "kBlkSlotsPerWorkgroup",
             "kBlkMaxPoseBlocks", "kPanelChunksPerBlock", "kDensePoseCap")
SLOT_ARRAYS = ("slotPtr", "slotBlk", "slotObsPtr", "slotObs", "slotLm")
ROWS_ARRAYS = ("pairWords", "batch", "waveTab", "recSlot", "panelWork", "blkOwn", "panelPairPtr", "counts", "balance")
PANELS_ARRAYS = ("panelWork", "panelChunks", "panelPairPtr", "counts")


@dataclass
class PlanInput:
    lmPtr: np.ndarray     # int32, L + 1
    obsIdx: np.ndarray    # uint32, N
    poseOff: np.ndarray   # int32, pose slots
    dC: int

    @property
    def L(self):
        return len(self.lmPtr) - 1


def _assemble(tracks, pose_off):
    """tracks: per landmark the list of (pose slot, camera) in insertion order"""
    ptr, idx = [0], []
    for tr in tracks:
        idx += [p | (cam << 24) for p, cam in tr]
        ptr.append(len(idx))
    pose_off = np.asarray(pose_off, np.int32)
    return PlanInput(np.asarray(ptr, np.int32), np.asarray(idx, np.uint32), pose_off, int(pose_off.max()) + 6)


def pose_offsets(n_slots, fixed=()):
    off, d = [], 0
    for i in range(n_slots):
        if i in fixed:
            off.append(-1)
        else:
            off.append(d)
            d += 6
    return off


def input_a(seed=1, n_lm=600):
    """43 variable pose blocks (dC = 258: three panels, the last with 11 blocks) among 45 pose slots, two of them fixed (about
    5 % of the observations); every landmark seen by 2..9 poses inside a span of 28, in no particular order, about a third of
    the observations stereo (a second observation on the same pose); ten landmarks seen by the fixed poses alone"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_slots, fixed = 45, (7, 30)
    tracks = []
    for l in range(n_lm):
        if l % 60 == 17:   # ten of 600: no variable pose at all
            tracks.append([(7, 0), (30, 0), (30, 1)])
            continue
        first = int(rng.integers(0, n_slots - 1))
        span = np.arange(first, min(first + 28, n_slots))
        k = min(int(rng.integers(2, 10)), len(span))
        tr = []
        for p in rng.permutation(span)[:k]:
            tr.append((int(p), 0))
            if rng.random() < 1.0 / 3.0:
                tr.append((int(p), 1))
        tracks.append(tr)
    return _assemble(tracks, pose_offsets(n_slots, fixed))


def input_b():
    """48 pose blocks (three full panels), 64 landmarks each seen from all 48 poses: an entry carries 16 + 16 records and 32 words
    per wave, so batches end at the word limit"""
    return _assemble([[(p, 0) for p in range(48)] for _ in range(64)], pose_offsets(48))


def input_c(seed=3, n_lm=3000):
    """49 pose blocks (four panels, the last with one block), landmarks seen from exactly two poses in different panels: batches
    end at the record limit"""
    rng = np.random.Generator(np.random.PCG64(seed))
    tracks = []
    for _ in range(n_lm):
        pa, pb = rng.choice(4, 2, replace=False)
        a = 48 if pa == 3 else 16 * int(pa) + int(rng.integers(0, 16))
        b = 48 if pb == 3 else 16 * int(pb) + int(rng.integers(0, 16))
        tracks.append([(a, 0), (b, 0)])
    return _assemble(tracks, pose_offsets(49))


# ------------------------------------------------------------------------------------------------ the shim
def build_shim(directory):
    so = os.path.join(str(directory), "libpp.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "pack_plan_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    for name in ("pp_slots", "pp_rows", "pp_panels"):
        getattr(lib, name).restype = C.c_void_p
    for name in ("pp_count", "pp_len", "pp_get", "pp_free"):
        getattr(lib, name).argtypes = [C.c_void_p] + {"pp_count": [], "pp_len": [C.c_int], "pp_get": [C.c_int, C.c_void_p], "pp_free": []}[name]
    return lib


def _i32(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data_as(C.c_void_p)


def _take(lib, handle, names):
    assert lib.pp_count(handle) == len(names)
    out = {}
    for k, name in enumerate(names):
        a = np.zeros(lib.pp_len(handle, k), np.int32)
        lib.pp_get(handle, k, a.ctypes.data_as(C.c_void_p))
        out[name] = a
    lib.pp_free(handle)
    return out


def _csr_args(inp):
    ptr, pp = _i32(inp.lmPtr)
    idx = np.ascontiguousarray(inp.obsIdx, np.uint32)
    off, po = _i32(inp.poseOff)
    return (ptr, idx, off), (inp.L, pp, idx.ctypes.data_as(C.c_void_p), len(idx), po, len(off))


def constants(lib):
    return {name: lib.pp_constant(k) for k, name in enumerate(CONSTANTS)}


def slots(lib, inp):
    keep, args = _csr_args(inp)
    return _take(lib, lib.pp_slots(*args), SLOT_ARRAYS)


def rows(lib, inp, compute_units, row_split, rounds=0):
    keep, args = _csr_args(inp)
    out = _take(lib, lib.pp_rows(*args, inp.dC, compute_units, rounds, 1 if row_split else 0), ROWS_ARRAYS)
    out["pairWords"] = out["pairWords"].view(np.uint32)
    return out


def panels(lib, inp):
    keep, args = _csr_args(inp)
    return _take(lib, lib.pp_panels(*args, inp.dC), PANELS_ARRAYS)


def choose_form(lib, dC, L, N, n_poses, any_ext_var=False, pairwise=False, panels_old=False, slab_chunks=0):
    out = (C.c_int * 6)()
    lib.pp_choose_form(dC, L, N, n_poses, int(any_ext_var), int(pairwise), int(panels_old), slab_chunks, out)
    return dict(zip(("schurDense", "schurPanels", "schurBlocks", "orderObs", "useLds", "nSlabs"), list(out)))


def order_landmarks(lib, off_lists):
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in off_lists])]).astype(np.int32)
    offs, po = _i32(np.concatenate([np.asarray(x, np.int32) for x in off_lists] + [np.zeros(0, np.int32)]))
    perm = np.zeros(len(off_lists), np.int32)
    lib.pp_order_landmarks(len(off_lists), ptr.ctypes.data_as(C.c_void_p), po, perm.ctypes.data_as(C.c_void_p))
    return perm


def chunk_order(lib, inp):
    keep, args = _csr_args(inp)
    order = np.zeros(len(inp.obsIdx), np.int32)
    lib.pp_chunk_order(args[0], args[1], args[2], args[3], len(inp.poseOff), order.ctypes.data_as(C.c_void_p))
    return order


def sb_chain(lib, sb_off, dC, d, factors, prior):
    """factors: per factor the speed / bias slots of its variable blocks; prior: the same list for the prior"""
    ptr = np.concatenate([[0], np.cumsum([len(f) for f in factors])]).astype(np.int32)
    flat, pf = _i32([s for f in factors for s in f])
    off, po = _i32(sb_off)
    pr, pp = _i32(prior)
    return lib.pp_sb_chain(len(off), po, dC, d, len(factors), ptr.ctypes.data_as(C.c_void_p), pf, len(pr), pp)
