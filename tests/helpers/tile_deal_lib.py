"""The deal of the reduced system's tile rows to the waves of the LDS-resident solver (svin_amd/csrc/pack_plan.hpp planTileDeal
through tests/csrc/tile_deal_shim.cpp), the properties a deal must have, and a model of the solver's flag protocol that rehearses
a deal on the CPU.  Shared by tests/test_tile_deal_host.py (CPU) and tests/test_gpu_tile_deal.py.

A skyline is hi[0 .. nT): the last tile row of tile column k that can hold a non-zero, closed under the fill of the factorisation.
A deal is owner[I] for the tile rows I >= 2: waves 1-3 and 5-7 are the owners, wave 4 is the quiet wave (it shares a SIMD with wave
0, the pivot wave, and runs the forward substitution once its rows are done)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MAX_TILES = 11
QUIET = 4
OWNERS = (1, 2, 3, 5, 6, 7)


def build_shim(directory):
    so = os.path.join(str(directory), "libtd.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "tile_deal_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.td_plan.restype, lib.td_plan.argtypes = C.c_uint64, [C.c_int, C.c_void_p, C.c_void_p]
    lib.td_plan_cut.restype, lib.td_plan_cut.argtypes = C.c_uint64, [C.c_int, C.c_uint64]
    lib.td_owner_of.argtypes = [C.c_uint64, C.c_int, C.c_int]
    assert lib.td_max_tiles() == MAX_TILES and lib.td_quiet_wave() == QUIET
    return lib


def plan(lib, hi):
    """-> (word, {I: wave} for I >= 2): the word DeviceProblem carries and the owners the planner lists"""
    nT = len(hi)
    h, owner = np.asarray(list(hi) + [0], np.int32), np.zeros(MAX_TILES, np.int32)
    word = int(lib.td_plan(nT, h.ctypes.data, owner.ctypes.data))
    n = nT if nT <= MAX_TILES else 0
    return word, {I: int(owner[I]) for I in range(2, n)}


def decode(lib, word, nT):
    """{I: wave}: the owners the kernel reads out of the word (nibble 0: its closed form)"""
    return {I: int(lib.td_owner_of(word, nT, I)) for I in range(2, nT)}


def pack_cut(hi):
    nT = len(hi)
    return sum((nT - 1 - h) << (4 * k) for k, h in enumerate(hi))


def close_fill(hi):
    """the skyline closed under the fill: column k eliminates into rows k+1 .. hi[k], each of which then reaches as far down"""
    hi = [max(int(h), k) for k, h in enumerate(hi)]
    for k in range(len(hi)):
        for r in range(k + 1, hi[k] + 1):
            hi[r] = max(hi[r], hi[k])
    return hi


def interval(hi, I):
    """columns in which tile row I has work for its owner: first[I] .. I - 2 (a range, possibly empty)"""
    first = min(k for k in range(I + 1) if hi[k] >= I)
    return range(first, I - 1)


def meet(hi, a, b):
    return bool(set(interval(hi, a)) & set(interval(hi, b)))


def check_deal(hi, owner):
    """the rules of a planned deal (a dict I -> wave over the rows 2 .. nT-1)"""
    nT = len(hi)
    assert sorted(owner) == list(range(2, nT)), "every row >= 2 has exactly one owner"
    assert all(w in OWNERS or w == QUIET for w in owner.values())
    rows = {w: [I for I in owner if owner[I] == w] for w in OWNERS + (QUIET,)}
    for w in OWNERS:
        for a in rows[w]:
            for b in rows[w]:
                assert a >= b or not meet(hi, a, b), "wave %d: rows %d and %d both have work in one column" % (w, b, a)
    for I in rows[QUIET]:
        for w in OWNERS:
            assert any(meet(hi, I, J) for J in rows[w]), "row %d stays on the quiet wave although wave %d is free for it" % (I, w)


# ---- the flag protocol of k_chol_solve_lds_body<0>, wave by wave, in the order the kernel issues its waits, its arithmetic and its
# flag stores.  Counters: pivotDone, xReady[I], rowUpd[I] (monotonic, one writer each).  The arithmetic is modelled by what it
# depends on: a pivot tile needs every column of its skyline applied to it, a panel solve needs the pivot and its own tile complete, a
# tile product needs both panel tiles, and the columns reach a tile in ascending order (the right-looking factorisation).
class Protocol:
    def __init__(self, hi, owner):
        self.hi, self.nT, self.owner = list(hi), len(hi), dict(owner)
        self.pivot_done = 0
        self.x_ready = [0] * self.nT
        self.row_upd = [0] * self.nT
        self.pivoted, self.solved = set(), set()
        self.applied = {(I, J): [] for I in range(self.nT) for J in range(I + 1)}
        self.writer = {}

    def need(self, I, J, below=None):
        """columns the factorisation applies to tile (I, J), J <= I: the k < J whose skyline reaches row I"""
        return [k for k in range(J if below is None else min(J, below)) if I <= self.hi[k]]

    def flag(self, wave, name, idx, val):
        arr = {"x": self.x_ready, "u": self.row_upd}[name]
        if wave == 0:   # the pivot wave stores xReady[I] once, for the row's last panel tile (I, I - 1), behind the owner's rowUpd[I]
            assert name == "x" and val == idx and self.row_upd[idx] >= idx - 1
        else:
            assert self.writer.setdefault((name, idx), wave) == wave, "flag %s[%d] has two writers" % (name, idx)
        assert arr[idx] <= val
        arr[idx] = val

    def ok(self, cond):
        name, idx, val = cond
        return (self.pivot_done if name == "p" else self.x_ready[idx] if name == "x" else self.row_upd[idx]) >= val

    def pivot(self, k):
        assert self.applied[(k, k)] == self.need(k, k), "pivot %d ahead of its updates" % k
        self.pivoted.add(k)
        self.pivot_done = k + 1

    def panel(self, I, k):
        assert k in self.pivoted and I <= self.hi[k] and (I, k) not in self.solved
        assert self.applied[(I, k)] == self.need(I, k), "panel solve (%d, %d) ahead of its updates" % (I, k)
        self.solved.add((I, k))

    def product(self, I, J, k):
        assert (I, k) in self.solved and (J, k) in self.solved, "product (%d, %d) column %d ahead of its panel tiles" % (I, J, k)
        assert self.applied[(I, J)] == self.need(I, J, below=k), "tile (%d, %d): column %d out of order" % (I, J, k)
        self.applied[(I, J)].append(k)

    def update_row(self, I, kb, skip):
        for J in range(kb + 1 + skip, I + 1):
            self.product(I, J, kb)

    def finished(self):
        assert self.pivoted == set(range(self.nT))
        for (I, J), got in self.applied.items():
            assert got == self.need(I, J), (I, J)
        assert self.solved == {(I, k) for k in range(self.nT) for I in range(k + 1, self.hi[k] + 1)}


def wave0(st):
    nT, hi = st.nT, st.hi
    for kb in range(nT):
        st.pivot(kb)
        if kb + 1 < nT:
            if kb > 0:
                yield ("u", kb + 1, kb)
            if kb + 1 <= hi[kb]:   # (outside the skyline the tile is zero: the kernel's solve and product leave zeros)
                st.panel(kb + 1, kb)
            st.flag(0, "x", kb + 1, kb + 1)
            if kb + 1 <= hi[kb]:
                st.product(kb + 1, kb + 1, kb)


def owner_wave(st, wave):
    nT, hi = st.nT, st.hi
    rows = [I for I in range(2, nT) if st.owner[I] == wave]
    kb_end = max(rows) - 1 if rows else 0
    early = set()
    for kb in range(kb_end):
        hi0, hi1 = hi[kb], hi[kb + 1]
        waited = False
        done, early = early, set()
        if kb + 2 in done and kb + 2 in rows:
            yield ("x", kb + 1, kb + 1)
            st.update_row(kb + 2, kb, 0)
            st.flag(wave, "u", kb + 2, kb + 1)
        for I in range(kb + 2, nT):
            if I not in rows or I in done:
                continue
            in0 = I <= hi0
            if in0:
                if not waited:
                    yield ("p", 0, kb + 1)
                    waited = True
                st.panel(I, kb)
            st.flag(wave, "x", I, kb + 1)
            if I == kb + 2:
                if in0:
                    yield ("x", kb + 1, kb + 1)
                    st.update_row(I, kb, 0)
                st.flag(wave, "u", I, kb + 1)
        for I in range(kb + 3, nT):
            if I not in rows:
                continue
            in0 = I <= hi0
            if in0:
                yield ("x", kb + 1, kb + 1)
                st.product(I, kb + 1, kb)
            if I <= hi1 and st.pivot_done >= kb + 2:   # (a look, not a wait)
                st.panel(I, kb + 1)
                st.flag(wave, "x", I, kb + 2)
                early.add(I)
            if in0:
                for J in range(kb + 2, I):
                    yield ("x", J, kb + 1)
                st.update_row(I, kb, 1)
            st.flag(wave, "u", I, kb + 1)
    if wave == QUIET:   # the forward substitution reads column kb of the factor
        for kb in range(nT):
            yield ("p", 0, kb + 1)
            for J in range(kb + 1, nT):
                yield ("x", J, kb + 1)
            assert all((J, kb) in st.solved for J in range(kb + 1, hi[kb] + 1))


def rehearse(hi, owner, rng=None, greedy=None):
    """runs the eight waves over the deal to the end: at every step one wave that can move moves to its next wait (picked by rng, or
    the lowest / highest wave for greedy = 'low' / 'high').  Raises if a dependency is broken or no wave can move."""
    st = Protocol(hi, owner)
    gens = {0: wave0(st)}
    gens.update({w: owner_wave(st, w) for w in OWNERS + (QUIET,)})
    waiting = {w: None for w in gens}   # the condition a wave is parked on (None: it can move)
    steps = 0
    while gens:
        ready = [w for w in sorted(gens) if waiting[w] is None or st.ok(waiting[w])]
        assert ready, "deadlock: %r" % ({w: waiting[w] for w in gens},)
        w = ready[0] if greedy == "low" else ready[-1] if greedy == "high" else ready[int(rng.integers(len(ready)))]
        try:
            waiting[w] = next(gens[w])
        except StopIteration:
            del gens[w]
        steps += 1
        assert steps < 100000
    st.finished()
    return st
