"""The host planning of Window::pack (svin_amd/csrc/pack_plan.hpp) on the CPU.

k_schur_rows trusts its work list without checking it: a wrong pair word adds a product into the wrong accumulator or reads past
a record.  decode_rows() below restates what the kernel needs from the format documented in kernels.hpp (DeviceProblem::blk*,
panelWork) -- every workgroup, batch, wave and word, nothing sampled -- and the other planning functions are restated from their
definitions.  tests/golden/pack_plan.npz pins the arrays themselves (a change of the work list on purpose re-records it:
tests/golden/make_golden_pack_plan.py)."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pack_plan_lib as ppl          # noqa: E402

ROOT = ppl.ROOT


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return ppl.build_shim(tmp_path_factory.mktemp("pp"))


@pytest.fixture(scope="module")
def inputs():
    return {"A": ppl.input_a(), "B": ppl.input_b(), "C": ppl.input_c()}


CASES = [("A", 4), ("A", 256), ("B", 256), ("C", 1), ("C", 8)]


# ------------------------------------------------------------------------------------------------ the slots, from their definition
def expected_slots(inp):
    """one slot per (landmark, distinct variable pose), ascending with the pose block, the observations of each in CSR order"""
    ptr, blk, obs_ptr, obs, lm = [], [], [0], [], []
    for l in range(inp.L):
        ptr.append(len(blk))
        by_block = collections.OrderedDict()
        for o in range(inp.lmPtr[l], inp.lmPtr[l + 1]):
            off = inp.poseOff[int(inp.obsIdx[o]) & 0xfff]
            if off >= 0:
                by_block.setdefault(off // 6, []).append(o)
        for b in sorted(by_block):
            blk.append(b)
            lm.append(l)
            obs += by_block[b]
            obs_ptr.append(len(obs))
    ptr.append(len(blk))
    return dict(slotPtr=ptr, slotBlk=blk, slotObsPtr=obs_ptr, slotObs=obs, slotLm=lm)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_slots_are_one_per_landmark_and_distinct_variable_pose(lib, inputs, name):
    got, ref = ppl.slots(lib, inputs[name]), expected_slots(inputs[name])
    for k in ppl.SLOT_ARRAYS:
        assert got[k].tolist() == ref[k], k


def test_a_landmark_prior_takes_a_slot_at_pose_zero(lib):
    """a prior's two pseudo-observations carry pose slot 0 (camera 15): a slot at pose 0 when that pose is variable, none when it is fixed"""
    tracks = [[(3, 0), (0, 15), (0, 15)], [(2, 0), (1, 0)]]
    got = ppl.slots(lib, ppl._assemble(tracks, ppl.pose_offsets(4)))
    assert got["slotBlk"].tolist() == [0, 3, 1, 2] and got["slotObs"].tolist() == [1, 2, 0, 4, 3] and got["slotObsPtr"].tolist() == [0, 2, 3, 4, 5]
    got = ppl.slots(lib, ppl._assemble(tracks, ppl.pose_offsets(4, fixed=(0,))))
    assert got["slotBlk"].tolist() == [2, 0, 1] and got["slotLm"].tolist() == [0, 1, 1]


# ------------------------------------------------------------------------------------------------ the work list of k_schur_rows
def decode_rows(sl, w, dC, consts, row_split):
    """Everything k_schur_rows relies on, or AssertionError.  sl: the slots; w: the work list (ppl.ROWS_ARRAYS)."""
    waves, zero_rec, batch_words = consts["kBlkWaves"], consts["kBlkBatchRecs"] - 1, consts["kBlkBatchWords"]
    blk, lm_of = sl["slotBlk"].tolist(), sl["slotLm"].tolist()
    words_all = w["pairWords"].tolist()
    batch, wave_tab, rec_slot = w["batch"].reshape(-1, 2).tolist(), w["waveTab"].reshape(-1, 4).tolist(), w["recSlot"].tolist()
    work = w["panelWork"].reshape(-1, 4).tolist()
    own = w["blkOwn"].view(np.uint8).reshape(-1, waves, 2).tolist()   # per workgroup: bytes 2 w, 2 w + 1 = the rows of wave w
    n_wg, n_pairs, fits = w["counts"].tolist()
    assert fits == 1 and n_wg == len(work) == len(own)
    n_pan = (dC + 95) // 96
    pair_order = [(I, J) for I in range(n_pan) for J in range(I + 1)]
    ptr = w["panelPairPtr"].tolist()
    assert n_pairs == len(pair_order) and len(ptr) == n_pairs + 1 and ptr[0] == 0 and ptr[-1] == n_wg
    assert all(ptr[k] <= ptr[k + 1] for k in range(n_pairs))
    seen = collections.Counter()
    next_batch = next_word = next_rec = 0
    for k, (I, J) in enumerate(pair_order):
        for g in range(ptr[k], ptr[k + 1]):
            assert work[g][:2] == [I, J], "workgroups in pair order"
            first_batch, n_batches = work[g][2:]
            assert first_batch == next_batch and n_batches >= 1
            next_batch += n_batches
            loaded = set()
            for b in range(first_batch, first_batch + n_batches):
                first_rec, recs = batch[b]
                assert first_rec == next_rec and 1 <= recs <= zero_rec, "a batch stages at most kBlkBatchRecs - 1 records"
                next_rec += recs
                for wv in range(waves):
                    first_word, n0, n1, z = wave_tab[b * waves + wv]
                    assert z == 0 and first_word == next_word
                    assert n0 % 8 == 0 and n1 % 8 == 0 and 0 <= n0 and 0 <= n1 and n0 + n1 <= batch_words, "a row's words in eights, a wave's within kBlkBatchWords"
                    next_word += n0 + n1
                    for sel, (beg, n) in enumerate(((first_word, n0), (first_word + n0, n1))):
                        row = own[g][wv][sel]
                        assert n == 0 or row < 16, "words on a row the wave does not own"
                        for j in range(beg, beg + n, 2):
                            w0, w1 = words_all[j], words_all[j + 1]
                            assert w0 >> 24 == w1 >> 24, "words 2 j, 2 j + 1 share their A record"
                            assert (w0 & 0xff) != (w1 & 0xff), "words 2 j, 2 j + 1 name two accumulators"
                            for wd in (w0, w1):
                                acc2, b_off, rec_a = wd & 0xff, (wd >> 8) & 0xffff, wd >> 24
                                assert acc2 % 2 == 0 and acc2 < 32 and b_off % 160 == 0
                                rec_b = b_off // 160
                                if rec_b == zero_rec:   # padding: of a run (A real) or of the row (A the zero record as well)
                                    assert rec_a == zero_rec or rec_a < recs
                                    continue
                                assert rec_a < recs and rec_b < recs, "a record of another batch"
                                sa, sb = rec_slot[first_rec + rec_a], rec_slot[first_rec + rec_b]
                                assert lm_of[sa] == lm_of[sb], "A and B of one landmark"
                                assert blk[sa] // 16 == I and blk[sa] - 16 * I == row, "the A record's block row is the row the wave owns"
                                assert blk[sb] // 16 == J and acc2 // 2 == blk[sb] - 16 * J, "the accumulator is B's pose block in panel J"
                                seen[(I, J, sa, sb)] += 1
                                loaded.add(row)
            for row in loaded:
                owners = [wv for wv in range(waves) for sel in range(2) if own[g][wv][sel] == row]
                assert len(owners) == len(set(owners)) and 1 <= len(owners) <= (2 if row_split else 1), "a row's sets sit on different waves"
    # exact cover: every pair of slots of one landmark with slotBlk[a] >= slotBlk[b], once, in its panel pair
    expected = set()
    sp = sl["slotPtr"].tolist()
    for l in range(len(sp) - 1):
        for a in range(sp[l], sp[l + 1]):
            for b in range(sp[l], a + 1):   # (a landmark's slots ascend with the pose block)
                assert blk[a] >= blk[b]
                expected.add((blk[a] // 16, blk[b] // 16, a, b))
    assert all(c == 1 for c in seen.values()), "a pair twice"
    assert set(seen) == expected, "pairs missing or invented"
    # tails: the kernel requests words in 64s and reads descriptors three batches ahead, unconditionally
    assert next_rec == len(rec_slot)
    assert len(words_all) >= next_word + 128 and not any(words_all[next_word:])
    assert len(batch) >= next_batch + 3 and not any(x for d in batch[next_batch:] for x in d)
    assert len(wave_tab) >= (next_batch + 3) * waves and not any(x for d in wave_tab[next_batch * waves:] for x in d)
    return dict(workgroups=n_wg, batches=next_batch, words=next_word, batch_recs=[d[1] for d in batch[:next_batch]],
                wave_words=[d[1] + d[2] for d in wave_tab[:next_batch * waves]], pair_ptr=ptr)


@pytest.fixture(scope="module")
def decoded(lib, inputs):
    """every case of the issue, row split on and off: decoded once, shared"""
    consts, out = ppl.constants(lib), {}
    for name, cu in CASES:
        sl = ppl.slots(lib, inputs[name])
        for split in (True, False):
            w = ppl.rows(lib, inputs[name], cu, split)
            out[(name, cu, split)] = (sl, w, decode_rows(sl, w, inputs[name].dC, consts, split))
    return out


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name,cu", CASES)
def test_rows_work_list_is_what_the_kernel_needs(decoded, name, cu, split):
    assert decoded[(name, cu, split)][2]["words"] > 0   # (the assertions are decode_rows')


def test_inputs_take_every_cut_of_the_list(lib, inputs, decoded):
    consts = ppl.constants(lib)
    # A: three panels, the last with 11 blocks; observations on fixed poses and landmarks without a slot
    a = inputs["A"]
    sl = decoded[("A", 4, True)][0]
    assert a.dC == 258 and sl["slotBlk"].max() == 42 and int(np.sum(np.diff(sl["slotPtr"]) == 0)) == 10
    fixed = a.poseOff[(a.obsIdx & 0xfff).astype(int)] < 0
    assert 0.02 < fixed.mean() < 0.09
    # the CU count decides the cut into workgroups
    assert decoded[("A", 4, True)][2]["workgroups"] < decoded[("A", 256, True)][2]["workgroups"]
    # B: three full panels; batches end at the word limit (no batch near the record limit, some wave within an entry of the word limit)
    b = decoded[("B", 256, True)][2]
    assert inputs["B"].dC == 288 and max(b["batch_recs"]) < consts["kBlkBatchRecs"] - 1 - 32
    assert max(b["wave_words"]) > consts["kBlkBatchWords"] - 12 - 32
    # C: four panels, the last with one block; batches end at the record limit
    c1, c8 = decoded[("C", 1, True)][2], decoded[("C", 8, True)][2]
    assert inputs["C"].dC == 294 and max(c8["batch_recs"]) >= consts["kBlkBatchRecs"] - 1 - 2
    # one place: every pair is one workgroup; at 8 CUs the list is cut at kBlkMinWordsPerBlock words, which the diagonal pairs of
    # the three full panels (1500 entries of two words each) exceed
    assert c1["workgroups"] == 10 and np.diff(c1["pair_ptr"]).tolist() == [1] * 10
    assert c8["workgroups"] > 10 and all(np.diff(c8["pair_ptr"])[[0, 2, 5]] > 1)


def test_the_decode_catches_a_corrupted_list(lib, inputs, decoded):
    """the decode is not vacuous: each corruption of a good list is caught"""
    consts = ppl.constants(lib)
    sl, good, _ = decoded[("A", 256, True)]
    dC = inputs["A"].dC

    def corrupted(**changes):
        w = {k: v.copy() for k, v in good.items()}
        w.update(changes)
        with pytest.raises(AssertionError):
            decode_rows(sl, w, dC, consts, True)

    words = good["pairWords"]
    zero = consts["kBlkBatchRecs"] - 1
    real = lambda x: ((int(x) >> 8) & 0xffff) // 160 != zero
    # a position 2 j + 1 | 2 j + 2 inside one row where two real words of different A records meet
    n0 = int(good["waveTab"][1])
    j = next(j for j in range(1, n0 - 1, 2) if real(words[j]) and real(words[j + 1]) and words[j] >> 24 != words[j + 1] >> 24)
    sw = words.copy()
    sw[[j, j + 1]] = sw[[j + 1, j]]
    corrupted(pairWords=sw)                                            # two words swapped across an even boundary
    first_real = next(i for i in range(len(words)) if real(words[i]))
    corrupted(pairWords=np.delete(words, first_real))                  # one word dropped (the rest moves up)
    gone = words.copy()
    gone[first_real] = (zero << 24) | ((zero * 160) << 8) | (int(gone[first_real]) & 0xff)
    corrupted(pairWords=gone)                                          # one product replaced by padding
    acc = words.copy()
    acc[first_real] = (int(acc[first_real]) & ~0xff) | ((int(acc[first_real]) + 4) & 0x1f)
    corrupted(pairWords=acc)                                           # one word adds into the wrong accumulator
    tab = good["waveTab"].copy()
    tab[1] = 4
    corrupted(waveTab=tab)                                             # a row of four words
    twice = words.copy()
    k = next(i for i in range(first_real + 2, len(words)) if real(words[i]) and words[i] != words[first_real] and i % 2 == first_real % 2)
    twice[k] = twice[first_real]
    corrupted(pairWords=twice)                                         # one product twice, another never
    own = good["blkOwn"].copy()
    own[0] ^= 0x0101
    corrupted(blkOwn=own)                                              # the first wave owns other rows than its words serve
    bt = good["batch"].copy()
    bt[1] = zero + 1
    corrupted(batch=bt)                                                # a batch of kBlkBatchRecs records
    corrupted(pairWords=words[:-1])                                    # a short tail


# ------------------------------------------------------------------------------------------------ golden arrays
def test_arrays_are_the_recorded_ones(lib):
    """the inputs stored in the fixture through today's builders: the arrays that reach the device, byte for byte"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "pack_plan.npz"))
    for name in ("A", "C"):
        inp = ppl.PlanInput(g[name + "_lmPtr"], g[name + "_obsIdx"], g[name + "_poseOff"], int(g[name + "_dC"]))
        got = dict(ppl.slots(lib, inp))
        got.update(ppl.rows(lib, inp, 256, True))
        got.update({"old_" + k: v for k, v in ppl.panels(lib, inp).items()})
        got["obsOrder"] = ppl.chunk_order(lib, inp)
        for k, v in got.items():
            ref = g[name + "_" + k]
            assert v.dtype == ref.dtype and v.shape == ref.shape and v.tobytes() == ref.tobytes(), (name, k)
    # the generators of this module's inputs still produce what was recorded
    for name, inp in (("A", ppl.input_a()), ("C", ppl.input_c())):
        assert inp.obsIdx.tobytes() == g[name + "_obsIdx"].tobytes() and inp.lmPtr.tobytes() == g[name + "_lmPtr"].tobytes()


# ------------------------------------------------------------------------------------------------ the other functions
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_chunk_observation_order(lib, inputs, name):
    inp = inputs[name]
    order = ppl.chunk_order(lib, inp).tolist()
    pose = (inp.obsIdx & 0xfff).astype(int).tolist()
    for l0 in range(0, inp.L, 16):
        beg, end = int(inp.lmPtr[l0]), int(inp.lmPtr[min(inp.L, l0 + 16)])
        part = order[beg:end]
        assert sorted(part) == list(range(beg, end))                              # a permutation of the chunk's range
        keys = [(pose[o], o) for o in part]
        assert keys == sorted(keys)                                               # pose slot non-decreasing, one pose's in order


def signature(offs):
    tiles = sorted({t for off in offs if off >= 0 for t in (off >> 4, (off + 5) >> 4)})
    lo = sum(1 << t for t in tiles if t < 64)
    hi = sum(1 << (t - 64) for t in tiles if 64 <= t < 128)
    return (tiles[0], tiles[-1], hi, lo) if tiles else (0, -1, 0, 0)


def test_landmarks_are_ordered_by_signature(lib, inputs):
    a = inputs["A"]
    lists = [a.poseOff[(a.obsIdx[a.lmPtr[l]:a.lmPtr[l + 1]] & 0xfff).astype(int)].tolist() for l in range(a.L)]
    lists += [[6 * 300, 6 * 170], [6 * 170, 6 * 300, 6 * 200], [], [-1]]   # tiles beyond 64 (high mask) and beyond 128 (first / last only)
    perm = ppl.order_landmarks(lib, lists).tolist()
    assert sorted(perm) == list(range(len(lists)))
    keys = [(signature(lists[l]), l) for l in perm]
    assert keys == sorted(keys)   # by (first tile, last tile, high mask, low mask); equal signatures keep their order
    assert len({k for k, _ in keys}) < len(keys) and len({k for k, _ in keys}) > 50


def chain(lib, fixed=(), factors=None, n=10, dC=60):
    sb_off, d = [], dC
    for i in range(n):
        sb_off.append(-1 if i in fixed else d)
        d += 0 if i in fixed else 9
    if factors is None:
        factors = [[i, i + 1] for i in range(n - 1)]
    variable = lambda f: [s for s in f if s not in fixed]
    return ppl.sb_chain(lib, sb_off, dC, d, [variable(f) for f in factors], variable([0, 1]))


def test_speed_bias_chain_length(lib):
    neighbours = [[i, i + 1] for i in range(9)]
    assert chain(lib) == 10                                          # neighbour factors and a prior over the first two
    assert chain(lib, factors=neighbours + [[0, 2]]) == 0            # one factor ties blocks 0 and 2
    # a fixed block in the middle takes no rows: its neighbours become neighbours in the order of the rows, and the factors
    # that tied them to it tie one variable block each -- a chain of nine
    assert chain(lib, fixed=(4,)) == 9
    assert chain(lib, fixed=(4,), factors=neighbours + [[3, 5]]) == 9
    assert chain(lib, fixed=(4,), factors=neighbours + [[3, 6]]) == 0
    # rows behind the chain (d larger than the chain accounts for), or a block out of row order: no chain
    assert ppl.sb_chain(lib, [60, 69], 60, 60 + 18 + 6, [[0, 1]], []) == 0
    assert ppl.sb_chain(lib, [69, 60], 60, 78, [[0, 1]], []) == 0
    assert ppl.sb_chain(lib, [60, 69], 60, 78, [[0, 1]], []) == 2
    assert ppl.sb_chain(lib, [], 60, 60, [[]], []) == 0


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_panels_work_list(lib, inputs, name):
    inp, per_wg = inputs[name], ppl.constants(lib)["kPanelChunksPerBlock"]
    w = ppl.panels(lib, inp)
    n_pan = (inp.dC + 95) // 96
    pair_order = [(I, J) for I in range(n_pan) for J in range(I + 1)]
    n_wg, n_pairs = w["counts"].tolist()
    work, ptr = w["panelWork"].reshape(-1, 4).tolist(), w["panelPairPtr"].tolist()
    assert n_pairs == len(pair_order) and len(ptr) == n_pairs + 1 and ptr[0] == 0 and ptr[-1] == n_wg == len(work)
    got = collections.Counter()
    nxt = 0
    for k, pair in enumerate(pair_order):
        assert ptr[k] <= ptr[k + 1]
        for g in range(ptr[k], ptr[k + 1]):
            I, J, first, cnt = work[g]
            assert (I, J) == pair and first == nxt and 1 <= cnt <= per_wg
            nxt += cnt
            for c in w["panelChunks"][first:first + cnt].tolist():
                got[(I, J, c)] += 1
    assert nxt == len(w["panelChunks"])
    expected = set()
    for c in range((inp.L + 15) // 16):
        offs = inp.poseOff[(inp.obsIdx[inp.lmPtr[16 * c]:inp.lmPtr[min(inp.L, 16 * c + 16)]] & 0xfff).astype(int)]
        offs = offs[offs >= 0]
        lo, hi = (int(offs.min()) // 96, int(offs.max()) // 96) if len(offs) else (0, 0)   # no variable pose: pair (0, 0)
        expected |= {(I, J, c) for I in range(lo, hi + 1) for J in range(lo, I + 1)}
    assert all(v == 1 for v in got.values()) and set(got) == expected


def test_a_chunk_without_variable_poses_goes_to_the_first_pair(lib):
    tracks = [[(0, 0)]] * 16 + [[(1, 0), (1, 1)]] * 5
    w = ppl.panels(lib, ppl._assemble(tracks, [300, -1]))
    assert w["panelWork"].reshape(-1, 4).tolist() == [[0, 0, 0, 1], [3, 3, 1, 1]] and w["panelChunks"].tolist() == [1, 0]


def test_schur_form_boundaries(lib):
    c = ppl.constants(lib)
    form = lambda *a, **k: ppl.choose_form(lib, *a, **k)
    # dC + 2 = 256 | 258: the dense form ends, the block-pair form of the panel form begins
    f = form(254, 1000, 9000, 42)
    assert (f["schurDense"], f["schurPanels"], f["schurBlocks"], f["orderObs"], f["nSlabs"]) == (1, 0, 0, 1, 63)
    f = form(256, 1000, 9000, 42)
    assert (f["schurDense"], f["schurPanels"], f["schurBlocks"], f["orderObs"]) == (0, 1, 1, 0)
    # more than eight tile rows, or variable extrinsics, order the observations; no observations, no order
    assert form(126, 100, 900, 21)["orderObs"] == 0 and form(127, 100, 900, 21)["orderObs"] == 1
    assert form(60, 100, 900, 5, any_ext_var=True)["orderObs"] == 1 and form(60, 100, 0, 5, any_ext_var=True)["orderObs"] == 0
    # the pose count at kDensePoseCap (fixed poses count: the kernel stages a row per pose slot)
    assert form(60, 100, 900, c["kDensePoseCap"])["schurDense"] == 1 and form(60, 100, 900, c["kDensePoseCap"] + 1)["schurDense"] == 0
    # variable extrinsics on a wide window: neither panel form; slabs by eights while a slab fits the LDS, one slab beyond
    f = form(258, 1000, 9000, 43, any_ext_var=True)
    assert (f["schurDense"], f["schurPanels"], f["schurBlocks"], f["useLds"], f["nSlabs"]) == (0, 0, 0, 0, 1)
    f = form(60, 1000, 9000, 300)
    assert (f["schurDense"], f["schurPanels"], f["useLds"]) == (0, 1, 1)
    f = form(60, 1000, 9000, 300, any_ext_var=True)
    assert (f["schurPanels"], f["useLds"], f["nSlabs"]) == (0, 1, 125) and form(60, 5000, 9000, 300, any_ext_var=True)["nSlabs"] == 256
    # dC / 6 at kBlkMaxPoseBlocks: a pose block index of the block-pair form
    assert form(6 * c["kBlkMaxPoseBlocks"], 100, 900, 600)["schurBlocks"] == 1
    f = form(6 * c["kBlkMaxPoseBlocks"] + 6, 100, 900, 600)
    assert (f["schurPanels"], f["schurBlocks"]) == (1, 0)
    # an empty window takes no form at all
    f = form(0, 0, 0, 0)
    assert (f["schurDense"], f["schurPanels"], f["nSlabs"]) == (0, 0, 1) and form(300, 0, 0, 50)["schurPanels"] == 0
    # SVIN_SCHUR_PAIRWISE, SVIN_PANELS_OLD, SVIN_SLAB_CHUNKS
    f = form(60, 1000, 9000, 10, pairwise=True)
    assert (f["schurDense"], f["schurPanels"], f["orderObs"], f["nSlabs"]) == (0, 0, 0, 125)
    assert form(300, 1000, 9000, 50, pairwise=True)["schurPanels"] == 0
    f = form(300, 1000, 9000, 50, panels_old=True)
    assert (f["schurPanels"], f["schurBlocks"]) == (1, 0)
    assert form(60, 1000, 9000, 10)["nSlabs"] == 63 and form(60, 1000, 9000, 10, slab_chunks=1)["nSlabs"] == 63
    assert form(60, 1000, 9000, 10, slab_chunks=4)["nSlabs"] == 16 and form(60, 1000, 9000, 10, slab_chunks=100)["nSlabs"] == 1
    assert form(60, 5000, 9000, 10)["nSlabs"] == 256 and form(60, 5000, 9000, 10, slab_chunks=1)["nSlabs"] == 256


# ------------------------------------------------------------------------------------------------ under a sanitizer
def test_planner_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program (its own main, inputs A, B, C from a fixed seed, every function of the header), run as a child"""
    exe = str(tmp_path / "pack_plan_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "pack_plan_sanitize.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout[-4000:]
