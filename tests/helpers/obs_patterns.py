"""Windows with designed observation structure for the landmark-elimination tests.

`design()` starts from a window in which every landmark projects into every frame and camera (syn.make_window with n_obs=None, a
small frame_dt and a far depth range) and keeps, per landmark, exactly the observations of a planned track.  Every pattern is
asserted on the spec itself before anything is fed to an estimator, and `work_list_stats()` restates the few lines of arithmetic
by which Window::pack cuts the block-pair work list (slots, entries, workgroups by pair words, batches by records and by words
per wave), so that a test can require that its window does reach the caps -- nothing here imports the product.

Pose BLOCKS are the variable poses in frame order (a constant pose has no block); a panel is 16 blocks.
"""
from dataclasses import dataclass, field

import numpy as np

from svin_amd import synthetic as syn

PANEL = 16
BATCH_RECS = 230          # kBlkBatchRecs (one of them is the zero record)
BATCH_WORDS = 128 - 12    # kBlkBatchWords less the padding reserve pack() keeps
WAVES = 8                 # kBlkWaves
MIN_WORDS_PER_WG = 1024   # kBlkMinWordsPerBlock


@dataclass
class Design:
    spec: object
    fixed_frame: int = None                 # frame index of the constant pose, or None
    roles: dict = field(default_factory=dict)   # role name -> landmark indices
    tracks: dict = field(default_factory=dict)  # landmark index -> sorted [(frame, cam)]
    outliers: list = field(default_factory=list)   # observation indices moved 30-80 px

    @property
    def min_obs(self):
        c = [len(t) for t in self.tracks.values() if len(t)]
        return min(c) if c else 0


def full_window(P, L, rig="euroc", seed=1):
    """a window of exactly L landmarks, each of which projects into every frame and camera (drawn from a larger seeded window:
    the first L of its landmarks that do)"""
    spec = syn.make_window(P=P, L=int(1.4 * L) + 16, n_obs=None, rig=rig, seed=seed, frame_dt=0.3 / max(P, 8),
                           depth_range=(6.0, 12.0), traj=dict(speed=0.5, rot_amp=0.1, wobble=0.1))
    cnt = np.bincount(spec.obs_lm, minlength=spec.L)
    pool = np.nonzero(cnt == 2 * P)[0][:L]
    assert len(pool) == L, "only %d landmarks project into every frame and camera, %d wanted" % (len(pool), L)
    new = np.full(spec.L, -1, np.int64)
    new[pool] = np.arange(L)
    keep = new[spec.obs_lm] >= 0
    for name in ("obs_frame", "obs_cam", "obs_uv", "obs_size"):
        setattr(spec, name, getattr(spec, name)[keep])
    spec.obs_lm = new[spec.obs_lm[keep]]
    spec.lm_true, spec.lm_init = spec.lm_true[pool], spec.lm_init[pool]
    assert spec.L == L and np.all(np.bincount(spec.obs_lm, minlength=L) == 2 * P)
    return spec


def block_frames(P, fixed_frame):
    """frame index of every pose block"""
    return [f for f in range(P) if f != fixed_frame]


def design(P, L, rig="euroc", seed=1, fixed_frame=None, wide=False, sparse_pairs=False, n_full=3, n_comb=0, n_outliers=6, short_tracks=True):
    """short_tracks=False leaves out the one- and two-observation tracks: every landmark then has at least three observations and
    the window can be linearised without damping"""
    spec = full_window(P, L, rig, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    # Every landmark of the window is observed, so the device holds all L of them (pack() drops a landmark without observations).
    # What a device chunk CAN hold is a landmark without slots and rows: one seen by the constant pose alone.  With a constant pose
    # landmarks 3 and 7 (holes inside chunk 0) and 16 .. 31 (the whole of chunk 1) are such; where pack() re-sorts the landmarks
    # (more than 42 pose blocks) the eighteen come first: chunk 0 is all of them, chunk 1 starts with two.
    reserved = sorted({3, 7} | set(range(16, 32))) if (fixed_frame is not None and L >= 33) else []
    free = [l for l in range(L) if l not in reserved]
    frames = block_frames(P, fixed_frame)
    nB = len(frames)
    nPan = (nB + PANEL - 1) // PANEL
    both = lambda fs: sorted((f, c) for f in fs for c in (0, 1))
    tracks, roles = {}, {}

    def take(role, n, make):
        got = []
        for _ in range(n):
            l = free.pop(0)
            tracks[l] = make(len(got))
            got.append(l)
        assert len(got) == n, "window too small for role %s" % role
        roles[role] = got

    tiny = L <= 17   # one landmark, a chunk less one, a chunk, a chunk and one: full tracks only
    if tiny:
        assert fixed_frame is None and not wide
        take("full", L, lambda k: both(range(P)))
    if short_tracks and not tiny:
        take("single", 2, lambda k: [(frames[(nB // 2 + k) % nB], k % 2)])
        take("stereo", 3, lambda k: both([frames[(3 * k + 1) % nB]]))
    elif not tiny:
        assert fixed_frame is None
    if 2 * nB >= 65:
        take("obs64", 1, lambda k: both(frames[:32]))
        if not (sparse_pairs and nPan == 3):   # (65 observations span three panels: with three panels pair (2, 0) would get an entry)
            take("obs65", 1, lambda k: both(frames[:32]) + [(frames[32], 0)])
    if not sparse_pairs and not tiny:
        take("full", n_full, lambda k: both(range(P)))
    if fixed_frame is not None:
        if reserved:
            roles["fixed_only"] = reserved
            for k, l in enumerate(reserved):
                tracks[l] = both([fixed_frame]) if k % 2 else [(fixed_frame, 0)]
        else:
            take("fixed_only", 3, lambda k: both([fixed_frame]) if k else [(fixed_frame, 0)])
        take("fixed_plus_one", 3, lambda k: both([fixed_frame, frames[(5 * k + 2) % nB]]))
    if wide:
        assert nPan >= 3
        for pan in range(nPan):
            lo, hi = PANEL * pan, min(nB, PANEL * (pan + 1))
            take("confined%d" % pan, 10, lambda k: both(frames[lo + k % max(1, hi - lo - 2):min(lo + k % max(1, hi - lo - 2) + 3, hi)]))
        take("boundary15_16", 4, lambda k: both([frames[15], frames[16]]))
        if sparse_pairs:
            b = PANEL * (nPan - 1)
            take("single_pair", 1, lambda k: both([frames[b - 1], frames[b]]))     # the only landmark of pair (nPan-1, nPan-2)
            take("two_panels", 2, lambda k: both(frames[:2 * PANEL]))
        else:
            take("boundary31_32", 4, lambda k: both([frames[31], frames[32]]))
            take("two_panels", 2, lambda k: both(frames[:PANEL] + frames[PANEL * (nPan - 1):]))
            # all blocks of panel 1, one block of panel 0: 17 records and 32 pair words (two per block row) per entry of pair (1, 0)
            take("comb", n_comb, lambda k: both(frames[PANEL:2 * PANEL] + [frames[k % PANEL]]))
    # the rest: short runs of consecutive blocks (inside one panel in the sparse variant), at least three observations
    rest = []
    while free:
        l = free.pop(0)
        n = int(rng.integers(2, 7))
        a = int(rng.integers(0, nB))
        if wide and sparse_pairs:
            pan = a // PANEL
            lo, hi = PANEL * pan, min(nB, PANEL * (pan + 1))
            a = min(a, max(lo, hi - n))
            run = frames[a:min(a + n, hi)]
        else:
            run = frames[a:a + n] if a + n <= nB else frames[nB - n:]
        t = both(run)
        if rng.random() < 0.25 and len(t) > 3:
            t.pop(int(rng.integers(len(t))))
        tracks[l] = t
        rest.append(l)
    roles["runs"] = rest
    assert sorted(tracks) == list(range(L)) and all(tracks.values()), "every landmark is observed"
    # keep exactly the planned observations
    key = (spec.obs_lm * P + spec.obs_frame) * 2 + spec.obs_cam
    want = np.array(sorted((l * P + f) * 2 + c for l, t in tracks.items() for f, c in t), np.int64)
    keep = np.isin(key, want)
    assert keep.sum() == len(want), "a planned observation is not in the window"
    for name in ("obs_lm", "obs_frame", "obs_cam", "obs_uv", "obs_size"):
        setattr(spec, name, getattr(spec, name)[keep])
    d = Design(spec=spec, fixed_frame=fixed_frame, roles=roles, tracks=tracks)
    # outliers: a handful of observations 30-80 px off (on landmarks with long enough tracks to stay determined)
    cand = np.nonzero(np.isin(spec.obs_lm, rest if rest else roles["full"]))[0]
    d.outliers = [int(i) for i in rng.choice(cand, min(n_outliers, len(cand)), replace=False)]
    for i in d.outliers:
        ang, mag = rng.uniform(0, 2 * np.pi), rng.uniform(30.0, 80.0)
        spec.obs_uv[i] += mag * np.array([np.cos(ang), np.sin(ang)])
    check(d, wide=wide, sparse_pairs=sparse_pairs, n_comb=n_comb, short_tracks=short_tracks)
    return d


def keep_tracks(spec, tracks):
    """reduce a full window to exactly the planned observations"""
    P = spec.P
    key = (spec.obs_lm * P + spec.obs_frame) * 2 + spec.obs_cam
    want = np.array(sorted((l * P + f) * 2 + c for l, t in tracks.items() for f, c in t), np.int64)
    keep = np.isin(key, want)
    assert keep.sum() == len(want), "a planned observation is not in the window"
    for name in ("obs_lm", "obs_frame", "obs_cam", "obs_uv", "obs_size"):
        setattr(spec, name, getattr(spec, name)[keep])
    assert np.all(np.bincount(spec.obs_lm, minlength=spec.L) == [len(tracks[l]) for l in range(spec.L)])


def design_track_lengths(P=17, lengths=(15, 16, 17, 31, 32, 33, 34), n_more=9, seed=1):
    """narrow window whose first landmarks have tracks of exactly the given numbers of observations (the post-solve pass gives a
    landmark sixteen lanes, each keeping its first observation in registers: one lane short, all lanes once, one lane twice, ...
    two lanes a third time), followed by n_more landmarks with three to six; every pose is observed"""
    assert max(lengths) <= 2 * P
    L = len(lengths) + n_more
    spec = full_window(P, L, "euroc", seed)
    every = sorted((f, c) for f in range(P) for c in (0, 1))
    tracks = {l: every[:n] for l, n in enumerate(lengths)}
    for k in range(n_more):
        tracks[len(lengths) + k] = every[(5 * k) % (2 * P - 6):][:3 + k % 4]
    keep_tracks(spec, tracks)
    assert set(spec.obs_frame.tolist()) == set(range(P))
    return Design(spec=spec, tracks=tracks, roles={"lengths": list(range(len(lengths)))})


def design_three_observations(L, P=3, seed=1):
    """L landmarks with three observations each on P = 3 poses (one per pose, cameras alternating): the smallest window with a
    given landmark count that can be linearised without damping"""
    spec = full_window(P, L, "euroc", seed)
    tracks = {l: [(f, (l + f) % 2) for f in range(P)] for l in range(L)}
    keep_tracks(spec, tracks)
    return Design(spec=spec, tracks=tracks, roles={"three": list(range(L))})


def slots_of(d):
    """per landmark with observations on variable poses: sorted block indices (one slot per distinct variable pose)"""
    spec = d.spec
    blk = {f: k for k, f in enumerate(block_frames(spec.P, d.fixed_frame))}
    out = {}
    for l in range(spec.L):
        fs = sorted({blk[f] for f, _ in d.tracks.get(l, []) if f in blk})
        if fs:
            out[l] = fs
    return out


def pair_lists(d):
    """{(I, J): [(landmark, blocks in I, blocks in J)]} in landmark order, I >= J -- the entries of pack()'s block-pair work list"""
    lists = {}
    for l, bl in slots_of(d).items():
        pans = sorted({b // PANEL for b in bl})
        for I in pans:
            for J in pans:
                if J <= I:
                    lists.setdefault((I, J), []).append((l, [b for b in bl if b // PANEL == I], [b for b in bl if b // PANEL == J]))
    return lists


def entry_words(nA, nB, diagonal):
    return sum((((ka + 1) if diagonal else nB) + 1) & ~1 for ka in range(nA))


def work_list_stats(d, compute_units, rounds=2):
    """what can be said for certain about pack()'s cut of the block-pair work list: per pair the number of entries and workgroups
    (cut by pair words), and whether the FIRST batch of some workgroup is ended by the record cap / by the words-per-wave cap.
    A batch ends at the record cap for certain when the records overflow while no wave can hold more than the word cap (a wave owns
    at most two block rows); at the word cap for certain when the words overflow what eight waves can hold while the records fit."""
    lists = pair_lists(d)
    nB = len(block_frames(d.spec.P, d.fixed_frame))
    nPan = (nB + PANEL - 1) // PANEL
    nPairs = nPan * (nPan + 1) // 2
    words = {k: [entry_words(len(a), len(b), k[0] == k[1]) for _, a, b in v] for k, v in lists.items()}
    total = sum(sum(w) for w in words.values())
    places = max(1, rounds * 2 * compute_units - nPairs)
    per_wg = max(MIN_WORDS_PER_WG, (total + places - 1) // places)
    out = dict(n_pairs=nPairs, entries={k: len(v) for k, v in lists.items()}, workgroups={}, record_cap=False, word_cap=False,
               words_per_workgroup=per_wg, pairs_without_entries=[(I, J) for I in range(nPan) for J in range(I + 1) if (I, J) not in lists])
    for k, v in lists.items():
        dg = k[0] == k[1]
        e, n_wg = 0, 0
        while e < len(v):
            e_end, wg = e, 0
            while e_end < len(v) and wg < per_wg:
                wg += words[k][e_end]
                e_end += 1
            n_wg += 1
            recs, tot, row = 0, 0, {}
            for i in range(e, e_end):
                _, a, b = v[i]
                need = len(a) + (0 if dg else len(b))
                for ka, blk in enumerate(a):
                    row[blk] = row.get(blk, 0) + ((((ka + 1) if dg else len(b)) + 1) & ~1)
                two = sum(sorted(row.values())[-2:])
                if recs + need > BATCH_RECS - 1:
                    if two <= BATCH_WORDS:
                        out["record_cap"] = True
                    break
                recs += need
                tot += words[k][i]
                if tot > WAVES * BATCH_WORDS:
                    out["word_cap"] = True
                    break
            e = e_end
        out["workgroups"][k] = n_wg
    return out


def check(d, wide=False, sparse_pairs=False, n_comb=0, short_tracks=True):
    """the patterns, asserted on the spec itself"""
    spec = d.spec
    P, L = spec.P, spec.L
    cnt = np.bincount(spec.obs_lm, minlength=L)
    for l in range(L):
        assert cnt[l] == len(d.tracks.get(l, [])), (l, cnt[l])
    key = set(zip(spec.obs_lm.tolist(), spec.obs_frame.tolist(), spec.obs_cam.tolist()))
    assert len(key) == spec.N
    for l, t in d.tracks.items():
        assert all((l, f, c) in key for f, c in t)
    assert np.all(cnt > 0), "a landmark without observations never reaches the device"
    r = d.roles
    tiny = L <= 17
    if tiny:
        assert r["full"] == list(range(L))
    if d.fixed_frame is not None and L >= 33:
        assert r["fixed_only"] == [3, 7] + list(range(16, 32))
    if short_tracks and not tiny:
        assert len(r["single"]) == 2 and all(cnt[l] == 1 for l in r["single"])
        assert len(r["stereo"]) == 3
        for l in r["stereo"]:
            assert cnt[l] == 2 and len({f for f, _ in d.tracks[l]}) == 1
    elif not tiny:
        assert d.min_obs >= 3
    nB = P - (d.fixed_frame is not None)
    if 2 * nB >= 65:
        assert cnt[r["obs64"][0]] == 64 and ("obs65" not in r or cnt[r["obs65"][0]] == 65)
    if not sparse_pairs:
        assert len(r["full"]) >= 1 and all(cnt[l] == 2 * P for l in r["full"])
    if d.fixed_frame is not None:
        assert len(r["fixed_only"]) in (3, 18) and len(r["fixed_plus_one"]) == 3
        for l in r["fixed_only"]:
            assert {f for f, _ in d.tracks[l]} == {d.fixed_frame}
        for l in r["fixed_plus_one"]:
            assert len({f for f, _ in d.tracks[l]}) == 2 and d.fixed_frame in {f for f, _ in d.tracks[l]}
    assert len(d.outliers) >= 1
    per_pose = np.bincount(spec.obs_frame, minlength=P)
    assert np.all(per_pose > 0), "a pose without observations"
    if wide:
        sl = slots_of(d)
        lists = pair_lists(d)
        nPan = (nB + PANEL - 1) // PANEL
        for pan in range(nPan):
            for l in r["confined%d" % pan]:
                assert {b // PANEL for b in sl[l]} == {pan}
        for l in r["boundary15_16"]:
            assert sl[l] == [15, 16]
        if sparse_pairs:
            assert (nPan - 1, 0) not in lists, "pair (%d, 0) was to stay without entries" % (nPan - 1)
            assert len(lists[(nPan - 1, nPan - 2)]) == 1 and lists[(nPan - 1, nPan - 2)][0][0] == r["single_pair"][0]
            for l in r["two_panels"]:
                assert sl[l] == list(range(2 * PANEL))
        else:
            for l in r["boundary31_32"]:
                assert sl[l] == [31, 32]
            for l in r["two_panels"]:
                assert sl[l] == list(range(PANEL)) + list(range(PANEL * (nPan - 1), nB))
            for l in r["full"]:
                assert sl[l] == list(range(nB))
            assert len(r["comb"]) == n_comb
            for l in r["comb"]:
                assert len(sl[l]) == 17 and sl[l][1:] == list(range(PANEL, 2 * PANEL))


# ------------------------------------------------------------------------------------------------ the case table
# name -> (design arguments, [(debug options, expected SVIN_LAST_SCHUR_FORM)]): kernels.hpp lists the form codes
D9, D9M, D10, D17 = 1090, 1091, 1101, 1171
TILE = dict(SVIN_SCHUR_A_MFMA=1)
PAIR = dict(SVIN_SCHUR_PAIRWISE=1)
OLD = dict(SVIN_PANELS_OLD=1)
CASES = {
    # device landmark counts 1, 15, 16, 17 (one landmark; a chunk less one; one chunk; one chunk and one)
    "narrow_L1": (dict(P=3, L=1, n_outliers=1), [({}, D9), (PAIR, 4000)]),
    "narrow_L15": (dict(P=3, L=15, n_outliers=2), [({}, D9), (PAIR, 4000)]),
    "narrow_L16": (dict(P=3, L=16, n_outliers=2), [({}, D9), (PAIR, 4000)]),
    "narrow_L17": (dict(P=3, L=17, n_outliers=2), [({}, D9), (PAIR, 4000)]),
    "narrow_P3": (dict(P=3, L=49, n_full=3), [({}, D9)]),
    "narrow_P10_fixed": (dict(P=10, L=113, fixed_frame=4), [({}, D9), (PAIR, 4000)]),
    "narrow_P10_min3": (dict(P=10, L=113, short_tracks=False), [({}, D9), (PAIR, 4000)]),
    "narrow_P21": (dict(P=21, L=112), [({}, D9)]),
    "narrow_P22": (dict(P=22, L=111), [({}, D10), (TILE, D10 + 1)]),
    "narrow_B31_fixed": (dict(P=32, L=113, fixed_frame=9), [({}, D10), (TILE, D10 + 1), (PAIR, 4001)]),   # 31 pose blocks: dC = 186
    "narrow_B32_fixed": (dict(P=33, L=113, fixed_frame=7), [({}, D17), (TILE, D17 + 1)]),                 # 32 pose blocks: dC = 192
    "narrow_P42": (dict(P=42, L=209), [({}, D17), (TILE, D17 + 1)]),
    "ext_P6_fixed": (dict(P=6, L=113, rig="test4", fixed_frame=2), [({}, D9M), (TILE, D9M + 1)]),
    "ext_P9_fixed": (dict(P=9, L=113, rig="test4", fixed_frame=3), [({}, D10), (TILE, D10 + 1)]),   # dC = 48 + 108: ten tile rows
    "ext_P64_fixed": (dict(P=64, L=209, rig="test4", n_full=2, fixed_frame=30), [({}, 4001)]),
    "wide_P43_dense": (dict(P=43, L=801, wide=True, n_full=12, n_comb=40), [({}, 2000), (OLD, 3000)]),
    "wide_P48_sparse": (dict(P=48, L=400, wide=True, sparse_pairs=True), [({}, 2000), (OLD, 3000)]),
    "wide_P48_fixed": (dict(P=48, L=401, wide=True, fixed_frame=20, n_full=4), [({}, 2000), (OLD, 3000)]),
    "wide_P48_min3": (dict(P=48, L=401, wide=True, n_full=4, short_tracks=False), [({}, 2000), (OLD, 3000)]),
    "wide_P49_dense": (dict(P=49, L=799, wide=True, n_full=12, n_comb=40), [({}, 2000), (OLD, 3000)]),
    "wide_P64_sparse": (dict(P=64, L=401, wide=True, sparse_pairs=True), [({}, 2000), (OLD, 3000)]),
    "wide_P64_dense": (dict(P=64, L=801, wide=True, fixed_frame=40, n_full=12, n_comb=40), [({}, 2000), (OLD, 3000)]),
}
RESORT_ABOVE = 42   # kResidentPoseCap: with more pose blocks pack() orders the landmarks by the tiles they touch
MI355X_CUS = 256


def build(name):
    return design(**CASES[name][0])
