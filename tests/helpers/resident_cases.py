"""Designed call sequences for the kernels of the device-resident window (svin_amd/csrc/resident.hip), in the style of
obs_patterns.py: every scenario is a list of steps on a window in which every landmark projects into every frame and camera
(obs_patterns.full_window, built once per frame count and sliced), and carries the edge it is meant to reach.  That edge is asserted
on the script by the model (resident_model.py) before any estimator exists: `Runner(scenario).run()` runs the steps on the model
alone, `scenario.expect(trace)` looks at what the checks saw.  tests/test_gpu_resident_edges.py runs the same steps on a resident
estimator and on a host-packed twin.

Steps:
  ("frame", k)                       add_states of frame k of the window
  ("landmark", key, point)           add_landmark; key: the landmark's index in the window, or ("u", n) for one that is never observed
  ("add", [i, ...])                  add_observations of the window's observation records i, in this order (one batched call)
  ("remove", [i, ...], "key"|"id")   remove_observation / remove_observation_by_id
  ("remove_all",)                    ... of every observation the window holds
  ("set_landmark", key, point)
  ("constant", key, flag)            setParameterBlockConstant on a landmark
  ("constant_pose", k)               ... on the pose of frame k
  ("check", tag)                     debug_csr on both estimators: one flush of the resident window
  ("optimize", n)
  ("marginalise", num_kf, num_imu, dict(remove=, linearised=, new=))   the frame classes (frame indices) are the scenario's design

A: handle_sweep(H, pattern)     k_window_rebuild phases 0-3 over the handle range, k_window_finish / k_window_store_landmarks
B: delta_edges()                consecutive flushes of one window: the delta's corner cases
C: staging_boundary(), order_small(L)   k_window_order at cnt = 1024 | 1025 and at the chunk-count edges
D: marg_gather(L)               k_window_marg_gather over the CSR slots
"""
import functools
from dataclasses import dataclass, field

import numpy as np

import obs_patterns as op
import resident_model as rm


@dataclass
class Scenario:
    name: str
    spec: object
    steps: list
    edge: str                                       # the edge the script is meant to reach, in words
    expect: object = None                           # expect(trace): asserts it on the model's trace
    constant_frames: list = field(default_factory=list)
    info: dict = field(default_factory=dict)


class Window:
    """a full window and the index of its observation records by (landmark, frame, camera); shared between scenarios, never changed"""

    def __init__(self, P, L, rig="euroc", seed=1):
        self.spec = op.full_window(P, L, rig, seed)
        s = self.spec
        self.at = {(int(l), int(f), int(c)): i for i, (l, f, c) in enumerate(zip(s.obs_lm, s.obs_frame, s.obs_cam))}
        assert len(self.at) == s.N == 2 * P * L

    def o(self, l, f, c):
        return self.at[(l, f, c)]


@functools.lru_cache(maxsize=None)
def window(P, L, rig="euroc"):
    return Window(P, L, rig)


def unobserved_point(n):
    return np.array([0.5 + 1e-3 * n, -1.0 + 7e-4 * n, 9.0 + 1e-2 * (n % 13), 1.0])


# ---------------------------------------------------------------------------------------------------------------- the runner
class Runner:
    """runs a scenario's steps on the model and on every estimator of `ests` (none: the model alone)"""

    def __init__(self, sc, ests=()):
        self.sc, self.ests, self.model = sc, list(ests), rm.ResidentModel()
        self.ids, self.frame_ids, self.kp_next, self.live, self.trace = {}, {}, {}, {}, []
        self._next_id = 0
        spec = sc.spec
        for e in self.ests:
            for cam in spec.cameras:
                e.add_camera(cam["model"], cam["intr"], cam["dist"], cam["width"], cam["height"], spec.extr_sigmas)
            e.add_imu(spec.imu_params)
        self.T_SC = np.stack([c["T_SC"] for c in spec.cameras])
        self.imu_sec = spec.imu_t[:, 0].astype(np.float64) - float(spec.imu_t[0, 0]) + 1e-9 * spec.imu_t[:, 1]
        self.frm_sec = spec.stamps[:, 0].astype(np.float64) - float(spec.imu_t[0, 0]) + 1e-9 * spec.stamps[:, 1]

    def new_id(self):
        if not self.ests:
            self._next_id += 1
            return self._next_id
        out = [e.new_id() for e in self.ests]
        assert all(o == out[0] for o in out), out     # one id sequence each: the same calls give the same ids
        return out[0]

    def run(self):
        for step in self.sc.steps:
            getattr(self, "do_" + step[0])(*step[1:])
        return self.trace

    # -- hooks of the GPU test
    def checked(self, tag, flush):
        pass

    def optimized(self, n):
        pass

    def marginalised(self, expected, results, num_kf, num_imu, classes):
        pass

    # -- the steps
    def do_frame(self, k):
        spec = self.sc.spec
        fid = self.new_id()
        self.frame_ids[k] = fid
        margin = 2.5 / spec.imu_params["rate"]
        lo = self.frm_sec[k - 1] - margin if k > 0 else self.frm_sec[0] - margin
        sel = (self.imu_sec >= lo) & (self.imu_sec <= self.frm_sec[k] + margin)
        for e in self.ests:
            assert e.add_states(fid, (int(spec.stamps[k, 0]), int(spec.stamps[k, 1])), 400, self.T_SC, spec.imu_t[sel], spec.imu_meas[sel],
                                bool(spec.keyframe[k]), None, None, spec.first_depth)
            if k > 0:
                e.set_T_WS(fid, spec.T_WS_init[k])
            e.set_speed_and_bias(fid, spec.sb_init[k])

    def do_landmark(self, key, point):
        lid = self.new_id()
        self.ids[key] = lid
        self.model.add_landmark(lid, point)
        for e in self.ests:
            assert e.add_landmark(lid, point)

    def do_add(self, rows):
        spec = self.sc.spec
        rows = [int(i) for i in rows]
        kps = []
        for i in rows:
            assert i not in self.live, "observation record %d is in the window already" % i
            l, f, c = int(spec.obs_lm[i]), int(spec.obs_frame[i]), int(spec.obs_cam[i])
            kp = self.kp_next.get((f, c), 0)
            self.kp_next[(f, c)] = kp + 1
            kps.append(kp)
            self.model.add_observation(self.ids[l], f, c, kp, spec.obs_uv[i], spec.obs_size[i])
            self.live[i] = [kp, []]
        for e in self.ests:
            rids = e.add_observations(np.array([self.ids[int(spec.obs_lm[i])] for i in rows], np.uint64),
                                      np.array([self.frame_ids[int(spec.obs_frame[i])] for i in rows], np.uint64),
                                      spec.obs_cam[rows].astype(np.uint64), np.array(kps, np.uint64), spec.obs_uv[rows], spec.obs_size[rows])
            assert np.all(rids != 0)
            for i, r in zip(rows, rids):
                self.live[i][1].append(int(r))

    def do_remove(self, rows, how="key"):
        spec = self.sc.spec
        for i in rows:
            kp, rids = self.live.pop(int(i))
            l, f, c = int(spec.obs_lm[i]), int(spec.obs_frame[i]), int(spec.obs_cam[i])
            self.model.remove_observation(self.ids[l], f, c, kp)
            for e, r in zip(self.ests, rids):
                assert e.remove_observation_by_id(r) if how == "id" else e.remove_observation(self.ids[l], self.frame_ids[f], c, kp)

    def do_remove_all(self):
        self.do_remove(sorted(self.live), "key")

    def do_set_landmark(self, key, point):
        self.model.set_landmark(self.ids[key], point)
        for e in self.ests:
            assert e.set_landmark(self.ids[key], point)

    def do_constant(self, key, flag):
        self.model.set_constant(self.ids[key], flag)
        for e in self.ests:
            assert e.set_parameter_block_constant(self.ids[key], flag)

    def do_constant_pose(self, k):
        assert k in self.sc.constant_frames
        for e in self.ests:
            hit = [b for b in e.parameter_block_ids() if e.describe_block(b) is not None and e.describe_block(b)[:2] == (self.frame_ids[k], 0)]
            assert len(hit) == 1 and e.set_parameter_block_constant(hit[0])

    def do_check(self, tag):
        flush = self.model.end_flush()
        exp = self.model.expected()
        order = sorted(self.model.lms)
        self.trace.append(dict(kind="check", tag=tag, flush=flush, L=exp["L"], N=exp["N"], H=len(order), lm_ptr=exp["lm_ptr"],
                               occupied=np.array([1 if self.model.lms[i].obs else 0 for i in order], np.int64)))
        self.checked(tag, flush)

    def do_optimize(self, n):
        for e in self.ests:
            e.optimize(n)
        self.optimized(n)

    def do_marginalise(self, num_kf, num_imu, classes):
        before = self.model.expected()
        slot_of = {lid: s for s, lid in enumerate(before["ids"])}
        for e in self.ests:   # the design's frame classes stand on the frames that are there
            assert e.frame_ids() == [self.frame_ids[k] for k in sorted(self.frame_ids)]
        results = [e.apply_marginalization(num_kf, num_imu) for e in self.ests]
        expected = self.model.marginalise(**classes)
        expected["job_slots"] = [slot_of[lid] for lid, _, _ in expected["job"]]
        expected["L_before"], expected["N_before"] = before["L"], before["N"]
        self.trace.append(dict(kind="marginalise", **expected))
        for k in classes["remove"]:
            del self.frame_ids[k]
        for e in self.ests:
            assert e.frame_ids() == [self.frame_ids[k] for k in sorted(self.frame_ids)], "the frames that left are not the design's"
            assert [k for k in sorted(self.frame_ids) if not e.is_in_imu_window(self.frame_ids[k])] == \
                [k for k in classes["linearised"] if k not in classes["remove"]], "the frames outside the IMU window are not the design's"
        self.marginalised(expected, results, num_kf, num_imu, classes)


def checks(trace):
    return [t for t in trace if t["kind"] == "check"]


# ---------------------------------------------------------------------------------------------------------------- A
HANDLE_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 5000)
PATTERNS = ("all", "seventh", "ends")
MAX_ALL = 2049


def handle_cases():
    return [(H, p) for H in HANDLE_COUNTS for p in PATTERNS if not (p == "all" and H > MAX_ALL)]


def observed_handles(H, pattern):
    if pattern == "all":
        return list(range(H))
    if pattern == "seventh":
        return list(range(0, H, 7))
    return sorted(set(range(min(5, H))) | set(range(max(0, H - 5), H)))


def handle_sweep(H, pattern):
    """H landmarks on P = 3 frames of which `pattern` are observed, three observations each (one per frame, cameras alternating:
    obs_patterns.design_three_observations); one full flush, then a solve"""
    win = window(3, MAX_ALL)
    obs = observed_handles(H, pattern)
    slot = {h: j for j, h in enumerate(obs)}
    steps = [("frame", k) for k in range(3)]
    for h in range(H):
        steps.append(("landmark", slot[h], win.spec.lm_init[slot[h]]) if h in slot else ("landmark", ("u", h), unobserved_point(h)))
    for f in range(3):
        steps.append(("add", [win.o(j, f, (j + f) % 2) for j in range(len(obs))]))
    steps += [("check", "full"), ("optimize", 2)]
    flags = np.zeros(H, np.int64)
    flags[obs] = 1

    def expect(trace):
        c = checks(trace)
        assert len(c) == 1 and c[0]["flush"]["full"]
        assert c[0]["H"] == H and np.array_equal(c[0]["occupied"], flags)
        assert (c[0]["L"], c[0]["N"]) == (len(obs), 3 * len(obs))
        r = rm.scan_ranges(H, c[0]["occupied"])
        assert r["per"] == (H + 1023) // 1024 and r["threads_with_items"] == (H + r["per"] - 1) // r["per"]
        if pattern == "ends" and H >= 1023:
            # every interior thread range sums to zero, and so does every wave but the first and the one or two that hold the last five
            inner = [t for t in range(1024) if r["hi"][t] > r["lo"][t] and r["lo"][t] >= 5 and r["hi"][t] <= H - 5]
            assert all(r["thread_sums"][t] == 0 for t in inner) and len(inner) >= r["threads_with_items"] - 10
            assert r["zero_waves"] >= (16 - r["empty_waves"]) - 3 and r["zero_waves"] >= 5
        return r
    return Scenario("A_H%d_%s" % (H, pattern), win.spec, steps,
                    "handle range H = %d (per = %d), occupancy %s" % (H, (H + 1023) // 1024, pattern), expect, info=dict(H=H, observed=obs))


# ---------------------------------------------------------------------------------------------------------------- B
def delta_edges():
    """one window (P = 4, 40 observed landmarks and unobserved ones between them) through consecutive flushes"""
    win = window(4, 40)
    o = win.o
    lm_init = win.spec.lm_init
    steps = [("frame", k) for k in range(4)]
    for l in range(40):
        if l % 4 == 0:
            steps.append(("landmark", ("u", l // 4), unobserved_point(l // 4)))
        steps.append(("landmark", l, lm_init[l]))
    # the first flush is the full one: frame 0 alone; landmarks 30 .. 39 hold a single observation
    steps += [("add", [o(l, 0, 0) for l in range(40)] + [o(l, 0, 1) for l in range(30)]), ("check", "full")]
    # many additions per flush: two frames of observations plus extra ones on the old frames, to the same landmarks.  The additions of
    # a landmark lie far apart in the flush's list (frame 2's, frame 3's, then the old frames'), on both sides of position Nold = 70:
    # the threads below it first move a surviving observation, the ones above start on their addition at once
    many = [o(l, 2, c) for l in range(36) for c in (0, 1)]
    many += [o(l, 3, 0) for l in range(36)] + [o(l, 3, 1) for l in range(10, 36)]
    many += [o(l, 1, c) for l in range(36) for c in (0, 1)] + [o(l, 0, 1) for l in range(30, 36)]
    steps += [("add", many), ("check", "many additions")]
    # removals inside a segment: the first, the last, one in the middle, first and last together, and the only observation of a segment
    steps += [("remove", [o(0, 0, 0)], "key"), ("remove", [o(1, 1, 1)], "id"), ("remove", [o(12, 3, 0)], "id"),
              ("remove", [o(13, 0, 0), o(13, 1, 1)], "key"), ("remove", [o(36, 0, 0)], "key"), ("check", "removals")]
    # removal and addition on one landmark in one flush; a landmark that had lost its only observation comes back
    steps += [("remove", [o(2, 2, 0)], "key"), ("add", [o(2, 3, 1), o(36, 1, 0)]), ("check", "removal and addition")]
    steps += [("optimize", 2), ("check", "after a solve")]
    # an addition withdrawn before it was ever flushed: alone in its flush, then next to an addition that stays and a removal
    steps += [("add", [o(3, 3, 1)]), ("remove", [o(3, 3, 1)], "key"), ("check", "withdrawn addition alone")]
    steps += [("add", [o(4, 3, 1), o(5, 3, 1)]), ("remove", [o(5, 3, 1)], "id"), ("remove", [o(6, 0, 0)], "key"), ("check", "withdrawn addition")]
    steps += [("remove_all",), ("check", "every observation removed")]
    steps += [("add", [o(7, 0, 0)]), ("check", "one again")]
    refill = [o(l, f, c) for f in range(4) for l in range(30) for c in (0, 1) if (l, f, c) != (7, 0, 0)]
    steps += [("add", refill), ("check", "refilled")]
    # a flush with nothing added or removed: new landmarks without observations, a landmark set by the host
    steps += [("landmark", ("u", 10 + n), unobserved_point(10 + n)) for n in range(3)]
    steps += [("set_landmark", 8, lm_init[8] + np.array([1e-3, -2e-3, 1e-3, 0.0])), ("check", "values only")]
    steps += [("constant", 9, True), ("check", "constant set"), ("constant", 9, False), ("check", "constant cleared")]
    steps += [("optimize", 3), ("check", "end")]

    def expect(trace):
        c = {t["tag"]: t for t in checks(trace)}
        assert c["full"]["flush"]["full"] and c["full"]["N"] == 70
        f = c["many additions"]["flush"]
        assert not f["full"] and max(len(v) for v in f["adds"].values()) >= 6
        nold = c["full"]["N"]
        assert sum(1 for v in f["adds"].values() if len(v) >= 6 and v[0] < nold < v[-1]) >= 20, "additions of one landmark on both sides of Nold"
        rem = c["removals"]["flush"]["removed"]
        pos = sorted(p for v in rem.values() for p in v)
        assert any(p == 0 and n > 1 for p, n in pos) and any(p == n - 1 and n > 1 for p, n in pos), "first and last of a segment"
        assert any(0 < p < n - 1 for p, n in pos) and (0, 1) in pos, "the middle and the only observation of a segment"
        assert c["removals"]["L"] == c["many additions"]["L"] - 1
        f = c["removal and addition"]["flush"]
        assert set(f["adds"]) & set(f["removed"]), "removal and addition on one landmark"
        f = c["withdrawn addition alone"]["flush"]
        assert f["withdrawn"] == 1 and f["n_adds"] == 1 and not f["removed"] and not f["values_only"]
        assert (c["withdrawn addition alone"]["L"], c["withdrawn addition alone"]["N"]) == (c["after a solve"]["L"], c["after a solve"]["N"])
        assert c["withdrawn addition"]["flush"]["withdrawn"] == 1 and c["withdrawn addition"]["flush"]["n_adds"] == 2
        z = c["every observation removed"]
        assert (z["L"], z["N"]) == (0, 0) and z["H"] == 50
        assert (c["one again"]["L"], c["one again"]["N"]) == (1, 1)
        f = c["values only"]["flush"]
        assert f["values_only"] and f["new_landmarks"] == 3 and f["set_landmarks"] == 1 and c["values only"]["H"] == 53
        for tag in ("constant set", "constant cleared", "after a solve", "end"):
            assert c[tag]["flush"]["values_only"], tag
        assert c["constant set"]["flush"]["const_changes"] == 1
    return Scenario("B_delta_edges", win.spec, steps, "the corner cases of one flush's delta, one per check", expect)


# ---------------------------------------------------------------------------------------------------------------- C
def staging_boundary():
    """euroc, P = 33 with one constant pose (32 pose blocks: dC = 192, 13 tile rows -> the ordered dense form), 40 landmarks:
    chunk 0 holds 16 x 64 = 1 024 observations (the last staged size), chunk 1 15 x 64 + 65 = 1 025 (the first unstaged one),
    chunk 2 is partial: 8 landmarks with full tracks of 66.  The observations are added in a seeded random order, so the pose
    slots inside a landmark are unsorted and every pose occurs many times in a chunk; no solve ahead of the check"""
    P, fixed = 33, 7
    win = window(P, 40)
    both = lambda fs: [(f, c) for f in fs for c in (0, 1)]
    tracks = {}
    for l in range(32):   # 32 of the 33 frames, the one left out differs from landmark to landmark
        tracks[l] = both([f for f in range(P) if f != (5 * l + fixed) % P])
    tracks[21] = tracks[21] + [((5 * 21 + fixed) % P, 1)]
    for l in range(32, 40):
        tracks[l] = both(range(P))
    rows = [win.o(l, f, c) for l, t in tracks.items() for f, c in t]
    rng = np.random.Generator(np.random.PCG64(33))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    steps = [("frame", k) for k in range(P)] + [("constant_pose", fixed)]
    steps += [("landmark", l, win.spec.lm_init[l]) for l in range(40)]
    steps += [("add", rows[i:i + 500]) for i in range(0, len(rows), 500)] + [("check", "full")]

    def expect(trace):
        c = checks(trace)[0]
        assert rm.chunk_counts(c["lm_ptr"]) == [1024, 1025, 528]
    return Scenario("C_staging_boundary", win.spec, steps, "k_window_order: chunks of 1 024 (staged), 1 025 (unstaged) and a partial one",
                    expect, constant_frames=[fixed], info=dict(tracks=tracks))


ORDER_SMALL = (1, 16, 17)


def order_small(L):
    """rig_v2 (variable extrinsics: the order is wanted at any P), P = 4, full tracks: one landmark, one chunk, one chunk and one"""
    win = window(4, 17, "rig_v2")
    rows = [win.o(l, f, c) for f in (2, 0, 3, 1) for l in range(L) for c in (1, 0)]
    steps = [("frame", k) for k in range(4)] + [("landmark", l, win.spec.lm_init[l]) for l in range(L)] + [("add", rows), ("check", "full")]

    def expect(trace):
        c = checks(trace)[0]
        assert rm.chunk_counts(c["lm_ptr"]) == [8 * min(16, L - 16 * k) for k in range((L + 15) // 16)]
    return Scenario("C_rig_v2_L%d" % L, win.spec, steps, "k_window_order with variable extrinsics, %d landmark(s)" % L, expect)


# ---------------------------------------------------------------------------------------------------------------- D
GATHER_COUNTS = (40, 1023, 1024, 1025, 2049)
# euroc, P = 6, every frame a keyframe, applyMarginalizationStrategy(3, 2): the IMU window keeps frames 4 and 5; of the four frames
# outside it the three newest keyframes 3, 2, 1 stay and frame 0 leaves; "new" is every frame not older than frame 3, the newest
# frame outside the IMU window (Estimator.cpp:668, :695)
MARG_CALL = (3, 2, dict(remove=[0], linearised=[0, 1, 2, 3], new=[3, 4, 5]))
KIND_TRACKS = {
    # (i) seen by the leaving frame, two or more observations outside the IMU window, none new -> linearised, the landmark marginalised
    # (two cameras in every track: between consecutive frames alone the window's baseline is a few centimetres)
    "lin": [[(0, 0), (0, 1)], [(0, 0), (1, 1)], [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)], [(0, 1), (2, 0), (2, 1)]],
    # (ii) the same with one such observation -> removed, not in the job
    "one": [[(0, 0)], [(0, 1)]],
    # (iii) seen by the leaving frame and a new one -> only the leaving observations go
    "new": [[(0, 0), (0, 1), (1, 0), (4, 0), (5, 1)], [(0, 1), (3, 0)], [(0, 0), (2, 1), (3, 1), (4, 1)]],
    # (iv) not seen by the leaving frame -> skipped
    "skip": [[(1, 0), (2, 0), (3, 1)], [(4, 0), (5, 0)], [(1, 1), (1, 0)]],
}


def gather_kind(s, L):
    """kind of CSR slot s.  Runs of three job landmarks (i) (v) (i) lie across every sixteenth thread-range boundary of the scan
    (per = ceil(L / 1024) slots per thread); between the runs the kinds alternate; from 1 023 slots on, the slots of waves 2 and 3
    hold no job landmark; the last slot holds one"""
    per = (L + 1023) // 1024
    if L >= 1023 and (s // per) // 64 in (2, 3):
        return ("one", "new", "skip")[s % 3]
    R = 16 * per
    if s % R == R - 1 or s % R == 1 or s == L - 1:
        return "lin"
    if s % R == 0:
        return "const"
    return ("one", "new", "skip", "lin")[s % 4]


def marg_gather(L):
    win = window(6, max(GATHER_COUNTS))
    assert bool(np.all(win.spec.keyframe))
    kinds = [gather_kind(s, L) for s in range(L)]
    tracks = {}
    for s, k in enumerate(kinds):
        v = KIND_TRACKS["lin" if k == "const" else k]
        tracks[s] = v[(s // 3) % len(v)]
    steps = [("frame", k) for k in range(6)]
    n_un = 0
    for s in range(L):
        if s % 5 == 2:   # unobserved handles in between: slots differ from handles
            steps.append(("landmark", ("u", n_un), unobserved_point(n_un)))
            n_un += 1
        steps.append(("landmark", s, win.spec.lm_init[s]))
    for f in range(6):
        steps.append(("add", [win.o(s, f, c) for s in range(L) for ff, c in tracks[s] if ff == f]))
    steps += [("constant", s, True) for s in range(L) if kinds[s] == "const"]
    steps += [("check", "before"), ("optimize", 2), ("marginalise",) + MARG_CALL, ("check", "after")]

    def expect(trace):
        c = {t["tag"]: t for t in checks(trace)}
        m = [t for t in trace if t["kind"] == "marginalise"][0]
        assert c["before"]["L"] == L and c["before"]["H"] == L + n_un and n_un >= L // 5
        want_job = [s for s in range(L) if kinds[s] in ("lin", "const")]
        assert m["job_slots"] == want_job and all(kinds.count(k) > 0 for k in ("lin", "const", "one", "new", "skip"))
        assert [cst for _, _, cst in m["job"]] == [kinds[s] == "const" for s in want_job]
        assert m["n_job_obs"] == sum(len(tracks[s]) for s in want_job)
        assert len(m["removed"]) == n_un + len(want_job) + kinds.count("one")
        assert m["n_removed_obs"] == m["n_job_obs"] + kinds.count("one") + sum(sum(1 for f, _ in tracks[s] if f == 0) for s in range(L) if kinds[s] == "new")
        assert c["after"]["L"] == kinds.count("new") + kinds.count("skip") and c["after"]["N"] == m["N_before"] - m["n_removed_obs"]
        flags = np.zeros(L, np.int64)
        flags[want_job] = 1
        r = rm.scan_ranges(L, flags)
        crossing = [s for s in range(L - 1) if (s + 1) % r["per"] == 0 and flags[s] and flags[s + 1]]
        assert len(crossing) >= 2, "runs of job landmarks across thread-range boundaries"
        if L >= 1023:
            assert r["zero_waves"] >= 2, "two whole waves of slots without a job landmark"
        return r
    return Scenario("D_L%d" % L, win.spec, steps, "k_window_marg_gather over %d CSR slots (per = %d)" % (L, (L + 1023) // 1024), expect,
                    info=dict(kinds=kinds, tracks=tracks, n_unobserved=n_un))
