"""What the observation CSR of a sliding window must be, stated from the calls that were made.

A plain restatement for tests/test_gpu_resident_edges.py: it is fed the calls an estimator receives (add_landmark, add_observation,
remove_observation, set_landmark, setParameterBlockConstant on a landmark, the landmark pass of applyMarginalizationStrategy) and
answers the arrays Estimator.debug_csr() has to return.  It imports nothing of the product and keeps no handle table -- landmark ids
grow with creation, so "creation order", "handle order" and "id order" are one order, renumbered or not:

  lm_ptr / obs_lm   the landmarks with at least one observation in id order, the observations of a landmark in insertion order
  uv / lm           copies of what was passed in
  w                 |w| = sqrt(64 / size^2); w < 0 exactly on the observations of a constant landmark
  obs_idx >> 24     the camera of the record
  obs_idx & 0xfff   pose slot, (obs_idx >> 12) & 0xfff extrinsics slot.  Which slot a block gets is Window::pack()'s business, so they
                    are held to a consistency rule: frame -> pose slot is single-valued over the window and injective on the variable
                    poses; (frame, camera) -> extrinsics slot is single-valued
  obs_order         all -1 (the window does not take the ordered dense form), or: within every chunk of 16 consecutive CSR landmarks
                    the STABLE sort of the chunk's observation indices by pose slot, a permutation of 0 .. N-1 as a whole

The landmark pass of the marginalisation policy (okvis_ceres/src/Estimator.cpp:671-766) is restated in marginalise(): its inputs are
the three frame sets of the call, which a scenario fixes by design (selectMargFrames has its own test, tests/test_marg_plan_host.py).
"""
import numpy as np

CHUNK = 16            # landmarks per chunk of the dense Schur kernels
REBUILD_THREADS = 1024   # threads of the single workgroup that scans the handles / the CSR slots
WAVE = 64


class Obs:
    __slots__ = ("frame", "cam", "kp", "uv", "size")

    def __init__(self, frame, cam, kp, uv, size):
        self.frame, self.cam, self.kp, self.size = int(frame), int(cam), int(kp), float(size)
        self.uv = np.array(uv, np.float64)


class Lm:
    __slots__ = ("point", "constant", "obs")

    def __init__(self, point):
        self.point, self.constant, self.obs = np.array(point, np.float64), False, []


class ResidentModel:
    def __init__(self):
        self.lms = {}            # landmark id -> Lm
        self.flush = self._new_flush()
        self.n_flushes = 0

    # ------------------------------------------------------------------------------------------------ the calls
    @staticmethod
    def _new_flush():
        # what happened since the last check: per landmark the positions of its additions in the flush's list of additions
        # (withdrawn ones keep their place) and its removals of observations that an earlier flush has seen
        return dict(adds={}, n_adds=0, withdrawn=0, removed={}, new_landmarks=0, set_landmarks=0, const_changes=0, fresh=set())

    def add_landmark(self, lid, point):
        assert lid not in self.lms and (not self.lms or lid > max(self.lms)), "landmark ids grow with creation"
        self.lms[lid] = Lm(point)
        self.flush["new_landmarks"] += 1

    def set_landmark(self, lid, point):
        self.lms[lid].point = np.array(point, np.float64)
        self.flush["set_landmarks"] += 1

    def set_constant(self, lid, flag):
        self.lms[lid].constant = bool(flag)
        self.flush["const_changes"] += 1

    def add_observation(self, lid, frame, cam, kp, uv, size):
        lm = self.lms[lid]
        assert all((o.frame, o.cam, o.kp) != (frame, cam, kp) for o in lm.obs), "duplicate observation"
        o = Obs(frame, cam, kp, uv, size)
        lm.obs.append(o)
        f = self.flush
        f["adds"].setdefault(lid, []).append(f["n_adds"])
        f["n_adds"] += 1
        f["fresh"].add(id(o))

    def remove_observation(self, lid, frame, cam, kp):
        lm = self.lms[lid]
        at = [i for i, o in enumerate(lm.obs) if (o.frame, o.cam, o.kp) == (frame, cam, kp)]
        assert len(at) == 1, "no such observation"
        o = lm.obs.pop(at[0])
        f = self.flush
        if id(o) in f["fresh"]:
            f["withdrawn"] += 1       # never reached a flush
            f["fresh"].discard(id(o))
        else:
            f["removed"].setdefault(lid, []).append((at[0], len(lm.obs) + 1))   # (position, segment length at that moment)
        return o

    def update_points(self, points):
        """after a solve the points are the solver's: {id: point} read back from an estimator"""
        for lid, p in points.items():
            self.lms[lid].point = np.array(p, np.float64)

    # ------------------------------------------------------------------------------------------------ the expected CSR
    def observed(self):
        return [lid for lid in sorted(self.lms) if self.lms[lid].obs]

    def expected(self):
        """the arrays of the CSR and, per record, its frame and camera"""
        ids = self.observed()
        L = len(ids)
        cnt = [len(self.lms[i].obs) for i in ids]
        N = int(sum(cnt))
        lm_ptr = np.zeros(L + 1, np.int32)
        lm_ptr[1:] = np.cumsum(cnt)
        obs = [(s, o, self.lms[i].constant) for s, i in enumerate(ids) for o in self.lms[i].obs]
        w = np.array([np.sqrt(64.0 / (o.size * o.size)) * (-1.0 if c else 1.0) for _, o, c in obs], np.float64).reshape(N)
        return dict(L=L, N=N, ids=ids, lm_ptr=lm_ptr, obs_lm=np.array([s for s, _, _ in obs], np.int32).reshape(N),
                    uv=np.array([o.uv for _, o, _ in obs], np.float64).reshape(N, 2), w=w,
                    lm=np.array([self.lms[i].point for i in ids], np.float64).reshape(L, 4),
                    frame=np.array([o.frame for _, o, _ in obs], np.int64).reshape(N),
                    cam=np.array([o.cam for _, o, _ in obs], np.int64).reshape(N))

    def end_flush(self):
        """closes the delta of one check and returns its description"""
        f, self.flush = self.flush, self._new_flush()
        del f["fresh"]
        f["full"] = self.n_flushes == 0
        f["values_only"] = not f["full"] and f["n_adds"] == 0 and not f["removed"]
        self.n_flushes += 1
        return f

    def check_csr(self, csr, constant_frames=(), tag=""):
        """asserts that a debug_csr() answer is the CSR of the calls made so far; returns True when obs_order is the ordered form"""
        e = self.expected()
        assert (csr["L"], csr["N"]) == (e["L"], e["N"]), "%s: L, N = %s, the calls give %s" % (tag, (csr["L"], csr["N"]), (e["L"], e["N"]))
        for k in ("lm_ptr", "obs_lm", "uv", "w", "lm"):
            assert csr[k].shape == e[k].shape and np.array_equal(csr[k], e[k]), "%s: %s is not what the calls give" % (tag, k)
        idx = np.asarray(csr["obs_idx"], np.uint32)
        assert np.array_equal((idx >> 24).astype(np.int64), e["cam"]), "%s: camera index" % tag
        check_slots(idx, e["frame"], e["cam"], constant_frames, tag)
        return check_obs_order(idx, csr["lm_ptr"], csr["obs_order"], tag)

    # ------------------------------------------------------------------------------------------------ marginalisation
    def marginalise(self, remove, linearised, new):
        """the landmark pass of applyMarginalizationStrategy for the frame id sets `remove` (the frames that leave), `linearised`
        (every frame outside the IMU window) and `new` (ids not older than the newest of those).  Applies it to the model and returns
        dict(removed: the removed landmark ids in id order, job: [(id, [frames of its linearised observations], constant)] in id
        order, n_job_obs, n_removed_obs)"""
        remove, linearised, new = set(remove), set(linearised), set(new)
        removed, job, n_removed_obs = [], [], 0
        for lid in sorted(self.lms):
            lm = self.lms[lid]
            if not lm.obs:                                   # :706-711
                removed.append(lid)
                continue
            skip = not any(o.frame in remove for o in lm.obs)              # :692-694
            has_new = any(o.frame in new for o in lm.obs)                  # :695-698
            marg = not has_new
            obs_count = sum(1 for o in lm.obs if o.frame in linearised)    # :699-702
            if skip:
                continue
            stay, lin = [], []
            for o in lm.obs:                                               # :719-748
                if (o.frame in remove and has_new) or (o.frame not in linearised and marg):
                    continue
                if marg and o.frame in linearised:
                    if obs_count >= 2:
                        lin.append(o)
                    continue
                stay.append(o)
            n_removed_obs += len(lm.obs) - len(stay)
            lm.obs = stay
            if lin:
                job.append((lid, [o.frame for o in lin], lm.constant))
            if (not stay and not lin) or (marg and lin):                   # :750-762
                assert not stay
                removed.append(lid)
        for lid in removed:
            del self.lms[lid]
        return dict(removed=removed, job=job, n_job_obs=sum(len(fr) for _, fr, _ in job), n_removed_obs=n_removed_obs)


def check_slots(obs_idx, frame, cam, constant_frames=(), tag=""):
    """the consistency rule of the slot fields"""
    pose = (np.asarray(obs_idx, np.uint32) & 0xfff).astype(np.int64)
    ext = ((np.asarray(obs_idx, np.uint32) >> 12) & 0xfff).astype(np.int64)
    slot_of, ext_of = {}, {}
    for p, x, f, c in zip(pose.tolist(), ext.tolist(), np.asarray(frame).tolist(), np.asarray(cam).tolist()):
        assert slot_of.setdefault(f, p) == p, "%s: frame %d has the pose slots %d and %d" % (tag, f, slot_of[f], p)
        assert ext_of.setdefault((f, c), x) == x, "%s: frame %d camera %d has the extrinsics slots %d and %d" % (tag, f, c, ext_of[(f, c)], x)
    variable = [p for f, p in slot_of.items() if f not in set(constant_frames)]
    assert len(set(variable)) == len(variable), "%s: two variable poses share a slot" % tag


def expected_obs_order(obs_idx, lm_ptr):
    pose = (np.asarray(obs_idx, np.uint32) & 0xfff).astype(np.int64)
    L = len(lm_ptr) - 1
    out = np.zeros(len(pose), np.int32)
    for c in range((L + CHUNK - 1) // CHUNK):
        beg, end = int(lm_ptr[CHUNK * c]), int(lm_ptr[min(L, CHUNK * c + CHUNK)])
        out[beg:end] = beg + np.argsort(pose[beg:end], kind="stable")
    return out


def check_obs_order(obs_idx, lm_ptr, obs_order, tag=""):
    """False: obs_order is all -1 (no order was wanted).  Otherwise it has to be the stable per-chunk sort by pose slot"""
    order = np.asarray(obs_order)
    N = len(order)
    if N == 0 or np.all(order == -1):
        return False
    assert np.array_equal(np.sort(order), np.arange(N)), "%s: obs_order is not a permutation of 0 .. N-1" % tag
    want = expected_obs_order(obs_idx, lm_ptr)
    bad = np.nonzero(order != want)[0]
    assert len(bad) == 0, "%s: obs_order is not the stable sort by pose slot inside its chunks (first at %d: %d, wanted %d; %d differ)" % (
        tag, bad[0] if len(bad) else -1, order[bad[0]] if len(bad) else -1, want[bad[0]] if len(bad) else -1, len(bad))
    return True


def chunk_counts(lm_ptr):
    L = len(lm_ptr) - 1
    return [int(lm_ptr[min(L, CHUNK * c + CHUNK)] - lm_ptr[CHUNK * c]) for c in range((L + CHUNK - 1) // CHUNK)]


def scan_ranges(n, flags):
    """how n items (handles or CSR slots) with the 0/1 `flags` fall onto the 1 024 threads of the scan: dict(per, the number of
    threads with items, the threads whose items are all unflagged, the number of whole 64-thread waves that have items but no flagged
    one, and of waves without items)"""
    flags = np.asarray(flags, np.int64)
    assert len(flags) == n
    per = (n + REBUILD_THREADS - 1) // REBUILD_THREADS
    lo = np.minimum(n, np.arange(REBUILD_THREADS) * per)
    hi = np.minimum(n, lo + per)
    csum = np.r_[0, np.cumsum(flags)]
    mine = csum[hi] - csum[lo]
    has = hi > lo
    w_has = has.reshape(-1, WAVE).any(1)
    w_sum = mine.reshape(-1, WAVE).sum(1)
    return dict(per=per, threads_with_items=int(has.sum()), zero_threads=int((has & (mine == 0)).sum()),
                zero_waves=int((w_has & (w_sum == 0)).sum()), empty_waves=int((~w_has).sum()), thread_sums=mine, lo=lo, hi=hi)
