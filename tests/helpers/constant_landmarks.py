"""Shared pieces of tests/test_gpu_constant_landmarks.py: windows whose landmarks are partly held constant (the way a caller anchors
the sliding window to a map it trusts), for the product and for the oracle alike.  No GPU is needed to import or to run any of this on
oracle estimators -- the fixture counts the tests rely on (how many constant landmarks a marginalisation linearises) are checked that way."""
import numpy as np

from svin_amd import synthetic as syn


def hold_constant(est, lid, constant=True):
    """Map::setParameterBlockConstant / Variable on a landmark, on either kind of estimator"""
    if hasattr(est, "set_parameter_block_constant"):
        assert est.set_parameter_block_constant(int(lid), constant)
    else:
        est.map().set_constant(int(lid), constant)


def cut_tracks(spec, after):
    """drops the observations of the even-indexed landmarks in the frames behind `after`: those landmarks are then seen by old frames
    only, so the marginalisation policy linearises them into the prior when their frames leave (constant ones included)"""
    keep = ~((spec.obs_lm % 2 == 0) & (spec.obs_frame > after))
    for name in ("obs_lm", "obs_frame", "obs_cam", "obs_uv", "obs_size"):
        setattr(spec, name, getattr(spec, name)[keep])
    return spec


def one_shot_window(rig):
    """the two fixtures of the one-marginalisation test"""
    kw = dict(P=8, L=250, n_obs=2500, seed=52, rig=rig, keyframe_every=2, frame_dt=0.3)
    if rig == "rig_v2":
        return syn.make_window(sonar=True, depth=True, **kw)
    return cut_tracks(syn.make_window(**kw), after=4)


def constant_pass(est, spec, snaps=None, iters=12, window=(2, 3), record=True, settle_imu=True):
    """feeds `spec`; in the first frame's callback, ahead of the first optimize, every third landmark is held constant; every frame
    optimises and marginalises.  With `snaps` the states recorded from another estimator are put in place right before each
    marginalisation.  Returns (records, frame ids, ids of the constant landmarks); a record is (snapshot, removed ids, prior,
    frame ids, landmark count, system after M1 or None)."""
    from test_gpu_parity import snapshot_states, inject_states
    rec, const = [], []

    def cb(k, fid):
        if k == 0:
            const.extend(est.landmark_ids()[::3])
            for lid in const:
                hold_constant(est, lid)
        est.optimize(iters)
        if snaps is not None and not settle_imu:
            inject_states(est, snaps[len(rec)])     # (test_marginalization_one_shot's procedure as it is)
        elif snaps is not None:
            # An IMU factor pre-integrates again only when the gyro bias has moved by more than 1e-4 / Delta_t since it last did
            # (ImuError.cpp:738-748); below that it corrects to first order around the biases of THAT evaluation, which the
            # injected states do not determine: they are a product of the estimator's own iterations (on the euroc fixture an
            # oracle that ran optimize(11) instead of optimize(12) ahead of the same injected states ends 1.5e-5 of a standard
            # deviation away: tests/test_constant_landmarks_oracle.py asserts both that and the cure).  So both sides are first evaluated far beyond the threshold -- every factor pre-integrates there --
            # and the recorded states then make every factor pre-integrate once more, at exactly the recorded biases.
            far = dict(snaps[len(rec)], sb={f: (None if v is None else v + np.r_[np.zeros(3), 0.1 * np.ones(3), np.zeros(3)])
                                            for f, v in snaps[len(rec)]["sb"].items()})
            inject_states(est, far)
            est.optimize(0)
            inject_states(est, snaps[len(rec)])
        snap = snapshot_states(est) if record else None
        ok, removed = est.apply_marginalization(*window)
        assert ok, "apply_marginalization failed at frame %d" % k
        rec.append((snap, sorted(int(i) for i in removed), est.marg() if record else None, est.frame_ids(), est.num_landmarks(),
                    est.marg_pre() if record else None))
    frames, _ = syn.feed(est, spec, on_frame=cb)
    return rec, frames, const


class ConstantDriver:
    """the frame script of the resident-against-host-pack test on top of test_gpu_resident.Driver: which landmarks are constant, and
    the edits that take the device-resident window through every case it has to handle"""

    def __init__(self, drv):
        self.drv = drv
        self.const = set()        # landmark indices (keys of drv.lm_ids) that are constant now
        self.gone = set()         # ids of the landmarks the marginalisation has removed

    def set(self, l, constant):
        for e in self.drv.ests:
            hold_constant(e, self.drv.lm_ids[l], constant)
        (self.const.add if constant else self.const.discard)(l)

    def alive(self, l):
        return self.drv.lm_ids[l] not in self.gone

    def prune(self, removed):
        self.gone.update(int(i) for i in removed)
        self.const = {l for l in self.const if self.alive(l)}

    def hold_new(self, known_before):
        """every third landmark the newest frame created: constant before it has ever reached the device"""
        for l in sorted(self.drv.lm_ids):
            if l not in known_before and l % 3 == 0:
                self.set(l, True)

    def remove_some(self, n, newest_only=False):
        """Driver.remove_some for estimators of either kind: the oracle removes by key only (the same records either way)"""
        drv = self.drv
        alive = set(drv.ests[0].frame_ids())
        drv.live = [r for r in drv.live if r[1] in alive]
        pool = [r for r in drv.live if (not newest_only or r[1] == drv.frame_ids[-1])]
        by_id_ok = all(hasattr(e, "remove_observation_by_id") for e in drv.ests)
        for _ in range(min(n, len(pool))):
            r = pool.pop(int(drv.rng.integers(len(pool))))
            drv.live.remove(r)
            if drv.rng.random() < 0.5 or not by_id_ok:
                res = [e.remove_observation(drv.lm_ids[r[0]], r[1], r[2], r[3]) for e in drv.ests]
            else:
                res = [e.remove_observation_by_id(rid) for e, rid in zip(drv.ests, r[4])]
            assert all(x == res[0] for x in res), res

    def remove_from_constant(self, n):
        """tombstones inside constant landmarks: observations of older frames that are on the device already"""
        drv = self.drv
        alive = set(drv.ests[0].frame_ids())
        pool = [r for r in drv.live if r[0] in self.const and r[1] in alive and r[1] != drv.frame_ids[-1]]
        done = 0
        for r in pool[:: max(1, len(pool) // n)][:n]:
            drv.live.remove(r)
            res = [e.remove_observation(drv.lm_ids[r[0]], r[1], r[2], r[3]) for e in drv.ests]
            assert all(x == res[0] for x in res), res
            done += 1 if res[0] else 0
        return done


def constant_observation_mask(est, csr, const_ids):
    """per CSR observation: does it belong to a constant landmark (the CSR lists the landmarks that have observations in handle
    order = creation order = id order here).  `est`: the host-packed estimator (its landmark read-back touches no device table)"""
    lids = [l for l, v in est.get_landmarks().items() if v["n_obs"] > 0]
    assert len(lids) == csr["L"]
    is_const = np.array([l in const_ids for l in lids], bool)
    return is_const[csr["obs_lm"]]


RESIDENT_WINDOW = dict(P=12, L=300, n_obs=3000, seed=9, rig="euroc", keyframe_every=2, frame_dt=0.3)
RESIDENT_CUT_AFTER = 4
RESIDENT_MARG = (3, 3)
# landmarks that come and go in one frame.  Window::flushResident drops the device copy when the handle range exceeds
# max(8192, 8 x landmarks) and then renumbers when it exceeds max(4096, 2 x landmarks): 9 000 is past both; the test asserts on
# Estimator.landmark_handles() that the range was that large at frame 6 and is the landmark count again after frame 7's flush
N_SHORT_LIVED = 9000


class NoChecks:
    def tables(self, k, tag, cd):
        pass

    def solve(self, k, tag, cd, iters):
        for e in cd.drv.ests:
            e.optimize(iters)

    def detour(self, cd, edit):
        edit()

    def marginalised(self, k, results, cd):
        pass


def run_resident_script(ests, spec, checks=None, iters=4, batched=True):
    """The frames of the resident-against-host-pack test.  Every estimator of `ests` receives the same calls; `checks` looks at them
    at the marked points.  The cases: (1) constant before the landmark has reached the device -- every frame;
    (2) constant in a flush that adds and removes nothing -- frames 2, 5, 9; (3) constant -> variable -- frames 3, 5, 10, and 8;
    (4) a constant landmark loses observations that are on the device and gains new ones -- every frame from 2 on; (5) constant
    landmarks erased by the marginalisation -- whenever the policy says so; (6) handle renumbering -- the flush of frame 7;
    (7) resident -> host pack -> resident with flags changed on the way -- frame 8.  Returns the ConstantDriver and, per frame,
    the removed landmark ids of the first estimator."""
    from test_gpu_resident import Driver
    checks = checks or NoChecks()
    drv = Driver(ests, spec, seed=2)
    cd = ConstantDriver(drv)
    removed_per_frame, late = [], []

    def in_window(l):
        return l in drv.lm_ids and cd.alive(l) and any(r[0] == l for r in drv.live)

    for k in range(spec.P):
        known = set(drv.lm_ids)
        drv.add_frame(k, batched=batched and k % 3 != 1)
        cd.hold_new(known)                                   # (1)
        cd.remove_some(4, newest_only=True)
        if k % 2 == 0:
            cd.remove_some(4)
        if k >= 2:
            cd.remove_from_constant(3)                       # (4)
        if k == 6:                                           # (6): the handles run out after this frame's marginalisation
            for _ in range(N_SHORT_LIVED):
                lid = drv.all(lambda e: e.new_id())
                for e in ests:
                    e.add_landmark(lid, np.array([1.0, 2.0, 3.0, 1.0]))
        if k == 7:                                           # ... and these flags travel through the renumbering
            for l in [l for l in sorted(drv.lm_ids) if l % 3 == 2 and in_window(l)][:3]:
                cd.set(l, True)
        if k == 8:                                           # (7)
            def edit():
                for l in [l for l in sorted(cd.const) if in_window(l)][:2]:
                    cd.set(l, False)
                for l in [l for l in sorted(drv.lm_ids) if l % 3 == 2 and l not in cd.const and in_window(l)][:2]:
                    cd.set(l, True)
            checks.detour(cd, edit)
        checks.tables(k, "frame %d" % k, cd)
        checks.solve(k, "frame %d" % k, cd, iters)
        if k in (2, 3, 5, 9, 10):
            if k in (2, 5, 9):                               # (2)
                fresh = [l for l in sorted(drv.lm_ids) if l % 3 == 1 and l not in cd.const and in_window(l)][:4]
                for l in fresh:
                    cd.set(l, True)
                late.extend(fresh)
            if k in (3, 5, 10):                              # (3): some made constant late, one constant from its first frame
                back = [l for l in late if l in cd.const and in_window(l)][:3]
                back += [l for l in sorted(cd.const) if l % 3 == 0 and in_window(l)][:1]
                for l in back:
                    cd.set(l, False)
            checks.tables(k, "frame %d, flags changed and nothing else" % k, cd)
            checks.solve(k, "frame %d, second solve" % k, cd, iters)
        results = [e.apply_marginalization(*RESIDENT_MARG) for e in ests]
        assert all(r[0] for r in results), "frame %d: apply_marginalization failed" % k
        removed_per_frame.append(sorted(int(i) for i in results[0][1]))
        checks.marginalised(k, results, cd)
        cd.prune(results[0][1])
    return cd, removed_per_frame
