"""Digest of what the marginalisation computes, for comparing two builds of the library bit for bit.

    python tools/marg_digest.py run OUT.npz                      runs the scenarios below on the GPU and writes every result
    python tools/marg_digest.py compare A1.npz A2.npz B.npz [REPORT.txt]
                                                                 A1, A2: two runs of the reference build, B: the build under test

Per marginalisation a scenario records the `removed` list, the frame ids and the landmark count, marg()'s n, H, b0, J, e0 and
block table, marg_pre() where SVIN_MARG_KEEP_PRE is on; at its end path_counters() and every pose, speed / bias block and
landmark.  M1 accumulates in a fixed order, so two runs of one build agree bit for bit; `compare` holds B to A1 in every scenario
in which A1 and A2 agree, and names the others.  The scenarios are the smallest shapes of the tests that reach each branch of
Window::applyMarginalizationStrategy (marg.hip)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EUROC = dict(P=7, L=150, n_obs=1500, seed=9, rig="euroc", keyframe_every=2, frame_dt=0.3)
RIG_V2 = dict(P=9, L=200, n_obs=2000, seed=45, rig="rig_v2", sonar=True, depth=True, keyframe_every=2, frame_dt=0.3)
TEST4 = dict(P=6, L=150, n_obs=1500, seed=12, rig="test4", keyframe_every=2, frame_dt=0.3)
WIDE = dict(P=46, L=400, n_obs=5000, seed=31, frame_dt=0.3)
LOSS_NONE, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2


class Recorder:
    def __init__(self, est, out, name):
        self.est, self.out, self.name, self.calls = est, out, name, 0

    def put(self, key, value):
        self.out["%s/%s" % (self.name, key)] = np.asarray(value)

    def marginalise(self, num_kf, num_imu):
        est, k = self.est, self.calls
        try:
            ok, removed = est.apply_marginalization(num_kf, num_imu)
        except RuntimeError as e:
            ok, removed = False, []
            self.put("call%d/refused" % k, np.frombuffer(str(e).encode(), np.uint8))
        self.calls += 1
        self.put("call%d/ok" % k, int(bool(ok)))
        self.put("call%d/removed" % k, np.array([int(i) for i in removed], np.uint64))   # (in the order the library returns them)
        self.put("call%d/frames" % k, np.array(est.frame_ids(), np.uint64))
        self.put("call%d/num_landmarks" % k, est.num_landmarks())
        m = est.marg()
        self.put("call%d/prior_n" % k, 0 if m is None else m["n"])
        if m is not None:
            for key in ("H", "b0", "J", "e0"):
                self.put("call%d/prior_%s" % (k, key), m[key])
            self.put("call%d/prior_blocks" % k, np.array([[b["id"], b["ordering"], b["mdim"]] for b in m["blocks"]], np.int64))
            self.put("call%d/prior_lin" % k, np.array([b["lin"] for b in m["blocks"]]))
        if est.debug_get_option("SVIN_MARG_KEEP_PRE"):
            p = est.marg_pre()
            if p is not None:
                self.put("call%d/pre_H" % k, p["H"])
                self.put("call%d/pre_b0" % k, p["b0"])
                self.put("call%d/pre_dense" % k, np.array(p["dense"], np.int64).reshape(-1, 2))
                self.put("call%d/pre_rows" % k, np.array([[i] + list(r) for i, r in sorted(p["rows_of"].items())], np.int64))
        return ok

    def finish(self):
        est = self.est
        est.wait_idle()
        pc = est.path_counters()
        self.put("path_counters", np.array([pc[k] for k in sorted(pc)], np.int64))
        frames = est.frame_ids()
        self.put("final_T_WS", np.array([est.get_T_WS(f) for f in frames]))
        sb = [est.get_speed_and_bias(f) for f in frames]
        self.put("final_speed_bias", np.array([np.full(9, np.nan) if v is None else v for v in sb]))
        lms = est.get_landmarks()
        self.put("final_landmark_ids", np.array(sorted(lms), np.uint64))
        self.put("final_landmarks", np.array([lms[i]["point"] for i in sorted(lms)]).reshape(-1, 4))
        self.put("calls", self.calls)


def slide(out, name, make, marg=(2, 2), start=0, chain=None, iters=4, frames=None, pack_mode=None, options=(), at_frame=None,
          repeat_last=False):
    """feeds the window; from frame `start` on optimize(iters) + apply_marginalization(*marg) per frame, until `chain` of them have
    left a prior (None: every frame).  at_frame(est, k, fids): edits ahead of frame k's optimize."""
    from svin_amd import synthetic as syn
    from svin_amd.estimator import Estimator
    saved = {o: Estimator.debug_get_option(o) for o, _ in options}
    for o, v in options:
        Estimator.debug_set_option(o, v)
    try:
        est = Estimator(0)
        if pack_mode is not None:
            est.set_pack_mode(pack_mode)
        rec = Recorder(est, out, name)
        fids, state = [], dict(priors=0)

        def on_frame(k, fid):
            fids.append(fid)
            if at_frame is not None:
                at_frame(est, k, fids)
            if k < start or (chain is not None and state["priors"] >= chain):
                return
            est.optimize(iters)
            rec.marginalise(*marg)
            if est.marg() is not None:
                state["priors"] += 1
        syn.feed(est, syn.make_window(**make), on_frame=on_frame, frames=frames)
        if repeat_last:   # nothing new to marginalise: the dense part is the old prior alone, every row of it stays
            rec.marginalise(*marg)
        rec.finish()
    finally:
        for o, v in saved.items():
            Estimator.debug_set_option(o, v)


def general_information(est, k, fids):
    if k != 2:
        return
    ev = est.eval_reprojection()
    for j in range(0, len(ev["res_id"]), 3):
        rid = int(ev["res_id"][j])
        w2 = est.map_get_reprojection_information(rid)[0, 0]
        assert est.map_set_reprojection_information(rid, np.array([[2.0, 0.3], [0.3, 1.0]]) * w2)


def losses(est, k, fids):
    if k != 2:
        return
    ev = est.eval_reprojection()
    for j in range(0, len(ev["res_id"]), 2):
        kind, a = ((LOSS_HUBER, 0.7), (LOSS_CAUCHY, 1.5))[(j // 2) % 2]
        assert est.map_set_residual_loss(int(ev["res_id"][j]), kind, a)


def constant_landmarks(est, k, fids):
    if k != 0:
        return
    lids = est.landmark_ids()
    rng = np.random.default_rng(4)
    for lid in rng.choice(lids, size=(3 * len(lids)) // 10, replace=False):
        assert est.set_parameter_block_constant(int(lid), True)


def landmark_prior(est, k, fids):
    if k != 3:
        return
    for lid in est.landmark_ids():   # a landmark the oldest frame (which (2, 2) lets go at this frame) observes
        if any(o[0] == fids[0] for o in est.landmark_observations(lid)):
            assert est.add_homogeneous_point_error(int(lid), np.array([1.0, 2.0, 3.0, 1.0]), np.eye(3))
            return
    raise AssertionError("no landmark is seen from the first frame")


SCENARIOS = [
    ("euroc_resident", lambda o, n: slide(o, n, EUROC)),
    ("euroc_host_pack", lambda o, n: slide(o, n, EUROC, pack_mode=1)),
    ("rig_v2_chain3", lambda o, n: slide(o, n, RIG_V2, chain=3)),
    ("test4_chain2", lambda o, n: slide(o, n, TEST4, chain=2)),
    ("euroc_general_information", lambda o, n: slide(o, n, EUROC, at_frame=general_information)),
    ("euroc_losses", lambda o, n: slide(o, n, EUROC, at_frame=losses)),
    ("euroc_constant_landmarks", lambda o, n: slide(o, n, EUROC, at_frame=constant_landmarks)),
    ("euroc_eig_direct", lambda o, n: slide(o, n, EUROC, options=(("SVIN_MARG_EIG", 1),))),
    ("euroc_eig_cholesky", lambda o, n: slide(o, n, EUROC, options=(("SVIN_MARG_EIG", 2),))),
    ("euroc_eig_jacobi", lambda o, n: slide(o, n, EUROC, options=(("SVIN_MARG_EIG", 3),))),
    ("euroc_keep_pre", lambda o, n: slide(o, n, EUROC, options=(("SVIN_MARG_KEEP_PRE", 1),))),
    ("euroc_sync_enqueue", lambda o, n: slide(o, n, EUROC, options=(("SVIN_MARG_SYNC_ENQUEUE", 1),))),
    ("wide_P46", lambda o, n: slide(o, n, WIDE, marg=(40, 3), start=44, chain=1, iters=3, frames=45)),
    # the three windows above once more with optimize(0): with variable extrinsics or a wide window the solves between the
    # marginalisations add with atomics and are not reproducible run to run; without steps the marginalisations see the same states
    ("rig_v2_chain3_no_steps", lambda o, n: slide(o, n, RIG_V2, chain=3, iters=0)),
    ("test4_chain2_no_steps", lambda o, n: slide(o, n, TEST4, chain=2, iters=0)),
    ("wide_P46_no_steps", lambda o, n: slide(o, n, WIDE, marg=(40, 3), start=44, chain=1, iters=0, frames=45)),
    ("fewer_frames_than_imu_window", lambda o, n: slide(o, n, EUROC, marg=(2, 4), frames=3)),
    ("landmark_prior_refused", lambda o, n: slide(o, n, EUROC, at_frame=landmark_prior, frames=4)),
    ("no_dense_row_marginalised", lambda o, n: slide(o, n, EUROC, repeat_last=True)),
]


def run(path):
    out = {}
    for name, fn in SCENARIOS:
        fn(out, name)
        print("%-32s %d marginalisations" % (name, int(out[name + "/calls"])), flush=True)
    np.savez_compressed(path, **out)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def compare(ref1, ref2, new, report=None):
    a1, a2, b = (np.load(p) for p in (ref1, ref2, new))
    lines, bad = [], 0
    for name, _ in SCENARIOS:
        keys = sorted(k for k in a1.files if k.startswith(name + "/"))
        other = sorted(k for k in b.files if k.startswith(name + "/"))
        if not keys:
            lines.append("%-32s MISSING from the reference run" % name)
            bad += 1
            continue
        stable = sorted(k for k in a2.files if k.startswith(name + "/")) == keys and all(same(a1[k], a2[k]) for k in keys)
        differ = [k for k in keys if k not in other or not same(a1[k], b[k])] + [k for k in other if k not in keys]
        calls, priors = int(a1[name + "/calls"]), sum(1 for k in keys if k.endswith("/prior_H"))
        what = "%d marginalisations, %d priors, %d arrays" % (calls, priors, len(keys))
        if not stable:
            # the solves between the marginalisations add with atomics: what is structure (ids, counts, orderings) must still be
            # equal wherever the reference's two runs have it equal; the numbers are set next to the reference's own spread
            def spread(x, y):
                worst = 0.0
                for k in keys:   # (not J and e0: the sign of an eigenvector is not determined)
                    if a1[k].dtype.kind == "f" and not k.endswith(("prior_J", "prior_e0")) and k in x.files and k in y.files and x[k].shape == y[k].shape and x[k].size:
                        worst = max(worst, float(np.nanmax(np.abs(x[k] - y[k])) / max(float(np.nanmax(np.abs(x[k]))), 1e-300)))
                return worst
            structure = [k for k in keys if a1[k].dtype.kind != "f" and k in a2.files and same(a1[k], a2[k]) and (k not in other or not same(a1[k], b[k]))]
            first = min((int(k.split("/")[1][4:]) for k in keys if k.split("/")[1].startswith("call") and a1[k].dtype.kind == "f"
                         and not (k in a2.files and same(a1[k], a2[k]))), default=-1)
            first_b = min((int(k.split("/")[1][4:]) for k in keys if k.split("/")[1].startswith("call") and a1[k].dtype.kind == "f"
                           and not (k in other and same(a1[k], b[k]))), default=-1)
            bad += 1 if structure else 0
            lines.append("%-32s the reference build does not agree with itself (first at marginalisation %d, largest relative difference of "
                         "an array %.1e); this build against it: first at marginalisation %d, %.1e; structure %s (%s)"
                         % (name, first, spread(a1, a2), first_b, spread(a1, b), "DIFFERS: " + ", ".join(structure[:4]) if structure else "equal", what))
        elif differ:
            bad += 1
            lines.append("%-32s DIFFERS in %s (%s)" % (name, ", ".join(k[len(name) + 1:] for k in differ[:6]), what))
        else:
            lines.append("%-32s bit-equal (%s)" % (name, what))
    text = "\n".join(lines)
    print(text)
    if report:
        with open(report, "w") as f:
            f.write(text + "\n")
    return bad


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) >= 5 and sys.argv[1] == "compare":
        sys.exit(1 if compare(*sys.argv[2:6]) else 0)
    else:
        sys.exit(__doc__)
