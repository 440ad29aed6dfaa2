"""Constant landmarks in a sliding window: a caller anchors the window to a map it trusts by holding landmarks constant
(Map::setParameterBlockConstant on a HomogeneousPointParameterBlock).  Such a window stays device-resident and marginalises:

  A  one marginalisation at rounding level against the oracle and the 40-digit restatement (tests/mp_marg.py)
  B  the device-resident window against the host re-pack, every frame, through every way a flag can reach or leave the device
  C  a sequence of optimise + marginalise against the oracle
  D  windows with constant landmarks in a batch
  E  a landmark under a HomogeneousPointError seen from a leaving frame is still refused

Reference: MarginalizationError::addResidualBlock gives a fixed block zero columns (MarginalizationError.cpp:156) and skips it in the
accumulation (:343, :367); the policy loop of Estimator::applyMarginalizationStrategy (Estimator.cpp:671-766) never asks whether a
landmark is fixed."""
import functools

import numpy as np
import pytest

from svin_amd import synthetic as syn
from helpers import constant_landmarks as cl

pytestmark = pytest.mark.gpu


def log(*a):
    print(*a, flush=True)


# ------------------------------------------------------------------------------------------------------------------ A
@functools.lru_cache(maxsize=None)
def one_shot_reference(rig):
    """the oracle's states ahead of every marginalisation, and a second oracle that received them through its setters -- once per
    fixture, shared by the pack modes; with the exact (40-digit) result of frame 7's marginalisation"""
    from oracle import orc
    import mp_marg
    spec = cl.one_shot_window(rig)
    rec_0, _, _ = cl.constant_pass(orc.OracleEstimator(), spec)
    snaps = [r[0] for r in rec_0]
    rec_c, fc, const = cl.constant_pass(orc.OracleEstimator(), spec, snaps=snaps)
    exact = {}
    for k in (4, 7) if rig == "rig_v2" else (7,):
        pm = rec_c[k][5]
        # (the oracle lists a constant landmark as a range of width 0: it has no column to eliminate)
        exact[k] = mp_marg.marginalize_mp(pm["H"], pm["b0"], [p for p in pm["lm"] if p[1] > 0], pm["dense"])
    return spec, snaps, rec_c, fc, const, exact


@pytest.mark.parametrize("pack_mode", [0, 1])
@pytest.mark.parametrize("rig", ["rig_v2", "euroc"])
def test_marginalization_one_shot_with_constant_landmarks(gpu_lib, rig, pack_mode):
    """test_marginalization_one_shot's procedure with every third landmark constant from the first frame on: the same states on
    both sides ahead of EVERY marginalisation, one applyMarginalizationStrategy each, (2, 3) every frame.  rig_v2 (sonar, depth,
    per-frame extrinsics): frame 4 removes 89 landmarks and linearises none, frame 7 linearises 76 of which 25 are constant;
    euroc with the tracks of the even landmarks cut behind frame 4: frame 7 linearises 22 of which 7 are constant.  Bars as in
    test_marginalization_one_shot; the oracle alone sits at 9.6e-12 / 3.6e-10 (H) of the exact result at frame 7.  One step is added to
    that procedure (helpers/constant_landmarks.constant_pass): both sides are evaluated once at far gyro biases ahead of the injection, so
    that the injected states alone determine where every IMU factor pre-integrates.  Without that step the euroc fixture misses the bars
    for a reason that has nothing to do with the product: the oracle itself, given the same injected states after optimize(11) instead
    of optimize(12), ends dH = 1.53e-5, db0 = 2.3e-6 away from its twin at frame 3 (tests/test_constant_landmarks_oracle.py asserts
    that, and that the step brings it to exactly 0); the product under the unmodified procedure measured the very same
    dH = 1.5277e-5 at that frame on an MI355X (one IMU factor re-integrated one iteration apart), rig_v2 8.5e-11."""
    from svin_amd.estimator import Estimator
    from test_gpu_parity import compare_priors
    spec, snaps, rec_c, fc, const_c, exact = one_shot_reference(rig)
    gpu = Estimator(0)
    gpu.set_pack_mode(pack_mode)
    rec_g, fg, const_g = cl.constant_pass(gpu, spec, snaps=snaps)
    assert fg == fc and const_g == const_c and len(const_g) == 84
    assert len(rec_g) == len(rec_c) == spec.P
    # the fixture does what it is there for: frame 7 linearises constant landmarks
    lm7 = rec_c[7][5]["lm"]
    n_lin, n_const = len(lm7), sum(1 for p in lm7 if p[1] == 0)
    log(rig, "frame 7: linearised landmarks", n_lin, "of them constant", n_const)
    assert n_lin >= 20 and n_const >= 5
    assert len([i for i in rec_c[7][1] if i in set(const_c)]) >= 5
    for k, (g, c) in enumerate(zip(rec_g, rec_c)):
        assert g[1] == c[1] and g[3] == c[3] and g[4] == c[4], "frame %d: removed landmarks / frames / landmark count" % k
        assert (g[2] is None) == (c[2] is None)
        if c[2] is None:
            continue
        o = compare_priors(g[2], c[2], "one-shot marginalisation with constant landmarks %s frame %d (GPU vs oracle)" % (rig, k))
        bs = max(1.0, o["b0_scale"])
        assert o["dH"] < 1e-8 and o["dJtJ"] < 1e-8 and o["selfH"] < 1e-9, (k, o)
        assert o["db0"] < 1e-8 * bs and o["dJte0"] < 1e-8 * bs, (k, o)
        if k not in exact:
            continue
        ex = exact[k]
        sd = np.sqrt(np.abs(np.diag(ex["H"])))
        err = {}
        for name, m in (("gpu", g[2]), ("oracle", c[2])):
            keyc = {(b["frame"], b["kind"], b["index"]): b for b in c[2]["blocks"]}
            perm = np.zeros(m["n"], int)
            for b in m["blocks"]:
                if b["frame"] is not None:
                    for j in range(b["mdim"]):
                        perm[keyc[(b["frame"], b["kind"], b["index"])]["ordering"] + j] = b["ordering"] + j
            H, b0, J = m["H"][np.ix_(perm, perm)], m["b0"][perm], m["J"][:, perm]
            err[name] = dict(H=float(np.max(np.abs(H - ex["H"]) / np.outer(sd, sd))), b0=float(np.max(np.abs(b0 - ex["b0"]) / sd)),
                             JtJ=float(np.max(np.abs(J.T @ J - ex["JtJ"]) / np.outer(sd, sd))),
                             Jte0=float(np.max(np.abs(J.T @ m["e0"] - ex["Jte0"]) / sd)))
        log("%s frame %d distance to the exact (40-digit) result:" % (rig, k), err)
        for name in ("gpu", "oracle"):
            assert err[name]["H"] < 1e-8 and err[name]["JtJ"] < 1e-8, (k, name, err)
            assert err[name]["b0"] < 1e-8 * bs and err[name]["Jte0"] < 1e-8 * bs, (k, name, err)
    if pack_mode == 0 and rig == "euroc":   # (rig_v2's sonar factors read the landmarks in addStates: its jobs are host-assembled)
        pc = gpu.path_counters()
        log(rig, pc)
        assert pc["host_pack_solves"] == 0


# ------------------------------------------------------------------------------------------------------------------ B
class ResidentChecks(cl.NoChecks):
    """what test B asserts at the marked points of helpers/constant_landmarks.run_resident_script; a = resident, b = host-packed"""

    def __init__(self, a, b):
        self.a, self.b = a, b
        self.n_tables = self.n_const_obs = self.n_const_removed = 0
        self.handles = {}     # frame -> (handle range, landmarks) of the resident estimator after the frame's first flush

    def const_ids(self, cd):
        return {cd.drv.lm_ids[l] for l in cd.const}

    def tables(self, k, tag, cd):
        from test_gpu_resident import assert_same_csr
        ca, cb = self.a.debug_csr(), self.b.debug_csr()
        assert ca["resident"], tag
        assert_same_csr(ca, cb, tag)
        mask = cl.constant_observation_mask(self.b, cb, self.const_ids(cd))
        assert np.array_equal(ca["w"] < 0, mask), "%s: the negative weights are not the observations of the constant landmarks" % tag
        assert np.all(ca["w"] != 0)
        self.n_tables += 1
        self.handles.setdefault(k, self.a.landmark_handles())
        self.n_const_obs += int(mask.sum())

    def solve(self, k, tag, cd, iters):
        from test_gpu_resident import same_states
        ids = sorted(self.const_ids(cd))
        before = [[e.get_landmark(i)["point"] for i in ids] for e in (self.a, self.b)]
        for e in (self.a, self.b):
            e.optimize(iters)
        same_states([self.a, self.b], tag + " after optimize")
        for e, pts in zip((self.a, self.b), before):
            for i, p in zip(ids, pts):
                assert np.array_equal(e.get_landmark(i)["point"], p), "%s: constant landmark %d moved" % (tag, i)
        la, lb = self.a.get_landmarks(), self.b.get_landmarks()
        assert la.keys() == lb.keys()
        for i in la:
            assert np.array_equal(la[i]["point"], lb[i]["point"]) and la[i]["quality"] == lb[i]["quality"], (tag, i)

    def detour(self, cd, edit):
        self.a.set_pack_mode(1)
        assert not self.a.debug_csr()["resident"]     # the device copy is dropped (a pack without a solve: no counter moves)
        edit()                                        # flags change while the host graph is the authority
        self.a.set_pack_mode(0)

    def marginalised(self, k, results, cd):
        assert list(results[0][1]) == list(results[1][1]), "frame %d: removed landmarks differ" % k
        self.n_const_removed += len(self.const_ids(cd) & {int(i) for i in results[0][1]})


def test_resident_window_with_constant_landmarks_equals_host_rebuild(gpu_lib):
    """two product estimators, one device-resident and one host-packed, through the frames of run_resident_script.  Every frame:
    the first is resident, the CSRs are equal array for array with w < 0 exactly on the observations of constant landmarks, the
    states after optimize(4) are bit-equal, no constant landmark moved, the removed landmarks are equal.  At the end: equal priors,
    no host-packed solve, device-gathered jobs that linearised constant landmarks (counted on the oracle driven by the same script:
    the policy depends on the graph alone)."""
    from svin_amd.estimator import Estimator
    from oracle import orc
    spec = cl.cut_tracks(syn.make_window(**cl.RESIDENT_WINDOW), cl.RESIDENT_CUT_AFTER)

    class Count(cl.NoChecks):
        def __init__(self):
            self.lin = []

        def marginalised(self, k, results, cd):
            pre = cd.drv.ests[0].marg_pre()
            self.lin.append(sum(1 for p in pre["lm"] if p[1] == 0) if pre else 0)
    count = Count()
    _, removed_o = cl.run_resident_script([orc.OracleEstimator()], spec, count, iters=1, batched=False)
    log("constant landmarks linearised per frame (oracle):", count.lin)
    assert sum(count.lin) >= 5

    a, b = Estimator(0), Estimator(0)
    b.set_pack_mode(1)
    checks = ResidentChecks(a, b)
    cd, removed = cl.run_resident_script([a, b], spec, checks, iters=4)
    assert removed == removed_o     # the same landmarks leave as in the reference's policy
    log("tables compared", checks.n_tables, "observations of constant landmarks in them", checks.n_const_obs,
        "constant landmarks erased by the marginalisation", checks.n_const_removed, "constant at the end", len(cd.const))
    assert checks.n_tables == spec.P + 5 and checks.n_const_obs > 1000 and checks.n_const_removed >= 5 and len(cd.const) >= 5
    # case (6) did happen: the short-lived landmarks of frame 6 used up the handle range, frame 7's flush renumbered the survivors
    log("handle range / landmarks per frame", checks.handles)
    assert checks.handles[5][0] < 4096 and checks.handles[6][0] > 8192 + checks.handles[5][0]
    assert checks.handles[7][0] == checks.handles[7][1] < 1000
    ma, mb = a.marg(), b.marg()
    assert ma is not None and mb is not None
    assert [x["id"] for x in ma["blocks"]] == [x["id"] for x in mb["blocks"]]
    for key in ("H", "b0"):
        assert np.array_equal(ma[key], mb[key]), "prior %s differs by %g" % (key, float(np.max(np.abs(ma[key] - mb[key]))))
    pa, pb = a.path_counters(), b.path_counters()
    log("resident", pa, "host", pb)
    assert pa["host_pack_solves"] == 0 and pa["resident_solves"] == spec.P + 5 and pb["resident_solves"] == 0
    # every job's tables were gathered from the resident CSR, those that linearised constant landmarks (count.lin) among them
    # (the first frames' calls return before there is anything to marginalise: num_imu_frames states or fewer)
    assert pa["device_gathered_marginalisations"] == spec.P - cl.RESIDENT_MARG[1] and pa["host_assembled_marginalisations"] == 0
    assert pb["device_gathered_marginalisations"] == 0


# ------------------------------------------------------------------------------------------------------------------ C
def test_marginalization_sequence_with_constant_landmarks(gpu_lib):
    """test_marginalization_sequence_parity's euroc case with every third landmark constant: the landmarks removed per frame are the
    oracle's ([0, 0, 0, 0, 1, 0, 0, 15]), the final window's poses within 1e-4, and no constant landmark ever moves on either side"""
    from svin_amd.estimator import Estimator
    from oracle import orc
    from test_gpu_parity import pose_diff
    spec = syn.make_window(P=8, L=250, n_obs=2500, seed=44, rig="euroc", keyframe_every=2, frame_dt=0.3)
    out = []
    for est in (Estimator(0), orc.OracleEstimator()):
        est.set_solver_options(1e-12, 1e-12, 1e-12)
        held, removed = {}, []

        def on_frame(k, fid, est=est, held=held, removed=removed):
            if k == 0:
                for lid in est.landmark_ids()[::3]:
                    cl.hold_constant(est, lid)
                    held[lid] = est.get_landmark(lid)["point"].copy()
            est.optimize(25)
            for lid in set(held) & set(est.landmark_ids()):
                assert np.array_equal(est.get_landmark(lid)["point"], held[lid]), "frame %d: constant landmark %d moved" % (k, lid)
            ok, rem = est.apply_marginalization(2, 3)
            assert ok
            removed.append(len(rem))
        syn.feed(est, spec, on_frame=on_frame)
        out.append((est, removed, held))
    (gpu, rg, hg), (cpu, rc, hc) = out
    log("removed landmarks per frame gpu", rg, "cpu", rc)
    assert rg == rc == [0, 0, 0, 0, 1, 0, 0, 15]
    assert len(hg) == 84 and hg.keys() == hc.keys() and all(np.array_equal(hg[i], hc[i]) for i in hg)
    assert gpu.num_frames() == cpu.num_frames() and gpu.num_landmarks() == cpu.num_landmarks()
    assert gpu.frame_ids() == cpu.frame_ids() and gpu.landmark_ids() == cpu.landmark_ids()
    worst = max(pose_diff(gpu.get_T_WS(f), cpu.get_T_WS(f)) for f in gpu.frame_ids())
    log("final window pose difference", worst)
    assert worst < 1e-4
    assert gpu.path_counters()["host_pack_solves"] == 0


# ------------------------------------------------------------------------------------------------------------------ D
def test_batch_with_constant_landmarks(gpu_lib):
    """four euroc windows of one state geometry, two of them with constant landmarks, in one batch: all four batched, each ends bit
    for bit where it ends alone (the flag is the sign of the slot's own weights: batchSupported does not look at landmarks)"""
    from svin_amd import estimator
    from test_gpu_batch import states_of

    def build(seed, every):
        est = estimator.Estimator(0)
        fids, lids = syn.feed(est, syn.make_window(seed=seed, P=6, L=250, n_obs=2500))
        held = lids[::every] if every else []
        for lid in held:
            cl.hold_constant(est, lid)
        return est, fids, lids, {l: est.get_landmark(l)["point"].copy() for l in held}
    cfgs = [(11, 0), (12, 3), (13, 0), (14, 2)]
    alone = []
    for c in cfgs:
        est, fids, lids, held = build(*c)
        est.optimize(8)
        alone.append((states_of(est, fids, lids), est.summary()))
    batch = [build(*c) for c in cfgs]
    assert estimator.optimize_batch([b[0] for b in batch], 8) == 4
    for k, (est, fids, lids, held) in enumerate(batch):
        s, (ref, s_ref) = est.summary(), alone[k]
        assert (s["iterations"], s["successful"], s["final_cost"]) == (s_ref["iterations"], s_ref["successful"], s_ref["final_cost"]), k
        for x, y in zip(states_of(est, fids, lids), ref):
            assert np.array_equal(x, y, equal_nan=True), k
        assert len(held) == (0, 84, 0, 125)[k]
        for l, p in held.items():
            assert np.array_equal(est.get_landmark(l)["point"], p), (k, l)
        assert est.path_counters()["host_pack_solves"] == 0


# ------------------------------------------------------------------------------------------------------------------ E
def test_landmark_prior_seen_from_a_leaving_frame_is_still_refused(gpu_lib):
    """a landmark under a HomogeneousPointError observed from a frame that leaves: applyMarginalizationStrategy fails and changes
    nothing (in release builds the reference silently drops that residual when the landmark is marginalised -- not copied).  The
    constant landmarks next to it are no reason to refuse: without the prior the same call goes through."""
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=6, L=120, n_obs=1200, seed=3, rig="euroc", keyframe_every=2, frame_dt=0.3)
    est = Estimator(0)
    fids, lids = syn.feed(est, spec)
    for lid in lids[::3]:
        cl.hold_constant(est, lid)
    est.optimize(3)
    # (2, 2) on six frames with every second one a keyframe: frames 1 and 3 leave
    seen = [lids[int(l)] for l in np.unique(spec.obs_lm[spec.obs_frame == 1]) if l % 3 != 0]
    assert est.get_landmark(seen[0])["n_obs"] > 0 and not est.is_parameter_block_constant(seen[0])
    rid = est.add_homogeneous_point_error(seen[0], np.array([1.0, 2.0, 3.0, 1.0]), np.eye(3))
    assert rid
    before = (est.frame_ids(), est.landmark_ids(), [est.get_landmark(l)["n_obs"] for l in lids], est.marg())
    with pytest.raises(RuntimeError, match="HomogeneousPointError"):
        est.apply_marginalization(2, 2)
    after = (est.frame_ids(), est.landmark_ids(), [est.get_landmark(l)["n_obs"] for l in lids], est.marg())
    assert before[:3] == after[:3] and before[3] is None and after[3] is None
    assert est.remove_homogeneous_point_error(rid)
    ok, removed = est.apply_marginalization(2, 2)
    assert ok and len(est.frame_ids()) < len(fids)
