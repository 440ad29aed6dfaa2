"""The dogleg step at the head of the evaluation's blocks (k_post_solve without its tail + k_eval_build with a radius) against the
tail it replaces (SVIN_NO_STEP_IN_EVAL restores it): the sums, the coefficients and the candidate are the tail's arithmetic, so
every comparison here is for equal bits.  SVIN_STEP_IN_EVAL_LAUNCHES says which form ran.

test_stage_*: ONE handle, svin_ba_debug_trust_region_step in form 3 twice per radius -- through the tail, then
(SVIN_STEP_HOOK_IN_EVAL) through the pair: the whole scalar record (group B, doglegStepNorm, jdSq, jdDotR, stepNormSq, xNormSq,
the coefficients cg / cn in spareA0 / spareA1, the candidate's costs, gradMax, failMax, cholFail), y_C / v_C / y_L / v_L, the
candidate blocks and the candidate landmarks.  One radius each makes the step the Gauss-Newton step, the scaled-gradient step and
the interpolated one.

test_solve_*: optimize() moves the states and the IMU pre-integrations, so the two forms of a solve run on two handles fed from
one spec (the new form twice): poses, speed / bias, landmarks, every summary field and every IMU factor's count of re-integrations.

Windows: 3 keyframes with 17 landmarks (two landmark blocks in the post-solve pass, nPost = 4) and with 16 (one); a constant first
pose (the gauge: a block without rows, offset < 0 in the retraction) and a constant second one; a constant landmark; tracks of 17
and 33 observations (the second pass of the deferred landmark step); a window behind a marginalisation (three and more terms on an
entry: k_factors_only follows the launch); general 2x2 informations (k_eval_build<true>); a start perturbed until steps are
rejected (k_step_retract reads the record the recording block published) with re-integrations in candidate evaluations.
nPost 255 / 256 / 257 -- the second, strided trip of the head's partial sums, with the maximum in the ninth slot -- run under
SVIN_SLAB_CHUNKS=2: in the default partition a chunk block per chunk of landmarks plus the evaluation's own blocks are more
workgroups than 256 compute units (that window is held to the tail), with two chunks per block 127 / 128 chunk blocks fit beside
some 50 evaluation blocks.  The windows hold exactly 4048 / 4064 / 4080 landmarks on the device.  "nPost_largest" is close to the
largest window of the default partition that fits (the seeded generator decides how many of its landmarks are seen, hence "at
least 210" landmark blocks).  The window behind a marginalisation is compared stage by stage as well (the prior's block: kHeadAll).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import obs_patterns as op          # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402

pytestmark = pytest.mark.gpu

DEFERRED = 3
SUMMARY = ("initial_cost", "final_cost", "iterations", "successful", "termination")


def head_launches():
    from svin_amd.estimator import Estimator
    return Estimator.debug_get_option("SVIN_STEP_IN_EVAL_LAUNCHES")


def general_information(rng):
    a = rng.uniform(0.5, 2.0, 2)
    c = rng.uniform(-0.4, 0.4) * np.sqrt(a[0] * a[1])
    return np.array([[a[0], c], [c, a[1]]])


def prepare(est, fids, lids, fixed_frame, what):
    if fixed_frame is not None:
        ev = est.eval_reprojection()
        pose_of = {est.describe_block(int(b))[0]: int(b) for b in np.unique(ev["pose_id"])}
        assert est.set_parameter_block_constant(pose_of[fids[fixed_frame]])
    if "constant_landmark" in what:
        for l in (0, len(lids) // 2):
            assert est.set_parameter_block_constant(int(lids[l]))
    if "information" in what:
        rng = np.random.default_rng(5)
        for rid in est.eval_reprojection()["res_id"][::3]:
            w2 = est.map_get_reprojection_information(int(rid))[0, 0]
            assert est.map_set_reprojection_information(int(rid), general_information(rng) * w2)


def states_of(est, fids, lids):
    """poses, speed / bias and landmarks as flat float64 arrays (behind a marginalisation a frame may have lost its speed / bias block)"""
    def flat(xs):
        return np.concatenate([np.ravel(np.asarray(x, np.float64)) for x in xs if x is not None] + [np.zeros(0)])
    T = flat(est.get_T_WS(f) for f in fids)
    sb = flat(est.get_speed_and_bias(f) for f in fids)
    lms = est.get_landmarks()
    lm = flat(np.r_[lms[l]["point"], lms[l]["quality"]] for l in lids)
    assert len(T) > 0 and len(sb) > 0 and len(lm) > 0
    return T, sb, lm


def design_spec(**kw):
    d = op.design(**kw)
    return d.spec, d.fixed_frame


def tracks_spec():
    d = op.design_track_lengths()
    return d.spec, d.fixed_frame


def exact_window(L_dev, seed):
    """a seeded window of P = 3 whose device holds exactly L_dev landmarks: the first L_dev landmarks of a larger window that are
    seen at least twice, with their observations"""
    spec = syn.make_window(P=3, L=2 * L_dev, n_obs=5 * L_dev, seed=seed)
    cnt = np.bincount(spec.obs_lm, minlength=spec.L)
    pool = np.nonzero(cnt >= 2)[0][:L_dev]
    assert len(pool) == L_dev, "only %d landmarks are seen twice, %d wanted" % (len(pool), L_dev)
    new = np.full(spec.L, -1, np.int64)
    new[pool] = np.arange(L_dev)
    keep = new[spec.obs_lm] >= 0
    for name in ("obs_frame", "obs_cam", "obs_uv", "obs_size"):
        setattr(spec, name, getattr(spec, name)[keep])
    spec.obs_lm = new[spec.obs_lm[keep]]
    spec.lm_true, spec.lm_init = spec.lm_true[pool], spec.lm_init[pool]
    assert spec.L == L_dev
    return spec, None


TWO_CHUNKS = dict(SVIN_SLAB_CHUNKS=2)   # two chunks of landmarks per chunk block: read by pack()

# name -> (spec and constant frame, edits, landmark blocks of the post-solve pass: exactly n, at least -n, or None; options)
WINDOWS = {
    "L17": (lambda: design_spec(P=3, L=17, n_outliers=2), (), 2, {}),
    "L16": (lambda: design_spec(P=3, L=16, n_outliers=2), (), 1, {}),
    "first_pose_constant": (lambda: design_spec(P=4, L=33, fixed_frame=0, n_full=2), (), None, {}),
    "second_pose_constant": (lambda: design_spec(P=4, L=33, fixed_frame=1, n_full=2), (), None, {}),
    "constant_landmark": (lambda: design_spec(P=4, L=33, n_full=2), ("constant_landmark",), None, {}),
    "tracks_17_33": (tracks_spec, (), None, {}),
    "information": (lambda: design_spec(P=4, L=33, n_full=2), ("information",), None, {}),
    "nPost_largest": (lambda: (syn.make_window(P=3, L=3800, n_obs=7700, seed=11), None), (), -210, {}),
    # 253 / 254 / 255 landmark blocks + one factor block + the camera block: the second, strided trip of the head's partial sums
    "nPost255": (lambda: exact_window(4048, 21), (), 253, TWO_CHUNKS),
    "nPost256": (lambda: exact_window(4064, 22), (), 254, TWO_CHUNKS),
    "nPost257": (lambda: exact_window(4080, 23), (), 255, TWO_CHUNKS),
}


def compare_step(name, radius, old, new):
    assert old["form"] == new["form"] == DEFERRED
    for k in old["scalars"]:
        a, b = np.asarray(old["scalars"][k], np.float64), np.asarray(new["scalars"][k], np.float64)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "%s radius %.6g: %s %r through the tail, %r at the head" % (name, radius, k, a, b)
    for k in ("y_C", "v_C", "y_L", "v_L", "lm_cand"):
        assert np.array_equal(old[k].view(np.uint64), new[k].view(np.uint64)), "%s radius %.6g: %s differs" % (name, radius, k)
    assert len(old["block_cand"]) == len(new["block_cand"]) > 0
    for bid, a, b in zip(old["block_ids"], old["block_cand"], new["block_cand"]):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "%s radius %.6g: candidate of block %d differs by %.3e" % (
            name, radius, int(bid), float(np.max(np.abs(a - b))))


def compare_stages(name, est, debug_option, post_lm=None, n_post_exact=None, constant_pose=False, interpolates=True):
    """form 3 of the hook through the tail and through the pair on this handle, at a radius per branch of the dogleg step"""
    mu = 1e-4
    debug_option("SVIN_STEP_HOOK_IN_EVAL", 0)
    n0 = head_launches()
    first = est.debug_trust_region_step(mu, 1e4, DEFERRED)
    assert head_launches() == n0 and first["form_solve"] == DEFERRED
    n_post = first["post_lm_blocks"] + first["post_fac_blocks"] + 1
    if post_lm is not None:
        assert first["post_lm_blocks"] == post_lm if post_lm > 0 else first["post_lm_blocks"] >= -post_lm, first["post_lm_blocks"]
    if n_post_exact is not None:
        assert n_post == n_post_exact, n_post
    if constant_pose:   # (the extrinsics are constant in every window here; one pose more is in this one)
        assert first["d"] == 6 * (int((first["block_kind"] == 0).sum()) - 1) + 9 * int((first["block_kind"] == 2).sum()), "no constant pose in the window"
    s = first["scalars"]
    gn, ag = float(np.sqrt(s["gnHatSq"])), float(s["gHatSq"] * np.sqrt(s["gHatSq"]) / s["jgSq"])
    if interpolates:
        assert ag < gn, "the Cauchy point lies beyond the Gauss-Newton step: no radius interpolates"
    branches = set()
    for radius in (2.0 * gn, 0.5 * min(ag, gn)) + ((0.5 * (ag + gn),) if ag < gn else ()):
        debug_option("SVIN_STEP_HOOK_IN_EVAL", 0)
        n1 = head_launches()
        old = est.debug_trust_region_step(mu, radius, DEFERRED)
        assert head_launches() == n1, "the tail was asked for"
        debug_option("SVIN_STEP_HOOK_IN_EVAL", 1)
        new = est.debug_trust_region_step(mu, radius, DEFERRED)
        assert head_launches() == n1 + 1, "the step did not go through the head of the evaluation's blocks"
        debug_option("SVIN_NO_STEP_IN_EVAL", 1)   # the switch wins over the hook's option
        off = est.debug_trust_region_step(mu, radius, DEFERRED)
        assert head_launches() == n1 + 1
        debug_option("SVIN_NO_STEP_IN_EVAL", 0)
        compare_step(name, radius, old, new)
        compare_step(name, radius, old, off)
        cg, cn = new["scalars"]["spareA0"], new["scalars"]["spareA1"]
        branches.add("newton" if (cg == 0.0 and cn == 1.0) else ("gradient" if cn == 0.0 else "interpolated"))
        assert new["scalars"]["stepNormSq"] > 0.0 and new["scalars"]["cholFail"] == 0
    assert branches == ({"newton", "gradient", "interpolated"} if ag < gn else {"newton", "gradient"}), branches
    print("%s: d %d, L %d, nPost %d, %d radii through both forms" % (name, first["d"], first["L"], n_post, len(branches)))


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_stage_by_stage_the_head_equals_the_tail(gpu_lib, debug_option, name):
    from svin_amd.estimator import Estimator
    make, what, post_lm, options = WINDOWS[name]
    for k, v in options.items():
        debug_option(k, v)
    spec, fixed_frame = make()
    est = Estimator(0)
    fids, lids = syn.feed(est, spec)
    prepare(est, fids, lids, fixed_frame, what)
    compare_stages(name, est, debug_option, post_lm=post_lm, n_post_exact=int(name[5:]) if name[5:].isdigit() else None,
                   constant_pose=fixed_frame is not None)


def slide(est, spec):
    """optimise and marginalise as the frames arrive: the window ends behind a prior"""
    def on_frame(k, fid):
        est.optimize(6)
        est.apply_marginalization(2, 2)
    fids, lids = syn.feed(est, spec, on_frame=on_frame)
    assert est.marg() is not None
    return est.frame_ids(), [l for l in lids if l in est.get_landmarks()]


PRIOR_WINDOW = dict(P=7, L=200, n_obs=2000, seed=9, keyframe_every=2, frame_dt=0.3)


def test_stage_by_stage_behind_a_marginalisation_prior(gpu_lib, debug_option):
    """the prior's block keeps every candidate block in its LDS (kHeadAll) and evaluates the prior there"""
    from svin_amd.estimator import Estimator
    est = Estimator(0)
    slide(est, syn.make_window(**PRIOR_WINDOW))
    compare_stages("prior", est, debug_option, interpolates=False)   # (a strong prior may leave no radius that interpolates)


def test_a_window_of_more_than_256_post_solve_blocks_keeps_the_tail_in_the_default_partition(gpu_lib, debug_option):
    """a chunk block per chunk of landmarks: that many landmark blocks bring as many chunk blocks to k_eval_build beside the
    evaluation's own, more workgroups than compute units"""
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=3, L=4600, n_obs=9300, seed=12)
    est = Estimator(0)
    syn.feed(est, spec)
    debug_option("SVIN_STEP_HOOK_IN_EVAL", 1)
    n0 = head_launches()
    res = est.debug_trust_region_step(1e-4, 1e4, DEFERRED)
    assert res["post_lm_blocks"] + res["post_fac_blocks"] + 1 > 256
    assert head_launches() == n0


def solve(spec, fixed_frame, what, iters, no_step_in_eval, debug_option, sliding=False):
    from svin_amd.estimator import Estimator
    debug_option("SVIN_NO_STEP_IN_EVAL", 1 if no_step_in_eval else 0)
    n0 = head_launches()
    est = Estimator(0)
    fids, lids = slide(est, spec) if sliding else syn.feed(est, spec)
    prepare(est, fids, lids, fixed_frame, what)
    est.optimize(0)                      # the first evaluation pre-integrates every IMU factor once
    redo0 = est.debug_build_arrays()["imu_redo"]
    est.optimize(iters)
    s = est.summary()
    out = {k: s[k] for k in SUMMARY}
    out["imu_redo"] = [int(v) for v in est.debug_build_arrays()["imu_redo"] - redo0]
    return states_of(est, fids, lids), out, head_launches() - n0


def assert_same_end(name, a, b):
    assert a[1] == b[1], (name, a[1], b[1])
    for x, y, what in zip(a[0], b[0], ("poses", "speed / bias", "landmarks")):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), "%s: %s differ by %.3e" % (name, what, float(np.max(np.abs(x - y))))


@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_solve_with_the_step_in_the_evaluation_ends_where_the_tail_ends(gpu_lib, debug_option, name):
    make, what, _, options = WINDOWS[name]
    for k, v in options.items():
        debug_option(k, v)
    spec, fixed_frame = make()
    iters = 8
    tail = solve(spec, fixed_frame, what, iters, True, debug_option)
    head = solve(spec, fixed_frame, what, iters, False, debug_option)
    again = solve(spec, fixed_frame, what, iters, False, debug_option)
    print("%s optimize(%d): %s, passes without a tail %d" % (name, iters, head[1], head[2]))
    assert tail[2] == 0 and head[2] > 0 and again[2] == head[2]
    assert_same_end(name, head, again)
    assert_same_end(name, head, tail)
    if name == "second_pose_constant":   # (its candidates move the gyro biases far enough: candidate evaluations re-integrate)
        assert min(head[1]["imu_redo"]) > 0, head[1]["imu_redo"]


def test_solve_behind_a_marginalisation_prior(gpu_lib, debug_option):
    """a sliding window: the prior's block takes the head as well, and with three and more terms on an entry of S the factors keep
    a launch of their own behind k_eval_build (k_factors_only)"""
    spec = syn.make_window(**PRIOR_WINDOW)
    tail = solve(spec, None, (), 8, True, debug_option, sliding=True)
    head = solve(spec, None, (), 8, False, debug_option, sliding=True)
    print("sliding window optimize(8): %s, passes without a tail %d" % (head[1], head[2]))
    assert tail[2] == 0 and head[2] > 0
    assert_same_end("prior", head, tail)


def test_solve_with_rejected_steps(gpu_lib, debug_option):
    """a start far enough off for the trust region to reject steps: the iteration behind a rejected step re-uses the linearisation
    through k_step_retract, which reads group B from the record the recording block published; and candidate evaluations of this
    solve re-integrate IMU factors"""
    cfg = dict(seed=72, pose_noise=(1.0, 0.25), lm_noise=2.5)
    spec = syn.make_window(P=6, L=250, n_obs=2500, **cfg)
    tail = solve(spec, None, (), 25, True, debug_option)
    head = solve(spec, None, (), 25, False, debug_option)
    again = solve(spec, None, (), 25, False, debug_option)
    print("perturbed optimize(25): %s, passes without a tail %d" % (head[1], head[2]))
    assert tail[2] == 0 and head[2] > 0
    assert head[1]["successful"] < head[1]["iterations"], "no step was rejected: raise the perturbation"
    assert max(head[1]["imu_redo"]) > 0, "no evaluation of the solve re-integrated"
    assert_same_end("rejected", head, again)
    assert_same_end("rejected", head, tail)
