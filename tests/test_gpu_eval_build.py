"""Evaluation and the build of the normal equations behind it in ONE launch (k_eval_build) against the two launches it replaces
(k_eval_all, k_schur_dense<9, false, 4>; SVIN_NO_EVAL_BUILD restores them): identical arithmetic is the contract, so every
comparison here is for equal bits wherever the build is ordered.

test_build_*: one handle, svin_ba_linearize twice at the same point -- through the two launches, then (SVIN_LINEARIZE_EVAL_BUILD)
through k_eval_build; SVIN_EVAL_BUILD_LAUNCHES says which ran.  Every entry of S (both triangles), g and the cost must be equal
bit for bit where at most two small factors add to it (the factors' atomic additions start from zero and two additions commute; the
landmark part arrives afterwards through k_reduce_slabs in a fixed order); an entry that three or more factors reach is unordered
in both forms and is held to the a-priori rounding bound of tests/helpers/schur_reference.py instead, for both forms.  gFull and hC
likewise, Vinv / bl / hL / scaleL everywhere (svin_ba_debug_build_arrays reads them back), and svin_ba_debug_reduced_solve in its
fused form gives the same step through both paths.

test_solve_*: optimize() moves the states, so the two forms run on two handles fed from one spec, the fused form twice: poses,
speed / bias, landmarks, the summary (costs, iterations, successful steps, termination) and every IMU factor's count of
re-integrations during the solve bit for bit; the "L33_fixed" window asserts that candidate evaluations of its fused solve re-integrate
(nothing but the steps moves its biases), the "bias" window moves the gyro biases past 1e-4 / Delta_t behind the first pre-integration and
asserts that the solve's evaluations re-integrate every factor.

Windows (tests/helpers/obs_patterns.py): device landmark counts 1 / 15 / 16 / 17 / 33 on P = 3-4 poses (33 with a constant pose: a
last chunk of one landmark, tracks of one observation and stereo pairs, lanes whose first observation is of the constant pose);
tracks of 15 / 16 / 17 / 31 / 32 / 33 / 34 observations need P = 17 poses of two cameras (one, two and three rounds per lane);
a constant landmark; a Huber loss; general 2x2 information; gyro biases moved past 1e-4 / Delta_t; variable extrinsics (the fallback).  Rejected steps (a discarded fused build) have a test of their own on the
badly perturbed windows of tests/test_gpu_batch.py.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import obs_patterns as op          # noqa: E402
import schur_reference as sr       # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402

pytestmark = pytest.mark.gpu

KIND = {0: "p", 1: "e", 2: "s"}
DIM = {0: 6, 1: 6, 2: 9}
HUBER = 2


def launches():
    from svin_amd.estimator import Estimator
    return Estimator.debug_get_option("SVIN_EVAL_BUILD_LAUNCHES")


def general_information(rng):
    a = rng.uniform(0.5, 2.0, 2)
    c = rng.uniform(-0.4, 0.4) * np.sqrt(a[0] * a[1])
    return np.array([[a[0], c], [c, a[1]]])


def prepare(est, fids, lids, design, what):
    """the case's edits on a fed estimator"""
    if design.fixed_frame is not None:
        ev = est.eval_reprojection()
        pose_of = {est.describe_block(int(b))[0]: int(b) for b in np.unique(ev["pose_id"])}
        assert est.set_parameter_block_constant(pose_of[fids[design.fixed_frame]])
    if "constant_landmark" in what:
        for l in (0, len(lids) // 2):
            assert est.set_parameter_block_constant(int(lids[l]))
    if "huber" in what:
        for rid in est.eval_reprojection()["res_id"][::2]:
            assert est.map_set_residual_loss(int(rid), HUBER, 1.5)
    if "information" in what:
        rng = np.random.default_rng(5)
        for rid in est.eval_reprojection()["res_id"][::3]:
            w2 = est.map_get_reprojection_information(int(rid))[0, 0]
            assert est.map_set_reprojection_information(int(rid), general_information(rng) * w2)
    if "bias" in what:
        move_gyro_bias(est, fids)


def move_gyro_bias(est, fids):
    """|delta b_g| Delta_t > 1e-4 with Delta_t <= 0.1 s: the next evaluation re-integrates every IMU factor"""
    for f in fids:
        sb = est.get_speed_and_bias(f)
        sb[3:6] += 0.02
        assert est.set_speed_and_bias(f, sb)


BUILD_CASES = {
    "L1": (lambda: op.design(P=3, L=1, n_outliers=1), ()),
    "L15": (lambda: op.design(P=3, L=15, n_outliers=2), ()),
    "L16": (lambda: op.design(P=3, L=16, n_outliers=2), ()),
    "L17": (lambda: op.design(P=4, L=17, n_outliers=2), ()),
    "L33_fixed": (lambda: op.design(P=4, L=33, fixed_frame=1, n_full=2), ()),
    "tracks": (lambda: op.design_track_lengths(), ()),
    "constant_landmark": (lambda: op.design(P=4, L=33, n_full=2), ("constant_landmark",)),
    "huber": (lambda: op.design(P=4, L=33, n_full=2), ("huber",)),
    "information": (lambda: op.design(P=4, L=33, n_full=2), ("information",)),
    "bias": (lambda: op.design(P=4, L=33, n_full=2), ("bias",)),
}


def factor_counts_and_reference(est, lin, mu):
    """per entry of the reduced system: how many small factors add to it; and (where np.longdouble is wider than float64) the
    long-double reference of linearize()'s system from the records the build consumes, with its rounding bound"""
    desc = {}

    def describe(b):
        if b not in desc:
            desc[b] = est.describe_block(b)
        return desc[b]
    ev = est.eval_reprojection(robust=True)
    recs = [(ev["r"][i], [(("p", int(ev["pose_id"][i])), ev["Jp"][i]), (("l", int(ev["lm_id"][i])), ev["Jl"][i])]) for i in range(len(ev["r"]))]
    touched = np.zeros((lin["d"], lin["d"]), np.int64)
    off_of = {int(b): (int(o), DIM[describe(int(b))[1]]) for b, o in zip(lin["block_ids"], lin["block_off"])}
    for f in est.eval_factors():
        bl, o, rows = [], 0, []
        for b in f["blocks"]:
            kind = describe(b)[1]
            bl.append(((KIND[kind], b), f["J"][:, o:o + DIM[kind]]))
            o += DIM[kind]
            if int(b) in off_of:
                rows += list(range(off_of[int(b)][0], off_of[int(b)][0] + off_of[int(b)][1]))
        recs.append((f["r"], bl))
        touched[np.ix_(rows, rows)] += 1
    blocks = [((KIND[describe(int(b))[1]], int(b)), int(o), DIM[describe(int(b))[1]]) for b, o in zip(lin["block_ids"], lin["block_off"])]
    return touched, (sr.assemble(recs, blocks, mu) if sr.have_long_double() else None)


@pytest.mark.parametrize("name", sorted(BUILD_CASES))
def test_build_in_the_evaluation_launch_equals_the_two_launches(gpu_lib, debug_option, name):
    from svin_amd.estimator import Estimator
    make, what = BUILD_CASES[name]
    design = make()
    est = Estimator(0)
    fids, lids = syn.feed(est, design.spec)
    prepare(est, fids, lids, design, what)
    mu = 1e-4
    est.linearize(mu)                       # (the first evaluation pre-integrates every IMU factor)
    n0 = launches()
    two = est.linearize(mu)
    two_arr = est.debug_build_arrays()
    y_two = est.debug_reduced_solve(mu, fused=True)
    assert launches() == n0 and Estimator.debug_get_option("SVIN_LAST_SCHUR_FORM") == op.D9
    debug_option("SVIN_LINEARIZE_EVAL_BUILD", 1)
    one = est.linearize(mu)
    one_arr = est.debug_build_arrays()
    n_lin = launches()
    y_one = est.debug_reduced_solve(mu, fused=True)        # (the hook's own evaluation + build + solve, through k_eval_build as well)
    assert launches() > n_lin
    solve_arr = est.debug_build_arrays()
    assert launches() > n0 and Estimator.debug_get_option("SVIN_LAST_SCHUR_FORM") == op.D9
    debug_option("SVIN_NO_EVAL_BUILD", 1)   # the switch wins over the hook
    n1 = launches()
    off = est.linearize(mu)
    assert launches() == n1
    debug_option("SVIN_NO_EVAL_BUILD", 0)
    debug_option("SVIN_LINEARIZE_EVAL_BUILD", 0)
    assert one["d"] == two["d"] and one["cost"] == two["cost"]
    touched, rf = factor_counts_and_reference(est, two, mu)
    ordered = touched <= 2
    if rf is not None:
        for lin, tag in ((two, "two launches"), (one, "one launch"), (off, "switch")):
            rS, rg = sr.worst_ratio(lin["S"], lin["g"], rf)
            print("%s %s: worst error / tol  S %.3g  g %.3g" % (name, tag, rS, rg))
            assert rS <= 1.0 and rg <= 1.0, "the reduced system leaves its rounding bound"
    dS = one["S"] != two["S"]
    print("%s: d %d, entries of S that differ %d (unordered entries %d), of g %d" %
          (name, two["d"], int(np.count_nonzero(dS)), int(np.count_nonzero(~ordered)), int(np.count_nonzero(one["g"] != two["g"]))))
    assert not np.any(dS & ordered), "S differs from the two launches where the build is ordered"
    g_ordered = np.diag(ordered)
    assert np.array_equal(one["g"][g_ordered], two["g"][g_ordered]), "g differs from the two launches where the build is ordered"
    # what the chunk blocks write per landmark is ordered everywhere; the full gradient and the column norms where the factors' sums are
    for key in ("Vinv", "b_l", "h_l", "scale_l"):
        assert two_arr[key].shape[0] == design.spec.L
        assert np.array_equal(one_arr[key], two_arr[key]) and np.array_equal(solve_arr[key], two_arr[key]), key
    for key in ("g_full", "h_c"):
        assert np.array_equal(one_arr[key][g_ordered], two_arr[key][g_ordered]), key
    assert np.array_equal(one_arr["imu_redo"], two_arr["imu_redo"])   # (no launch compared here re-integrates: see the solves)
    # svin_ba_debug_reduced_solve in the form optimize() runs, its build in the evaluation's launch: the same step
    if np.all(ordered):
        assert np.array_equal(y_one, y_two), "the Gauss-Newton step differs by %.3e" % float(np.max(np.abs(y_one - y_two)))
    else:
        assert np.allclose(y_one, y_two, rtol=1e-9, atol=1e-12)


def states_of(est, fids, lids):
    T = np.stack([est.get_T_WS(f) for f in fids])
    sb = np.stack([est.get_speed_and_bias(f) for f in fids])
    lms = est.get_landmarks()
    lm = np.stack([np.r_[lms[l]["point"], lms[l]["quality"]] for l in lids])
    return T, sb, lm


SOLVE_CASES = {
    "L17": (lambda: op.design(P=4, L=17, n_outliers=2), (), True),
    "L33_fixed": (lambda: op.design(P=4, L=33, fixed_frame=1, n_full=2), ("redo",), True),   # (its candidates move the gyro biases far enough)
    "tracks": (lambda: op.design_track_lengths(), (), True),
    "mixed": (lambda: op.design(P=4, L=33, n_full=2), ("constant_landmark", "huber", "information"), True),
    "bias": (lambda: op.design(P=4, L=33, n_full=2), ("bias late", "redo"), True),
    "extrinsics": (lambda: op.design(P=6, L=113, rig="test4", fixed_frame=2), (), False),
}


@pytest.mark.parametrize("name", sorted(SOLVE_CASES))
def test_solve_with_the_build_in_the_evaluation_launch_ends_where_the_two_launches_end(gpu_lib, debug_option, name):
    from svin_amd.estimator import Estimator
    make, what, taken = SOLVE_CASES[name]
    design = make()

    def run(iters, no_eval_build):
        debug_option("SVIN_NO_EVAL_BUILD", 1 if no_eval_build else 0)
        n0 = launches()
        est = Estimator(0)
        fids, lids = syn.feed(est, design.spec)
        prepare(est, fids, lids, design, what)
        est.optimize(0)                      # the first evaluation pre-integrates every IMU factor once
        redo0 = est.debug_build_arrays()["imu_redo"]
        if "bias late" in what:              # moved AFTER that pre-integration: the solve's own evaluations re-integrate
            move_gyro_bias(est, fids)
        est.optimize(iters)
        s = est.summary()
        out = {k: s[k] for k in ("initial_cost", "final_cost", "iterations", "successful", "termination")}
        out["imu_redo"] = [int(v) for v in est.debug_build_arrays()["imu_redo"] - redo0]   # re-integrations of this solve per IMU factor
        return states_of(est, fids, lids), out, launches() - n0

    for iters in (3, 10):
        two, again_two, one, again = run(iters, True), run(iters, True), run(iters, False), run(iters, False)
        assert two[2] == 0 and again_two[2] == 0
        # the launch ran once per enqueued build (initial evaluation + every candidate evaluation with clean accumulators), or never
        assert (one[2] > 0) == taken, (name, one[2])
        if not taken:
            assert Estimator.debug_get_option("SVIN_LAST_SCHUR_FORM") != op.D9
        print("%s optimize(%d): %s, fused launches %d" % (name, iters, one[1], one[2]))
        if "redo" in what:   # evaluations of the fused solve re-integrated (their factor blocks: the long chain, then their sums)
            assert min(one[1]["imu_redo"]) > 0, one[1]["imu_redo"]
            if "bias late" not in what:   # (nothing was moved by hand: every one of them was a candidate evaluation)
                assert one[1]["imu_redo"] == two[1]["imu_redo"]
        if not taken:   # (the form this window takes instead sums with unordered atomics: nothing of this change runs, nothing to compare)
            continue
        assert one[1] == again[1] and all(np.array_equal(a, b) for a, b in zip(one[0], again[0])), "the same call twice differs"
        if two[1] == again_two[1] and all(np.array_equal(a, b) for a, b in zip(two[0], again_two[0])):   # the parent path repeats itself
            assert one[1] == two[1], (one[1], two[1])
            for a, b, what_ in zip(one[0], two[0], ("poses", "speed / bias", "landmarks")):
                assert np.array_equal(a, b), "%s differ by %.3e" % (what_, float(np.max(np.abs(a - b))))
        else:
            print("%s optimize(%d): the two launches do not repeat themselves (unordered factor sums)" % (name, iters))


def test_solve_with_rejected_steps_discards_the_build_of_the_evaluation_launch(gpu_lib, debug_option):
    """starts far enough off for the trust region to reject steps (the windows of tests/test_gpu_batch.py's rejected-step test):
    a rejected step discards the build its candidate evaluation took along, and the next one starts from re-zeroed accumulators"""
    from svin_amd.estimator import Estimator
    cfgs = [dict(seed=71, pose_noise=(0.6, 0.15), lm_noise=1.5), dict(seed=72, pose_noise=(1.0, 0.25), lm_noise=2.5),
            dict(seed=73, pose_noise=(1.5, 0.4), lm_noise=4.0)]
    rejected = 0
    for c in cfgs:
        spec = syn.make_window(P=6, L=250, n_obs=2500, **c)
        ends = []
        for no_eval_build in (1, 0, 0):
            debug_option("SVIN_NO_EVAL_BUILD", no_eval_build)
            n0 = launches()
            est = Estimator(0)
            fids, lids = syn.feed(est, spec)
            est.optimize(25)
            s = est.summary()
            ends.append((states_of(est, fids, lids), {k: s[k] for k in ("initial_cost", "final_cost", "iterations", "successful", "termination")}, launches() - n0))
        two, one, again = ends
        print("seed %d: %s, fused launches %d" % (c["seed"], one[1], one[2]))
        assert two[2] == 0 and one[2] > 0
        rejected += one[1]["successful"] < one[1]["iterations"]
        assert one[1] == again[1] == two[1], (one[1], again[1], two[1])
        for x, y, z in zip(one[0], again[0], two[0]):
            assert np.array_equal(x, y) and np.array_equal(x, z)
    assert rejected, "no step was rejected: raise the perturbation"
