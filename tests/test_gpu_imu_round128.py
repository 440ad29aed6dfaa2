"""The IMU integration's two round lengths against each other: one round of up to 128 steps per covariance block (the
default: waves 2 / 3 scan steps 64.. beside waves 0 / 1 and take the state after step 63 from them) and two rounds of 64
(SVIN_IMU_ROUND64, the form before).  The round length decides when the per-step phases run, not what they compute, so
every comparison is for equal bits.  tests/test_gpu_imu_edges.py holds whichever form is the default to the mpmath bars.

(a) every case of tests/golden/imu_edges.npz -- high halves of 1, 2 and 64 steps (counts 65, 66, 128), no high half
    (counts <= 64), a low half or a whole block of samples before t0, saturated samples either side of step 64, duplicate
    stamps at 63/64, blocks after the first (129 .. 640): propagation with covariance, Jacobian and integrals, and the
    factor's r and J behind its first integration and behind the fixture's bias steps (below and above the threshold)
(b) the fixture's chain window (intervals of 3, 64, 129, 9 and 257 samples in one window): r and J of every factor
(c) optimize(10) on a window of 4 keyframes with 100 steps per interval whose gyro biases start away from the
    pre-integration's: states, summary and every factor's count of re-integrations
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import imu_edges as E  # noqa: E402

from svin_amd import synthetic as syn   # noqa: E402

pytestmark = pytest.mark.gpu
T_SC = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])
OPTION = "SVIN_IMU_ROUND64"
SUMMARY = ("initial_cost", "final_cost", "iterations", "successful", "termination")


def new_estimator(par):
    from svin_amd.estimator import Estimator
    est = Estimator(0)
    est.add_camera(1, [450.0, 450.0, 376.0, 240.0], [0.0, 0.0, 0.0, 0.0], 752, 480, [0.0, 0.0, 0.0, 0.0])
    est.add_imu(par)
    return est


def imu_factors(est):
    return [f for f in est.eval_factors() if f["kind"] == 0]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_propagation_is_the_same_in_rounds_of_64_and_128(gpu_lib, debug_option):
    g = E.load()
    par = E.params(g)
    est = {0: new_estimator(par), 1: new_estimator(par)}
    assert len(g["count"]) == 41
    for i in range(len(g["count"])):
        t, m, t0, t1 = E.case(g, i)
        out = {}
        for round64 in (0, 1):
            debug_option(OPTION, round64)
            out[round64] = est[round64].imu_propagation(t, m, par, g["T0"][i], g["sb0"][i], t0, t1, want_cov=True, want_jac=True,
                                                        want_integrals=True)
        name = str(g["name"][i])
        assert out[0][0] == out[1][0] == int(g["used"][i]), (name, out[0][0], out[1][0])
        for what, a, b in zip(("T", "sb", "cov", "jac", "integrals"), out[0][1:], out[1][1:]):
            assert (a is None) == (b is None), (name, what)
            assert a is None or same_bits(a, b), "%s: %s differs by %.3e" % (name, what, float(np.max(np.abs(np.asarray(a) - np.asarray(b)))))


def test_factor_is_the_same_in_rounds_of_64_and_128(gpu_lib, debug_option):
    """two-frame windows as tests/test_gpu_imu_edges.py builds them: the first evaluation integrates, the bias step "a"
    stays below the redo threshold, "b" crosses it and integrates again"""
    g = E.load()
    par = E.params(g)
    bias = {int(c): k for k, c in enumerate(g["bias_case"])}
    compared = 0
    for i in range(len(g["count"])):
        if int(g["used"][i]) < 0:
            continue
        t, m, t0, t1 = E.case(g, i)
        out = {}
        for round64 in (0, 1):
            debug_option(OPTION, round64)
            est = new_estimator(par)
            f0, f1 = est.new_id(), est.new_id()
            assert est.add_states(f0, t0, 400, T_SC, t, m, True)
            assert est.set_T_WS(f0, g["T0"][i]) and est.set_speed_and_bias(f0, g["sb0"][i])
            assert est.add_states(f1, t1, 400, T_SC, t, m, False)
            assert est.set_T_WS(f1, g["T1"][i]) and est.set_speed_and_bias(f1, g["sb1"][i])
            (f,) = imu_factors(est)
            got = [("first integration", f["r"], f["J"])]
            if i in bias:
                for tag in ("a", "b"):
                    assert est.set_speed_and_bias(f0, g["sb0" + tag][bias[i]])
                    (f,) = imu_factors(est)
                    got.append(("bias step " + tag, f["r"], f["J"]))
            out[round64] = got
        for (what, r0, J0), (_, r1, J1) in zip(out[0], out[1]):
            assert same_bits(r0, r1) and same_bits(J0, J1), "%s, %s: r differs by %.3e, J by %.3e" % (
                g["name"][i], what, float(np.max(np.abs(r0 - r1))), float(np.max(np.abs(J0 - J1))))
            compared += 1
    assert compared > len(bias) > 0


def test_chain_window_is_the_same_in_rounds_of_64_and_128(gpu_lib, debug_option):
    g = E.load()
    par = E.params(g)
    nf = len(g["chain_count"])
    assert [int(c) for c in g["chain_count"]] == [3, 64, 129, 9, 257]
    out = {}
    for round64 in (0, 1):
        debug_option(OPTION, round64)
        est = new_estimator(par)
        fids = [est.new_id() for _ in range(nf + 1)]
        for f in range(nf + 1):
            t, m, _, _ = E.chain_case(g, max(f - 1, 0))
            assert est.add_states(fids[f], tuple(int(v) for v in g["chain_t"][f]), 400, T_SC, t, m, True)
        for f in range(nf + 1):
            assert est.set_T_WS(fids[f], g["chain_T"][f]) and est.set_speed_and_bias(fids[f], g["chain_sb"][f])
        facs = imu_factors(est)
        assert len(facs) == nf
        out[round64] = {fids.index(f["blocks"][0]): (f["r"], f["J"]) for f in facs}
    assert sorted(out[0]) == sorted(out[1]) == list(range(nf))
    for k in range(nf):
        assert same_bits(out[0][k][0], out[1][k][0]) and same_bits(out[0][k][1], out[1][k][1]), "chain interval %d (%d samples)" % (
            k, int(g["chain_count"][k]))


def test_solve_is_the_same_in_rounds_of_64_and_128(gpu_lib, debug_option):
    """frame_dt 0.5 s at 200 Hz: 100 steps per interval, a low half of 64 and a high half of 36.  The gyro biases move by
    0.02 rad/s behind the first pre-integration (0.02 * 0.5 s is a hundred times the threshold of 1e-4), so the solve's first
    evaluation integrates again, and so does every candidate whose step takes the biases back"""
    from svin_amd.estimator import Estimator
    spec = syn.make_window(P=4, L=64, n_obs=500, seed=31, frame_dt=0.5)

    def run(round64):
        debug_option(OPTION, round64)
        est = Estimator(0)
        fids, lids = syn.feed(est, spec)
        est.optimize(0)
        redo0 = est.debug_build_arrays()["imu_redo"]
        for f in fids:
            sb = est.get_speed_and_bias(f)
            sb[3:6] += 0.02
            assert est.set_speed_and_bias(f, sb)
        est.optimize(10)
        s = est.summary()
        T = np.stack([est.get_T_WS(f) for f in fids])
        sb = np.stack([est.get_speed_and_bias(f) for f in fids])
        lms = est.get_landmarks()
        lm = np.stack([np.r_[lms[l]["point"], lms[l]["quality"]] for l in lids])
        return (T, sb, lm), {k: s[k] for k in SUMMARY}, [int(v) for v in est.debug_build_arrays()["imu_redo"] - redo0]

    new, old = run(0), run(1)
    print("optimize(10): %s, re-integrations per factor %s (rounds of 128), %s (rounds of 64)" % (new[1], new[2], old[2]))
    assert len(new[2]) == 3 and new[2] == old[2] and max(new[2]) >= 2, (new[2], old[2])
    assert new[1] == old[1], (new[1], old[1])
    for what, a, b in zip(("poses", "speed / bias", "landmarks"), new[0], old[0]):
        assert same_bits(a, b), "%s differ by %.3e" % (what, float(np.max(np.abs(a - b))))
