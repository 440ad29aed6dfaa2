"""The device's IMU pre-integration (imuIntegrate: rounds of 64 steps, covariance blocks of 128 in four segments) against
tests/golden/imu_edges.npz (50-digit mpmath, make_golden_imu_edges.py) at the sample counts and interval edges where its
tiling can go wrong: counts 2..257 and 640 across the round / block boundaries, interval ends on samples, whole rounds and
blocks of samples before t0, samples after t1, duplicate stamps, saturated samples on round boundaries, IMU gaps either side
of the series branches, the production-like 5-12 samples per interval, and a deque that ends before t1.

Propagation (k_imu_propagation) and the factor (imuRedoPreintegration in the factor evaluation) are held to the bars of
tests/helpers/imu_edges.py, the same for every case; test_imu_edges_host.py holds the serial FP64 loops to the same bars."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import imu_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu
T_SC = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])


def new_estimator(par):
    from svin_amd.estimator import Estimator
    est = Estimator(0)
    est.add_camera(1, [450.0, 450.0, 376.0, 240.0], [0.0, 0.0, 0.0, 0.0], 752, 480, [0.0, 0.0, 0.0, 0.0])
    est.add_imu(par)
    return est


def imu_factors(est):
    return [f for f in est.eval_factors() if f["kind"] == 0]


def test_imu_propagation_edges_match_mpmath(gpu_lib):
    g = E.load()
    par = E.params(g)
    est = new_estimator(par)
    worst = {}
    for i in range(len(g["count"])):
        t, m, t0, t1 = E.case(g, i)
        used, T, sb, cov, jac, integ = est.imu_propagation(t, m, par, g["T0"][i], g["sb0"][i], t0, t1, want_cov=True, want_jac=True,
                                                           want_integrals=True)
        assert used == int(g["used"][i]), (str(g["name"][i]), used)
        if used < 0:
            assert np.array_equal(T, g["T0"][i]) and np.array_equal(sb, g["sb0"][i])
            continue
        E.fold(worst, E.prop_errors(g, i, T, sb[:3], cov, jac, integ), str(g["name"][i]))
    print("device propagation vs mpmath:", E.report(worst))
    assert not E.failures(worst), E.failures(worst)


def test_imu_factor_edges_match_mpmath(gpu_lib):
    """two-frame windows built like the pipeline builds them (addStates with the slice, states set to the fixture's); for the
    bias-step cases sb0 then moves below the redo threshold (linearised correction, no re-integration) and above it
    (re-integrated at the new biases)"""
    g = E.load()
    par = E.params(g)
    bias = {int(c): k for k, c in enumerate(g["bias_case"])}
    worst = {}
    for i in range(len(g["count"])):
        if int(g["used"][i]) < 0:
            continue
        t, m, t0, t1 = E.case(g, i)
        est = new_estimator(par)
        f0, f1 = est.new_id(), est.new_id()
        assert est.add_states(f0, t0, 400, T_SC, t, m, True)
        assert est.set_T_WS(f0, g["T0"][i]) and est.set_speed_and_bias(f0, g["sb0"][i])
        assert est.add_states(f1, t1, 400, T_SC, t, m, False)
        assert est.set_T_WS(f1, g["T1"][i]) and est.set_speed_and_bias(f1, g["sb1"][i])
        facs = imu_factors(est)
        assert len(facs) == 1 and facs[0]["m"] == 15 and facs[0]["J"].shape == (15, 30)
        E.fold(worst, E.factor_errors(facs[0]["r"], facs[0]["J"], g["e"][i], float(g["chi2"][i]), g["P_delta"][i], g["g"][i], g["H"][i]),
               str(g["name"][i]))
        if i in bias:
            k = bias[i]
            for tag in ("a", "b"):
                assert est.set_speed_and_bias(f0, g["sb0" + tag][k])
                (f,) = imu_factors(est)
                P = g["P_delta_b"][k] if tag == "b" else g["P_delta"][i]
                E.fold(worst, E.factor_errors(f["r"], f["J"], g["e_" + tag][k], float(g["chi2_" + tag][k]), P, g["g_" + tag][k], g["H_" + tag][k]),
                       "%s, bias step %s" % (g["name"][i], tag))
    print("device factor vs mpmath:", E.report(worst))
    assert not E.failures(worst), E.failures(worst)


def test_imu_factor_chain_window_matches_mpmath(gpu_lib):
    """one window of six frames whose IMU intervals hold 3, 64, 129, 9 and 257 samples: every factor reads its own slice of
    the packed sample pool"""
    g = E.load()
    par = E.params(g)
    est = new_estimator(par)
    nf = len(g["chain_count"])
    fids = [est.new_id() for _ in range(nf + 1)]
    for f in range(nf + 1):
        t, m, _, _ = E.chain_case(g, max(f - 1, 0))
        assert est.add_states(fids[f], tuple(int(v) for v in g["chain_t"][f]), 400, T_SC, t, m, True)
    for f in range(nf + 1):
        assert est.set_T_WS(fids[f], g["chain_T"][f]) and est.set_speed_and_bias(fids[f], g["chain_sb"][f])
    facs = imu_factors(est)
    assert len(facs) == nf
    worst = {}
    for f in facs:
        k = fids.index(f["blocks"][0])
        assert f["blocks"][2] == fids[k + 1]
        E.fold(worst, E.factor_errors(f["r"], f["J"], g["chain_e"][k], float(g["chain_chi2"][k]), g["chain_P_delta"][k], g["chain_g"][k],
                                      g["chain_H"][k]), "chain interval %d (%d samples)" % (k, int(g["chain_count"][k])))
    print("device chain window vs mpmath:", E.report(worst))
    assert not E.failures(worst), E.failures(worst)


def test_imu_factor_map_builder_matches_mpmath(gpu_lib):
    """ImuError through the Map builder (svin_ba_map_add_imu_error) on blocks named by the caller: the same values as the
    window path"""
    from svin_amd.estimator import Estimator
    g = E.load()
    par = E.params(g)
    names = [str(n) for n in g["name"]]
    worst = {}
    for name in ("count 5", "count 129", "duplicate stamps at 63/64"):
        i = names.index(name)
        t, m, t0, t1 = E.case(g, i)
        est = Estimator(0)
        for bid, key in ((1, "T0"), (2, "sb0"), (3, "T1"), (4, "sb1")):
            assert est.map_add_parameter_block(bid, est.BLOCK_POSE if key[0] == "T" else est.BLOCK_SPEED_AND_BIAS, g[key][i])
        rid = est.map_add_imu_error([1, 2, 3, 4], t, m, par, t0, t1)
        assert rid != 0
        (f,) = [f for f in est.eval_factors() if f["res_id"] == rid]
        E.fold(worst, E.factor_errors(f["r"], f["J"], g["e"][i], float(g["chi2"][i]), g["P_delta"][i], g["g"][i], g["H"][i]), name)
    print("device Map-built factor vs mpmath:", E.report(worst))
    assert not E.failures(worst), E.failures(worst)
