"""tests/golden/imu_edges.npz (50-digit mpmath, make_golden_imu_edges.py) against the two serial FP64 restatements of the
IMU pre-integration that run on the CPU: the oracle (orc_imu_propagation, OracleMap's ImuError) and the product's host
twin (svin_host_imu_propagation).  This validates the fixture independently of the GPU, and measures how far a
straightforward serial FP64 loop lands from the 50-digit values at every count and edge of the fixture.

Worst serial FP64 errors measured over all cases (over the oracle and the host twin; the bars of tests/helpers/imu_edges.py
in brackets):
  propagation  position 1.95e-13 [2e-12] and velocity 1.29e-13 [1.3e-12], both on the 640-sample case (3.2 s);
               integrals 1.43e-14 [1e-13], rotation 1.24e-15 [1e-13], covariance 4.18e-15 [1e-12], Jacobian 1.31e-15 [1e-12]
  factor       chi^2 1.93e-14 [1e-9], e 7.67e-12 [1e-8], H 1.69e-12 [1e-9], g 1.64e-13 [1e-9]  (bias steps and chain included)
Position and velocity are the only quantities a plain serial loop cannot hold to 1e-13: over 639 steps its rounding grows to
2e-13.  Their bars are 10x that worst serial error, for every case alike."""
import os
import sys

import numpy as np

from oracle import orc
from svin_amd import estimator

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import imu_edges as E  # noqa: E402


def oracle_propagation(par, t, m, T0, sb0, t0, t1):
    L = orc.lib()
    T, sb, cov, jac = orc.arr(T0).copy(), orc.arr(sb0).copy(), np.zeros((15, 15)), np.zeros((15, 15))
    used = L.orc_imu_propagation(len(t), orc.u32ptr(orc.arr(t, np.uint32)), orc.dptr(orc.arr(m)), orc.dptr(orc.imu_params_vector(par)),
                                 orc.dptr(T), orc.dptr(sb), t0[0], t0[1], t1[0], t1[1], orc.dptr(cov), orc.dptr(jac))
    return used, T, sb, cov, jac


def oracle_factor(m, rid):
    r, _, Jm = m.eval(rid)
    return r, np.concatenate(Jm, axis=1)


def test_fixture_cases_cover_the_edges():
    """the fixture holds what its generator promises: the count sweep, both streams, a -1 case, eight bias-step cases and
    the chain's very different interval lengths"""
    g = E.load()
    counts = set(int(c) for c in g["count"])
    assert {2, 3, 5, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 640}.issubset(counts)
    assert set(int(s) for s in g["stream"]) == {0, 1}
    assert list(g["used"]).count(-1) == 1
    assert len(g["bias_case"]) == 8 and list(g["chain_count"]) == [3, 64, 129, 9, 257]
    assert (g["used"] == 1).sum() == 2       # count 2 and the case with t0, t1 inside one sample interval


def test_propagation_serial_fp64_against_fixture():
    g = E.load()
    par = E.params(g)
    worst = {}
    for i in range(len(g["count"])):
        t, m, t0, t1 = E.case(g, i)
        used, T, sb, cov, jac = oracle_propagation(par, t, m, g["T0"][i], g["sb0"][i], t0, t1)
        nh, Th, sbh, covh, jach, integ = estimator.host_imu_propagation(t, m, par, g["T0"][i], g["sb0"][i], t0, t1, True, True)
        assert used == nh == int(g["used"][i]), (str(g["name"][i]), used, nh)
        if used < 0:
            assert np.array_equal(T, g["T0"][i]) and np.array_equal(Th, g["T0"][i])
            continue
        assert np.array_equal(sb[3:], g["sb0"][i][3:]) and np.array_equal(sbh[3:], g["sb0"][i][3:])
        E.fold(worst, E.prop_errors(g, i, T, sb[:3], cov, jac), "oracle " + str(g["name"][i]))
        E.fold(worst, E.prop_errors(g, i, Th, sbh[:3], covh, jach, integ), "host " + str(g["name"][i]))
    print("serial FP64 propagation vs mpmath:", E.report(worst))
    assert not E.failures(worst), E.failures(worst)


def test_factor_serial_fp64_against_fixture():
    """the oracle's ImuError in a Map, at the fixture's states; for the bias-step cases the same factor after sb0 moved
    below the redo threshold (linearised correction) and above it (re-integrated)"""
    g = E.load()
    pv = orc.imu_params_vector(E.params(g))
    worst = {}
    bias = {int(c): k for k, c in enumerate(g["bias_case"])}
    for i in range(len(g["count"])):
        if int(g["used"][i]) < 0:
            continue
        t, m, t0, t1 = E.case(g, i)
        mp_ = orc.OracleMap()
        for pid, key in ((1, "T0"), (2, "sb0"), (3, "T1"), (4, "sb1")):
            mp_.add_param(pid, orc.BLOCK_POSE if key[0] == "T" else orc.BLOCK_SPEEDBIAS, g[key][i])
        rid = mp_.add_imu(t, m, pv, t0, t1, [1, 2, 3, 4])
        r, J = oracle_factor(mp_, rid)
        E.fold(worst, E.factor_errors(r, J, g["e"][i], float(g["chi2"][i]), g["P_delta"][i], g["g"][i], g["H"][i]), str(g["name"][i]))
        if i in bias:
            k = bias[i]
            for tag in ("a", "b"):
                mp_.set_param(2, g["sb0" + tag][k])
                r, J = oracle_factor(mp_, rid)
                P = g["P_delta_b"][k] if tag == "b" else g["P_delta"][i]
                E.fold(worst, E.factor_errors(r, J, g["e_" + tag][k], float(g["chi2_" + tag][k]), P, g["g_" + tag][k], g["H_" + tag][k]),
                       "%s, bias step %s" % (g["name"][i], tag))
    # the chain: six frames, five factors on consecutive slices
    mp_ = orc.OracleMap()
    nf = len(g["chain_count"])
    for f in range(nf + 1):
        mp_.add_param(10 + 2 * f, orc.BLOCK_POSE, g["chain_T"][f])
        mp_.add_param(11 + 2 * f, orc.BLOCK_SPEEDBIAS, g["chain_sb"][f])
    for k in range(nf):
        t, m, t0, t1 = E.chain_case(g, k)
        rid = mp_.add_imu(t, m, pv, t0, t1, [10 + 2 * k, 11 + 2 * k, 12 + 2 * k, 13 + 2 * k])
        r, J = oracle_factor(mp_, rid)
        E.fold(worst, E.factor_errors(r, J, g["chain_e"][k], float(g["chain_chi2"][k]), g["chain_P_delta"][k], g["chain_g"][k],
                                      g["chain_H"][k]), "chain interval %d" % k)
    print("serial FP64 factor vs mpmath:", E.report(worst))
    assert not E.failures(worst), E.failures(worst)
