"""CPU-side facts tests/test_gpu_constant_landmarks.py stands on, checked on the oracle alone (no GPU):
the fixtures do linearise constant landmarks, and the one-marginalisation procedure is independent of the iteration history only
with the IMU pre-integration settled ahead of the injection (helpers/constant_landmarks.constant_pass)."""
import numpy as np
import pytest

from svin_amd import synthetic as syn
from helpers import constant_landmarks as cl


def prior_gap(a, b):
    """worst entry of H and b0 between two priors of one ordering, in standard deviations"""
    sd = np.sqrt(np.maximum(np.abs(np.diag(b["H"])), 1e-300))
    return float(np.max(np.abs(a["H"] - b["H"]) / np.outer(sd, sd))), float(np.max(np.abs(a["b0"] - b["b0"]) / sd))


def test_one_shot_procedure_needs_the_imu_preintegration_settled(oracle_lib):
    """the same recorded states injected after optimize(11) and after optimize(12): as test_marginalization_one_shot does it the euroc
    fixture's priors differ by more than the 1e-8 bar (an IMU factor corrects to first order around the biases of its last
    pre-integration, ImuError.cpp:738-748, and those depend on the iterations run); with both sides evaluated at far gyro biases
    first they are bit-equal"""
    from oracle import orc
    spec = cl.one_shot_window("euroc")
    rec_0, _, _ = cl.constant_pass(orc.OracleEstimator(), spec)
    snaps = [r[0] for r in rec_0]
    gaps = {}
    for settle in (False, True):
        a, _, _ = cl.constant_pass(orc.OracleEstimator(), spec, snaps=snaps, iters=12, settle_imu=settle)
        b, _, _ = cl.constant_pass(orc.OracleEstimator(), spec, snaps=snaps, iters=11, settle_imu=settle)
        gaps[settle] = [prior_gap(x[2], y[2]) for x, y in zip(a, b) if x[2] is not None]
    print("history gap per frame, unsettled:", gaps[False], "settled:", gaps[True])
    assert max(g[0] for g in gaps[False]) > 1e-6 and max(g[1] for g in gaps[False]) > 1e-7
    assert all(g == (0.0, 0.0) for g in gaps[True])


@pytest.mark.parametrize("rig,n_lin,n_const", [("rig_v2", 76, 25), ("euroc", 22, 7)])
def test_one_shot_fixtures_linearise_constant_landmarks(oracle_lib, rig, n_lin, n_const):
    from oracle import orc
    rec, _, const = cl.constant_pass(orc.OracleEstimator(), cl.one_shot_window(rig))
    lm = rec[7][5]["lm"]
    assert len(const) == 84 and (len(lm), sum(1 for p in lm if p[1] == 0)) == (n_lin, n_const)


def test_resident_script_linearises_constant_landmarks(oracle_lib):
    """the frame script of the resident-against-host-pack test on the oracle: at least 5 constant landmarks are linearised"""
    from oracle import orc
    lin = []

    class Count(cl.NoChecks):
        def marginalised(self, k, results, cd):
            pre = cd.drv.ests[0].marg_pre()
            lin.append(sum(1 for p in pre["lm"] if p[1] == 0) if pre else 0)
    spec = cl.cut_tracks(syn.make_window(**cl.RESIDENT_WINDOW), cl.RESIDENT_CUT_AFTER)
    cd, removed = cl.run_resident_script([orc.OracleEstimator()], spec, Count(), iters=1, batched=False)
    assert sum(lin) >= 5 and len(cd.const) >= 5, lin
