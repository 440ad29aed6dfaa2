"""Levenberg-Marquardt as a trust-region strategy of the window solver (svin_ba_set_trust_region), on the device, against
tests/helpers/lm_reference.py -- Ceres 2.2's TrustRegionMinimizer with LevenbergMarquardtStrategy restated in float64 numpy on the
oracle's per-residual evaluation, licensed by tests/test_lm_reference_host.py (its dogleg mode reproduces the oracle's solve).

The iteration log (svin_ba_get_iteration_log) is what is compared: the outcome of every iteration equal, and the cost, radius and
damping columns within a relative bound (lm_reference.compare_logs, the comparison test_lm_reference_host.py shows to reject three
planted defects of the strategy).  Bounds: on tests/golden/tiny_window.npz 1e-9, what test_gpu_map.py and
test_gpu_reproj_information.py hold the dogleg solve of that window to; on the estimator-built windows, which stop unconverged,
1e-5 on the costs -- test_gpu_parity.test_rejected_steps_follow_the_oracle's bound for such runs -- and RADIUS_RTOL on radius and
damping (reasoned at its definition).  The windows are the smallest that reach each route (tests/helpers/lm_cases.py)."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lm_cases as cases  # noqa: E402
import lm_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# An accepted step below the clamp multiplies the radius by 1 / (1 - (2 rho - 1)^3), whose logarithmic derivative in rho is
# 6 (2 rho - 1)^2 / (1 - (2 rho - 1)^3) <= 6 * 0.764 / (1 / 3) < 14 there; rho = cost change / model change inherits the relative error
# of the cost (1e-5) times cost / |cost change|, and the tests assert that every unclamped accepted step of the reference's logs
# changes the cost by at least a hundredth of itself: 14 * 1e-5 * 100 < 1.5e-2.  Clamped and rejected steps scale the radius by
# constants (3, 1 / 2, 1 / 4, ...), so the bound still tells every rule of the strategy from its neighbours.
RADIUS_RTOL = 1.5e-2
CAUCHY = lambda rid: (ref.LOSS_CAUCHY, 1.0)   # noqa: E731


def log_(*a):
    print(*a, flush=True)


def worst(got, want):
    got, want = np.asarray(got).reshape(-1, 6), np.asarray(want).reshape(-1, 6)
    n = min(len(got), len(want))
    return [float(np.max(np.abs(got[:n, c] - want[:n, c]) / np.abs(want[:n, c]))) if n else 0.0 for c in (0, 2, 4)]


@functools.lru_cache(maxsize=None)
def reference_run(name, strategy, r0):
    """the numpy reference on the named estimator-built window (computed once, shared)"""
    from oracle import orc
    e = orc.OracleEstimator()
    cases.feed_estimator(e, name)
    out = ref.minimize(e.map(), strategy, cases.ESTIMATOR_WINDOWS[name][1], *cases.TIGHT, initial_radius=r0)
    out["log"].setflags(write=False)
    return out


def device_run(name, strategy, r0):
    from svin_amd.estimator import Estimator
    est = Estimator(0)
    fids, lids = cases.feed_estimator(est, name)
    est.set_solver_options(*cases.TIGHT)
    if strategy is not None:
        est.set_trust_region(strategy, r0, 1e16)
    est.optimize(cases.ESTIMATOR_WINDOWS[name][1])
    return est, fids, lids


def state_bits(est, fids, lids):
    return np.concatenate([est.get_T_WS(f) for f in fids] + [est.get_speed_and_bias(f) for f in fids] +
                          [est.get_landmark(l)["point"] for l in lids]).tobytes()


def unclamped_steps_move_the_cost(out):
    prev = out["initial_cost"]
    for row in out["log"]:
        if row[5] == ref.ACCEPTED and 1.0 - math.pow(2.0 * row[1] - 1.0, 3) > 1.0 / 3.0:
            assert prev - row[0] >= 0.01 * prev, "RADIUS_RTOL's premise does not hold on this window"
        prev = row[0]


@pytest.mark.parametrize("r0", [1e4, 1e-1])
def test_tiny_window_through_the_map_entry_points(gpu_lib, r0):
    from oracle import orc
    from svin_amd.estimator import Estimator
    g = cases.load_tiny()
    T1, lm = cases.tiny_start(g, 0.0)
    want = ref.minimize(cases.tiny_on_oracle(orc, g, T1, lm), "lm", 30, *cases.TIGHT, initial_radius=r0, loss_of=CAUCHY)
    est = cases.tiny_on_device(Estimator(0), g, T1, lm)
    est.set_solver_options(*cases.TIGHT)
    est.set_trust_region("lm", r0)
    est.optimize(30)
    got, s = est.iteration_log(), est.summary()
    log_("tiny window r0", r0, "iterations", s["iterations"], want["iterations"], "worst cost / radius / mu difference", worst(got, want["log"]))
    assert s["iterations"] == want["iterations"] and s["termination"] == want["termination"] and s["successful"] == want["successful"]
    assert ref.compare_logs(got, want["log"], 1e-9, 1e-9) is None
    assert got[0, 4] == 1.0 / r0 and abs(s["final_cost"] - want["final_cost"]) <= 1e-9 * want["final_cost"]
    assert est.get_trust_region() == dict(strategy="lm", initial_radius=r0, max_radius=1e16)


@pytest.mark.parametrize("name", ["imu", "imu_mild", "chain", "prior"])
def test_estimator_built_windows_follow_the_reference(gpu_lib, name):
    """"imu": IMU factors, from the start whose reference log has clamped and unclamped accepted steps and two rejected steps in a row;
    "chain": per-frame extrinsics, sonar and depth (the chain elimination); "prior": after two marginalisations"""
    want = reference_run(name, "lm", 1e4)
    unclamped_steps_move_the_cost(want)
    est, _, _ = device_run(name, "lm", 1e4)
    got, s = est.iteration_log(), est.summary()
    log_(name, "iterations", s["iterations"], want["iterations"], "outcomes", got[:, 5].astype(int), "worst cost / radius / mu difference",
         worst(got, want["log"]), "final", s["final_cost"], want["final_cost"])
    assert s["iterations"] == want["iterations"] and s["successful"] == want["successful"] and s["termination"] == want["termination"]
    assert ref.compare_logs(got, want["log"], 1e-5, RADIUS_RTOL) is None
    assert abs(s["final_cost"] - want["final_cost"]) <= 1e-5 * want["final_cost"]
    if name == "imu":
        ev = ref.log_events(got)
        assert ev["clamped"] >= 1 and ev["unclamped"] >= 1 and ev["rejected_run"] >= 2


def test_the_step_is_the_gauss_newton_step_exactly(gpu_lib):
    """one iteration through svin_ba_debug_trust_region_step with the radius the solve hands the device in Levenberg-Marquardt mode
    (+inf), in every form the window takes: cg = 0 and cn = 1, |J delta|^2 = |J y|^2 and (J delta).r = -(J y).r to the bit, the
    candidate Plus(x, -y) -- Euclidean blocks and positions to the bit, quaternions as exp(-y_alpha) * q -- and the whole record
    equal, bit for bit, to the one a finite radius beyond the step gives (the dogleg solve's Gauss-Newton branch)"""
    from svin_amd.estimator import Estimator
    est = Estimator(0)
    fids, lids = cases.feed_estimator(est, "imu_mild")
    lin = est.linearize()
    row_of = {int(b): int(o) for b, o in zip(lin["block_ids"], lin["block_off"])}   # the variable blocks' rows in the reduced system
    forms = 0
    for form in (0, 1, 2, 3):
        try:
            a = est.debug_trust_region_step(1e-4, math.inf, form)
        except RuntimeError:
            continue
        forms += 1
        b = est.debug_trust_region_step(1e-4, 1e300, form)
        sc = a["scalars"]
        assert sc["cholFail"] == 0 and sc["jdSq"] == sc["jySq"] and sc["jdDotR"] == -sc["jyDotR"]
        assert sc["doglegStepNorm"] == math.sqrt(sc["gnHatSq"]) and sc["jdSq"] > 0.0
        for k in ("y_C", "y_L", "lm_cand"):
            assert np.array_equal(a[k], b[k]), k
        assert all(np.array_equal(u, v) for u, v in zip(a["block_cand"], b["block_cand"]))
        assert {k: v for k, v in sc.items() if k != "gather"} == {k: v for k, v in b["scalars"].items() if k != "gather"}
        for lid, y, cand in zip(a["lm_ids"], a["y_L"], a["lm_cand"]):
            x = est.get_parameter_block(int(lid))
            assert np.array_equal(cand[:3], x[:3] + (-y)) and cand[3] == x[3]
        moved = 0
        for bid, kind, cand in zip(a["block_ids"], a["block_kind"], a["block_cand"]):
            x = est.get_parameter_block(int(bid))
            n = 9 if len(cand) == 9 else 6
            if int(bid) not in row_of:      # a constant block: the candidate is the block
                assert np.array_equal(cand, x)
                continue
            y = a["y_C"][row_of[int(bid)]:row_of[int(bid)] + n]
            moved += n
            if n == 9:
                assert np.array_equal(cand, x + (-y))
            else:
                assert np.array_equal(cand[:3], x[:3] + (-y[:3]))
                want = ref.plus((7, 6), x, -y)
                assert np.max(np.abs(cand[3:] - want[3:])) <= 4 * np.finfo(float).eps
        assert moved == a["d"] == lin["d"]
    assert forms >= 2


def spec_counters():
    from svin_amd.estimator import Estimator
    return Estimator.debug_get_option("SVIN_SPEC_BUILD_HITS"), Estimator.debug_get_option("SVIN_SPEC_BUILD_MISSES")


def expected_hits(log, max_radius=1e16):
    """iterations that follow a step whose speculative build assumed the damping it left: accepted, radius = min(max, 3 x before)"""
    return sum(1 for row in log[:-1] if row[5] == ref.ACCEPTED and row[2] == min(max_radius, (1.0 / row[4]) / (1.0 / 3.0)))


@pytest.mark.parametrize("name", ["imu_mild", "imu"])
def test_speculation_changes_no_bit_and_counts_its_hits(gpu_lib, debug_option, name):
    runs = {}
    for no_spec in (0, 1):
        for no_eval_build in (0, 1):
            debug_option("SVIN_NO_SPECULATION", no_spec)
            debug_option("SVIN_NO_EVAL_BUILD", no_eval_build)
            h0, m0 = spec_counters()
            est, fids, lids = device_run(name, "lm", 1e4)
            h1, m1 = spec_counters()
            runs[(no_spec, no_eval_build)] = (state_bits(est, fids, lids), est.iteration_log().tobytes(), est.summary()["final_cost"])
            log = est.iteration_log()
            n = est.summary()["iterations"]
            assert est.summary()["termination"] == 1 and n == len(log)   # (stopped by the iteration limit: every iteration has its row)
            log_(name, "no_spec", no_spec, "no_eval_build", no_eval_build, "hits", h1 - h0, "misses", m1 - m0, "expected hits", expected_hits(log),
                 "of", n - 1, "speculative builds")
            if no_spec:
                assert (h1 - h0, m1 - m0) == (0, 0)
            else:   # every iteration but the last enqueues a speculative build
                assert h1 - h0 == expected_hits(log) and m1 - m0 == (n - 1) - expected_hits(log)
    assert len(set(runs.values())) == 1
    log = np.frombuffer(runs[(0, 0)][1]).reshape(-1, 6)
    if name == "imu":
        assert 0 < expected_hits(log) < len(log) - 1     # (hits and misses both happen on this window)
    else:
        assert expected_hits(log) == len(log) - 1        # (a converging window: every step accepted with the clamp active)


def test_speculation_counters_count_for_dogleg_too(gpu_lib):
    h0, m0 = spec_counters()
    est, _, _ = device_run("imu", None, None)
    h1, m1 = spec_counters()
    log = est.iteration_log()
    log_("dogleg: hits", h1 - h0, "misses", m1 - m0, "outcomes", log[:, 5].astype(int))
    assert h1 - h0 > 0 and m1 - m0 > 0 and (log[:, 5] == ref.REJECTED).any()
    # a speculative build is kept exactly when the step it assumed was accepted (the mu ladder did not run on this window)
    assert h1 - h0 <= int((log[:-1, 5] == ref.ACCEPTED).sum())


def test_batch_of_both_strategies_ends_where_each_window_ends_alone(gpu_lib):
    """four windows in one optimize_batch, two Levenberg-Marquardt (different initial radii) and two dogleg (one with its own
    radii): the Levenberg-Marquardt windows take the ordinary path inside the call, the dogleg ones share their launches"""
    from svin_amd import estimator
    settings = [("lm", 1e4, 1e16), ("dogleg", 1e4, 1e16), ("lm", 1e2, 1e16), ("dogleg", 50.0, 1e3)]
    n = cases.ESTIMATOR_WINDOWS["imu_mild"][1]

    def make(k):
        est = estimator.Estimator(0)
        fids, lids = cases.feed_estimator(est, "imu_mild")
        est.set_solver_options(*cases.TIGHT)
        est.set_trust_region(*settings[k])
        return est, fids, lids
    alone = []
    for k in range(4):
        est, fids, lids = make(k)
        est.optimize(n)
        alone.append((state_bits(est, fids, lids), est.iteration_log().tobytes(), est.summary()["iterations"]))
    batch = [make(k) for k in range(4)]
    n_batched = estimator.optimize_batch([b[0] for b in batch], n)
    log_("batched", n_batched, "of 4")
    assert n_batched == 2
    for k, (est, fids, lids) in enumerate(batch):
        assert (state_bits(est, fids, lids), est.iteration_log().tobytes(), est.summary()["iterations"]) == alone[k], k
    assert len({a[0] for a in alone}) == 4


def test_nothing_moved_for_dogleg(gpu_lib):
    """a handle left at its defaults and one set to ("dogleg", 1e4, 1e16) end on the same bits, on the window whose dogleg solve
    rejects steps; the dogleg iteration log's costs are the oracle's cost history (a window without rejected steps: after one, the
    oracle forms its model cost change with the residual vector its candidate evaluation overwrote -- lm_reference.minimize's
    oracle_residual_vector -- which the device, like Ceres, does not), and on the window with rejected steps the log is the numpy
    reference's in dogleg mode"""
    from oracle import orc
    a, fa, la = device_run("imu", None, None)
    b, fb, lb = device_run("imu", "dogleg", 1e4)
    assert state_bits(a, fa, la) == state_bits(b, fb, lb) and a.iteration_log().tobytes() == b.iteration_log().tobytes()
    assert a.get_trust_region() == b.get_trust_region() == dict(strategy="dogleg", initial_radius=1e4, max_radius=1e16)
    want, log = reference_run("imu", "dogleg", 1e4), a.iteration_log()
    log_("dogleg log against the reference's:", worst(log, want["log"]), log[:, 5].astype(int))
    assert ref.compare_logs(log, want["log"], 1e-5, RADIUS_RTOL) is None
    assert log[0, 4] == 1e-8 and (log[:, 5] == ref.REJECTED).any()
    m, fm, lm = device_run("imu_mild", None, None)
    o = orc.OracleEstimator()
    cases.feed_estimator(o, "imu_mild")
    o.set_solver_options(*cases.TIGHT)
    o.optimize(cases.ESTIMATOR_WINDOWS["imu_mild"][1])
    hist, log = np.array(o.cost_history()), m.iteration_log()
    log_("dogleg log against the oracle's cost history:", float(np.max(np.abs(log[:, 0] - hist[1:]) / hist[1:])), log[:, 5].astype(int))
    assert len(log) == len(hist) - 1 == m.summary()["iterations"]
    # (test_rejected_steps_follow_the_oracle's bound for runs that stop unconverged)
    assert np.all(np.abs(log[:, 0] - hist[1:]) <= 1e-5 * hist[1:])
    assert np.array_equal(log[:, 5] == ref.ACCEPTED, hist[1:] < hist[:-1])


def test_return_codes(gpu_lib):
    from svin_amd import estimator
    est = estimator.Estimator(0)
    L, h = est.L, est.h
    assert est.get_trust_region() == dict(strategy="dogleg", initial_radius=1e4, max_radius=1e16)
    assert L.svin_ba_set_trust_region(h, 1, 5.0, 7.0) == 1
    assert est.get_trust_region() == dict(strategy="lm", initial_radius=5.0, max_radius=7.0)
    for bad in ((2, 1.0, 2.0), (-1, 1.0, 2.0), (1, 0.0, 2.0), (1, -1.0, 2.0), (0, math.inf, math.inf), (1, 1.0, math.inf), (0, math.nan, 2.0),
                (0, 1.0, math.nan), (1, 3.0, 2.0)):
        assert L.svin_ba_set_trust_region(h, *bad) == estimator.SVIN_ERR_INVALID_ARG, bad
        assert est.get_trust_region() == dict(strategy="lm", initial_radius=5.0, max_radius=7.0)
    assert L.svin_ba_set_trust_region(None, 0, 1.0, 2.0) == estimator.SVIN_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        est.set_trust_region("gauss-newton")
    with pytest.raises(RuntimeError):
        est.set_trust_region("lm", 2.0, 1.0)
    assert L.svin_ba_set_trust_region(h, 1, 3.0, 3.0) == 1      # max == initial is allowed
    # a handle with Levenberg-Marquardt set is not taken into landmark-sharded mode; world = 1 is not sharded
    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p)(lambda *args: 1)
    assert L.svin_ba_set_distributed(h, 0, 2, C.cast(cb, C.c_void_p), None) == estimator.SVIN_ERR_UNSUPPORTED
    assert L.svin_ba_set_distributed_rccl(h, 0, 2, bytes(128)) == estimator.SVIN_ERR_UNSUPPORTED
    assert L.svin_ba_set_distributed(h, 0, 1, None, None) == 1
    # and the other way round: a sharded handle refuses the strategy, keeps what it had, and still takes radii for dogleg
    other = estimator.Estimator(0)
    assert other.L.svin_ba_set_distributed(other.h, 0, 2, C.cast(cb, C.c_void_p), None) == 1
    assert other.L.svin_ba_set_trust_region(other.h, 1, 1e4, 1e16) == estimator.SVIN_ERR_UNSUPPORTED
    assert other.L.svin_ba_set_trust_region(other.h, 0, 10.0, 1e3) == 1
    assert other.get_trust_region() == dict(strategy="dogleg", initial_radius=10.0, max_radius=1e3)
    assert other.L.svin_ba_set_distributed(other.h, 0, 1, None, None) == 1
    # the iteration log of a handle that has not solved is empty; bad arguments
    n = C.c_int32(-1)
    assert L.svin_ba_get_iteration_log(h, 0, None, C.byref(n)) == 1 and n.value == 0 and est.iteration_log().shape == (0, 6)
    assert L.svin_ba_get_iteration_log(h, 3, None, C.byref(n)) == estimator.SVIN_ERR_INVALID_ARG
    assert L.svin_ba_get_iteration_log(h, -1, None, C.byref(n)) == estimator.SVIN_ERR_INVALID_ARG


def test_shim_program_ends_on_the_bits_of_the_python_binding(gpu_lib, tmp_path):
    """tests/csrc/shim_trust_region.cpp: a TestMap-shaped problem solved through okvis::ceres::Map with LEVENBERG_MARQUARDT and an
    initial radius of 100, against the same problem built here through the C ABI with the same settings"""
    import subprocess
    from svin_amd import synthetic as syn
    from svin_amd.estimator import Estimator
    from test_shim_compile import _compile
    exe = _compile(tmp_path, "shim_trust_region")
    p = subprocess.run([exe, "lm", "100", "1e6"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    obs, rows, tail, got = [], [], None, None
    for line in p.stdout.splitlines():
        t = line.split()
        if t[0] == "obs":
            obs.append((int(t[1]), np.array([float(t[2]), float(t[3])]), np.array([float(x) for x in t[4:7]])))
        elif t[0] == "row":
            rows.append([float(x) for x in t[1:7]])
        elif t[0] == "get":
            got = (int(t[1]), float(t[2]), float(t[3]))
        elif t[0] == "pose":
            tail = (np.array([float(x) for x in t[1:8]]), {t[i]: t[i + 1] for i in range(8, len(t) - 1, 2)})
    assert len(obs) == 90 and tail is not None and got == (1, 100.0, 1e6)
    est = Estimator(0)
    est.add_camera(syn.DIST_EQUIDISTANT, [350.0, 360.0, 378.0, 238.0], [-0.21, 0.14, 0.0006, 0.0003], 752, 480, [0, 0, 0, 0])
    assert est.map_add_parameter_block(1, est.BLOCK_POSE, np.r_[1.4, -2.3, 0.2, 0, 0, 0, 1.0])
    assert est.map_add_parameter_block(2, est.BLOCK_POSE, np.r_[0.1, -0.05, 0.02, 0, 0, 0, 1.0]) and est.set_parameter_block_constant(2)
    for i, (pid, uv, pw) in enumerate(obs):
        assert pid == i + 3
        assert est.map_add_parameter_block(pid, est.BLOCK_HOMOGENEOUS_POINT, np.r_[pw, 1.0]) and est.set_parameter_block_constant(pid)
        rid = est.map_add_reprojection_error(1, pid, 2, 0, uv, np.eye(2))
        assert rid != 0 and est.map_set_residual_loss(rid, 0)
    est.set_solver_options(1e-6, 1e-10, 1e-8)   # okvis::ceres::Map::Options' defaults
    est.set_trust_region("lm", 100.0, 1e6)
    est.optimize(20)
    s, log = est.summary(), est.iteration_log()
    log_("shim", tail[1], "C ABI", s["final_cost"], s["iterations"], "rows", len(rows), len(log))
    assert int(tail[1]["iterations"]) == s["iterations"] and float(tail[1]["final_cost"]) == s["final_cost"]
    assert np.array_equal(np.array(rows).reshape(-1, 6), log) and len(log) > 0 and log[0, 4] == 1.0 / 100.0
    assert np.array_equal(tail[0], est.get_parameter_block(1))
    # and it is not what the dogleg solve of the same problem gives
    q = subprocess.run([exe, "dogleg", "1e4", "1e16"], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0 and [ln for ln in q.stdout.splitlines() if ln.startswith("row")] != [ln for ln in p.stdout.splitlines() if ln.startswith("row")]
