"""Window::solve's loop on the device, on the smallest windows of tests/test_gpu_lm.py: what the accumulator ledger and the plan of
a pass (svin_amd/csrc/iteration_plan.hpp) decide must not show in any bit.

With SVIN_NO_SPECULATION every build is a fresh one in front of its solve, so that setting is the path independent of the ledger:
for the dogleg strategy and for Levenberg-Marquardt the four settings of SVIN_NO_SPECULATION x SVIN_NO_EVAL_BUILD end on the same
state bits, iteration log and final cost, and the log follows tests/helpers/lm_reference.py at the bounds of test_gpu_lm.py.  The
window ("imu": poses, speed / bias, IMU factors, from a start far off) is one whose REFERENCE log shows rejected steps under either
strategy -- asserted on the reference's log, so the test cannot pass by missing them.  SVIN_SPEC_BUILD_HITS / _MISSES move by what
the CPU shim's replay of the device's own log predicts (tests/csrc/iteration_plan_shim.cpp ip_replay: test_gpu_lm.py's
expected_hits for both strategies, the retry ladder included).  Four such windows in one optimize_batch end where each ends alone.

No small window was found on which the reference's dogleg solve walks the mu retry ladder (log column 4 above 1e-8):
tests/golden/tiny_window.npz with both poses free -- no pose prior, a six-dimensional gauge freedom -- factorises at 1e-8 on every
iteration from four starts; the damping of the scaled system is enough.  The ladder with a speculative build pending is walked on
the CPU only (tests/test_iteration_plan_host.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import iteration_plan_lib as ip  # noqa: E402
import lm_cases as cases  # noqa: E402
import lm_reference as ref  # noqa: E402
from test_gpu_lm import RADIUS_RTOL, device_run, log_, reference_run, spec_counters, state_bits  # noqa: E402

pytestmark = pytest.mark.gpu
WINDOW = "imu"
STRATEGIES = {"dogleg": None, "lm": "lm"}   # device_run's argument: a handle left at its defaults is the dogleg solve


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return ip.build_shim(tmp_path_factory.mktemp("iteration_plan"))


@pytest.mark.parametrize("strategy", ["dogleg", "lm"])
def test_four_switch_settings_one_result(gpu_lib, debug_option, shim, strategy):
    want = reference_run(WINDOW, strategy, 1e4)
    assert (want["log"][:, 5] == ref.REJECTED).any(), "the window's reference log has no rejected step"
    n_iter = cases.ESTIMATOR_WINDOWS[WINDOW][1]
    runs = {}
    for no_spec in (0, 1):
        for no_eval_build in (0, 1):
            debug_option("SVIN_NO_SPECULATION", no_spec)
            debug_option("SVIN_NO_EVAL_BUILD", no_eval_build)
            h0, m0 = spec_counters()
            est, fids, lids = device_run(WINDOW, STRATEGIES[strategy], 1e4)
            h1, m1 = spec_counters()
            log, s = est.iteration_log(), est.summary()
            runs[(no_spec, no_eval_build)] = (state_bits(est, fids, lids), log.tobytes(), s["final_cost"])
            hits, misses, passes = ip.replay(shim, log, strategy, no_spec, n_iter, terminated_pass=s["termination"] not in (1, 2))
            log_(strategy, "no_spec", no_spec, "no_eval_build", no_eval_build, "hits", h1 - h0, "misses", m1 - m0, "replay", hits, misses,
                 "passes", passes, "outcomes", log[:, 5].astype(int), "mu", log[:, 4])
            assert (h1 - h0, m1 - m0) == (hits, misses)
            if no_spec:
                assert (hits, misses) == (0, 0)
            else:
                assert hits > 0 and misses > 0
    assert len(set(runs.values())) == 1
    log = np.frombuffer(runs[(1, 1)][1]).reshape(-1, 6)
    assert ref.compare_logs(log, want["log"], 1e-5, RADIUS_RTOL) is None
    assert abs(runs[(1, 1)][2] - want["final_cost"]) <= 1e-5 * want["final_cost"]
    assert (log[:, 5] == ref.REJECTED).any()


def test_batch_of_four_ends_where_each_window_ends_alone(gpu_lib):
    """four dogleg windows with rejected steps, each under radii of its own, share their launches in one optimize_batch"""
    from svin_amd import estimator
    settings = [("dogleg", 1e4, 1e16), ("dogleg", 50.0, 1e3), ("dogleg", 1e2, 1e16), ("dogleg", 10.0, 1e16)]
    n = cases.ESTIMATOR_WINDOWS[WINDOW][1]

    def make(k):
        est = estimator.Estimator(0)
        fids, lids = cases.feed_estimator(est, WINDOW)
        est.set_solver_options(*cases.TIGHT)
        est.set_trust_region(*settings[k])
        return est, fids, lids

    def result(est, fids, lids):
        s = est.summary()
        return state_bits(est, fids, lids), est.iteration_log().tobytes(), s["iterations"], s["final_cost"], s["termination"], s["successful"]
    alone = []
    for k in range(4):
        est, fids, lids = make(k)
        est.optimize(n)
        alone.append(result(est, fids, lids))
    batch = [make(k) for k in range(4)]
    assert estimator.optimize_batch([b[0] for b in batch], n) == 4
    for k, b in enumerate(batch):
        assert result(*b) == alone[k], k
    logs = [np.frombuffer(a[1]).reshape(-1, 6) for a in alone]
    log_("batch: outcomes", [lg[:, 5].astype(int) for lg in logs])
    assert len({a[0] for a in alone}) >= 2 and any((lg[:, 5] == ref.REJECTED).any() for lg in logs)
