"""tests/helpers/lm_reference.py -- the float64 numpy restatement of Ceres 2.2's TrustRegionMinimizer with both strategies that
tests/test_gpu_lm.py holds the device's Levenberg-Marquardt solve against -- checked on the CPU.

(a) In dogleg mode it reproduces the oracle's own solve on the windows the GPU tests use: same iteration count, same accept /
    reject sequence, the same cost history.  The two are float64 evaluations of the same formulas in a different summation order (a
    dense Jacobian against the oracle's Schur complement), so the bound on the cost history is measured: DOGLEG_RTOL holds, per
    window, the worst relative discrepancy seen and ten times it, which is what is asserted.  The windows start far from their
    minimum (costs fall by three to five orders of magnitude in the first iterations), which is what amplifies a last-bit
    difference to 1e-8 on "imu" and, next to the prior's 1e16 entries, to 3e-6 on "prior".  This is what licenses the helper.
    The oracle keeps one residual vector, which its candidate evaluation overwrites: after a rejected step it forms the model cost
    change with the candidate's uncorrected residuals (orc_map.cpp, Problem::evalOne / Jtimes).  Ceres keeps the residuals of x, and
    so do the device and the helper's default; oracle_residual_vector=True reproduces the oracle for this comparison, and the test
    shows that the two readings part on the window with rejected steps and nowhere else.
(b) In Levenberg-Marquardt mode the cost never rises over accepted steps; with tolerances at 1e-14 the solve ends converged, at a
    point whose gradient maximum meets the gradient tolerance or whose last cost change meets the function tolerance; and its final
    cost agrees with the dogleg run's to the function tolerance.  The agreement is asserted on tests/golden/tiny_window.npz without
    its robust loss, where both strategies converge fast (7 to 18 iterations).  With CauchyLoss(1) the Gauss-Newton model
    over-estimates the curvature (Ceres' corrector drops the rho'' term when it is negative), both strategies converge linearly over
    some 220 iterations, and a run that stops when one step changes the cost by less than 1e-14 of itself is still a few such steps
    from the minimum: measured, Levenberg-Marquardt ends 2.9e-14 (radius 1e4) and 2.4e-14 (radius 0.1) below dogleg, relative.  That
    window is held to the first two properties and to 1e-12; the figures are printed.
(c) The starts reach the rules: the reference's own Levenberg-Marquardt log on "imu" has an accepted step with the 1/3 clamp
    active, one with it inactive, and two consecutive rejected steps.
(d) lm_reference.compare_logs, at the bounds test_gpu_lm.py uses, rejects a log produced with the decrease factor not doubling, one
    with the clamp at 1/2, and one whose rejected steps keep the old damping."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lm_cases as cases  # noqa: E402
import lm_reference as ref  # noqa: E402

# window -> (worst relative discrepancy of the cost history measured against the oracle, the bound asserted = ten times it)
DOGLEG_RTOL = {"imu": (1.93e-8, 1.93e-7), "imu_mild": (9.1e-12, 9.1e-11), "chain": (3.97e-9, 3.97e-8), "prior": (2.66e-6, 2.66e-5)}
CAUCHY = lambda rid: (ref.LOSS_CAUCHY, 1.0)   # noqa: E731
NO_LOSS = lambda rid: (ref.LOSS_NONE, 1.0)    # noqa: E731
GPU_COST_RTOL, GPU_RADIUS_RTOL = 1e-5, 1.5e-2   # tests/test_gpu_lm.py's bounds on the estimator-built windows (the wider pair)


@functools.lru_cache(maxsize=None)
def run(name, strategy, defect=None, oracle_residual_vector=False):
    from oracle import orc
    e = orc.OracleEstimator()
    cases.feed_estimator(e, name)
    out = ref.minimize(e.map(), strategy, cases.ESTIMATOR_WINDOWS[name][1], *cases.TIGHT, defect=defect,
                       oracle_residual_vector=oracle_residual_vector)
    out["log"].setflags(write=False)
    return out


@pytest.mark.parametrize("name", sorted(DOGLEG_RTOL))
def test_dogleg_mode_reproduces_the_oracle(oracle_lib, name):
    from oracle import orc
    o = orc.OracleEstimator()
    cases.feed_estimator(o, name)
    o.set_solver_options(*cases.TIGHT)
    o.optimize(cases.ESTIMATOR_WINDOWS[name][1])
    hist, s = np.array(o.cost_history()), o.summary()
    got = run(name, "dogleg", oracle_residual_vector=True)
    mine = np.array(got["cost_history"])
    assert got["iterations"] == s["iterations"] and got["successful"] == s["successful"] and got["termination"] == s["termination"]
    assert len(mine) == len(hist)
    seen = float(np.max(np.abs(mine - hist) / hist))
    print(name, "dogleg against the oracle: worst relative discrepancy of the cost history %.3e (recorded %.3e)" % (seen, DOGLEG_RTOL[name][0]))
    assert np.array_equal(mine[1:] < mine[:-1], hist[1:] < hist[:-1])          # the accept / reject sequence
    assert np.array_equal(got["log"][:, 5] == ref.ACCEPTED, hist[1:] < hist[:-1]) and not (got["log"][:, 5] == ref.INVALID).any()
    assert seen <= DOGLEG_RTOL[name][1]
    # Ceres' reading of the residual vector: the same solve unless a step was rejected
    ceres = run(name, "dogleg")
    rejected = (got["log"][:, 5] == ref.REJECTED).any()
    assert rejected == (name == "imu")
    assert np.array_equal(ceres["log"], got["log"]) == (not rejected)


def test_dogleg_mode_reproduces_the_oracle_map_on_the_tiny_window(oracle_lib):
    from oracle import orc
    g = cases.load_tiny()
    T1, lm = cases.tiny_start(g, 0.0)
    m = cases.tiny_on_oracle(orc, g, T1, lm)
    orc.lib().orc_map_set_tolerances(m.h, *cases.TIGHT)
    so = m.solve(30)
    got = ref.minimize(cases.tiny_on_oracle(orc, g, T1, lm), "dogleg", 30, *cases.TIGHT, loss_of=CAUCHY, oracle_residual_vector=True)
    seen = abs(got["final_cost"] - so["final_cost"]) / so["final_cost"]
    print("tiny window, dogleg against the oracle's Map::solve: final cost differs by %.3e relative" % seen)
    assert got["iterations"] == so["iterations"] == 30 and got["successful"] == so["successful"]
    # (measured 1e-15: 48 terms of a cost sum in another order; ten times that is the rounding of the sum itself, so the bound is
    # 48 terms x 2 ulp x the thirty iterations that carry it)
    assert got["initial_cost"] == pytest.approx(so["initial_cost"], rel=1e-14) and seen <= 1e-12


def check_lm_converged(out, ftol=1e-14, gtol=1e-14):
    acc = out["log"][out["log"][:, 5] == ref.ACCEPTED, 0]
    assert np.all(np.diff(np.r_[out["initial_cost"], acc]) <= 0.0)                      # non-increasing over accepted steps
    rej = out["log"][out["log"][:, 5] != ref.ACCEPTED]
    held = np.r_[out["initial_cost"], out["log"][:, 0]]
    assert all(held[i + 1] == held[i] for i in range(len(out["log"])) if out["log"][i, 5] != ref.ACCEPTED) and len(rej) < len(out["log"])
    assert out["termination"] == 0
    assert out["grad_max"] <= gtol or out["last_cost_change"] <= ftol * out["final_cost"]


@pytest.mark.parametrize("r0", [1e4, 1e-1])
def test_lm_mode_converges_where_dogleg_does(oracle_lib, r0):
    from oracle import orc
    g = cases.load_tiny()
    T1, lm = cases.tiny_start(g, 0.0)

    def solve(strategy, loss, radius):
        m = cases.tiny_on_oracle(orc, g, T1, lm, orc.LOSS_CAUCHY if loss is CAUCHY else orc.LOSS_NONE)
        return ref.minimize(m, strategy, 3000, *cases.TIGHT, initial_radius=radius, loss_of=loss)
    # without the robust loss: fast convergence, agreement to the function tolerance
    d, l = solve("dogleg", NO_LOSS, 1e4), solve("lm", NO_LOSS, r0)
    check_lm_converged(l)
    print("tiny window, no loss, r0 %g: LM %d iterations %.17g, dogleg %d iterations %.17g, relative difference %.2e" %
          (r0, l["iterations"], l["final_cost"], d["iterations"], d["final_cost"], (l["final_cost"] - d["final_cost"]) / d["final_cost"]))
    assert d["termination"] == 0 and abs(l["final_cost"] - d["final_cost"]) <= 1e-14 * d["final_cost"]
    # CauchyLoss(1): linear convergence (see the module's docstring, (b))
    d, l = solve("dogleg", CAUCHY, 1e4), solve("lm", CAUCHY, r0)
    check_lm_converged(l)
    print("tiny window, CauchyLoss(1), r0 %g: LM %d iterations %.17g, dogleg %d iterations %.17g, relative difference %.2e" %
          (r0, l["iterations"], l["final_cost"], d["iterations"], d["final_cost"], (l["final_cost"] - d["final_cost"]) / d["final_cost"]))
    assert abs(l["final_cost"] - d["final_cost"]) <= 1e-12 * d["final_cost"]
    assert abs(l["final_cost"] - float(g["cost"])) <= 1e-8 * float(g["cost"])     # the independent minimiser's (scipy) minimum


def test_the_windows_reach_the_rules(oracle_lib):
    ev = ref.log_events(run("imu", "lm")["log"])
    print("imu, Levenberg-Marquardt:", ev, run("imu", "lm")["log"][:, 5].astype(int))
    assert ev["clamped"] >= 1 and ev["unclamped"] >= 1 and ev["rejected_run"] >= 2, "raise the perturbation of lm_cases' imu window"
    for name in ("imu_mild", "chain", "prior"):     # the converging ones: what the speculative build's hit counter is read on
        log = run(name, "lm")["log"]
        assert (log[:, 5] == ref.ACCEPTED).all() and ref.log_events(log)["unclamped"] == 0


@pytest.mark.parametrize("defect", ["no_doubling", "clamp_half", "reject_keeps_damping"])
def test_the_log_comparison_rejects_planted_defects(oracle_lib, defect):
    good, bad = run("imu", "lm"), run("imu", "lm", defect=defect)
    assert ref.compare_logs(good["log"], good["log"], 0.0, 0.0) is None
    why = ref.compare_logs(bad["log"], good["log"], GPU_COST_RTOL, GPU_RADIUS_RTOL)
    print(defect, "->", why)
    assert why is not None
    assert ref.compare_logs(bad["log"][:-1], good["log"], 1.0, 1.0) is not None      # a missing row
    flipped = np.array(good["log"])
    flipped[3, 5] = ref.REJECTED
    assert "outcome" in ref.compare_logs(flipped, good["log"], 1.0, 1.0)
