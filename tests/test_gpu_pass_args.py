"""What a single launch is told besides the window -- where its cost sum publishes the scalars, whether the evaluation moves the
landmarks, whether the build may fork onto the side lane -- is an argument of that launch (svin_amd/csrc/kernels.hpp PassArgs), and a
window's own problem is constant from one pack() to the next.  So nothing an entry point did on a handle may show in the next one:

1. a handle that ran the inspection hooks solves exactly as a fresh one;
2. a handle that took part in a batched solve solves on, alone, exactly as one that solved alone before;
3. the side lane of the wide window -- the one host flag that used to travel in the problem itself -- at its smallest shape:
   switched off it changes nothing beyond rounding, and the step hook, which sets it too, leaves nothing behind.

These pin behaviour, not a layout: they hold on either side of the change that introduced PassArgs."""
import os
import sys

import numpy as np
import pytest

from svin_amd import synthetic as syn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lm_cases as cases  # noqa: E402
import solve_plan_lib as spl  # noqa: E402
from test_gpu_lm import log_, state_bits  # noqa: E402

pytestmark = pytest.mark.gpu
WINDOW = "imu"


def result(est, fids, lids):
    s = est.summary()
    return state_bits(est, fids, lids), est.iteration_log().tobytes(), s["iterations"], s["final_cost"], s["termination"], s["successful"]


def imu_handle(strategy=("dogleg", 1e4, 1e16)):
    from svin_amd.estimator import Estimator
    est = Estimator(0)
    fids, lids = cases.feed_estimator(est, WINDOW)
    est.set_solver_options(*cases.TIGHT)
    est.set_trust_region(*strategy)
    return est, fids, lids


def tiny_handle(strategy):
    from svin_amd.estimator import Estimator
    g = cases.load_tiny()
    T1, lm = cases.tiny_start(g, 1.0)
    est = cases.tiny_on_device(Estimator(0), g, T1, lm)
    est.set_solver_options(*cases.TIGHT)
    est.set_trust_region(*strategy)
    return est, g


def tiny_result(est, g):
    s = est.summary()
    blocks = [est.get_parameter_block(2)] + [est.get_parameter_block(10 + l) for l in range(len(g["lm_init"]))]
    return np.concatenate(blocks).tobytes(), est.iteration_log().tobytes(), s["iterations"], s["final_cost"], s["termination"], s["successful"]


def run_hooks(est, fused_form):
    """every hook that launches with an argument of its own: the step, uncommitted, in form 2 (k_step_retract moves the landmarks)
    and in the fused form the window takes (3: the candidate evaluation moves them -- the form that sets lmDeferred; 1 on a window
    whose evaluation is not the fused one, which refuses 3); the reduced solve in the form optimize() runs; linearize()"""
    assert est.debug_trust_region_step(1e-8, 1e4, form=0, commit=False)["form_solve"] == fused_form
    for form in (2, fused_form):
        out = est.debug_trust_region_step(1e-8, 1e4, form=form, commit=False)
        assert out["form"] == form
    est.debug_reduced_solve(1e-8, fused=True)
    est.linearize(1e-8)


@pytest.mark.parametrize("strategy", ["dogleg", "lm"])
def test_a_handles_history_does_not_show(gpu_lib, strategy):
    """imu: IMU factors and reprojection residuals, the fused evaluation (k_eval_all / k_eval_build); tiny: reprojection residuals
    alone, the split evaluation whose cost a launch of its own sums and publishes.  An IMU factor re-preintegrates on its first
    evaluation and keeps the state; the hooks evaluate at the very point optimize() starts from, so the state they leave is the one
    optimize() computes -- the hooks stay in the sequence on both windows."""
    tr = (strategy, 1e4, 1e16)
    n = cases.ESTIMATOR_WINDOWS[WINDOW][1]
    a = imu_handle(tr)
    run_hooks(a[0], 3)
    a[0].optimize(n)
    b = imu_handle(tr)
    b[0].optimize(n)
    ra, rb = result(*a), result(*b)
    log_(strategy, "imu: iterations", ra[2], rb[2], "final cost", ra[3], rb[3])
    assert ra == rb
    assert ra[2] > 2
    ta, g = tiny_handle(tr)
    run_hooks(ta, 1)
    ta.optimize(12)
    tb, _ = tiny_handle(tr)
    tb.optimize(12)
    ra, rb = tiny_result(ta, g), tiny_result(tb, g)
    log_(strategy, "tiny: iterations", ra[2], rb[2], "final cost", ra[3], rb[3])
    assert ra == rb
    assert ra[2] > 2


def test_a_batch_leaves_nothing_behind(gpu_lib):
    """the four windows of test_gpu_solve_loop.py's batch (each under radii of its own): optimize_batch, then every handle alone,
    against four fresh handles that solve alone twice"""
    from svin_amd import estimator
    settings = [("dogleg", 1e4, 1e16), ("dogleg", 50.0, 1e3), ("dogleg", 1e2, 1e16), ("dogleg", 10.0, 1e16)]
    n = cases.ESTIMATOR_WINDOWS[WINDOW][1]
    alone = [imu_handle(settings[k]) for k in range(4)]
    first_alone = []
    for h in alone:
        h[0].optimize(n)
        first_alone.append(result(*h))
        h[0].optimize(n)
    batch = [imu_handle(settings[k]) for k in range(4)]
    assert estimator.optimize_batch([b[0] for b in batch], n) == 4
    for k, b in enumerate(batch):
        assert result(*b) == first_alone[k], k
        b[0].optimize(n)
    for k in range(4):
        log_("window", k, "second solve: iterations", result(*alone[k])[2], result(*batch[k])[2])
        assert result(*batch[k]) == result(*alone[k]), k
    assert len({r[0] for r in first_alone}) >= 2


# ---- the side lane at its smallest: the block-pair form with the speed / bias chain eliminated takes more than 254 camera rows
# (43 variable poses: 258)
SIDE = dict(P=43, L=320, n_obs=3200, frame_dt=0.25)


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return spl.build_shim(tmp_path_factory.mktemp("solve_plan"))


def test_side_lane_at_its_smallest(gpu_lib, debug_option, planner):
    """Agreement as in test_gpu_wide_paths.py (the side lane reorders sums: same iteration count, cost to 1e-11 relative, poses to
    1e-9).  The wide build sums with atomic additions whose order is not fixed, so two runs of one library agree to rounding only
    (profiles/iteration_plan_bits.txt, wide_P46): the handle that ran the step hook is held to the fresh one at the same bounds.
    Each setting of SVIN_NO_SB_EARLY solves twice on a handle of its own, fed alike, as in test_gpu_wide_paths.py: the second of two
    settings on ONE handle would start where the first ended and could be compared with nothing.  The step hook then runs on the
    handle of the default setting."""
    from svin_amd.estimator import Estimator
    spec = syn.make_window(**SIDE)

    def handle():
        est = Estimator(0)
        fids, _ = syn.feed(est, spec)
        return est, fids

    def solved(est, fids):
        s = est.summary()
        return s["final_cost"], s["iterations"], np.stack([est.get_T_WS(f) for f in fids])

    def agree(got, want, what):
        log_(what, "iterations", got[1], want[1], "cost", got[0], want[0], "poses", float(np.max(np.abs(got[2] - want[2]))))
        assert got[1] == want[1], what
        assert abs(got[0] - want[0]) < 1e-11 * want[0], (what, got[0], want[0])
        assert np.max(np.abs(got[2] - want[2])) < 1e-9, what

    # the path: a reduced solve that eliminates the chain (the reduced system's block table, speed / bias blocks last) ...
    lin = handle()[0].linearize(1e-8)
    sizes = np.diff(np.r_[lin["block_off"], lin["d"]])
    n_sb = int((sizes == 9).sum())
    assert n_sb > 0 and (sizes[len(sizes) - n_sb:] == 9).all()
    d, dC = lin["d"], lin["d"] - 9 * n_sb
    log_("side lane window: d", d, "dC", dC, "chain", n_sb)
    assert spl.plan_one(planner, d, dC=dC, n=n_sb)["chainMode"] != 0
    runs = {}
    for off in (0, 1):
        debug_option("SVIN_NO_SB_EARLY", off)
        est, fids = handle()
        for _ in range(2):
            est.optimize(4)
        assert Estimator.debug_get_option("SVIN_LAST_SCHUR_FORM") == 2000   # ... behind the block-pair form of the build
        runs[off] = (est, fids)
    debug_option("SVIN_NO_SB_EARLY", 0)
    agree(solved(*runs[1]), solved(*runs[0]), "SVIN_NO_SB_EARLY")
    # the step hook in the form solve() chooses sets the side lane for its own build and reduced solve
    est, fids = runs[0]
    est.debug_trust_region_step(1e-8, 1e4, form=0, commit=False)
    est.optimize(4)
    fresh, ffids = handle()
    for _ in range(3):
        fresh.optimize(4)
    agree(solved(est, fids), solved(fresh, ffids), "behind the step hook")
