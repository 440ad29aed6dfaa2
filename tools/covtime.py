"""Time of the marginal-covariance query (svin_ba_get_covariance) beside the solve it would run next to, on the config-#2 window
(10 keyframes / 2 000 landmarks / 20 000 residuals, d = 150) and on the stereo_rig_v2 window (ten frames with per-frame
extrinsics, d = 258): the all-blocks pass (the first call after a change: build with mu = 0, factor, inverse, refinement, landmark
pass, read-back), a look-up of a kept camera-side block, a landmark-pose pair computed on request from the kept Sigma_cc, and on
the same window the getLhs pass and optimize(10).

Every timed call ends in a synchronise of the handle's stream inside the library, so the host clock around it is the time of the
device work plus its enqueueing; each figure is the median of `--repeat` calls behind a warm-up call.  Landmarks seen fewer than
three times are left out (their block has no inverse without damping, and the call would say SINGULAR).
Prints one JSON line; `--out FILE` also writes it there."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svin_amd import synthetic as syn  # noqa: E402
from svin_amd.estimator import Estimator, SingularError  # noqa: E402


def well_observed(spec):
    cnt = np.bincount(spec.obs_lm, minlength=spec.L)
    keep = cnt[spec.obs_lm] >= 3
    for name in ("obs_lm", "obs_frame", "obs_cam", "obs_uv", "obs_size"):
        setattr(spec, name, getattr(spec, name)[keep])
    return spec


def median_ms(fn, repeat, before=None):
    fn() if before is None else (before(), fn())   # warm-up
    out = []
    for _ in range(repeat):
        if before is not None:
            before()
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)


def one_window(name, spec, repeat):
    est = Estimator(0)
    frames, _ = syn.feed(est, spec)
    est.optimize(10)
    newest = frames[-1]
    lm = next(l for l in est.landmark_ids() if len(est.landmark_observations(l)) >= 3)
    d = est.linearize(0.0)["d"]

    def touch():   # any setter drops what the handle keeps
        est.set_T_WS(newest, est.get_T_WS(newest))
    n0 = est.covariance_pass_count()
    t_pass = median_ms(lambda: est.get_covariance(newest, newest), repeat, touch)
    assert est.covariance_pass_count() == n0 + repeat + 1
    est.get_covariance(newest, newest)
    t_look = median_ms(lambda: est.get_covariance(newest, frames[0]), repeat)
    t_pair = median_ms(lambda: est.get_covariance(lm, newest), repeat)
    t_lmdiag = median_ms(lambda: est.get_covariance(lm, lm), repeat)
    assert est.covariance_pass_count() == n0 + repeat + 1   # look-ups and pairs ran no pass
    t_lin = median_ms(lambda: est.linearize(0.0), repeat)
    t_lhs = median_ms(lambda: est.get_lhs(newest), repeat, touch)
    # optimize(10) from the seeded start on fresh handles (the solve a frame runs)
    t_opt = []
    for _ in range(max(3, repeat // 4)):
        e2 = Estimator(0)
        syn.feed(e2, spec)
        t0 = time.perf_counter()
        e2.optimize(10)
        t_opt.append(1e3 * (time.perf_counter() - t0))
    sd = np.sqrt(np.diag(est.get_covariance(newest, newest)))
    return dict(window=name, d=int(d), landmarks=len(est.landmark_ids()), repeat=repeat,
                covariance_all_blocks_pass_ms=dict(zip(("median", "min", "max"), t_pass)),
                linearize_mu0_ms=dict(zip(("median", "min", "max"), t_lin)),
                covariance_lookup_camera_block_ms=dict(zip(("median", "min", "max"), t_look)),
                covariance_landmark_pose_pair_ms=dict(zip(("median", "min", "max"), t_pair)),
                covariance_lookup_landmark_block_ms=dict(zip(("median", "min", "max"), t_lmdiag)),
                get_lhs_pass_ms=dict(zip(("median", "min", "max"), t_lhs)),
                optimize10_ms=dict(median=round(statistics.median(t_opt), 4), min=round(min(t_opt), 4), max=round(max(t_opt), 4)),
                newest_pose_sigma=[float("%.3e" % v) for v in sd])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    def guarded(name, spec):
        try:
            return one_window(name, spec, a.repeat)
        except SingularError as e:   # a numerical answer of this window, not a failure of the tool
            return dict(window=name, singular=str(e))
    res = [guarded("config #2: 10 KF / 2 000 landmarks / 20 000 residuals", well_observed(syn.make_window())),
           guarded("stereo_rig_v2: 10 frames, per-frame extrinsics / 600 landmarks / 6 000 residuals",
                      well_observed(syn.make_window(P=10, L=600, n_obs=6000, seed=11, rig="rig_v2", frame_dt=0.25)))]
    line = json.dumps(dict(tool="covtime", clock="host clock around calls that end in a stream synchronise; median of repeats", windows=res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
