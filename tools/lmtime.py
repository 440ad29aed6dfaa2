"""What Levenberg-Marquardt costs next to dogleg: solve_prepared on the config-#2 window and on the frames of a sliding window, both
strategies, from the same starts.  Prints one JSON line per case: iterations, termination, final cost, solve time, time per
iteration, and the speculative builds kept / discarded (SVIN_SPEC_BUILD_HITS / _MISSES) -- per frame for the sliding window.
    python tools/lmtime.py [--iters 30] [--repeat 5] [--frames 12]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svin_amd import synthetic as syn  # noqa: E402
from svin_amd.estimator import Estimator  # noqa: E402


def counters():
    return Estimator.debug_get_option("SVIN_SPEC_BUILD_HITS"), Estimator.debug_get_option("SVIN_SPEC_BUILD_MISSES")


def timed_solve(est, iters):
    est.prepare()
    h0, m0 = counters()
    t = time.perf_counter()
    est.solve_prepared(iters)
    dt = time.perf_counter() - t
    h1, m1 = counters()
    est.finish()
    s = est.summary()
    log = est.iteration_log()
    return dict(iterations=s["iterations"], successful=s["successful"], termination=s["termination"], final_cost=s["final_cost"],
                solve_us=1e6 * dt, us_per_iteration=1e6 * dt / max(1, s["iterations"]), spec_hits=h1 - h0, spec_misses=m1 - m0,
                rejected=int((log[:, 5] == 1).sum()), invalid=int((log[:, 5] == 2).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--frames", type=int, default=12)
    a = ap.parse_args()
    spec = syn.make_window()
    for strategy in ("dogleg", "lm"):
        runs = []
        for _ in range(a.repeat + 1):     # (the first run warms the handle's buffers and the code objects up)
            est = Estimator(0)
            syn.feed(est, spec)
            est.set_trust_region(strategy)
            runs.append(timed_solve(est, a.iters))
        runs = sorted(runs[1:], key=lambda r: r["solve_us"])
        print(json.dumps(dict(case="config2", strategy=strategy, median=runs[len(runs) // 2], fastest_us=runs[0]["solve_us"])), flush=True)
    seq = syn.make_window(P=a.frames, L=600, n_obs=8000, seed=9, keyframe_every=2, frame_dt=0.3)
    for strategy in ("dogleg", "lm"):
        est = Estimator(0)
        est.set_trust_region(strategy)
        frames = []

        def on_frame(k, fid):
            if k >= 2:
                frames.append(dict(frame=k, **timed_solve(est, 10)))
            else:
                est.optimize(10)
            est.apply_marginalization(3, 2)
        syn.feed(est, seq, on_frame=on_frame)
        for f in frames:
            print(json.dumps(dict(case="sliding_window", strategy=strategy, **f)), flush=True)


if __name__ == "__main__":
    main()
