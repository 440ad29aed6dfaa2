"""What a window anchored to a map costs per optimize(): bench.py's sliding_window protocol (its window and seed, fed frame by
frame, optimize(10) per frame) with 30 % of the landmarks held constant from the first frame on.  Only the optimize() calls are
timed and nothing is marginalised, so that the same frames can be run by a library that cannot marginalise such a window
(SVIN_BA_LIB selects the library: one process per library); the window therefore stops at ten frames, the size the protocol's
(5 keyframes, 3 IMU frames) window has, and frames 5-10 of three passes are what is timed.  --pack-mode 1 forces the host pack + full upload; the default is the
device-resident window wherever the library allows it (svin_ba_get_path_counters says which path the solves took).
No bar; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svin_amd import synthetic as syn  # noqa: E402
from svin_amd.estimator import Estimator, library_path  # noqa: E402


def run(pack_mode, share, frames):
    spec = syn.make_window(P=frames, L=2400, n_obs=24000 * frames // 24, seed=7, rig="euroc", keyframe_every=2, frame_dt=0.25)
    est = Estimator(0)
    est.set_pack_mode(pack_mode)
    rng = np.random.default_rng(3)
    rows, held = [], []

    def on_frame(k, fid):
        if k == 0:
            ids = est.landmark_ids()
            held.extend(int(i) for i in rng.choice(ids, size=int(share * len(ids)), replace=False))
            for lid in held:
                assert est.set_parameter_block_constant(lid, True)
        t0 = time.perf_counter()
        est.optimize(10)
        t1 = time.perf_counter()
        s = est.summary()
        rows.append(dict(optimize=t1 - t0, iterations=s["iterations"], upload=s.get("upload_time", 0.0), solve=s.get("solve_time", 0.0)))
    syn.feed(est, spec, on_frame=on_frame)
    return rows[4:], len(held), est.path_counters()


def summary(pack_mode, rows, held, pc):
    med = lambda key: float(statistics.median(r[key] for r in rows))   # noqa: E731
    return dict(library=os.path.relpath(library_path(), ROOT), pack_mode=pack_mode, constant_landmarks=held, timed_frames=len(rows),
                optimize_call_ms=1e3 * med("optimize"), pack_upload_ms=1e3 * med("upload"), device_solve_ms=1e3 * med("solve"),
                iterations=med("iterations"), resident_solves=int(pc["resident_solves"]), host_pack_solves=int(pc["host_pack_solves"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pack-mode", type=int, default=0)
    ap.add_argument("--share", type=float, default=0.3)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    run(args.pack_mode, args.share, args.frames)          # warm-up pass (allocations, code objects)
    rows = []
    for _ in range(args.passes):
        r, held, pc = run(args.pack_mode, args.share, args.frames)
        rows += r
    print(json.dumps(summary(args.pack_mode, rows, held, pc)))


if __name__ == "__main__":
    main()
