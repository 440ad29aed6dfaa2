"""The batched solve on windows of DIFFERENT sizes (svin_ba_solve_prepared_batch; svin_amd/csrc/batch_plan.hpp): what bench.py's
`batched` record measures on windows of one size, here on a fleet whose front ends found different numbers of landmarks.

B windows of config #2's generator (10 keyframes), L drawn from a seeded uniform [1 600, 2 400], n_obs = 10 L.  Protocol of
bench.batched_record: per step every window starts from its own initial state, is packed and uploaded untimed (inputs resident in
HBM), and the batch call is timed; aggregate = the Gauss-Newton iterations of all windows per step / that time.  Printed per B:
the aggregate rate, how many windows ran batched, the share of launched blocks that left at once (SVIN_LAST_BATCH_IDLE_PPM: the
padding a lane's grid carries for its smaller windows, plus windows sitting out a stage) and the same windows solved one after the
other.  A library without the read-only option (an older build given with SVIN_BA_LIB) reports the share as null.

    python tools/raggedtime.py [B ...] [--steps K] [--warmup W] [--equal]      (--equal: every L = 2 000, the `batched` record's case)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import bench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", type=int, nargs="*", default=[16, 32, 64])
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--equal", action="store_true")
    args = ap.parse_args()
    import torch
    from svin_amd import estimator as E
    from svin_amd import synthetic as syn
    from svin_amd.estimator import Estimator
    B_max = max(args.sizes)
    rng = np.random.default_rng(20250629)
    Ls = [2000] * B_max if args.equal else [int(x) for x in rng.integers(1600, 2401, B_max)]
    ws = []
    for k in range(B_max):
        spec = syn.make_window(L=Ls[k], n_obs=10 * Ls[k], seed=20250629 + 7 * k)
        est = Estimator(0)
        fids, lids = syn.feed(est, spec)
        ws.append((est, fids, lids, bench.snapshot_init(est, fids, lids, spec)))
    out = {"unit": "GN iterations/s", "workload": "B config #2 windows (10 KF), L %s, n_obs = 10 L, optimize(10) per step"
           % ("= 2000" if args.equal else "~ U[1600, 2400] (seed 20250629)")}

    def measure(B, solve):
        times, its, nb = [], [], 0
        for k in range(args.warmup + args.steps):
            for est, fids, lids, snap in ws[:B]:
                bench.reset_state(est, fids, lids, snap)
                est.prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nb = solve([w[0] for w in ws[:B]])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            n_it = sum(w[0].summary()["iterations"] for w in ws[:B])
            for w in ws[:B]:
                w[0].finish()
            if k >= args.warmup:
                times.append(dt)
                its.append(n_it)
        return {"aggregate": sum(its) / sum(times), "windows_batched": nb, "ms_per_step": 1e3 * sum(times) / len(times),
                "iterations_per_step": sum(its) / len(its)}

    def one_after_the_other(ests):
        for e in ests:
            e.solve_prepared(10)
        return 0

    for B in args.sizes:
        rec = measure(B, lambda ests: E.solve_prepared_batch(ests, 10))
        try:
            rec["idle_block_share"] = 1e-6 * Estimator.debug_get_option("SVIN_LAST_BATCH_IDLE_PPM")
        except KeyError:
            rec["idle_block_share"] = None
        serial = measure(B, one_after_the_other)
        rec["one_after_the_other"] = serial["aggregate"]
        rec["x_one_after_the_other"] = rec["aggregate"] / serial["aggregate"]
        rec["landmarks"] = [min(Ls[:B]), max(Ls[:B])]
        out["B%d" % B] = rec
        print(json.dumps({"B%d" % B: rec}), flush=True)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
