"""What a window with general 2x2 information matrices costs: config #2 (bench.py's window and seed) timed the way bench.py times
its headline -- prepare() untimed, solve_prepared(10) between two device synchronisations, 20 timed steps after the warm-up --
once with every observation carrying 64 / size^2 * I (the one-weight form: obsS null) and once with every observation carrying a
general matrix of the same scale (obsS set: three more doubles read per residual by the evaluation kernel, nothing elsewhere).
The two windows solve different problems, so the iteration counts are reported and the ratio is taken per iteration as well.
No bar; prints one JSON line."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from svin_amd import synthetic as syn  # noqa: E402
from svin_amd.estimator import Estimator  # noqa: E402


def general_information(rng, scale):
    """symmetric positive definite, eigenvalues scale x [1, up to 4], rotated"""
    l0, l1 = scale, scale * rng.uniform(1.5, 4.0)
    a = rng.uniform(0.0, np.pi)
    c, s = np.cos(a), np.sin(a)
    off = c * s * (l0 - l1)
    return np.array([[c * c * l0 + s * s * l1, off], [off, s * s * l0 + c * c * l1]])


def run(general, steps, warmup):
    import torch
    spec = syn.make_window(seed=20250629)
    est = Estimator(0)
    fids, lids = syn.feed(est, spec)
    rids = [int(r) for r in est.eval_reprojection()["res_id"]]
    rng = np.random.default_rng(1)
    for rid in rids:
        w2 = est.map_get_reprojection_information(rid)
        est.map_set_reprojection_information(rid, general_information(rng, w2[0, 0]) if general else w2)
    snap = bench.snapshot_init(est, fids, lids, spec)
    times, its, last = bench.timed_solves(est, fids, lids, snap, steps, warmup, 10, torch.cuda.synchronize)
    pc = est.path_counters()
    return dict(median_ms=1e3 * statistics.median(times), iterations=statistics.median(its),
                ms_per_iteration=1e3 * statistics.median(t / max(1, i) for t, i in zip(times, its)),
                host_pack_solves=int(pc["host_pack_solves"]), resident_solves=int(pc["resident_solves"]), residuals=len(rids))


def main():
    steps, warmup = 20, 5
    iso, gen = run(False, steps, warmup), run(True, steps, warmup)
    print(json.dumps(dict(workload="config #2 window, solve_prepared(10), %d timed steps" % steps, isotropic=iso, general=gen,
                          ratio_per_solve=round(gen["median_ms"] / iso["median_ms"], 4),
                          ratio_per_iteration=round(gen["ms_per_iteration"] / iso["ms_per_iteration"], 4),
                          k1_traffic_model="191.2 B + 24 B per residual in the evaluation kernel, nothing elsewhere")))


if __name__ == "__main__":
    main()
