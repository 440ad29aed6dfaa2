"""Timing of the pose graph's marginal covariances (svin_pg_get_covariance_blocks) on the config-#5 graph, both DoF.
usage: python tools/pgcovtime.py [n] [laps] [loop_every] [reps] [--out profiles/pg_covtime.json]

Per DoF, on one handle after one optimisation (so that the covariance is taken at the optimised poses, as a caller would):
  lm_iteration_ms     device time of one Levenberg-Marquardt iteration of that optimisation (summary: solve seconds / iterations)
  first_query_ms      a query on a handle without a kept factor: construction, symbolic step, upload, evaluation, node pass,
                      undamped assembly, factorisation, one substitution pass (host clock around the synchronous call)
  repeated_query_ms   the same query again with the factor kept: one substitution pass
  columns_1 / 8 / 64  diagonal blocks of the last 1 / 8 / 64 keyframes with the factor kept: 1 / 1 / 8 substitution passes
Every figure is the median of `reps` runs after one warm-up run of the same shape; the spread (min, max) is recorded next to it.
No pass or fail number is attached: the expectation to read the figures against is that a first query costs about one solve of
the normal equations plus the host work of an optimize() call, and a repeated one only the substitutions."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svin_amd import synthetic_pg as spg  # noqa: E402
from svin_amd.posegraph import PoseGraph  # noqa: E402

argv = sys.argv[1:]
out_path = None
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
n, laps, loop_every, reps = (int(a) for a in (argv + ["5000", "20", "25", "9"][len(argv):]))
spec = spg.make_pose_graph(n=n, laps=laps, loop_every=loop_every, seed=7)
result = dict(graph=dict(keyframes=n, loops=len(spec.loops), laps=laps, loop_every=loop_every, seed=7), reps=reps, unit="ms",
              method="host clock around the synchronous C call; median (min, max) of reps after one warm-up", dof={})


def stats(xs):
    xs = sorted(1e3 * x for x in xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])


for six in (False, True):
    g = PoseGraph(0, six_dof=six)
    earliest, cur = spg.feed(g, spec)
    s = g.optimize(earliest, cur)
    part = g.partition()

    def timed(pairs, fresh):
        ts = []
        for rep in range(reps + 1):
            if fresh:
                g.set_levels(2, 0)      # drops the kept factor and changes nothing else
            c0 = g.covariance_counters()
            t0 = time.perf_counter()
            g.covariance_blocks(earliest, cur, pairs)
            ts.append(time.perf_counter() - t0)
            c1 = g.covariance_counters()
            assert c1["factorisations"] - c0["factorisations"] == (1 if fresh else 0)
        return stats(ts[1:]), c1["passes"] - c0["passes"]
    one = [(cur, cur)]
    rec = dict(optimize=dict(iterations=s["iterations"], device_ms=1e3 * s["solve_seconds"],
                             lm_iteration_ms=1e3 * s["solve_seconds"] / max(1, s["iterations"])),
               partition=dict(free=part["free"], pieces=part["pieces"], level2_pieces=part["level2_pieces"], root_unknowns=part["separator_unknowns"]))
    rec["first_query_ms"], _ = timed(one, True)
    rec["repeated_query_ms"], _ = timed(one, False)
    for k in (1, 8, 64):
        st, passes = timed([(cur - i, cur - i) for i in range(k)], False)
        rec["columns_%d_ms" % k] = dict(st, passes=passes)
    blk = g.covariance(earliest, cur, cur, cur)
    rec["sigma_last_diag"] = [float(v) for v in np.diag(blk)]
    result["dof"]["6" if six else "4"] = rec
    print("%s: LM iteration %.3f ms (device), first query %.3f ms, repeated %.3f ms, 1 / 8 / 64 column keyframes %.3f / %.3f / %.3f ms" %
          ("6dof" if six else "4dof", rec["optimize"]["lm_iteration_ms"], rec["first_query_ms"]["median"], rec["repeated_query_ms"]["median"],
           rec["columns_1_ms"]["median"], rec["columns_8_ms"]["median"], rec["columns_64_ms"]["median"]), flush=True)
    g.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
