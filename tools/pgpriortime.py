"""Cost of absolute keyframe measurements (svin_pg_add_prior) on the config-#5 graph, both DoF.
usage: python tools/pgpriortime.py [n] [laps] [loop_every] [reps] [--out FILE.json]

Two forms of the same graph, each optimised `reps` times on a fresh handle after one warm-up run:
  bare     the graph as bench.py --workload posegraph measures it: k_pg_eval
  depth    the same graph with a DEPTH prior on every keyframe (the keyframe's own SVIn depth, information 1 / (0.05 m)^2): n more
           entries in the list, evaluated by k_pg_eval_terms, each one more incidence for k_pg_node
The priors change the problem, so the iteration counts may differ; compare per iteration.  Per form: LM iterations, device ms per
iteration (summary solve_seconds / iterations; inputs resident), host ms of the whole optimize() call.  Median (min, max) over the
reps.  No pass or fail number is attached."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svin_amd import synthetic_pg as spg  # noqa: E402
from svin_amd.posegraph import PRIOR_DEPTH, PoseGraph  # noqa: E402

argv = sys.argv[1:]
out_path = None
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
n, laps, loop_every, reps = (int(a) for a in (argv + ["5000", "20", "25", "5"][len(argv):]))
spec = spg.make_pose_graph(n=n, laps=laps, loop_every=loop_every, seed=7)
result = dict(graph=dict(keyframes=n, loops=len(spec.loops), laps=laps, loop_every=loop_every, seed=7), reps=reps, unit="ms",
              method="fresh handle per run; device ms = summary solve_seconds / iterations; median (min, max) of reps after one warm-up",
              dof={})
INFO = np.array([[1.0 / 0.05 ** 2]])


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1], runs=xs)


def run(six, form):
    per_it, wall, its = [], [], None
    for rep in range(reps + 1):
        g = PoseGraph(0, six_dof=six)
        earliest, cur = spg.feed(g, spec)
        if form == "depth":
            for k in range(spec.n):
                g.add_prior(k, PRIOR_DEPTH, spec.t_svin[k], None, 0.0, INFO)
        t0 = time.perf_counter()
        s = g.optimize(earliest, cur)
        wall.append(1e3 * (time.perf_counter() - t0))
        per_it.append(1e3 * s["solve_seconds"] / max(1, s["iterations"]))
        its = s["iterations"]
        g.close()
    return dict(iterations=its, device_ms_per_iteration=stats(per_it[1:]), optimize_call_ms=stats(wall[1:]), final_cost=s["final_cost"])


for six in (False, True):
    rec = {form: run(six, form) for form in ("bare", "depth")}
    result["dof"]["6" if six else "4"] = rec
    for form, r in rec.items():
        print("%d-DoF %-6s %2d iterations, %.3f ms / iteration (%.3f - %.3f), optimize() %.1f ms" %
              (6 if six else 4, form, r["iterations"], r["device_ms_per_iteration"]["median"], r["device_ms_per_iteration"]["min"],
               r["device_ms_per_iteration"]["max"], r["optimize_call_ms"]["median"]), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
