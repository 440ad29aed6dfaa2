"""Timing of caller-given pose-graph edges (svin_pg_add_edge) on the config-#5 graph, both DoF.
usage: python tools/pgedgetime.py [n] [laps] [loop_every] [reps] [--out profiles/pg_edges_time.json]

Three forms of the same graph, each optimised `reps` times on a fresh handle after one warm-up run:
  builtin        the loops handed over with their keyframes (svin_pg_add_keyframe): k_pg_eval, atomic assembly -- the form bench.py
                 --workload posegraph measures
  caller_default the loops as caller edges, information NULL + Huber(0.1): the same numbers through k_pg_eval_edges
  caller_dense   the loops as caller edges with a dense information matrix (the loop weights squared, rotated by a fixed
                 orthogonal matrix) + Cauchy(1): a different problem, so iterations may differ; compare per iteration
Per form: LM iterations, device ms per iteration (summary solve_seconds / iterations; inputs resident), host ms of the whole
optimize() call.  Median (min, max) over the reps.  No pass or fail number is attached."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svin_amd import synthetic_pg as spg  # noqa: E402
from svin_amd.posegraph import LOSS_CAUCHY, LOSS_HUBER, PoseGraph  # noqa: E402

argv = sys.argv[1:]
out_path = None
if "--out" in argv:
    i = argv.index("--out")
    out_path = argv[i + 1]
    del argv[i:i + 2]
n, laps, loop_every, reps = (int(a) for a in (argv + ["5000", "20", "25", "5"][len(argv):]))
spec = spg.make_pose_graph(n=n, laps=laps, loop_every=loop_every, seed=7)
bare = spg.PoseGraphSpec(spec.n, spec.t_true, spec.R_true, spec.t_svin, spec.q_svin, {}, spec.sequence)
result = dict(graph=dict(keyframes=n, loops=len(spec.loops), laps=laps, loop_every=loop_every, seed=7), reps=reps, unit="ms",
              method="fresh handle per run; device ms = summary solve_seconds / iterations; median (min, max) of reps after one warm-up",
              dof={})


def dense_information(six):
    D = 6 if six else 4
    w = np.array([20.0, 20, 20, 100, 100, 100] if six else [1.0, 1, 1, 0.1]) ** 2
    Q, _ = np.linalg.qr(np.random.default_rng(5).normal(size=(D, D)))
    A = (Q * w) @ Q.T
    return (A + A.T) / 2


def stats(xs):
    xs = sorted(xs)
    return dict(median=xs[len(xs) // 2], min=xs[0], max=xs[-1])


def run(six, form):
    per_it, wall, its = [], [], None
    for rep in range(reps + 1):
        g = PoseGraph(0, six_dof=six)
        if form == "builtin":
            earliest, cur = spg.feed(g, spec)
        else:
            spg.feed(g, bare)
            earliest, cur = min(v[0] for v in spec.loops.values()), spec.n - 1
            info = dense_information(six) if form == "caller_dense" else None
            for k, (old, rt, rq, ry) in sorted(spec.loops.items()):
                if form == "caller_dense":
                    g.add_edge(old, k, rt, rq, ry, info, LOSS_CAUCHY, 1.0)
                else:
                    g.add_edge(old, k, rt, rq, ry, None, LOSS_HUBER, 0.1)
        t0 = time.perf_counter()
        s = g.optimize(earliest, cur)
        wall.append(1e3 * (time.perf_counter() - t0))
        per_it.append(1e3 * s["solve_seconds"] / max(1, s["iterations"]))
        its = s["iterations"]
        g.close()
    return dict(iterations=its, device_ms_per_iteration=stats(per_it[1:]), optimize_call_ms=stats(wall[1:]),
                final_cost=s["final_cost"])


for six in (False, True):
    rec = {form: run(six, form) for form in ("builtin", "caller_default", "caller_dense")}
    result["dof"]["6" if six else "4"] = rec
    for form, r in rec.items():
        print("%d-DoF %-14s %2d iterations, %.3f ms / iteration (%.3f - %.3f), optimize() %.1f ms" %
              (6 if six else 4, form, r["iterations"], r["device_ms_per_iteration"]["median"], r["device_ms_per_iteration"]["min"],
               r["device_ms_per_iteration"]["max"], r["optimize_call_ms"]["median"]), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
