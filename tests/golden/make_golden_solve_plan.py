#!/usr/bin/env python3
"""Golden fixture of the reduced solve's routing (tests/golden/solve_plan.npz): for every row of the sweep of
tests/helpers/solve_plan_lib.py, and for a few rows with d != dC + 9 n, the chain mode, the dense route of the system actually
solved, its border rows, the blocked solver's dp and the offsets of Lf, Y, tvec, S' and g' in DeviceProblem::cholL (-1: not used).

The rows were NOT produced by svin_amd/csrc/solve_plan.hpp.  They were recorded from the functions that decided the routes before
that header existed (solverClass, cholBorderRows and planSbElimination of kernels.hip at commit c527f06) by a throw-away program
that included that kernels.hip, called them with each switch set and wrote one row of 14 int32 per point:
    d, dC, sbChain, sPadded, switches, chain mode, route, border, dp, Lf, Y, tvec, S', g'
This script only packs such a dump, after checking that its inputs are the sweep's.  The planner is held to the fixture; a change
of a route ON PURPOSE edits the affected rows and says so.
Run:  python tests/golden/make_golden_solve_plan.py DUMP      (writes solve_plan.npz)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import solve_plan_lib as spl  # noqa: E402


def main(dump):
    rows = np.fromfile(dump, np.int32).reshape(-1, 14)
    sw = spl.sweep()
    assert np.array_equal(rows[:len(sw), :5], sw), "the dump's first rows are the sweep, in its order"
    extra = rows[len(sw):]
    assert np.any(extra[:, 0] != extra[:, 1] + 9 * extra[:, 2])
    # column-major: a column of the sweep is long runs and ramps, which is what makes the file small
    out = dict(sweep_out=np.ascontiguousarray(rows[:len(sw), 5:].T), extra_in=extra[:, :5].copy(), extra_out=extra[:, 5:].copy())
    path = os.path.join(HERE, "solve_plan.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d + %d rows, %d bytes" % (path, len(sw), len(extra), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
