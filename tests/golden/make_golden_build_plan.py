#!/usr/bin/env python3
"""Golden fixture of the build's and the evaluation's launch decisions (tests/golden/build_plan.npz): for every row of the sweep of
tests/helpers/build_plan_lib.py, and for its extra rows off the grid, the SVIN_LAST_SCHUR_FORM code, the dense variant (-1: another
form), aMfma, DeviceProblem::aBlocks, the dense form's dynamic LDS bytes, useLds, nSlabs, the slab count k_reduce_slabs is told to
sum (0: not launched), whether k_eval_build takes the window on 256 / 40 compute units, whether the evaluation can be fused, and
the LDS bytes of the split evaluation's reprojection launch.

The rows were NOT produced by svin_amd/csrc/build_plan.hpp.  They were recorded from the code that took these decisions before
that header existed -- kernels.hip and pack_plan.hpp at commit 1a8e1c0 -- by a throw-away program that included that kernels.hip
and, per row, filled a DeviceProblem as pack() does from chooseSchurForm, called denseSchurPlan, schurDenseABlocks,
canFuseEvaluation, evalSplitStageBytes and evalBuildFits, and walked the conditions of launchAccumulateNormalEquations and
launchEvalBuild copied from there (it also checked that the three copies of the "a slab fits LDS" test agreed on every row).  It
wrote one row of 27 int32 per point: the 15 inputs (build_plan_lib.INPUTS), then the 12 columns of build_plan_lib.RECORDED, and
printed sizeof(CameraModel) and sizeof(FactorShared) of that commit, which the planner takes as arguments.
This script only packs such a dump, after checking that its inputs are the sweep's.  The planner is held to the fixture; a change
of a decision ON PURPOSE edits the affected rows and says so.
Run:  python tests/golden/make_golden_build_plan.py DUMP SIZEOF_CAMERA_MODEL SIZEOF_FACTOR_SHARED      (writes build_plan.npz)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import build_plan_lib as bpl  # noqa: E402


def main(dump, camera_model_bytes, factor_shared_bytes):
    n_in, n_out = len(bpl.INPUTS), len(bpl.RECORDED)
    rows = np.fromfile(dump, np.int32).reshape(-1, n_in + n_out)
    sw, extra = bpl.sweep(), bpl.extra_rows()
    assert np.array_equal(rows[:len(sw), :n_in], sw), "the dump's first rows are the sweep, in its order"
    assert np.array_equal(rows[len(sw):, :n_in], extra), "... and the extra rows behind it"
    # column-major, the narrowest type per column: a column of the sweep is long runs, which is what makes the file small
    cols = {}
    for k, name in enumerate(bpl.RECORDED):
        c = rows[:, n_in + k]
        cols[name] = c.astype(np.int8 if np.all(np.abs(c) < 128) else np.int32)
    path = os.path.join(HERE, "build_plan.npz")
    np.savez_compressed(path, sizes=np.array([camera_model_bytes, factor_shared_bytes, bpl.SMALL_CUS], np.int64), **cols)
    print("wrote %s: %d + %d rows, %d bytes" % (path, len(sw), len(extra), os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
