#!/usr/bin/env python3
"""Golden fixture of the host planning of Window::pack (tests/golden/pack_plan.npz): for inputs A and C of
tests/test_pack_plan_host.py (tests/helpers/pack_plan_lib.py) the inputs themselves and every array the planner hands the
device -- the slots, the work list of k_schur_rows (256 compute units, row split on), the older work list of k_schur_panels and
the per-chunk observation order -- as svin_amd/csrc/pack_plan.hpp builds them today.

The fixture pins the bytes: a change that alters a work list ON PURPOSE re-records it and says so.
Run:  python tests/golden/make_golden_pack_plan.py      (writes pack_plan.npz; a few seconds)
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import pack_plan_lib as ppl  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib = ppl.build_shim(tmp)
        for name, inp in (("A", ppl.input_a()), ("C", ppl.input_c())):
            arrays = dict(lmPtr=inp.lmPtr, obsIdx=inp.obsIdx, poseOff=inp.poseOff, dC=np.int32(inp.dC))
            arrays.update(ppl.slots(lib, inp))
            arrays.update(ppl.rows(lib, inp, 256, True))
            arrays.update({"old_" + k: v for k, v in ppl.panels(lib, inp).items()})
            arrays["obsOrder"] = ppl.chunk_order(lib, inp)
            out.update({name + "_" + k: v for k, v in arrays.items()})
    path = os.path.join(HERE, "pack_plan.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
