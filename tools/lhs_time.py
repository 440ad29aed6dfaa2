"""Map::getLhs on a config-#4-size window (64 keyframes / 50 000 landmarks / 500 000 residuals, bench.py's seed): one all-blocks
pass through svin_ba_get_lhs_blocks (run under `rocprofv3 --kernel-trace --stats -- python tools/lhs_time.py` for the kernel table
in profiles/), the first svin_ba_get_lhs after a change (one pass), then the wall time of 50 000 cached svin_ba_get_lhs calls alone
and with the parameter-block read of the reference's per-landmark loop (Estimator.cpp:902-923); no extra pass allowed.
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svin_amd import synthetic as syn  # noqa: E402
from svin_amd.estimator import Estimator  # noqa: E402


def main():
    spec = syn.make_window(P=64, L=50000, n_obs=500000, seed=20250629, frame_dt=0.25)
    est = Estimator(0)
    frames, lms = syn.feed(est, spec)
    ids = [int(b) for b in est.parameter_block_ids()]
    est.get_lhs_blocks(ids)                      # warm-up: code objects, buffers, the window's first pack
    est.set_T_WS(frames[-1], est.get_T_WS(frames[-1]))   # any call drops the cached result
    t0 = time.perf_counter()
    est.get_lhs_blocks(ids)                      # the profiled pass
    t_pass = time.perf_counter() - t0
    lm_ids = est.landmark_ids()
    import ctypes as C
    H = np.zeros(9)
    ptr = H.ctypes.data_as(C.POINTER(C.c_double))
    L, h = est.L, est.h
    est.set_T_WS(frames[-1], est.get_T_WS(frames[-1]))   # drops the kept result ...
    t0 = time.perf_counter()
    if L.svin_ba_get_lhs(h, lm_ids[0], ptr, 9) != 3:     # ... and the first call runs the pass again
        raise RuntimeError("get_lhs failed")
    t_first = time.perf_counter() - t0
    passes = est.lhs_pass_count()
    t0 = time.perf_counter()
    for lid in lm_ids:                           # the reference's landmark loop: look-ups of the kept result
        if L.svin_ba_get_lhs(h, lid, ptr, 9) != 3:
            raise RuntimeError("get_lhs failed")
    t_loop = time.perf_counter() - t0
    x = np.zeros(9)
    xp = x.ctypes.data_as(C.POINTER(C.c_double))
    t0 = time.perf_counter()
    for lid in lm_ids:                           # with parameterBlockPtr's read right after each getLhs, as Estimator.cpp:902-923
        if L.svin_ba_get_lhs(h, lid, ptr, 9) != 3 or L.svin_ba_get_parameter_block(h, lid, None, xp, None, None, None, None) < 0:
            raise RuntimeError("get_lhs / get_parameter_block failed")
    t_loop2 = time.perf_counter() - t0
    if est.lhs_pass_count() != passes:
        raise RuntimeError("the loops ran %d extra passes" % (est.lhs_pass_count() - passes))
    print(json.dumps(dict(workload="config #4 window: 64 KF / 50 000 landmarks / 500 000 residuals", blocks=len(ids),
                          all_blocks_pass_ms=round(1e3 * t_pass, 3), first_call_after_a_change_ms=round(1e3 * t_first, 3),
                          cached_calls=len(lm_ids), cached_loop_ms=round(1e3 * t_loop, 3),
                          per_cached_call_us=round(1e6 * t_loop / max(1, len(lm_ids)), 3),
                          loop_with_parameter_block_ms=round(1e3 * t_loop2, 3), extra_passes=0)))

if __name__ == "__main__":
    main()
