"""The host planning of the marginal-covariance pass (svin_amd/csrc/cov_plan.hpp through tests/csrc/cov_plan_shim.cpp) on the CPU:
at d = 6, 16, 45, 150, 198, 270, 272 the regions of the window's covariance buffer do not overlap and hold what the kernels index,
every launch stays within a workgroup's 160 KiB of LDS and 1024 threads, and d = 273 is refused."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIONS = ("scaled", "factor", "linv", "scale", "xs", "sigma", "lmCov", "flags")
LAUNCHES = ("factorize", "inverse", "refine", "landmarks", "pairs")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("covplan")), "libcp.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "csrc", "cov_plan_shim.cpp"), "-o", so])
    L = C.CDLL(so)
    L.cp_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.cp_plan.restype = None
    L.cp_constant.restype = C.c_int64
    return L


def plan(lib, d, dC, L, n_pairs=7):
    out = np.zeros(lib.cp_fields(), np.int64)
    lib.cp_plan(d, dC, L, n_pairs, out.ctypes.data_as(C.c_void_p))
    q = dict(supported=bool(out[0]), nT=int(out[1]), dpad=int(out[2]), end=int(out[19]))
    for k, name in enumerate(REGIONS):
        q[name] = (int(out[3 + 2 * k]), int(out[4 + 2 * k]))
    for k, name in enumerate(LAUNCHES):
        q[name] = tuple(int(v) for v in out[20 + 3 * k:23 + 3 * k])
    return q


@pytest.mark.parametrize("d,dC,L", [(6, 6, 0), (16, 6, 1), (45, 18, 12), (150, 60, 2000), (198, 144, 300), (270, 180, 600),
                                    (272, 272, 65), (0, 0, 5)])
def test_regions_and_launches(lib, d, dC, L):
    q = plan(lib, d, dC, L)
    assert q["supported"] and q["nT"] == (d + 15) // 16 and q["dpad"] == 16 * q["nT"]
    dp = q["dpad"]
    want = dict(scaled=dp * dp, factor=dp * dp, linv=256 * q["nT"], scale=dp, xs=dp * dp, sigma=d * d, lmCov=9 * L, flags=2)
    spans = []
    for name in REGIONS:
        off, ln = q[name]
        assert ln == want[name], name
        assert off % 2 == 0, name   # 16-byte aligned starts
        spans.append((off, off + ln, name))
    spans.sort()
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, (an, bn)
    assert spans[-1][1] <= q["end"]
    max_lds = lib.cp_constant(1)
    assert max_lds == 160 * 1024
    for name in LAUNCHES:
        grid, threads, lds = q[name]
        assert lds <= max_lds and threads % 64 == 0 and 64 <= threads <= 1024, name
    assert q["factorize"][0] == (1 if d > 0 else 0)
    assert q["inverse"][0] == q["refine"][0] == q["nT"]
    per = lib.cp_constant(3)
    assert q["landmarks"][0] == (L + per - 1) // per and q["pairs"][0] == 7
    # what the kernels index: the block column / the panel in 16 x 17 tiles, the residual panel, a landmark's W image
    assert q["factorize"][2] >= 8 * (q["nT"] * 272 + 272 + 16 + dp) + 4
    assert q["inverse"][2] == 8 * q["nT"] * 272 and q["refine"][2] == 8 * dp * 16
    assert q["landmarks"][2] == 8 * per * 3 * max(dC, 1) and q["pairs"][2] == 8 * 2 * 3 * max(dC, 1)


def test_refusals(lib):
    assert lib.cp_constant(0) == 272
    assert not plan(lib, 273, 180, 10)["supported"]
    assert not plan(lib, 285, 285, 10)["supported"]
    assert not plan(lib, 100, 101, 10)["supported"]   # more camera-side rows than unknowns
    assert plan(lib, 272, 0, 0)["supported"]
