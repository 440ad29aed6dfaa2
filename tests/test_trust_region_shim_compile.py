"""The trust-region options of the public interface without a GPU: tests/csrc/shim_trust_region.cpp (okvis::ceres::Map with
options.trust_region_strategy_type = LEVENBERG_MARQUARDT and the two radii) builds with every warning an error against
integration/okvis/ceres/Map.hpp and links against the library, the library exports the three C entry points, the header declares
them, and the Python mirror binds them."""
import ctypes as C
import os
import subprocess

from test_shim_compile import INC, ROOT, _compile


def test_shim_trust_region_program_builds_and_links(tmp_path):
    src = os.path.join(ROOT, "tests", "csrc", "shim_trust_region.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror"] + INC + [src])
    assert os.path.exists(_compile(tmp_path, "shim_trust_region"))


def test_trust_region_entry_points_are_exported_and_declared():
    from svin_amd import estimator
    lib = C.CDLL(estimator.library_path())
    for name in ("svin_ba_set_trust_region", "svin_ba_get_trust_region", "svin_ba_get_iteration_log"):
        assert hasattr(lib, name) and name in estimator.EXPORTS
    with open(os.path.join(ROOT, "include", "svin_ba.h")) as f:
        hdr = f.read()
    assert "int svin_ba_set_trust_region(svin_ba* h, int strategy, double initial_radius, double max_radius);" in hdr
    assert "int svin_ba_get_trust_region(svin_ba* h, int* strategy, double* initial_radius, double* max_radius);" in hdr
    assert "int svin_ba_get_iteration_log(svin_ba* h, int cap_rows, double* out, int* n_rows);" in hdr
    assert "#define SVIN_STRATEGY_DOGLEG 0" in hdr and "#define SVIN_STRATEGY_LEVENBERG_MARQUARDT 1" in hdr
    assert estimator.Estimator.STRATEGIES == {"dogleg": 0, "lm": 1}
    for method in ("set_trust_region", "get_trust_region", "iteration_log"):
        assert callable(getattr(estimator.Estimator, method))
    # the two speculation counters are names svin_ba_debug_get_option knows (process-wide, read-only; no GPU is touched)
    v = C.c_int32(-1)
    lib.svin_ba_debug_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int32)]
    for name in (b"SVIN_SPEC_BUILD_HITS", b"SVIN_SPEC_BUILD_MISSES"):
        assert lib.svin_ba_debug_get_option(name, C.byref(v)) == 1 and v.value >= 0


def test_the_shim_keeps_dogleg_as_its_default_and_the_estimator_sets_it():
    with open(os.path.join(ROOT, "integration", "okvis", "ceres", "Map.hpp")) as f:
        hdr = f.read()
    assert "::ceres::TrustRegionStrategyType trust_region_strategy_type = ::ceres::DOGLEG;" in hdr
    assert "double initial_trust_region_radius = 1e4, max_trust_region_radius = 1e16;" in hdr
    with open(os.path.join(ROOT, "integration", "okvis", "Estimator.hpp")) as f:
        assert "options.trust_region_strategy_type = ::ceres::DOGLEG;" in f.read()
