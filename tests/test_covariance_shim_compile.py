"""Marginal covariances in the C++ shim without a GPU: tests/csrc/shim_covariance.cpp (Map::getCovarianceBlock of
integration/okvis/ceres/Map.hpp with a matrix type of its own) builds with every warning an error against the shim and the
stand-in headers, and the library exports the three C entry points the Python mirror binds."""
import ctypes as C
import os

from test_shim_compile import ROOT, _compile


def test_shim_covariance_program_builds(tmp_path):
    assert os.path.exists(_compile(tmp_path, "shim_covariance"))


def test_covariance_entry_points_are_exported_and_declared():
    from svin_amd import estimator
    lib = C.CDLL(estimator.library_path())
    for name in ("svin_ba_get_covariance", "svin_ba_get_covariance_blocks", "svin_ba_get_covariance_pass_count"):
        assert hasattr(lib, name) and name in estimator.EXPORTS
    with open(os.path.join(ROOT, "include", "svin_ba.h")) as f:
        hdr = f.read()
    assert "#define SVIN_ERR_SINGULAR (-5)" in hdr and estimator.SVIN_ERR_SINGULAR == -5
    assert "int svin_ba_get_covariance(svin_ba* h, uint64_t block_a, uint64_t block_b, double* cov, int cap);" in hdr
    assert ("int64_t svin_ba_get_covariance_blocks(svin_ba* h, int n_pairs, const uint64_t* blocks_a, const uint64_t* blocks_b,\n"
            "                                      int32_t* dims_a, int32_t* dims_b, double* cov, int64_t cap_doubles);") in hdr
    assert "int64_t svin_ba_get_covariance_pass_count(svin_ba* h);" in hdr
    for method in ("get_covariance", "get_covariance_blocks", "covariance_pass_count"):
        assert callable(getattr(estimator.Estimator, method))
    with open(os.path.join(ROOT, "integration", "okvis", "ceres", "Map.hpp")) as f:
        assert "bool getCovarianceBlock(uint64_t parameterBlockIdA, uint64_t parameterBlockIdB, MatrixT& cov) const" in f.read()
