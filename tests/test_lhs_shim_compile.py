"""Map::getLhs in the C++ shim without a GPU: tests/csrc/shim_lhs.cpp (the reference's landmark loop, Estimator.cpp:902-923,
through integration/okvis/ceres/Map.hpp with a matrix type of its own) builds with every warning an error against the shim and
the stand-in headers, and the library exports the two C entry points the Python mirror binds."""
import ctypes as C
import os

from test_shim_compile import ROOT, _compile


def test_shim_getlhs_program_builds(tmp_path):
    assert os.path.exists(_compile(tmp_path, "shim_lhs"))


def test_getlhs_entry_points_are_exported_and_declared():
    from svin_amd import estimator
    lib = C.CDLL(estimator.library_path())
    for name in ("svin_ba_get_lhs", "svin_ba_get_lhs_blocks"):
        assert hasattr(lib, name) and name in estimator.EXPORTS
    with open(os.path.join(ROOT, "include", "svin_ba.h")) as f:
        hdr = f.read()
    assert "int svin_ba_get_lhs(svin_ba* h, uint64_t block_id, double* H, int cap);" in hdr
    assert "int64_t svin_ba_get_lhs_blocks(svin_ba* h, int n, const uint64_t* block_ids, int32_t* dims, double* H, int64_t cap_doubles);" in hdr
