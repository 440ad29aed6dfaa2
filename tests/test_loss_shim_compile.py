"""Loss functions in the C++ shim without a GPU: tests/csrc/shim_loss.cpp (reprojection residuals under NULL, HuberLoss and
CauchyLoss, a PoseError under HuberLoss, an unsupported loss object) builds with every warning an error against
integration/okvis/ceres/Map.hpp and CeresTypes.hpp, and the library exports the two C entry points the Python mirror binds."""
import ctypes as C
import os

from test_shim_compile import ROOT, _compile


def test_shim_loss_program_builds(tmp_path):
    assert os.path.exists(_compile(tmp_path, "shim_loss"))


def test_loss_entry_points_are_exported_and_declared():
    from svin_amd import estimator
    lib = C.CDLL(estimator.library_path())
    for name in ("svin_ba_map_set_residual_loss", "svin_ba_map_get_residual_loss"):
        assert hasattr(lib, name) and name in estimator.EXPORTS
    with open(os.path.join(ROOT, "include", "svin_ba.h")) as f:
        hdr = f.read()
    assert "int svin_ba_map_set_residual_loss(svin_ba* h, uint64_t residual_id, int kind, double scale);" in hdr
    assert "int svin_ba_map_get_residual_loss(svin_ba* h, uint64_t residual_id, int* kind, double* scale);" in hdr
    assert (estimator.SVIN_LOSS_NONE, estimator.SVIN_LOSS_CAUCHY, estimator.SVIN_LOSS_HUBER) == (0, 1, 2)
    for k, v in (("NONE", 0), ("CAUCHY", 1), ("HUBER", 2)):
        assert "#define SVIN_LOSS_%s %d" % (k, v) in hdr
