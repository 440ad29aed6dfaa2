// Test-only shim: the square-root information helper and the general form of the reprojection residual from the product's
// device math header (svin_amd/csrc/dmath.hpp), compiled for the HOST.  Not part of the product.
#include "../../svin_amd/csrc/dmath.hpp"
using namespace svin;
namespace {
CameraModel cameraOf(const double* cam12, int model) {
  CameraModel c;
  c.fu = cam12[0]; c.fv = cam12[1]; c.cu = cam12[2]; c.cv = cam12[3];
  for (int i = 0; i < 8; ++i) c.k[i] = cam12[4 + i];
  c.model = model; c.width = 0; c.height = 0; c.pad = 0; c.pad2 = 0;
  return c;
}
}  // namespace
extern "C" {
// S = (s00, s01, s11); 1 when the matrix is finite and positive definite (lower triangle read), else 0
int ri_sqrt_information(const double* info4, double* S3) { return reprojSqrtInformation(info4, S3) ? 1 : 0; }
// the same with the symmetry demand of the C ABI
int ri_information_valid(const double* info4, double* S3) { return reprojInformationValid(info4, S3) ? 1 : 0; }
void ri_reproj_general(const double* cam12, int model, const double* T_WS, const double* hp, const double* T_SC, double u, double v,
                       const double* S3, double* r, double* Jp, double* Jl, double* Je) {
  const CameraModel c = cameraOf(cam12, model);
  reprojEval(c, T_WS, hp, T_SC, u, v, S3[0], S3[1], S3[2], r, Jp, Jl, Je);
}
void ri_reproj_scalar(const double* cam12, int model, const double* T_WS, const double* hp, const double* T_SC, double u, double v,
                      double w, double* r, double* Jp, double* Jl, double* Je) {
  const CameraModel c = cameraOf(cam12, model);
  reprojEval(c, T_WS, hp, T_SC, u, v, w, r, Jp, Jl, Je);
}
}
