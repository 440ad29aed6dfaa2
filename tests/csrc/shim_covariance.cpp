// Map::getCovarianceBlock through the shim (integration/okvis/ceres/Map.hpp): what the reference's Map::computeCovariance
// (Map.hpp:352-372) asks of ::ceres::Covariance, read into a dynamic matrix type of this program's own (resize + operator(), the
// part of Eigen::MatrixXd the template needs).  Built with every warning an error by tests/test_covariance_shim_compile.py; run
// on a GPU it prints the covariance of the newest pose of an empty window's first frame, or the error the backend reports.
#include <okvis/Estimator.hpp>

#include <cstdio>
#include <vector>

namespace {
struct DynMatrix {
  int rows = 0, cols = 0;
  std::vector<double> a;
  void resize(int r, int c) { rows = r; cols = c; a.assign((size_t)r * c, 0.0); }
  double& operator()(int i, int j) { return a[(size_t)i * cols + j]; }
};
}  // namespace

int main(int argc, char** argv) {
  okvis::Estimator est(0);
  const uint64_t a = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1, b = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : a;
  DynMatrix cov;
  try {
    if (!est.map()->getCovarianceBlock(a, b, cov)) {
      std::printf("singular: %s\n", svin_ba_last_error());
      return 0;
    }
  } catch (const std::exception& e) {
    std::printf("error: %s\n", e.what());
    return 0;
  }
  for (int i = 0; i < cov.rows; ++i) {
    for (int j = 0; j < cov.cols; ++j) std::printf("%.17g ", cov(i, j));
    std::printf("\n");
  }
  return svin_ba_get_covariance_pass_count(nullptr) == SVIN_ERR_INVALID_ARG ? 0 : 1;
}
