// The trust-region options through the shim (integration/okvis/ceres/Map.hpp): the TestMap.cpp-shaped graph of shim_loss.cpp (pose,
// constant extrinsics, constant points, equidistant camera), solved with options.trust_region_strategy_type = LEVENBERG_MARQUARDT and
// a non-default initial radius -- the knobs the reference leaves commented out around its solve (Estimator.cpp:879-883).
// argv[1]: "lm" or "dogleg"; argv[2]: initial radius; argv[3]: max radius.
// Prints one line per residual, "obs <point id> <u> <v> <x> <y> <z>" (17 significant digits: the caller rebuilds the same problem
// through the C ABI), "get <strategy> <initial> <max>" as svin_ba_get_trust_region reports them after the solve, one line
// "row <6 doubles>" per row of svin_ba_get_iteration_log, and "pose <7 doubles> final_cost <c> initial_cost <c0> iterations <it>".
#include <okvis/MultiFrame.hpp>
#include <okvis/ceres/Map.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace {
void quatRotate(const double q[4], const double v[3], double out[3]) {   // q = (x, y, z, w)
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                       2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
  for (int i = 0; i < 3; ++i) out[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}
okvis::kinematics::Transformation makeT(const double r[3], const double q[4]) {
  return okvis::kinematics::Transformation(Eigen::Vector3d(r[0], r[1], r[2]), Eigen::Quaterniond(q[3], q[0], q[1], q[2]));
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const bool lm = std::strcmp(argv[1], "lm") == 0;
  const double rWS[3] = {1.0, -2.0, 0.5}, qWS[4] = {0.0, 0.0, 0.0, 1.0};
  const double rInit[3] = {1.4, -2.3, 0.2};
  const double rSC[3] = {0.1, -0.05, 0.02}, qSC[4] = {0.0, 0.0, 0.0, 1.0};
  std::shared_ptr<okvis::ceres::PoseParameterBlock> pose(new okvis::ceres::PoseParameterBlock(makeT(rInit, qWS), 1, okvis::Time(0, 0)));
  std::shared_ptr<okvis::ceres::PoseParameterBlock> extr(new okvis::ceres::PoseParameterBlock(makeT(rSC, qSC), 2, okvis::Time(0, 0)));
  okvis::ceres::Map map;
  // the shim's default is DOGLEG with Ceres' radii (Map.hpp says why)
  if (map.options.trust_region_strategy_type != ::ceres::DOGLEG || map.options.initial_trust_region_radius != 1e4 ||
      map.options.max_trust_region_radius != 1e16)
    return 3;
  if (!map.addParameterBlock(pose, okvis::ceres::Map::Pose6d) || !map.addParameterBlock(extr, okvis::ceres::Map::Pose6d)) return 5;
  map.setParameterBlockConstant(extr);
  typedef okvis::cameras::CameraBase Geometry;
  std::shared_ptr<const Geometry> geometry(new Geometry(752, 480, "EquidistantDistortion", {350.0, 360.0, 378.0, 238.0, -0.21, 0.14, 0.0006, 0.0003}));
  const double Tws[7] = {rWS[0], rWS[1], rWS[2], qWS[0], qWS[1], qWS[2], qWS[3]};
  const double Tsc[7] = {rSC[0], rSC[1], rSC[2], qSC[0], qSC[1], qSC[2], qSC[3]};
  const double intr[4] = {350.0, 360.0, 378.0, 238.0}, dist[4] = {-0.21, 0.14, 0.0006, 0.0003}, zero2[2] = {0, 0}, eye2[4] = {1, 0, 0, 1};
  const int N = 90;
  for (int i = 0; i < N; ++i) {
    const double depth = (double)(i % 10) * 3 + 2.0;
    const double pc[3] = {0.6 * std::sin(1.7 * i) * depth, 0.4 * std::cos(2.3 * i) * depth, depth};
    double ps[3], pw[3];
    quatRotate(qSC, pc, ps);
    for (int k = 0; k < 3; ++k) ps[k] += rSC[k];
    quatRotate(qWS, ps, pw);
    for (int k = 0; k < 3; ++k) pw[k] += rWS[k];
    const double hp[4] = {pw[0], pw[1], pw[2], 1.0};
    double r[2];
    if (svin_host_reprojection_error(SVIN_DIST_EQUIDISTANT, intr, dist, 4, Tws, hp, Tsc, zero2, eye2, r, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr) != 1) return 6;
    Eigen::Vector2d kp(-r[0] + 0.5 * std::sin(0.9 * i), -r[1] + 0.5 * std::cos(1.3 * i));
    Eigen::Vector4d start(pw[0], pw[1], pw[2], 1.0);
    std::shared_ptr<okvis::ceres::HomogeneousPointParameterBlock> point(new okvis::ceres::HomogeneousPointParameterBlock(start, i + 3));
    if (!map.addParameterBlock(point, okvis::ceres::Map::HomogeneousPoint)) return 7;
    if (!map.setParameterBlockConstant(point)) return 8;
    okvis::ceres::ReprojectionError<Geometry>::covariance_t information;
    information(0, 0) = 1.0; information(1, 1) = 1.0; information(0, 1) = 0.0; information(1, 0) = 0.0;
    std::shared_ptr<okvis::ceres::ReprojectionError<Geometry> > cost(new okvis::ceres::ReprojectionError<Geometry>(geometry, 1, kp, information));
    if (!map.addResidualBlock(cost, nullptr, pose, point, extr)) return 9;
    std::printf("obs %d %.17g %.17g %.17g %.17g %.17g\n", i + 3, kp[0], kp[1], pw[0], pw[1], pw[2]);
  }
  map.options.max_num_iterations = 20;
  map.options.trust_region_strategy_type = lm ? ::ceres::LEVENBERG_MARQUARDT : ::ceres::DOGLEG;
  map.options.initial_trust_region_radius = std::atof(argv[2]);
  map.options.max_trust_region_radius = std::atof(argv[3]);
  map.solve();
  int strategy = -1, rows = 0;
  double r0 = 0, rmax = 0;
  if (svin_ba_get_trust_region(map.handle(), &strategy, &r0, &rmax) != 1) return 10;
  std::printf("get %d %.17g %.17g\n", strategy, r0, rmax);
  if (svin_ba_get_iteration_log(map.handle(), 0, nullptr, &rows) != 1) return 11;
  std::vector<double> log(6 * (size_t)rows + 1);
  if (svin_ba_get_iteration_log(map.handle(), rows, log.data(), &rows) != 1) return 12;
  for (int i = 0; i < rows; ++i)
    std::printf("row %.17g %.17g %.17g %.17g %.17g %.17g\n", log[6 * i], log[6 * i + 1], log[6 * i + 2], log[6 * i + 3], log[6 * i + 4], log[6 * i + 5]);
  const double* x = pose->parameters();
  std::printf("pose %.17g %.17g %.17g %.17g %.17g %.17g %.17g final_cost %.17g initial_cost %.17g iterations %d\n", x[0], x[1], x[2], x[3], x[4],
              x[5], x[6], map.summary.final_cost, map.summary.initial_cost, (int)map.summary.iterations.size() - 1);
  return 0;
}
