// Loss functions through the shim (integration/okvis/ceres/Map.hpp): the TestMap.cpp-shaped graph of shim_map_tests.cpp part 2
// (pose, constant extrinsics, constant points, equidistant camera) with its reprojection residuals under NULL, HuberLoss(1) and
// CauchyLoss(2) in turn, plus a PoseError under HuberLoss(0.5).  Checks that ResidualBlockSpec::lossFunctionPtr hands back the
// object passed, that the device reports the matching kind and scale, and that a loss object the backend does not know throws.
// Prints "loss <n_ok> of <n> specs <m> unsupported_throws <0|1> final_cost <c> initial_cost <c0> d_trans <t>".
#include <okvis/MultiFrame.hpp>
#include <okvis/ceres/Map.hpp>

#include <cmath>
#include <cstdio>
#include <memory>

namespace {
struct OtherLoss : public ::ceres::LossFunction {};   // stands for SoftLOneLoss, TukeyLoss, ...: not supported
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

int main() {
  const double rWS[3] = {1.0, -2.0, 0.5}, qWS[4] = {0.0, 0.0, 0.0, 1.0};
  const double rInit[3] = {1.1, -2.05, 0.45};
  const double rSC[3] = {0.1, -0.05, 0.02}, qSC[4] = {0.0, 0.0, 0.0, 1.0};
  std::shared_ptr<okvis::ceres::PoseParameterBlock> pose(new okvis::ceres::PoseParameterBlock(makeT(rInit, qWS), 1, okvis::Time(0, 0)));
  std::shared_ptr<okvis::ceres::PoseParameterBlock> extr(new okvis::ceres::PoseParameterBlock(makeT(rSC, qSC), 2, okvis::Time(0, 0)));
  okvis::ceres::Map map;
  if (!map.addParameterBlock(pose, okvis::ceres::Map::Pose6d) || !map.addParameterBlock(extr, okvis::ceres::Map::Pose6d)) return 5;
  map.setParameterBlockConstant(extr);
  typedef okvis::cameras::CameraBase Geometry;
  std::shared_ptr<const Geometry> geometry(new Geometry(752, 480, "EquidistantDistortion", {350.0, 360.0, 378.0, 238.0, -0.21, 0.14, 0.0006, 0.0003}));
  ::ceres::HuberLoss huber(1.0);
  ::ceres::CauchyLoss cauchy(2.0);
  ::ceres::LossFunction* losses[3] = {nullptr, &huber, &cauchy};
  const int kinds[3] = {SVIN_LOSS_NONE, SVIN_LOSS_HUBER, SVIN_LOSS_CAUCHY};
  const double scales[3] = {1.0, 1.0, 2.0};
  const double Tws[7] = {rWS[0], rWS[1], rWS[2], qWS[0], qWS[1], qWS[2], qWS[3]};
  const double Tsc[7] = {rSC[0], rSC[1], rSC[2], qSC[0], qSC[1], qSC[2], qSC[3]};
  const double intr[4] = {350.0, 360.0, 378.0, 238.0}, dist[4] = {-0.21, 0.14, 0.0006, 0.0003}, zero2[2] = {0, 0}, eye2[4] = {1, 0, 0, 1};
  const int N = 90;
  int nOk = 0, unsupportedThrows = 0;
  std::shared_ptr<okvis::ceres::ReprojectionError<Geometry> > lastCost;
  std::shared_ptr<okvis::ceres::HomogeneousPointParameterBlock> lastPoint;
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
    const double out = (i % 15 == 1) ? 30.0 : 0.0;   // a few outliers, on HuberLoss(1) residuals
    Eigen::Vector2d kp(-r[0] + 0.5 * std::sin(0.9 * i) + out, -r[1] + 0.5 * std::cos(1.3 * i));
    Eigen::Vector4d start(pw[0], pw[1], pw[2], 1.0);
    std::shared_ptr<okvis::ceres::HomogeneousPointParameterBlock> point(new okvis::ceres::HomogeneousPointParameterBlock(start, i + 3));
    if (!map.addParameterBlock(point, okvis::ceres::Map::HomogeneousPoint)) return 7;
    if (!map.setParameterBlockConstant(point)) return 8;
    okvis::ceres::ReprojectionError<Geometry>::covariance_t information;
    information(0, 0) = 1.0; information(1, 1) = 1.0; information(0, 1) = 0.0; information(1, 0) = 0.0;
    std::shared_ptr<okvis::ceres::ReprojectionError<Geometry> > cost(new okvis::ceres::ReprojectionError<Geometry>(geometry, 1, kp, information));
    ::ceres::ResidualBlockId id = map.addResidualBlock(cost, losses[i % 3], pose, point, extr);
    if (!id) return 9;
    int kind = -1;
    double scale = 0.0;
    if (svin_ba_map_get_residual_loss(map.handle(), reinterpret_cast<uint64_t>(id), &kind, &scale) == 1 && kind == kinds[i % 3] &&
        scale == scales[i % 3])
      ++nOk;
    lastCost = cost;
    lastPoint = point;
  }
  // lossFunctionPtr round-trips: every spec of the pose block names the object passed for its residual
  int specs = 0;
  for (const okvis::ceres::Map::ResidualBlockSpec& s : map.residuals(pose->id())) {
    int kind = -1;
    double scale = 0.0;
    svin_ba_map_get_residual_loss(map.handle(), reinterpret_cast<uint64_t>(s.residualBlockId), &kind, &scale);
    const ::ceres::LossFunction* want = kind == SVIN_LOSS_NONE ? nullptr : (kind == SVIN_LOSS_HUBER ? static_cast<::ceres::LossFunction*>(&huber) : &cauchy);
    if (s.lossFunctionPtr == want) ++specs;
  }
  OtherLoss other;
  try {
    map.addResidualBlock(lastCost, &other, pose, lastPoint, extr);
  } catch (const std::exception&) {
    unsupportedThrows = 1;
  }
  std::shared_ptr<okvis::ceres::PoseError> prior(new okvis::ceres::PoseError(makeT(rWS, qWS), 1e-2, 1e-2));
  ::ceres::HuberLoss huberPrior(0.5);
  if (!map.addResidualBlock(prior, &huberPrior, pose)) return 10;
  map.options.max_num_iterations = 20;
  map.solve();
  const okvis::kinematics::Transformation est = pose->estimate();
  const double dTr = std::sqrt((est.r()[0] - rWS[0]) * (est.r()[0] - rWS[0]) + (est.r()[1] - rWS[1]) * (est.r()[1] - rWS[1]) +
                               (est.r()[2] - rWS[2]) * (est.r()[2] - rWS[2]));
  std::printf("loss %d of %d specs %d unsupported_throws %d final_cost %.6e initial_cost %.6e d_trans %.3e\n", nOk, N, specs,
              unsupportedThrows, map.summary.final_cost, map.summary.initial_cost, dTr);
  return 0;
}
