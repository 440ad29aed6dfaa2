// Map::getLhs through the shim (integration/okvis/ceres/Map.hpp) in the shape of the reference's landmark loop
// (okvis_ceres/src/Estimator.cpp:902-923): a window dumped by tests/test_gpu_lhs.py is fed to okvis::Estimator as in
// tests/csrc/shim_smoke.cpp and optimised; then every landmark's 3 x 3 block is read with mapPtr_->getLhs(id, H) into a dynamic
// matrix type of this program's own (resize + operator(), the part of Eigen::MatrixXd the template needs), the block snapshot is
// read with parameterBlockPtr(id) as the reference does right after it, its quality is formed
// as the reference does, and the blocks are held bit for bit against one svin_ba_get_lhs_blocks call on the same handle.
// Prints "lhs <id> <9 values> q <quality>" per landmark, then "blocks <n> match <m> pose_dim <d> loop_us <t> loop_passes <k>
// same_point <s>": k = all-blocks passes the loop ran (parameterBlockPtr is a look-up: one pass for the whole loop).
#include <okvis/Estimator.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

struct PinholeRadTan {};   // plays the GEOMETRY_TYPE template argument of addObservation

namespace {
struct DynMatrix {   // what Map::getLhs needs of Eigen::MatrixXd
  int rows = 0, cols = 0;
  std::vector<double> a;
  void resize(int r, int c) { rows = r; cols = c; a.assign((size_t)r * c, 0.0); }
  double& operator()(int i, int j) { return a[(size_t)i * cols + j]; }
};
// eigenvalues of a symmetric 3 x 3 (cyclic Jacobi): what Eigen::SelfAdjointEigenSolver<Matrix3d> gives the reference loop
void eig3(const double* H, double* lo, double* hi) {
  double A[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) A[i][j] = H[3 * i + j];
  for (int sweep = 0; sweep < 50; ++sweep) {
    const double off = std::fabs(A[0][1]) + std::fabs(A[0][2]) + std::fabs(A[1][2]);
    if (off < 1e-300) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (A[p][q] == 0.0) continue;
        const double th = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (th >= 0 ? 1.0 : -1.0) / (std::fabs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
      }
  }
  *lo = std::fmin(A[0][0], std::fmin(A[1][1], A[2][2]));
  *hi = std::fmax(A[0][0], std::fmax(A[1][1], A[2][2]));
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  int nCam;
  in >> nCam;
  std::vector<std::shared_ptr<const okvis::cameras::CameraBase>> geo;
  std::vector<std::shared_ptr<const okvis::kinematics::Transformation>> T_SC;
  okvis::Estimator est(0);
  for (int c = 0; c < nCam; ++c) {
    std::string dist;
    int w, h, nIntr;
    in >> dist >> w >> h >> nIntr;
    std::vector<double> intr(nIntr);
    for (double& v : intr) in >> v;
    double T[7], s[4];
    for (double& v : T) in >> v;
    for (double& v : s) in >> v;
    geo.push_back(std::make_shared<okvis::cameras::CameraBase>(w, h, dist, intr));
    T_SC.push_back(std::make_shared<okvis::kinematics::Transformation>(Eigen::Vector3d(T[0], T[1], T[2]), Eigen::Quaterniond(T[6], T[3], T[4], T[5])));
    okvis::ExtrinsicsEstimationParameters e;
    e.sigma_absolute_translation = s[0]; e.sigma_absolute_orientation = s[1];
    e.sigma_c_relative_translation = s[2]; e.sigma_c_relative_orientation = s[3];
    if (est.addCamera(e) != c) return 3;
  }
  okvis::ImuParameters ip;
  in >> ip.a_max >> ip.g_max >> ip.sigma_g_c >> ip.sigma_a_c >> ip.sigma_bg >> ip.sigma_ba >> ip.sigma_gw_c >> ip.sigma_aw_c >> ip.tau >> ip.g;
  in >> ip.a0[0] >> ip.a0[1] >> ip.a0[2];
  if (est.addImu(ip) != 0) return 4;
  int L;
  in >> L;
  std::vector<uint64_t> lmIds(L);
  for (int l = 0; l < L; ++l) {
    double hp[4];
    for (double& v : hp) in >> v;
    lmIds[l] = okvis::IdProvider::instance().newId();
    if (!est.addLandmark(lmIds[l], Eigen::Vector4d(hp[0], hp[1], hp[2], hp[3]))) return 5;
  }
  int P, numKf, numImu, iters;
  in >> P >> numKf >> numImu >> iters;
  std::vector<uint64_t> frameIds;
  for (int k = 0; k < P; ++k) {
    auto mf = std::make_shared<okvis::MultiFrame>();
    int keyframe, nImu, nObs;
    in >> mf->stamp_.sec >> mf->stamp_.nsec >> keyframe >> nImu;
    okvis::ImuMeasurementDeque imu;
    for (int i = 0; i < nImu; ++i) {
      okvis::ImuMeasurement m;
      in >> m.timeStamp.sec >> m.timeStamp.nsec;
      for (int a = 0; a < 3; ++a) in >> m.measurement.gyroscopes[a];
      for (int a = 0; a < 3; ++a) in >> m.measurement.accelerometers[a];
      imu.push_back(m);
    }
    double Tinit[7], sbInit[9];
    for (double& v : Tinit) in >> v;
    for (double& v : sbInit) in >> v;
    in >> nObs;
    struct Obs { int lm, cam; double u, v, size; };
    std::vector<Obs> obs(nObs);
    mf->kps_.assign(nCam, {});
    for (Obs& o : obs) {
      in >> o.lm >> o.cam >> o.u >> o.v >> o.size;
      mf->kps_[o.cam].push_back({o.u, o.v, o.size});
    }
    // pad with unmatched keypoints so that numKeypoints() > 10 on the first frame (Estimator.cpp:116-122)
    while (mf->numKeypoints() < 400) mf->kps_[0].push_back({0.0, 0.0, 8.0});
    mf->id_ = okvis::IdProvider::instance().newId();
    mf->T_SC_ = T_SC;
    mf->geo_ = geo;
    if (!est.addStates(mf, imu, keyframe != 0)) { std::printf("addStates failed at frame %d\n", k); return 6; }
    frameIds.push_back(mf->id());
    if (k > 0) est.set_T_WS(mf->id(), okvis::kinematics::Transformation(Eigen::Vector3d(Tinit[0], Tinit[1], Tinit[2]),
                                                                        Eigen::Quaterniond(Tinit[6], Tinit[3], Tinit[4], Tinit[5])));
    okvis::SpeedAndBias sb;
    for (int a = 0; a < 9; ++a) sb[a] = sbInit[a];
    est.setSpeedAndBias(mf->id(), 0, sb);
    std::vector<size_t> next(nCam, 0);
    for (const Obs& o : obs) {
      const size_t kp = next[o.cam]++;
      // NULL: the landmark has been marginalised in the meantime (the frontend checks isLandmarkAdded first, Frontend.cpp:928)
      if (est.addObservation<PinholeRadTan>(lmIds[o.lm], mf->id(), o.cam, kp) == nullptr && est.isLandmarkAdded(lmIds[o.lm])) return 7;
    }
    // a duplicate returns NULL (implementation/Estimator.hpp:55-57)
    for (const Obs& o : obs)
      if (est.isLandmarkAdded(lmIds[o.lm])) {
        if (est.addObservation<PinholeRadTan>(lmIds[o.lm], mf->id(), o.cam, 0) != nullptr && o.cam == obs[0].cam && &o == &obs[0]) return 8;
        break;
      }
    if (numKf > 0) {
      est.optimize(iters, 2, false);
      okvis::MapPointVector removed;
      if (!est.applyMarginalizationStrategy(numKf, numImu, removed)) return 9;
      std::printf("frame %d removed %zu stateCount %d frames %zu\n", k, removed.size(), est.stateCount_, est.numFrames());
    }
  }
  if (numKf == 0) est.optimize(iters, 2, false);
  okvis::PointMap lms;
  est.getLandmarks(lms);
  std::vector<uint64_t> ids;
  std::vector<double> mine;
  const int64_t passes0 = svin_ba_get_lhs_pass_count(est.handle());
  size_t samePoint = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (auto it = lms.begin(); it != lms.end(); ++it) {   // Estimator.cpp:902-923
    DynMatrix H;
    H.resize(3, 3);
    est.map()->getLhs(it->first, H);
    if (H.rows != 3 || H.cols != 3) return 10;
    ids.push_back(it->first);
    mine.insert(mine.end(), H.a.begin(), H.a.end());
    // "update coordinates" (:919-921): the block snapshot read right after getLhs, as the reference does
    const Eigen::Vector4d point =
        std::static_pointer_cast<okvis::ceres::HomogeneousPointParameterBlock>(est.map()->parameterBlockPtr(it->first))->estimate();
    samePoint += point[0] == it->second.point[0] && point[3] == it->second.point[3];
  }
  const double loopUs = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  const int64_t loopPasses = svin_ba_get_lhs_pass_count(est.handle()) - passes0;
  for (size_t i = 0; i < ids.size(); ++i) {
    double lo = 0, hi = 0;
    eig3(&mine[9 * i], &lo, &hi);
    const double q = lo < 1.0e-12 ? 0.0 : std::sqrt(lo) / std::sqrt(hi);
    std::printf("lhs %llu", (unsigned long long)ids[i]);
    for (int k = 0; k < 9; ++k) std::printf(" %.17g", mine[9 * i + k]);
    std::printf(" q %.17g\n", q);
  }
  // the same blocks from one batched call on the estimator's handle
  std::vector<int32_t> dims(ids.size());
  const int64_t total = svin_ba_get_lhs_blocks(est.handle(), (int)ids.size(), ids.data(), dims.data(), nullptr, 0);
  if (total != (int64_t)mine.size()) return 11;
  std::vector<double> all((size_t)total);
  if (svin_ba_get_lhs_blocks(est.handle(), (int)ids.size(), ids.data(), dims.data(), all.data(), total) != total) return 12;
  size_t match = 0;
  for (size_t i = 0; i < ids.size(); ++i) match += dims[i] == 3 && std::memcmp(&all[9 * i], &mine[9 * i], 9 * sizeof(double)) == 0;
  DynMatrix Hp;
  est.map()->getLhs(est.currentFrameId(), Hp);
  std::printf("blocks %zu match %zu pose_dim %d loop_us %.1f loop_passes %lld same_point %zu\n", ids.size(), match, Hp.rows, loopUs,
              (long long)loopPasses, samePoint);
  return 0;
}
