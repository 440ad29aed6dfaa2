// svin_amd C ABI (include/svin_ba.h).  Plain pointers and sizes only; nothing throws across the boundary.
#include "../../include/svin_ba.h"

#include <algorithm>
#include "window.hpp"
#include <vector>

using namespace svin;

struct svin_ba {
  Window w;
  explicit svin_ba(int device) : w(device) {}
};

// The window keeps its last getLhs pass (Window::getLhs) and its last covariance pass (Window::getCovarianceBlocks) until something changes.  An entry point that calls a NON-const method of
// the window -- every setter, graph edit, parameterisation change, solve, marginalisation, and the inspection hooks that evaluate --
// reaches it through win(), which drops that result; the look-ups (const methods: getters, graph queries, parameterBlockPtr's
// svin_ba_get_parameter_block) go through ro(), which cannot call a non-const method, and keep it.  So the reference's landmark loop
// (Estimator.cpp:902-923: getLhs, then parameterBlockPtr, per landmark) costs one pass.
static inline Window& win(svin_ba* h) {
  h->w.invalidateLhs();
  h->w.invalidateCovariance();
  return h->w;
}
static inline const Window& ro(const svin_ba* h) { return h->w; }

#define GUARD_BEGIN try {
#define GUARD_END(errval)                     \
  }                                           \
  catch (const std::exception& e) {           \
    lastError() = e.what();                   \
    return errval;                            \
  }                                           \
  catch (...) {                               \
    lastError() = "unknown error";            \
    return errval;                            \
  }

// function-try-block tail for the entry points that are host look-ups most of the time but may reach quiesce() /
// syncLandmarks() (which rethrow what the asynchronous marginalisation job threw, or a HIP error): nothing crosses the C ABI
#define CATCH_ALL(errval)                     \
  catch (const std::exception& e) {           \
    lastError() = e.what();                   \
    return errval;                            \
  }                                           \
  catch (...) {                               \
    lastError() = "unknown error";            \
    return errval;                            \
  }

static void splitSamples(const svin_imu_sample* imu, int n, std::vector<uint32_t>& t, std::vector<double>& m) {
  t.resize(2 * (size_t)n);
  m.resize(6 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    t[2 * i] = imu[i].sec; t[2 * i + 1] = imu[i].nsec;
    for (int k = 0; k < 3; ++k) { m[6 * i + k] = imu[i].gyr[k]; m[6 * i + 3 + k] = imu[i].acc[k]; }
  }
}
static ImuParams toParams(const svin_imu_params* p) {
  ImuParams q;
  q.a_max = p->a_max; q.g_max = p->g_max; q.sigma_g_c = p->sigma_g_c; q.sigma_a_c = p->sigma_a_c;
  q.sigma_bg = p->sigma_bg; q.sigma_ba = p->sigma_ba; q.sigma_gw_c = p->sigma_gw_c; q.sigma_aw_c = p->sigma_aw_c;
  q.tau = p->tau; q.g = p->g;
  q.a0[0] = p->a0[0]; q.a0[1] = p->a0[1]; q.a0[2] = p->a0[2];
  return q;
}

extern "C" {

svin_ba* svin_ba_create(int device) {
  try {
    return new svin_ba(device);
  } catch (const std::exception& e) {
    lastError() = e.what();
    return nullptr;
  } catch (...) {
    lastError() = "unknown error";
    return nullptr;
  }
}
void svin_ba_destroy(svin_ba* h) { delete h; }
const char* svin_ba_last_error(void) { return lastError().c_str(); }
uint64_t svin_ba_new_id(svin_ba* h) try { return h ? win(h).newId() : 0; } CATCH_ALL(0)
int svin_ba_set_id_provider(svin_ba* h, svin_id_provider_fn fn, void* user) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  win(h).setIdProvider(fn, user);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_reserve_ids(svin_ba* h, uint64_t largest) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  win(h).reserveIds(largest);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_camera_geometry(svin_ba* h, uint64_t cam, int model, const double intr[4], const double* dist, int n_dist,
                                int width, int height) try {
  if (!h || !intr || (n_dist > 0 && !dist) || n_dist < 0 || n_dist > 8) return SVIN_ERR_INVALID_ARG;
  return win(h).setCameraGeometry(cam, model, intr, dist, n_dist, width, height) ? 1 : SVIN_ERR_NOT_FOUND;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_clear_cameras(svin_ba* h) try { if (!h) return SVIN_ERR_INVALID_ARG; win(h).clearCameras(); return 1; } CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_clear_imus(svin_ba* h) try { if (!h) return SVIN_ERR_INVALID_ARG; win(h).clearImus(); return 1; } CATCH_ALL(SVIN_ERR_DEVICE)

int svin_ba_add_camera(svin_ba* h, int model, const double intr[4], const double* dist, int n_dist, int width, int height,
                       const double sigmas[4]) {
  if (!h || !intr || !sigmas) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).addCamera(model, intr, dist, n_dist, width, height, sigmas);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_add_imu(svin_ba* h, const svin_imu_params* p) {
  if (!h || !p) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).addImu(toParams(p));
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_set_sonar_extrinsics(svin_ba* h, const double T_SSo[7]) try {
  if (!h || !T_SSo) return SVIN_ERR_INVALID_ARG;
  win(h).setSonarExtrinsics(T_SSo);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_add_states(svin_ba* h, uint64_t frame_id, uint32_t sec, uint32_t nsec, uint64_t num_keypoints,
                       const double* T_SC, int n_cam, const svin_imu_sample* imu, int n_imu, int as_keyframe,
                       const double* sonar, int n_sonar, const double* depth, int n_depth, double first_depth) {
  if (!h || n_imu < 0 || n_cam < 0 || n_sonar < 0 || n_depth < 0 || (n_imu > 0 && !imu) || (n_cam > 0 && !T_SC) ||
      (n_sonar > 0 && !sonar) || (n_depth > 0 && !depth))
    return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
  std::vector<uint32_t> t;
  std::vector<double> m;
  splitSamples(imu, n_imu, t, m);
  TimeStamp ts; ts.sec = sec; ts.nsec = nsec;
  return win(h).addStates(frame_id, ts, num_keypoints, T_SC, n_cam, t.data(), m.data(), n_imu, as_keyframe != 0, sonar,
                        n_sonar, depth, n_depth, first_depth);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_add_landmark(svin_ba* h, uint64_t id, const double hp[4]) {
  if (!h || !hp) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).addLandmark(id, hp);
  GUARD_END(SVIN_ERR_DEVICE)
}
uint64_t svin_ba_add_observation(svin_ba* h, uint64_t lm, uint64_t pose, uint64_t cam, uint64_t kp, const double uv[2],
                                 double size) {
  if (!h || !uv) return 0;
  GUARD_BEGIN return win(h).addObservation(lm, pose, cam, kp, uv, size);
  GUARD_END(0)
}
int svin_ba_add_observations(svin_ba* h, int n, const uint64_t* lm, const uint64_t* pose, const uint64_t* cam, const uint64_t* kp,
                             const double* uv, const double* size, uint64_t* out_ids) {
  if (!h || n < 0 || (n > 0 && (!lm || !pose || !cam || !kp || !uv || !size))) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).addObservations(n, lm, pose, cam, kp, uv, size, out_ids);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_remove_observation(svin_ba* h, uint64_t lm, uint64_t pose, uint64_t cam, uint64_t kp) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).removeObservation(lm, pose, cam, kp);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_remove_observation_by_id(svin_ba* h, uint64_t rid) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).removeObservationById(rid);
  GUARD_END(SVIN_ERR_DEVICE)
}
uint64_t svin_ba_add_homogeneous_point_error(svin_ba* h, uint64_t lm, const double* meas, const double* info) {
  if (!h || !meas || !info) return 0;
  try { return win(h).addLandmarkPrior(lm, meas, info); } catch (const std::exception& e) { svin::lastError() = e.what(); return 0; }
}
int svin_ba_remove_homogeneous_point_error(svin_ba* h, uint64_t rid) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).removeLandmarkPrior(rid);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_optimize(svin_ba* h, uint64_t num_iter, uint64_t, int verbose) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).optimize(num_iter, verbose != 0);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_prepare(svin_ba* h) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).prepare();
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_solve_prepared(svin_ba* h, uint64_t num_iter, int verbose) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).solvePrepared(num_iter, verbose != 0);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_solve_prepared_batch(svin_ba* const* hs, int n, uint64_t num_iter, int verbose, int* n_batched) {
  if (n_batched) *n_batched = 0;
  if (n < 0 || (n > 0 && !hs)) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
    std::vector<svin::Window*> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      if (!hs[i]) return SVIN_ERR_INVALID_ARG;
      ws[(size_t)i] = &win(hs[i]);
    }
    return svin::Window::solvePreparedBatch(ws.data(), n, num_iter, verbose != 0, n_batched);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_optimize_batch(svin_ba* const* hs, int n, uint64_t num_iter, int verbose, int* n_batched) {
  if (n_batched) *n_batched = 0;
  if (n < 0 || (n > 0 && !hs)) return SVIN_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i)
    if (!hs[i]) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
    for (int i = 0; i < n; ++i) win(hs[i]).prepare();
  GUARD_END(SVIN_ERR_DEVICE)
  const int rc = svin_ba_solve_prepared_batch(hs, n, num_iter, verbose, n_batched);
  if (rc != 1) return rc;
  GUARD_BEGIN
    for (int i = 0; i < n; ++i) win(hs[i]).finish();
    return 1;
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_finish(svin_ba* h) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).finish();
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_invalidate_preintegration(svin_ba* h) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  win(h).invalidatePreintegration();
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_optimization_time_limit(svin_ba* h, double tl, int min_iter) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  return win(h).setOptimizationTimeLimit(tl, min_iter);
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_apply_marginalization_strategy(svin_ba* h, uint64_t nkf, uint64_t nimu, uint64_t* removed, int cap,
                                           int* n_removed) {
  if (!h || cap < 0 || (cap > 0 && !removed)) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
  std::vector<uint64_t> rem;
  const int r = win(h).applyMarginalizationStrategy(nkf, nimu, rem);
  if (n_removed) *n_removed = (int)rem.size();
  for (int i = 0; i < (int)rem.size() && i < cap; ++i) removed[i] = rem[i];
  return r;
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_get_summary(svin_ba* h, svin_summary* out) try {
  if (!h || !out) return SVIN_ERR_INVALID_ARG;
  const Summary& s = ro(h).summary();
  out->initial_cost = s.initial_cost; out->final_cost = s.final_cost; out->iterations = s.iterations;
  out->num_successful_steps = s.num_successful_steps; out->termination = s.termination;
  out->total_time_s = s.total_time; out->upload_time_s = s.upload_time; out->solve_time_s = s.solve_time;
  out->download_time_s = s.download_time;
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_distributed(svin_ba* h, int rank, int world, svin_allreduce_fn fn, void* user) try {
  if (!h || world < 1 || rank < 0 || rank >= world || (world > 1 && !fn)) return SVIN_ERR_INVALID_ARG;
  if (world > svin::kScalGatherSlots / 2) {   // every rank publishes its (gradient max, factorisation flag) pair in a slot of its own
    svin::lastError() = "set_distributed: at most " + std::to_string(svin::kScalGatherSlots / 2) + " ranks (one node of MI355X)";
    return SVIN_ERR_INVALID_ARG;
  }
  if (world > 1 && ro(h).hasNonDefaultLoss()) {   // (svin_ba_map_set_residual_loss refuses them in sharded mode, too)
    svin::lastError() = "set_distributed: the window has residuals with a non-default loss function (not available in sharded mode)";
    return SVIN_ERR_UNSUPPORTED;
  }
  if (world > 1 && ro(h).levenbergMarquardt()) {   // (svin_ba_set_trust_region refuses it in sharded mode, too)
    svin::lastError() = "set_distributed: the handle has the Levenberg-Marquardt strategy set (not available in sharded mode)";
    return SVIN_ERR_UNSUPPORTED;
  }
  win(h).setDistributed(rank, world, fn, user);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_rccl_unique_id(unsigned char id_out[128]) {
  if (!id_out) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return Window::rcclUniqueId(id_out);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_set_distributed_rccl(svin_ba* h, int rank, int world, const unsigned char id[128]) {
  if (!h || !id || world < 1 || rank < 0 || rank >= world) return SVIN_ERR_INVALID_ARG;
  if (world > svin::kScalGatherSlots / 2) {
    svin::lastError() = "set_distributed_rccl: at most " + std::to_string(svin::kScalGatherSlots / 2) + " ranks (one node of MI355X)";
    return SVIN_ERR_INVALID_ARG;
  }
  GUARD_BEGIN
  if (world > 1 && ro(h).hasNonDefaultLoss()) {
    svin::lastError() = "set_distributed_rccl: the window has residuals with a non-default loss function (not available in sharded mode)";
    return SVIN_ERR_UNSUPPORTED;
  }
  if (ro(h).levenbergMarquardt()) {
    svin::lastError() = "set_distributed_rccl: the handle has the Levenberg-Marquardt strategy set (not available in sharded mode)";
    return SVIN_ERR_UNSUPPORTED;
  }
  return win(h).setDistributedRccl(rank, world, id);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_set_solver_tolerances(svin_ba* h, double f, double g, double p) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  win(h).setTolerances(f, g, p);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
// (neither goes through win(): no value of the window changes, the kept getLhs / covariance passes stay)
int svin_ba_set_trust_region(svin_ba* h, int strategy, double initial_radius, double max_radius) try {
  return h ? h->w.setTrustRegion(strategy, initial_radius, max_radius) : SVIN_ERR_INVALID_ARG;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_trust_region(svin_ba* h, int* strategy, double* initial_radius, double* max_radius) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  ro(h).getTrustRegion(strategy, initial_radius, max_radius);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_iteration_log(svin_ba* h, int cap_rows, double* out, int* n_rows) try {
  if (!h || cap_rows < 0 || (cap_rows > 0 && !out)) return SVIN_ERR_INVALID_ARG;
  const std::vector<double>& log = ro(h).iterationLog();
  const int n = (int)(log.size() / 6);
  if (n_rows) *n_rows = n;
  std::copy(log.begin(), log.begin() + 6 * (size_t)std::min(n, cap_rows), out);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_T_WS(svin_ba* h, uint64_t id, double T[7]) try { return h ? ro(h).get_T_WS(id, T) : SVIN_ERR_INVALID_ARG; } CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_speed_and_bias(svin_ba* h, uint64_t id, uint64_t imu, double sb[9]) try {
  return h ? ro(h).getSpeedAndBias(id, imu, sb) : SVIN_ERR_INVALID_ARG;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_camera_sensor_states(svin_ba* h, uint64_t id, uint64_t cam, double T[7]) try {
  return h ? ro(h).getCameraSensorStates(id, cam, T) : SVIN_ERR_INVALID_ARG;
} CATCH_ALL(SVIN_ERR_DEVICE)
static void fillInfo(const Landmark& lm, svin_landmark_info* out) {
  for (int k = 0; k < 4; ++k) out->point[k] = lm.hp[k];
  out->quality = lm.quality; out->distance = lm.distance;
  out->num_observations = (int32_t)lm.obs.size();
  out->initialized = lm.initialized ? 1 : 0;
}
int svin_ba_get_landmark(svin_ba* h, uint64_t id, svin_landmark_info* out) try {
  if (!h || !out) return SVIN_ERR_INVALID_ARG;
  const Landmark* lm = ro(h).landmark(id);
  if (!lm) return 0;
  fillInfo(*lm, out);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_landmarks(svin_ba* h, uint64_t* ids, svin_landmark_info* infos, int cap) try {
  if (!h || cap < 0) return SVIN_ERR_INVALID_ARG;
  int n = 0;
  for (const auto& kv : ro(h).landmarks()) {
    if (n < cap) {
      if (ids) ids[n] = kv.first;
      if (infos) fillInfo(kv.second, infos + n);
    }
    ++n;
  }
  return n;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_landmark_observations(svin_ba* h, uint64_t id, uint64_t* frames, uint64_t* cams, uint64_t* kps, uint64_t* rids,
                                      int cap) try {
  if (!h || cap < 0) return SVIN_ERR_INVALID_ARG;
  const Landmark* lm = ro(h).landmarkGraph(id);
  if (!lm) return SVIN_ERR_NOT_FOUND;
  std::vector<const svin::Observation*> sorted;
  for (const svin::Observation& o : lm->obs) sorted.push_back(&o);
  std::sort(sorted.begin(), sorted.end(), [](const svin::Observation* a, const svin::Observation* b) {
    if (a->poseId != b->poseId) return a->poseId < b->poseId;
    if (a->cam != b->cam) return a->cam < b->cam;
    return a->kp < b->kp;
  });
  for (int i = 0; i < (int)sorted.size() && i < cap; ++i) {
    if (frames) frames[i] = sorted[i]->poseId;
    if (cams) cams[i] = (uint64_t)sorted[i]->cam;
    if (kps) kps[i] = sorted[i]->kp;
    if (rids) rids[i] = sorted[i]->resId;
  }
  return (int)sorted.size();
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_all_landmark_observations(svin_ba* h, int cap_landmarks, uint64_t* ids, svin_landmark_info* infos, int32_t* obs_ptr,
                                          int cap_obs, uint64_t* frames, uint64_t* cams, uint64_t* kps, uint64_t* rids, int32_t* n_obs_total) try {
  if (!h || cap_landmarks < 0 || cap_obs < 0) return SVIN_ERR_INVALID_ARG;
  int n = 0, total = 0;
  std::vector<const svin::Observation*> sorted;
  for (const auto& kv : ro(h).landmarks()) {
    const Landmark& lm = kv.second;
    if (n < cap_landmarks) {
      if (ids) ids[n] = kv.first;
      if (infos) fillInfo(lm, infos + n);
      if (obs_ptr) obs_ptr[n] = total;
      sorted.clear();
      for (const svin::Observation& o : lm.obs) sorted.push_back(&o);
      std::sort(sorted.begin(), sorted.end(), [](const svin::Observation* a, const svin::Observation* b) {
        if (a->poseId != b->poseId) return a->poseId < b->poseId;
        if (a->cam != b->cam) return a->cam < b->cam;
        return a->kp < b->kp;
      });
      for (size_t i = 0; i < sorted.size(); ++i) {
        const int at = total + (int)i;
        if (at >= cap_obs) break;
        if (frames) frames[at] = sorted[i]->poseId;
        if (cams) cams[at] = (uint64_t)sorted[i]->cam;
        if (kps) kps[at] = sorted[i]->kp;
        if (rids) rids[at] = sorted[i]->resId;
      }
    }
    total += (int)lm.obs.size();
    ++n;
  }
  if (obs_ptr && n <= cap_landmarks) obs_ptr[n] = total;
  if (n_obs_total) *n_obs_total = total;
  return n;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_parameter_block(svin_ba* h, uint64_t id, int32_t* type, double* values, uint32_t* sec, uint32_t* nsec, int32_t* fixed,
                                int32_t* initialized) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  return ro(h).getParameterBlock(id, type, values, sec, nsec, fixed, initialized);
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_parameter_block_ids(svin_ba* h, uint64_t* ids, int cap) try {
  if (!h || cap < 0 || (cap > 0 && !ids)) return SVIN_ERR_INVALID_ARG;
  std::vector<uint64_t> v;
  ro(h).parameterBlockIds(v);
  for (int i = 0; i < (int)v.size() && i < cap; ++i) ids[i] = v[i];
  return (int)v.size();
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_is_landmark_initialized(svin_ba* h, uint64_t id) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  const Landmark* lm = ro(h).landmarkGraph(id);
  return lm ? (lm->initialized ? 1 : 0) : SVIN_ERR_NOT_FOUND;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_landmark_initialized(svin_ba* h, uint64_t id, int initialized) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  return win(h).setLandmarkInitialized(id, initialized != 0) ? 1 : SVIN_ERR_NOT_FOUND;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_keyframe(svin_ba* h, uint64_t id, int is_kf) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  return win(h).setKeyframe(id, is_kf != 0) ? 1 : SVIN_ERR_NOT_FOUND;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_timestamp(svin_ba* h, uint64_t id, uint32_t* sec, uint32_t* nsec) try {
  if (!h || !sec || !nsec) return SVIN_ERR_INVALID_ARG;
  auto it = ro(h).states().find(id);
  if (it == ro(h).states().end()) return SVIN_ERR_NOT_FOUND;
  *sec = it->second.stamp.sec; *nsec = it->second.stamp.nsec;
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_state_count(svin_ba* h) try { return h ? ro(h).stateCount() : SVIN_ERR_INVALID_ARG; } CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_imu_preintegral(svin_ba* h, uint64_t pose_id, double adi[3], double ai[3], double* dt) try {
  if (!h || !adi || !ai || !dt) return SVIN_ERR_INVALID_ARG;
  double v[7];
  if (!ro(h).getImuPreIntegral(pose_id, v)) return 0;
  for (int k = 0; k < 3; ++k) { adi[k] = v[k]; ai[k] = v[3 + k]; }
  *dt = v[6];
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_imu_preintegral(svin_ba* h, uint64_t pose_id, const double adi[3], const double ai[3], double dt) try {
  if (!h || !adi || !ai) return SVIN_ERR_INVALID_ARG;
  const double v[7] = {adi[0], adi[1], adi[2], ai[0], ai[1], ai[2], dt};
  win(h).setImuPreIntegral(pose_id, v);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_init_pose_from_imu(const svin_imu_sample* imu, int n_imu, double T_WS[7]) {
  if (!T_WS || n_imu < 0 || (n_imu > 0 && !imu)) return SVIN_ERR_INVALID_ARG;
  std::vector<uint32_t> t;
  std::vector<double> m;
  splitSamples(imu, n_imu, t, m);
  return Window::initPoseFromImu(m.data(), n_imu, T_WS) ? 1 : 0;
}
int svin_ba_is_landmark_added(svin_ba* h, uint64_t id) try { return h && ro(h).landmarkExists(id) ? 1 : 0; } CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_T_WS(svin_ba* h, uint64_t id, const double T[7]) try { return h ? win(h).set_T_WS(id, T) : SVIN_ERR_INVALID_ARG; } CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_speed_and_bias(svin_ba* h, uint64_t id, uint64_t imu, const double sb[9]) try {
  return h ? win(h).setSpeedAndBias(id, imu, sb) : SVIN_ERR_INVALID_ARG;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_camera_sensor_states(svin_ba* h, uint64_t id, uint64_t cam, const double T[7]) try {
  return h ? win(h).setCameraSensorStates(id, cam, T) : SVIN_ERR_INVALID_ARG;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_landmark(svin_ba* h, uint64_t id, const double hp[4]) try { return h ? win(h).setLandmark(id, hp) : SVIN_ERR_INVALID_ARG; } CATCH_ALL(SVIN_ERR_DEVICE)
uint64_t svin_ba_num_frames(svin_ba* h) try { return h ? ro(h).states().size() : 0; } CATCH_ALL(0)
uint64_t svin_ba_num_landmarks(svin_ba* h) try { return h ? ro(h).numLandmarks() : 0; } CATCH_ALL(0)
uint64_t svin_ba_current_keyframe_id(svin_ba* h) try { return h ? ro(h).currentKeyframeId() : 0; } CATCH_ALL(0)
uint64_t svin_ba_current_frame_id(svin_ba* h) try { return (h && !ro(h).states().empty()) ? ro(h).states().rbegin()->first : 0; } CATCH_ALL(0)
uint64_t svin_ba_frame_id_by_age(svin_ba* h, uint64_t age) try { return h ? ro(h).frameIdByAge(age) : 0; } CATCH_ALL(0)
int svin_ba_is_keyframe(svin_ba* h, uint64_t id) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  auto it = ro(h).states().find(id);
  return it == ro(h).states().end() ? SVIN_ERR_NOT_FOUND : (it->second.isKeyframe ? 1 : 0);
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_is_in_imu_window(svin_ba* h, uint64_t id) try { return h ? (ro(h).isInImuWindow(id) ? 1 : 0) : SVIN_ERR_INVALID_ARG; } CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_frame_ids(svin_ba* h, uint64_t* ids, int cap) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  int n = 0;
  for (auto& kv : ro(h).states()) { if (n < cap && ids) ids[n] = kv.first; ++n; }
  return n;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_landmark_ids(svin_ba* h, uint64_t* ids, int cap) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  int n = 0;
  for (auto& kv : ro(h).landmarksGraph()) { if (n < cap && ids) ids[n] = kv.first; ++n; }
  return n;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_parameter_block_exists(svin_ba* h, uint64_t id) try { return h ? (ro(h).parameterBlockExists(id) ? 1 : 0) : SVIN_ERR_INVALID_ARG; } CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_parameter_block_constant(svin_ba* h, uint64_t id, int constant) try {
  return h ? win(h).setParameterBlockConstant(id, constant != 0) : SVIN_ERR_INVALID_ARG;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_reset_parameterization(svin_ba* h, uint64_t id, int parameterization) try {
  return h ? win(h).resetParameterization(id, parameterization) : SVIN_ERR_INVALID_ARG;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_parameterization(svin_ba* h, uint64_t id) try { return h ? ro(h).parameterization(id) : SVIN_ERR_INVALID_ARG; } CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_is_parameter_block_constant(svin_ba* h, uint64_t id) try { return h ? ro(h).isParameterBlockConstant(id) : SVIN_ERR_INVALID_ARG; } CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_residuals_of(svin_ba* h, uint64_t id, uint64_t* out, int cap) {
  if (!h || cap < 0 || (cap > 0 && !out)) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
  std::vector<uint64_t> v;
  if (!ro(h).residualsOf(id, v)) return SVIN_ERR_NOT_FOUND;
  for (int i = 0; i < (int)v.size() && i < cap; ++i) out[i] = v[i];
  return (int)v.size();
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_parameters_of(svin_ba* h, uint64_t rid, uint64_t* out, int cap, int32_t* kind) {
  if (!h || cap < 0 || (cap > 0 && !out)) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
  std::vector<uint64_t> v;
  if (!ro(h).parametersOf(rid, v)) return SVIN_ERR_NOT_FOUND;
  if (kind) *kind = ro(h).residualKind(rid);
  for (int i = 0; i < (int)v.size() && i < cap; ++i) out[i] = v[i];
  return (int)v.size();
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_keyframe_points(svin_ba* h, uint64_t frame_id, uint64_t cam_idx, int cap_points, uint64_t* lm_ids, double* xyz,
                            uint64_t* kp_idx, double* quality, int32_t* obs_ptr, int cap_obs, uint64_t* obs_frame_ids,
                            int32_t* n_obs_total) {
  if (!h || cap_points < 0 || cap_obs < 0) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
  int n = 0, no = 0;
  std::vector<const svin::Observation*> sorted;
  for (const auto& kv : ro(h).landmarks()) {   // PointMap order (std::map by landmark id)
    const svin::Landmark& lm = kv.second;
    // MapPoint::observations is ordered by (frame, camera, keypoint); the publisher takes the first entry of the frame
    sorted.clear();
    for (const svin::Observation& o : lm.obs) sorted.push_back(&o);
    std::sort(sorted.begin(), sorted.end(), [](const svin::Observation* a, const svin::Observation* b) {
      if (a->poseId != b->poseId) return a->poseId < b->poseId;
      if (a->cam != b->cam) return a->cam < b->cam;
      return a->kp < b->kp;
    });
    const svin::Observation* first = nullptr;
    for (const svin::Observation* o : sorted)
      if (o->poseId == frame_id) { first = o; break; }
    if (!first || (uint64_t)first->cam != cam_idx) continue;   // ThreadedKFVio.cpp:1167, :1183
    if (n < cap_points) {
      if (lm_ids) lm_ids[n] = lm.id;
      if (xyz) for (int k = 0; k < 3; ++k) xyz[3 * n + k] = lm.hp[k] / lm.hp[3];
      if (kp_idx) kp_idx[n] = first->kp;
      if (quality) quality[n] = lm.quality;
      if (obs_ptr) obs_ptr[n] = no;
    }
    for (const svin::Observation* o : sorted) {
      if (o->poseId == frame_id) continue;   // :1213
      if (no < cap_obs && obs_frame_ids) obs_frame_ids[no] = o->poseId;
      ++no;
    }
    ++n;
  }
  if (obs_ptr && n <= cap_points) obs_ptr[n] = no;
  if (n_obs_total) *n_obs_total = no;
  return n;
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_imu_propagation(svin_ba* h, const svin_imu_sample* imu, int n_imu, const svin_imu_params* p, double T[7],
                            double sb[9], uint32_t s0, uint32_t ns0, uint32_t s1, uint32_t ns1, double* cov, double* jac) {
  if (!h || !imu || !p) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
  std::vector<uint32_t> t;
  std::vector<double> m;
  splitSamples(imu, n_imu, t, m);
  TimeStamp a, b; a.sec = s0; a.nsec = ns0; b.sec = s1; b.nsec = ns1;
  return win(h).imuPropagation(t.data(), m.data(), n_imu, toParams(p), T, sb, a, b, cov, jac);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_imu_propagation_integrals(svin_ba* h, const svin_imu_sample* imu, int n_imu, const svin_imu_params* p, double T[7],
                                      double sb[9], uint32_t s0, uint32_t ns0, uint32_t s1, uint32_t ns1, double* cov,
                                      double* jac, double integrals[7]) {
  if (!h || !imu || !p || !T || !sb || n_imu < 0) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
  std::vector<uint32_t> t;
  std::vector<double> m;
  splitSamples(imu, n_imu, t, m);
  TimeStamp a, b; a.sec = s0; a.nsec = ns0; b.sec = s1; b.nsec = ns1;
  return win(h).imuPropagation(t.data(), m.data(), n_imu, toParams(p), T, sb, a, b, cov, jac, integrals);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_eval_reprojection(svin_ba* h, int robust, double* r, double* Jp, double* Jl, double* Je, int cap) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).evalReprojection(robust != 0, r, Jp, Jl, Je, cap);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_observation_ids(svin_ba* h, uint64_t* rid, uint64_t* lm, uint64_t* pose, int32_t* cam, int cap) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).observationIds(rid, lm, pose, cam, cap);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_eval_factors(svin_ba* h, int32_t* kind, int32_t* m, int32_t* ncols, double* r, double* J, uint64_t* blocks,
                         uint64_t* rids, int cap) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).evalFactors(kind, m, ncols, r, J, blocks, rids, cap);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_linearize(svin_ba* h, double mu, double* S, double* g, uint64_t* ids, int32_t* off, int32_t* nb, int cap_d,
                      double* cost) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).linearize(mu, S, g, ids, off, nb, cap_d, cost);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_wait_idle(svin_ba* h) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN win(h).waitIdle(); return 1;
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_reduced_solve(svin_ba* h, double mu, double* y, int cap_d) {
  if (!h || !y) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).debugReducedSolve(mu, y, cap_d);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_reduced_solve_ex(svin_ba* h, double mu, int fuse_finalize, double* y, int cap_d) {
  if (!h || !y) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).debugReducedSolve(mu, y, cap_d, fuse_finalize != 0);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_build_arrays(svin_ba* h, double* g_full, double* h_c, int cap_d, double* v_inv, double* b_l, double* h_l,
                               double* scale_l, int cap_landmarks, int32_t* imu_redo_counters, int cap_imu, int32_t* sizes3) {
  if (!h || !sizes3) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).debugBuildArrays(g_full, h_c, cap_d, v_inv, b_l, h_l, scale_l, cap_landmarks, imu_redo_counters, cap_imu, sizes3);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_trust_region_step(svin_ba* h, double mu, double radius, int form, int commit, double* scalars38, double* y_c,
                                    double* v_c, int cap_d, double* y_l, double* v_l, double* landmark_candidates,
                                    uint64_t* landmark_ids, int cap_landmarks, uint64_t* block_ids, int32_t* block_kinds,
                                    double* block_candidates, int cap_blocks, int32_t* info8) {
  if (!h || !info8) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
  Window::DebugStepOut o{scalars38, y_c, v_c, cap_d, y_l, v_l, landmark_candidates, landmark_ids, cap_landmarks,
                         block_ids, block_kinds, block_candidates, cap_blocks, info8};
  return win(h).debugTrustRegionStep(mu, radius, form, commit, o);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_get_path_counters(svin_ba* h, int64_t out[4]) try {
  if (!h || !out) return SVIN_ERR_INVALID_ARG;
  const long long* c = ro(h).pathCounters();
  for (int i = 0; i < 4; ++i) out[i] = c[i];
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_debug_landmark_handles(svin_ba* h, int32_t out[2]) try {
  if (!h || !out) return SVIN_ERR_INVALID_ARG;
  ro(h).landmarkHandles(out);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_debug_sym_eig(int n, const double* A, double* eigenvalues, double* eigenvectors, double* device_ms) {
  if (!A || !eigenvalues || !eigenvectors) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return svin::debugSymEig(n, A, eigenvalues, eigenvectors, device_ms);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_last_system(svin_ba* h, double* S, double* g, int cap_d) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).debugLastSystem(S, g, cap_d);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_solve_dense(int d, int dC, int sb_chain, int s_padded, int ld_s, const double* s_buffer, uint64_t s_buffer_doubles,
                              uint64_t s_offset, const double* g, const double* h_c, const double* scale_c, double mu, int fuse_finalize,
                              int init_scale, int scratch_fill, double* y, double* htil, int32_t* chol_fail, int32_t* info10,
                              double* s_buffer_after, double* scratch, uint64_t cap_scratch) {
  GUARD_BEGIN
  const svin::DebugDenseIn in{d, dC, sb_chain, s_padded, ld_s, s_buffer, (size_t)s_buffer_doubles, (size_t)s_offset, g, h_c, scale_c,
                              mu, fuse_finalize, init_scale, scratch_fill};
  const svin::DebugDenseOut out{y, htil, chol_fail, info10, s_buffer_after, scratch, (size_t)cap_scratch};
  return svin::debugSolveDense(in, out);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_tile_skyline(svin_ba* h, uint64_t* cut2) {
  if (!h || !cut2) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
  unsigned long long w[2];
  win(h).debugTileSkyline(w);
  cut2[0] = w[0]; cut2[1] = w[1];
  return 1;
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_tile_deal(svin_ba* h, uint64_t* deal) {
  if (!h || !deal) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN
  *deal = win(h).debugTileDeal();
  return 1;
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_solve_dense_profiled(int d, int dC, int sb_chain, int s_padded, int ld_s, const double* s_buffer, uint64_t s_buffer_doubles,
                                       uint64_t s_offset, const double* g, const double* h_c, const double* scale_c, double mu, int fuse_finalize,
                                       int init_scale, int scratch_fill, double* y, double* htil, int32_t* chol_fail, int32_t* info10,
                                       double* s_buffer_after, double* scratch, uint64_t cap_scratch, uint64_t tile_cut) {
  GUARD_BEGIN
  svin::DebugDenseIn in{d, dC, sb_chain, s_padded, ld_s, s_buffer, (size_t)s_buffer_doubles, (size_t)s_offset, g, h_c, scale_c,
                        mu, fuse_finalize, init_scale, scratch_fill};
  in.tileCut = tile_cut & ((1ull << 44) - 1);
  const svin::DebugDenseOut out{y, htil, chol_fail, info10, s_buffer_after, scratch, (size_t)cap_scratch};
  return svin::debugSolveDense(in, out);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_marginalize(int m, int Lm, const int32_t* marg_rows, int stages, const double* U, const double* ba, const double* W,
                              const double* V, const double* bb, double* U_out, double* ba_out, double* Hk, double* bk, double* J,
                              double* e0, double* Ht, double* bp, double* scal3, int32_t* flags8, int32_t* info16) {
  GUARD_BEGIN
  const svin::DebugMargIn in{m, Lm, marg_rows, stages, U, ba, W, V, bb};
  const svin::DebugMargOut out{U_out, ba_out, Hk, bk, J, e0, Ht, bp, scal3, flags8, info16};
  return svin::debugMarginalize(in, out);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_debug_set_option(const char* name, int value) { return svin::setDebugOption(name, value); }
int svin_ba_debug_get_option(const char* name, int* value) { return svin::debugOptionByName(name, value); }
int svin_ba_debug_set_switch(const char* name, int value) { return svin::setDebugOption(name, value ? 1 : 0); }
int svin_ba_debug_peek_solver_scratch(svin_ba* h, uint64_t offset, uint64_t count, double* out) {
  if (!h || !out) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).debugPeekSolverScratch(offset, count, out);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_get_prior(svin_ba* h, double* H, double* b0, double* J, double* e0, uint64_t* ids, int32_t* ord,
                      int32_t* mdim, int32_t* nb, int cap_m) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).getPrior(H, b0, J, e0, ids, ord, mdim, nb, cap_m);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_get_prior_lin(svin_ba* h, double* lin, int cap_blocks) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).getPriorLin(lin, cap_blocks);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_get_marg_pre(svin_ba* h, int32_t* m, int32_t* n_landmarks, double* U, double* ba, double* W, double* V, double* bb,
                         int32_t* marg_rows, int cap_m, int cap_landmarks) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  const auto& q = ro(h).margPre();
  if (m) *m = q.m;
  if (n_landmarks) *n_landmarks = q.Lm;
  if (q.m > cap_m || q.Lm > cap_landmarks) return 0;
  if (U) std::memcpy(U, q.U.data(), sizeof(double) * q.U.size());
  if (ba) std::memcpy(ba, q.ba.data(), sizeof(double) * q.m);
  if (W) std::memcpy(W, q.W.data(), sizeof(double) * q.W.size());
  if (V) std::memcpy(V, q.V.data(), sizeof(double) * q.V.size());
  if (bb) std::memcpy(bb, q.bb.data(), sizeof(double) * q.bb.size());
  if (marg_rows) for (size_t i = 0; i < q.margRows.size(); ++i) marg_rows[i] = q.margRows[i];
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_get_marg_pre_blocks(svin_ba* h, uint64_t* dense_ids, int32_t* dense_ord, int32_t* dense_mdim, int cap_dense, uint64_t* landmark_ids,
                                int cap_landmarks) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  const auto& q = ro(h).margPre();
  for (size_t i = 0; i < q.denseIds.size() && (int)i < cap_dense; ++i) {
    if (dense_ids) dense_ids[i] = q.denseIds[i];
    if (dense_ord) dense_ord[i] = q.denseOrd[i];
    if (dense_mdim) dense_mdim[i] = q.denseMdim[i];
  }
  for (size_t i = 0; i < q.lmIds.size() && (int)i < cap_landmarks; ++i)
    if (landmark_ids) landmark_ids[i] = q.lmIds[i];
  return (int)q.denseIds.size();
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_describe_block(svin_ba* h, uint64_t id, uint64_t* frame, int32_t* kind, int32_t* index) try {
  if (!h) return SVIN_ERR_INVALID_ARG;
  return ro(h).describeBlock(id, frame, kind, index);
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_bench_allreduce(svin_ba* h, uint64_t n_doubles, int iters, double* mean_us) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).benchAllReduce((size_t)n_doubles, iters, mean_us);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_bench_jacobian_eval(svin_ba* h, int copies, int iters, double* mean_ms, double* bytes) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).benchJacobianEval(copies, iters, mean_ms, bytes);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_residual_info(svin_ba* h, int n, const uint64_t* residual_ids, int32_t* kind, int32_t* residual_dim, int32_t* n_blocks,
                          int32_t* block_dims) {
  if (!h || n < 0 || (n > 0 && !residual_ids)) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return ro(h).residualInfo(n, residual_ids, kind, residual_dim, n_blocks, block_dims);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_map_add_parameter_block(svin_ba* h, uint64_t id, int type, const double* values) {
  if (!h || !values) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).mapAddParameterBlock(id, type, values);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_set_parameter_block(svin_ba* h, uint64_t id, const double* values) {
  if (!h || !values) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).mapSetParameterBlock(id, values);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_map_remove_parameter_block(svin_ba* h, uint64_t id) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).mapRemoveParameterBlock(id);
  GUARD_END(SVIN_ERR_DEVICE)
}
uint64_t svin_ba_map_add_pose_error(svin_ba* h, uint64_t block, const double meas[7], const double information[36]) {
  if (!h) return 0;
  GUARD_BEGIN return win(h).mapAddPoseError(block, meas, information);
  GUARD_END(0)
}
uint64_t svin_ba_map_add_speed_and_bias_error(svin_ba* h, uint64_t block, const double meas[9], const double information[81]) {
  if (!h) return 0;
  GUARD_BEGIN return win(h).mapAddSpeedAndBiasError(block, meas, information);
  GUARD_END(0)
}
uint64_t svin_ba_map_add_relative_pose_error(svin_ba* h, uint64_t block0, uint64_t block1, const double information[36]) {
  if (!h) return 0;
  GUARD_BEGIN return win(h).mapAddRelativePoseError(block0, block1, information);
  GUARD_END(0)
}
uint64_t svin_ba_map_add_imu_error(svin_ba* h, const uint64_t blocks[4], const svin_imu_sample* imu, int n_imu, const svin_imu_params* p,
                                   uint32_t t0_sec, uint32_t t0_nsec, uint32_t t1_sec, uint32_t t1_nsec) {
  if (!h || !blocks || !imu || !p || n_imu < 2) return 0;
  GUARD_BEGIN
  std::vector<uint32_t> t;
  std::vector<double> m;
  splitSamples(imu, n_imu, t, m);
  TimeStamp a, b;
  a.sec = t0_sec; a.nsec = t0_nsec; b.sec = t1_sec; b.nsec = t1_nsec;
  return win(h).mapAddImuError(blocks, t.data(), m.data(), n_imu, toParams(p), a, b);
  GUARD_END(0)
}
uint64_t svin_ba_map_add_sonar_error(svin_ba* h, uint64_t pose_block, double range, double heading, double information,
                                     const double* patch_xyz, int n_patch) {
  if (!h) return 0;
  GUARD_BEGIN return win(h).mapAddSonarError(pose_block, range, heading, information, patch_xyz, n_patch);
  GUARD_END(0)
}
uint64_t svin_ba_map_add_depth_error(svin_ba* h, uint64_t pose_block, double depth, double information, double first_depth) {
  if (!h) return 0;
  GUARD_BEGIN return win(h).mapAddDepthError(pose_block, depth, information, first_depth);
  GUARD_END(0)
}
uint64_t svin_ba_map_add_host_residual(svin_ba* h, const uint64_t* block_ids, int n_blocks, int residual_dim, svin_cost_function fn, void* user) {
  if (!h) return 0;
  GUARD_BEGIN return win(h).mapAddHostResidual(block_ids, n_blocks, residual_dim, fn, user);
  GUARD_END(0)
}
uint64_t svin_ba_map_add_reprojection_error(svin_ba* h, uint64_t pose_block, uint64_t landmark, uint64_t extrinsics_block, uint64_t cam,
                                            const double uv[2], const double information[4]) {
  if (!h) return 0;
  GUARD_BEGIN return win(h).mapAddReprojectionError(pose_block, landmark, extrinsics_block, cam, uv, information);
  GUARD_END(0)
}
int svin_ba_map_remove_residual_block(svin_ba* h, uint64_t rid) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).mapRemoveResidualBlock(rid);
  GUARD_END(SVIN_ERR_DEVICE)
}
static int lossCode(int r) {
  return r == 1 ? 1 : (r == -2 ? SVIN_ERR_NOT_FOUND : (r == -3 ? SVIN_ERR_UNSUPPORTED : SVIN_ERR_INVALID_ARG));
}
int svin_ba_map_set_residual_loss(svin_ba* h, uint64_t rid, int kind, double scale) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return lossCode(win(h).setResidualLoss(rid, kind, scale));
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_map_get_residual_loss(svin_ba* h, uint64_t rid, int* kind, double* scale) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return lossCode(ro(h).getResidualLoss(rid, kind, scale));
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_map_set_reprojection_information(svin_ba* h, uint64_t rid, const double information[4]) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).setReprojectionInformation(rid, information);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_map_get_reprojection_information(svin_ba* h, uint64_t rid, double information[4]) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return ro(h).getReprojectionInformation(rid, information);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_get_lhs(svin_ba* h, uint64_t block_id, double* H, int cap) {
  if (!h || (!H && cap > 0)) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return h->w.getLhs(block_id, H, cap);
  GUARD_END(SVIN_ERR_DEVICE)
}
int64_t svin_ba_get_lhs_blocks(svin_ba* h, int n, const uint64_t* block_ids, int32_t* dims, double* H, int64_t cap_doubles) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return h->w.getLhsBlocks(n, block_ids, dims, H, cap_doubles);
  GUARD_END(SVIN_ERR_DEVICE)
}
int64_t svin_ba_get_lhs_pass_count(svin_ba* h) try { return h ? ro(h).lhsPassCount() : SVIN_ERR_INVALID_ARG; } CATCH_ALL(SVIN_ERR_DEVICE)
// (like get_lhs: straight to the window, so that neither query drops what the other keeps)
int svin_ba_get_covariance(svin_ba* h, uint64_t block_a, uint64_t block_b, double* cov, int cap) {
  if (!h || !cov || cap < 0) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return (int)h->w.getCovarianceBlocks(1, &block_a, &block_b, nullptr, nullptr, cov, cap);
  GUARD_END(SVIN_ERR_DEVICE)
}
int64_t svin_ba_get_covariance_blocks(svin_ba* h, int n_pairs, const uint64_t* blocks_a, const uint64_t* blocks_b, int32_t* dims_a,
                                      int32_t* dims_b, double* cov, int64_t cap_doubles) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return h->w.getCovarianceBlocks(n_pairs, blocks_a, blocks_b, dims_a, dims_b, cov, cap_doubles);
  GUARD_END(SVIN_ERR_DEVICE)
}
int64_t svin_ba_get_covariance_pass_count(svin_ba* h) try { return h ? ro(h).covariancePassCount() : SVIN_ERR_INVALID_ARG; } CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_set_pack_mode(svin_ba* h, int mode) try {
  if (!h || mode < 0 || mode > 1) return SVIN_ERR_INVALID_ARG;
  win(h).setPackMode(mode);
  return 1;
} CATCH_ALL(SVIN_ERR_DEVICE)
int svin_ba_debug_csr(svin_ba* h, int32_t* n_landmarks, int32_t* n_observations, int32_t* lm_ptr, int32_t* obs_lm, uint32_t* obs_idx,
                      double* uv, double* w, double* lm, int32_t* obs_order, int32_t* resident) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).debugCsr(n_landmarks, n_observations, lm_ptr, obs_lm, obs_idx, uv, w, lm, obs_order, resident);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_bench_jacobian_eval_b2b(svin_ba* h, int copies, int iters, double* mean_ms, double* b2b_ms, double* bytes) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).benchJacobianEval(copies, iters, mean_ms, bytes, b2b_ms);
  GUARD_END(SVIN_ERR_DEVICE)
}
int svin_ba_bench_kernel_times(svin_ba* h, int iters, double* e, double* b, double* s) {
  if (!h) return SVIN_ERR_INVALID_ARG;
  GUARD_BEGIN return win(h).benchKernelTimes(iters, e, b, s);
  GUARD_END(SVIN_ERR_DEVICE)
}

}  // extern "C"
