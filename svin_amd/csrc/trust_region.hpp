// Host side of the trust-region iteration: every DECISION Window::solve takes, as a HIP-free state machine.
//
// Ceres 2.2 TrustRegionMinimizer + DoglegStrategy(TRADITIONAL_DOGLEG) semantics with the options Estimator::optimize sets
// (okvis_ceres/src/Estimator.cpp:878-890): monotonic steps, min_relative_decrease 1e-3, initial radius 1e4, the mu retry
// ladder of the dogleg strategy (min_mu 1e-8, max_mu 1, x10), five consecutive invalid steps = failure.  All numbers the
// decisions read come from ONE record per evaluation (SolverScalars); in the landmark-sharded mode every field read here is
// either all-reduced or computed redundantly from all-reduced data, so the ranks take identical decisions
// (tests/test_trust_region_host.py feeds two instances the same reduced fields and different rank-local ones).
// A second strategy, Ceres 2.2's LevenbergMarquardtStrategy, is a choice of the same state machine (configure()): the damping is
// 1 / radius, the step is the Gauss-Newton step of the damped system (the driver hands the device an infinite step radius, so
// doglegCoefficients takes its first branch: delta = -y, jdSq = jySq, jdDotR = -jyDotR), a rejected or invalid step divides the
// radius by a factor that doubles, and every such step is followed by a new build at the same point under the new damping.
// Included by window.cpp (the driver: launches + read-back) and by tests/csrc/trust_region_shim.cpp and
// tests/csrc/trust_region_lm_shim.cpp (g++, no GPU).
#pragma once
#include <algorithm>
#include <cmath>

// (as in dmath.hpp: the device functions of this header are the ones the kernels call, and g++ compiles them for the CPU tests)
#ifndef SVIN_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SVIN_HD __host__ __device__ __forceinline__
#else
#define SVIN_HD inline
#endif
#endif

namespace svin {

// Coefficients of the traditional dogleg step (ceres dogleg_strategy.cc) on the un-scaled vectors, delta = cg v + cn (-y), from
// group B of SolverScalars and the radius; |J delta|^2 and (J delta).r follow from group B by linearity.  Called by k_post_solve
// (fused step) and k_step_retract (kernels.hip); tests/test_dogleg_host.py holds it against mpmath through the shim.
struct DoglegCoeff { double cg, cn, stepNorm, jdSq, jdDotR; };
SVIN_HD DoglegCoeff doglegCoefficients(double gHatSq, double jgSq, double gnHatSq, double gDotGn,
                                       double jySq, double jvDotJy, double jvDotR, double jyDotR, double radius) {
  const double gnorm = sqrt(gHatSq), gnnorm = sqrt(gnHatSq);
  const double alpha = gHatSq / jgSq;
  DoglegCoeff c;
  if (gnnorm <= radius) { c.cg = 0; c.cn = 1; c.stepNorm = gnnorm; }
  else if (gnorm * alpha >= radius) { c.cg = -(radius / gnorm); c.cn = 0; c.stepNorm = radius; }
  else {
    const double b_dot_a = -alpha * gDotGn;
    const double a_sq = (alpha * gnorm) * (alpha * gnorm);
    const double b_minus_a_sq = a_sq - 2 * b_dot_a + gnnorm * gnnorm;
    const double cc = b_dot_a - a_sq;
    const double dd = sqrt(cc * cc + b_minus_a_sq * (radius * radius - a_sq));
    const double beta = (cc <= 0) ? (dd - cc) / b_minus_a_sq : (radius * radius - a_sq) / (dd + cc);
    c.cg = -alpha * (1.0 - beta);
    c.cn = beta;
    c.stepNorm = sqrt(fmax(c.cg * c.cg * gHatSq + 2 * c.cg * c.cn * gDotGn + c.cn * c.cn * gnHatSq, 0.0));
  }
  c.jdSq = c.cg * c.cg * jgSq - 2.0 * c.cg * c.cn * jvDotJy + c.cn * c.cn * jySq;
  c.jdDotR = c.cg * jvDotR - c.cn * jyDotR;
  return c;
}

// the fields of SolverScalars the host reads (kernels.hpp); rank-invariant in sharded mode
struct TrScalars {
  double cost = 0;            // group A (summed over ranks)
  double stepNormSq = 0, xNormSq = 0;
  double gradMax = 0;         // max over the ranks' gathered values
  double failMax = 0;         // != 0: the reduced system or a landmark block was not positive definite, on some rank
  double jdSq = 0, jdDotR = 0, doglegStepNorm = 0;   // derived on every rank from all-reduced sums and the radius
};

struct TrustRegionHost {
  // options
  double fTol = 1e-6, gTol = 1e-10, pTol = 1e-8;
  int maxIterations = 10;
  enum Strategy { kDogleg = 0, kLevenbergMarquardt = 1 };
  int strategy = kDogleg;
  double initialRadius = 1e4, maxRadius = 1e16;   // (ceres: initial_trust_region_radius, max_trust_region_radius; both strategies)
  // state
  double radius = 1e4, mu = 1e-8, x_cost = 0;
  double decreaseFactor = 2.0;   // Levenberg-Marquardt: what the next rejected or invalid step divides the radius by
  bool reuse = false, initScale = true;
  int invalid = 0, iteration = 0, successful = 0;
  int termination = 1;   // 0 convergence, 1 max iterations, 2 time limit (callback), 3 failure
  bool stepOk = true;
  static constexpr double kMinMu = 1e-8, kMaxMu = 1.0, kMuIncrease = 10.0;

  // strategy and radii, before start(); an object that is never configured is the dogleg solve with ceres' default radii
  void configure(int strategy_, double initialRadius_, double maxRadius_) {
    strategy = strategy_; initialRadius = initialRadius_; maxRadius = maxRadius_;
    radius = initialRadius;
    if (lm()) mu = 1.0 / radius;
  }
  bool lm() const { return strategy == kLevenbergMarquardt; }
  // the radius the device takes its step in: Levenberg-Marquardt's step is the whole Gauss-Newton step of the damped system
  double stepRadius() const { return lm() ? HUGE_VAL : radius; }
  // LevenbergMarquardtStrategy::StepAccepted: radius / max(1/3, 1 - (2 rho - 1)^3), at most maxRadius
  double lmAcceptedRadius(double shrink) const { return std::min(maxRadius, radius / std::max(1.0 / 3.0, shrink)); }
  void start(double initialCost) { x_cost = initialCost; }
  // top of an iteration: false = the loop ends here with `termination` set (stopRequested: the time-limit callback)
  bool beginIteration(bool stopRequested) {
    if (stopRequested) { termination = 2; return false; }
    if (iteration >= maxIterations) { termination = 1; return false; }
    if (radius <= 1e-32) { termination = 0; return false; }
    ++iteration;
    stepOk = true;
    return true;
  }
  // damping an accepted step would leave behind (what the speculative build of the next iteration assumes)
  // (Levenberg-Marquardt: of a step accepted with the 1/3 clamp active -- rho above 0.937, what a converging solve mostly sees;
  // the expression is endIteration()'s own, so the driver's test `specMu == mu` holds exactly when the clamp was active)
  double muAfterAccept() const {
    if (lm()) return 1.0 / lmAcceptedRadius(0.0);
    return std::max(kMinMu, 2.0 * mu / kMuIncrease);
  }
  // after the candidate evaluation of a FRESH linearisation: true = the factorisation failed and the same iteration is
  // retried with a larger mu (DoglegStrategy::ComputeStep's retry ladder); false = go on to endIteration()
  // Levenberg-Marquardt has no ladder: a failed factorisation is an invalid step (the radius shrinks, endIteration())
  bool retryFactorisation(const TrScalars& sc) {
    if (reuse || sc.failMax == 0.0) return false;
    if (lm()) { stepOk = false; return false; }
    mu *= kMuIncrease;
    if (mu < kMaxMu) return true;
    stepOk = false;
    return false;
  }
  enum Outcome { kAccepted, kRejected, kInvalid, kTerminated };
  // the decision of the iteration; kTerminated: `termination` is set
  Outcome endIteration(const TrScalars& sc) {
    if (!reuse) { initScale = false; reuse = true; }
    if (sc.gradMax <= gTol) { --iteration; termination = 0; return kTerminated; }
    const double model_cost_change = -(sc.jdDotR + 0.5 * sc.jdSq);
    if (!stepOk || !(model_cost_change > 0.0)) {
      if (++invalid >= 5) { termination = 3; return kTerminated; }
      if (lm()) { lmShrink(); return kInvalid; }
      mu *= kMuIncrease;
      reuse = false;
      return kInvalid;
    }
    invalid = 0;
    const double step_norm = std::sqrt(sc.stepNormSq), x_norm = std::sqrt(sc.xNormSq);
    if (step_norm <= pTol * (x_norm + pTol)) { termination = 0; return kTerminated; }
    const double candidate_cost = sc.cost;
    const double cost_change = x_cost - candidate_cost;
    if (std::fabs(cost_change) <= fTol * x_cost) { termination = 0; return kTerminated; }
    relative_decrease = cost_change / model_cost_change;
    last_step_norm = step_norm;
    if (relative_decrease > 1e-3) {
      x_cost = candidate_cost;
      ++successful;
      if (lm()) {
        radius = lmAcceptedRadius(1.0 - std::pow(2.0 * relative_decrease - 1.0, 3));
        decreaseFactor = 2.0;
        mu = 1.0 / radius;
        reuse = false;
        return kAccepted;
      }
      if (relative_decrease < 0.25) radius *= 0.5;
      if (relative_decrease > 0.75) radius = std::max(radius, 3.0 * sc.doglegStepNorm);
      radius = std::min(radius, maxRadius);
      mu = muAfterAccept();
      reuse = false;
      return kAccepted;
    }
    if (lm()) { lmShrink(); return kRejected; }
    radius *= 0.5;
    reuse = true;
    return kRejected;
  }
  double relative_decrease = 0, last_step_norm = 0;   // of the last accepted / rejected step (progress output)
  // one row of the iteration log (svin_ba_get_iteration_log) for the iteration endIteration() has just decided with outcome o
  // (not kTerminated), muUsed = mu as it stood before that call: cost held, relative decrease, radius after, step norm, mu, outcome
  void logRow(double muUsed, Outcome o, double row[6]) const {
    row[0] = x_cost; row[1] = o == kInvalid ? 0.0 : relative_decrease; row[2] = radius; row[3] = o == kInvalid ? 0.0 : last_step_norm;
    row[4] = muUsed; row[5] = (double)(int)o;
  }

 private:
  // LevenbergMarquardtStrategy::StepRejected / StepIsInvalid; the same linearisation is solved again under the new damping
  void lmShrink() {
    radius /= decreaseFactor;
    decreaseFactor *= 2.0;
    mu = 1.0 / radius;
    reuse = false;
  }
};

}  // namespace svin
