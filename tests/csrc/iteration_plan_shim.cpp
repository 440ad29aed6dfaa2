// C entry points over svin_amd/csrc/iteration_plan.hpp for tests/test_iteration_plan_host.py: the loop of Window::solve with the
// launches left out.  ip_run drives AccumulatorLedger, planPass and the real TrustRegionHost through one scripted sequence of
// per-pass events, in the order solve() calls them, and writes down what every pass would have enqueued; ip_run_all does so for
// every sequence of a given length.  The test interprets those rows; nothing here judges them.
//
// cfg: strategy (0 dogleg, 1 Levenberg-Marquardt), SVIN_NO_SPECULATION, SVIN_NO_EVAL_BUILD, mode (0 one GPU, 1 sharded with the
//      native all-reduce, 2 sharded with the callback, 3 a window of a batched solve: Window::solveBatchGroup's loop, which plans
//      without speculation and k_eval_build whatever the switches say and enqueues no build behind the initial evaluation),
//      numIter, what stepInEvalTaken answers for the window's sizes
// events, one per pass: 0 the factorisation fails, 1 a step accepted at the 1/3 clamp (it leaves the damping a speculative build
//      assumes), 2 a step accepted with rho = 0.5 (Levenberg-Marquardt: another damping), 3 rejected, 4 invalid, 5 gradient below tolerance
// a row, kIpFields doubles: see the enum
#include <cstdint>
#include "../../svin_amd/csrc/iteration_plan.hpp"

namespace {
using namespace svin;
enum { kAlive, kReuse, kMu, kInitScale, kIteration, kSolve, kLaunch, kZeroFirst, kAllReduceSystem, kPrepareRadius, kStepInEval, kLmDeferredPost,
       kDoglegStep, kLmDeferredEval, kSpecWanted, kSpecMu, kSpecInEval, kSpecFused, kEnd, kHitsIfClosed, kMissesIfClosed, kStepRadius,
       kBatchStages /* mode 3: batchStagesOf(pass, cand = true), -1 where it throws */, kIpFields };
constexpr int kIpEvents = 6;

TrScalars scalarsOf(int event, const TrustRegionHost& tr) {
  TrScalars t;   // model cost change 1, rho 1
  t.cost = tr.x_cost - 1.0; t.stepNormSq = 1.0; t.xNormSq = 1.0; t.gradMax = 1.0; t.failMax = 0.0;
  t.jdSq = 1.0; t.jdDotR = -1.5; t.doglegStepNorm = 1.0;
  if (event == 0) t.failMax = 1.0;
  if (event == 2) t.cost = tr.x_cost - 0.5;
  if (event == 3) t.cost = tr.x_cost + 1.0;
  if (event == 4) t.jdDotR = 1.0;
  if (event == 5) t.gradMax = 0.0;
  return t;
}

// Window::finishPass without the window
PassEnd finishPass(TrustRegionHost& tr, const TrScalars& t) {
  if (tr.retryFactorisation(t)) return kPassRetry;
  const TrustRegionHost::Outcome o = tr.endIteration(t);
  if (o == TrustRegionHost::kTerminated) return kPassTerminated;
  return o == TrustRegionHost::kAccepted ? kPassAccepted : o == TrustRegionHost::kRejected ? kPassRejected : kPassInvalid;
}

int batchStagesOrMinusOne(const IterationPass& pass, bool cand) {
  try { return batchStagesOf(pass, cand); } catch (const std::logic_error&) { return -1; }
}

// Window::solve; rows: nPass x kIpFields, zeroed by the caller.  Returns the passes run.
int run(const int32_t* cfg, const int32_t* events, int nPass, double* rows) {
  const bool batched = cfg[3] == 3;
  const bool lm = cfg[0] != 0, noSpeculation = cfg[1] != 0 || batched, noEvalBuild = cfg[2] != 0, dist = cfg[3] == 1 || cfg[3] == 2, distNative = cfg[3] == 1;
  const int numIter = cfg[4];
  const bool headFits = cfg[5] != 0;
  const StepMode stepMode = stepModeOf(StepDims{10, 2, 10, 100, 1000, true}, StepSwitches{false, false, false}, dist);
  TrustRegionHost tr;
  if (lm) tr.configure(TrustRegionHost::kLevenbergMarquardt, 1e4, 1e16);
  const bool evalBuild = !dist && !noSpeculation;
  AccumulatorLedger ledger;
  if (!dist && !batched && numIter > 0) ledger.firstEnqueued(tr.mu);
  tr.maxIterations = numIter;
  tr.start(100.0);
  const bool speculate = !noSpeculation && (!dist || distNative);
  int k = 0;
  while (k < nPass) {
    if (!tr.beginIteration(false)) break;
    PassEnd end;
    do {
      if (k >= nPass) return k;
      double* r = rows + (size_t)k * kIpFields;
      r[kAlive] = 1; r[kReuse] = tr.reuse; r[kMu] = tr.mu; r[kInitScale] = tr.initScale; r[kIteration] = tr.iteration; r[kStepRadius] = tr.stepRadius();
      const bool stepInEval = !tr.reuse && stepMode.fuseStep && stepMode.deferLm && evalBuild && headFits &&
                              specBuildWanted(speculate, true, tr.iteration, numIter);
      const IterationPass pass = planPass(stepMode, dist, evalBuild, speculate, tr, numIter, stepInEval, ledger);
      r[kSolve] = pass.solve; r[kLaunch] = pass.build.launch; r[kZeroFirst] = pass.build.zeroFirst; r[kAllReduceSystem] = pass.allReduceSystem;
      r[kPrepareRadius] = pass.prepareRadius; r[kStepInEval] = pass.stepInEval; r[kLmDeferredPost] = pass.lmDeferredPost;
      r[kDoglegStep] = pass.doglegStep; r[kLmDeferredEval] = pass.lmDeferredEval; r[kSpecWanted] = pass.specWanted; r[kSpecMu] = pass.specMu;
      r[kSpecInEval] = pass.specInEval;
      r[kSpecFused] = pass.specInEval && !noEvalBuild;   // evaluateAll's answer
      if (batched) r[kBatchStages] = batchStagesOrMinusOne(pass, true);
      if (pass.specWanted) ledger.specEnqueued(pass.specMu);
      end = finishPass(tr, scalarsOf(events[k], tr));
      ledger.end(end);
      r[kEnd] = end;
      AccumulatorLedger closed = ledger;   // had the solve ended here
      closed.close();
      r[kHitsIfClosed] = closed.hits; r[kMissesIfClosed] = closed.misses;
      ++k;
    } while (end == kPassRetry);
    if (end == kPassTerminated) break;
  }
  return k;
}
}  // namespace

extern "C" {
int ip_fields() { return kIpFields; }
int ip_run(const int32_t* cfg, const int32_t* events, int nPass, double* rows) { return run(cfg, events, nPass, rows); }
// every sequence of nPass events, the last event fastest: rows of sequence q at rows + q * nPass * kIpFields
void ip_run_all(const int32_t* cfg, int nPass, double* rows) {
  if (nPass < 0 || nPass > 8) return;
  long long n = 1;
  for (int k = 0; k < nPass; ++k) n *= kIpEvents;
  for (long long q = 0; q < n; ++q) {
    int32_t events[8];
    long long v = q;
    for (int k = nPass - 1; k >= 0; --k) { events[k] = (int32_t)(v % kIpEvents); v /= kIpEvents; }
    run(cfg, events, nPass, rows + (size_t)q * (size_t)nPass * kIpFields);
  }
}
// batchStagesOf on a pass put together by hand.  f: solve, build.launch, build.zeroFirst, allReduceSystem, stepInEval, doglegStep,
// specWanted; -1 where it throws
int ip_batch_stages(const int32_t* f, double prepareRadius, int cand) {
  IterationPass q{};
  q.solve = f[0] != 0; q.build = BuildNeed{f[1] != 0, f[2] != 0}; q.allReduceSystem = f[3] != 0; q.stepInEval = f[4] != 0; q.doglegStep = f[5] != 0;
  q.specWanted = f[6] != 0; q.prepareRadius = prepareRadius;
  return batchStagesOrMinusOne(q, cand != 0);
}
// The speculative builds a solve on one GPU kept and discarded, from its iteration log (n rows of 6: TrustRegionHost::logRow) -- for
// tests/test_gpu_solve_loop.py, which holds SVIN_SPEC_BUILD_HITS / _MISSES against it.  The trust region's state in front of every
// pass is put together from the rows (radius after, mu used, outcome); an iteration whose mu used lies above the damping it started
// with walked the retry ladder, one pass per factor of ten.  terminatedPass: the solve ended inside a pass that has no row.
// cfg as ip_run's (mode 0); out: hits, misses, passes
void ip_replay(const int32_t* cfg, double initialRadius, double maxRadius, int n, const double* log, int terminatedPass, int32_t* out) {
  const bool lm = cfg[0] != 0, noSpeculation = cfg[1] != 0;
  const int numIter = cfg[4];
  const StepMode stepMode = stepModeOf(StepDims{10, 2, 10, 100, 1000, true}, StepSwitches{false, false, false}, false);
  TrustRegionHost tr;
  tr.configure(lm ? TrustRegionHost::kLevenbergMarquardt : TrustRegionHost::kDogleg, initialRadius, maxRadius);
  AccumulatorLedger ledger;
  if (numIter > 0) ledger.firstEnqueued(tr.mu);
  int passes = 0;
  auto pass = [&](PassEnd end) {
    const IterationPass q = planPass(stepMode, false, !noSpeculation, !noSpeculation, tr, numIter, false, ledger);
    if (q.specWanted) ledger.specEnqueued(q.specMu);
    ledger.end(end);
    ++passes;
  };
  for (int i = 0; i < n + (terminatedPass ? 1 : 0); ++i) {
    ++tr.iteration;
    if (i == n) { pass(kPassTerminated); break; }
    const double* row = log + 6 * i;
    const int outcome = (int)row[5];
    if (!lm && !tr.reuse)
      for (; tr.mu < 0.5 * row[4]; tr.mu *= TrustRegionHost::kMuIncrease) pass(kPassRetry);
    pass(outcome == TrustRegionHost::kAccepted ? kPassAccepted : outcome == TrustRegionHost::kRejected ? kPassRejected : kPassInvalid);
    tr.initScale = false;
    if (outcome == TrustRegionHost::kAccepted && !lm) tr.mu = tr.muAfterAccept();
    if (outcome == TrustRegionHost::kInvalid && !lm) tr.mu *= TrustRegionHost::kMuIncrease;
    tr.radius = row[2];
    if (lm) tr.mu = 1.0 / tr.radius;
    tr.reuse = !lm && outcome == TrustRegionHost::kRejected;   // (dogleg: the linearisation of a rejected step is used again)
  }
  ledger.close();
  out[0] = ledger.hits; out[1] = ledger.misses; out[2] = passes;
}
// one question to a ledger in a given state.  state: contents, initScale, onCandidate, pending; out: launch, zeroFirst, hits, misses
void ip_need(const int32_t* state, double heldMu, double mu, int initScale, int32_t* out) {
  AccumulatorLedger l;
  l.contents = (AccumulatorLedger::Contents)state[0]; l.mu = heldMu; l.initScale = state[1] != 0; l.onCandidate = state[2] != 0; l.pending = state[3] != 0;
  const BuildNeed n = l.need(mu, initScale != 0);
  out[0] = n.launch; out[1] = n.zeroFirst; out[2] = l.hits; out[3] = l.misses;
}
// today's predicate through the ledger: contents -> specWanted(speculate, iteration, numIter)
int ip_spec_wanted(int contents, int speculate, int iteration, int numIter) {
  AccumulatorLedger l;
  l.contents = (AccumulatorLedger::Contents)contents;
  return l.specWanted(speculate != 0, iteration, numIter) ? 1 : 0;
}
}
