// svin_amd: what one pass of Window::solve's inner loop enqueues, decided before anything is enqueued (IterationPass), and the one
// fact those decisions rest on besides the trust region's own state: what the normal-equation accumulators S / gRed / hC hold
// (AccumulatorLedger).  They are zero (pack(), or the post-solve pass behind a reduced solve), or hold exactly one build -- of a
// point, with a damping and a metric -- or hold something no solve can use.  A build is launched, and zeroes the accumulators
// first, by that fact alone; a wrong answer would not crash, it would sum two builds.
// HIP-free (tests/test_iteration_plan_host.py drives the ledger, the pass and the real TrustRegionHost through every sequence of
// events of six passes on the CPU, through tests/csrc/iteration_plan_shim.cpp, and holds the launches against a model of the
// accumulators that knows nothing of the ledger).  Inline, on the stack, no allocation: the host has some 7 us between the
// mailbox record and the first launch of the next iteration.
#pragma once
#include <stdexcept>
#include "batch_plan.hpp"     // kBatchFull / kBatchReuse / kBatchEval
#include "build_plan.hpp"     // StepMode, specBuildWanted
#include "trust_region.hpp"   // TrustRegionHost

namespace svin {

// how a pass ended (Window::finishPass): the factorisation failed and the iteration is tried again with more damping; the solve
// is over; or the iteration's outcome
enum PassEnd : int { kPassRetry = 0, kPassTerminated = 1, kPassAccepted = 2, kPassRejected = 3, kPassInvalid = 4 };

struct BuildNeed { bool launch, zeroFirst; };   // the build in front of a reduced solve

struct AccumulatorLedger {
  enum Contents : int { kZero = 0, kBuild = 1, kStale = 2 };
  Contents contents = kZero;
  double mu = 0;                                  // kBuild: the damping, the metric (Jacobi scaling initialised by this build),
  bool initScale = false, onCandidate = false;    // and the state set it stands on: the current one, or the candidate's
  bool pending = false;   // a speculative build is enqueued and not yet counted as kept or discarded
  int hits = 0, misses = 0;

  // the build (mu, initScale = true) of the current point was enqueued behind the initial evaluation, into pack()'s zeros
  void firstEnqueued(double mu_) { hold(mu_, true, false); }
  // The build in front of the reduced solve with (mu, initScale) at the current point.  What is held is kept exactly when it is
  // that build; anything else is launched over, zeroing first unless the accumulators are zero.  A pending speculative build is
  // counted here: a hit when it is the one kept.
  BuildNeed need(double mu_, bool initScale_) {
    const bool kept = contents == kBuild && !onCandidate && mu == mu_ && initScale == initScale_;
    if (pending) { ++(kept ? hits : misses); pending = false; }
    const BuildNeed n{!kept, !kept && contents != kZero};
    hold(mu_, initScale_, false);
    return n;
  }
  void postSolveDone() { contents = kZero; }   // the post-solve pass has cleared the accumulators
  // build_plan.hpp specBuildWanted (the predicate stepInEvalTaken is asked with), the cleanliness read here
  bool specWanted(bool speculate, int iteration, int numIter) const { return specBuildWanted(speculate, contents == kZero, iteration, numIter); }
  // the build of the candidate with the damping an accepted step leaves (initScale = false) is in the accumulators
  void specEnqueued(double mu_) { hold(mu_, false, true); pending = true; }
  // an accepted step swaps the candidate's sets in: a build on them stands on the current point.  Any other end but the solve's
  // leaves that build behind (a retry's and an invalid step's damping differ from what it assumed; a rejected step's point does).
  void end(PassEnd e) {
    if (contents != kBuild || !onCandidate || e == kPassTerminated) return;
    if (e == kPassAccepted) onCandidate = false;
    else contents = kStale;
  }
  // the loop is over: whatever is still pending -- a termination, a rejected step on the last iteration -- was built for nothing
  void close() { if (pending) { ++misses; pending = false; } }

 private:
  void hold(double mu_, bool initScale_, bool onCandidate_) { contents = kBuild; mu = mu_; initScale = initScale_; onCandidate = onCandidate_; }
};

// One pass of the inner loop of Window::solve, in the order it is enqueued.
struct IterationPass {
  bool solve;              // a fresh linearisation: [build,] [pack + all-reduce + unpack of the system,] reduced solve, post-solve pass
  BuildNeed build;         // ... launchAccumulateNormalEquations(tr.mu, tr.initScale) in front of it
  bool allReduceSystem;    // ... sharded: the system travels between the build and the solve
  double prepareRadius;    // ... launchDoglegPrepare's radius: the pass takes the step itself (fused), or -1
  bool stepInEval;         // ... the pass ends at its partials, k_eval_build takes the step at the head of its blocks
  int lmDeferredPost;      // PassArgs::lmDeferred (kernels.hpp) for the post-solve pass
  bool doglegStep;         // launchDoglegStep: a re-used linearisation, or a step that is not fused
  int lmDeferredEval;      // PassArgs::lmDeferred for the candidate evaluation
  bool specWanted;         // a speculative build behind the candidate evaluation, with damping specMu,
  double specMu;
  bool specInEval;         // asked of evaluateAll (k_eval_build) -- otherwise, and where evaluateAll declines, a launch of its own
};
// stepInEvalTaken_: build_plan.hpp stepInEvalTaken's answer for this pass (asked only where the step is fused with the landmarks
// deferred and the evaluation may take a build along).  Moves the ledger over the build and the post-solve pass of the plan;
// the speculative build is the caller's to report (specEnqueued) once it is enqueued.
inline IterationPass planPass(const StepMode& sm, bool dist, bool evalBuild, bool speculate, const TrustRegionHost& tr, int numIter,
                              bool stepInEvalTaken_, AccumulatorLedger& ledger) {
  IterationPass q{};
  q.solve = !tr.reuse;
  q.prepareRadius = -1.0;
  if (q.solve) {
    q.build = ledger.need(tr.mu, tr.initScale);
    q.allReduceSystem = dist;
    if (sm.fuseStep) q.prepareRadius = tr.stepRadius();
    q.stepInEval = stepInEvalTaken_;
    q.lmDeferredPost = sm.deferLm ? 1 : 0;
    ledger.postSolveDone();
  }
  q.doglegStep = tr.reuse || !sm.fuseStep;
  q.lmDeferredEval = (sm.deferLm && !tr.reuse) ? 1 : 0;
  q.specWanted = ledger.specWanted(speculate, tr.iteration, numIter);
  if (q.specWanted) q.specMu = tr.muAfterAccept();
  q.specInEval = q.specWanted && evalBuild;
  return q;
}

// A window of a batched solve (Window::solveBatchGroup) plans its pass like any other -- one GPU, no speculation, no k_eval_build, a
// ledger of its own -- and the round's stages (batch_plan.hpp, BatchSlot::stages) are that pass: the initial evaluation (!cand, no
// pass) is kBatchEval alone.  A round has no launch for a zeroing build, a kept build, a system all-reduce, a speculative build or a
// step that is not the fused one.
inline int batchStagesOf(const IterationPass& q, bool cand) {
  if (!cand) return kBatchEval;
  const bool full = q.solve && q.build.launch && !q.build.zeroFirst && !q.allReduceSystem && !q.stepInEval && q.prepareRadius > 0.0 && !q.doglegStep;
  const bool reuse = !q.solve && q.doglegStep;
  if (!(full || reuse) || q.specWanted) throw std::logic_error("batchStagesOf: a pass a batched round has no launches for");
  return (full ? kBatchFull : kBatchReuse) | kBatchEval;
}

}  // namespace svin
