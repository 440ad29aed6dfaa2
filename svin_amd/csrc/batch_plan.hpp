// Host-side planning of a batched solve (svin_ba_solve_prepared_batch), HIP-free: which windows may share a launch sequence,
// how many blocks of every launch belong to each of them, and how a group is dealt to the lanes.
//
// What ties a window to its partners is what the launcher derives ONCE per launch: the kernel variant, the LDS sizes and the
// uniform kernel arguments -- all functions of the reduced system, the factor list, the prior and the cameras (BatchGroupFields).
// The number of landmarks and of observations only decides how many blocks a launch has, and that is a per-window quantity
// (BatchExtents): the grid of a lane's launch is the largest extent among its windows, a block at or beyond its own window's
// extent leaves at once, and everything a kernel used to read from gridDim.x it reads from the extent.  The grid expressions
// below are the ones the single-window launchers use (kernels.hip calls these functions too), so a window's blocks have the
// roles, and its partial sums the indices and the order, that they have when the window runs alone.
// Included by kernels.hpp / window.cpp and by tests/csrc/batch_plan_shim.cpp (g++, no GPU).
#pragma once
#include <algorithm>
#include <vector>

namespace svin {

// ---- grid expressions shared with the single-window launchers
// launchAccumulateNormalEquations, dense form: one block per slab, one per small factor, the prior's blocks
inline int denseSlabCount(int L) { return std::max(1, std::min(256, (L + 15) / 16)); }
inline int priorAccBlockCount(int priorM, bool ownsCamera) { return (priorM > 0 && ownsCamera) ? (priorM * priorM + 255) / 256 : 0; }
// launchDoglegPrepare: landmark blocks (16 landmarks each, grid-strided beyond 1024), factor blocks (4 factors each), one tail block
inline int postLmBlockCount(int L, int N) { return (L > 0 && N > 0) ? std::min((L + 15) / 16, 1024) : 0; }
inline int postFacBlockCount(int F) { return F > 0 ? std::min((F + 3) / 4, 1024) : 0; }
// launchDoglegStep: one thread per parameter block and landmark
inline int stepBlockCount(int nPose, int nExt, int nSb, int L) { return (nPose + nExt + nSb + L + 255) / 256; }
// launchEvalAll: 256 observations per reprojection block, one block per small factor, one for the prior
inline int evalReprojBlockCount(int N) { return (N + 255) / 256; }
inline int evalPriorBlockCount(int priorM) { return priorM > 0 ? 1 : 0; }

// the integers of a window the extents are computed from
struct BatchDims { int L, N, F, nPose, nExt, nSb, priorM, ownsCamera, nSlabs; };

// The blocks of every launch of a round that belong to ONE window (launchBatchRound).  Plain ints: part of the slot table.
struct BatchExtents {
  int buildSlabs, buildFac, buildPri;   // k_schur_dense: [slab blocks | factor blocks | prior blocks]
  int postLm, postFac;                  // k_post_solve: [landmark blocks | factor blocks | tail block]
  int step;                             // k_step_retract
  int evalR;                            // k_eval_reproj
  int evalF, evalPri;                   // k_eval_rest: [factor blocks | prior block]
  int build() const { return buildSlabs + buildFac + buildPri; }
  int post() const { return postLm + postFac + 1; }
  int evalRest() const { return evalF + evalPri; }
};
inline BatchExtents batchExtentsOf(const BatchDims& w) {
  BatchExtents e;
  e.buildSlabs = w.nSlabs; e.buildFac = w.F; e.buildPri = priorAccBlockCount(w.priorM, w.ownsCamera != 0);
  e.postLm = postLmBlockCount(w.L, w.N); e.postFac = postFacBlockCount(w.F);
  e.step = stepBlockCount(w.nPose, w.nExt, w.nSb, w.L);
  e.evalR = evalReprojBlockCount(w.N);
  e.evalF = w.F; e.evalPri = evalPriorBlockCount(w.priorM);
  return e;
}

// stages of a round a window takes part in (BatchSlot::stages)
enum : int { kBatchFull = 1,    // build + reduced solve + post-solve pass with the fused dogleg step (a fresh linearisation)
             kBatchReuse = 2,   // k_step_retract only (a rejected step: smaller radius on the same Gauss-Newton / Cauchy pair)
             kBatchEval = 4 };  // the candidate (or initial) evaluation

// gridDim.x of every launch of a lane's round: per launch the largest extent among the windows that take part in its stage
struct BatchGrid {
  int build = 0, post = 0, step = 0, evalR = 0, evalRest = 0;
  void include(const BatchExtents& e, int stages) {
    if (stages & kBatchFull) { build = std::max(build, e.build()); post = std::max(post, e.post()); }
    if (stages & kBatchReuse) step = std::max(step, e.step);
    if (stages & kBatchEval) { evalR = std::max(evalR, e.evalR); evalRest = std::max(evalRest, e.evalRest()); }
  }
  // blocks per window row of the round's launches whose extent differs from window to window (the launches with one grid for
  // every window -- slab sum, reduced solve -- are not counted: no block of a participating window is idle there)
  long long blocks(int stagesUnion) const {
    long long n = 0;
    if (stagesUnion & kBatchFull) n += (long long)build + post;
    if (stagesUnion & kBatchReuse) n += step;
    if (stagesUnion & kBatchEval) n += (long long)evalR + evalRest;
    return n;
  }
};
// the blocks of those launches that do work for a window with extents `e` taking part in `stages`
inline long long batchBusyBlocks(const BatchExtents& e, int stages) {
  BatchGrid g;
  g.include(e, stages);
  return g.blocks(stages);
}

// ---- grouping: windows whose fields agree share a launch sequence, whatever their landmark and observation counts
struct BatchGroupFields {
  int d, dC, dCPose, F, nPose, nExt, nSb, priorM, anyExtVariable, ldS, sPadded, priorBlocks, nCam /* (staging area of the evaluation) */, schurDense;
};
struct BatchGroupKey {
  static constexpr int kFields = 14;
  int v[kFields];
  bool operator<(const BatchGroupKey& o) const { return std::lexicographical_compare(v, v + kFields, o.v, o.v + kFields); }
  bool operator==(const BatchGroupKey& o) const { return std::equal(v, v + kFields, o.v); }
};
inline BatchGroupKey batchGroupKey(const BatchGroupFields& f) {
  return BatchGroupKey{{f.d, f.dC, f.dCPose, f.F, f.nPose, f.nExt, f.nSb, f.priorM, f.anyExtVariable, f.ldS, f.sPadded, f.priorBlocks, f.nCam, f.schurDense}};
}

// ---- lanes: a lane's grid is as large as its largest window, so similar windows share a lane.  The windows of a group are
// sorted by (landmark chunks, observation blocks) -- stable: windows of equal size keep the order they were handed in -- and
// dealt as contiguous runs to up to `maxLanes` lanes of at least two windows each (a group of fewer than four: one lane).
struct BatchLane { int first, count; };   // positions [first, first + count) of the sorted order
struct BatchLanePlan {
  std::vector<int> order;        // sorted position -> index into the group
  std::vector<BatchLane> lanes;
};
inline BatchLanePlan planBatchLanes(const std::vector<BatchDims>& ws, int maxLanes) {
  BatchLanePlan plan;
  const int B = (int)ws.size();
  plan.order.resize((size_t)B);
  for (int i = 0; i < B; ++i) plan.order[(size_t)i] = i;
  auto chunks = [&](int i) { return (ws[(size_t)i].L + 15) / 16; };
  auto obsBlocks = [&](int i) { return (ws[(size_t)i].N + 255) / 256; };
  std::stable_sort(plan.order.begin(), plan.order.end(), [&](int a, int b) {
    return chunks(a) != chunks(b) ? chunks(a) < chunks(b) : obsBlocks(a) < obsBlocks(b);
  });
  const int nLanes = std::max(1, std::min(maxLanes, B / 2));
  for (int k = 0; k < nLanes && B > 0; ++k) {
    BatchLane ln;
    ln.first = (int)((long long)B * k / nLanes);
    ln.count = (int)((long long)B * (k + 1) / nLanes) - ln.first;
    plan.lanes.push_back(ln);
  }
  return plan;
}

}  // namespace svin
