// svin_amd: host planning of the launches in front of and behind the reduced solve -- which landmark-elimination form builds the
// normal equations (launchAccumulateNormalEquations, launchEvalBuild, launchBatchRound; kernels.hip), with which kernel variant,
// grids and dynamic LDS; how the evaluation is issued (one launch, split, fused with the build); and how the dogleg step is taken.
// HIP-free (tests/test_build_plan_host.py runs it on the CPU through tests/csrc/build_plan_shim.cpp): the launchers walk the
// plans, so every threshold and every size is written once.  The plans are functions of plain integers; debug options arrive as
// switches the caller reads once, and the two sizes only the kernels' translation unit knows -- sizeof(CameraModel),
// sizeof(FactorShared) -- as arguments.
//
// The forms (DeviceProblem::schurDense / schurPanels / schurBlocks are pack()'s choice, pack_plan.hpp chooseSchurForm):
//   kBuildDense        L, N, dC > 0, schurDense    k_schur_dense<...> (DenseVariant) | k_eval_build, k_reduce_slabs
//   kBuildBlockPairs   ... schurPanels, schurBlocks  k_panels_landmarks, k_blocks_slots, k_schur_rows, k_blocks_pose_reduce,
//                                                  k_factors_only, k_reduce_panel_slabs
//   kBuildPanels       ... schurPanels             k_panels_landmarks, k_schur_panels, k_factors_only, k_reduce_panel_slabs
//   kBuildPairwise     ... neither                 k_schur<USE_LDS, ...>, k_reduce_slabs
//   kBuildFactorsOnly  no landmark part            k_factors_only
#pragma once
#include <algorithm>
#include <cstddef>
#include "dmath.hpp"       // SVIN_HD
#include "tile_dims.hpp"   // kStage, pairwiseSlabFitsLds
#include "batch_plan.hpp"  // the block counts shared with the batched extents
#include "pack_plan.hpp"   // kBlk*: the work lists the wide forms' kernels walk
#include "solve_plan.hpp"  // PlannedLaunch

namespace svin {

// ---------------------------------------------------------------- constants the planning and the kernels share
// dense form (k_schur_dense)
constexpr int kDenseLm = 16;              // landmarks per chunk
constexpr int kDenseK = 3 * kDenseLm;     // columns of G per chunk
constexpr int kDenseLd = kDenseK + 1;     // odd leading dimension keeps the MFMA operand reads off the same banks
constexpr int kPoseAcc = 28;              // per pose: 21 (upper 6x6) + 6 (Jp^T r) + pad
// observations per batch of the A part on the MFMA path (U = [.. Jc_o^T ..], two columns each), by the rows of the tiles
SVIN_HD constexpr int denseObsBatch(int rows) { return rows <= 128 ? 32 : (rows <= 192 ? 16 : 8); }
// panel forms (k_schur_panels, k_schur_rows): the camera matrix in panels of 96 rows (16 pose blocks, 6 MFMA tile rows)
constexpr int kPanelRows = 96;
constexpr int kPanelSlab = kPanelRows * kPanelRows + 3 * kPanelRows;
constexpr int kBlkPanelPoses = kPanelRows / 6;   // 16
constexpr int kBlkStride = 20;                   // doubles per record staged in LDS: 18, then a pair nothing ever writes (zero: the K = 3 padding of every operand)
constexpr int kBlkPoseLd = 35;                   // per pose block of the slot pass's accumulators: odd, so that the sixteen slots of a landmark hit different banks
#ifndef SVIN_SLOT_COPIES_KB
#define SVIN_SLOT_COPIES_KB 76
#endif
// evaluation and post-solve pass
constexpr int kMaxPartials = 4096;        // partial-sum slots in DeviceProblem::partial: each slot holds up to this many doubles
constexpr int kEvalSplitBlocks = 512;     // more blocks than this: the evaluation's reprojection blocks get a launch of their own
                                          // (launchEvalAll), the post-solve pass the kernel held to two workgroups per CU (launchDoglegPrepare)
constexpr int kMaxLosses = 15;            // entries of a window's reprojection loss table (entry 0: CauchyLoss(1))
constexpr size_t kLossTabBytes = (size_t)2 * kMaxLosses * 8;   // (kind, a) per entry, as doubles: the LDS the evaluation stages
constexpr int kFusedStepMaxBlocks = 16384;   // parameter blocks + landmarks one workgroup of k_post_solve retracts itself

// ---------------------------------------------------------------- the build
enum BuildForm : int { kBuildDense = 0, kBuildBlockPairs = 1, kBuildPanels = 2, kBuildPairwise = 3, kBuildFactorsOnly = 4 };
// the template instances of k_schur_dense / k_schur_dense_batch <MAXT, A_MFMA, NW>
enum DenseVariant : int { kDense17Mfma8 = 0,    // <17, true, 8>: more than 12 tile rows
                          kDense10Mfma8 = 1,    // <10, true, 8>: 9 .. 12 tile rows
                          kDense9Mfma4 = 2,     // <9, true, 4>: up to 8 tile rows, variable extrinsics
                          kDense9Copies4 = 3 }; // <9, false, 4>: up to 8 tile rows, A in per-wave block copies
struct BuildDims {   // DeviceProblem's fields of these names
  int dC, dCPose, L, N, F;
  int priorM, ownsCamera, anyExtVariable;
  int schurDense, schurPanels, schurBlocks, nSlabs;
  int nSlots, nPanelBlocks, nPanelPairs;
};
struct BuildSwitches { bool schurAMfma; };   // SVIN_SCHUR_A_MFMA

struct BuildPlan {
  BuildForm form;
  int formCode;        // SVIN_LAST_SCHUR_FORM (kernels.hpp lastSchurForm)
  int nFac, nPri;      // factor blocks and the prior's blocks that ride in the form's launches
  // dense form
  DenseVariant variant;
  bool aMfma, aBlocks; // the A part on the MFMA path; ... accumulated block-wise in LDS (DeviceProblem::aBlocks)
  int denseThreads;    // block size of the variant
  // block-pair form
  int nCopies;         // copies of the slot pass's per-pose accumulators
  int nSlotBlocks;     // workgroups of k_blocks_slots = partials k_blocks_pose_reduce sums
  // pairwise form
  bool useLds;         // a private slab per workgroup in LDS (otherwise one global slab and atomics)
  int pairwiseChunkBlocks;   // landmark blocks of k_schur: nSlabs with LDS slabs, up to 2048 blocks of four landmarks without
  size_t slabBytes;    // ... of the one global slab cleared ahead of the launch then
  // the launches of the sequence; grid 0: not part of it (factor / prior blocks included where they ride along)
  PlannedLaunch schurDense;                                              // dense
  PlannedLaunch panelsLandmarks, blocksSlots, schurRows, blocksPoseReduce;   // block-pair (panelsLandmarks: the tile form too)
  PlannedLaunch schurPanels;                                             // tile form
  PlannedLaunch factorsOnly;                                             // both panel forms, and a window without a landmark part
  PlannedLaunch reducePanelSlabs; int reducePanelPairs;                  // gridDim.x | gridDim.y
  PlannedLaunch pairwise;
  PlannedLaunch reduceSlabs; int reduceSlabCount;                        // slabs k_reduce_slabs is told to sum: those the build's grid wrote
};

// LDS doubles of k_schur_dense behind its G tile (rows x kDenseLd), for nP reduced 6-blocks of which nPB are poses: the blocks
// of A and the extrinsics x pose cross blocks (aBlocks), the U tile of the MFMA path, or four per-wave copies of the pose blocks.
// (k_schur_dense_body forms the same sum itself, `extraLds`, and says there why it does not call this function.)
constexpr size_t denseExtraLdsDoubles(int rows, int nP, int nPB, bool aMfma, bool aBlocks) {
  return aBlocks ? (size_t)nP * kPoseAcc + (size_t)(nP - nPB) * nPB * 36
                 : (aMfma ? (size_t)rows * (2 * denseObsBatch(rows) + 1) : (size_t)4 * nP * kPoseAcc);
}
inline int denseTileRows(int dC) { return (dC + 2 + 15) / 16; }   // two augmented rows carry the gradients
inline size_t blockPairRowsLdsBytes() {   // k_schur_rows: two record buffers / the slab image
  return (size_t)std::max(2 * kBlkBatchRecs * kBlkStride, kBlkPanelPoses * kBlkPanelPoses * 36) * 8;
}
// off-diagonal pairs of k_schur_panels: two G tiles + c; diagonal pairs: one G tile + the per-wave pose blocks + c (smaller)
constexpr size_t kPanelsLdsBytes = ((size_t)2 * kPanelRows * kDenseLd + kDenseK) * 8;
static_assert(2 * kPanelRows * kDenseLd >= kPanelRows * kDenseLd + 4 * (kPanelRows / 6) * kPoseAcc, "diagonal pairs fit the same allocation");

inline BuildPlan planBuild(const BuildDims& m, const BuildSwitches& sw) {
  BuildPlan q{};
  const int dC = m.dC;
  q.nFac = m.F;   // this rank's factors
  q.nPri = priorAccBlockCount(m.priorM, m.ownsCamera != 0);   // the prior rides along as extra blocks
  const int nRide = q.nFac + q.nPri;
  const bool landmarks = m.L > 0 && m.N > 0 && dC > 0;
  const PlannedLaunch reduceSlabs{(dC * dC + 3 * dC + 15) / 16, 0};
  q.variant = kDense9Copies4;
  if (landmarks && m.schurDense) {
    q.form = kBuildDense;
    const int nTr = denseTileRows(dC), rows = 16 * nTr;
    q.aMfma = m.anyExtVariable || nTr > 8;
    // A on the MFMA path needs a fill / barrier / clear round per batch of observations; when the blocks of A fit LDS
    // next to G they are accumulated directly (LDS atomics) and merged into the accumulator tiles once per chunk
    const int nP = dC / 6, nPB = m.dCPose / 6;
    q.aBlocks = q.aMfma && !sw.schurAMfma && ((size_t)rows * kDenseLd + denseExtraLdsDoubles(rows, nP, nPB, true, true)) * 8 <= 150 * 1024;
    // <= 16 tile rows: 136 tiles over 8 waves; <= 12 tile rows: 78 tiles
    q.variant = nTr > 12 ? kDense17Mfma8 : nTr > 8 ? kDense10Mfma8 : q.aMfma ? kDense9Mfma4 : kDense9Copies4;
    q.denseThreads = 64 * (q.variant <= kDense10Mfma8 ? 8 : 4);
    q.formCode = 1000 + 10 * (q.variant == kDense17Mfma8 ? 17 : q.variant == kDense10Mfma8 ? 10 : 9) + (q.aMfma ? (q.aBlocks ? 1 : 2) : 0);
    q.schurDense = {m.nSlabs + nRide, ((size_t)rows * kDenseLd + denseExtraLdsDoubles(rows, nP, nPB, q.aMfma, q.aBlocks)) * 8};
    q.reduceSlabs = reduceSlabs; q.reduceSlabCount = m.nSlabs;
  } else if (landmarks && m.schurPanels) {
    q.form = m.schurBlocks ? kBuildBlockPairs : kBuildPanels;
    q.formCode = m.schurBlocks ? 2000 : 3000;
    q.panelsLandmarks = {(m.L + 15) / 16, 0};
    if (m.schurBlocks) {
      // the slot pass keeps up to four copies of its per-pose accumulators (one per 16-lane group of a wave: the four landmarks a
      // wave works on see the same poses, and four lanes adding to one address serialise) -- as many as SVIN_SLOT_COPIES_KB hold
      q.nCopies = 4;
      while (q.nCopies > 1 && (size_t)q.nCopies * (dC / 6) * kBlkPoseLd * 8 > SVIN_SLOT_COPIES_KB * 1024) q.nCopies >>= 1;
      q.nSlotBlocks = (m.nSlots + kBlkSlotsPerWorkgroup - 1) / kBlkSlotsPerWorkgroup;
      q.blocksSlots = {q.nSlotBlocks, (size_t)q.nCopies * (dC / 6) * kBlkPoseLd * 8};
      q.schurRows = {m.nPanelBlocks, blockPairRowsLdsBytes()};
      if (q.nSlotBlocks > 0) q.blocksPoseReduce = {dC / 6, 0};
    } else {
      q.schurPanels = {m.nPanelBlocks, kPanelsLdsBytes};
    }
    q.factorsOnly = {nRide, 0};
    q.reducePanelSlabs = {(kPanelSlab + 15) / 16, 0}; q.reducePanelPairs = m.nPanelPairs;
  } else if (landmarks) {
    q.form = kBuildPairwise;
    q.useLds = pairwiseSlabFitsLds(dC);
    q.formCode = q.useLds ? 4000 : 4001;
    q.slabBytes = pairwiseSlabBytes(dC);
    q.pairwiseChunkBlocks = q.useLds ? m.nSlabs : std::min((m.L + 3) / 4, 2048);
    q.pairwise = {q.pairwiseChunkBlocks + nRide, q.useLds ? q.slabBytes + kPairwiseStageBytes : kPairwiseStageBytes};
    q.reduceSlabs = reduceSlabs; q.reduceSlabCount = q.useLds ? m.nSlabs : 1;
  } else {
    q.form = kBuildFactorsOnly;
    q.formCode = 5000;
    q.factorsOnly = {nRide, 0};
  }
  return q;
}

// ---------------------------------------------------------------- the evaluation and the post-solve pass
struct EvalDims { int nPose, nExt, nCam, L, N, F, priorM; };   // DeviceProblem's fields of these names
struct EvalSwitches { bool noEvalSplit; };                     // SVIN_NO_EVAL_SPLIT
struct KernelSizes { size_t cameraModel, factorShared; };      // sizeof(CameraModel), sizeof(FactorShared): the factor blocks' LDS

// LDS bytes of the tables a reprojection block stages: poses, extrinsics, camera models, loss table.
// reductionAhead: the 48 doubles of the block's reduction scratch in front of them (the kernels whose LDS is this area alone);
// headRoom: 64 bytes more, which the forms that share a launch with the factor blocks have always asked for (nothing reads them)
inline size_t evalStageBytes(const EvalDims& e, size_t cameraModelBytes, bool reductionAhead, bool headRoom) {
  return (size_t)(e.nPose + e.nExt) * 7 * 8 + (size_t)e.nCam * cameraModelBytes + kLossTabBytes + (reductionAhead ? (size_t)48 * 8 : 0) +
         (headRoom ? 64 : 0);
}
struct EvalPlan {
  int nR, pri;               // reprojection blocks (256 observations each), the prior's block
  bool fusable;              // factors, reprojection blocks and prior in one launch (k_eval_all): factors and observations present,
                             // the staging area fits the factor blocks' LDS, a partial slot holds every block's sum
  bool split;                // more than kEvalSplitBlocks blocks: the reprojection blocks in a launch of their own
  size_t stageBytes;         // the staged tables alone (the chunk blocks of k_eval_build place them behind their tiles)
  PlannedLaunch evalAll;     // k_eval_all / the evaluation blocks of k_eval_build: F + nR + pri blocks, static LDS
  PlannedLaunch reprojSplit, restSplit;   // k_eval_reproj_split (_batch: the same LDS) + k_eval_rest_split
  PlannedLaunch reprojAlone; // k_eval_reproj (128 observations per block), the un-fused evaluation
  // post-solve pass (k_post_solve): landmark blocks, factor blocks, one tail block
  int postLm, postFac;
  bool postSplit;            // more than kEvalSplitBlocks blocks: k_post_solve_wide
  PlannedLaunch post;
};
inline EvalPlan planEvaluation(const EvalDims& e, const EvalSwitches& sw, const KernelSizes& ks) {
  EvalPlan q{};
  q.nR = evalReprojBlockCount(e.N); q.pri = evalPriorBlockCount(e.priorM);
  q.fusable = e.F > 0 && e.N > 0 && evalStageBytes(e, ks.cameraModel, false, true) <= ks.factorShared && q.nR + e.F <= kMaxPartials;
  const int nEval = e.F + q.nR + q.pri;
  q.split = nEval > kEvalSplitBlocks && !sw.noEvalSplit;
  q.stageBytes = evalStageBytes(e, ks.cameraModel, false, false);
  q.evalAll = {nEval, 0};
  q.reprojSplit = {q.nR, evalStageBytes(e, ks.cameraModel, true, true)};
  q.restSplit = {e.F + q.pri, 0};
  q.reprojAlone = {(e.N + 127) / 128, q.stageBytes};
  q.postLm = postLmBlockCount(e.L, e.N); q.postFac = postFacBlockCount(e.F);
  q.post = {q.postLm + q.postFac + 1, 0};
  q.postSplit = q.post.grid > kEvalSplitBlocks && !sw.noEvalSplit;
  return q;
}

// ---- evaluation and build of the next normal equations in ONE launch (k_eval_build: the blocks of the fused evaluation, then the
// chunk blocks of the narrow dense form, which evaluate their own observations).  Every workgroup of that launch brings the factor
// blocks' LDS, one workgroup per compute unit: the launch is taken when all of them run at once (a second round of workgroups
// would cost what the launch boundary it removes costs) and when a chunk block's tiles and staged tables fit that LDS.
// denseFormPlain: k_schur_dense<9, false, 4> is the window's form (fixed extrinsics, at most 8 tile rows); chunkLdsBytes: the
// dynamic LDS that form takes; stageBytes: poses, extrinsics, camera models and loss table; ldsBytes: the factor blocks' LDS.
inline bool evalBuildFits(bool denseFormPlain, int evalBlocks, int chunkBlocks, int computeUnits, size_t chunkLdsBytes, size_t stageBytes,
                          size_t ldsBytes) {
  if (!denseFormPlain || evalBlocks <= 0 || chunkBlocks <= 0) return false;
  if ((long long)evalBlocks + chunkBlocks > computeUnits) return false;
  return ((chunkLdsBytes + 15) & ~(size_t)15) + stageBytes <= ldsBytes;
}
// Whether launchEvalBuild takes the window: the narrow dense form with fixed extrinsics on one GPU, a fusable evaluation, and
// the fit above.  (The dense form never has a chain on the side lane: sbEarlyActive asks for the wide form.)
inline bool evalBuildTaken(const BuildDims& m, const BuildPlan& b, const EvalPlan& e, bool sharded, int computeUnits, size_t factorSharedBytes) {
  if (b.form != kBuildDense || sharded || !e.fusable) return false;
  return evalBuildFits(!b.aMfma && !m.anyExtVariable, e.evalAll.grid, m.nSlabs, computeUnits, b.schurDense.ldsBytes, e.stageBytes, factorSharedBytes);
}

// ---------------------------------------------------------------- the dogleg step
// How the step behind the post-solve pass is taken: by k_post_solve's last block (fused: no all-reduce sits between them), with
// the landmark half of the retraction left to the candidate evaluation, which reads every landmark anyway (deferred: then the
// fused step has no size limit), or by a launch of its own (k_step_retract).
struct StepDims { int nPose, nExt, nSb, L, N; bool fusable; };   // fusable: EvalPlan::fusable
struct StepSwitches { bool splitEval, noFuseStep, noDeferLm; };   // SVIN_SPLIT_EVAL, SVIN_NO_FUSE_STEP, SVIN_NO_DEFER_LM
struct StepMode {
  bool deferPossible;   // the candidate evaluation is the fused one and may move the landmarks
  bool small;           // one workgroup retracts the whole window quickly enough
  bool fuseStep, deferLm;
  int chosenForm;       // svin_ba_debug_trust_region_step's numbering: 1 fused, landmarks by k_post_solve's tail; 2 k_step_retract;
                        // 3 fused, landmarks by the candidate evaluation
};
inline StepMode stepModeOf(const StepDims& m, const StepSwitches& sw, bool sharded) {
  StepMode q{};
  q.deferPossible = m.fusable && !sw.splitEval && !sw.noDeferLm && m.L > 0 && m.N > 0;
  q.small = m.nPose + m.nExt + m.nSb + m.L <= kFusedStepMaxBlocks;
  q.fuseStep = !sw.noFuseStep && !sharded && (q.small || q.deferPossible);
  q.deferLm = q.fuseStep && q.deferPossible;
  q.chosenForm = q.fuseStep ? (q.deferPossible ? 3 : 1) : 2;
  return q;
}
// ---- the step at the head of the evaluation's blocks (k_post_solve without its tail + k_eval_build with a radius).  The serial
// tail of the post-solve pass -- ticket, partials, reduction, coefficients, retraction of the parameter blocks -- produces only what
// the blocks of the next launch read first; each of those blocks computes it itself instead, from the partials.  The pair is taken
// where the narrow pass runs (k_post_solve, not k_post_solve_wide), where the old tail staged everything (its limits below), where the next launch is k_eval_build (a build is wanted behind this
// evaluation: never on the last iteration of a solve, which k_eval_all follows), and never on a re-used linearisation, whose step
// k_step_retract takes.  A window with host-evaluated factors keeps the tail: the host reads the candidate blocks before the launch.
constexpr int kStepHeadMaxD = 1024;       // y_C and v_C staged in LDS (k_post_solve: kStageMax)
constexpr int kStepHeadMaxItems = 96;     // parameter blocks one pass of a workgroup retracts (k_post_solve: kStageItems)
constexpr int kStepHeadRedDoubles = 16 * 9 + 8;   // the block sum's rows and group B
inline size_t stepHeadLdsBytes(int d) { return (size_t)(kStepHeadRedDoubles + 2 * d) * 8; }   // behind a block's staged tables
// Whether Window::solve enqueues a speculative build behind the candidate evaluation of this iteration: speculation on, clean
// accumulators (they are, right behind a post-solve pass), and an iteration to use it -- never the last one of the solve.
inline bool specBuildWanted(bool speculate, bool accumulatorsClean, int iteration, int numIter) {
  return speculate && accumulatorsClean && iteration < numIter;
}
struct StepInEvalIn {
  int chosenForm;        // StepMode::chosenForm
  bool sharded;          // more than one GPU (or the forced one-rank communicator)
  bool buildWanted;      // a speculative build is enqueued behind this iteration's candidate evaluation
  bool evalBuildTaken;   // evalBuildTaken() of the window
  bool reuse;            // the iteration re-uses the linearisation (a rejected step before it)
  bool postSplit;        // EvalPlan::postSplit: the pass is k_post_solve_wide, which keeps its tail
  bool hostFactors;      // the window has factors the host evaluates
  bool noStepInEval;     // SVIN_NO_STEP_IN_EVAL
  int d, items, nPost;   // reduced unknowns, pose + extrinsics + speed/bias blocks, blocks of the post-solve pass
  size_t evalStageBytes, chunkLdsBytes, stageBytes, factorSharedBytes;   // as evalBuildFits takes them; evalStageBytes: the reprojection blocks' tables behind their reduction scratch
};
inline bool stepInEvalTaken(const StepInEvalIn& q) {
  if (q.noStepInEval || q.chosenForm != 3 || q.sharded || !q.buildWanted || !q.evalBuildTaken || q.reuse || q.postSplit || q.hostFactors) return false;
  if (q.d <= 0 || q.d > kStepHeadMaxD || q.items <= 0 || q.items > kStepHeadMaxItems || q.nPost <= 0 || q.nPost > kMaxPartials) return false;
  const size_t head = stepHeadLdsBytes(q.d);
  if (q.evalStageBytes + head > q.factorSharedBytes) return false;
  return ((q.chunkLdsBytes + 15) & ~(size_t)15) + q.stageBytes + head <= q.factorSharedBytes;
}

// the batched round has the fused step with the landmarks deferred and nothing else (k_post_solve_batch, k_eval_reproj_batch)
inline bool batchedStepTakes(const StepMode& q) { return q.fuseStep && q.deferLm && q.small; }

}  // namespace svin
