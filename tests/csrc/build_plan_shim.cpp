// C entry points over svin_amd/csrc/build_plan.hpp (the host planning of the build, the evaluation and the step) for
// tests/test_build_plan_host.py: the planners take plain integers and switches, so the form, the variant and the size of every
// launch are checked on the CPU.  A row goes in as the kInputs integers of INPUTS in tests/helpers/build_plan_lib.py -- pack()'s
// part, chooseSchurForm, is applied here as Window::pack() applies it -- and comes back as kFields 64-bit integers in the order
// of FIELDS there.
#include <cstdint>
#include <initializer_list>
#include "../../svin_amd/csrc/build_plan.hpp"

namespace {
constexpr int kInputs = 15, kFields = 57;
}  // namespace

extern "C" {
int bp_fields() { return kFields; }
int bp_inputs() { return kInputs; }
// in: rows x kInputs (switches: 1 SVIN_SCHUR_PAIRWISE, 2 SVIN_PANELS_OLD, 4 SVIN_SCHUR_A_MFMA, 8 SVIN_SLAB_CHUNKS=2, 16 SVIN_NO_EVAL_SPLIT)
void bp_plan(int rows, const int32_t* in, int64_t cameraModelBytes, int64_t factorSharedBytes, int smallCus, int64_t* out) {
  using namespace svin;
  for (int r = 0; r < rows; ++r) {
    const int32_t* a = in + (size_t)kInputs * r;
    int64_t* o = out + (size_t)kFields * r;
    const int dC = a[0], dCPose = a[1], anyExt = a[2], L = a[3], N = a[4], F = a[5], priorM = a[6], owns = a[7], nPose = a[8], nExt = a[9], nCam = a[10];
    const int sw = a[14];
    const SchurForm f = chooseSchurForm(dC, L, N, nPose, anyExt != 0, (sw & 1) != 0, (sw & 2) != 0, (sw & 8) ? 2 : 0);
    const BuildDims m{dC, dCPose, L, N, F, priorM, owns, anyExt, f.schurDense, f.schurPanels, f.schurBlocks, f.nSlabs, a[11], a[12], a[13]};
    const BuildPlan q = planBuild(m, BuildSwitches{(sw & 4) != 0});
    const EvalPlan e = planEvaluation(EvalDims{nPose, nExt, nCam, L, N, F, priorM}, EvalSwitches{(sw & 16) != 0},
                                      KernelSizes{(size_t)cameraModelBytes, (size_t)factorSharedBytes});
    int k = 0;
    for (int64_t v : {(int64_t)f.schurDense, (int64_t)f.schurPanels, (int64_t)f.schurBlocks, (int64_t)f.nSlabs, (int64_t)f.useLds,
                      (int64_t)q.form, (int64_t)q.formCode, (int64_t)q.nFac, (int64_t)q.nPri, (int64_t)(q.form == kBuildDense ? (int)q.variant : -1),
                      (int64_t)q.aMfma, (int64_t)q.aBlocks, (int64_t)q.denseThreads, (int64_t)q.nCopies, (int64_t)q.nSlotBlocks, (int64_t)q.useLds,
                      (int64_t)q.pairwiseChunkBlocks, (int64_t)q.slabBytes, (int64_t)q.reducePanelPairs, (int64_t)q.reduceSlabCount})
      o[k++] = v;
    for (const PlannedLaunch& l : {q.schurDense, q.panelsLandmarks, q.blocksSlots, q.schurRows, q.blocksPoseReduce, q.schurPanels, q.factorsOnly,
                                   q.reducePanelSlabs, q.pairwise, q.reduceSlabs}) {
      o[k++] = l.grid;
      o[k++] = (int64_t)l.ldsBytes;
    }
    for (int64_t v : {(int64_t)e.fusable, (int64_t)e.split, (int64_t)e.nR, (int64_t)e.pri, (int64_t)e.stageBytes, (int64_t)e.evalAll.grid,
                      (int64_t)e.reprojSplit.grid, (int64_t)e.reprojSplit.ldsBytes, (int64_t)e.restSplit.grid, (int64_t)e.reprojAlone.grid,
                      (int64_t)e.reprojAlone.ldsBytes, (int64_t)e.postSplit, (int64_t)e.postLm, (int64_t)e.postFac, (int64_t)e.post.grid,
                      (int64_t)evalBuildTaken(m, q, e, false, 256, (size_t)factorSharedBytes),
                      (int64_t)evalBuildTaken(m, q, e, false, smallCus, (size_t)factorSharedBytes)})
      o[k++] = v;
    static_assert(20 + 20 + 17 == kFields, "FIELDS of build_plan_lib.py");
  }
}
// whether k_eval_build takes the row on `computeUnits` compute units (sharded: a rank of a landmark-sharded window)
int bp_eval_build(const int32_t* a, int64_t cameraModelBytes, int64_t factorSharedBytes, int computeUnits, int sharded) {
  using namespace svin;
  const int sw = a[14];
  const SchurForm f = chooseSchurForm(a[0], a[3], a[4], a[8], a[2] != 0, (sw & 1) != 0, (sw & 2) != 0, (sw & 8) ? 2 : 0);
  const BuildDims m{a[0], a[1], a[3], a[4], a[5], a[6], a[7], a[2], f.schurDense, f.schurPanels, f.schurBlocks, f.nSlabs, a[11], a[12], a[13]};
  const EvalPlan e = planEvaluation(EvalDims{a[8], a[9], a[10], a[3], a[4], a[5], a[6]}, EvalSwitches{(sw & 16) != 0},
                                    KernelSizes{(size_t)cameraModelBytes, (size_t)factorSharedBytes});
  return evalBuildTaken(m, planBuild(m, BuildSwitches{(sw & 4) != 0}), e, sharded != 0, computeUnits, (size_t)factorSharedBytes) ? 1 : 0;
}
// in: rows x {nPose, nExt, nSb, L, N, fusable, switches (1 SVIN_SPLIT_EVAL, 2 SVIN_NO_FUSE_STEP, 4 SVIN_NO_DEFER_LM), sharded};
// out: rows x {fuseStep, deferLm, chosenForm, deferPossible, small, batchedStepTakes}
void bp_step_mode(int rows, const int32_t* in, int32_t* out) {
  using namespace svin;
  for (int r = 0; r < rows; ++r) {
    const int32_t* a = in + (size_t)8 * r;
    const StepMode q = stepModeOf(StepDims{a[0], a[1], a[2], a[3], a[4], a[5] != 0}, StepSwitches{(a[6] & 1) != 0, (a[6] & 2) != 0, (a[6] & 4) != 0}, a[7] != 0);
    int32_t* o = out + (size_t)6 * r;
    o[0] = q.fuseStep; o[1] = q.deferLm; o[2] = q.chosenForm; o[3] = q.deferPossible; o[4] = q.small; o[5] = batchedStepTakes(q);
  }
}
// CONSTANTS of build_plan_lib.py
int bp_constant(int which) {
  using namespace svin;
  const int c[19] = {kDenseLm, kDenseK, kDenseLd, kPoseAcc, kStage, kPanelRows, kPanelSlab, kBlkPanelPoses, kBlkStride, kBlkPoseLd,
                     SVIN_SLOT_COPIES_KB, kEvalSplitBlocks, kMaxPartials, kBlkMaxPoseBlocks, kDensePoseCap, (int)kLossTabBytes,
                     kBlkBatchRecs, kBlkSlotsPerWorkgroup, kBlkWaves};
  return c[which];
}
}
