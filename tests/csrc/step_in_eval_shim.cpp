// C entry points over stepInEvalTaken of svin_amd/csrc/build_plan.hpp for tests/test_step_in_eval_host.py: whether the dogleg step
// of an iteration moves from the tail of k_post_solve to the head of k_eval_build's blocks.  sie_decide puts the predicate's inputs
// together from a window's sizes as Window::solve and kernels.hip do (stepModeOf, planBuild, planEvaluation, evalBuildTaken);
// sie_raw takes the predicate's own inputs.
#include <cstdint>
#include "../../svin_amd/csrc/build_plan.hpp"

extern "C" {
// a: dC dCPose anyExtVariable L N F priorM ownsCamera nPose nExt nCam nSb d                        (the window, 0..12)
//    stepSwitches (1 SVIN_SPLIT_EVAL, 2 SVIN_NO_FUSE_STEP, 4 SVIN_NO_DEFER_LM)                        (13)
//    sharded noSpeculation iteration numIter reuse hostFactors noStepInEval noEvalBuild computeUnits  (14..22)
//    SVIN_SLAB_CHUNKS (0: unset)                                                                      (23)
int sie_decide(const int32_t* a, int64_t cameraModelBytes, int64_t factorSharedBytes) {
  using namespace svin;
  const int dC = a[0], dCPose = a[1], anyExt = a[2], L = a[3], N = a[4], F = a[5], priorM = a[6], owns = a[7], nPose = a[8], nExt = a[9],
            nCam = a[10], nSb = a[11], d = a[12];
  const bool sharded = a[14] != 0, noSpeculation = a[15] != 0, reuse = a[18] != 0;
  const SchurForm f = chooseSchurForm(dC, L, N, nPose, anyExt != 0, false, false, a[23]);
  const BuildDims m{dC, dCPose, L, N, F, priorM, owns, anyExt, f.schurDense, f.schurPanels, f.schurBlocks, f.nSlabs, 0, 0, 0};
  const BuildPlan q = planBuild(m, BuildSwitches{false});
  const EvalDims ed{nPose, nExt, nCam, L, N, F, priorM};
  const EvalPlan e = planEvaluation(ed, EvalSwitches{false}, KernelSizes{(size_t)cameraModelBytes, (size_t)factorSharedBytes});
  const StepMode sm = stepModeOf(StepDims{nPose, nExt, nSb, L, N, e.fusable}, StepSwitches{(a[13] & 1) != 0, (a[13] & 2) != 0, (a[13] & 4) != 0}, sharded);
  StepInEvalIn in{};
  in.chosenForm = sm.chosenForm;
  in.sharded = sharded;
  // Window::solve: `speculate` on one GPU, and the accumulators are clean behind the post-solve pass
  in.buildWanted = specBuildWanted(!noSpeculation && !sharded, true, a[16], a[17]);
  in.evalBuildTaken = a[21] == 0 && evalBuildTaken(m, q, e, sharded, a[22], (size_t)factorSharedBytes);
  in.reuse = reuse;
  in.postSplit = e.postSplit;
  in.hostFactors = a[19] != 0;
  in.noStepInEval = a[20] != 0;
  in.d = d; in.items = nPose + nExt + nSb; in.nPost = e.post.grid;
  in.evalStageBytes = evalStageBytes(ed, (size_t)cameraModelBytes, true, true);
  in.chunkLdsBytes = q.schurDense.ldsBytes; in.stageBytes = e.stageBytes; in.factorSharedBytes = (size_t)factorSharedBytes;
  return stepInEvalTaken(in) ? 1 : 0;
}
// a: chosenForm sharded buildWanted evalBuildTaken reuse hostFactors noStepInEval d items nPost postSplit; b: the four LDS sizes in bytes
int sie_raw(const int32_t* a, const int64_t* b) {
  using namespace svin;
  StepInEvalIn in{};
  in.chosenForm = a[0]; in.sharded = a[1] != 0; in.buildWanted = a[2] != 0; in.evalBuildTaken = a[3] != 0; in.reuse = a[4] != 0;
  in.hostFactors = a[5] != 0; in.noStepInEval = a[6] != 0; in.d = a[7]; in.items = a[8]; in.nPost = a[9]; in.postSplit = a[10] != 0;
  in.evalStageBytes = (size_t)b[0]; in.chunkLdsBytes = (size_t)b[1]; in.stageBytes = (size_t)b[2]; in.factorSharedBytes = (size_t)b[3];
  return stepInEvalTaken(in) ? 1 : 0;
}
int sie_constant(int which) {
  using namespace svin;
  const int c[5] = {kStepHeadMaxD, kStepHeadMaxItems, kMaxPartials, kStepHeadRedDoubles, (int)stepHeadLdsBytes(150)};
  return c[which];
}
}
