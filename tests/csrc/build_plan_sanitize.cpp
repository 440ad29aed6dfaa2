// A stand-alone run of svin_amd/csrc/build_plan.hpp (the host planning of the build, the evaluation and the step) for
// AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_build_plan_host.py compiles this file with
// -fsanitize=address,undefined -fno-sanitize-recover=all and requires exit status 0.  It walks the sweep of that test -- dC from 0
// past 6 * kBlkMaxPoseBlocks (here EVERY size, not only whole pose blocks), fixed and variable extrinsics with the reduced rows
// split several ways, landmark counts around the chunk size and the slab and grid caps, with and without observations, factors and
// a prior, every combination of the switches -- and the step mode on both sides of its size limit.
// What the plans must hold is the Python test's business; here a few sums are cross-checked so that nothing is optimised away.
#include <cstdio>
#include "../../svin_amd/csrc/build_plan.hpp"

int main() {
  using namespace svin;
  long long plans = 0, forms[5] = {0, 0, 0, 0, 0}, taken = 0, modes = 0;
  unsigned long long sum = 0;
  const int Ls[] = {0, 1, 15, 16, 17, 2048, 2049, 4096, 4097, 8192, 8193};
  const KernelSizes ks{120, 133584};
  for (int dC = 0; dC <= 3100; dC += (dC < 330 || dC > 3060 ? 1 : 7))
    for (int split = 0; split < 4; ++split) {
      const int anyExt = split > 0, nB = dC / 6;
      const int dCPose = split == 0 ? dC : 6 * (split == 1 ? nB / 2 : split == 2 ? (nB > 0 ? nB - 1 : 0) : nB / 5);
      for (int sw = 0; sw < 32; ++sw)
        for (int L : Ls)
          for (int N = 0; N <= 3 * L + 5; N += 3 * L + 5)
            for (int F = 0; F <= 9; F += 9) {
              const int priorM = (sw & 1) ? 30 : 0, owns = (F > 0) ? 1 : 0, nPose = dCPose / 6 + 1, nExt = 2 + (dC - dCPose) / 6;
              const SchurForm f = chooseSchurForm(dC, L, N, nPose, anyExt != 0, (sw & 1) != 0, (sw & 2) != 0, (sw & 8) ? 2 : 0);
              const int nPan = (dC + 95) / 96;
              const BuildDims m{dC, dCPose, L, N, F, priorM, owns, anyExt, f.schurDense, f.schurPanels, f.schurBlocks, f.nSlabs, 7 * L,
                                L > 0 ? 3 * nPan * (nPan + 1) / 2 + 1 : 0, nPan * (nPan + 1) / 2};
              const BuildPlan q = planBuild(m, BuildSwitches{(sw & 4) != 0});
              const EvalPlan e = planEvaluation(EvalDims{nPose, nExt, 2, L, N, F, priorM}, EvalSwitches{(sw & 16) != 0}, ks);
              const size_t largest = std::max({q.schurDense.ldsBytes, q.blocksSlots.ldsBytes, q.schurRows.ldsBytes, q.schurPanels.ldsBytes,
                                               q.pairwise.ldsBytes, e.reprojSplit.ldsBytes});
              if (q.form < kBuildDense || q.form > kBuildFactorsOnly || ((q.reduceSlabs.grid > 0) != (q.reduceSlabCount > 0)) ||
                  (f.schurDense && !anyExt && largest > 160 * 1024)) {
                std::fprintf(stderr, "dC %d dCPose %d L %d N %d switches %d: form %d, %zu bytes of LDS\n", dC, dCPose, L, N, sw, (int)q.form, largest);
                return 1;
              }
              taken += evalBuildTaken(m, q, e, false, 256, ks.factorShared) + evalBuildTaken(m, q, e, true, 256, ks.factorShared);
              ++plans;
              ++forms[q.form];
              sum += largest + (unsigned)q.formCode + (unsigned)q.reduceSlabCount + (unsigned)e.evalAll.grid + (unsigned)e.post.grid + e.stageBytes;
            }
    }
  for (int blocks : {0, 1, 16383, 16384, 16385, 1 << 30})
    for (int sw = 0; sw < 8; ++sw)
      for (int k = 0; k < 8; ++k) {
        const StepMode q = stepModeOf(StepDims{blocks / 3, blocks / 3, blocks - 2 * (blocks / 3), (k & 1) ? 1000 : 0, (k & 2) ? 9000 : 0, (k & 4) != 0},
                                      StepSwitches{(sw & 1) != 0, (sw & 2) != 0, (sw & 4) != 0}, false);
        if (q.chosenForm < 1 || q.chosenForm > 3 || (q.deferLm && !q.fuseStep)) return 1;
        modes += q.chosenForm + batchedStepTakes(q);
      }
  std::printf("%lld plans (dense %lld, block pairs %lld, panels %lld, pairwise %lld, factors only %lld), %lld taken by k_eval_build, %lld, %llu\n", plans,
              forms[0], forms[1], forms[2], forms[3], forms[4], taken, modes, sum);
  for (long long n : forms)
    if (n == 0) return 1;
  return plans > 0 && taken > 0 && modes > 0 && sum > 0 ? 0 : 1;
}
