// A stand-alone run of svin_amd/csrc/solve_plan.hpp (the host planning of the reduced solve) for AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_solve_plan_host.py compiles this file with -fsanitize=address,undefined
// -fno-sanitize-recover=all and requires exit status 0.  It plans the sweep of that test -- dC = 0, 6, ..., 2394, chains of
// 0 ... 69 blocks, unpadded and padded S, each switch -- plus sizes that are no multiple of anything, and walks every back panel.
// What the plans must hold is the Python test's business; here a few sums are cross-checked so that nothing is optimised away.
#include <cstdio>
#include "../../svin_amd/csrc/solve_plan.hpp"

int main() {
  using namespace svin;
  long long plans = 0, chains = 0, panels = 0;
  unsigned long long sum = 0;
  for (int cfg = 0; cfg < 5; ++cfg) {
    const SolveSwitches sw{cfg == 2, cfg == 3, cfg == 4};
    for (int dC = 0; dC <= 2394; dC += (cfg == 0 ? 1 : 6))   // (unpadded: every size, not only whole pose blocks)
      for (int n = 0; n < 70; ++n) {
        const int d = dC + 9 * n;
        const ReducedSolvePlan q = planReducedSolve(SolveDims{d, dC, n, cfg == 0 ? 0 : 1}, sw);
        if (q.end > solveReducedScratchDoubles(d, true) || q.chainOverflow) {
          std::fprintf(stderr, "d %d dC %d chain %d: the plan ends at %zu\n", d, dC, n, q.end);
          return 1;
        }
        for (int k = 0; k < q.nBackPanels; ++k) {
          const BackPanel b = backPanel(q.dp, k);
          if (b.c0 < 0 || b.c1 > q.dp || b.c0 >= b.c1 || bigPartialOff(q.dp, b.nChunks) > bigMatrixDoubles(q.dp)) return 1;
          ++panels;
        }
        ++plans;
        chains += q.chainMode != 0;
        sum += q.end + q.cholLds.ldsBytes + q.cholLL.ldsBytes + q.bigChain.ldsBytes + q.sbFactor.ldsBytes + (unsigned)q.bigChain.grid;
      }
  }
  std::printf("%lld plans, %lld with the chain eliminated, %lld back panels, %llu\n", plans, chains, panels, sum);
  return plans > 0 && chains > 0 && panels > 0 && sum > 0 ? 0 : 1;
}
