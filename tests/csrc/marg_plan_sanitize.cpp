// A stand-alone run of svin_amd/csrc/marg_plan.hpp (the host planning of the marginalisation) for AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_marg_plan_host.py compiles this file with -fsanitize=address,undefined
// -fno-sanitize-recover=all and requires exit status 0.  It calls every function of the header on seeded inputs: the LDS helpers
// for n = 0 ... 400, planMargJob over every split of every dense size up to 320 with pseudo-random landmark, residual and factor
// counts, and selectMargFrames over pseudo-random windows of up to 40 frames.  What the plans must hold is the Python test's
// business; here a few bounds are cross-checked so that nothing is optimised away.
#include <cstdio>
#include "../../svin_amd/csrc/marg_plan.hpp"

static unsigned long long rngState = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n) {   // xorshift64*, seeded
  rngState ^= rngState >> 12; rngState ^= rngState << 25; rngState ^= rngState >> 27;
  return (unsigned)((rngState * 0x2545f4914f6cdd1dull) >> 33) % n;
}

int main() {
  using namespace svin;
  const size_t js = 16;
  unsigned long long sum = 0;
  long long plans = 0, selections = 0;
  for (int n = 0; n <= 400; ++n) {
    if (jacobiLdsBytes(n, js) > jacobiLdsLimit(js) || jacobiLdsBytesGOnly(n, js) > jacobiLdsLimit(js) || jacobiLd(n) < n) return 1;
    sum += jacobiLdsBytes(n, js) + jacobiLdsBytesGOnly(n, js) + margCholLdsBytes(n) + symEigLdsBytes(n) + margGatherScratchInts(n);
  }
  for (int m = 0; m <= 320; ++m)
    for (int nk = 0; nk <= m; ++nk) {
      const int Lm = (int)rnd(3) == 0 ? 0 : (int)rnd(2001), N = (int)rnd(4) == 0 ? 0 : Lm + (int)rnd(5000), F = (int)rnd(40);
      const MargDims d{m, Lm, N, F, nk, m - nk, 1 + (int)rnd(46), 1 + (int)rnd(8), 1 + (int)rnd(4), (int)rnd(2), (int)rnd(nk + 1)};
      const MargPlan q = planMargJob(d, MargSwitches{(int)rnd(4)}, MargKernelSizes{js});
      for (const PlannedLaunch& l : {q.accumLm, q.accumFactors, q.lmPrepare, q.lmApply, q.lmUpdate, q.dense, q.finalChol, q.finalDc, q.final})
        if (l.grid < 0 || l.ldsBytes + js > kMargLdsPerWorkgroup) {
          std::fprintf(stderr, "m %d nk %d: a launch asks for %zu bytes of LDS\n", m, nk, l.ldsBytes);
          return 1;
        }
      if (q.finalTmp.off + q.finalTmp.len > q.bOut || q.denseTmp.off + q.denseTmp.len > q.bScratch || q.bk.off + q.bk.len > q.bHk ||
          q.vb.off + q.vb.len > q.clearVec || q.linJe.off + q.linJe.len > q.bLin || (q.dense.grid != 0) == q.copyPair + (nk == 0)) {
        std::fprintf(stderr, "m %d nk %d Lm %d N %d: a region leaves its buffer\n", m, nk, Lm, N);
        return 1;
      }
      ++plans;
      sum += q.bU + q.bW2 + q.bV + q.bVec + q.bOut + q.gLm + q.dense.ldsBytes + q.final.ldsBytes + (unsigned)q.finalMode;
    }
  for (int rep = 0; rep < 4000; ++rep) {
    const int n = (int)rnd(41);
    std::vector<uint64_t> ids;
    std::vector<char> kf;
    uint64_t id = rnd(1000);
    for (int i = 0; i < n; ++i) { id += 1 + rnd(5); ids.push_back(id); kf.push_back((char)rnd(2)); }
    const size_t numKeyframes = rnd(8), numImuFrames = rnd(8);
    const MargFrames f = selectMargFrames(ids, kf, numKeyframes, numImuFrames);
    if (f.enough != (numImuFrames == 0 || (size_t)n > numImuFrames)) return 1;
    if (f.enough && (f.removeAllButPose.size() + numImuFrames != (size_t)n || f.removeFrames.size() > f.removeAllButPose.size() ||
                     f.allLinearizedFrames != f.removeAllButPose))
      return 1;
    ++selections;
    sum += f.removeFrames.size();
  }
  std::printf("%lld plans, %lld frame selections, %llu\n", plans, selections, sum);
  return plans > 0 && selections > 0 && sum > 0 ? 0 : 1;
}
