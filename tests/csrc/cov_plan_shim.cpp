// C entry points over svin_amd/csrc/cov_plan.hpp (the host planning of the marginal-covariance pass) for
// tests/test_cov_plan_host.py: regions of the window's covariance buffer and the size of every launch, checked on the CPU.
// A plan is handed over as kFields 64-bit integers: supported, nT, dpad, then (off, len) of scaled, factor, linv, scale, xs,
// sigma, lmCov, flags, then end, then (grid, threads, ldsBytes) of factorize, inverse, refine, landmarks, pairs.
#include <cstdint>
#include <initializer_list>
#include "../../svin_amd/csrc/cov_plan.hpp"

extern "C" {
int cp_fields() { return 3 + 16 + 1 + 15; }
void cp_plan(int d, int dC, int L, int nPairs, int64_t* o) {
  const svin::CovPlan q = svin::planCovariance(d, dC, L);
  int k = 0;
  o[k++] = q.supported ? 1 : 0;
  o[k++] = q.nT;
  o[k++] = q.dpad;
  for (const svin::CovRegion& r : {q.scaled, q.factor, q.linv, q.scale, q.xs, q.sigma, q.lmCov, q.flags}) {
    o[k++] = (int64_t)r.off;
    o[k++] = (int64_t)r.len;
  }
  o[k++] = (int64_t)q.end;
  for (const svin::CovLaunch& l : {q.factorize, q.inverse, q.refine, q.landmarks, svin::planCovariancePairs(dC, nPairs)}) {
    o[k++] = l.grid;
    o[k++] = l.threads;
    o[k++] = (int64_t)l.ldsBytes;
  }
}
// kCovMaxD, kCovMaxLdsBytes, kCovFlagInts, kCovLmPerBlock
int64_t cp_constant(int which) {
  const int64_t c[4] = {svin::kCovMaxD, (int64_t)svin::kCovMaxLdsBytes, svin::kCovFlagInts, svin::kCovLmPerBlock};
  return c[which];
}
}
