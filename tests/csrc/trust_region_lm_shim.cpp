// C entry points over svin_amd/csrc/trust_region.hpp for tests/test_trust_region_lm_host.py: the same state machine as
// trust_region_shim.cpp drives, with the strategy and the two radii configurable (TrustRegionHost::configure) and the fields the
// Levenberg-Marquardt rules add readable.  HIP-free: g++, no GPU.
#include "../../svin_amd/csrc/trust_region.hpp"

extern "C" {
// strategy < 0: the object is never configured (what Window::solve does for a handle left at its defaults)
void* trlm_create(int strategy, double initialRadius, double maxRadius, double fTol, double gTol, double pTol, int maxIterations, double initialCost) {
  auto* t = new svin::TrustRegionHost();
  t->fTol = fTol; t->gTol = gTol; t->pTol = pTol; t->maxIterations = maxIterations;
  if (strategy >= 0) t->configure(strategy, initialRadius, maxRadius);
  t->start(initialCost);
  return t;
}
void trlm_destroy(void* h) { delete static_cast<svin::TrustRegionHost*>(h); }
int trlm_begin(void* h, int stopRequested) { return static_cast<svin::TrustRegionHost*>(h)->beginIteration(stopRequested != 0) ? 1 : 0; }
static svin::TrScalars unpack(const double* v) {
  svin::TrScalars s;
  s.cost = v[0]; s.stepNormSq = v[1]; s.xNormSq = v[2]; s.gradMax = v[3]; s.failMax = v[4]; s.jdSq = v[5]; s.jdDotR = v[6]; s.doglegStepNorm = v[7];
  return s;
}
int trlm_retry(void* h, const double* v) { return static_cast<svin::TrustRegionHost*>(h)->retryFactorisation(unpack(v)) ? 1 : 0; }
// the decision, and the row Window::solve would append to the iteration log for it (row6 untouched when the loop terminates)
int trlm_end(void* h, const double* v, double* row6) {
  auto* t = static_cast<svin::TrustRegionHost*>(h);
  const double muUsed = t->mu;
  const svin::TrustRegionHost::Outcome o = t->endIteration(unpack(v));
  if (o != svin::TrustRegionHost::kTerminated && row6) t->logRow(muUsed, o, row6);
  return (int)o;
}
// radius, mu, x_cost, reuse, initScale, invalid, iteration, successful, termination, muAfterAccept, decreaseFactor, stepRadius,
// strategy, initialRadius, maxRadius
void trlm_state(void* h, double* out) {
  auto* t = static_cast<svin::TrustRegionHost*>(h);
  out[0] = t->radius; out[1] = t->mu; out[2] = t->x_cost; out[3] = t->reuse; out[4] = t->initScale; out[5] = t->invalid;
  out[6] = t->iteration; out[7] = t->successful; out[8] = t->termination; out[9] = t->muAfterAccept();
  out[10] = t->decreaseFactor; out[11] = t->stepRadius(); out[12] = t->strategy; out[13] = t->initialRadius; out[14] = t->maxRadius;
}
// the step the kernels take from the radius the driver hands them: in = gHatSq jgSq gnHatSq gDotGn jySq jvDotJy jvDotR jyDotR radius
void trlm_dogleg(const double* in, double* out) {
  const svin::DoglegCoeff c = svin::doglegCoefficients(in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8]);
  out[0] = c.cg; out[1] = c.cn; out[2] = c.stepNorm; out[3] = c.jdSq; out[4] = c.jdDotR;
}
}
