// C entry points over svin_amd/csrc/marg_plan.hpp (the host planning of the marginalisation) for tests/test_marg_plan_host.py
// through tests/helpers/marg_plan_lib.py.  mp_plan takes rows of 13 ints -- MargDims' eleven fields in their order, margEig,
// jacobiShared -- and hands every plan over as mp_fields() 64-bit integers in the order of marg_plan_lib.FIELDS.
#include <cstdint>
#include <initializer_list>
#include "../../svin_amd/csrc/marg_plan.hpp"

extern "C" {
int mp_fields() { return 2 + 2 * 2 + 2 + 3 * 2 + 2 + 4 + 3 * 2 + 4 + 18 + 4 + 2 * 22; }
void mp_plan(int rows, const int32_t* in, int64_t* out) {
  using namespace svin;
  const int nf = mp_fields();
  for (int r = 0; r < rows; ++r) {
    const int32_t* a = in + (size_t)13 * r;
    const MargDims d{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]};
    const MargPlan q = planMargJob(d, MargSwitches{a[11]}, MargKernelSizes{(size_t)a[12]});
    int64_t* o = out + (size_t)nf * r;
    int k = 0;
    auto launch = [&](const PlannedLaunch& l) { o[k++] = l.grid; o[k++] = (int64_t)l.ldsBytes; };
    o[k++] = q.reproj; o[k++] = q.factors;
    launch(q.accumLm); launch(q.accumFactors);
    o[k++] = q.accumCamX; o[k++] = q.accumCamY;
    launch(q.lmPrepare); launch(q.lmApply); launch(q.lmUpdate);
    launch(q.dense);
    o[k++] = q.denseUseLds; o[k++] = q.denseProdLds; o[k++] = q.denseTileChol; o[k++] = q.copyPair;
    launch(q.finalChol); launch(q.finalDc); launch(q.final);
    o[k++] = q.finalDcAfterChol; o[k++] = q.finalMode; o[k++] = q.finalFallbackLds; o[k++] = q.finalSkipIfDone;
    for (size_t v : {q.bU, q.bW2, q.bV, q.bVec, q.bScratch, q.bHk, q.bOut, q.bLin, q.bFacLin, q.bPartial, q.bFlag, q.bScal, q.gLm, q.gUv,
                     q.gW, q.gLmPtr, q.gObsLm, q.gIdx})
      o[k++] = (int64_t)v;
    for (size_t v : {q.clearU, q.clearW2, q.clearV, q.clearVec}) o[k++] = (int64_t)v;
    for (const MargRegion& g : {q.ba, q.bb, q.vb, q.linR, q.linJp, q.linJl, q.linJe, q.Vm, q.Qm, q.denseTmp, q.Hk, q.bk, q.oldH, q.oldB0,
                                q.G, q.Q, q.J, q.Ht, q.e0, q.bp, q.scal, q.finalTmp}) {
      o[k++] = (int64_t)g.off;
      o[k++] = (int64_t)g.len;
    }
    if (k != nf) out[0] = -1;   // (the helper checks the first plan's first field: a bool)
  }
}
// 0 jacobiLdsBytes, 1 jacobiLdsBytesGOnly, 2 margCholLdsBytes, 3 symEigLdsBytes, 4 jacobiLdsLimit, 5 jacobiLd, 6 margGatherScratchInts
int64_t mp_lds(int which, int n, int jacobiShared) {
  using namespace svin;
  switch (which) {
    case 0: return (int64_t)jacobiLdsBytes(n, jacobiShared);
    case 1: return (int64_t)jacobiLdsBytesGOnly(n, jacobiShared);
    case 2: return (int64_t)margCholLdsBytes(n);
    case 3: return (int64_t)symEigLdsBytes(n);
    case 4: return (int64_t)jacobiLdsLimit(jacobiShared);
    case 5: return jacobiLd(n);
    default: return (int64_t)margGatherScratchInts(n);
  }
}
// kJacobiRegLen, kPanelLd, kSymEigMaxN, kMargLdsPerWorkgroup
int64_t mp_constant(int which) {
  const int64_t c[4] = {svin::kJacobiRegLen, svin::kPanelLd, svin::kSymEigMaxN, (int64_t)svin::kMargLdsPerWorkgroup};
  return c[which];
}
// ids / isKeyframe: n frames, oldest first.  out: enough, then the three lists, each as its length and its entries (room for 4 + 3 n)
void mp_select_frames(int n, const uint64_t* ids, const uint8_t* isKeyframe, int numKeyframes, int numImuFrames, int64_t* out) {
  const std::vector<uint64_t> v(ids, ids + n);
  const std::vector<char> kf(isKeyframe, isKeyframe + n);
  const svin::MargFrames f = svin::selectMargFrames(v, kf, (size_t)numKeyframes, (size_t)numImuFrames);
  int k = 0;
  out[k++] = f.enough ? 1 : 0;
  for (const std::vector<uint64_t>* l : {&f.removeFrames, &f.removeAllButPose, &f.allLinearizedFrames}) {
    out[k++] = (int64_t)l->size();
    for (uint64_t id : *l) out[k++] = (int64_t)id;
  }
}
}
