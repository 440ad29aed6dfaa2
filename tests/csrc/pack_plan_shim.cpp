// C entry points over svin_amd/csrc/pack_plan.hpp (the host planning of Window::pack) for tests/test_pack_plan_host.py: the
// choice of the Schur form, the landmark and observation orders, the speed / bias chain test, the slots and the work lists of
// k_schur_rows / k_schur_panels are HIP-free, so what the kernels need of them is checked on the CPU.
// A builder's result is handed over as a list of int32 arrays behind a handle (pp_count / pp_len / pp_get / pp_free).
#include "../../svin_amd/csrc/pack_plan.hpp"

namespace {
struct Arrays { std::vector<std::vector<int32_t>> v; };
template <class T>
std::vector<int32_t> widen(const std::vector<T>& a) {
  std::vector<int32_t> out(a.size());
  for (size_t i = 0; i < a.size(); ++i) out[i] = (int32_t)a[i];
  return out;
}
std::vector<int> vec(const int* p, int n) { return std::vector<int>(p, p + n); }
svin::SchurSlots slotsOf(int L, const int* lmPtr, const uint32_t* obsIdx, int N, const int* poseOff, int nPose) {
  return svin::buildSchurSlots(vec(lmPtr, L + 1), std::vector<uint32_t>(obsIdx, obsIdx + N), vec(poseOff, nPose), L);
}
}  // namespace

extern "C" {
// kBlkMinWordsPerBlock, kBlkWaves, kBlkBatchRecs, kBlkBatchWords, kBlkRec, kBlkSlotsPerWorkgroup, kBlkMaxPoseBlocks, kPanelChunksPerBlock, kDensePoseCap
int pp_constant(int which) {
  const int c[9] = {svin::kBlkMinWordsPerBlock, svin::kBlkWaves, svin::kBlkBatchRecs, svin::kBlkBatchWords, svin::kBlkRec,
                    svin::kBlkSlotsPerWorkgroup, svin::kBlkMaxPoseBlocks, svin::kPanelChunksPerBlock, svin::kDensePoseCap};
  return c[which];
}
// out: schurDense, schurPanels, schurBlocks, orderObs, useLds, nSlabs
void pp_choose_form(int dC, int L, int N, int nPoses, int anyExtVar, int pairwise, int panelsOld, int slabChunks, int* out) {
  const svin::SchurForm f = svin::chooseSchurForm(dC, L, N, nPoses, anyExtVar != 0, pairwise != 0, panelsOld != 0, slabChunks);
  out[0] = f.schurDense; out[1] = f.schurPanels; out[2] = f.schurBlocks; out[3] = f.orderObs; out[4] = f.useLds; out[5] = f.nSlabs;
}
void pp_order_landmarks(int n, const int* offPtr, const int* offs, int* perm) {
  const std::vector<int> p = svin::orderLandmarksBySignature(vec(offPtr, n + 1), vec(offs, offPtr[n]));
  for (int i = 0; i < n; ++i) perm[i] = p[(size_t)i];
}
void pp_chunk_order(int L, const int* lmPtr, const uint32_t* obsIdx, int N, int nPoseSlots, int* order) {
  const std::vector<int> o = svin::chunkObservationOrder(vec(lmPtr, L + 1), std::vector<uint32_t>(obsIdx, obsIdx + N), L, nPoseSlots);
  for (int i = 0; i < N; ++i) order[i] = o[(size_t)i];
}
int pp_sb_chain(int nSb, const int* sbOff, int dC, int d, int nFac, const int* facPtr, const int* facSlots, int nPrior, const int* priorSlots) {
  return svin::speedBiasChainLength(vec(sbOff, nSb), dC, d, vec(facPtr, nFac + 1), vec(facSlots, facPtr[nFac]), vec(priorSlots, nPrior));
}
// arrays: slotPtr, slotBlk, slotObsPtr, slotObs, slotLm
void* pp_slots(int L, const int* lmPtr, const uint32_t* obsIdx, int N, const int* poseOff, int nPose) {
  const svin::SchurSlots s = slotsOf(L, lmPtr, obsIdx, N, poseOff, nPose);
  return new Arrays{{s.slotPtr, widen(s.slotBlk), s.slotObsPtr, s.slotObs, s.slotLm}};
}
// arrays: pairWords, batch, waveTab, recSlot, panelWork, blkOwn, panelPairPtr, {nPanelBlocks, nPanelPairs, fits}, {balWgMax, balWgAll, balAll, balMax}
void* pp_rows(int L, const int* lmPtr, const uint32_t* obsIdx, int N, const int* poseOff, int nPose, int dC, int computeUnits, int blkRounds, int rowSplit) {
  const svin::SchurSlots s = slotsOf(L, lmPtr, obsIdx, N, poseOff, nPose);
  const svin::SchurRowsWorkList w = svin::buildSchurRowsWorkList(s, dC, L, computeUnits, blkRounds, rowSplit != 0);
  return new Arrays{{widen(w.pairWords), w.batch, w.waveTab, w.recSlot, w.panelWork, w.blkOwn, w.panelPairPtr,
                     {w.nPanelBlocks, w.nPanelPairs, w.fits ? 1 : 0},
                     {(int32_t)w.balWgMax, (int32_t)w.balWgAll, (int32_t)w.balAll, (int32_t)w.balMax}}};
}
// arrays: panelWork, panelChunks, panelPairPtr, {nPanelBlocks, nPanelPairs}
void* pp_panels(int L, const int* lmPtr, const uint32_t* obsIdx, int N, const int* poseOff, int nPose, int dC) {
  const svin::SchurPanelsWorkList w =
      svin::buildSchurPanelsWorkList(vec(lmPtr, L + 1), std::vector<uint32_t>(obsIdx, obsIdx + N), vec(poseOff, nPose), dC, L);
  return new Arrays{{w.panelWork, w.panelChunks, w.panelPairPtr, {w.nPanelBlocks, w.nPanelPairs}}};
}
int pp_count(void* h) { return (int)static_cast<Arrays*>(h)->v.size(); }
int pp_len(void* h, int k) { return (int)static_cast<Arrays*>(h)->v[(size_t)k].size(); }
void pp_get(void* h, int k, int32_t* out) {
  const std::vector<int32_t>& a = static_cast<Arrays*>(h)->v[(size_t)k];
  std::copy(a.begin(), a.end(), out);
}
void pp_free(void* h) { delete static_cast<Arrays*>(h); }
}
