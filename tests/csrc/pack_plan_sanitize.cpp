// A stand-alone run of svin_amd/csrc/pack_plan.hpp (the host planning of Window::pack) for AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_pack_plan_host.py compiles this file with -fsanitize=address,undefined
// -fno-sanitize-recover=all and requires exit status 0.  The inputs are the three of that test -- A (43 pose blocks, ragged
// tracks, stereo pairs, fixed poses, landmarks without a slot), B (every landmark seen from all 48 poses: batches end at the word
// limit), C (two poses in different panels: batches end at the record limit) -- generated here from a fixed seed; every function
// of the header runs on each, the list builders with the row split on and off and at several CU counts.  What the arrays must
// hold is the Python test's business; here only their sizes are cross-checked so that nothing is optimised away.
#include <cstdio>
#include "../../svin_amd/csrc/pack_plan.hpp"

namespace {
struct Rng {   // (64-bit LCG, Knuth's constants: the high bits)
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};
struct Input {
  std::vector<int> lmPtr{0}, poseOff;
  std::vector<uint32_t> obsIdx;
  int dC = 0;
  int L() const { return (int)lmPtr.size() - 1; }
  void poses(int n, int fixedA = -1, int fixedB = -1) {
    for (int i = 0; i < n; ++i) {
      if (i == fixedA || i == fixedB) poseOff.push_back(-1);
      else { poseOff.push_back(dC); dC += 6; }
    }
  }
  void observe(int pose, int cam) { obsIdx.push_back((uint32_t)pose | ((uint32_t)cam << 24)); }
  void endLandmark() { lmPtr.push_back((int)obsIdx.size()); }
};

Input inputA(uint64_t seed) {
  Input in;
  Rng r{seed};
  in.poses(45, 7, 30);
  for (int l = 0; l < 600; ++l) {
    if (l % 60 == 17) { in.observe(7, 0); in.observe(30, 0); in.observe(30, 1); in.endLandmark(); continue; }
    const int first = r.below(44), span = std::min(28, 45 - first), k = std::min(2 + r.below(8), span);
    std::vector<int> p((size_t)span);
    for (int i = 0; i < span; ++i) p[(size_t)i] = first + i;
    for (int i = 0; i < k; ++i) {   // (a partial shuffle: the observations come in no particular order)
      std::swap(p[(size_t)i], p[(size_t)(i + r.below(span - i))]);
      in.observe(p[(size_t)i], 0);
      if (r.below(3) == 0) in.observe(p[(size_t)i], 1);
    }
    in.endLandmark();
  }
  return in;
}
Input inputB() {
  Input in;
  in.poses(48);
  for (int l = 0; l < 64; ++l) {
    for (int p = 0; p < 48; ++p) in.observe(p, 0);
    in.endLandmark();
  }
  return in;
}
Input inputC(uint64_t seed) {
  Input in;
  Rng r{seed};
  in.poses(49);
  for (int l = 0; l < 3000; ++l) {
    const int pa = r.below(4), pb = (pa + 1 + r.below(3)) % 4;
    in.observe(pa == 3 ? 48 : 16 * pa + r.below(16), 0);
    in.observe(pb == 3 ? 48 : 16 * pb + r.below(16), 0);
    in.endLandmark();
  }
  return in;
}

long long run(const Input& in, const int* cus, int nCus) {
  using namespace svin;
  const int L = in.L(), N = (int)in.obsIdx.size(), nPose = (int)in.poseOff.size();
  long long sum = 0;
  for (int opt = 0; opt < 8; ++opt) {
    const SchurForm f = chooseSchurForm(in.dC, L, N, nPose, (opt & 1) != 0, (opt & 2) != 0, (opt & 4) != 0, opt);
    sum += f.nSlabs + f.schurDense + 2 * f.schurPanels + 4 * f.schurBlocks + 8 * f.orderObs + 16 * f.useLds;
  }
  std::vector<int> offPtr{0}, offs;
  for (int l = 0; l < L; ++l) {
    for (int o = in.lmPtr[(size_t)l]; o < in.lmPtr[(size_t)l + 1]; ++o) offs.push_back(in.poseOff[in.obsIdx[(size_t)o] & 0xfff]);
    offPtr.push_back((int)offs.size());
  }
  sum += (long long)orderLandmarksBySignature(offPtr, offs).size();
  sum += (long long)chunkObservationOrder(in.lmPtr, in.obsIdx, L, nPose).size();
  const SchurSlots slots = buildSchurSlots(in.lmPtr, in.obsIdx, in.poseOff, L);
  sum += (long long)slots.slotBlk.size();
  for (int c = 0; c < nCus; ++c)
    for (int split = 0; split < 2; ++split)
      for (int rounds = 0; rounds < 4; rounds += 3) {
        const SchurRowsWorkList w = buildSchurRowsWorkList(slots, in.dC, L, cus[c], rounds, split != 0);
        if (!w.fits || w.waveTab.size() != w.batch.size() / 2 * 4 * kBlkWaves || w.panelWork.size() != (size_t)4 * w.nPanelBlocks ||
            w.blkOwn.size() != w.panelWork.size() || w.panelPairPtr.size() != (size_t)w.nPanelPairs + 1) {
          std::fprintf(stderr, "k_schur_rows work list: inconsistent sizes\n");
          return -1;
        }
        sum += (long long)w.pairWords.size() + (long long)w.balAll + (long long)w.balMax + (long long)w.balWgAll + (long long)w.balWgMax;
      }
  const SchurPanelsWorkList old = buildSchurPanelsWorkList(in.lmPtr, in.obsIdx, in.poseOff, in.dC, L);
  if (old.panelWork.size() != (size_t)4 * old.nPanelBlocks || old.panelPairPtr.size() != (size_t)old.nPanelPairs + 1) return -1;
  return sum + (long long)old.panelChunks.size();
}

// the chain test: ten blocks tied by neighbour factors and a prior over the first two; one factor across; a fixed block; no blocks
long long runChain() {
  using namespace svin;
  long long sum = 0;
  for (int variant = 0; variant < 4; ++variant) {
    std::vector<int> sbOff, facPtr{0}, facSlots, prior{0, 1};
    int d = 60;
    const int n = variant == 3 ? 0 : 10;
    for (int i = 0; i < n; ++i) {
      if (variant == 2 && i == 4) sbOff.push_back(-1);
      else { sbOff.push_back(d); d += 9; }
    }
    for (int i = 0; i + 1 < n; ++i) {
      for (int s : {i, i + 1})
        if (sbOff[(size_t)s] >= 0) facSlots.push_back(s);
      facPtr.push_back((int)facSlots.size());
    }
    if (variant == 1) { facSlots.push_back(0); facSlots.push_back(2); facPtr.push_back((int)facSlots.size()); }
    if (n == 0) prior.clear();
    sum = 16 * sum + speedBiasChainLength(sbOff, 60, d, facPtr, facSlots, prior);
  }
  return sum;   // 10, 0, 9, 0
}
}  // namespace

int main() {
  const int cuA[2] = {4, 256}, cuB[1] = {256}, cuC[2] = {1, 8};
  long long total = 0;
  const struct { Input in; const int* cus; int nCus; const char* name; } cases[] = {
      {inputA(1), cuA, 2, "A"}, {inputA(2), cuA, 2, "A'"}, {inputB(), cuB, 1, "B"}, {inputC(3), cuC, 2, "C"}, {Input{}, cuB, 1, "empty"}};
  for (const auto& c : cases) {
    const long long s = run(c.in, c.cus, c.nCus);
    if (s < 0) return 1;
    std::printf("%s: %d landmarks, %zu observations, dC %d: %lld\n", c.name, c.in.L(), c.in.obsIdx.size(), c.in.dC, s);
    total += s;
  }
  const long long ch = runChain();
  std::printf("chains: %llx\n", ch);
  if (ch != 0xa090) return 1;
  return total > 0 ? 0 : 1;
}
