// Host-side planning of Window::pack(), HIP-free: which Schur form a window takes and what that form's kernels are told to do --
// the landmark order of wide windows, the per-chunk observation order, the speed / bias chain test, the slots of the
// block-pair form and the work lists of k_schur_rows and k_schur_panels.  Pure integer logic over flat arrays: debug options
// and the compute-unit count arrive as plain arguments that pack() reads once.  The kernels trust every invariant of these lists
// without checking them (kernels.hip, the comment above SVIN_ROWS_RD; kernels.hpp, DeviceProblem::blk*).
// Included by kernels.hpp / window.cpp and by tests/csrc/pack_plan_shim.cpp, tests/csrc/pack_plan_sanitize.cpp (g++, no GPU).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "batch_plan.hpp"
#include "tile_dims.hpp"

namespace svin {

constexpr int kDensePoseCap = 256;   // k_schur_dense stages the pose -> row map of at most this many poses in LDS

// wide windows: 16-landmark chunks one workgroup of k_schur_panels works through (the host builds the work list: buildSchurPanelsWorkList).
// Config #4 on one GPU, 8 / 12 / 16: k_schur_panels 523 / 545 / 551 us, k_reduce_panel_slabs (one 74 KB slab per workgroup) 45 / 25 /
// 19 us -- a wash on one GPU, and a rank of an 8-GPU run has an eighth of the chunks: 8 keeps its ~210 workgroups from becoming ~105.
#ifndef SVIN_PANEL_CHUNKS
#define SVIN_PANEL_CHUNKS 8
#endif
constexpr int kPanelChunksPerBlock = SVIN_PANEL_CHUNKS;
// block-pair form (round 6): entries (landmark x panel pair) per workgroup of k_schur_rows, its waves (the host deals the block
// rows of a panel pair to them), records a batch stages in LDS (x 20 doubles = 160 bytes: two buffers of 36.8 KB, two workgroups
// per CU; the last record of a buffer is never staged: all zero, the B operand of the padding pairs), pair words per wave and batch
constexpr int kBlkMinWordsPerBlock = 1024;    // pair words per workgroup, at least (buildSchurRowsWorkList cuts the work list by words)
constexpr int kBlkWaves = 8;
constexpr int kBlkBatchRecs = 230;
constexpr int kBlkBatchWords = 128;
constexpr int kBlkRec = 18;                   // doubles per slot record: E_la (6 x 3), rec[6 k + row]
#ifndef SVIN_SLOTS_PER_WG
#define SVIN_SLOTS_PER_WG 1024
#endif
constexpr int kBlkSlotsPerWorkgroup = SVIN_SLOTS_PER_WG;   // slots (one thread each, four trips) per workgroup of k_blocks_slots
constexpr int kBlkMaxPoseBlocks = 512;      // the per-pose accumulators of k_blocks_slots live in LDS (28 doubles per pose block)

// ---- the Schur form of a window and its slab count
struct SchurForm {
  bool schurDense;    // narrow window: dense Gram-matrix Schur complement on MFMA (k_schur_dense)
  bool schurPanels;   // wide window with fixed extrinsics: per pair of 96-row panels (k_schur_panels / k_schur_rows)
  bool schurBlocks;   // ... in the block-pair form (k_blocks_slots + k_schur_rows)
  bool orderObs;      // dense form with the A part on MFMA: the observations of a chunk are visited pose by pose
  bool useLds;        // pairwise form: a slab fits the LDS
  int nSlabs;
};
// nPoses: pose slots of the window (a phantom pose not counted); optSlabChunks: SVIN_SLAB_CHUNKS (0: unset)
inline SchurForm chooseSchurForm(int dC, int L, int N, int nPoses, bool anyExtVar, bool optSchurPairwise, bool optPanelsOld, int optSlabChunks) {
  SchurForm f;
  f.useLds = pairwiseSlabFitsLds(dC);   // (tile_dims.hpp: the launcher's own test)
  f.nSlabs = 1;
  // windows whose camera block fits 16 x 16 MFMA tiles (dC <= 254, e.g. 42 poses or 10 poses with per-frame extrinsics):
  // dense Gram-matrix Schur complement on MFMA
  f.schurDense = dC > 0 && dC + 2 <= 256 && nPoses <= kDensePoseCap && !optSchurPairwise;
  if (f.schurDense) {
    f.nSlabs = denseSlabCount(L);   // (batch_plan.hpp)
    // SVIN_SLAB_CHUNKS=n: n chunks of 16 landmarks per workgroup and private slab (default 1 up to 256 workgroups)
    if (optSlabChunks > 1) f.nSlabs = std::max(1, std::min(f.nSlabs, ((L + 15) / 16 + optSlabChunks - 1) / optSlabChunks));
  }
  else if (f.useLds) f.nSlabs = std::max(1, std::min(256, (L + 7) / 8));
  // dense Schur with the A part on MFMA (variable extrinsics, or more than 8 tile rows): within every chunk of 16
  // landmarks the observations are visited pose by pose, so that a batch only touches a few tile rows (counting sort)
  f.orderObs = f.schurDense && (anyExtVar || (dC + 2 + 15) / 16 > 8) && N > 0;
  // wide windows with fixed extrinsics: Gram-matrix Schur complement per pair of 96-row panels (k_schur_panels).
  f.schurPanels = !f.schurDense && !anyExtVar && dC > 0 && L > 0 && !optSchurPairwise;
  // Round 6: the block-pair form (k_schur_blocks) is what runs unless SVIN_PANELS_OLD keeps the tile form (k_schur_panels).
  // A pose block index has to fit 16 bits.
  f.schurBlocks = f.schurPanels && !optPanelsOld && dC / 6 <= kBlkMaxPoseBlocks;
  return f;
}

// ---- landmark order of wide windows (k_schur_panels): order by VISIBILITY SIGNATURE -- the set of 16-row tiles of the camera
// matrix a landmark's observations write to (first tile, last tile, then the bit pattern) -- so that the 16 landmarks of a chunk
// hit the same tile rows and the kernel's step masks drop whole products.  A product step (tile row, tile column, 4 columns of G)
// runs when both tile rows hold something in those columns; modelled on the host (tools/panel_order_model.py) for the bench
// window of configs[3]: executed / algorithmic MFMA flops 9.28 ordered by first pose (measured 9.3), 7.84 by (first, last)
// pose, 6.30 by signature.  The rest is granularity: a landmark there sees 9 poses scattered over a span of 28 (its 55 rows
// live in ~8 tiles of 16), which no order of the landmarks changes.
// offPtr / off: per landmark (CSR) the reduced-row offset of the pose of each of its observations (-1: a fixed pose).
// Returns the permutation: place i of the new order holds landmark perm[i] of the old one (stable).
inline std::vector<int> orderLandmarksBySignature(const std::vector<int>& offPtr, const std::vector<int>& offs) {
  struct Key { int first, last; uint64_t lo, hi; int lm; };
  const int n = (int)offPtr.size() - 1;
  std::vector<Key> keyed;
  keyed.reserve((size_t)std::max(n, 0));
  for (int l = 0; l < n; ++l) {
    Key k{INT32_MAX, -1, 0, 0, l};
    for (int o = offPtr[l]; o < offPtr[l + 1]; ++o) {
      const int off = offs[o];
      if (off < 0) continue;
      for (int tr : {off >> 4, (off + 5) >> 4}) {
        k.first = std::min(k.first, tr); k.last = std::max(k.last, tr);
        if (tr < 64) k.lo |= 1ull << tr; else if (tr < 128) k.hi |= 1ull << (tr - 64);
      }
    }
    if (k.last < 0) k.first = 0;
    keyed.push_back(k);
  }
  std::stable_sort(keyed.begin(), keyed.end(), [](const Key& a, const Key& b) {
    if (a.first != b.first) return a.first < b.first;
    if (a.last != b.last) return a.last < b.last;
    if (a.hi != b.hi) return a.hi < b.hi;
    return a.lo < b.lo;
  });
  std::vector<int> perm(keyed.size());
  for (size_t i = 0; i < keyed.size(); ++i) perm[i] = keyed[i].lm;
  return perm;
}

// ---- dense Schur with the A part on MFMA: within every chunk of 16 landmarks the observations sorted by pose slot (counting
// sort per chunk; its device twin is phase 4 of k_window_rebuild).  obsIdx: packed observation indices (pose slot in bits 0-11).
inline std::vector<int> chunkObservationOrder(const std::vector<int>& lmPtr, const std::vector<uint32_t>& obsIdx, int L, int nPoseSlots) {
  std::vector<int> order(obsIdx.size());
  std::vector<int> cnt;
  for (int l0 = 0; l0 < L; l0 += 16) {
    const int oBeg = lmPtr[l0], oEnd = lmPtr[std::min(L, l0 + 16)];
    cnt.assign((size_t)nPoseSlots + 2, 0);
    for (int o = oBeg; o < oEnd; ++o) cnt[(obsIdx[o] & 0xfff) + 1]++;
    for (size_t k = 1; k < cnt.size(); ++k) cnt[k] += cnt[k - 1];
    for (int o = oBeg; o < oEnd; ++o) order[oBeg + cnt[obsIdx[o] & 0xfff]++] = o;
  }
  return order;
}

// ---- Do the variable speed / bias blocks form a chain behind the kept rows -- every factor (of ANY rank: the all-reduced system
// holds them all) and the prior tying two of them only ties neighbours in the order of the rows?  Then the wide-window solver
// eliminates them ahead of its blocked Cholesky (kernels.hip, k_sb_factor ...).  Returns the length of the chain, 0 without one.
// sbOff: reduced-row offset per speed / bias slot (-1: fixed); facPtr / facSlots: per factor (CSR) the slots of its variable
// blocks that are neither poses nor extrinsics; priorSlots: the same list for the prior.
inline int speedBiasChainLength(const std::vector<int>& sbOff, int dC, int d, const std::vector<int>& facPtr,
                                const std::vector<int>& facSlots, const std::vector<int>& priorSlots) {
  std::vector<int> chainPos(sbOff.size(), -1);
  int n = 0;
  bool ok = true;
  for (size_t i = 0; i < sbOff.size(); ++i)
    if (sbOff[i] >= 0) { ok = ok && sbOff[i] == dC + 9 * n; chainPos[i] = n++; }
  auto neighbours = [&](const int* pos, int cnt) {
    for (int x = 0; x < cnt; ++x)
      for (int y = x + 1; y < cnt; ++y) ok = ok && (pos[x] - pos[y] == 1 || pos[y] - pos[x] == 1);
  };
  std::vector<int> pos;
  for (size_t f = 0; f + 1 < facPtr.size(); ++f) {
    pos.clear();
    for (int k = facPtr[f]; k < facPtr[f + 1]; ++k) pos.push_back(chainPos[facSlots[k]]);
    neighbours(pos.data(), (int)pos.size());
  }
  pos.clear();
  for (int sl : priorSlots) pos.push_back(chainPos[sl]);
  neighbours(pos.data(), (int)pos.size());
  return (ok && d == dC + 9 * n) ? n : 0;
}

// ---- The tile skyline of the reduced system for the LDS-resident solver (kernels.hip k_chol_solve_lds_body<0>): hi[k] = the last
// tile row of tile column k (16-row tiling of the padded system) that can hold a non-zero, so that the factorisation leaves the
// tiles below it alone.  Structure: the camera part (rows < dC: landmarks couple any two poses / extrinsics) is one dense clique;
// every factor couples all of its variable blocks pairwise, and so does the prior -- each is a CLIQUE, a list of row ranges
// (cliquePtr: CSR over blkOff / blkLen; fixed blocks are left out by the caller).  Locked rows only lose entries.
// `pre` is the profile of S as the build leaves it, `hi` the one the factorisation keeps: for k ascending column k eliminates into
// rows k+1 .. hi[k] only, so each of those columns reaches at least as far down (skyline fill).  hi[k] >= k always.
// recognised = false (a factor of unknown kind, a host-evaluated factor, any caller that has no block lists) or a system of more
// than kTileSkylineMaxTiles tile rows: the dense profile.  `cut` / `cutPre` carry the profiles in DeviceProblem: nibble k =
// nT - 1 - hi[k], so that 0 -- a cleared problem -- is the dense profile.
constexpr int kTileSkylineMaxTiles = 11;   // (= kCholLdsMaxTiles, solve_plan.hpp: the largest system the LDS-resident solver holds)
struct TileSkyline {
  int nT;
  int hi[kTileSkylineMaxTiles], pre[kTileSkylineMaxTiles];
  uint64_t cut, cutPre;
};
inline uint64_t packTileCut(const int* hi, int nT) {
  uint64_t w = 0;
  for (int k = 0; k < nT && k < kTileSkylineMaxTiles; ++k) w |= (uint64_t)(nT - 1 - hi[k]) << (4 * k);
  return w;
}
inline int tileHiOf(uint64_t cut, int nT, int k) { return nT - 1 - (int)((cut >> (4 * k)) & 15); }
inline TileSkyline planTileSkyline(int d, int dC, const std::vector<int>& cliquePtr, const std::vector<int>& blkOff,
                                   const std::vector<int>& blkLen, bool recognised) {
  TileSkyline t{};
  const int nT = (std::max(d, 0) + 15) / 16;
  t.nT = nT;
  if (nT > kTileSkylineMaxTiles) return t;   // (not a system of the LDS-resident solver: nothing reads the profile)
  for (int k = 0; k < nT; ++k) t.pre[k] = k;
  bool ok = recognised && dC >= 0 && dC <= d;
  auto addClique = [&](uint32_t tiles) {   // bit I: the clique has a row in tile row I
    if (!tiles) return;
    int top = 0;
    for (int I = 0; I < nT; ++I) if ((tiles >> I) & 1) top = I;
    for (int J = 0; J < nT; ++J) if ((tiles >> J) & 1) t.pre[J] = std::max(t.pre[J], top);
  };
  auto tilesOf = [&](int off, int len) {
    uint32_t m = 0;
    if (off < 0 || len <= 0 || off + len > d) { ok = ok && len <= 0; return m; }
    for (int I = off / 16; I <= (off + len - 1) / 16; ++I) m |= 1u << I;
    return m;
  };
  if (ok && dC > 0) addClique(tilesOf(0, dC));
  for (size_t c = 0; ok && c + 1 < cliquePtr.size(); ++c) {
    uint32_t m = 0;
    if (cliquePtr[c] < 0 || cliquePtr[c + 1] < cliquePtr[c] || (size_t)cliquePtr[c + 1] > blkOff.size() || blkLen.size() != blkOff.size()) { ok = false; break; }
    for (int k = cliquePtr[c]; k < cliquePtr[c + 1]; ++k) m |= tilesOf(blkOff[k], blkLen[k]);
    addClique(m);
  }
  if (!ok) for (int k = 0; k < nT; ++k) t.pre[k] = nT - 1;
  for (int k = 0; k < nT; ++k) t.hi[k] = t.pre[k];
  for (int k = 0; k < nT; ++k)
    for (int r = k + 1; r <= t.hi[k]; ++r) t.hi[r] = std::max(t.hi[r], t.hi[k]);
  t.cut = packTileCut(t.hi, nT);
  t.cutPre = packTileCut(t.pre, nT);
  return t;
}

// ---- The deal of the tile rows I >= 2 to the waves of the LDS-resident solver (kernels.hip k_chol_solve_lds_body<0>: wave 0 is the
// serial chain and owns rows 0 and 1; waves 1-3 and 5-7 are the owners; wave 4, the quiet wave, shares SIMD 0 with wave 0).
// The closed form (tileDealBaseOwner) gives rows nT-1 .. nT-6 one per owner -- waves 1, 2, 3, 7, 6, 5, so that the waves w and w + 4
// of one SIMD hold the longest row with the shortest -- and rows 2 .. nT-7 to the quiet wave, where their products come out of wave
// 0's matrix pipe.  Inside a skyline, row I has work in the columns first[I] .. I-2 only, first[I] = min{k : hi[k] >= I}: a long row
// starts late, a quiet-wave row ends early, and an owner whose own rows are idle in a row's columns takes it at no cost to itself.
// planTileDeal moves each row of the quiet wave, longest first, to the owner whose rows start latest among those whose work
// intervals are all disjoint from the row's (ties: the owner of the longer row); a row no owner is free for stays where it is.  No
// owner ever has two rows with work in one column, and a row keeps its owner for the whole factorisation (one writer per flag).
// `word` carries the deal in DeviceProblem::tileDeal: nibble I = the wave of a row that MOVED, 0 = the closed form for this row, so
// that a cleared problem, the dense profile and every nT <= 7 (no row on the quiet wave) keep the closed form unchanged.
constexpr int kTileDealQuietWave = 4;
constexpr int tileDealBaseOwner(int nT, int I) {   // I >= 2
  return nT - 1 - I >= 6 ? kTileDealQuietWave : (nT - 1 - I < 3 ? nT - I : 11 - nT + I);   // r = nT - 1 - I: r + 1 | 10 - r
}
// the rows of wave w in the closed form, bit I (the kernel starts from this mask and walks the non-zero nibbles of the word alone:
// decoding row by row cost every wave ~250 scalar instructions ahead of the load barrier, 1.8 k cycles of the solve)
constexpr unsigned tileDealBaseRows(int nT, int w) {
  return w == kTileDealQuietWave ? (nT >= 9 ? ((1u << (nT - 6)) - 1u) & ~3u : 0u)
                                 : (w < 1 || w > 7 || nT - (w < 4 ? w : 11 - w) < 2 ? 0u : 1u << (nT - (w < 4 ? w : 11 - w)));
}
inline int tileDealOwnerOf(uint64_t word, int nT, int I) {
  const int nib = (int)((word >> (4 * I)) & 15);
  return nib ? nib : tileDealBaseOwner(nT, I);
}
struct TileDeal {
  int owner[kTileSkylineMaxTiles];   // wave of tile row I (0 for rows 0, 1 and beyond nT: wave 0's, or none)
  uint64_t word;
};
inline TileDeal planTileDeal(int nT, const int* hi) {
  TileDeal t{};
  if (nT < 2 || nT > kTileSkylineMaxTiles) return t;
  int first[kTileSkylineMaxTiles];
  for (int I = 0; I < nT; ++I) {
    first[I] = I;
    for (int k = I; k >= 0; --k) if (hi[k] >= I) first[I] = k;
  }
  for (int I = 2; I < nT; ++I) t.owner[I] = tileDealBaseOwner(nT, I);
  // [first[a], a - 2] and [first[b], b - 2] share a column (an empty interval shares none)
  auto meet = [&](int a, int b) { return std::max(first[a], first[b]) <= std::min(a, b) - 2; };
  for (int I = nT - 7; I >= 2; --I) {
    int best = 0, bestStart = -1, bestRow = -1;
    for (int w = 1; w < 8; ++w) {
      if (w == kTileDealQuietWave) continue;
      bool free = true;
      int baseRow = -1;
      for (int J = 2; J < nT; ++J) {
        if (t.owner[J] != w) continue;
        free = free && !meet(I, J);
        baseRow = std::max(baseRow, J);
      }
      if (!free || baseRow < 0) continue;
      if (first[baseRow] > bestStart || (first[baseRow] == bestStart && baseRow > bestRow)) { best = w; bestStart = first[baseRow]; bestRow = baseRow; }
    }
    if (best) { t.owner[I] = best; t.word |= (uint64_t)best << (4 * I); }
  }
  return t;
}
inline TileDeal planTileDeal(int nT, uint64_t cut) {   // from the profile as DeviceProblem::tileCut carries it
  int hi[kTileSkylineMaxTiles] = {};
  for (int k = 0; k < nT && k < kTileSkylineMaxTiles; ++k) hi[k] = tileHiOf(cut, nT, k);
  return planTileDeal(nT, hi);
}

// ---- the SLOTS of the block-pair form -- one per (landmark, distinct variable pose), ascending with the pose inside a landmark,
// each with the list of its observations (two for a stereo pair) -- are structure, built once per pack(); k_blocks_slots writes a
// 24-double record per slot and build.
// (A landmark-prior pseudo-observation carries pose slot 0 in its packed index: it gets a slot at pose 0 when that pose is
// variable.  Its Jacobians are zero, so the slot only adds zeros.)
struct SchurSlots {
  std::vector<int> slotPtr;              // per landmark: first slot (L + 1 entries)
  std::vector<unsigned short> slotBlk;   // per slot: pose block of the reduced camera system (poseOff / 6)
  std::vector<int> slotObsPtr;           // per slot: its observations (nSlots + 1 entries into slotObs)
  std::vector<int> slotObs;              // observation numbers
  std::vector<int> slotLm;               // per slot: its landmark
};
inline SchurSlots buildSchurSlots(const std::vector<int>& lmPtr, const std::vector<uint32_t>& obsIdx, const std::vector<int>& poseOff, int L) {
  SchurSlots s;
  const size_t N = obsIdx.size();
  s.slotPtr.resize((size_t)L + 1); s.slotObs.reserve(N); s.slotBlk.reserve(N); s.slotObsPtr.reserve(N + 1);
  struct Seen { int first, second; };   // (pose block, observation) of one landmark
  std::vector<Seen> seen;
  for (int l = 0; l < L; ++l) {
    s.slotPtr[l] = (int)s.slotBlk.size();
    seen.clear();
    for (int o = lmPtr[l]; o < lmPtr[l + 1]; ++o) {
      const int off = poseOff[obsIdx[o] & 0xfff];
      if (off >= 0) seen.push_back(Seen{off / 6, o});
    }
    std::stable_sort(seen.begin(), seen.end(), [](const Seen& a, const Seen& b) { return a.first < b.first; });
    for (size_t k = 0; k < seen.size(); ++k) {
      if (k == 0 || seen[k].first != seen[k - 1].first) { s.slotBlk.push_back((unsigned short)seen[k].first); s.slotObsPtr.push_back((int)s.slotObs.size()); s.slotLm.push_back(l); }
      s.slotObs.push_back(seen[k].second);
    }
  }
  s.slotPtr[L] = (int)s.slotBlk.size();
  s.slotObsPtr.push_back((int)s.slotObs.size());
  return s;
}

// ---- the work list of k_schur_rows
struct SchurRowsWorkList {
  std::vector<uint32_t> pairWords;   // DeviceProblem::blkPairs (+ 128 zero words: a wave requests its words in 64s)
  std::vector<int> batch;            // blkBatch: per batch first entry of recSlot, records (+ three zero descriptors)
  std::vector<int> waveTab;          // blkWaveTab: per (batch, wave) first pair word, words of its first / second row, 0 (+ 3 x kBlkWaves zero descriptors)
  std::vector<int> recSlot;          // blkRecSlot: per staged record its slot
  std::vector<int> panelWork;        // per workgroup: panel I, panel J, first batch, batches
  std::vector<int> blkOwn;           // per workgroup four ints: the two block rows of wave w in bytes 2 w, 2 w + 1 (255: none)
  std::vector<int> panelPairPtr;     // per panel pair: first workgroup (nPanelPairs + 1 entries)
  int nPanelBlocks = 0, nPanelPairs = 0;
  size_t balWgMax = 0, balWgAll = 0, balAll = 0, balMax = 0;   // pair words of the busiest wave / of all waves: per workgroup, per batch (a barrier pair per batch)
  bool fits = true;                  // false: an entry does not fit a batch (the list is unusable)
};
// work list: per panel pair (I >= J; a panel is 16 pose blocks = 96 rows) the landmarks with slots in both panels, as ENTRIES
// (first slot and count in either panel -- the slots of a panel are a run, they ascend with the pose), cut into workgroups of
// pair words (below); the pairs in the order k_reduce_panel_slabs expects (panelPairPtr).
// computeUnits: of the device; blkRounds: SVIN_BLK_ROUNDS (0: unset, the default 2); rowSplit: heavy rows get a second accumulator set.
// The three-batch / 128-word tail of zeros is part of the result: the kernel reads ahead unconditionally.
inline SchurRowsWorkList buildSchurRowsWorkList(const SchurSlots& slots, int dC, int L, int computeUnits, int blkRounds, bool rowSplit) {
  SchurRowsWorkList w;
  const std::vector<int>& hSlotPtr = slots.slotPtr;
  const std::vector<unsigned short>& hSlotBlk = slots.slotBlk;
  const int nPan = (dC + 95) / 96;
  w.nPanelPairs = nPan * (nPan + 1) / 2;
  std::vector<std::vector<int>> lists((size_t)w.nPanelPairs);   // four ints per entry: first slot in I, in J, counts, landmark
  std::vector<int> runPanel, runFirst, runCount;
  for (int l = 0; l < L; ++l) {
    runPanel.clear(); runFirst.clear(); runCount.clear();
    for (int sl = hSlotPtr[l]; sl < hSlotPtr[l + 1]; ++sl) {
      const int pan = hSlotBlk[sl] / 16;
      if (runPanel.empty() || runPanel.back() != pan) { runPanel.push_back(pan); runFirst.push_back(sl); runCount.push_back(1); }
      else ++runCount.back();
    }
    for (size_t a = 0; a < runPanel.size(); ++a)
      for (size_t b = 0; b <= a; ++b) {
        std::vector<int>& li = lists[runPanel[a] * (runPanel[a] + 1) / 2 + runPanel[b]];
        li.insert(li.end(), {runFirst[a], runFirst[b], runCount[a] | (runCount[b] << 8), l});
      }
  }
  // ... and for k_schur_rows (kernels.hip), per panel pair: the sixteen block rows dealt to the kernel's eight waves (two each, by
  // their pair counts, heaviest first, per workgroup), the entries cut into workgroups by pair words and those into BATCHES (records
  // staged in LDS at a time: at most kBlkBatchRecs, and at most kBlkBatchWords pair words per wave), and per batch and wave the
  // PAIR WORDS (pairWord below) in the order the wave works through them, its first row's, then
  // its second row's, each sorted by A record (entry, slot in I); the run of an A record is padded to an even length and a row's
  // words to whole eights with pairs whose B operand is the zero record (the kernel takes the A record of words 2 j, 2 j + 1 from
  // word 2 j, and words 2 j, 2 j + 1 must name two accumulators).  A diagonal pair takes the blocks on and below the block diagonal.
  // Workgroups: cut by PAIR WORDS (an entry of a pair of different panels has 17 pairs on the bench window of configs[3], one of a
  // diagonal pair 12), so many that SVIN_BLK_ROUNDS (default 2) workgroups per place run one after the other -- two places per
  // CU.  (900 workgroups of 256 entries: 181 us; one round of equal entry counts: 233 us, the heaviest workgroup is the kernel.)
  // (pair word: twice the accumulator's number | byte offset of the B record in its LDS buffer << 8 | A record << 24 -- what the
  // kernel needs with the fewest scalar instructions; a staged record is 160 bytes)
  auto pairWord = [](int recA, int recB, int pb) { return (uint32_t)(2 * pb) | ((uint32_t)(recB * 160) << 8) | ((uint32_t)recA << 24); };
  static_assert(kBlkBatchRecs <= 256 && kBlkBatchRecs * 160 < 65536, "pair word fields");
  auto entryWords = [&](const int* en, bool dg) {
    const int nA = en[2] & 0xff, nB = en[2] >> 8;
    int wds = 0;
    for (int ka = 0; ka < nA; ++ka) wds += ((dg ? ka + 1 : nB) + 1) & ~1;
    return wds;
  };
  size_t wordsPerWg = 0;
  {
    size_t total = 0;
    for (int I = 0; I < nPan; ++I)
      for (int J = 0; J <= I; ++J) {
        const std::vector<int>& li = lists[I * (I + 1) / 2 + J];
        for (size_t e = 0; e < li.size() / 4; ++e) total += entryWords(&li[4 * e], I == J);
      }
    const int rounds = blkRounds > 0 ? blkRounds : 2;
    const size_t places = (size_t)std::max(1, rounds * 2 * computeUnits - w.nPanelPairs);
    wordsPerWg = std::max<size_t>(kBlkMinWordsPerBlock, (total + places - 1) / places);
  }
  w.panelPairPtr.push_back(0);
  for (int I = 0; I < nPan; ++I)
    for (int J = 0; J <= I; ++J) {
      const std::vector<int>& li = lists[I * (I + 1) / 2 + J];
      const size_t nEnt = li.size() / 4;
      const bool dg = I == J;
      for (size_t k = 0; k < nEnt;) {
        size_t kEnd = k, wgWords = 0;
        while (kEnd < nEnt && wgWords < wordsPerWg) wgWords += entryWords(&li[4 * kEnd++], dg);
        // The workgroup's block rows dealt to the sixteen accumulator sets of its eight waves (two each).  Rows no landmark of the
        // list touches get none; the sets that are left go to the heaviest rows as a SECOND set (the row's runs are then shared
        // between two waves -- by the lighter wave of the moment, below -- and k_schur_rows adds both sets into the slab image:
        // two terms, so the sum does not depend on their order).  Sets heaviest first, to the wave with the least so far.
        // (round 6, measured on the bench window: one set per row and rows dealt by load left the busiest wave of a batch with
        //  1.59 x the mean number of pair words and the busiest wave of a workgroup with 1.24 x; rows r, r + 8 to wave r: 1.71;
        //  entries re-ordered round robin by the wave they load most: 1.57)
        long rowLoad[16] = {0};
        for (size_t e = k; e < kEnd; ++e) {
          const int fa = li[4 * e], nA = li[4 * e + 2] & 0xff, nB = li[4 * e + 2] >> 8;
          for (int ka = 0; ka < nA; ++ka) rowLoad[hSlotBlk[fa + ka] - 16 * I] += ((dg ? ka + 1 : nB) + 1) & ~1;
        }
        int nOwn[16] = {0}, ownerWave[16][2], ownerSel[16][2], ownRows[kBlkWaves][2];
        long waveLoad[kBlkWaves] = {0};
        for (int wvv = 0; wvv < kBlkWaves; ++wvv) ownRows[wvv][0] = ownRows[wvv][1] = 255;
        {
          int mult[16], sets = 0;
          for (int r = 0; r < 16; ++r) { mult[r] = rowLoad[r] > 0 ? 1 : 0; sets += mult[r]; }
          const bool split = rowSplit;
          while (split && sets < 2 * kBlkWaves) {
            int best = -1;
            for (int r = 0; r < 16; ++r)
              if (mult[r] == 1 && rowLoad[r] >= 16 && (best < 0 || rowLoad[r] > rowLoad[best])) best = r;
            if (best < 0) break;
            mult[best] = 2; ++sets;
          }
          struct Unit { int row; long load; };
          std::vector<Unit> units;
          for (int r = 0; r < 16; ++r)
            for (int c = 0; c < mult[r]; ++c) units.push_back(Unit{r, rowLoad[r] / mult[r]});
          std::stable_sort(units.begin(), units.end(), [](const Unit& a, const Unit& b) { return a.load > b.load; });
          for (const Unit& u : units) {
            int best = -1;
            for (int wvv = 0; wvv < kBlkWaves; ++wvv) {
              if (ownRows[wvv][1] != 255) continue;
              if (nOwn[u.row] == 1 && ownerWave[u.row][0] == wvv) continue;   // (the two sets of a row: two waves)
              if (best < 0 || waveLoad[wvv] < waveLoad[best]) best = wvv;
            }
            if (best < 0) continue;   // (only the second set of a row can be left over: the row keeps its first)
            const int sel = ownRows[best][0] == 255 ? 0 : 1;
            ownRows[best][sel] = u.row;
            ownerWave[u.row][nOwn[u.row]] = best; ownerSel[u.row][nOwn[u.row]] = sel; ++nOwn[u.row];
            waveLoad[best] += u.load;
          }
        }
        {
          long mx = 0, sum = 0;
          for (int wvv = 0; wvv < kBlkWaves; ++wvv) { mx = std::max(mx, waveLoad[wvv]); sum += waveLoad[wvv]; }
          w.balWgMax += (size_t)mx; w.balWgAll += (size_t)sum;
        }
        int ownWords[4] = {0, 0, 0, 0};
        for (int wvv = 0; wvv < kBlkWaves; ++wvv)
          ownWords[wvv >> 1] |= (ownRows[wvv][0] | (ownRows[wvv][1] << 8)) << (16 * (wvv & 1));
        const int firstBatch = (int)(w.batch.size() / 2);
        size_t e = k;
        while (e < kEnd) {
          std::vector<uint32_t> words[kBlkWaves][2];   // per wave and owned row
          const int firstRec = (int)w.recSlot.size();
          int recs = 0;
          for (; e < kEnd; ++e) {
            const int fa = li[4 * e], fb = li[4 * e + 1], nA = li[4 * e + 2] & 0xff, nB = li[4 * e + 2] >> 8;
            const int need = nA + (dg ? 0 : nB);
            if (recs + need > kBlkBatchRecs - 1) break;
            int add[kBlkWaves] = {0};   // (every run of an A record is padded to an even number of words)
            int pick[64];               // which of its row's sets the run of slot ka goes to: the wave with fewer words in this batch
            for (int ka = 0; ka < nA; ++ka) {
              const int row = hSlotBlk[fa + ka] - 16 * I;
              int c = 0;
              if (nOwn[row] == 2) {
                const int w0 = ownerWave[row][0], w1 = ownerWave[row][1];
                const size_t l0 = words[w0][0].size() + words[w0][1].size() + (size_t)add[w0], l1 = words[w1][0].size() + words[w1][1].size() + (size_t)add[w1];
                c = l1 < l0 ? 1 : 0;
              }
              pick[ka] = c;
              add[ownerWave[row][c]] += ((dg ? ka + 1 : nB) + 1) & ~1;
            }
            bool fits = true;
            for (int wvv = 0; wvv < kBlkWaves; ++wvv) fits = fits && (int)(words[wvv][0].size() + words[wvv][1].size()) + add[wvv] <= kBlkBatchWords - 12;
            if (!fits) break;
            const int recA0 = recs, recB0 = dg ? recs : recs + nA;
            for (int ka = 0; ka < nA; ++ka) w.recSlot.push_back(fa + ka);
            if (!dg) for (int kb = 0; kb < nB; ++kb) w.recSlot.push_back(fb + kb);
            recs += need;
            for (int ka = 0; ka < nA; ++ka) {
              const int row = hSlotBlk[fa + ka] - 16 * I;
              std::vector<uint32_t>& wl = words[ownerWave[row][pick[ka]]][ownerSel[row][pick[ka]]];
              const int cnt = dg ? ka + 1 : nB;
              int pb = 0;
              for (int kb = 0; kb < cnt; ++kb) {
                pb = hSlotBlk[fb + kb] - 16 * J;
                wl.push_back(pairWord(recA0 + ka, recB0 + kb, pb));
              }
              // (padding word of the run: the zero record as B, an accumulator other than its partner's)
              if (cnt & 1) wl.push_back(pairWord(recA0 + ka, kBlkBatchRecs - 1, (pb + 1) & 15));
            }
          }
          if (recs == 0) { w.fits = false; return w; }   // (an entry does not fit a batch: pack() throws)
          w.batch.insert(w.batch.end(), {firstRec, recs});
          {
            size_t mx = 0;
            for (int wvv = 0; wvv < kBlkWaves; ++wvv) { const size_t n = words[wvv][0].size() + words[wvv][1].size(); w.balAll += n; mx = std::max(mx, n); }
            w.balMax += mx;
          }
          for (int wvv = 0; wvv < kBlkWaves; ++wvv) {
            for (int sel = 0; sel < 2; ++sel)   // (a row's words in eights: padding words in twos -- both operands the zero record, two accumulators)
              while (words[wvv][sel].size() % 8) {
                words[wvv][sel].push_back(pairWord(kBlkBatchRecs - 1, kBlkBatchRecs - 1, 0));
                words[wvv][sel].push_back(pairWord(kBlkBatchRecs - 1, kBlkBatchRecs - 1, 1));
              }
            w.waveTab.insert(w.waveTab.end(), {(int)w.pairWords.size(), (int)words[wvv][0].size(), (int)words[wvv][1].size(), 0});
            w.pairWords.insert(w.pairWords.end(), words[wvv][0].begin(), words[wvv][0].end());
            w.pairWords.insert(w.pairWords.end(), words[wvv][1].begin(), words[wvv][1].end());
          }
        }
        w.panelWork.insert(w.panelWork.end(), {I, J, firstBatch, (int)(w.batch.size() / 2) - firstBatch});
        w.blkOwn.insert(w.blkOwn.end(), ownWords, ownWords + 4);   // (blkOwn: one int4 per workgroup)
        ++w.nPanelBlocks;
        k = kEnd;
      }
      w.panelPairPtr.push_back(w.nPanelBlocks);
    }
  w.pairWords.resize(w.pairWords.size() + 128, 0u);   // (a wave requests its words in 64s)
  w.batch.resize(w.batch.size() + 2 * 3, 0); w.waveTab.resize(w.waveTab.size() + (size_t)4 * kBlkWaves * 3, 0);   // (the kernel reads descriptors three batches ahead, unconditionally)
  return w;
}

// ---- the older tile form (k_schur_panels, SVIN_PANELS_OLD).  Work list: every chunk of 16 landmarks goes to all panel pairs
// (I >= J) inside the row range its observations touch.
struct SchurPanelsWorkList {
  std::vector<int> panelWork;      // per workgroup: panel I, panel J, first chunk entry, chunk count
  std::vector<int> panelChunks;    // chunk ids (16 landmarks each)
  std::vector<int> panelPairPtr;   // per panel pair: first workgroup (nPanelPairs + 1 entries)
  int nPanelBlocks = 0, nPanelPairs = 0;
};
inline SchurPanelsWorkList buildSchurPanelsWorkList(const std::vector<int>& lmPtr, const std::vector<uint32_t>& obsIdx, const std::vector<int>& poseOff, int dC, int L) {
  SchurPanelsWorkList w;
  constexpr int kRows = 96, kChunk = 16, kPerBlock = kPanelChunksPerBlock;
  const int nPan = (dC + kRows - 1) / kRows;
  w.nPanelPairs = nPan * (nPan + 1) / 2;
  std::vector<std::vector<int>> lists((size_t)w.nPanelPairs);
  const int nChunks = (L + kChunk - 1) / kChunk;
  for (int c = 0; c < nChunks; ++c) {
    int lo = INT32_MAX, hi = -1;
    const int o0 = lmPtr[c * kChunk], o1 = lmPtr[std::min(L, (c + 1) * kChunk)];
    for (int o = o0; o < o1; ++o) {
      const int off = poseOff[obsIdx[o] & 0xfff];
      if (off < 0) continue;
      lo = std::min(lo, off); hi = std::max(hi, off);
    }
    // a chunk without variable poses still has to produce V^-1, b, htil for its landmarks: give it to pair (0, 0)
    const int pLo = hi < 0 ? 0 : lo / kRows, pHi = hi < 0 ? 0 : hi / kRows;
    for (int I = pLo; I <= pHi; ++I)
      for (int J = pLo; J <= I; ++J) lists[I * (I + 1) / 2 + J].push_back(c);
  }
  w.panelPairPtr.push_back(0);
  for (int I = 0; I < nPan; ++I)
    for (int J = 0; J <= I; ++J) {
      const std::vector<int>& li = lists[I * (I + 1) / 2 + J];
      for (size_t k = 0; k < li.size(); k += kPerBlock) {
        const int cnt = (int)std::min<size_t>(kPerBlock, li.size() - k);
        w.panelWork.insert(w.panelWork.end(), {I, J, (int)w.panelChunks.size(), cnt});
        w.panelChunks.insert(w.panelChunks.end(), li.begin() + k, li.begin() + k + cnt);
        ++w.nPanelBlocks;
      }
      w.panelPairPtr.push_back(w.nPanelBlocks);
    }
  return w;
}

}  // namespace svin
