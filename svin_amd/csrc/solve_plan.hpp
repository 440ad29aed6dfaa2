// svin_amd: host planning of the reduced solve (launchSolveReduced, kernels.hip) -- which of the ten launch sequences takes a
// reduced camera system, where every launch keeps its data in DeviceProblem::cholL, and the grid and dynamic LDS of every launch.
// HIP-free (tests/test_solve_plan_host.py runs it on the CPU through tests/csrc/solve_plan_shim.cpp); the launchers walk the
// plan and the kernels take their offsets into cholL from the layout functions below, so each expression is written once.
//
// The routes (d = unknowns of the system the dense solver takes, after the chain elimination if there is one):
//   kRouteLdsWhole            d <= 176                 k_chol_solve_lds<0>: the lower triangle in LDS
//   kRouteLdsBorderLoad       d = 177 .. 180, padded S k_chol_solve_lds<1>: 1-4 border rows eliminated while the tiles are loaded
//   kRouteLdsBorderPrepared   d = 181 .. 200, padded S k_chol_border_prepare + k_chol_solve_lds<2>: 5-24 border rows
//   kRouteLeftLooking         d <= 272 otherwise       k_chol_solve_ll: one workgroup, finished tiles written through to cholL
//   kRouteBlocked             d > 272                  k_big_load | k_sb_load, k_big_chol_chain, (k_big_back_gemv, k_big_back) per super-panel
// With the speed / bias chain eliminated first (k_sb_factor, k_sb_forward, k_sb_load, ..., k_sb_back: a chain of 8 .. 64 blocks
// behind a system the LDS-resident solver does not take whole) the kept dC rows go to the blocked solver's matrix (chain mode 1)
// or to a compact system S' | g' that one of the four one-workgroup routes takes (chain mode 2).
#pragma once
#include <cstddef>
#include "dmath.hpp"   // SVIN_HD
#include "tile_dims.hpp"   // kPanelLd

namespace svin {

// ---------------------------------------------------------------- constants the planning and the kernels share
constexpr int kTile = 16 * kPanelLd;     // doubles per tile
// LDS-resident solver
constexpr int kCholFlagInts = 48;
#ifdef SVIN_CHOL_TIMING
constexpr int kCholTimingDoubles = 240;  // (the timing build's stamp buffer, behind the flags and ahead of the border rows)
#else
constexpr int kCholTimingDoubles = 0;
#endif
constexpr int kCholLdsMaxTiles = 11;     // tile rows of the largest system LDS holds (156 KB)
constexpr size_t kCholLdsMaxBytes = 156 * 1024;
// its border variants.  Layout of the border scratch (doubles):
// V [32 x 176] | Lc^-1 [32 x 32, row-major, lower] | q [32] | g1 - B^T q [176] | tile-column mask [16]
constexpr int kBorderMaxRows = 24, kBorderLdV = 176;
constexpr int kBorderMP = 32, kBorderOffLinv = kBorderMP * kBorderLdV, kBorderOffQ = kBorderOffLinv + kBorderMP * kBorderMP,
              kBorderOffG = kBorderOffQ + kBorderMP /* g1 - B^T q, 176 */, kBorderOffMask = kBorderOffG + kBorderLdV /* 16: tile column J of V is not zero */,
              kBorderScratchDoubles = kBorderOffMask + 16;
#ifdef SVIN_BORDER_TIMING
constexpr int kBorderTimingDoubles = 8;  // (stamps of k_chol_border_prepare behind the scratch)
#else
constexpr int kBorderTimingDoubles = 0;
#endif
// left-looking solver: LDS slots of the live tiles
SVIN_HD constexpr int llHalf(int nT) { return (nT + 1) / 2; }
SVIN_HD constexpr int llSlots(int nT) { return (nT - llHalf(nT)) * llHalf(nT); }
SVIN_HD constexpr size_t llLdsDoubles(int nT) { return (size_t)llSlots(nT) * 256 + 2 * 256 + 16 * kPanelLd + 16 + 2 * 16 * nT; }
// blocked solver
constexpr int kNB = 64;
constexpr int kBigTileLd = kPanelLd;                 // 16 x 17 LDS tiles
constexpr int kBigBlockLds = 16 * 16 * kBigTileLd;   // a 64x64 block as 4x4 tiles
// Workgroups of one k_big_chol_chain: all must be co-resident (1 per CU: 104 KB of LDS each).  120 leaves room for a second
// solve of another handle / stream on the same GPU (2 x 120 <= 256 CUs); roots with more than kPersistWideTasks
// block tasks (> ~2000 unknowns) take the whole chip.
constexpr int kPersistMaxGrid = 120, kPersistWideGrid = 256, kPersistWideTasks = 512;
constexpr int kBackSpan = 512;           // columns of a super-panel of the backward substitution
// speed / bias chain
constexpr int kSbRec = 264, kSbG = 0, kSbFlo = 88, kSbFhi = 176;   // a block's record: G | F_lo | F_hi, 9x9 row-major each (16-byte aligned starts)
constexpr int kSbMaxChain = 64;          // k_sb_factor keeps the whole chain in LDS
constexpr int kSbMinChain = 8;           // shorter chains stay with the dense solvers (the four launches cost ~45 us before they gain anything)
constexpr int kSbLdsRec = 243;           // records in LDS: G | F_lo | F_hi back to back (an odd stride: eight blocks per wave, eight banks apart)
constexpr int kSbCols = 8;               // columns of [S_sk | g_s] per workgroup of k_sb_forward

// ---------------------------------------------------------------- layout of cholL, as the kernels index it
// blocked solver: M = cholL, (dp + kNB) x dp row-major, dp = the unknowns rounded up to kNB.  Row dp is the right-hand side; the
// rows behind it take the partial sums of k_big_back_gemv, one row per chunk of kBackSpan rows.
SVIN_HD constexpr size_t bigMatrixDoubles(int dp) { return (size_t)(dp + kNB) * dp; }
SVIN_HD constexpr size_t bigRhsOff(int dp) { return (size_t)dp * dp; }
// (the sum is formed in the caller's index type -- int in k_big_back's loop, unsigned blockIdx.y in k_big_back_gemv -- as it was
// when each kernel wrote the expression out, so that both compile to the instructions they compiled to then)
template <class Index>
SVIN_HD constexpr size_t bigPartialOff(int dp, Index chunk) { return (size_t)(dp + 1 + chunk) * dp; }
constexpr int bigReadyInts(int nb) { return (nb + 3) * nb; }   // block-ready flags
// everything the blocked solver keeps: the matrix | 1/L_ii (dp) | the factorised diagonal blocks (dp x kNB) | the flags (+ 2 spare)
constexpr size_t bigSolverDoubles(int dp) {
  return bigMatrixDoubles(dp) + (size_t)dp + (size_t)dp * kNB + ((size_t)bigReadyInts(dp / kNB) + 1) / 2 + 2;
}
constexpr int roundUpTo(int x, int m) { return (x + m - 1) / m * m; }
// doubles DeviceProblem::cholL must hold for a reduced system of d unknowns: the one-workgroup solvers' dpad x dpad area (border
// scratch / tiles written through) or the blocked solver's
// (withChain: room for the speed / bias chain elimination next to either solver -- the compact kept system, the chain's records,
// Y and t; a window's buffer is sized with it, the pose graph's root solve has no chain)
inline size_t solveReducedScratchDoubles(int d, bool withChain = false) {
  const size_t dpad = (size_t)roundUpTo(d, 16), big = bigSolverDoubles(roundUpTo(d, kNB));
  const size_t chain = withChain ? 2 * dpad * dpad + (dpad + 8) * (dpad + 32) + 64 * 264 + 64 : 0;
  return (dpad * dpad > big ? dpad * dpad : big) + chain;
}

// ---------------------------------------------------------------- the plan
enum DenseRoute : int { kRouteLdsWhole = 0, kRouteLdsBorderLoad = 1, kRouteLdsBorderPrepared = 2, kRouteLeftLooking = 3, kRouteBlocked = 4 };
struct SolveDims { int d, dC, sbChain, sPadded; };       // DeviceProblem's fields of these names
struct SolveSwitches { bool noLL, noSbElim, noLdsBorder; };   // SVIN_NO_LL, SVIN_NO_SB_ELIM, SVIN_NO_LDS_BORDER
struct ScratchRegion { size_t off, len; };               // doubles of cholL; len 0: the sequence does not use the region
struct PlannedLaunch { int grid; size_t ldsBytes; };      // grid 0: not part of the sequence
struct BackPanel { int c0, c1, blocks, nChunks; };       // a super-panel of the backward substitution: columns [c0, c1) = `blocks` column blocks, chunks of rows below

struct ReducedSolvePlan {
  int chainMode;       // 0: no chain elimination; 1: the kept rows go to the blocked solver's matrix; 2: to the compact S' | g'
  bool chainOverflow;  // the chain's regions did not fit the buffer and the plan fell back to chain mode 0 (no window size reaches this)
  // the dense solve of the system actually solved: the whole one, or the kept rows
  DenseRoute route;
  int dSolve;          // its unknowns (d, or dC behind a chain elimination)
  int dpad;            // the size the one-workgroup kernels are launched with: dSolve rounded up to 16, 176 with border rows
  int border;          // border rows of the LDS-resident solver
  int dp, nb;          // blocked solver: dSolve rounded up to kNB, and its block rows (0 otherwise)
  // the chain (chain mode 1 | 2): SbElimArgs' fields of these names
  int n, dK, ldY, rowsY, ldOut;
  int dpK;             // SbElimArgs::dp: dK rounded up to kNB (chain mode 1: the blocked matrix's dp)
  // regions of cholL
  ScratchRegion factor;      // left-looking solver: the finished tiles, written through
  ScratchRegion borderScr;   // k_chol_border_prepare -> k_chol_solve_lds<2>
  ScratchRegion bigM, dinvG, diagF, ready;   // blocked solver (ready: bigReadyInts(nb) ints)
  ScratchRegion compactS, compactG;          // chain mode 2: the kept system
  ScratchRegion Lf, Y, tvec, counter;        // the chain's records, Y, t and the ticket of k_sb_back (an int)
  size_t end;                // one past the last double any region takes
  // launches, in the order of the sequence
  PlannedLaunch sbFactor, sbForward, sbLoad;   // (sbLoad replaces bigLoad in chain mode 1 and precedes the compact solve in mode 2)
  PlannedLaunch borderPrepare, cholLds, cholLL;
  PlannedLaunch bigLoad, bigChain;
  int helperTasks;           // of k_big_chol_chain
  int nBackPanels;           // (k_big_back_gemv, k_big_back) pairs: backPanel(dp, 0 .. nBackPanels - 1)
  size_t bigBackLdsBytes;
  PlannedLaunch sbBack;
};

// LDS bytes of k_chol_solve_lds for nT tile rows (+ kBorderMP doubles of the border variants)
inline size_t cholLdsBytes(int nT) {
  return ((size_t)nT * (nT + 1) / 2 * kTile + 3 * 16 * nT) * 8 + kCholFlagInts * 4 + kCholTimingDoubles * 8 + kBorderMP * 8;
}
// rows beyond the LDS-resident solver's eleven tile rows that it eliminates first; needs the window's padded S
inline int cholBorderRows(int d, bool padded, const SolveSwitches& sw) {
  const int m = d - 16 * kCholLdsMaxTiles;
  return (padded && m >= 1 && m <= kBorderMaxRows && !sw.noLdsBorder) ? m : 0;
}
inline DenseRoute denseRoute(int d, bool padded, const SolveSwitches& sw) {
  const int nT = (d + 15) / 16, border = cholBorderRows(d, padded, sw);
  if (border > 4) return kRouteLdsBorderPrepared;
  if (border > 0) return kRouteLdsBorderLoad;
  if (cholLdsBytes(nT) <= kCholLdsMaxBytes) return kRouteLdsWhole;
  if (nT >= 12 && nT <= 17 && !sw.noLL) return kRouteLeftLooking;
  return kRouteBlocked;
}
// Whether the batched LDS-resident solver (k_chol_solve_lds_batch<0>, which has no border and no chain form) takes the WHOLE
// system: q.route alone does not say so -- behind a chain elimination it is the route of the kept rows
inline bool batchedSolverTakes(const ReducedSolvePlan& q) { return q.chainMode == 0 && q.route == kRouteLdsWhole; }
// super-panel k of the backward substitution (the last columns first)
inline BackPanel backPanel(int dp, int k) {
  const int c1 = dp - k * kBackSpan;
  const int c0 = c1 > kBackSpan ? c1 - kBackSpan : 0;
  return BackPanel{c0, c1, (c1 - c0) / kNB, k};   // k chunks of kBackSpan rows lie below: <= 63, the spare rows of the rhs block
}

// Whether the chain is eliminated ahead of the dense solve.  A system the LDS-resident solver takes whole is left alone (14 us at
// d = 150: the elimination's four launches cost more), and so is a chain of fewer than 8 blocks.
// Measured (tools/sb_elim_time.py, reduced solve with / without): d = 180 66 / 64 us, 240: 73 / 91, 270: 85 / 113, 360: 99 / 183,
// 600: 185 / 313, 960: 289 / 476.  (Tried and dropped: eliminating only the last blocks of a chain in ONE fused launch so that a
// system a few rows over the LDS-resident solver's limit drops into it: 39 + 35 + 10 us against the left-looking solver's 70.
// d = 177 .. 200 is now the LDS-resident solver's own border variant; the stereo_rig_v2 sliding window is d = 198.)
// (the compact form needed 16 blocks until the kept rows could go to the LDS-resident solver's border variants; with it taking
//  up to 200 rows a chain of 8 pays: config #3 -- chain of 10, 180 kept rows -- 112.6 -> 83.6 us, d = 210 / 225 (chains of
//  14 / 15) 80.9 -> 65.2 / 90.2 -> 65.6)
inline int chainModeOf(const SolveDims& m, const SolveSwitches& sw) {
  if (sw.noSbElim || m.sbChain < kSbMinChain || m.sbChain > kSbMaxChain || m.dC < 16 || m.dC + 9 * m.sbChain != m.d) return 0;
  if (denseRoute(m.d, m.sPadded != 0, sw) <= kRouteLdsBorderPrepared) return 0;
  return denseRoute(m.dC, false, sw) == kRouteBlocked ? 1 : 2;   // (asked without the border rows, which the compact S' would allow)
}

// forceBlocked: the blocked route whatever the size (chain mode 0 only) -- the one route whose factor stays behind in cholL
// (bigM, dinvG, diagF), for a caller that substitutes right-hand sides of its own (the pose graph's covariance pass)
inline ReducedSolvePlan planWithChainMode(const SolveDims& m, const SolveSwitches& sw, int mode, bool forceBlocked = false) {
  ReducedSolvePlan q{};
  q.chainMode = mode;
  q.dSolve = mode ? m.dC : m.d;
  const bool padded = mode == 2 || m.sPadded != 0;   // (the compact S' is padded)
  q.route = (mode == 1 || forceBlocked) ? kRouteBlocked : denseRoute(q.dSolve, padded, sw);
  const bool lds = q.route <= kRouteLdsBorderPrepared;
  q.border = lds ? cholBorderRows(q.dSolve, padded, sw) : 0;
  q.dpad = q.border ? 16 * kCholLdsMaxTiles : roundUpTo(q.dSolve, 16);
  const int nT = q.dpad / 16;
  size_t chainOff = 0;
  if (mode) {
    q.n = m.sbChain; q.dK = m.dC;
    q.dpK = roundUpTo(q.dK, kNB);
    q.ldY = roundUpTo(q.dK + 1, 16);
    q.rowsY = roundUpTo(9 * q.n, 4);
    const int nTk = (q.dK + 15) / 16;
    q.sbFactor = {1, ((size_t)q.n * 162 + (size_t)((q.n + 1) / 2) * kSbLdsRec) * 8};
    q.sbForward = {q.ldY / kSbCols, ((size_t)q.rowsY * kSbCols + (size_t)q.n * kSbLdsRec) * 8};
    q.sbLoad = {nTk * (nTk + 1) / 2 + nTk, 0};   // a tile of S' per workgroup, then 16 entries of g' each
    q.sbBack = {(9 * q.n + 15) / 16, ((size_t)q.n * kSbRec + 18 * (size_t)q.n) * 8};
  }
  if (mode == 2) {   // S' | g' behind the kept solver's own area
    const size_t dpadK = (size_t)roundUpTo(q.dK, 16);
    q.ldOut = (int)dpadK;
    q.compactS = {dpadK * dpadK, dpadK * dpadK};
    q.compactG = {2 * dpadK * dpadK, dpadK};
    chainOff = 2 * dpadK * dpadK + dpadK;
  }
  if (q.route == kRouteLdsBorderPrepared) {
    q.borderScr = {0, (size_t)kBorderScratchDoubles + kBorderTimingDoubles};
    q.borderPrepare = {1, 0};
  }
  if (lds) q.cholLds = {1, cholLdsBytes(q.border ? kCholLdsMaxTiles : nT)};
  if (q.route == kRouteLeftLooking) {
    q.factor = {0, (size_t)q.dpad * q.dpad};
    q.cholLL = {1, llLdsDoubles(nT) * 8};
  }
  if (q.route == kRouteBlocked) {
    q.dp = roundUpTo(q.dSolve, kNB);
    q.nb = q.dp / kNB;
    q.bigM = {0, bigMatrixDoubles(q.dp)};
    q.dinvG = {q.bigM.len, (size_t)q.dp};
    q.diagF = {q.dinvG.off + q.dinvG.len, (size_t)q.dp * kNB};   // per panel the factorised 64x64 diagonal block
    q.ready = {q.diagF.off + q.diagF.len, ((size_t)bigReadyInts(q.nb) + 1) / 2};
    if (mode == 1) chainOff = (bigSolverDoubles(q.dp) + 1) & ~(size_t)1;
    else q.bigLoad = {256, 0};
    for (int st = 0; st < q.nb; ++st) q.helperTasks += (q.nb - st - 1 > 0 ? q.nb - st - 1 : 0) + ((st + 2 <= q.nb - 1) ? 2 : 0);
    const int helpers = (q.helperTasks > kPersistWideTasks ? kPersistWideGrid : kPersistMaxGrid) - 1;
    q.bigChain = {1 + (q.helperTasks < 1 ? 1 : q.helperTasks < helpers ? q.helperTasks : helpers), ((size_t)3 * kBigBlockLds + kNB + 2) * 8};
    q.nBackPanels = (q.dp + kBackSpan - 1) / kBackSpan;
    q.bigBackLdsBytes = ((size_t)kBackSpan + 8 * 64 + kNB * (kNB + 1) + kNB) * 8;
  }
  q.end = q.factor.len > q.borderScr.len ? q.factor.len : q.borderScr.len;
  if (q.route == kRouteBlocked) q.end = q.ready.off + q.ready.len;
  if (mode) {
    q.Lf = {chainOff, (size_t)q.n * kSbRec};
    q.Y = {q.Lf.off + q.Lf.len, (size_t)q.rowsY * q.ldY};
    q.tvec = {q.Y.off + q.Y.len, (size_t)q.rowsY};
    q.counter = {q.tvec.off + q.tvec.len, 2};
    q.end = q.counter.off + q.counter.len;
  }
  return q;
}

// The plan of the reduced solve of a system with these dimensions.  The chain is eliminated only where its regions fit the buffer
// a window allocates (solveReducedScratchDoubles(d, true)).
inline ReducedSolvePlan planReducedSolve(const SolveDims& m, const SolveSwitches& sw) {
  const int mode = chainModeOf(m, sw);
  ReducedSolvePlan q = planWithChainMode(m, sw, mode);
  if (mode && q.end > solveReducedScratchDoubles(m.d, true)) {
    q = planWithChainMode(m, sw, 0);
    q.chainOverflow = true;
  }
  return q;
}

}  // namespace svin
