// svin_amd: host planning of the marginalisation (Window::applyMarginalizationStrategy and launchMarginalization, marg.hip) --
// which frames leave, the grid and dynamic LDS of every launch of the job M1-M3, what every job buffer must hold and where each
// launch keeps its data in it.  HIP-free (tests/test_marg_plan_host.py runs it on the CPU through tests/csrc/marg_plan_shim.cpp);
// the reservations and the launcher read the plan and the kernels take their LDS row lengths from the functions below, so each
// expression is written once.
//
// The job (m dense rows = nk kept + nm marginalised, Lm marginalised landmarks, N reprojection residuals, F small factors):
//   M1  launchEvalReproj, k_marg_accum_lm, k_marg_accum_cam     N > 0: linearise and accumulate U | ba | W | V | bb in a fixed order
//       launchEvalFactors, k_marg_accum_factors                 F > 0
//   M2  k_marg_lm_prepare, k_marg_lm_apply, k_marg_lm_update    Lm > 0 and m > 0: U -= W V^+ W^T, ba -= W V^+ bb
//       k_marg_dense                                            nk > 0 and nm > 0: (Hk | bk) = Schur complement of the marginalised rows
//       two device-to-device copies                             nk > 0 and nm == 0: (Hk | bk) = (U | ba)
//   M3  k_marg_final_chol, k_marg_final_dc, k_marg_final        nk > 0: H = J^T J, e0; which of the three run: SVIN_MARG_EIG
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "dmath.hpp"       // SVIN_HD
#include "solve_plan.hpp"  // PlannedLaunch
#include "tile_dims.hpp"   // kPanelLd, kSymEigMaxN

namespace svin {

// ---------------------------------------------------------------- constants and LDS sizes the planning and the kernels share
constexpr int kJacobiRegLen = 144;   // columns up to this (padded) length are held in registers by their lane group
// row length of the LDS images: the column length rounded up to the lane-group size (the tail is kept zero, so the
// register path needs no predication), odd so that the columns of a round start on different banks
SVIN_HD int jacobiLd(int n) { return ((n + 15) & ~15) | 1; }
// 160 KB per workgroup less the static __shared__ scalars of the Jacobi kernels (jacobiShared = sizeof(JacobiShared), which only
// the kernels' translation unit knows)
constexpr size_t kMargLdsPerWorkgroup = 160 * 1024;
constexpr size_t jacobiLdsLimit(size_t jacobiShared) { return 158 * 1024 - jacobiShared; }
// G and Q of the one-sided Jacobi (0: they do not fit)
inline size_t jacobiLdsBytes(int n, size_t jacobiShared) {
  const size_t b = (size_t)2 * n * jacobiLd(n) * sizeof(double);
  return b <= jacobiLdsLimit(jacobiShared) ? b : 0;
}
// G alone, its columns in registers (0: no)
inline size_t jacobiLdsBytesGOnly(int n, size_t jacobiShared) {
  const size_t b = (size_t)n * jacobiLd(n) * sizeof(double);
  return b <= jacobiLdsLimit(jacobiShared) && n <= kJacobiRegLen ? b : 0;
}
// the tile Cholesky of k_marg_dense / k_marg_final_chol: the image (NP x (NP + 1)) | nT scratch tiles | 1 / L_ii
inline size_t margCholLdsBytes(int n) {
  const size_t nT = ((size_t)n + 15) / 16, NP = 16 * nT;
  return (NP * (NP + 1) + nT * 16 * kPanelLd + NP) * sizeof(double);
}
// the direct solver (symeig.hpp): the n x (n | 1) image
inline size_t symEigLdsBytes(int n) { return (size_t)n * (n | 1) * sizeof(double); }

// ---------------------------------------------------------------- which frames leave (Estimator.cpp:499-540)
// ids / isKeyframe: the window's frames, oldest first.  enough == false: fewer states than the IMU window, nothing to do.
struct MargFrames {
  bool enough;
  std::vector<uint64_t> removeFrames, removeAllButPose, allLinearizedFrames;   // newest first, as the reference collects them
};
inline MargFrames selectMargFrames(const std::vector<uint64_t>& ids, const std::vector<char>& isKeyframe, size_t numKeyframes,
                                   size_t numImuFrames) {
  MargFrames f;
  f.enough = numImuFrames == 0 || ids.size() > numImuFrames;
  if (!f.enough) return f;
  size_t countedKeyframes = 0;
  for (size_t i = ids.size() - numImuFrames; i-- > 0;) {   // :529-538, behind the newest numImuFrames
    if (!isKeyframe[i] || countedKeyframes >= numKeyframes) f.removeFrames.push_back(ids[i]);
    else countedKeyframes++;
    f.removeAllButPose.push_back(ids[i]);
    f.allLinearizedFrames.push_back(ids[i]);
  }
  return f;
}

// ---------------------------------------------------------------- the plan of the job
struct MargDims {
  int m, Lm, N, F;           // dense rows, marginalised landmarks, reprojection residuals, small factors
  int nk, nm;                // dense rows that stay (the new prior) / that are marginalised
  int nPose, nExt, nCam;     // pose / extrinsics blocks and cameras of the job's tables
  int anyExtVar;             // an extrinsics block has rows of its own
  int oldPriorM;             // rows of the prior this job builds on (0: none)
};
struct MargSwitches { int margEig; };               // SVIN_MARG_EIG: 0 default, 1 "direct", 2 "cholesky", 3 "jacobi" (options.hpp)
struct MargKernelSizes { size_t jacobiShared; };    // sizeof(JacobiShared)
struct MargRegion { size_t off, len; };             // doubles of a job buffer; len 0: the job does not use the region

struct MargPlan {
  // ---- launches (grid 0: not part of the job)
  bool reproj, factors;                   // launchEvalReproj / launchEvalFactors ahead of their accumulation kernels
  PlannedLaunch accumLm, accumFactors;
  int accumCamX, accumCamY;               // k_marg_accum_cam: (camera-side block, part)
  PlannedLaunch lmPrepare, lmApply, lmUpdate;
  PlannedLaunch dense;                    // k_marg_dense ...
  int denseUseLds, denseProdLds, denseTileChol;
  bool copyPair;                          // ... or (Hk | bk) = (U | ba) by two copies
  PlannedLaunch finalChol, finalDc, final;
  int finalDcAfterChol;                   // k_marg_final_dc: k_marg_final_chol runs ahead of it
  int finalMode, finalFallbackLds, finalSkipIfDone;   // k_marg_final's useLds / fallbackLds / skipIfDone
  // ---- what the job buffers must hold (elements; 0: not reserved by this job)
  size_t bU, bW2, bV, bVec, bScratch, bHk, bOut, bLin, bFacLin, bPartial, bFlag, bScal;
  size_t gLm, gUv, gW, gLmPtr, gObsLm, gIdx;   // the tables k_window_marg_gather writes (device-gathered job)
  // ---- regions
  size_t clearU, clearW2, clearV, clearVec;    // the zeroed prefix of each accumulator (the clears ride in the staged block)
  MargRegion ba, bb, vb;                       // bVec
  MargRegion linR, linJp, linJl, linJe;        // bLin
  MargRegion Vm, Qm, denseTmp;                 // bScratch
  MargRegion Hk, bk;                           // bHk: what M2 leaves
  MargRegion oldH, oldB0;                      // bHk as the previous job left it (read before this job writes Hk)
  MargRegion G, Q, J, Ht, e0, bp, scal, finalTmp;   // bOut
};

// ints of Resident::margScratch for a resident window of L landmarks
constexpr size_t margGatherScratchInts(int residentL) { return (size_t)2 * residentL > 1 ? (size_t)2 * residentL : 1; }

inline MargPlan planMargJob(const MargDims& d, const MargSwitches& sw, const MargKernelSizes& ks) {
  MargPlan q{};
  const auto atLeast1 = [](size_t v) { return v > 1 ? v : (size_t)1; };
  const int m = d.m, Lm = d.Lm, N = d.N, F = d.F, nk = d.nk, nm = d.nm;
  const size_t mm = atLeast1(m), L3 = atLeast1((size_t)3 * Lm), n2 = (size_t)nk * nk;
  const size_t limit = jacobiLdsLimit(ks.jacobiShared);
  // ---- M1
  q.reproj = N > 0;
  if (q.reproj) {
    q.accumLm = {(Lm + 63) / 64, 0};
    q.accumCamX = d.nPose + d.nExt; q.accumCamY = d.anyExtVar ? 1 + d.nCam : 1;
  }
  q.factors = F > 0;
  if (q.factors) q.accumFactors = {1, 0};
  // ---- M2, landmark part
  if (Lm > 0 && m > 0) {
    q.lmPrepare = {(Lm + 127) / 128, 0};
    q.lmApply = {m, 0};
    q.lmUpdate = {((m + 15) / 16) * ((m + 15) / 16), 0};
  }
  if (nk > 0) {
    // ---- M2, dense part
    if (nm > 0) {
      const size_t ldsEig = jacobiLdsBytes(nm, ks.jacobiShared);
      const size_t ldsProd = sizeof(double) * ((size_t)2 * nk * nm + (size_t)nm * nm);   // W, Mu, N^T of the products
      const bool prodLds = ldsProd <= limit;
      const size_t ldsTile = margCholLdsBytes(nm);   // the certified Cholesky route of the pseudo-inverse, on tiles
      const bool tileChol = ldsTile <= limit;
      size_t lds = ldsEig;
      if (prodLds && ldsProd > lds) lds = ldsProd;
      if (tileChol && ldsTile > lds) lds = ldsTile;
      q.dense = {1, lds};
      q.denseUseLds = ldsEig ? 1 : 0; q.denseProdLds = prodLds ? 1 : 0; q.denseTileChol = tileChol ? 1 : 0;
    } else {
      q.copyPair = true;
    }
    // ---- M3.  Eigen-solver of the prior (k_marg_final's `useLds`):
    //   4  A + delta I = R^T R, one-sided Jacobi on the rows of R, image in LDS (default: n <= 136)
    //   6  the same with the image in global memory (larger priors)
    //   1 / 0  the ONE fall-back: one-sided Jacobi on A itself with G and Q in LDS (n <= 96) / in global memory; taken
    //          inside the kernel when a pivot of the factorisation is not positive, or with SVIN_MARG_EIG=jacobi
    //          (the test that keeps the fall-back honest)
    const bool want = sw.margEig != 0;
    const bool forceFallback = sw.margEig == 3;
    const size_t ldsBoth = jacobiLdsBytes(nk, ks.jacobiShared), ldsOne = jacobiLdsBytesGOnly(nk, ks.jacobiShared);
    const int mode = forceFallback ? (ldsBoth ? 1 : 0) : (ldsOne ? 4 : 6);
    const size_t lds = (mode == 4) ? (ldsOne > ldsBoth ? ldsOne : ldsBoth) : (mode == 1 ? ldsBoth : 0);
    // default: the direct solve (tridiagonalisation + divide and conquer) for priors up to kSymEigMaxN unknowns, the Jacobi kernel
    // behind it as the fall-back for a non-finite result (it returns at once when flag[4] says "done"); SVIN_MARG_EIG=cholesky /
    // jacobi select the Jacobi solvers alone
    // ... and ahead of both, for a prior of full numerical rank (every steady-state prior of the sliding windows), the Cholesky
    // factor with its certificate that the rank rule drops nothing (k_marg_final_chol); SVIN_MARG_EIG=direct skips it
    const bool wantDirect = sw.margEig == 1;
    const bool direct = (!want || wantDirect) && nk <= kSymEigMaxN;
    const bool chol = !want && nk <= kSymEigMaxN;
    if (chol) q.finalChol = {1, margCholLdsBytes(nk)};
    if (direct) q.finalDc = {1, symEigLdsBytes(nk)};
    q.finalDcAfterChol = chol ? 1 : 0;
    q.final = {1, lds};
    q.finalMode = mode; q.finalFallbackLds = (mode == 4 && ldsBoth) ? 1 : 0; q.finalSkipIfDone = direct ? 1 : 0;
  }
  // ---- buffers
  q.clearU = mm * mm; q.clearW2 = mm * L3; q.clearV = (size_t)9 * atLeast1(Lm); q.clearVec = mm + 2 * L3 + 14;
  q.bU = q.clearU + 2; q.bW2 = q.clearW2 + 2; q.bV = q.clearV + 2; q.bVec = q.clearVec + 2;
  q.bLin = atLeast1((size_t)32 * N);
  q.bFacLin = atLeast1(F);
  q.bPartial = (size_t)16 * 4096;
  q.bScal = 1;
  q.bFlag = 8;
  q.bHk = atLeast1(n2 + nk);
  q.bScratch = (nk > 0 && nm > 0) ? (size_t)2 * nm * nm + (size_t)nk * nm + 2 * nm + 16 : 0;
  q.bOut = nk > 0 ? 5 * n2 + 4 * nk + 16 : 0;
  q.gLm = atLeast1((size_t)4 * Lm); q.gUv = atLeast1((size_t)2 * N); q.gW = atLeast1(N);
  q.gLmPtr = (size_t)Lm + 1; q.gObsLm = atLeast1(N); q.gIdx = atLeast1(N);
  // ---- regions
  q.ba = {0, (size_t)m}; q.bb = {mm, (size_t)3 * Lm}; q.vb = {mm + L3, (size_t)3 * Lm};
  q.linR = {0, (size_t)2 * N}; q.linJp = {(size_t)2 * N, (size_t)12 * N}; q.linJl = {(size_t)14 * N, (size_t)6 * N};
  q.linJe = {(size_t)20 * N, (size_t)12 * N};
  if (q.dense.grid) {   // tmp: pm (nm) | tv (nm) | Mu (nk x nm)
    q.Vm = {0, (size_t)nm * nm}; q.Qm = {(size_t)nm * nm, (size_t)nm * nm};
    q.denseTmp = {(size_t)2 * nm * nm, (size_t)2 * nm + (size_t)nk * nm};
  }
  if (nk > 0) {
    // (the copy pair writes U and ba whole: nm == 0 means m == nk)
    q.Hk = {0, q.copyPair ? (size_t)m * m : n2}; q.bk = {q.Hk.len, q.copyPair ? (size_t)m : (size_t)nk};
    q.G = {0, n2}; q.Q = {n2, n2}; q.J = {2 * n2, n2}; q.Ht = {3 * n2, n2};
    q.e0 = {4 * n2, (size_t)nk}; q.bp = {4 * n2 + nk, (size_t)nk}; q.scal = {4 * n2 + 2 * nk, 8};
    q.finalTmp = {4 * n2 + 2 * nk + 8, (size_t)3 * nk};   // p | eigenvalues | 1 / sigma
  }
  if (d.oldPriorM > 0) {
    const size_t o2 = (size_t)d.oldPriorM * d.oldPriorM;
    q.oldH = {0, o2}; q.oldB0 = {o2, (size_t)d.oldPriorM};
  }
  return q;
}

}  // namespace svin
