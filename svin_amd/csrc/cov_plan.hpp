// svin_amd: host planning of the marginal-covariance pass (cov.hip, Window::computeCovariance) -- the layout of the window's
// covariance buffer, and the grid and dynamic LDS of every launch.  HIP-free (tests/test_cov_plan_host.py runs it on the CPU
// through tests/csrc/cov_plan_shim.cpp); the launcher walks the plan and the kernels take their LDS offsets from the functions
// below, so each expression is written once.
//
// The pass (Sigma = (J^T J)^-1 by blocks, S = A - W V^-1 W^T the undamped reduced system of a build with mu = 0):
//   k_cov_factor     one workgroup: M = S scaled to a diagonal in [1, 4) (S_ij / sqrt(S_ii S_jj) with the scale rounded to a power of
//                    two, so that M is S exactly) into `scaled`, left-looking Cholesky by 16 x 16 tiles, the finished tiles written
//                    through to `factor`, the inverses of the diagonal tiles to `linv`
//   k_cov_inverse    one workgroup per 16-column panel J: L L^T X = I for the tile rows I >= J, mirrored into `xs`
//   k_cov_refine     one workgroup per panel J: R_J = E_J - M X_J with compensated sums, X_J + X R_J unscaled and mirrored into `sigma`
//   k_cov_landmarks  16 lanes per landmark: V_l, Y_l = V_l^-1 W_l^T and Sigma_ll = V_l^-1 + Y_l Sigma_cc Y_l^T into `lmCov`
//   k_cov_pairs      one wave per requested (landmark, block) / (landmark, landmark') pair, into a buffer of the request's own
#pragma once
#include <cstddef>
#include "tile_dims.hpp"   // kPanelLd

namespace svin {

constexpr int kCovMaxD = 272;            // unknowns of the widest reduced system the pass takes: 17 tile rows
constexpr int kCovFactorThreads = 1024;  // k_cov_factor: 16 waves share the tiles of a block column
constexpr int kCovInverseThreads = 256;  // k_cov_inverse: 4 waves share the tile rows of a panel
constexpr int kCovRefineThreads = 320;   // k_cov_refine: a thread per row of the panel (dpad <= 272: one sweep)
constexpr int kCovLmThreads = 64;        // k_cov_landmarks: 4 landmarks of 16 lanes
constexpr int kCovLmPerBlock = kCovLmThreads / 16;
constexpr int kCovPairThreads = 64;      // k_cov_pairs: one wave
constexpr size_t kCovMaxLdsBytes = 160 * 1024;
constexpr int kCovFlagInts = 4;          // fail bits (1: a landmark block, 2: the reduced system) | first offending landmark | spare
// A pivot below this, of a block whose diagonal is of size one (S: scaled into [1, 4); a landmark block: relative to its own
// diagonal entry), is rank deficiency to working precision: what is left of a zero pivot after the cancellation of terms of
// size one.  A block this close to singular has no covariance a double can hold (Ceres' Covariance draws the same line with
// min_reciprocal_condition_number = 1e-14 on J).
constexpr double kCovPivotTol = 1e-12;

struct CovRegion { size_t off, len; };              // doubles of the window's covariance buffer
struct CovLaunch { int grid, threads; size_t ldsBytes; };
struct CovPlan {
  bool supported;   // d <= kCovMaxD
  int d, dC, L;
  int nT, dpad;     // tile rows, d rounded up to 16
  CovRegion scaled;   // dpad x dpad row-major: M, the scaled S, both triangles (identity beyond row d)
  CovRegion factor;   // dpad x dpad row-major: the lower tiles of the factor of M
  CovRegion linv;     // nT tiles of 256: the inverse of every diagonal tile of the factor, row-major, zero above the diagonal
  CovRegion scale;    // dpad: the power of two next to 1 / sqrt(S_ii) (1 beyond row d)
  CovRegion xs;       // dpad x dpad row-major: X = M^-1 as the substitution leaves it, symmetric bit for bit
  CovRegion sigma;    // d x d row-major: Sigma_cc, symmetric bit for bit
  CovRegion lmCov;    // 9 L: the diagonal block of every landmark, CSR order
  CovRegion flags;    // kCovFlagInts ints
  size_t end;
  CovLaunch factorize, inverse, refine, landmarks;
};

// LDS of k_cov_factor (doubles): the block column's tiles (nT x 16 x kPanelLd) | the pivot tile's factors (16 x kPanelLd) |
// 1 / L_ii (16) | the scale (dpad) | a flag word
constexpr size_t covFactorLdsDoubles(int nT) { return (size_t)nT * 16 * kPanelLd + 16 * kPanelLd + 16 + (size_t)16 * nT + 2; }
// LDS of k_cov_inverse (doubles): the panel's tiles (nT x 16 x kPanelLd)
constexpr size_t covInverseLdsDoubles(int nT) { return (size_t)nT * 16 * kPanelLd; }
// LDS of k_cov_refine (doubles): the panel of the residual (dpad x 16)
constexpr size_t covRefineLdsDoubles(int nT) { return (size_t)16 * nT * 16; }
// LDS of a landmark of k_cov_landmarks / k_cov_pairs (doubles): W_l, then Y_l^T in its place (dC x 3)
constexpr size_t covLandmarkLdsDoubles(int dC) { return (size_t)3 * (dC > 0 ? dC : 1); }

inline CovPlan planCovariance(int d, int dC, int L) {
  CovPlan q{};
  q.d = d; q.dC = dC; q.L = L;
  q.supported = d >= 0 && d <= kCovMaxD && dC >= 0 && dC <= d && L >= 0;
  if (!q.supported) return q;
  q.nT = (d + 15) / 16;
  q.dpad = 16 * q.nT;
  size_t at = 0;
  auto take = [&](size_t len) { CovRegion r{at, len}; at += (len + 1) & ~(size_t)1; return r; };   // (16-byte aligned starts)
  q.scaled = take((size_t)q.dpad * q.dpad);
  q.factor = take((size_t)q.dpad * q.dpad);
  q.linv = take((size_t)q.nT * 256);
  q.scale = take((size_t)q.dpad);
  q.xs = take((size_t)q.dpad * q.dpad);
  q.sigma = take((size_t)d * d);
  q.lmCov = take((size_t)9 * L);
  q.flags = take((kCovFlagInts + 1) / 2);
  q.end = at;
  q.factorize = {d > 0 ? 1 : 0, kCovFactorThreads, covFactorLdsDoubles(q.nT) * 8};
  q.inverse = {q.nT, kCovInverseThreads, covInverseLdsDoubles(q.nT) * 8};
  q.refine = {q.nT, kCovRefineThreads, covRefineLdsDoubles(q.nT) * 8};
  q.landmarks = {(L + kCovLmPerBlock - 1) / kCovLmPerBlock, kCovLmThreads, kCovLmPerBlock * covLandmarkLdsDoubles(dC) * 8};
  return q;
}
// the pairs launch of a request: one wave per pair, two landmarks' Y in LDS
inline CovLaunch planCovariancePairs(int dC, int nPairs) { return CovLaunch{nPairs, kCovPairThreads, 2 * covLandmarkLdsDoubles(dC) * 8}; }

}  // namespace svin
