// svin_amd: marginal covariances of the window's blocks (Map::computeCovariance, Map.hpp:352-372, through ::ceres::Covariance).
//
//   Sigma = (J^T J)^-1, J the stacked minimal Jacobian of every residual as the trust-region build sees it (square-root
//   information and loss corrector applied, prior / host residuals / HomogeneousPointErrors included, no columns for constant
//   blocks), in unscaled tangent coordinates, undamped.  By blocks, with S = A - W V^-1 W^T and Y_l = V_l^-1 W_l^T:
//       Sigma_cc = S^-1      Sigma_lc = -Y_l Sigma_cc      Sigma_ll' = delta_ll' V_l^-1 + Y_l Sigma_cc Y_l'^T
//
// What the pass reads was left on the device by a build with mu = 0 (Window::linearize): S (lower triangle, undamped: the metric
// enters S only as mu * htil) and the per-observation Jacobian arrays JpCur / JlCur / JeCur.  V_l is summed again from JlCur rather
// than read back as Vinv: the build's factorisation of V_l substitutes for a pivot that is not positive (a constant landmark has
// V_l = 0) and reports one bit for all landmarks, and the pass must name the landmark.
//
// Five kernels (layout and launch sizes: cov_plan.hpp), none of which waits on another workgroup -- every dependency is a launch
// boundary -- no floating-point atomics, every sum in a fixed order (bit-identical from call to call):
//   k_cov_factor     ONE workgroup of 16 waves.  M = D S D, D = diag(1 / sqrt(S_ii)) rounded to powers of two (the first-frame prior puts
//                    1e16 beside 1e5 on the diagonal of S: condition 5e14 unscaled, 2e8 .. 8e8 scaled; with powers of two M is S
//                    exactly and its diagonal lies in [1, 4)), identity beyond row d, kept for k_cov_refine.  Left-looking Cholesky
//                    by block columns of 16 x 16 tiles on v_mfma_f64_16x16x4_f64: tile (I, K) of M minus sum_J<K L_IJ L_KJ^T with the
//                    finished tiles read back from the L2-resident factor, the block column staged in LDS, its pivot tile factorised
//                    by wave 0 (cholDiag16Acc, tile16.hpp), the tiles below multiplied with L_KK^-T and written through.  A pivot
//                    that is not positive, or below kCovPivotTol, sets a flag; the kernel substitutes one and runs to its end.
//   k_cov_inverse    one workgroup per 16-column panel J of X = M^-1: forward and backward substitution with the panel (tile rows
//                    J .. nT-1: only the lower triangle of X is kept) in LDS, right-looking, the diagonal solves on wave 0 and the
//                    updates of the other tile rows dealt over four waves; X_ij = X_ji for i >= j.
//   k_cov_refine     one workgroup per panel J, a thread per row (320: one sweep up to dpad = 272): one step of iterative refinement X <- X + X (I - M X) with the
//                    residual in twice the working precision (TwoProduct / TwoSum: Dot2 of Ogita, Rump and Oishi), the correction
//                    in plain doubles; then Sigma_cc[i][j] = Sigma_cc[j][i] = (X_ij D_ii) D_jj for i >= j.  Without it the error
//                    of the factorisation sits on the weakest direction of the window -- measured at d = 150, condition 7e8:
//                    5.0e-8 in units of the standard deviations against 1.9e-8 for LAPACK's Cholesky and 0.5e-8 for its LU on the
//                    same matrix; the residual of the unrefined X is 2e-8, so one step takes the error to the rounding of the
//                    last addition.
//   k_cov_landmarks  16 lanes per landmark.  V_l and its inverse; W_l summed observation by observation (table order) into an LDS
//                    image of dC x 3, the set of camera-side blocks it touches as a bit mask (dC / 6 <= 45 blocks);
//                    Sigma_ll = V_l^-1 + sum over the touched rows r of Y_r^T (sum over the touched columns c of Sigma_cc[r][c] Y_c),
//                    rows strided over the lanes, columns in ascending order, the lanes by a shuffle tree.  Sigma_cc is read from
//                    L2 (at d = 150 it is 180 KB: more than a workgroup's LDS).  Constant landmarks get zeros.
//   k_cov_pairs      one wave per requested (landmark, block) or (landmark, landmark') pair, Y_l formed as above.
#include "kernels.hpp"
#include "cov_plan.hpp"
#include "tile16.hpp"

namespace svin {

namespace {

constexpr int kCovTile = 16 * kPanelLd;   // doubles of a 16 x 16 tile in LDS

__device__ __forceinline__ void covWaveSync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------- factor of the scaled S
__global__ __launch_bounds__(kCovFactorThreads) void k_cov_factor(const double* __restrict__ S, int ldS, int d, int nT,
                                                                  double* __restrict__ Ms, double* __restrict__ Lf,
                                                                  double* __restrict__ Linv, double* __restrict__ scaleOut,
                                                                  int* __restrict__ flags) {
  extern __shared__ double sm[];
  constexpr int NW = kCovFactorThreads / 64;
  const int dpad = 16 * nT;
  double* panel = sm;                            // nT tiles
  double* Dg = panel + (size_t)nT * kCovTile;    // the pivot tile: L lower, L^-1 transposed strictly upper
  double* dinv = Dg + kCovTile;                  // 1 / L_ii
  double* sc = dinv + 16;                        // dpad
  int* sFail = reinterpret_cast<int*>(sc + dpad);
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, g = lane >> 4, c = lane & 15;
  if (t == 0) *sFail = 0;
  __syncthreads();
  for (int i = t; i < dpad; i += kCovFactorThreads) {
    double s = 1.0;
    if (i < d) {
      const double x = S[(size_t)i * ldS + i];
      if (x > 0.0 && x < 1e300) s = ldexp(1.0, -(ilogb(x) >> 1));   // x s^2 in [1, 4), exactly
      else atomicOr(sFail, 2);
    }
    sc[i] = s;
    scaleOut[i] = s;
  }
  __syncthreads();
  const lds_f64* DgL = tileToLds(Dg);
  const lds_f64* dinvL = tileToLds(dinv);
  for (int K = 0; K < nT; ++K) {
    // the block column's tiles: M_IK - sum_J<K L_IJ L_KJ^T
    for (int I = K + wave; I < nT; I += NW) {
      d4_t acc;
      const int j = 16 * K + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * I + g + 4 * r;
        double x = i == j ? 1.0 : 0.0;
        if (i < d && j < d) {
          const int hi = i > j ? i : j, lo = i > j ? j : i;
          x = (S[(size_t)hi * ldS + lo] * sc[hi]) * sc[lo];
        }
        acc[r] = x;
        Ms[(size_t)i * dpad + j] = x;
        Ms[(size_t)j * dpad + i] = x;
      }
      for (int J = 0; J < K; ++J) {
        double av[4], bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          av[q] = -Lf[(size_t)(16 * I + c) * dpad + 16 * J + 4 * q + g];   // A[i = c][k] = -L_IJ[c][k]
          bv[q] = Lf[(size_t)(16 * K + c) * dpad + 16 * J + 4 * q + g];    // B[k][j = c] = L_KJ[c][k]
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) panel[(size_t)I * kCovTile + (g + 4 * r) * kPanelLd + c] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
      d4_t acc;
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = panel[(size_t)K * kCovTile + (g + 4 * r) * kPanelLd + c];
      cholDiag16Acc<false>(acc, Dg, dinv, lane, sFail);
    }
    __syncthreads();
    if (t < 16) {   // pivot = L_ii^2 of a matrix with its diagonal in [1, 4)
      const double li = 1.0 / dinv[t];
      if (!(li * li >= kCovPivotTol)) atomicOr(sFail, 2);
    }
    // tiles below the pivot tile: L_IK = P_I L_KK^-T, written through
    for (int I = K + 1 + wave; I < nT; I += NW) {
      d4_t x = {0.0, 0.0, 0.0, 0.0};
      double av[4], bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        av[q] = panel[(size_t)I * kCovTile + c * kPanelLd + 4 * q + g];
        bv[q] = tileLinvAt(DgL, dinvL, 0, c, 4 * q + g);   // B[k][j = c] = L_KK^-1[c][k]
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) x = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], x, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) Lf[(size_t)(16 * I + g + 4 * r) * dpad + 16 * K + c] = x[r];
    }
    if (t >= kCovFactorThreads - 256) {   // the pivot tile itself and its inverse (the last four waves: the first take the tiles below)
      const int e = t - (kCovFactorThreads - 256), r = e >> 4, cc = e & 15;
      Lf[(size_t)(16 * K + r) * dpad + 16 * K + cc] = cc <= r ? Dg[r * kPanelLd + cc] : 0.0;
      Linv[(size_t)K * 256 + e] = tileLinvAt(DgL, dinvL, 0, r, cc);
    }
    __syncthreads();   // (the tiles written through are read back by this workgroup alone)
  }
  if (t == 0 && *sFail) atomicOr(flags, *sFail);
}

// ---------------------------------------------------------------------------------------------- X = M^-1, panel by panel
__global__ __launch_bounds__(kCovInverseThreads) void k_cov_inverse(const double* __restrict__ Lf, const double* __restrict__ Linv,
                                                                    int nT, double* __restrict__ Xs) {
  extern __shared__ double Z[];   // nT tiles (those of the tile rows >= J are used)
  constexpr int NW = kCovInverseThreads / 64;
  const int dpad = 16 * nT, J = blockIdx.x;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, g = lane >> 4, c = lane & 15;
  for (int e = t; e < (nT - J) * 256; e += kCovInverseThreads) {
    const int I = J + (e >> 8), r = (e >> 4) & 15, cc = e & 15;
    Z[(size_t)I * kCovTile + r * kPanelLd + cc] = (I == J && r == cc) ? 1.0 : 0.0;
  }
  __syncthreads();
  auto loadAcc = [&](int I) {
    d4_t x;
#pragma unroll
    for (int r = 0; r < 4; ++r) x[r] = Z[(size_t)I * kCovTile + (g + 4 * r) * kPanelLd + c];
    return x;
  };
  auto storeAcc = [&](int I, const d4_t& x) {
#pragma unroll
    for (int r = 0; r < 4; ++r) Z[(size_t)I * kCovTile + (g + 4 * r) * kPanelLd + c] = x[r];
  };
  // forward: L Z = E_J
  for (int K = J; K < nT; ++K) {
    if (wave == 0) {   // Z_K <- L_KK^-1 Z_K
      double av[4], bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        av[q] = Linv[(size_t)K * 256 + c * 16 + 4 * q + g];
        bv[q] = Z[(size_t)K * kCovTile + (4 * q + g) * kPanelLd + c];
      }
      d4_t y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 4; ++q) y = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], y, 0, 0, 0);
      storeAcc(K, y);
    }
    __syncthreads();
    for (int I = K + 1 + wave; I < nT; I += NW) {   // Z_I -= L_IK Z_K
      d4_t acc = loadAcc(I);
      double av[4], bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        av[q] = -Lf[(size_t)(16 * I + c) * dpad + 16 * K + 4 * q + g];
        bv[q] = Z[(size_t)K * kCovTile + (4 * q + g) * kPanelLd + c];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], acc, 0, 0, 0);
      storeAcc(I, acc);
    }
    __syncthreads();
  }
  // backward: L^T X = Z, down to tile row J
  for (int K = nT - 1; K >= J; --K) {
    if (wave == 0) {   // X_K <- L_KK^-T Z_K
      double av[4], bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        av[q] = Linv[(size_t)K * 256 + (4 * q + g) * 16 + c];   // A[i = c][k] = L_KK^-1[k][c]
        bv[q] = Z[(size_t)K * kCovTile + (4 * q + g) * kPanelLd + c];
      }
      d4_t y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < 4; ++q) y = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], y, 0, 0, 0);
      storeAcc(K, y);
    }
    __syncthreads();
    for (int I = J + wave; I < K; I += NW) {   // Z_I -= L_KI^T X_K
      d4_t acc = loadAcc(I);
      double av[4], bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        av[q] = -Lf[(size_t)(16 * K + 4 * q + g) * dpad + 16 * I + c];   // A[i = c][k] = -L_KI[k][c]
        bv[q] = Z[(size_t)K * kCovTile + (4 * q + g) * kPanelLd + c];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], acc, 0, 0, 0);
      storeAcc(I, acc);
    }
    __syncthreads();
  }
  // the lower triangle, mirrored
  for (int e = t; e < (nT - J) * 256; e += kCovInverseThreads) {
    const int I = J + (e >> 8), r = (e >> 4) & 15, cc = e & 15;
    const int i = 16 * I + r, j = 16 * J + cc;
    if (i < j) continue;
    const double v = Z[(size_t)I * kCovTile + r * kPanelLd + cc];
    Xs[(size_t)i * dpad + j] = v;
    Xs[(size_t)j * dpad + i] = v;
  }
}

// ---------------------------------------------------------------------------------------------- one step of refinement, unscaling
// (hi, lo) += a * b without the rounding of either the product or the sum (TwoProduct by fma, Knuth's TwoSum).  No contraction in
// here: with hi + p fused into fma(a, b, hi) and p - bb into fma(a, b, -bb) the error of the product is counted twice and the
// sum is an ordinary double's again.
__device__ __forceinline__ void covDot2Step(double a, double b, double& hi, double& lo) {
#pragma clang fp contract(off)
  const double p = a * b;
  const double pe = __builtin_fma(a, b, -p);
  const double s = hi + p;
  const double bb = s - hi;
  const double se = (hi - (s - bb)) + (p - bb);
  hi = s;
  lo += pe + se;
}

__global__ __launch_bounds__(kCovRefineThreads) void k_cov_refine(const double* __restrict__ Ms, const double* __restrict__ Xs,
                                                                  const double* __restrict__ scale, int d, int nT,
                                                                  double* __restrict__ sigma) {
  extern __shared__ double R[];   // dpad x 16: -(M X_J - E_J)
  const int dpad = 16 * nT, J = blockIdx.x, t = threadIdx.x;
  for (int i = t; i < dpad; i += kCovRefineThreads) {   // row i of the panel; M and X are symmetric, so the lanes read neighbours
    double hi[16], lo[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) { hi[c] = (i == 16 * J + c) ? -1.0 : 0.0; lo[c] = 0.0; }
    for (int k = 0; k < dpad; ++k) {
      const double m = Ms[(size_t)k * dpad + i];
      const double* x = Xs + (size_t)k * dpad + 16 * J;
#pragma unroll
      for (int c = 0; c < 16; ++c) covDot2Step(m, x[c], hi[c], lo[c]);
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) R[i * 16 + c] = -(hi[c] + lo[c]);
  }
  __syncthreads();
  for (int i = 16 * J + t; i < d; i += kCovRefineThreads) {   // rows of the lower triangle
    double acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0.0;
    for (int k = 0; k < dpad; ++k) {
      const double x = Xs[(size_t)k * dpad + i];
#pragma unroll
      for (int c = 0; c < 16; ++c) acc[c] = __builtin_fma(x, R[k * 16 + c], acc[c]);
    }
    const double si = scale[i];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int j = 16 * J + c;
      if (j >= d || j > i) continue;
      const double v = ((Xs[(size_t)i * dpad + j] + acc[c]) * si) * scale[j];
      sigma[(size_t)i * d + j] = v;
      sigma[(size_t)j * d + i] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------- landmarks
struct CovLm {
  double vi[6];              // V_l^-1: 00 01 02 11 12 22 (zeros for a landmark that has no covariance of its own)
  unsigned long long mask;   // camera-side blocks (reduced row / 6) the landmark's observations touch
  int state;                 // 0 regular, 1 constant or unobserved (zeros), 2 V_l not positive definite
};

// The 16 lanes of a landmark's group (lane gl) together: V_l^-1, and Y_l^T = W_l V_l^-1 (dC x 3, rows of untouched blocks zero)
// into the group's LDS image Y.  Every lane returns the same record.
__device__ __forceinline__ CovLm covLandmarkY(const DeviceProblem& p, int l, int gl, double* Y) {
  CovLm q;
  const size_t N = (size_t)p.N;
  const int start = p.lmPtr[l], n = p.lmPtr[l + 1] - start, dC = p.dC;
  double v[6] = {0, 0, 0, 0, 0, 0};
  int cst = 0;
  for (int i = gl; i < n; i += 16) {
    const size_t o = (size_t)start + i;
    const double a0 = p.JlCur[o], a1 = p.JlCur[N + o], a2 = p.JlCur[2 * N + o];
    const double c0 = p.JlCur[3 * N + o], c1 = p.JlCur[4 * N + o], c2 = p.JlCur[5 * N + o];
    v[0] += a0 * a0 + c0 * c0; v[1] += a0 * a1 + c0 * c1; v[2] += a0 * a2 + c0 * c2;
    v[3] += a1 * a1 + c1 * c1; v[4] += a1 * a2 + c1 * c2; v[5] += a2 * a2 + c2 * c2;
    if (p.obsW[o] < 0.0) cst = 1;   // (the evaluation wrote a zero landmark Jacobian: a constant landmark)
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += __shfl_xor(v[k], off, 16);   // (a + b == b + a: every lane ends with the same bits)
    cst |= __shfl_xor(cst, off, 16);
  }
  for (int i = gl; i < 3 * dC; i += 16) Y[i] = 0.0;
  q.mask = 0ull;
#pragma unroll
  for (int k = 0; k < 6; ++k) q.vi[k] = 0.0;
  q.state = (cst || n == 0) ? 1 : 0;
  if (q.state == 0) {
    // V = L L^T with every pivot held against the block's own diagonal
    bool bad = !(v[0] > 0.0) || !(v[3] > 0.0) || !(v[5] > 0.0);
    const double l00 = sqrt(bad ? 1.0 : v[0]);
    const double l10 = v[1] / l00, l20 = v[2] / l00;
    const double t11 = v[3] - l10 * l10;
    bad = bad || !(t11 > kCovPivotTol * v[3]);
    const double l11 = sqrt(bad ? 1.0 : t11);
    const double l21 = (v[4] - l20 * l10) / l11;
    const double t22 = v[5] - l20 * l20 - l21 * l21;
    bad = bad || !(t22 > kCovPivotTol * v[5]);
    const double l22 = sqrt(bad ? 1.0 : t22);
    if (bad) {
      q.state = 2;
    } else {
      const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
      const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
      q.vi[0] = i00 * i00 + i10 * i10 + i20 * i20; q.vi[1] = i10 * i11 + i20 * i21; q.vi[2] = i20 * i22;   // V^-1 = L^-T L^-1
      q.vi[3] = i11 * i11 + i21 * i21; q.vi[4] = i21 * i22; q.vi[5] = i22 * i22;
    }
  }
  covWaveSync();
  if (q.state != 0) return q;
  // W_l = sum_o Jc_o^T Jl_o, one observation after the other (table order); entry (a, k) of a block always falls to the same lane
  for (int i = 0; i < n; ++i) {
    const size_t o = (size_t)start + i;
    const uint32_t idx = p.obsIdx[o];
    if (((idx >> 24) & 0xf) == (uint32_t)kPriorCam) continue;   // HomogeneousPointError: no camera-side block
    int offP = p.poseOff[idx & 0xfff];
    int offE = p.anyExtVariable ? p.extOff[(idx >> 12) & 0xfff] : -1;
    if (offP < 0 || offP + 6 > dC) offP = -1;
    if (offE < 0 || offE + 6 > dC) offE = -1;
    if (offP < 0 && offE < 0) continue;
    double jl[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) jl[k] = p.JlCur[k * N + o];
#pragma unroll
    for (int e0 = 0; e0 < 48; e0 += 16) {
      const int e = e0 + gl;
      if (e >= 36) continue;
      const bool ext = e >= 18;
      const int m = ext ? e - 18 : e, a = m / 3, k = m - 3 * a, off = ext ? offE : offP;
      if (off < 0) continue;
      const double* Jc = ext ? p.JeCur : p.JpCur;
      Y[3 * (off + a) + k] += Jc[a * N + o] * jl[k] + Jc[(6 + a) * N + o] * jl[3 + k];
    }
    if (offP >= 0) q.mask |= 1ull << (offP / 6);
    if (offE >= 0) q.mask |= 1ull << (offE / 6);
  }
  covWaveSync();
  // Y_l^T = W_l V_l^-1, row by row in place
  for (int r = gl; r < dC; r += 16) {
    if (!((q.mask >> (r / 6)) & 1ull)) continue;
    const double w0 = Y[3 * r], w1 = Y[3 * r + 1], w2 = Y[3 * r + 2];
    Y[3 * r] = w0 * q.vi[0] + w1 * q.vi[1] + w2 * q.vi[2];
    Y[3 * r + 1] = w0 * q.vi[1] + w1 * q.vi[3] + w2 * q.vi[4];
    Y[3 * r + 2] = w0 * q.vi[2] + w1 * q.vi[4] + w2 * q.vi[5];
  }
  covWaveSync();
  return q;
}

__global__ __launch_bounds__(kCovLmThreads) void k_cov_landmarks(DeviceProblem p, const double* __restrict__ sigma,
                                                                 double* __restrict__ lmCov, int* __restrict__ flags) {
  extern __shared__ double sm[];
  const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15, l = blockIdx.x * kCovLmPerBlock + grp;
  if (l >= p.L) return;   // whole 16-lane rows leave together
  const int d = p.d, dC = p.dC;
  double* Y = sm + (size_t)grp * covLandmarkLdsDoubles(dC);
  const CovLm q = covLandmarkY(p, l, gl, Y);
  if (q.state == 2 && gl == 0) {
    atomicOr(flags, 1);
    atomicMax(flags + 1, p.L - l);   // the first offending landmark is L - flags[1]
  }
  double s[6] = {0, 0, 0, 0, 0, 0};
  if (q.state == 0) {
    for (int r = gl; r < dC; r += 16) {
      if (!((q.mask >> (r / 6)) & 1ull)) continue;
      double t0 = 0.0, t1 = 0.0, t2 = 0.0;
      for (int b = 0; 6 * b < dC; ++b) {
        if (!((q.mask >> b) & 1ull)) continue;
#pragma unroll
        for (int cc = 6 * b; cc < 6 * b + 6; ++cc) {
          const double sg = sigma[(size_t)cc * d + r];   // (= Sigma_cc[r][cc] bit for bit; this way the lanes read neighbours)
          t0 += sg * Y[3 * cc]; t1 += sg * Y[3 * cc + 1]; t2 += sg * Y[3 * cc + 2];
        }
      }
      const double y0 = Y[3 * r], y1 = Y[3 * r + 1], y2 = Y[3 * r + 2];
      s[0] += y0 * t0; s[1] += y0 * t1; s[2] += y0 * t2; s[3] += y1 * t1; s[4] += y1 * t2; s[5] += y2 * t2;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off, 16);
  if (gl < 9) {
    const int r = gl / 3, c = gl % 3, lo = r < c ? r : c, hi = r < c ? c : r;
    const int k = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
    lmCov[(size_t)9 * l + gl] = q.state == 0 ? q.vi[k] + s[k] : 0.0;
  }
}

// ---------------------------------------------------------------------------------------------- requested pairs
__global__ __launch_bounds__(kCovPairThreads) void k_cov_pairs(DeviceProblem p, const double* __restrict__ sigma,
                                                               const CovPair* __restrict__ pairs, double* __restrict__ out) {
  extern __shared__ double sm[];
  __shared__ unsigned long long sMask[2];
  __shared__ int sState[2];
  const CovPair rq = pairs[blockIdx.x];
  const int t = threadIdx.x, grp = t >> 4, gl = t & 15, d = p.d, dC = p.dC;
  double* YA = sm;
  double* YB = sm + covLandmarkLdsDoubles(dC);
  if (grp == 0 || (grp == 1 && rq.kind == 1)) {
    const CovLm q = covLandmarkY(p, grp == 0 ? rq.lm : rq.other, gl, grp == 0 ? YA : YB);
    if (gl == 0) { sMask[grp] = q.mask; sState[grp] = q.state; }
  }
  __syncthreads();
  const unsigned long long mA = sMask[0];
  const bool zero = sState[0] != 0 || (rq.kind == 1 && sState[1] != 0);
  if (rq.kind == 0) {   // Sigma_l,b = -Y_l Sigma_cc[:, b]: 3 x md
    const int md = rq.md;
    if (t >= 3 * md) return;
    const int k = t / md, c = rq.other + (t - k * md);
    double acc = 0.0;
    if (!zero)
      for (int r = 0; r < dC; ++r)
        if ((mA >> (r / 6)) & 1ull) acc += YA[3 * r + k] * sigma[(size_t)r * d + c];
    out[(size_t)rq.out + t] = zero ? 0.0 : -acc;
  } else {              // Sigma_l,l' = Y_l Sigma_cc Y_l'^T: 3 x 3
    if (t >= 9) return;
    const unsigned long long mB = sMask[1];
    const int k = t / 3, k2 = t - 3 * k;
    double acc = 0.0;
    if (!zero)
      for (int r = 0; r < dC; ++r) {
        if (!((mA >> (r / 6)) & 1ull)) continue;
        double tr = 0.0;
        for (int c = 0; c < dC; ++c)
          if ((mB >> (c / 6)) & 1ull) tr += sigma[(size_t)r * d + c] * YB[3 * c + k2];
        acc += YA[3 * r + k] * tr;
      }
    out[(size_t)rq.out + t] = acc;
  }
}

}  // namespace

void launchCovariancePass(const DeviceProblem& p, const CovPlan& q, double* buf, hipStream_t s) {
  int* flags = reinterpret_cast<int*>(buf + q.flags.off);
  HIP_OK(hipMemsetAsync(flags, 0, sizeof(int) * kCovFlagInts, s));
  launch(k_cov_factor, dim3(q.factorize.grid), dim3(q.factorize.threads), q.factorize.ldsBytes, s, (const double*)p.S, p.ldS, p.d, q.nT,
         buf + q.scaled.off, buf + q.factor.off, buf + q.linv.off, buf + q.scale.off, flags);
  launch(k_cov_inverse, dim3(q.inverse.grid), dim3(q.inverse.threads), q.inverse.ldsBytes, s, (const double*)(buf + q.factor.off),
         (const double*)(buf + q.linv.off), q.nT, buf + q.xs.off);
  launch(k_cov_refine, dim3(q.refine.grid), dim3(q.refine.threads), q.refine.ldsBytes, s, (const double*)(buf + q.scaled.off),
         (const double*)(buf + q.xs.off), (const double*)(buf + q.scale.off), p.d, q.nT, buf + q.sigma.off);
  launch(k_cov_landmarks, dim3(q.landmarks.grid), dim3(q.landmarks.threads), q.landmarks.ldsBytes, s, p,
         (const double*)(buf + q.sigma.off), buf + q.lmCov.off, flags);
}

void launchCovariancePairs(const DeviceProblem& p, const CovPlan& q, const double* buf, const CovPair* pairs, int nPairs, double* out,
                           hipStream_t s) {
  const CovLaunch l = planCovariancePairs(p.dC, nPairs);
  launch(k_cov_pairs, dim3(l.grid), dim3(l.threads), l.ldsBytes, s, p, buf + q.sigma.off, pairs, out);
}

}  // namespace svin
