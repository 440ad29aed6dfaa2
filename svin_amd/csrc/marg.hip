// svin_amd marginalisation (K10): Estimator::applyMarginalizationStrategy policy on the host,
// MarginalizationError algebra on the device.
//
// Reference (relative to /root/reference/okvis_ros/okvis/okvis_ceres/):
//   policy  src/Estimator.cpp:495-814
//   M1      src/MarginalizationError.cpp:126-397  (linearise at first-estimate points, H += J^T J, b0 -= J^T r)
//   M2      :463-721 + include/okvis/ceres/implementation/MarginalizationError.hpp:48-220
//   M3      :725-758
// Device layout of one marginalisation job: dense part U (m x m) / ba (m), landmark coupling W (m x 3Lm),
// landmark blocks V (Lm x 9) / bb (3Lm).  The reference's Jacobi preconditioner only influences the
// rank-revealing thresholds of the eliminated blocks; it is applied to exactly those blocks here
// (U - W V^+ W^T with V^+ = D^-1 (D^-1 V D^-1)^+ D^-1), which is the same matrix in exact arithmetic.
#include "window.hpp"
#include "marg_plan.hpp"
#include "symeig.hpp"
#include "tile16.hpp"
#include <chrono>
#include <memory>
#include <type_traits>
#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace svin {

__device__ __forceinline__ double waveSumM(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- M1 accumulation
struct MargDev {
  int m, Lm, N, F;
  double *U, *ba, *W, *V, *bb;  // U m x m, W m x 3Lm (row-major), V Lm x 9, bb 3Lm
};

// M1 is accumulated in a FIXED order (no atomics): the prior feeds a sequence of optimisations that amplifies rounding
// differences, so two runs of the same window must produce the same bits.
//   k_marg_accum_lm    one thread per marginalised landmark: V_l, bb_l and the three columns of W it owns, over its
//                      observations in CSR order
//   k_marg_accum_cam   one wave per (camera-side block, part): lane i sums the observations i, i + 64, ... that touch
//                      the block, then a fixed butterfly over the lanes; part 0 = diagonal block + right-hand side,
//                      part 1 + c = the pose x extrinsics cross block of camera c (written with its transpose)
//   k_marg_accum_factors  one workgroup, the small factors one after the other
template <bool WITH_EXT>
__global__ void k_marg_accum_lm(DeviceProblem p, MargDev md) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= md.Lm) return;
  const size_t N = (size_t)p.N;
  const int wld = 3 * md.Lm;
  double V[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bb[3] = {0, 0, 0};
  for (int o = p.lmPtr[l]; o < p.lmPtr[l + 1]; ++o) {
    const uint32_t idx = p.obsIdx[o];
    const int offP = p.poseOff[idx & 0xfff];
    const int offE = WITH_EXT ? p.extOff[(idx >> 12) & 0xfff] : -1;
    const double r0 = p.rCur[o], r1 = p.rCur[N + o];
    double jl[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) jl[k] = p.JlCur[k * N + o];
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) V[a * 3 + b] += jl[a] * jl[b] + jl[3 + a] * jl[3 + b];
      bb[a] += -(jl[a] * r0 + jl[3 + a] * r1);
    }
    auto cam = [&](const double* J, int off) {
      if (off < 0) return;
      for (int a = 0; a < 6; ++a) {
        const double j0 = J[(size_t)a * N + o], j1 = J[(size_t)(6 + a) * N + o];
        double* w = md.W + (size_t)(off + a) * wld + 3 * l;   // columns 3l .. 3l+2 belong to this thread
        for (int b = 0; b < 3; ++b) w[b] += j0 * jl[b] + j1 * jl[3 + b];
      }
    };
    cam(p.JpCur, offP);
    if (WITH_EXT) cam(p.JeCur, offE);
  }
  for (int k = 0; k < 9; ++k) md.V[9 * (size_t)l + k] = V[k];
  for (int a = 0; a < 3; ++a) md.bb[3 * l + a] = bb[a];
}

template <bool WITH_EXT>
__global__ __launch_bounds__(64) void k_marg_accum_cam(DeviceProblem p, MargDev md) {
  const int target = blockIdx.x, part = blockIdx.y, lane = threadIdx.x;
  const bool isPose = target < p.nPose;
  const int slot = isPose ? target : target - p.nPose;
  const int off = isPose ? p.poseOff[slot] : p.extOff[slot];
  if (off < 0) return;
  if (part > 0 && !isPose) return;                 // cross blocks are written by the pose side
  const size_t N = (size_t)p.N;
  const int m = md.m;
  double acc[42];
#pragma unroll
  for (int k = 0; k < 42; ++k) acc[k] = 0.0;
  int partner = -1;                                // extrinsics slot of the cross block (unique per pose and camera)
  for (int o = lane; o < p.N; o += 64) {
    const uint32_t idx = p.obsIdx[o];
    const int ps = idx & 0xfff, es = (idx >> 12) & 0xfff, cam = (idx >> 24) & 0xf;
    if (isPose ? ps != slot : es != slot) continue;
    const double* J = isPose ? p.JpCur : p.JeCur;
    double ja[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) ja[k] = J[(size_t)k * N + o];
    if (part == 0) {
      const double r0 = p.rCur[o], r1 = p.rCur[N + o];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = 0; b < 6; ++b) acc[a * 6 + b] += ja[a] * ja[b] + ja[6 + a] * ja[6 + b];
        acc[36 + a] += -(ja[a] * r0 + ja[6 + a] * r1);
      }
    } else if (WITH_EXT) {
      if (cam != part - 1 || p.extOff[es] < 0) continue;
      partner = es;
      double je[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) je[k] = p.JeCur[(size_t)k * N + o];
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) acc[a * 6 + b] += ja[a] * je[b] + ja[6 + a] * je[6 + b];
    }
  }
#pragma unroll
  for (int k = 0; k < 42; ++k) acc[k] = waveSumM(acc[k]);   // xor butterfly: the same order on every run
  for (int o = 32; o > 0; o >>= 1) partner = max(partner, __shfl_xor(partner, o, 64));
  if (lane != 0) return;
  if (part == 0) {
    for (int a = 0; a < 6; ++a) {
      for (int b = 0; b < 6; ++b) md.U[(size_t)(off + a) * m + off + b] += acc[a * 6 + b];
      md.ba[off + a] += acc[36 + a];
    }
  } else if (partner >= 0) {
    const int offE = p.extOff[partner];
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) {
        md.U[(size_t)(off + a) * m + offE + b] += acc[a * 6 + b];
        md.U[(size_t)(offE + b) * m + off + a] += acc[a * 6 + b];
      }
  }
}

__global__ __launch_bounds__(256) void k_marg_accum_factors(DeviceProblem p, MargDev md) {
  __shared__ int colRow[30];
  for (int f = 0; f < md.F; ++f) {
    const FactorLin& lin = p.linCur[f];
    const int mm = lin.m, nc = lin.ncols;
    const double sc2 = lin.sc * lin.sc;   // the factor's loss corrector (MarginalizationError.cpp:283-330), 1 without a loss
    __syncthreads();
    if (threadIdx.x < 30) {
      int c = threadIdx.x, row = -1, base = 0;
      for (int b = 0; b < 4; ++b) {
        if (c >= base && c < base + lin.dim[b]) row = lin.off[b] < 0 ? -1 : lin.off[b] + (c - base);
        base += lin.dim[b];
      }
      colRow[threadIdx.x] = (c < nc) ? row : -1;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < nc * nc; idx += blockDim.x) {
      const int a = idx / nc, b = idx % nc;
      const int ra = colRow[a], rb = colRow[b];
      if (ra < 0 || rb < 0) continue;
      double s = 0;
      for (int k = 0; k < mm; ++k) s += lin.J[k * nc + a] * lin.J[k * nc + b];
      md.U[(size_t)ra * md.m + rb] += s * sc2;       // distinct columns of one factor are distinct rows of U
      if (a == b) {
        double g = 0;
        for (int k = 0; k < mm; ++k) g += lin.J[k * nc + a] * lin.r[k];
        md.ba[ra] -= g * sc2;
      }
    }
  }
}

// ---------------------------------------------------------------- small symmetric eigen-solvers
// 3x3: cyclic Jacobi with eigenvectors (columns of Q, row-major 3x3)
__device__ void symEig3(const double* A9, double* ev, double* Q) {
  double a00 = A9[0], a01 = 0.5 * (A9[1] + A9[3]), a02 = 0.5 * (A9[2] + A9[6]), a11 = A9[4], a12 = 0.5 * (A9[5] + A9[7]),
         a22 = A9[8];
  for (int k = 0; k < 9; ++k) Q[k] = (k % 4 == 0) ? 1.0 : 0.0;
  auto rotQ = [&](int p, int q, double c, double s) {
    for (int r = 0; r < 3; ++r) {
      const double qp = Q[r * 3 + p], qq = Q[r * 3 + q];
      Q[r * 3 + p] = c * qp - s * qq;
      Q[r * 3 + q] = s * qp + c * qq;
    }
  };
  for (int sweep = 0; sweep < 16; ++sweep) {
    if (fabs(a01) + fabs(a02) + fabs(a12) == 0.0) break;
    if (a01 != 0.0) {
      const double th = (a11 - a00) / (2.0 * a01);
      const double tt = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
      const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
      const double n00 = a00 - tt * a01, n11 = a11 + tt * a01, n02 = c * a02 - s * a12, n12 = s * a02 + c * a12;
      a00 = n00; a11 = n11; a01 = 0; a02 = n02; a12 = n12;
      rotQ(0, 1, c, s);
    }
    if (a02 != 0.0) {
      const double th = (a22 - a00) / (2.0 * a02);
      const double tt = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
      const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
      const double n00 = a00 - tt * a02, n22 = a22 + tt * a02, n01 = c * a01 - s * a12, n12 = s * a01 + c * a12;
      a00 = n00; a22 = n22; a02 = 0; a01 = n01; a12 = n12;
      rotQ(0, 2, c, s);
    }
    if (a12 != 0.0) {
      const double th = (a22 - a11) / (2.0 * a12);
      const double tt = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
      const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
      const double n11 = a11 - tt * a12, n22 = a22 + tt * a12, n01 = c * a01 - s * a02, n02 = s * a01 + c * a02;
      a11 = n11; a22 = n22; a12 = 0; a01 = n01; a02 = n02;
      rotQ(1, 2, c, s);
    }
  }
  ev[0] = a00; ev[1] = a11; ev[2] = a22;
}

// n x n symmetric eigendecomposition by one-sided (Hestenes) Jacobi, executed by one workgroup.
// G (row j = column j of A on entry) is overwritten by the columns of A*Q; Q (row j = eigenvector j)
// must hold the identity on entry.  Eigenvalue j = Q_j . G_j.  Rounds follow the round-robin
// tournament so that the n/2 rotations of one round touch disjoint columns.
// columns count as orthogonal below this relative inner product: a few times the rounding noise eps*sqrt(n) of the
// dot product itself (1e-15 kept the solver chasing that noise for 5+ extra sweeps)
constexpr double kJacobiOrthTol = 2.0e-14;
constexpr double kJacobiFinalCos = 3.0e-9;
// (kJacobiRegLen, the column length the lane groups hold in registers, and jacobiLd, the row length of the LDS images: marg_plan.hpp)

// one 32-bit half at a time through DPP; kCtrl: row_ror:N = 0x120 + N (lane i of a 16-lane row reads lane (i - N) & 15)
template <int kCtrl>
__device__ __forceinline__ double dppRowMov(double v) {
  const long long b = __double_as_longlong(v);
  int lo = (int)b, hi = (int)(b >> 32);
  lo = __builtin_amdgcn_mov_dpp(lo, kCtrl, 0xf, 0xf, false);   // (row rotations only: every lane receives a value)
  hi = __builtin_amdgcn_mov_dpp(hi, kCtrl, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned long long)(unsigned)lo);
}
// sum over the 16 lanes of a DPP row, in every lane; all 16 lanes must be active.  (__shfl_xor(.., 16) compiles to
// ds_bpermute: 24 LDS round trips per pair for the three inner products.)
__device__ __forceinline__ double rowSum16(double v) {
  v += dppRowMov<0x128>(v);
  v += dppRowMov<0x124>(v);
  v += dppRowMov<0x122>(v);
  v += dppRowMov<0x121>(v);
  return v;
}

// Workgroup barrier that only orders LDS traffic (__syncthreads() also waits for every outstanding global access).
__device__ __forceinline__ void ldsBarrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// pair k of round `round` of the round-robin tournament over np players (np even)
__device__ __forceinline__ void jacobiPair(int np, int round, int k, int& a, int& b) {
  if (k == 0) { a = np - 1; b = round; return; }
  a = round + k; if (a >= np - 1) a -= np - 1;
  b = round - k; if (b < 0) b += np - 1;
}
// Jacobi rotation that orthogonalises two columns with |p|^2 = al, |q|^2 = be, p.q = ga: the small-angle solution of
// tan(2 theta) = 2 ga / (be - al).  The rotation sits on the critical path of every tournament round, so it is written
// with two reciprocal square roots and no division: with h = hypot(be - al, 2 ga), cos(2 theta) = |be - al| / h and
// x = (1 + cos(2 theta)) / 2 in [1/2, 1]:  c = sqrt(x) = x rsqrt(x),  s = sin(2 theta) / (2 c) = sin(2 theta) rsqrt(x) / 2.
__device__ __forceinline__ void jacobiRotation(double al, double be, double ga, double& c, double& s) {
  const double d = be - al, g2 = 2.0 * ga;
  const double rh = rsqrt(d * d + g2 * g2);
  const double x = 0.5 + 0.5 * fabs(d) * rh;
  const double rx = rsqrt(x);
  c = x * rx;
  s = copysign(0.5 * g2 * rh * rx, d * g2);
}
// Lanes per column pair: 16 (one DPP row).  A tournament round is one dependent chain per wave (LDS read -> inner
// products -> reduce -> rotation -> LDS write -> barrier) and what it costs is that chain's instruction count, not VALU
// throughput: 8 lanes per pair (twice the per-lane column length) measured 11 % slower at n = 105.
// Pointers into the LDS images carry their address space: through a generic double* every access is a FLAT
// instruction (aperture check in the texture addresser, counted on vmcnt and lgkmcnt), several times slower than ds_*.
using lds_double = __attribute__((address_space(3))) double;
__device__ __forceinline__ lds_double* toLds(double* p) { return (lds_double*)p; }

// one copy for all instantiations of the solver
struct JacobiShared {
  double nullTol2;
  int anyRotation, anyLargeRotation;
};
__shared__ JacobiShared gJacobiShared;

// LPG lanes per pair; P = lds_double* (the LDS images: every column has jacobiLd(n) addressable entries with a zero
// tail) or double* (global memory, leading dimension n).
// Returns the number of sweeps.  kHasQ: rotate the rows of Q along with G (compile-time: each use gets a straight-line round).
// NU > 0: the columns have exactly NU slices of LPG entries (compile-time: the register loops of a round then have no exit
// test between their LDS reads -- with the test each slice was its own LDS round trip, three in a row at n = 45)
template <int LPG, class P, bool kHasQ, int NU = 0>
__device__ int jacobiEigBlock(P G, P Q, int n, int ld, int* flag) {
  constexpr bool padded = std::is_same<P, lds_double*>::value;
  constexpr int kRegCols = kJacobiRegLen / LPG;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nWaves = blockDim.x >> 6;
  if (n <= 1) return 0;
  const int np = (n & 1) ? n + 1 : n;  // phantom player when n is odd
  constexpr bool inRegs = padded;   // the LDS images exist for n <= 136 < kJacobiRegLen only
  int sweeps = 0;
  // Columns whose norm (= |eigenvalue|) is below eps*n*max-norm belong to the numerical null space: the callers zero
  // those eigenvalues anyway, and rotating two such columns against each other only chases rounding noise (it used
  // to keep the solver busy for all 40 sweeps).  Pairs with at least one significant column are still rotated.
  double& nullTol2 = gJacobiShared.nullTol2;
  int& anyRotation = gJacobiShared.anyRotation;
  // (Skipping pairs whose columns did not change since they were last found orthogonal buys nothing: the sweeps are
  // dense, nearly every column still moves a little in every one of the 14 .. 19 sweeps.)
  for (int sweep = 0; sweep < 40; ++sweep) {
    __syncthreads();
    if (threadIdx.x == 0) { anyRotation = 0; gJacobiShared.anyLargeRotation = 0; nullTol2 = 0.0; }
    __syncthreads();
    {
      double mx = 0;
      for (int j = wave; j < n; j += nWaves) {
        double a2 = 0;
        for (int i = lane; i < n; i += 64) { const double x = G[(size_t)j * ld + i]; a2 += x * x; }
        a2 = waveSumM(a2);
        mx = fmax(mx, a2);
      }
      // non-negative doubles order like their bit patterns
      if (lane == 0) atomicMax(reinterpret_cast<unsigned long long*>(&nullTol2), (unsigned long long)__double_as_longlong(mx));
    }
    __syncthreads();
    const double eps_n = 2.220446049250313e-16 * n;
    const double tol2 = nullTol2 * eps_n * eps_n;
    // the n/2 disjoint pairs of a round run side by side, one lane group each
    const int grp = threadIdx.x / LPG, gl = threadIdx.x % LPG, nGroups = blockDim.x / LPG;
    bool rotated = false, large = false;
    for (int round = 0; round < np - 1; ++round) {
      for (int k = grp; k < np / 2; k += nGroups) {
        int a, b;
        jacobiPair(np, round, k, a, b);
        if (a >= n || b >= n) continue;
        const int pI = a < b ? a : b, qI = a < b ? b : a;
        P gp = G + pI * ld + gl;
        P gq = G + qI * ld + gl;
        double al = 0, be = 0, ga = 0;
        double xs[kRegCols], ys[kRegCols];
        if (inRegs) {
          if (NU > 0) {
#pragma unroll
            for (int u = 0; u < (NU > 0 ? NU : 1); ++u) { xs[u] = gp[LPG * u]; ys[u] = gq[LPG * u]; }
#pragma unroll
            for (int u = 0; u < (NU > 0 ? NU : 1); ++u) { al += xs[u] * xs[u]; be += ys[u] * ys[u]; ga += xs[u] * ys[u]; }
          } else {
#pragma unroll
            for (int u = 0; u < kRegCols; ++u) {
              if (LPG * u >= n) break;
              const double x = gp[LPG * u], y = gq[LPG * u];
              xs[u] = x; ys[u] = y;
              al += x * x; be += y * y; ga += x * y;
            }
          }
        } else {
          for (int i = gl; i < n; i += LPG) { const double x = gp[i - gl], y = gq[i - gl]; al += x * x; be += y * y; ga += x * y; }
        }
        static_assert(LPG == 16, "one DPP row per column pair");
        al = rowSum16(al); be = rowSum16(be); ga = rowSum16(ga);
        if (ga * ga <= (kJacobiOrthTol * kJacobiOrthTol) * (al * be) || al == 0.0 || be == 0.0 || (al <= tol2 && be <= tol2))
          continue;
        rotated = true;
        large = large || ga * ga >= (kJacobiFinalCos * kJacobiFinalCos) * (al * be);
        double c, s;
        jacobiRotation(al, be, ga, c, s);
        if (inRegs) {
          if (NU > 0) {
#pragma unroll
            for (int u = 0; u < (NU > 0 ? NU : 1); ++u) {
              gp[LPG * u] = c * xs[u] - s * ys[u];
              gq[LPG * u] = s * xs[u] + c * ys[u];
            }
          } else {
#pragma unroll
            for (int u = 0; u < kRegCols; ++u) {
              if (LPG * u >= n) break;
              gp[LPG * u] = c * xs[u] - s * ys[u];
              gq[LPG * u] = s * xs[u] + c * ys[u];
            }
          }
        } else {
          for (int i = gl; i < n; i += LPG) {
            const double x = gp[i - gl], y = gq[i - gl];
            gp[i - gl] = c * x - s * y; gq[i - gl] = s * x + c * y;
          }
        }
        if (kHasQ) {
          P vp = Q + pI * ld;
          P vq = Q + qI * ld;
          for (int i = gl; i < n; i += LPG) {
            const double u = vp[i], w = vq[i];
            vp[i] = c * u - s * w; vq[i] = s * u + c * w;
          }
        }
      }
      if (padded) ldsBarrier(); else __syncthreads();   // padded = G and Q are LDS images
    }
    if (rotated) anyRotation = 1;   // racing stores of the same value
    if (large) gJacobiShared.anyLargeRotation = 1;
    if (threadIdx.x == 0) flag[1] = sweep + 1;
    sweeps = sweep + 1;
    __syncthreads();
    // Converged when nothing was rotated - or when every rotation of this sweep was by less than kJacobiFinalCos: the
    // pairs it left alone were orthogonal to kJacobiOrthTol when visited and have since moved by products of two such
    // angles at most (n of them: 1e-15), so the sweep that would only confirm it is not run.
    if (anyRotation == 0 || gJacobiShared.anyLargeRotation == 0) break;
  }
  __syncthreads();
  return sweeps;
}
constexpr int kJacobiLanes = 16;

// Same, with G and Q staged through LDS when the kernel was launched with 2*n*jacobiLd(n) doubles of dynamic shared
// memory (lds != nullptr): every round of the tournament is one LDS round trip instead of a global-memory one
// (12 sweeps x 50 rounds at n = 51: 1.9 ms -> 0.2 ms).
__device__ void jacobiEig(double* G, double* Q, int n, int* flag, double* lds) {
  if (!lds) { jacobiEigBlock<kJacobiLanes, double*, true>(G, Q, n, n, flag); return; }
  const int ld = jacobiLd(n);
  lds_double* sG = toLds(lds);
  lds_double* sQ = sG + n * ld;
  for (int idx = threadIdx.x; idx < n * ld; idx += blockDim.x) {
    const int i = idx / ld, j = idx - i * ld;
    sG[idx] = j < n ? G[i * n + j] : 0.0;
    sQ[idx] = j < n ? Q[i * n + j] : 0.0;
  }
  __syncthreads();
  jacobiEigBlock<kJacobiLanes, lds_double*, true>(sG, sQ, n, ld, flag);
  for (int idx = threadIdx.x; idx < n * n; idx += blockDim.x) {
    const int i = idx / n, j = idx - i * n;
    G[idx] = sG[i * ld + j];
    Q[idx] = sQ[i * ld + j];
  }
  __syncthreads();
}
// (the LDS the launches ask for -- jacobiLdsBytes, jacobiLdsBytesGOnly, margCholLdsBytes, symEigLdsBytes: marg_plan.hpp)

// ---------------------------------------------------------------- M2: landmark part (:557-619)
// per landmark: p_b from diag(V), V' = V/(p_b p_b^T), (V')^+ by 3x3 eigendecomposition with tolerance
// eps*3*lmax, N = D_b^-1 U_e diag(sqrt(1/l)|0);  Mu = W_l N (m x 3) overwrites W_l; vb = N N^T bb_l.
// A landmark with V = 0 (a constant one) leaves the stage with N = 0, vb = 0: it takes nothing out of U and ba.
__global__ void k_marg_lm_prepare(MargDev md, double* vb) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= md.Lm) return;
  const double* V = md.V + 9 * (size_t)l;
  if (V[0] == 0.0 && V[4] == 0.0 && V[8] == 0.0) {
    // a constant landmark (every Jl of it is zero, so V, W's columns and bb are exact zeros): N = 0 and vb = 0, stated here and
    // not left to the 3x3 eigen-solver (a positive semi-definite V with a zero diagonal is zero: the general branch below
    // gives the same N)
    for (int a = 0; a < 3; ++a) vb[3 * l + a] = 0.0;
    for (int k = 0; k < 9; ++k) md.V[9 * (size_t)l + k] = 0.0;   // N
    return;
  }
  double pb[3];
  for (int a = 0; a < 3; ++a) pb[a] = (V[a * 4] > 1.0e-9) ? sqrt(V[a * 4]) : 1.0e-3;
  double Vs[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) Vs[a * 3 + b] = V[a * 3 + b] / (pb[a] * pb[b]);
  double ev[3], Q[9];
  symEig3(Vs, ev, Q);
  const double mx = fmax(ev[0], fmax(ev[1], ev[2]));
  const double tol = 2.220446049250313e-16 * 3 * mx;
  double Nm[9];
  for (int j = 0; j < 3; ++j) {
    const double sc = (ev[j] > tol) ? sqrt(1.0 / ev[j]) : 0.0;
    for (int a = 0; a < 3; ++a) Nm[a * 3 + j] = Q[a * 3 + j] * sc / pb[a];
  }
  // vb = N N^T bb
  const double* bb = md.bb + 3 * l;
  double t[3];
  for (int j = 0; j < 3; ++j) t[j] = Nm[j] * bb[0] + Nm[3 + j] * bb[1] + Nm[6 + j] * bb[2];
  for (int a = 0; a < 3; ++a) vb[3 * l + a] = Nm[a * 3] * t[0] + Nm[a * 3 + 1] * t[1] + Nm[a * 3 + 2] * t[2];
  // store N in V (no longer needed)
  double* Vw = md.V + 9 * (size_t)l;
  for (int k = 0; k < 9; ++k) Vw[k] = Nm[k];
}
// ba -= W vb (uses the original W) ; then W_l <- W_l N_l.  One workgroup per row of W, the landmarks dealt over its threads,
// the row's sum reduced in a fixed order (deterministic); one THREAD per row walking all landmarks took 130-220 us.
__global__ __launch_bounds__(256) void k_marg_lm_apply(MargDev md, const double* vb) {
  __shared__ double red[256];
  const int i = blockIdx.x, t = threadIdx.x;
  double* Wr = md.W + (size_t)i * 3 * md.Lm;
  double s = 0;
  for (int l = t; l < md.Lm; l += 256) {
    const double w0 = Wr[3 * l], w1 = Wr[3 * l + 1], w2 = Wr[3 * l + 2];
    s += w0 * vb[3 * l] + w1 * vb[3 * l + 1] + w2 * vb[3 * l + 2];
    const double* Nm = md.V + 9 * (size_t)l;
    Wr[3 * l] = w0 * Nm[0] + w1 * Nm[3] + w2 * Nm[6];
    Wr[3 * l + 1] = w0 * Nm[1] + w1 * Nm[4] + w2 * Nm[7];
    Wr[3 * l + 2] = w0 * Nm[2] + w1 * Nm[5] + w2 * Nm[8];
  }
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) md.ba[i] -= red[0];
}
// U -= Mu Mu^T: 16 x 16 tiles on v_mfma_f64_16x16x4 (A[i = l & 15][k = l >> 4], B[k][j = l & 15], C: column l & 15, row
// (l >> 4) + 4 reg), one wave per tile over all 3 Lm columns of Mu in order (deterministic).  One thread per entry streaming
// two rows of Mu from global memory took 100-180 us.
__global__ __launch_bounds__(64) void k_marg_lm_update(MargDev md) {
  const int tr = (md.m + 15) >> 4, ti = blockIdx.x / tr, tj = blockIdx.x - ti * tr, l = threadIdx.x;
  const int K = 3 * md.Lm;
  const int ra = ti * 16 + (l & 15), rb = tj * 16 + (l & 15);
  const double* pa = md.W + (size_t)min(ra, md.m - 1) * K;
  const double* pb = md.W + (size_t)min(rb, md.m - 1) * K;
  const bool okA = ra < md.m, okB = rb < md.m;
  typedef double d4m __attribute__((ext_vector_type(4)));
  d4m acc = {0.0, 0.0, 0.0, 0.0};
  for (int kk = 0; kk < K; kk += 4) {
    const int k = kk + (l >> 4);
    const double av = (okA && k < K) ? pa[k] : 0.0, bv = (okB && k < K) ? pb[k] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
  }
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int r = ti * 16 + (l >> 4) + 4 * rg, c = tj * 16 + (l & 15);
    if (r < md.m && c < md.m) md.U[(size_t)r * md.m + c] -= acc[rg];
  }
}

// ---------------------------------------------------------------- M2 dense part (:622-667) + M3 (:725-758)
// Single workgroup.  keep/marg index lists select rows of U (m x m).  Outputs the reduced Hk (nk x nk), bk.
struct DenseArgs {
  int m, nk, nm;
  const int* keep; const int* marg;
  const double* U; const double* ba;
  double *Hk, *bk;          // outputs
  double *Vm, *Qm, *tmp;    // scratch: nm x nm, nm x nm, nk x nm + 2 nm
  int* flag;
};
__global__ __launch_bounds__(1024) void k_marg_dense(DenseArgs a, int useLds, int prodLds, int tileChol) {
  extern __shared__ double jacobiLds[];
  const int t = threadIdx.x, nt = blockDim.x, nm = a.nm, nk = a.nk, m = a.m;
  double* pm = a.tmp;                 // nm
  double* tv = a.tmp + nm;            // nm
  double* Mu = a.tmp + 2 * nm;        // nk x nm
  for (int i = t; i < nm; i += nt) {
    const double hd = a.U[(size_t)a.marg[i] * m + a.marg[i]];
    pm[i] = (hd > 1.0e-9) ? sqrt(hd) : 1.0e-3;
  }
  __syncthreads();
  // V' = 0.5 (V + V^T) scaled ; Q = I
  for (int idx = t; idx < nm * nm; idx += nt) {
    const int i = idx / nm, j = idx % nm;
    const double v = 0.5 * (a.U[(size_t)a.marg[i] * m + a.marg[j]] + a.U[(size_t)a.marg[j] * m + a.marg[i]]);
    a.Vm[idx] = v / (pm[i] * pm[j]);
    a.Qm[idx] = (i == j) ? 1.0 : 0.0;
  }
  __syncthreads();
  // The pseudo-inverse of V' drops the eigenvalues <= eps nm lambda_max (MarginalizationError.hpp:48-220).  The marginalised
  // pose / speed-bias block is well conditioned in every frame of the sliding windows (eigenvalues of V' 0.5 .. 1.7, unit
  // diagonal), and then NOTHING is dropped and (V')^+ = (V')^-1 = R^-1 R^-T: a Cholesky factor is a proof -- lambda_min >=
  // 1 / trace(V'^-1) = 1 / |R^-1|_F^2 and lambda_max <= trace(V') = nm, so 1 / |R^-1|_F^2 > eps nm^2 certifies the rank rule's
  // outcome without an eigenvalue -- and N = D^-1 R^-1 replaces D^-1 Q sqrt(1 / lambda) (N N^T is the same matrix).  The
  // eigen-solve below remains for blocks the certificate does not cover (a non-positive pivot, a gauge freedom in the block).
  __shared__ int sDirect;
  if (t == 0) sDirect = 0;
  __syncthreads();
  if (tileChol) {   // blocked on 16 x 16 MFMA tiles (tileCholFactor / tileCholInverse above; the unblocked first version took ~40 us at nm = 27)
    const int nTm = (nm + 15) >> 4, NPm = 16 * nTm, ldm = NPm + 1;
    lds_double* A = toLds(jacobiLds);
    double* DgGen = jacobiLds + (size_t)NPm * ldm;
    double* dinvGen = DgGen + nTm * 16 * kPanelLd;
    const lds_double* Dg = toLds(DgGen);
    const lds_double* dinv = toLds(dinvGen);
    __shared__ int sFailD;
    __shared__ double sFroD[16];
    if (t == 0) sFailD = 0;
    for (int idx = t; idx < NPm * ldm; idx += nt) {
      const int r = idx / ldm, c = idx - r * ldm;
      A[idx] = (r < nm && c < nm) ? a.Vm[(size_t)r * nm + c] : ((r == c) ? 1.0 : 0.0);
    }
    __syncthreads();
    tileCholFactor<16>(A, ldm, nTm, DgGen, dinvGen, &sFailD);
    if (!sFailD) {   // (uniform)
      const double fro = waveSumM(tileCholInverse<16>(A, ldm, nTm, nm, Dg, dinv));
      if ((t & 63) == 0) sFroD[t >> 6] = fro;
      __syncthreads();
      if (t == 0) {
        double f2 = 0;
        for (int w = 0; w < 16; ++w) f2 += sFroD[w];
        sDirect = (f2 > 0.0 && f2 < 1.0e300 && 1.0 / f2 > 2.220446049250313e-16 * (double)nm * (double)nm) ? 1 : 0;
      }
      __syncthreads();
      if (sDirect) {   // N^T row j = column j of N = D^-1 R^-1 e_j, R^-1 = L^-T: N^T[j][i] = L^-1[j][i] / pm[i], i <= j
        for (int idx = t; idx < nm * nm; idx += nt) {
          const int j = idx / nm, i = idx - j * nm;
          double y = 0.0;
          if (i <= j) y = ((i >> 4) < (j >> 4)) ? (double)A[i * ldm + j] : tileLinvAt(Dg, dinv, j >> 4, j & 15, i & 15);
          a.Qm[idx] = y / pm[i];
        }
        if (t == 0) a.flag[5] = 1;
      }
    }
    __syncthreads();
  }
  if (!sDirect) {
  jacobiEig(a.Vm, a.Qm, nm, a.flag, useLds ? jacobiLds : nullptr);
  // eigenvalues, tolerance, N = D^-1 Q diag(sqrt(1/l)|0)  (column j of N = eigenvector j scaled)
  __shared__ double smax;
  for (int j = t; j < nm; j += nt) {
    double s = 0;
    for (int i = 0; i < nm; ++i) s += a.Qm[(size_t)j * nm + i] * a.Vm[(size_t)j * nm + i];
    tv[j] = s;
  }
  __syncthreads();
  if (t == 0) { double mx = tv[0]; for (int j = 1; j < nm; ++j) mx = fmax(mx, tv[j]); smax = mx; }
  __syncthreads();
  const double tol = 2.220446049250313e-16 * nm * smax;
  // overwrite Q rows: N^T row j = sqrt(1/l_j) * q_j / pm
  for (int idx = t; idx < nm * nm; idx += nt) {
    const int j = idx / nm, i = idx % nm;
    const double sc = (tv[j] > tol) ? sqrt(1.0 / tv[j]) : 0.0;
    a.Qm[idx] = a.Qm[idx] * sc / pm[i];
  }
  if (t == 0) a.flag[5] = 0;
  }
  __syncthreads();
  // Mu = W N  (W = U[keep, marg]) : Mu[r][j] = sum_i W[r][i] N[i][j] = sum_i W[r][i] Qm[j][i]; then Hk = U[keep, keep] - Mu Mu^T,
  // bk = ba[keep] - Mu (N^T b_m).  With W, N^T and Mu staged in LDS when the launch has room for them (prodLds: every operand
  // used to come from global memory once per multiply-add -- a third of this kernel's 220 us at nk = 117, nm = 27).
  if (prodLds) {
    __syncthreads();
    double* sW = jacobiLds;                    // nk x nm
    double* sN = sW + (size_t)nk * nm;         // nm x nm (row j = column j of N)
    double* sMu = sN + (size_t)nm * nm;        // nk x nm
    for (int idx = t; idx < nk * nm; idx += nt) { const int r = idx / nm, i = idx - r * nm; sW[idx] = a.U[(size_t)a.keep[r] * m + a.marg[i]]; }
    for (int idx = t; idx < nm * nm; idx += nt) sN[idx] = a.Qm[idx];
    __syncthreads();
    for (int idx = t; idx < nk * nm; idx += nt) {
      const int r = idx / nm, j = idx - r * nm;
      double s = 0;
      for (int i = 0; i < nm; ++i) s += sW[r * nm + i] * sN[j * nm + i];
      sMu[idx] = s;
      Mu[idx] = s;
    }
    for (int j = t; j < nm; j += nt) {
      double s = 0;
      for (int i = 0; i < nm; ++i) s += sN[j * nm + i] * a.ba[a.marg[i]];
      pm[j] = s;  // pm reused
    }
    __syncthreads();
    for (int idx = t; idx < nk * nk; idx += nt) {
      const int r = idx / nk, c = idx - r * nk;
      double s = 0;
      for (int j = 0; j < nm; ++j) s += sMu[r * nm + j] * sMu[c * nm + j];
      a.Hk[idx] = a.U[(size_t)a.keep[r] * m + a.keep[c]] - s;
    }
    for (int r = t; r < nk; r += nt) {
      double s = 0;
      for (int j = 0; j < nm; ++j) s += sMu[r * nm + j] * pm[j];
      a.bk[r] = a.ba[a.keep[r]] - s;
    }
    return;
  }
  for (int idx = t; idx < nk * nm; idx += nt) {
    const int r = idx / nm, j = idx % nm;
    double s = 0;
    for (int i = 0; i < nm; ++i) s += a.U[(size_t)a.keep[r] * m + a.marg[i]] * a.Qm[(size_t)j * nm + i];
    Mu[idx] = s;
  }
  // tv2 = N^T b_m
  __syncthreads();
  for (int j = t; j < nm; j += nt) {
    double s = 0;
    for (int i = 0; i < nm; ++i) s += a.Qm[(size_t)j * nm + i] * a.ba[a.marg[i]];
    pm[j] = s;  // pm reused
  }
  __syncthreads();
  for (int idx = t; idx < nk * nk; idx += nt) {
    const int r = idx / nk, c = idx % nk;
    double s = 0;
    for (int j = 0; j < nm; ++j) s += Mu[(size_t)r * nm + j] * Mu[(size_t)c * nm + j];
    a.Hk[idx] = a.U[(size_t)a.keep[r] * m + a.keep[c]] - s;
  }
  for (int r = t; r < nk; r += nt) {
    double s = 0;
    for (int j = 0; j < nm; ++j) s += Mu[(size_t)r * nm + j] * pm[j];
    a.bk[r] = a.ba[a.keep[r]] - s;
  }
}

// M3: H = U S U^T of the Jacobi-preconditioned H; J = (p U sqrt(S))^T, e0 = -(sqrt(S)^+ U^T p^-1) b0;
// plus the H-space form used by the solver: Ht = J^T J, bp = J^T e0, c0 = e0.e0 (out[0]).
struct FinalArgs {
  int n;
  const double* H; const double* b0;
  double *G, *Q, *J, *e0, *Ht, *bp, *scal, *tmp;
  int* flag;
};
__device__ __forceinline__ double margScale(double hd) { return (hd > 1.0e-9) ? sqrt(hd) : 1.0e-3; }

// ---- Cholesky-preconditioned solve (mode 4, Veselic / Hari): A + delta I = R^T R, then one-sided Jacobi on the rows of R
// (the columns of L = R^T).  R V = Sigma U^T with U the eigenvectors of A and sigma_j^2 = lambda_j + delta, so the
// eigenvectors come out of the rotated rows themselves - no Q, no rotation log, no second workgroup - and because the
// rows of R carry the square roots of the spectrum (condition 1e6 instead of 1e15 for the columns of A) the tournament
// converges in 11-12 sweeps instead of 18-19.  delta = 64 n eps (A has a unit diagonal) keeps the factorisation away
// from the rounding-negative eigenvalues of the numerically semidefinite A and is removed again from sigma^2 exactly
// (sigma^2 >= delta is computed to relative precision); an eigen-direction is reliable to eps |R| / sigma_j, i.e. 1e-10 for
// the null space (which is dropped) and better than 1e-12 for everything above 1e-8.  Returns false (uniformly) if a
// pivot is not positive; the caller then runs the two-phase solve.
// P = lds_double* (the image in LDS, n <= 136) or double* (the image in a.G: larger priors; the same arithmetic at
// global-memory latency, still 2-3x faster than mode 0 for its fewer sweeps and the missing Q).
template <class P>
__device__ bool margFinalCholesky(const FinalArgs& a, P lds, int ld) {
  constexpr bool inLds = std::is_same<P, lds_double*>::value;
  const int t = threadIdx.x, nt = blockDim.x, n = a.n;
  const int wave = t >> 6, lane = t & 63, nWaves = nt >> 6;
  const int grp = t >> 4, gl = t & 15, nGroups = nt >> 4;
  double* p = a.tmp;            // n
  double* ev = a.tmp + n;       // n
  double* rsig = a.tmp + 2 * n; // n: 1 / sigma_j
  const double delta = 64.0 * n * 2.220446049250313e-16;
  const long long tStart = wall_clock64();
  for (int i = t; i < n; i += nt) p[i] = margScale(a.H[(size_t)i * n + i]);
  __syncthreads();
  // upper triangle of A + delta I, the rest (lower triangle and the padding) zero
  for (int idx = t; idx < n * ld; idx += nt) {
    const int r = idx / ld, c = idx - r * ld;
    double v = 0.0;
    if (c >= r && c < n)
      v = 0.5 * (a.H[(size_t)r * n + c] + a.H[(size_t)c * n + r]) / (p[r] * p[c]) + (r == c ? delta : 0.0);
    lds[idx] = v;
  }
  __syncthreads();
  // right-looking Cholesky on the upper triangle; row k is left unscaled (A[j][i] -= A[k][j] A[k][i] / A[k][k]) so that
  // a step is one pass and one barrier, and scaled afterwards
  for (int k = 0; k < n - 1; ++k) {
    const double pivot = lds[k * ld + k];
    if (!(pivot > 0.0)) return false;
    const double rp = 1.0 / pivot;
    for (int j = k + 1 + wave; j < n; j += nWaves) {
      const double f = lds[k * ld + j] * rp;
      for (int i = j + lane; i < n; i += 64) lds[j * ld + i] -= f * lds[k * ld + i];
    }
    if (inLds) ldsBarrier(); else __syncthreads();
  }
  if (!(lds[(n - 1) * ld + (n - 1)] > 0.0)) return false;
  for (int k = wave; k < n; k += nWaves) {
    const double rs = rsqrt(lds[k * ld + k]);
    for (int i = k + lane; i < n; i += 64) lds[k * ld + i] *= rs;
  }
  __syncthreads();
  const long long tPrep = wall_clock64(), cPrep = clock64();
  if (inLds) {
    switch ((n + kJacobiLanes - 1) / kJacobiLanes) {   // slices per column: <= 9 for the LDS image (n <= 136)
      case 1: jacobiEigBlock<kJacobiLanes, P, false, 1>(lds, (P) nullptr, n, ld, a.flag); break;
      case 2: jacobiEigBlock<kJacobiLanes, P, false, 2>(lds, (P) nullptr, n, ld, a.flag); break;
      case 3: jacobiEigBlock<kJacobiLanes, P, false, 3>(lds, (P) nullptr, n, ld, a.flag); break;
      case 4: jacobiEigBlock<kJacobiLanes, P, false, 4>(lds, (P) nullptr, n, ld, a.flag); break;
      case 5: jacobiEigBlock<kJacobiLanes, P, false, 5>(lds, (P) nullptr, n, ld, a.flag); break;
      case 6: jacobiEigBlock<kJacobiLanes, P, false, 6>(lds, (P) nullptr, n, ld, a.flag); break;
      case 7: jacobiEigBlock<kJacobiLanes, P, false, 7>(lds, (P) nullptr, n, ld, a.flag); break;
      case 8: jacobiEigBlock<kJacobiLanes, P, false, 8>(lds, (P) nullptr, n, ld, a.flag); break;
      default: jacobiEigBlock<kJacobiLanes, P, false, 9>(lds, (P) nullptr, n, ld, a.flag); break;
    }
  } else {
    jacobiEigBlock<kJacobiLanes, P, false>(lds, (P) nullptr, n, ld, a.flag);
  }
  const long long tEig = wall_clock64(), cEig = clock64();
  // row j = sigma_j u_j
  for (int j = grp; j < n; j += nGroups) {
    double s = 0;
    for (int i = gl; i < n; i += 16) { const double x = lds[j * ld + i]; s += x * x; }
    s = rowSum16(s);
    if (gl == 0) { ev[j] = s - delta; rsig[j] = rsqrt(s); }
  }
  __syncthreads();
  if (t < 64) {
    double mx = -1.0e300, mn = 1.0e300;
    for (int j = t; j < n; j += 64) { mx = fmax(mx, ev[j]); mn = fmin(mn, ev[j]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mx = fmax(mx, __shfl_xor(mx, o, 64)); mn = fmin(mn, __shfl_xor(mn, o, 64)); }
    const double tl = 2.220446049250313e-16 * n * mx;
    int c = 0;
    for (int j = t; j < n; j += 64) c += ev[j] <= tl;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (t == 0) { gJacobiShared.nullTol2 = mx; a.flag[2] = c; a.scal[1] = mn; a.scal[2] = mx; }
  }
  __syncthreads();
  const double tol = 2.220446049250313e-16 * n * gJacobiShared.nullTol2;
  for (int i = grp; i < n; i += nGroups) {
    double e = 0;
    for (int j = gl; j < n; j += 16) e += lds[i * ld + j] * (a.b0[j] / p[j]);
    e = rowSum16(e);
    if (gl == 0) a.e0[i] = ev[i] > tol ? -sqrt(1.0 / ev[i]) * (e * rsig[i]) : 0.0;
  }
  __syncthreads();
  // J = (p U sqrt(S))^T in place of the rows
  for (int idx = t; idx < n * n; idx += nt) {
    const int i = idx / n, j = idx - i * n;
    const double s = ev[i] > tol ? sqrt(ev[i]) * rsig[i] : 0.0;
    const double v = p[j] * lds[i * ld + j] * s;
    a.J[idx] = v;
    lds[i * ld + j] = v;
  }
  __syncthreads();
  // One step of refinement of e0 against J^T e0 = -b0 (on the kept directions): the rows the Jacobi leaves are orthogonal to
  // kJacobiOrthTol = 2e-14 only, and e0 above takes them for orthogonal -- J^T e0 + b0 came out at 125 eps of a scaled unit at
  // n = 17.  rho = -b0 - J^T e0, e0_i += (J_i / p) . (rho / p) / lambda_i.
  {
    double* rho = rsig;   // (1 / sigma is not read again)
    for (int j = t; j < n; j += nt) {
      double s = 0;
      for (int k = 0; k < n; ++k) s += lds[k * ld + j] * a.e0[k];
      rho[j] = (-a.b0[j] - s) / (p[j] * p[j]);
    }
    __syncthreads();
    for (int i = grp; i < n; i += nGroups) {
      double e = 0;
      for (int j = gl; j < n; j += 16) e += lds[i * ld + j] * rho[j];
      e = rowSum16(e);
      if (gl == 0 && ev[i] > tol) a.e0[i] += e / ev[i];
    }
    __syncthreads();
  }
  for (int idx = t; idx < n * n; idx += nt) {
    const int i = idx / n, j = idx - i * n;
    double s = 0;
    for (int k = 0; k < n; ++k) s += lds[k * ld + i] * lds[k * ld + j];
    a.Ht[idx] = s;
  }
  for (int i = t; i < n; i += nt) {
    double s = 0;
    for (int k = 0; k < n; ++k) s += lds[k * ld + i] * a.e0[k];
    a.bp[i] = s;
  }
  if (t < 64) {
    double c = 0;
    for (int k = t; k < n; k += 64) c += a.e0[k] * a.e0[k];
    c = waveSumM(c);
    if (t == 0) {
      a.scal[0] = c;
      a.scal[3] = (double)(tPrep - tStart); a.scal[4] = (double)(tEig - tPrep); a.scal[5] = (double)(wall_clock64() - tEig);
      a.scal[6] = (double)(cEig - cPrep);
      a.scal[7] = (double)n;
      a.flag[3] = inLds ? -4 : -6;   // marks the mode in the SVIN_MARG_TIMING line
    }
  }
  return true;
}

// ---- M3 without an eigenvalue, when the prior has full numerical rank (round 5).  The reference drops the eigen-directions of the
// Jacobi-scaled H = p A p with lambda <= eps n lambda_max (MarginalizationError.cpp:739-742) and takes J = (p U sqrt(S))^T,
// e0 = -(sqrt(S)^+ U^T p^-1) b0.  The optimiser sees the prior through J^T J, J^T e0 and e0.e0 only, which ANY square root of
// the kept part delivers -- and when nothing is dropped, the Cholesky factor is one: A = R^T R, J = R p, e0 = -R^-T p^-1 b0,
// J^T J = H, J^T e0 = -b0.  "Nothing is dropped" is certified, not assumed: lambda_min >= 1 / trace(A^-1) = 1 / |R^-1|_F^2 and
// lambda_max <= trace(A) = n (unit diagonal), so 1 / |R^-1|_F^2 > eps n^2 implies every eigenvalue is above the reference's
// threshold.  Steady-state priors of both sliding windows pass (smallest eigenvalue 1e-8, threshold 9e-14); a prior with a
// gauge freedom, a non-positive pivot or a failed certificate writes flag[4] = 0 and k_marg_final_dc, enqueued behind, does
// the eigen-solve.  One workgroup, everything in 16 x 16 tiles on v_mfma_f64_16x16x4 (the unblocked first version -- one barrier
// per column, R^-1 column by column on 8 lanes -- took 107 + 154 us at n = 117):
//   * A = L L^T blocked right-looking over the lower tiles of the LDS image (identity padding to a multiple of 16): per block
//     column the diagonal tile by wave 0 out of registers (cholDiag16Acc of the dense solvers, tile16.hpp: L and L^-1 of the tile
//     into a 16 x 17 scratch tile), the panel tiles X = A_IK L_KK^-T one per wave, the trailing tiles A_IJ -= X_I X_J^T dealt over
//     the 16 waves; three barriers per block column, eight block columns at n = 117;
//   * Y = L^-1 one block column per wave without a barrier: Y_JJ is the scratch tile's inverse, Y_IJ = -L_II^-1 sum_K L_IK Y_KJ
//     with the running sum in the accumulator layout, which IS the B operand of the product with L_II^-1; Y_IJ^T goes to the upper
//     tile (J, I), which the factorisation never reads, so element Y[i][j] sits at image[j][i];
//   * |Y|_F^2 (the certificate), e0 = -Y (b0 / p) (8 lanes per row), J = L^T p, Ht = the symmetrised H, bp = -b0, c0 = e0.e0.
__global__ __launch_bounds__(1024) void k_marg_final_chol(FinalArgs a) {
  extern __shared__ double jacobiLds[];
  const int t = threadIdx.x, nt = 1024, n = a.n, nT = (n + 15) >> 4, NP = 16 * nT, ld = NP + 1;
  const int wave = t >> 6, lane = t & 63, g = lane >> 4, c = lane & 15;
  lds_double* A = toLds(jacobiLds);                       // NP x ld image
  double* DgGen = jacobiLds + (size_t)NP * ld;            // nT scratch tiles (16 x kPanelLd): L (lower) | L^-1 transposed (strict upper)
  double* dinvGen = DgGen + nT * 16 * kPanelLd;           // 1 / L_ii
  lds_double* Dg = toLds(DgGen);
  lds_double* dinv = toLds(dinvGen);
  double* p = a.tmp;            // n
  double* bt = a.tmp + n;       // n: b0 / p
  __shared__ double sFro[16];
  __shared__ int sOk, sFail;
  const long long tStart = wall_clock64();
  if (t == 0) { a.flag[4] = 0; sFail = 0; }
  for (int i = t; i < n; i += nt) { const double pi = margScale(a.H[(size_t)i * n + i]); p[i] = pi; bt[i] = a.b0[i] / pi; }
  __syncthreads();
  for (int idx = t; idx < NP * ld; idx += nt) {
    const int r = idx / ld, cc = idx - r * ld;
    A[idx] = (r < n && cc < n) ? 0.5 * (a.H[(size_t)r * n + cc] + a.H[(size_t)cc * n + r]) / (p[r] * p[cc]) : ((r == cc) ? 1.0 : 0.0);
  }
  __syncthreads();
  tileCholFactor<16, true>(A, ld, nT, DgGen, dinvGen, &sFail);   // (refined panels: L leaves the library as J)
  if (sFail) return;   // (uniform) a pivot was not positive: the eigen-solve behind this launch decides
  const long long tChol = wall_clock64();
  {
    const double fro = waveSumM(tileCholInverse<16>(A, ld, nT, n, Dg, dinv));
    if (lane == 0) sFro[wave] = fro;
  }
  __syncthreads();
  // e0 = -Y (b0 / p): 8 lanes per row
  {
    const int i = t >> 3, sub = t & 7;
    double e = 0.0;
    if (i < n) {
      const int bi = i >> 4;
      for (int j = sub; j <= i; j += 8) {
        const double yv = ((j >> 4) < bi) ? (double)A[j * ld + i] : tileLinvAt(Dg, dinv, bi, i & 15, j & 15);
        e = __builtin_fma(yv, bt[j], e);
      }
    }
    e = symeig::sum8(e);
    if (i < n && sub == 0) a.e0[i] = -e;
  }
  // One step of refinement against L e0 = -b0 / p: the product with the explicit inverse leaves J^T e0 + b0 at kappa(L) eps
  // (4 700 eps of a scaled unit on a prior of condition 7e8 that passes the certificate), the step brings it to a few n eps.
  {
    double* rho = a.tmp + 2 * n;   // n: b0 / p + L e0
    __syncthreads();
    const int i = t >> 3, sub = t & 7;
    double r = 0.0;
    if (i < n) {
      const int bi = i >> 4;
      for (int j = sub; j <= i; j += 8) {
        const double lv = ((j >> 4) < bi) ? (double)A[i * ld + j] : (double)Dg[bi * 16 * kPanelLd + (i & 15) * kPanelLd + (j & 15)];
        r = __builtin_fma(lv, a.e0[j], r);
      }
    }
    r = symeig::sum8(r);
    if (i < n && sub == 0) rho[i] = bt[i] + r;
    __syncthreads();
    double e = 0.0;
    if (i < n) {
      const int bi = i >> 4;
      for (int j = sub; j <= i; j += 8) {
        const double yv = ((j >> 4) < bi) ? (double)A[j * ld + i] : tileLinvAt(Dg, dinv, bi, i & 15, j & 15);
        e = __builtin_fma(yv, rho[j], e);
      }
    }
    e = symeig::sum8(e);
    if (i < n && sub == 0) a.e0[i] -= e;
  }
  if (t == 0) {
    double f2 = 0;
    for (int w = 0; w < 16; ++w) f2 += sFro[w];
    sOk = (f2 > 0.0 && f2 < 1.0e300 && 1.0 / f2 > 2.220446049250313e-16 * (double)n * (double)n) ? 1 : 0;
    a.scal[1] = f2 > 0.0 ? 1.0 / f2 : 0.0;   // (a lower bound of the smallest eigenvalue, an upper bound of the largest)
    a.scal[2] = (double)n;
  }
  __syncthreads();
  if (!sOk) return;
  // J = L^T p (row i = column i of L, columns scaled), Ht = the symmetrised H itself (= J^T J), bp = J^T e0 = -b0, c0 = e0.e0
  for (int idx = t; idx < n * n; idx += nt) {
    const int i = idx / n, j = idx - i * n;
    double lji = 0.0;   // L[j][i], j >= i
    if (j >= i) lji = ((j >> 4) > (i >> 4)) ? (double)A[j * ld + i] : (double)Dg[(j >> 4) * 16 * kPanelLd + (j & 15) * kPanelLd + (i & 15)];
    a.J[idx] = lji * p[j];
    a.Ht[idx] = 0.5 * (a.H[idx] + a.H[(size_t)j * n + i]);
  }
  for (int i = t; i < n; i += nt) a.bp[i] = -a.b0[i];
  __syncthreads();
  if (t < 64) {
    double cs = 0;
    for (int k = t; k < n; k += 64) cs += a.e0[k] * a.e0[k];
    cs = waveSumM(cs);
    if (t == 0) {
      a.scal[0] = cs;
      a.scal[3] = 0.0; a.scal[4] = (double)(tChol - tStart); a.scal[5] = (double)(wall_clock64() - tChol);
      a.scal[6] = 0.0;
      a.scal[7] = (double)n;
      a.flag[1] = 0; a.flag[2] = 0;
      a.flag[3] = -8;   // marks the mode in the SVIN_MARG_TIMING line
      __threadfence();
      a.flag[4] = 1;
    }
  }
}

// ---- M3 by a direct eigen-solve (round 5): tridiagonalisation + divide and conquer (symeig.hpp) instead of ~1 400 dependent
// Jacobi rounds.  H = p A p (A with a unit diagonal), A = U S U^T; J = (p U sqrt(S))^T, e0 = -(sqrt(S)^+ U^T p^-1) b0 with the
// eigenvalues <= eps n lambda_max dropped (MarginalizationError.cpp:739-742), and the H-space form the solver reads: Ht = J^T J,
// bp = J^T e0, c0 = e0.e0.  Writes flag[4] = 1 when it has produced the prior; k_marg_final, enqueued right behind it with
// `skipIfDone`, then returns at once -- otherwise (a non-finite result) it runs the Jacobi solve as before.
__global__ __launch_bounds__(1024) void k_marg_final_dc(FinalArgs a, int skipIfDone) {
  extern __shared__ double jacobiLds[];
  if (skipIfDone && a.flag[4] == 1) return;   // k_marg_final_chol, enqueued ahead of this launch, has produced the prior
  lds_double* X = toLds(jacobiLds);
  const int t = threadIdx.x, n = a.n, ld = n | 1;
  double* p = a.tmp;            // n
  double* ev = a.tmp + n;       // n
  const long long tStart = wall_clock64();
  for (int i = t; i < n; i += 1024) p[i] = margScale(a.H[(size_t)i * n + i]);
  __syncthreads();
  for (int idx = t; idx < n * ld; idx += 1024) {
    const int r = idx / ld, c = idx - r * ld;
    X[idx] = (c < n) ? 0.5 * (a.H[(size_t)r * n + c] + a.H[(size_t)c * n + r]) / (p[r] * p[c]) : 0.0;
  }
  __syncthreads();
  const long long tPrep = wall_clock64();
  const bool ok = symeig::solve(X, n, ld, a.G);
  const long long tEig = wall_clock64();
  if (!ok) {
    if (t == 0) a.flag[4] = 0;
    return;
  }
  // X[i * ld + j] = component i of eigenvector j, symeig::gS.d[j] = eigenvalue j (ascending).  Per-vector scalars once, in LDS
  // (the solver's per-phase arrays are free again): sq = sqrt(l) or 0 (dropped), lamp = l or 0, bt = b0 / p
  double* sq = symeig::gS.u.dc.z;
  double* lamp = symeig::gS.u.dc.dcur;
  double* bt = symeig::gS.u.dc.ztil;
  double* e0s = symeig::gS.u.dc.cd;
  const double mx = symeig::gS.d[n - 1], mn = symeig::gS.d[0];
  const double tol = 2.220446049250313e-16 * n * mx;
  if (t < n) {
    const double l = symeig::gS.d[t];
    ev[t] = l;
    lamp[t] = l > tol ? l : 0.0;
    sq[t] = l > tol ? sqrt(l) : 0.0;
    bt[t] = a.b0[t] / p[t];
  }
  if (t < 64) {
    int c = 0;
    for (int j = t; j < n; j += 64) c += symeig::gS.d[j] <= tol;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (t == 0) { a.flag[2] = c; a.flag[1] = 0; a.scal[1] = mn; a.scal[2] = mx; }
  }
  symeig::ldsBarrier();
  // e0_j = -(1 / sqrt(l_j)) u_j . (b0 / p): 8 lanes per eigenvector
  {
    const int j = t >> 3, sub = t & 7;
    double s = 0;
    if (j < n)
      for (int i = sub; i < n; i += 8) s += X[i * ld + j] * bt[i];
    s = symeig::sum8(s);
    if (j < n && sub == 0) { const double e = sq[j] > 0.0 ? -s / sq[j] : 0.0; a.e0[j] = e; e0s[j] = e; }
  }
  // J = (p U sqrt(S))^T: row j = eigen-direction j
  for (int idx = t; idx < n * n; idx += 1024) {
    const int j = idx / n, i = idx - j * n;
    a.J[idx] = p[i] * X[i * ld + j] * sq[j];
  }
  symeig::ldsBarrier();
  // Ht = J^T J = p (U S U^T) p: 16 x 16 tiles on v_mfma_f64_16x16x4, both operands rows of X
  {
    const int wave = t >> 6, l = t & 63, tr = (n + 15) >> 4;
    for (int id = wave; id < tr * tr; id += 16) {
      const int ra = (id / tr) * 16 + (l & 15), cb = (id % tr) * 16 + (l & 15);
      symeig::d4 acc = {0.0, 0.0, 0.0, 0.0};
      for (int kk = 0; kk < n; kk += 4) {
        const int j = kk + (l >> 4);
        const double av = (ra < n && j < n) ? (double)X[ra * ld + j] : 0.0;
        const double bv = (cb < n && j < n) ? (double)X[cb * ld + j] * lamp[j] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int r = (id / tr) * 16 + (l >> 4) + 4 * rg;
        if (r < n && cb < n) a.Ht[(size_t)r * n + cb] = acc[rg] * p[r] * p[cb];
      }
    }
  }
  // bp = J^T e0
  {
    const int i = t >> 3, sub = t & 7;
    double s = 0;
    if (i < n)
      for (int j = sub; j < n; j += 8) s += X[i * ld + j] * (sq[j] * e0s[j]);
    s = symeig::sum8(s);
    if (i < n && sub == 0) a.bp[i] = p[i] * s;
  }
  if (t < 64) {
    double c = 0;
    for (int k = t; k < n; k += 64) c += e0s[k] * e0s[k];
    c = waveSumM(c);
    if (t == 0) {
      a.scal[0] = c;
      a.scal[3] = (double)(tPrep - tStart); a.scal[4] = (double)(tEig - tPrep); a.scal[5] = (double)(wall_clock64() - tEig);
      a.scal[6] = 0.0;
      a.scal[7] = (double)n;
      a.flag[3] = -7;   // marks the mode in the SVIN_MARG_TIMING line
      __threadfence();
      a.flag[4] = 1;
    }
  }
}

// inspection hook (svin_ba_debug_sym_eig): the solver on an arbitrary symmetric matrix
__global__ __launch_bounds__(1024) void k_sym_eig_debug(int n, const double* A, double* lam, double* Xout, double* scratch, int* okOut) {
  extern __shared__ double jacobiLds[];
  lds_double* X = toLds(jacobiLds);
  const int t = threadIdx.x, ld = n | 1;
  for (int idx = t; idx < n * ld; idx += 1024) {
    const int r = idx / ld, c = idx - r * ld;
    X[idx] = (c < n) ? 0.5 * (A[(size_t)r * n + c] + A[(size_t)c * n + r]) : 0.0;
  }
  __syncthreads();
  const bool ok = symeig::solve(X, n, ld, scratch);
  if (t == 0) *okOut = ok ? 1 : 0;
  if (t < n) lam[t] = symeig::gS.d[t];
#ifdef SVIN_SYMEIG_TIMING
  if (t < 80) scratch[t] = t < symeig::gS.nstamp ? (double)(symeig::gS.stamp[t] - symeig::gS.stamp[0]) : -1.0;
#endif
  for (int idx = t; idx < n * n; idx += 1024) { const int i = idx / n, j = idx - i * n; Xout[idx] = X[i * ld + j]; }
}
int debugSymEig(int n, const double* A, double* lam, double* X, double* deviceMs) {
  if (n < 1 || n > kSymEigMaxN) return 0;
  // (a test hook that bench and tests call repeatedly: buffers and events are released on every path, also when a HIP call throws)
  struct Scratch {
    double* dA = nullptr; int* dOk = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Scratch() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
      if (dA) (void)hipFree(dA);
      if (dOk) (void)hipFree(dOk);
    }
  } sc;
  const size_t n2 = (size_t)n * n;
  HIP_OK(hipMalloc(&sc.dA, sizeof(double) * (3 * n2 + n)));
  double *dA = sc.dA, *dX = dA + n2, *dS = dX + n2, *dLam = dS + n2;
  HIP_OK(hipMalloc(&sc.dOk, sizeof(int)));
  int* dOk = sc.dOk;
  HIP_OK(hipMemcpy(dA, A, sizeof(double) * n2, hipMemcpyHostToDevice));
  const size_t lds = symEigLdsBytes(n);
  HIP_OK(hipEventCreate(&sc.e0)); HIP_OK(hipEventCreate(&sc.e1));
  const hipEvent_t e0 = sc.e0, e1 = sc.e1;
  float best = 1e30f;
  for (int rep = 0; rep < 3; ++rep) {   // (the first launch pays the code upload)
    HIP_OK(hipEventRecord(e0, 0));
    launch(k_sym_eig_debug, dim3(1), dim3(1024), lds, 0, n, dA, dLam, dX, dS, dOk);
    HIP_OK(hipEventRecord(e1, 0));
    HIP_OK(hipEventSynchronize(e1));
    float ms = 0; HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    best = std::min(best, ms);
  }
  int ok = 0;
  HIP_OK(hipMemcpy(&ok, dOk, sizeof(int), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(lam, dLam, sizeof(double) * n, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(X, dX, sizeof(double) * n2, hipMemcpyDeviceToHost));
#ifdef SVIN_SYMEIG_TIMING
  if (n2 >= 80) {   // stage stamps of the last launch (100 MHz ticks since the first), one line
    double st[80];
    HIP_OK(hipMemcpy(st, dS, sizeof(st), hipMemcpyDeviceToHost));
    std::printf("[symeig] n %d stamps(us):", n);
    for (int i = 0; i < 80 && st[i] >= 0; ++i) std::printf(" %.1f", st[i] / 100.0);
    std::printf("\n");
  }
#endif
  if (deviceMs) *deviceMs = best;
  return ok ? 1 : -1;
}

__global__ __launch_bounds__(1024) void k_marg_final(FinalArgs a, int useLds, int fallbackLds, int skipIfDone) {
  extern __shared__ double jacobiLds[];
  if (skipIfDone && a.flag[4] == 1) return;   // k_marg_final_dc, enqueued ahead of this launch, has produced the prior
  // modes: 4 = Cholesky-preconditioned Jacobi, image in LDS; 6 = the same with the image in global memory (priors too
  // large for LDS); 1 / 0 = the fall-back, one-sided Jacobi on A itself with G and Q in LDS / in global memory
  // (also what runs when a pivot of the factorisation is not positive: `fallbackLds` says whether G and Q both fit)
  if (useLds == 6) {
    if (margFinalCholesky<double*>(a, a.G, a.n)) return;
    __syncthreads();
    useLds = 0;
  } else if (useLds == 4) {
    if (margFinalCholesky<lds_double*>(a, toLds(jacobiLds), jacobiLd(a.n))) return;
    __syncthreads();
    useLds = fallbackLds ? 1 : 0;
  }
  const int t = threadIdx.x, nt = blockDim.x, n = a.n;
  double* p = a.tmp;        // n
  double* ev = a.tmp + n;   // n
  const long long tStart = wall_clock64();
  for (int i = t; i < n; i += nt) {
    const double hd = a.H[(size_t)i * n + i];
    p[i] = (hd > 1.0e-9) ? sqrt(hd) : 1.0e-3;
  }
  __syncthreads();
  for (int idx = t; idx < n * n; idx += nt) {
    const int i = idx / n, j = idx % n;
    a.G[idx] = 0.5 * (a.H[idx] + a.H[(size_t)j * n + i]) / (p[i] * p[j]);
    a.Q[idx] = (i == j) ? 1.0 : 0.0;
  }
  __syncthreads();
  const long long tPrep = wall_clock64(), cPrep = clock64();
  jacobiEig(a.G, a.Q, n, a.flag, useLds ? jacobiLds : nullptr);
  const long long tEig = wall_clock64(), cEig = clock64();
  __shared__ double smax;
  const int grp = t >> 4, gl = t & 15, nGroups = nt >> 4;   // 16-lane groups (one DPP row each)
  for (int j = grp; j < n; j += nGroups) {
    double s = 0;
    for (int i = gl; i < n; i += 16) s += a.Q[(size_t)j * n + i] * a.G[(size_t)j * n + i];
    s = rowSum16(s);
    if (gl == 0) ev[j] = s;
  }
  __syncthreads();
  if (t < 64) {
    double mx = -1.0e300, mn = 1.0e300;
    for (int j = t; j < n; j += 64) { mx = fmax(mx, ev[j]); mn = fmin(mn, ev[j]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mx = fmax(mx, __shfl_xor(mx, o, 64)); mn = fmin(mn, __shfl_xor(mn, o, 64)); }
    const double tl = 2.220446049250313e-16 * n * mx;
    int c = 0;
    for (int j = t; j < n; j += 64) c += ev[j] <= tl;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (t == 0) { smax = mx; a.flag[2] = c; a.scal[1] = mn; a.scal[2] = mx; }
  }
  __syncthreads();
  const double tol = 2.220446049250313e-16 * n * smax;
  // J = (p U sqrt(S))^T: row i = eigen-direction i; kept in LDS (when the launch has it) for the J^T J below
  const int ld = jacobiLd(n);
  lds_double* sJ = useLds ? toLds(jacobiLds) : nullptr;
  for (int idx = t; idx < n * n; idx += nt) {
    const int i = idx / n, j = idx - i * n;
    const double s = ev[i] > tol ? sqrt(ev[i]) : 0.0;
    const double v = p[j] * a.Q[idx] * s;
    a.J[idx] = v;
    if (sJ) sJ[i * ld + j] = v;
  }
  for (int i = grp; i < n; i += nGroups) {
    double e = 0;
    for (int j = gl; j < n; j += 16) e += a.Q[(size_t)i * n + j] * (a.b0[j] / p[j]);
    e = rowSum16(e);
    if (gl == 0) a.e0[i] = ev[i] > tol ? -sqrt(1.0 / ev[i]) * e : 0.0;
  }
  __syncthreads();
  if (sJ) {
    for (int idx = t; idx < n * n; idx += nt) {
      const int i = idx / n, j = idx - i * n;
      double s = 0;
      for (int k = 0; k < n; ++k) s += sJ[k * ld + i] * sJ[k * ld + j];
      a.Ht[idx] = s;
    }
    for (int i = t; i < n; i += nt) {
      double s = 0;
      for (int k = 0; k < n; ++k) s += sJ[k * ld + i] * a.e0[k];
      a.bp[i] = s;
    }
  } else {
    for (int idx = t; idx < n * n; idx += nt) {
      const int i = idx / n, j = idx % n;
      double s = 0;
      for (int k = 0; k < n; ++k) s += a.J[(size_t)k * n + i] * a.J[(size_t)k * n + j];
      a.Ht[idx] = s;
    }
    for (int i = t; i < n; i += nt) {
      double s = 0;
      for (int k = 0; k < n; ++k) s += a.J[(size_t)k * n + i] * a.e0[k];
      a.bp[i] = s;
    }
  }
  if (t < 64) {
    double c = 0;
    for (int k = t; k < n; k += 64) c += a.e0[k] * a.e0[k];
    c = waveSumM(c);
    if (t == 0) {
      a.scal[0] = c;
      // 100 MHz ticks: prepare, eigen-solve, everything after it (printed under SVIN_MARG_TIMING)
      a.scal[3] = (double)(tPrep - tStart); a.scal[4] = (double)(tEig - tPrep); a.scal[5] = (double)(wall_clock64() - tEig);
      a.scal[6] = (double)(cEig - cPrep);   // shader clocks of the eigen-solve
      a.scal[7] = (double)n;
    }
  }
}

// ================================================================ host: policy, job tables, reservation, issue, graph update
static double nowSec() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// What the policy (Estimator.cpp:509-770) takes out of the host graph in one call: the residuals to linearise, copied out of the
// graph as they are removed, and the blocks they connect
struct Window::MargSelection {
  struct JobObs { Observation o; uint64_t lmId, extId; double S[3]; bool lmFixed; };   // S: the square-root information of a general observation (o.general)
  bool hadPrior = false;
  bool deviceJob = false;       // the observation tables come out of the device-resident CSR (no JobObs, no lmLin)
  bool reDoFixation = false;    // the pose prior of a leaving frame went with it (:624-629)
  std::vector<Factor> factors;
  std::vector<JobObs> obs;
  int nObs = 0;                 // linearised reprojection residuals (both forms of the job)
  int m = 0;                    // rows of the dense part
  std::vector<uint64_t> toMarginalize, margLandmarks;
  std::vector<PriorBlockHost> dense;   // connected dense blocks in insertion order (after the blocks of the old prior) ...
  std::vector<uint64_t> lmOrder;       // ... and landmarks
  std::unordered_map<uint64_t, std::vector<double>> lmLin;   // linearisation points of marginalised landmarks
  std::vector<unsigned char> poseClass;                      // kMargRemove | kMargLin | kMargNew per pose handle
  std::vector<PriorBlockHost> kept;    // the blocks of the new prior (filled with the job tables)
};

// Everything the launches of one job read.  It is assembled on the caller's thread and then only read: by launchMarginalization,
// which may run on the handle's enqueue thread after applyMarginalizationStrategy has returned, so the closure handed to
// enqueueAsync holds the job by shared_ptr and nothing else.
struct Window::MargJob {
  MargDims dims{};
  MargPlan plan{};
  int nSb = 0, nImu = 0;
  bool deviceJob = false, lossOn = false, generalOn = false, keepPre = false;
  int margEig = 0;   // SVIN_MARG_EIG, read on the caller's thread
  hipStream_t stream = nullptr;
  // host tables at the linearisation points
  std::vector<double> hPose, hExt, hSb, hLm, hUv, hW, hS, hImuM, lossTab;
  std::vector<int> oPose, oExt, oSb, hObsLm, hLmPtr, idxLists, jobPoseSlot, jobExtSlot;
  std::vector<uint32_t> hIdx, hImuT;
  std::vector<DevFactor> hFac;
  std::vector<DevImu> hImu;
  std::vector<unsigned char> poseClass;
  std::vector<CameraModel> cams;
  std::vector<StagedCopy> pending;
  // (H | b0) of the previous prior: bHk is only ever re-allocated when it has to grow, and then the old allocation is kept alive
  // here until the job has copied out of it
  const double* oldPrior = nullptr;
  DevBuf<double> oldPriorKeep;
  // read by the SVIN_MARG_KEEP_PRE inspection
  std::vector<uint64_t> lmOrder, toMarginalize;
  std::vector<PriorBlockHost> dense;

  // Queues the upload of a table.  THE RULE: a pointer handed to flushStaged points into storage this job owns -- `host` is one
  // of the vectors above, complete when it is staged and never touched again (a vector's storage does not move with the job).
  template <class B, class V>
  void stage(B& buf, const V& host) {
    using T = typename V::value_type;
    buf.reserve(std::max<size_t>(host.size() + 16 / sizeof(T) + 1, 1));   // room for the 16-byte rounding of the copy
    if (!host.empty()) pending.push_back({host.data(), sizeof(T) * host.size(), buf.p});
  }
};

MargFrames Window::margFrames(size_t numKeyframes, size_t numImuFrames) const {
  std::vector<uint64_t> ids;
  std::vector<char> isKeyframe;
  ids.reserve(states_.size()); isKeyframe.reserve(states_.size());
  for (const auto& kv : states_) { ids.push_back(kv.second.id); isKeyframe.push_back(kv.second.isKeyframe ? 1 : 0); }
  return selectMargFrames(ids, isKeyframe, numKeyframes, numImuFrames);
}

// ---- step 1: what the kernels cannot marginalise is refused before anything is modified.  false: lastError() says why
bool Window::margAccepts(const MargFrames& frames) const {
  // A pose on a reduced manifold (Map::resetParameterization, a Map-level feature okvis::Estimator never uses: Estimator.cpp:801 is
  // commented out): the prior's columns would have to be the 3 / 4 / 2 minimal ones (MarginalizationError.cpp:147-160 takes
  // minimalDimension()).  Not built; refuse before anything is modified.
  for (const auto& kv : factors_)
    if (kv.second.kind == F_HOST)
      throw std::runtime_error("applyMarginalizationStrategy: a residual evaluated by a host cost function is in the window (its linearisation is not available to the marginalisation kernels)");
  for (const auto& kv : blocks_)
    if (kv.second.lock != 0)
      throw std::runtime_error("applyMarginalizationStrategy: a pose block on a reduced manifold (Pose3d / Pose4d / Pose2d) is in the window");
  // A constant landmark is marginalised like any other (the policy loop of Estimator.cpp:671-766 never asks): its linearised
  // observations enter the job with the negative weight, so their landmark Jacobian is zero (MarginalizationError.cpp:156 gives a
  // fixed block zero columns, :343 / :367 skip it).  Landmark-sharded handles keep refusing it.
  const bool refuseFixedLm = margRefusesFixedLandmarks();
  if (numLandmarkPriors_ == 0 && !refuseFixedLm) return true;
  // Landmarks that carry a HomogeneousPointError stay out of the marginalisation: the reference's policy loop assumes
  // every residual of a landmark is a ReprojectionError (Estimator.cpp:689-698) and never meets one, because Estimator
  // adds none.  Observed from a frame that is about to leave, such a landmark cannot be handled.
  const std::vector<uint64_t>& leaving = frames.removeFrames;
  for (const auto& kv : landmarks_) {
    if (kv.second.priors.empty() && !(refuseFixedLm && kv.second.fixed)) continue;
    for (const Observation& o : kv.second.obs)
      if (std::find(leaving.begin(), leaving.end(), o.poseId) != leaving.end()) {
        lastError() = kv.second.priors.empty()
                          ? "applyMarginalizationStrategy: a constant landmark of a landmark-sharded handle is observed from a frame that leaves the window"
                          : "applyMarginalizationStrategy: a landmark with a HomogeneousPointError is observed from a frame that leaves the window";
        return false;
      }
  }
  return true;
}

// ---- step 2: the policy (Estimator.cpp:509-770), operating on the host graph only
void Window::margApplyPolicy(const MargFrames& frames, MargSelection& sel, std::vector<uint64_t>& removed, bool timing) {
  const bool refuseFixedLm = margRefusesFixedLandmarks();
  // :509-514 the old prior leaves the graph; its content is re-used by the job
  sel.hadPrior = hasPrior_;
  if (sel.hadPrior) {
    for (const PriorBlockHost& pb : priorBlocks_)
      if (Block* b = findBlock(pb.id)) {
        for (size_t i = 0; i < b->residuals.size(); ++i)
          if (b->residuals[i] == priorResId_) { b->residuals.erase(b->residuals.begin() + i); break; }
      }
    priorResId_ = 0;
  }
  const std::vector<uint64_t>&removeFrames = frames.removeFrames, &removeAllButPose = frames.removeAllButPose,
                             &allLinearizedFrames = frames.allLinearizedFrames;
  std::vector<uint64_t>& toMarginalize = sel.toMarginalize;
  std::vector<PriorBlockHost>& dense = sel.dense;
  dense = priorBlocks_;
  // (one flag per block handle: the landmark pass asks "is it connected already" twice per linearised residual)
  std::vector<char> connected[3];
  for (int k = 0; k < 3; ++k) connected[k].assign(std::max(nextBlockH_[k], 1), 0);
  for (const PriorBlockHost& pb : dense)
    if (const Block* b = findBlock(pb.id)) connected[b->kind][b->handle] = 1;
  auto connect = [&](const Block& b) {
    if (connected[b.kind][b.handle]) return;
    connected[b.kind][b.handle] = 1;
    PriorBlockHost pb;
    pb.id = b.id; pb.kind = b.kind; pb.dim = (b.kind == B_SB) ? 9 : 7;
    pb.mdim = b.fixed ? 0 : ((b.kind == B_SB) ? 9 : 6);
    std::memcpy(pb.lin, b.x, sizeof(double) * pb.dim);
    dense.push_back(pb);
  };
  auto addFactorToJob = [&](uint64_t rid) {
    auto it = factors_.find(rid);
    if (it == factors_.end()) return;
    for (int b = 0; b < it->second.nblk; ++b) connect(blocks_.at(it->second.blocks[b]));
    sel.factors.push_back(it->second);
    removeFactor(rid);
  };
  auto isReproj = [&](uint64_t rid) { return obsRes2Lm_.count(rid); };
  auto isPrior = [&](uint64_t rid) { return rid != 0 && !isReproj(rid) && !factors_.count(rid); };

  for (uint64_t fid : removeAllButPose) {  // :541-605
    auto it = states_.find(fid);
    for (size_t j = 0; j < it->second.sb.size(); ++j) {
      StateInfo& si = it->second.sb[j];
      if (!si.exists) continue;
      if (blocks_.at(si.id).fixed) continue;
      auto checkit = it;
      checkit++;
      if (checkit != states_.end() && checkit->second.sb.size() > j && checkit->second.sb[j].exists &&
          checkit->second.sb[j].id == si.id) continue;
      si.exists = false;
      toMarginalize.push_back(si.id);
      const std::vector<uint64_t> res = blocks_.at(si.id).residuals;
      for (uint64_t rid : res)
        if (!isReproj(rid) && !isPrior(rid)) addFactorToJob(rid);
    }
  }
  bool landmarksDone = false;
  // The job's observation tables come out of the device-resident CSR when it mirrors the graph as it is now (nothing was
  // added or removed since the last solve); otherwise they are assembled from the records the policy removes.
  const bool deviceJob = residentValid_ && residentUsed_ && addLog_.empty() && remLog_.empty() && setLog_.empty() && constLog_.empty() && res_.N == (int)numObs_;
  sel.deviceJob = deviceJob;
  ++pathCounters_[deviceJob ? 2 : 3];
  if (!deviceJob) syncLandmarks();   // the linearisation points of the marginalised landmarks are read from the host graph
  for (uint64_t fid : removeFrames) {  // :607-770
    auto it = states_.find(fid);
    it->second.pose.exists = false;
    toMarginalize.push_back(it->second.pose.id);
    {
      const std::vector<uint64_t> res = blocks_.at(it->second.pose.id).residuals;
      for (uint64_t rid : res) {
        auto fit = factors_.find(rid);
        if (fit != factors_.end() && fit->second.kind == F_POSE_PRIOR) {  // :624-629
          removeFactor(rid);
          sel.reDoFixation = true;
          continue;
        }
        if (!isReproj(rid) && fit != factors_.end()) addFactorToJob(rid);
      }
    }
    for (size_t j = 0; j < it->second.ext.size(); ++j) {  // :638-664
      StateInfo& si = it->second.ext[j];
      if (!si.exists) continue;
      if (blocks_.at(si.id).fixed) continue;
      auto checkit = it;
      checkit++;
      if (checkit != states_.end() && checkit->second.ext[j].exists && checkit->second.ext[j].id == si.id) continue;
      si.exists = false;
      toMarginalize.push_back(si.id);
      const std::vector<uint64_t> res = blocks_.at(si.id).residuals;
      for (uint64_t rid : res)
        if (!isReproj(rid) && factors_.count(rid)) addFactorToJob(rid);
    }
    if (!landmarksDone) {  // :671-766
      // The reference walks every landmark once per leaving frame.  What it does with a landmark depends only on the three
      // frame sets, which are fixed for the whole call, and applying it a second time changes nothing -- so ONE pass, over the
      // landmarks a leaving frame has seen (Block::seenLm) and the ones without observations, in handle order (the order of
      // the device-resident CSR, whose gather kernel picks the same residuals: resident.hpp margObsAction).
      landmarksDone = true;
      const double tl0 = nowSec();
      const size_t obs0 = numObs_;
      const uint64_t currentKfId = allLinearizedFrames.at(0);
      std::vector<unsigned char>& cls = sel.poseClass;
      cls.assign(std::max(nextBlockH_[B_POSE], 1), 0);
      for (uint64_t f : removeFrames) cls[blocks_.at(f).handle] |= kMargRemove;
      for (uint64_t f : allLinearizedFrames) cls[blocks_.at(f).handle] |= kMargLin;
      for (auto st = states_.lower_bound(currentKfId); st != states_.end(); ++st)
        if (const Block* pb = findBlock(st->second.pose.id)) cls[pb->handle] |= kMargNew;
      std::vector<int> cand;
      ++visitStamp_;
      auto consider = [&](int h) {
        Landmark* lp = (h >= 0 && h < (int)lmByHandle_.size()) ? lmByHandle_[h] : nullptr;
        if (!lp || lp->visit == visitStamp_) return;
        lp->visit = visitStamp_;
        cand.push_back(h);
      };
      for (uint64_t f : removeFrames) for (int h : blocks_.at(f).seenLm) consider(h);
      for (int h : emptyLm_) {
        Landmark* lp = (h >= 0 && h < (int)lmByHandle_.size()) ? lmByHandle_[h] : nullptr;
        if (lp && lp->obs.empty()) consider(h);
      }
      emptyLm_.clear();
      std::sort(cand.begin(), cand.end());
      const double tl1 = nowSec();
      for (int h : cand) {
        Landmark& lm = *lmByHandle_[h];
        if (!lm.priors.empty() || (refuseFixedLm && lm.fixed)) continue;   // see margAccepts
        if (lm.obs.empty()) {
          removed.push_back(lm.id);
          eraseLandmark(lm);
          continue;
        }
        bool skipLandmark = true, hasNewObservations = false, marginalize = true, errorTermAdded = false;
        int obsCount = 0;
        for (const Observation& o : lm.obs) {
          const int c = cls[o.poseH];
          if (c & kMargRemove) skipLandmark = false;
          if (c & kMargNew) { marginalize = false; hasNewObservations = true; }
          if (c & kMargLin) obsCount++;
        }
        if (skipLandmark) continue;
        size_t keep = 0;   // the list is compacted once (an erase per removed record moves its tail every time)
        for (size_t i = 0; i < lm.obs.size(); ++i) {
          const Observation& ob = lm.obs[i];
          const int action = margObsAction(cls[ob.poseH], hasNewObservations, marginalize, obsCount);
          if (action == 0) {
            if (keep != i) lm.obs[keep] = ob;
            ++keep;
            continue;
          }
          if (action == 2) {
            errorTermAdded = true;
            connect(*blockByHandle_[B_POSE][ob.poseH]);
            connect(*blockByHandle_[B_EXT][ob.extH]);
            if (sel.lmOrder.empty() || sel.lmOrder.back() != lm.id) {
              sel.lmOrder.push_back(lm.id);
              if (!deviceJob) sel.lmLin[lm.id].assign(lm.hp, lm.hp + 4);
            }
            if (!deviceJob) {
              MargSelection::JobObs jo{ob, lm.id, extIdOf(ob), {0.0, 0.0, 0.0}, lm.fixed};
              if (const ObsInformation* gi = generalInformation(ob)) { jo.S[0] = gi->S[0]; jo.S[1] = gi->S[1]; jo.S[2] = gi->S[2]; }   // (detachObsRecord drops the entry)
              else jo.o.general = 0;
              sel.obs.push_back(jo);
            }
            ++sel.nObs;
          }
          detachObsRecord(lm, ob);
        }
        if (keep != lm.obs.size()) {
          lm.obs.resize(keep);
          afterObsRemoval(lm);
        }
        if (lm.obs.empty() && !errorTermAdded) {   // every residual was dropped: "justDelete"
          removed.push_back(lm.id);
          eraseLandmark(lm);
        } else if (marginalize && errorTermAdded) {
          toMarginalize.push_back(lm.id);
          sel.margLandmarks.push_back(lm.id);
          removed.push_back(lm.id);
          eraseLandmark(lm);
        }
      }
      if (timing)
        std::printf("[marg] landmark pass: %zu candidates collected in %.0f us, handled in %.0f us; %zu observations removed, %zu landmarks erased\n",
                    cand.size(), 1e6 * (tl1 - tl0), 1e6 * (nowSec() - tl1), obs0 - numObs_, removed.size());
    }
    states_.erase(it->second.id);
  }
  std::sort(removed.begin(), removed.end());   // PointMap order (the reference erases while walking its std::map)
  std::sort(sel.margLandmarks.begin(), sel.margLandmarks.end());
  obsCachePose_ = 0;
  std::sort(toMarginalize.begin(), toMarginalize.end());
  toMarginalize.erase(std::unique(toMarginalize.begin(), toMarginalize.end()), toMarginalize.end());
  // ordering of the dense part
  for (PriorBlockHost& pb : dense) { pb.ord = sel.m; sel.m += pb.mdim; }
}

// ---- step 3: the job's tables at the linearisation points, the host-assembled form (observations from sel.obs) or the
// device-gathered one (k_window_marg_gather writes them from the resident CSR), its dimensions and its plan
void Window::margBuildTables(MargSelection& sel, MargJob& job) {
  const bool deviceJob = sel.deviceJob;
  const int Lm = (int)sel.lmOrder.size();
  std::unordered_map<uint64_t, int> sPose, sExt, sSb, sLm;
  for (const PriorBlockHost& pb : sel.dense) {
    const int off = pb.mdim > 0 ? pb.ord : -1;
    if (pb.kind == B_POSE) { sPose[pb.id] = (int)job.oPose.size(); job.hPose.insert(job.hPose.end(), pb.lin, pb.lin + 7); job.oPose.push_back(off); }
    else if (pb.kind == B_EXT) { sExt[pb.id] = (int)job.oExt.size(); job.hExt.insert(job.hExt.end(), pb.lin, pb.lin + 7); job.oExt.push_back(off); }
    else { sSb[pb.id] = (int)job.oSb.size(); job.hSb.insert(job.hSb.end(), pb.lin, pb.lin + 9); job.oSb.push_back(off); }
  }
  job.nSb = (int)job.oSb.size();
  if (job.hExt.empty()) { job.hExt.assign(7, 0.0); job.hExt[6] = 1.0; job.oExt.push_back(-1); }
  if (job.hPose.empty()) { job.hPose.assign(7, 0.0); job.hPose[6] = 1.0; job.oPose.push_back(-1); }
  if (!deviceJob) {
    for (int l = 0; l < Lm; ++l) {
      sLm[sel.lmOrder[l]] = l;
      const std::vector<double>& hp = sel.lmLin.at(sel.lmOrder[l]);
      job.hLm.insert(job.hLm.end(), hp.begin(), hp.end());
    }
    // observations sorted landmark-major (the policy hands them over landmark by landmark already)
    std::stable_sort(sel.obs.begin(), sel.obs.end(),
                     [&](const MargSelection::JobObs& a, const MargSelection::JobObs& b) { return sLm.at(a.lmId) < sLm.at(b.lmId); });
    job.hLmPtr.assign(Lm + 1, 0);
  } else {
    // device job: k_window_marg_gather needs to know the class of every pose handle and where a block sits in the job's tables
    job.poseClass = std::move(sel.poseClass);
    job.jobPoseSlot.assign(std::max(nextBlockH_[B_POSE], 1), -1); job.jobExtSlot.assign(std::max(nextBlockH_[B_EXT], 1), -1);
    for (const auto& kv : sPose) job.jobPoseSlot[blocks_.at(kv.first).handle] = kv.second;
    for (const auto& kv : sExt) job.jobExtSlot[blocks_.at(kv.first).handle] = kv.second;
  }
  // DeviceProblem::obsS of the job (3 N, component-major): only when one of its observations has a general information matrix
  for (const MargSelection::JobObs& jo : sel.obs) job.generalOn = job.generalOn || jo.o.general;
  job.hS.assign(job.generalOn ? 3 * sel.obs.size() : 0, 0.0);
  for (const MargSelection::JobObs& jo : sel.obs) {
    job.hUv.push_back(jo.o.uv[0]); job.hUv.push_back(jo.o.uv[1]);
    const double w = obsWeight(jo.o.size);
    job.hW.push_back(jo.lmFixed ? -w : w);   // (the sign Window::pack() and the resident CSR give a constant landmark's observations)
    if (job.generalOn) {
      const size_t o = job.hW.size() - 1, n = sel.obs.size();
      job.hS[o] = jo.o.general ? jo.S[0] : w; job.hS[n + o] = jo.o.general ? jo.S[1] : 0.0; job.hS[2 * n + o] = jo.o.general ? jo.S[2] : w;
    }
    const int es = sExt.count(jo.extId) ? sExt.at(jo.extId) : 0;
    job.hIdx.push_back(packObs(sPose.at(jo.o.poseId), es, jo.o.cam, jo.o.loss));
    job.hObsLm.push_back(sLm.at(jo.lmId));
    job.hLmPtr[sLm.at(jo.lmId) + 1]++;
  }
  if (!deviceJob) for (int l = 0; l < Lm; ++l) job.hLmPtr[l + 1] += job.hLmPtr[l];
  bool anyExtVar = false;
  for (int o : job.oExt) if (o >= 0) anyExtVar = true;
  for (Factor& f : sel.factors)
    packFactorInto(f, [&](uint64_t id, int& kind, int& slot) {
      if (sPose.count(id)) { kind = B_POSE; slot = sPose.at(id); }
      else if (sExt.count(id)) { kind = B_EXT; slot = sExt.at(id); }
      else { kind = B_SB; slot = sSb.at(id); }
    }, job.hFac, job.hImu, job.hImuT, job.hImuM);
  job.nImu = (int)job.hImu.size();
  // M2 dense part: which rows stay (the new prior) and which are marginalised
  std::vector<int> margIdx;
  for (const PriorBlockHost& pb : sel.dense) {
    const bool marg = std::binary_search(sel.toMarginalize.begin(), sel.toMarginalize.end(), pb.id);
    for (int k = 0; k < pb.mdim; ++k) (marg ? margIdx : job.idxLists).push_back(pb.ord + k);
    if (!marg) sel.kept.push_back(pb);
  }
  const int nk = (int)job.idxLists.size(), nm = (int)margIdx.size();
  job.idxLists.insert(job.idxLists.end(), margIdx.begin(), margIdx.end());
  int ordk = 0;
  for (PriorBlockHost& pb : sel.kept) { pb.ord = ordk; ordk += pb.mdim; }
  job.cams = cameras_;
  job.deviceJob = deviceJob;
  job.lossOn = nLoss_ > 1;   // observations with a loss other than CauchyLoss(1): the job evaluates them through the loss table
  if (job.lossOn) job.lossTab = lossTab_;
  job.keepPre = optOn(kOptMargKeepPre);
  job.margEig = debugOption(kOptMargEig);   // read HERE, on the caller's thread: the job may be issued by the enqueue thread
  job.stream = stream_;
  job.dims = MargDims{sel.m, Lm, sel.nObs, (int)job.hFac.size(), nk, nm, (int)(job.hPose.size() / 7), (int)(job.hExt.size() / 7),
                      (int)cameras_.size(), anyExtVar ? 1 : 0, (sel.hadPrior && priorM_ > 0) ? priorM_ : 0};
  job.plan = planMargJob(job.dims, MargSwitches{job.margEig}, MargKernelSizes{sizeof(JacobiShared)});
  job.lmOrder = std::move(sel.lmOrder);
  job.dense = std::move(sel.dense);
  job.toMarginalize = sel.toMarginalize;
}

// ---- step 4: the persistent job buffers (grow-only: hipMalloc / hipFree per call used to cost more than the algebra) sized from
// the plan, and the job's tables queued for the one pinned block of flushStaged (one DMA, one scatter kernel: 17 pageable copies
// cost ~100 us of enqueueing).  The job is asynchronous: nothing here waits for the device.
void Window::margReserveAndStage(MargJob& job) {
  MargBuffers& mb = margBuf_;
  const MargPlan& q = job.plan;
  mb.bU.reserve(q.bU); mb.bW2.reserve(q.bW2); mb.bV.reserve(q.bV); mb.bVec.reserve(q.bVec);
  // U, W, V and the vectors start from zero: clears riding in the same launch
  job.pending.push_back({nullptr, sizeof(double) * q.clearU, mb.bU.p});
  job.pending.push_back({nullptr, sizeof(double) * q.clearW2, mb.bW2.p});
  job.pending.push_back({nullptr, sizeof(double) * q.clearV, mb.bV.p});
  job.pending.push_back({nullptr, sizeof(double) * q.clearVec, mb.bVec.p});
  job.stage(mb.bPose, job.hPose); job.stage(mb.bExt, job.hExt); job.stage(mb.bSb, job.hSb); job.stage(mb.bLm, job.hLm);
  job.stage(mb.bUv, job.hUv); job.stage(mb.bW, job.hW);
  if (job.generalOn) job.stage(mb.bS, job.hS);
  job.stage(mb.bOP, job.oPose); job.stage(mb.bOE, job.oExt); job.stage(mb.bOS, job.oSb); job.stage(mb.bLmPtr, job.hLmPtr);
  job.stage(mb.bObsLm, job.hObsLm); job.stage(mb.bIdx, job.hIdx);
  job.stage(mb.bFac, job.hFac); job.stage(mb.bImu, job.hImu); job.stage(mb.bImuT, job.hImuT); job.stage(mb.bImuM, job.hImuM);
  job.stage(dCams_, job.cams);
  if (job.lossOn) job.stage(dLossTab_, job.lossTab);
  job.stage(mb.bIdxList, job.idxLists);
  if (job.deviceJob) {
    job.stage(res_.poseClass, job.poseClass); job.stage(res_.poseSlotOfH, job.jobPoseSlot); job.stage(res_.extSlotOfH, job.jobExtSlot);
    mb.bLm.reserve(q.gLm); mb.bUv.reserve(q.gUv); mb.bW.reserve(q.gW);
    mb.bLmPtr.reserve(q.gLmPtr); mb.bObsLm.reserve(q.gObsLm); mb.bIdx.reserve(q.gIdx);
    res_.margScratch.reserve(margGatherScratchInts(res_.L));
  }
  mb.bLin.reserve(q.bLin);
  mb.bFacLin.reserve(q.bFacLin);
  mb.bPartial.reserve(q.bPartial);
  mb.bScal.reserve(q.bScal);
  mb.bFlag.reserve(q.bFlag);
  job.oldPrior = mb.bHk.p;
  if (q.bHk > mb.bHk.cap && job.dims.oldPriorM > 0) { std::swap(job.oldPriorKeep.p, mb.bHk.p); std::swap(job.oldPriorKeep.cap, mb.bHk.cap); }
  mb.bHk.reserve(q.bHk);
  mb.bScratch.reserve(q.bScratch);
  mb.bOut.reserve(q.bOut);
  if (job.dims.nk > 0) priorHostValid_ = false;  // results stay on the device (solver reads Ht / bp / c0 in place); getPrior() fetches
}

// ---- the algebra of the job, M2 and M3, on the system M1 has left in the job buffers: U | ba | W | V | bb in bU / bVec / bW2 / bV,
// the keep | marg lists in bIdxList.  Walks the plan like the rest of step 5.  Its own function because the inspection hook below
// (debugMarginalize) runs it on a system of the caller's: what a test sees there are the job's launches, not a restatement.
static void launchMargAlgebra(const MargBuffers& mb, const MargPlan& pl, const MargDims& d, hipStream_t s) {
  MargDev md;
  md.m = d.m; md.Lm = d.Lm; md.N = d.N; md.F = d.F;
  md.U = mb.bU.p; md.ba = mb.bVec.p + pl.ba.off; md.W = mb.bW2.p; md.V = mb.bV.p; md.bb = mb.bVec.p + pl.bb.off;
  double* vb = mb.bVec.p + pl.vb.off;
  // M2 landmark part
  if (pl.lmPrepare.grid) {
    launch(k_marg_lm_prepare, dim3(pl.lmPrepare.grid), dim3(128), pl.lmPrepare.ldsBytes, s, md, vb);
    launch(k_marg_lm_apply, dim3(pl.lmApply.grid), dim3(256), pl.lmApply.ldsBytes, s, md, (const double*)vb);
    launch(k_marg_lm_update, dim3(pl.lmUpdate.grid), dim3(64), pl.lmUpdate.ldsBytes, s, md);
  }
  // M2 dense part
  if (pl.dense.grid) {
    DenseArgs da;
    da.m = d.m; da.nk = d.nk; da.nm = d.nm;
    da.keep = mb.bIdxList.p; da.marg = mb.bIdxList.p + d.nk;
    da.U = mb.bU.p; da.ba = mb.bVec.p + pl.ba.off;
    da.Hk = mb.bHk.p + pl.Hk.off; da.bk = mb.bHk.p + pl.bk.off;
    da.Vm = mb.bScratch.p + pl.Vm.off; da.Qm = mb.bScratch.p + pl.Qm.off; da.tmp = mb.bScratch.p + pl.denseTmp.off;
    da.flag = mb.bFlag.p;
    launch(k_marg_dense, dim3(pl.dense.grid), dim3(1024), pl.dense.ldsBytes, s, da, pl.denseUseLds, pl.denseProdLds, pl.denseTileChol);
  } else if (pl.copyPair) {
    HIP_OK(hipMemcpyAsync(mb.bHk.p + pl.Hk.off, mb.bU.p, sizeof(double) * pl.Hk.len, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(mb.bHk.p + pl.bk.off, mb.bVec.p + pl.ba.off, sizeof(double) * pl.bk.len, hipMemcpyDeviceToDevice, s));
  }
  // M3 (which eigen-solvers run, and k_marg_final's mode: planMargJob)
  if (pl.final.grid) {
    FinalArgs fa;
    fa.n = d.nk; fa.H = mb.bHk.p + pl.Hk.off; fa.b0 = mb.bHk.p + pl.bk.off;
    fa.G = mb.bOut.p + pl.G.off; fa.Q = mb.bOut.p + pl.Q.off; fa.J = mb.bOut.p + pl.J.off; fa.Ht = mb.bOut.p + pl.Ht.off;
    fa.e0 = mb.bOut.p + pl.e0.off; fa.bp = mb.bOut.p + pl.bp.off; fa.scal = mb.bOut.p + pl.scal.off;
    fa.tmp = mb.bOut.p + pl.finalTmp.off;
    fa.flag = mb.bFlag.p;
    if (pl.finalChol.grid) launch(k_marg_final_chol, dim3(pl.finalChol.grid), dim3(1024), pl.finalChol.ldsBytes, s, fa);
    if (pl.finalDc.grid) launch(k_marg_final_dc, dim3(pl.finalDc.grid), dim3(1024), pl.finalDc.ldsBytes, s, fa, pl.finalDcAfterChol);
    launch(k_marg_final, dim3(pl.final.grid), dim3(1024), pl.final.ldsBytes, s, fa, pl.finalMode, pl.finalFallbackLds, pl.finalSkipIfDone);
  }
}

// ---- step 5: M1-M3, next to their kernels.  Everything the launches need was fixed by steps 3 and 4: no allocation and no host
// table is touched here, so the launches themselves (a DMA, the scatter and 6-13 kernels: 25-50 us of API calls) can be issued by
// the handle's enqueue thread while the call goes on with the graph update and returns (Window::quiesce joins it before the stream,
// the job buffers or the prior are touched again).  It walks the plan: no size or offset is formed here.
void Window::launchMarginalization(const MargJob& job) {
  MargBuffers& mb = margBuf_;
  const MargPlan& pl = job.plan;
  const MargDims& d = job.dims;
  hipStream_t s = job.stream;
  flushStaged(job.pending, s);
  if (job.deviceJob && (d.N > 0 || d.Lm > 0)) {
    MargGatherArgs ga;
    std::memset(&ga, 0, sizeof(ga));
    ga.L = res_.L; ga.H = res_.H; ga.expectN = d.N; ga.expectLm = d.Lm;
    ga.lmPtr = res_.lmPtr[res_.cur].p; ga.handleOfSlot = res_.handleOfSlot[res_.cur].p;
    ga.uv = res_.uv[res_.cur].p; ga.w = res_.w[res_.cur].p; ga.hnd = res_.hnd[res_.cur].p;
    ga.lmHp = res_.lmHp.p;
    ga.poseClass = res_.poseClass.p; ga.jobPoseSlot = res_.poseSlotOfH.p; ga.jobExtSlot = res_.extSlotOfH.p;
    ga.jLmPtr = mb.bLmPtr.p; ga.jObsLm = mb.bObsLm.p; ga.jIdx = mb.bIdx.p; ga.jUv = mb.bUv.p; ga.jW = mb.bW.p; ga.jLm = mb.bLm.p;
    ga.scratch = res_.margScratch.p;
    ga.status = resStatusDev_;
    launchWindowMargGather(ga, s);
  }
  // (the four clears rode in the scatter launch of the staged block) the two copies of the old prior land inside the cleared U / ba:
  // its content (H_, b0_) occupies the leading block and is still on the device, exactly where k_marg_dense left it
  if (d.oldPriorM > 0) {
    FillJobs copies;
    copies.n = 0;
    addFill(copies, mb.bU.p, job.oldPrior + pl.oldH.off, pl.oldH.len, d.oldPriorM, d.m, d.oldPriorM);
    addFill(copies, mb.bVec.p + pl.ba.off, job.oldPrior + pl.oldB0.off, pl.oldB0.len);
    launchFillJobs(copies, s);
  }
  DeviceProblem q;
  std::memset(&q, 0, sizeof(q));
  q.nPose = d.nPose; q.nExt = d.nExt; q.nSb = job.nSb;
  q.L = d.Lm; q.N = d.N; q.F = d.F; q.nImu = job.nImu; q.d = d.m; q.dC = 0; q.nCam = d.nCam;
  q.anyExtVariable = d.anyExtVar;
  q.ownsCamera = 1;
  q.pose = mb.bPose.p; q.ext = mb.bExt.p; q.sb = mb.bSb.p; q.lm = mb.bLm.p;
  q.poseC = mb.bPose.p; q.extC = mb.bExt.p; q.sbC = mb.bSb.p; q.lmC = mb.bLm.p;
  q.poseOff = mb.bOP.p; q.extOff = mb.bOE.p; q.sbOff = mb.bOS.p;
  q.cams = dCams_.p;
  q.lossTab = job.lossOn ? dLossTab_.p : nullptr;
  q.obsS = job.generalOn ? mb.bS.p : nullptr;
  q.lmPtr = mb.bLmPtr.p; q.obsUv = mb.bUv.p; q.obsW = mb.bW.p; q.obsIdx = mb.bIdx.p; q.obsLm = mb.bObsLm.p;
  q.rCur = mb.bLin.p + pl.linR.off; q.JpCur = mb.bLin.p + pl.linJp.off; q.JlCur = mb.bLin.p + pl.linJl.off; q.JeCur = mb.bLin.p + pl.linJe.off;
  q.factors = mb.bFac.p; q.linCur = mb.bFacLin.p; q.linCand = mb.bFacLin.p;
  q.imus = mb.bImu.p; q.imuT = mb.bImuT.p; q.imuMeas = mb.bImuM.p;
  q.scal = mb.bScal.p; q.partial = mb.bPartial.p;
  MargDev md;
  md.m = d.m; md.Lm = d.Lm; md.N = d.N; md.F = d.F;
  md.U = mb.bU.p; md.ba = mb.bVec.p + pl.ba.off; md.W = mb.bW2.p; md.V = mb.bV.p; md.bb = mb.bVec.p + pl.bb.off;
  double* vb = mb.bVec.p + pl.vb.off;
  // M1: evaluate at the linearisation points (each residual's loss corrector as in :283-330) and accumulate
  if (pl.reproj) {
    launchEvalReproj(q, false, true, s);
    const dim3 camGrid(pl.accumCamX, pl.accumCamY);
    if (d.anyExtVar) {
      launch(k_marg_accum_lm<true>, dim3(pl.accumLm.grid), dim3(64), pl.accumLm.ldsBytes, s, q, md);
      launch(k_marg_accum_cam<true>, camGrid, dim3(64), 0, s, q, md);
    } else {
      launch(k_marg_accum_lm<false>, dim3(pl.accumLm.grid), dim3(64), pl.accumLm.ldsBytes, s, q, md);
      launch(k_marg_accum_cam<false>, camGrid, dim3(64), 0, s, q, md);
    }
  }
  if (pl.factors) {
    launchEvalFactors(q, PassArgs{}, false, s);
    launch(k_marg_accum_factors, dim3(pl.accumFactors.grid), dim3(256), pl.accumFactors.ldsBytes, s, q, md);
  }
  if (job.keepPre) {   // inspection: the system after M1 (svin_ba_get_marg_pre), before anything is eliminated
    const int m = d.m, Lm = d.Lm;
    HIP_OK(hipStreamSynchronize(s));
    margPre_.m = m; margPre_.Lm = Lm;
    margPre_.U.assign((size_t)m * m, 0.0); margPre_.ba.assign(std::max(m, 1), 0.0);
    margPre_.W.assign((size_t)m * 3 * Lm, 0.0); margPre_.V.assign((size_t)9 * Lm, 0.0); margPre_.bb.assign((size_t)3 * Lm, 0.0);
    if (m > 0) {
      HIP_OK(hipMemcpy(margPre_.U.data(), md.U, sizeof(double) * m * m, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(margPre_.ba.data(), md.ba, sizeof(double) * m, hipMemcpyDeviceToHost));
    }
    if (Lm > 0) {
      if (m > 0) HIP_OK(hipMemcpy(margPre_.W.data(), md.W, sizeof(double) * m * 3 * Lm, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(margPre_.V.data(), md.V, sizeof(double) * 9 * Lm, hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(margPre_.bb.data(), md.bb, sizeof(double) * 3 * Lm, hipMemcpyDeviceToHost));
    }
    margPre_.margRows.clear();
    margPre_.denseIds.clear(); margPre_.denseOrd.clear(); margPre_.denseMdim.clear();
    margPre_.lmIds.assign(job.lmOrder.begin(), job.lmOrder.end());
    for (const PriorBlockHost& pb : job.dense) { margPre_.denseIds.push_back(pb.id); margPre_.denseOrd.push_back(pb.ord); margPre_.denseMdim.push_back(pb.mdim); }
    for (const PriorBlockHost& pb : job.dense) {
      const bool mg = std::binary_search(job.toMarginalize.begin(), job.toMarginalize.end(), pb.id);
      for (int k = 0; k < pb.mdim; ++k) margPre_.margRows.push_back(mg ? 1 : 0);
    }
  }
  launchMargAlgebra(mb, pl, d, s);
}

// SVIN_MARG_TIMING: what the device reports of the job it has just run (the launches were issued inline)
void Window::margPrintDeviceTiming(const MargJob& job) {
  const MargBuffers& mb = margBuf_;
  HIP_OK(hipStreamSynchronize(job.stream));
  int fl[4] = {0, 0, 0, 0};
  HIP_OK(hipMemcpy(fl, mb.bFlag.p, sizeof(fl), hipMemcpyDeviceToHost));
  double sc3[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const double* dbgScal = job.plan.final.grid ? mb.bOut.p + job.plan.scal.off : nullptr;   // FinalArgs::scal
  if (dbgScal) HIP_OK(hipMemcpy(sc3, dbgScal, sizeof(sc3), hipMemcpyDeviceToHost));
  std::printf("[marg] m %d Lm %d; Jacobi sweeps of the last eigen-solve: %d; eigenvalues <= tol: %d (min %.3e max %.3e)\n", job.dims.m, job.dims.Lm,
              fl[1], fl[2], sc3[1], sc3[2]);
  if (dbgScal && sc3[7] > 0 && fl[3] != -8) {   // the eigenvalues sit behind p[] in the kernel's scratch (flag[3] == -8: the certified
                                                // Cholesky route produced the prior -- tmp + n holds b0 / p there, no eigenvalues exist)
    const int nn = (int)sc3[7];
    std::vector<double> evh(nn);
    HIP_OK(hipMemcpy(evh.data(), dbgScal + 8 + nn, sizeof(double) * nn, hipMemcpyDeviceToHost));
    std::sort(evh.begin(), evh.end());
    std::printf("[marg] smallest eigenvalues:");
    for (int i = 0; i < std::min(nn, 8); ++i) std::printf(" %.3e", evh[i]);
    std::printf("  (tol %.3e)\n", 2.220446049250313e-16 * nn * sc3[2]);
  }
  std::printf("[marg] k_marg_final: n %d, prepare %.0f us, eigen-solve %.0f us (two-phase: phase 1 %d us; %.0f shader clocks per us), "
              "J / e0 / J^T J %.0f us\n", (int)sc3[7], sc3[3] / 100.0, sc3[4] / 100.0, fl[3], sc3[6] / std::max(1.0, sc3[4] / 100.0),
              sc3[5] / 100.0);
}

// ---- step 6: graph update (:710-716, :788-811) -- the marginalised blocks leave, the prior's bookkeeping, the re-done fixation
void Window::margUpdateGraph(const MargSelection& sel) {
  for (uint64_t id : sel.toMarginalize)
    if (!std::binary_search(sel.margLandmarks.begin(), sel.margLandmarks.end(), id)) removeBlock(id);
  int nk = 0;
  for (const PriorBlockHost& pb : sel.kept) nk += pb.mdim;
  if (nk > 0) {
    hasPrior_ = true;
    priorBlocks_ = sel.kept;
    priorM_ = nk;
    priorResId_ = nextResId_++;
    for (const PriorBlockHost& pb : priorBlocks_) blocks_.at(pb.id).residuals.push_back(priorResId_);
  } else {
    hasPrior_ = false;
    priorBlocks_.clear();
    priorM_ = 0;
  }
  if (sel.reDoFixation && !states_.empty()) {
    const uint64_t firstId = states_.begin()->first;
    Factor f;
    f.kind = F_POSE_PRIOR; f.nblk = 1; f.blocks[0] = firstId; f.m = 6;
    std::memcpy(f.meas, blocks_.at(firstId).x, 7 * sizeof(double));
    // information 1e14 on the position and the yaw; Eigen LLT early-exit semantics
    for (int i = 0; i < 36; ++i) f.sqrtInfo[i] = 0;
    f.sqrtInfo[0] = f.sqrtInfo[7] = f.sqrtInfo[14] = std::sqrt(1.0e14);
    f.sqrtInfo[35] = 1.0e14;
    addFactor(std::move(f));
  }
}

int Window::applyMarginalizationStrategy(size_t numKeyframes, size_t numImuFrames, std::vector<uint64_t>& removed) {
  quiesce();
  const bool timing = optOn(kOptMargTiming);
  const double tm0 = nowSec();
  double tm1 = tm0, tm2 = tm0, tm3 = tm0, tm4 = tm0;
  const MargFrames frames = margFrames(numKeyframes, numImuFrames);
  if (!frames.enough) return 1;
  if (!margAccepts(frames)) return -1;
  MargSelection sel;
  margApplyPolicy(frames, sel, removed, timing);
  tm1 = nowSec();
  if (sel.m > 0 || !sel.lmOrder.empty()) {   // the device job (M1-M3)
    auto job = std::make_shared<MargJob>();
    margBuildTables(sel, *job);
    tm2 = nowSec();
    margReserveAndStage(*job);
    // SVIN_MARG_SYNC_ENQUEUE is the A/B switch that issues the launches from this thread; the timing and inspection paths read
    // what the job leaves
    if (timing || job->keepPre || optOn(kOptMargSyncEnqueue)) launchMarginalization(*job);
    else enqueueAsync([this, job]() { launchMarginalization(*job); });
    tm3 = nowSec();
    if (timing) margPrintDeviceTiming(*job);
  }
  tm4 = nowSec();
  margUpdateGraph(sel);
  if (timing)
    std::printf("[marg] policy %.0f us, job assembly %.0f us, upload+enqueue %.0f us, device wait %.0f us, graph update %.0f us\n",
                1e6 * (tm1 - tm0), 1e6 * (tm2 - tm1), 1e6 * (tm3 - tm2), 1e6 * (tm4 - tm3), 1e6 * (nowSec() - tm4));
  return 1;
}

// inspection hook (svin_ba_debug_marginalize): launchMargAlgebra on a caller-supplied system after M1.  No window: the current
// device, the default stream, buffers of its own reserved by the plan's sizes like Window::margReserveAndStage does.  The plan is
// the one a job of these dimensions walks (planMargJob, the same SVIN_MARG_EIG option, sizeof(JacobiShared)); a stage the mask
// leaves out is taken out of the plan (its grid set to 0), nothing else is changed.  What the launches do not write is NaN
// beforehand (Hk | bk, the scratch of the dense part, G | Q | J | Ht | e0 | bp | scal | tmp): a window's job buffers are not
// cleared either, so nothing may depend on what they held.  The flag words start from 0, as in a handle's first job.
int debugMarginalize(const DebugMargIn& in, const DebugMargOut& out) {
  const int m = in.m, Lm = in.Lm;
  if (m < 0 || m > 4096 || Lm < 0 || Lm > (1 << 20) || !out.info || !out.flags) return -1 /* SVIN_ERR_INVALID_ARG */;
  if (in.stages < 1 || in.stages > 7 || ((in.stages & 4) && !(in.stages & 2))) return -1 /* SVIN_ERR_INVALID_ARG */;   // (M3 reads what the dense part leaves)
  if (m > 0 && (!in.margRows || !in.U || !in.ba || !out.U || !out.ba)) return -1 /* SVIN_ERR_INVALID_ARG */;
  if (Lm > 0 && (!in.V || !in.bb || (m > 0 && !in.W))) return -1 /* SVIN_ERR_INVALID_ARG */;
  std::vector<int> idxLists, margIdx;   // keep | marg, both ascending (margBuildTables' idxLists)
  for (int i = 0; i < m; ++i) {
    if (in.margRows[i] != 0 && in.margRows[i] != 1) return -1 /* SVIN_ERR_INVALID_ARG */;
    (in.margRows[i] ? margIdx : idxLists).push_back(i);
  }
  const int nk = (int)idxLists.size(), nm = (int)margIdx.size();
  idxLists.insert(idxLists.end(), margIdx.begin(), margIdx.end());
  if (nk > 0 && (in.stages & 2) && (!out.Hk || !out.bk)) return -1 /* SVIN_ERR_INVALID_ARG */;
  if (nk > 0 && (in.stages & 4) && (!out.J || !out.e0 || !out.Ht || !out.bp || !out.scal)) return -1 /* SVIN_ERR_INVALID_ARG */;
  const MargDims d{m, Lm, 0, 0, nk, nm, 0, 0, 0, 0, 0};
  MargPlan pl = planMargJob(d, MargSwitches{debugOption(kOptMargEig)}, MargKernelSizes{sizeof(JacobiShared)});
  if (!(in.stages & 1)) pl.lmPrepare.grid = pl.lmApply.grid = pl.lmUpdate.grid = 0;
  if (!(in.stages & 2)) { pl.dense.grid = 0; pl.copyPair = false; }
  if (!(in.stages & 4)) pl.finalChol.grid = pl.finalDc.grid = pl.final.grid = 0;
  int32_t* info = out.info;
  info[0] = nk; info[1] = nm; info[2] = pl.lmPrepare.grid; info[3] = pl.lmApply.grid; info[4] = pl.lmUpdate.grid;
  info[5] = pl.dense.grid; info[6] = pl.denseUseLds; info[7] = pl.denseProdLds; info[8] = pl.denseTileChol; info[9] = pl.copyPair ? 1 : 0;
  info[10] = pl.finalChol.grid; info[11] = pl.finalDc.grid; info[12] = pl.final.grid;
  info[13] = pl.finalMode; info[14] = pl.finalFallbackLds; info[15] = pl.finalSkipIfDone;
  MargBuffers mb;
  mb.bU.reserve(pl.bU); mb.bW2.reserve(pl.bW2); mb.bV.reserve(pl.bV); mb.bVec.reserve(pl.bVec);
  mb.bIdxList.reserve(std::max<size_t>(idxLists.size(), 1));
  mb.bFlag.reserve(pl.bFlag); mb.bHk.reserve(pl.bHk); mb.bScratch.reserve(pl.bScratch); mb.bOut.reserve(pl.bOut);
  HIP_OK(hipMemset(mb.bU.p, 0, sizeof(double) * pl.bU)); HIP_OK(hipMemset(mb.bW2.p, 0, sizeof(double) * pl.bW2));
  HIP_OK(hipMemset(mb.bV.p, 0, sizeof(double) * pl.bV)); HIP_OK(hipMemset(mb.bVec.p, 0, sizeof(double) * pl.bVec));
  HIP_OK(hipMemset(mb.bFlag.p, 0, sizeof(int) * pl.bFlag));
  HIP_OK(hipMemset(mb.bHk.p, 0xff, sizeof(double) * pl.bHk));
  if (pl.bScratch) HIP_OK(hipMemset(mb.bScratch.p, 0xff, sizeof(double) * pl.bScratch));
  if (pl.bOut) HIP_OK(hipMemset(mb.bOut.p, 0xff, sizeof(double) * pl.bOut));
  const size_t L3 = (size_t)3 * Lm;
  if (m > 0) {
    HIP_OK(hipMemcpy(mb.bU.p, in.U, sizeof(double) * m * m, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(mb.bVec.p + pl.ba.off, in.ba, sizeof(double) * m, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(mb.bIdxList.p, idxLists.data(), sizeof(int) * m, hipMemcpyHostToDevice));
  }
  if (Lm > 0) {
    if (m > 0) HIP_OK(hipMemcpy(mb.bW2.p, in.W, sizeof(double) * m * L3, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(mb.bV.p, in.V, sizeof(double) * 9 * Lm, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(mb.bVec.p + pl.bb.off, in.bb, sizeof(double) * L3, hipMemcpyHostToDevice));
  }
  launchMargAlgebra(mb, pl, d, 0);
  HIP_OK(hipStreamSynchronize(0));
  HIP_OK(hipMemcpy(out.flags, mb.bFlag.p, sizeof(int) * 8, hipMemcpyDeviceToHost));
  if (m > 0) {
    HIP_OK(hipMemcpy(out.U, mb.bU.p, sizeof(double) * m * m, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out.ba, mb.bVec.p + pl.ba.off, sizeof(double) * m, hipMemcpyDeviceToHost));
  }
  if (nk > 0 && (in.stages & 2)) {
    HIP_OK(hipMemcpy(out.Hk, mb.bHk.p + pl.Hk.off, sizeof(double) * nk * nk, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out.bk, mb.bHk.p + pl.bk.off, sizeof(double) * nk, hipMemcpyDeviceToHost));
  }
  if (nk > 0 && (in.stages & 4)) {
    const size_t n2 = (size_t)nk * nk;
    HIP_OK(hipMemcpy(out.J, mb.bOut.p + pl.J.off, sizeof(double) * n2, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out.Ht, mb.bOut.p + pl.Ht.off, sizeof(double) * n2, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out.e0, mb.bOut.p + pl.e0.off, sizeof(double) * nk, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out.bp, mb.bOut.p + pl.bp.off, sizeof(double) * nk, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out.scal, mb.bOut.p + pl.scal.off, sizeof(double) * 3, hipMemcpyDeviceToHost));
  }
  return 1;
}

}  // namespace svin
