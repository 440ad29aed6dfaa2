// svin_amd: Map::getLhs (Map.cpp:105-150) for every parameter block of the window in one device pass.
//
//   H_b = sum over the residual blocks touching b of J_b^T J_b, J_b the minimal Jacobian of EvaluateWithMinimalJacobians at the
//   current values: square-root information in, loss function out (no Cauchy corrector), constant blocks like any other.
//
// Three launches, no floating-point atomics, every sum in a fixed order (bit-identical from call to call):
//   k_lhs_cam        pose / extrinsics blocks from the reprojection observations.  A work item is (camera-side block, range of the
//                    observation table): its four waves scan their quarter of the range, compact the observations of that block
//                    into a wave-private LDS queue (ballot + prefix count: table order) and evaluate 64 of them at a time, one
//                    per lane.  The workgroup's 21 sums of the upper triangle go to partial[item].  Window::computeLhs cuts each
//                    block's range into about one item per 256 of its observations, so a long list (a shared extrinsics block
//                    sees every observation) is spread over many workgroups.
//   k_lhs_landmarks  landmark blocks, 16 lanes per landmark as k_landmark_quality (reprojection rows and the HomogeneousPointError
//                    pseudo-observations; |w| for the observations of constant landmarks).
//   k_lhs_blocks     one workgroup per pose / extrinsics / speed-bias block: its items' partials (strided over the 256 threads,
//                    then a shuffle tree and the waves in order: a shared extrinsics block has ~2 000 items), then its small
//                    factors' records (FactorLin of the current point, written by launchEvalFactors / evaluateHostFactors just
//                    before) in list order, then its diagonal block of the prior's H-space matrix Ht = J^T J.
#include "kernels.hpp"

namespace svin {

namespace {

constexpr int kLhsThreads = 256;
constexpr int kLhsWaves = kLhsThreads / 64;

__device__ __forceinline__ void lhsWaveSync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// index of (a, c), a <= c, in the 21-entry upper triangle of a 6 x 6 matrix (row by row)
__host__ __device__ __forceinline__ int lhsSym6(int a, int c) { return a * 6 - a * (a - 1) / 2 + (c - a); }

// one observation's J^T J (both rows) into the upper triangle `acc`: the pose part (POSE) or the extrinsics part
// GENERAL (here and below): the window holds general 2x2 information matrices (p.obsS set); chosen at launch, so that the
// one-weight kernels keep their registers
template <bool POSE, bool GENERAL>
__device__ __forceinline__ void lhsObservation(const DeviceProblem& p, int o, double (&acc)[21]) {
  const uint32_t idx = p.obsIdx[o];
  const double4 hp = reinterpret_cast<const double4*>(p.lm)[p.obsLm[o]];
  const double hpw[4] = {hp.x, hp.y, hp.z, hp.w};
  const double2 uv = reinterpret_cast<const double2*>(p.obsUv)[o];
  double rr[2], jp[12], jl[6], je[12];
  if (GENERAL)   // general 2x2 information: S = (s00, s01, s11), component-major with stride N
    reprojEval(p.cams[(idx >> 24) & 0xf], p.pose + (size_t)(idx & 0xfff) * 7, hpw, p.ext + (size_t)((idx >> 12) & 0xfff) * 7, uv.x,
               uv.y, p.obsS[o], p.obsS[(size_t)p.N + o], p.obsS[2 * (size_t)p.N + o], rr, jp, jl, je);
  else
    reprojEval(p.cams[(idx >> 24) & 0xf], p.pose + (size_t)(idx & 0xfff) * 7, hpw, p.ext + (size_t)((idx >> 12) & 0xfff) * 7, uv.x,
               uv.y, fabs(p.obsW[o]), rr, jp, jl, je);
  const double* J = POSE ? jp : je;
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = a; c < 6; ++c) acc[k++] += J[a] * J[c] + J[6 + a] * J[6 + c];
}

template <bool POSE, bool GENERAL>
__device__ __forceinline__ void lhsScan(const DeviceProblem& p, uint32_t want, int b0, int b1, int* q, double (&acc)[21]) {
  const int lane = threadIdx.x & 63;
  const int shift = POSE ? 0 : 12;
  int qn = 0;   // queued observations (uniform across the wave)
  for (int base = b0; base < b1; base += 256) {
    uint32_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int o = base + 64 * u + lane;
      v[u] = o < b1 ? p.obsIdx[o] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int o = base + 64 * u + lane;
      // landmark-prior pseudo-observations (camera kPriorCam) name slots (0, 0) but touch no camera-side block
      const bool hit = o < b1 && ((v[u] >> 24) & 0xf) != (uint32_t)kPriorCam && ((v[u] >> shift) & 0xfff) == want;
      const unsigned long long mask = __ballot(hit);
      const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
      if (hit) q[qn + before] = o;
      qn += __popcll(mask);
      if (qn >= 64) {
        lhsWaveSync();
        lhsObservation<POSE, GENERAL>(p, q[lane], acc);
        const int rest = qn - 64;
        const int moved = lane < rest ? q[64 + lane] : 0;
        lhsWaveSync();
        if (lane < rest) q[lane] = moved;
        lhsWaveSync();
        qn = rest;
      }
    }
  }
  lhsWaveSync();
  if (lane < qn) lhsObservation<POSE, GENERAL>(p, q[lane], acc);
}

template <bool GENERAL>
__global__ __launch_bounds__(kLhsThreads) void k_lhs_cam(DeviceProblem p, const LhsItem* __restrict__ items,
                                                         double* __restrict__ partial) {
  __shared__ int queue[kLhsWaves][128];
  __shared__ double red[kLhsWaves][21];
  const LhsItem it = items[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (it.end - it.begin + kLhsWaves - 1) / kLhsWaves;
  const int b0 = it.begin + wave * per, b1 = min(it.end, b0 + per);
  double acc[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) acc[k] = 0.0;
  if (it.key < p.nPose) lhsScan<true, GENERAL>(p, (uint32_t)it.key, b0, b1, queue[wave], acc);
  else lhsScan<false, GENERAL>(p, (uint32_t)(it.key - p.nPose), b0, b1, queue[wave], acc);
  // fixed-order reduction: lanes by a shuffle tree, then the four waves in order
#pragma unroll
  for (int k = 0; k < 21; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 21) {
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kLhsWaves; ++w) s += red[w][threadIdx.x];
    partial[(size_t)blockIdx.x * 21 + threadIdx.x] = s;
  }
}

template <bool GENERAL>
__global__ __launch_bounds__(256) void k_lhs_landmarks(DeviceProblem p, double* __restrict__ out) {
  const int l = blockIdx.x * 16 + (threadIdx.x >> 4), gl = threadIdx.x & 15;
  if (l >= p.L) return;   // whole 16-lane rows leave together
  double a[6] = {0, 0, 0, 0, 0, 0};   // 00 01 02 11 12 22
  const double4 hp = reinterpret_cast<const double4*>(p.lm)[l];
  const double hpw[4] = {hp.x, hp.y, hp.z, hp.w};
  const int oEnd = p.lmPtr[l + 1];
  for (int o = p.lmPtr[l] + gl; o < oEnd; o += 16) {
    const uint32_t idx = p.obsIdx[o];
    double rr[2], jp[12], jl[6], je[12];
    if (((idx >> 24) & 0xf) == kPriorCam) {   // HomogeneousPointError: rows 0-1 (part 0) or row 2 (part 1) of its S
      const double* pr = p.lmPrior + 12 * (int)p.obsUv[2 * (size_t)o];
      const bool second = p.obsUv[2 * (size_t)o + 1] != 0.0;
      for (int k = 0; k < 3; ++k) { jl[k] = pr[3 + (second ? 6 : 0) + k]; jl[3 + k] = second ? 0.0 : pr[6 + k]; }
    } else {
      if (GENERAL)
        reprojEval(p.cams[(idx >> 24) & 0xf], p.pose + (size_t)(idx & 0xfff) * 7, hpw, p.ext + (size_t)((idx >> 12) & 0xfff) * 7,
                   p.obsUv[2 * (size_t)o], p.obsUv[2 * (size_t)o + 1], p.obsS[o], p.obsS[(size_t)p.N + o], p.obsS[2 * (size_t)p.N + o], rr, jp, jl, je);
      else
        reprojEval(p.cams[(idx >> 24) & 0xf], p.pose + (size_t)(idx & 0xfff) * 7, hpw, p.ext + (size_t)((idx >> 12) & 0xfff) * 7,
                   p.obsUv[2 * (size_t)o], p.obsUv[2 * (size_t)o + 1], fabs(p.obsW[o]), rr, jp, jl, je);
    }
    a[0] += jl[0] * jl[0] + jl[3] * jl[3]; a[1] += jl[0] * jl[1] + jl[3] * jl[4]; a[2] += jl[0] * jl[2] + jl[3] * jl[5];
    a[3] += jl[1] * jl[1] + jl[4] * jl[4]; a[4] += jl[1] * jl[2] + jl[4] * jl[5]; a[5] += jl[2] * jl[2] + jl[5] * jl[5];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) a[k] += __shfl_xor(a[k], off, 16);   // (a + b == b + a: every lane ends with the same bits)
  if (gl < 9) {
    const int r = gl / 3, c = gl % 3, lo = r < c ? r : c, hi = r < c ? c : r;
    const int k = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
    out[(size_t)9 * l + gl] = a[k];
  }
}

__global__ __launch_bounds__(kLhsThreads) void k_lhs_blocks(DeviceProblem p, const LhsBlock* __restrict__ blocks, const int2* __restrict__ facs,
                                                            const double* __restrict__ partial, double* __restrict__ out) {
  __shared__ double red[kLhsWaves][21];
  __shared__ double cam[21];
  const LhsBlock b = blocks[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, md = b.md;
  if (md == 6) {   // (uniform) the block's item partials: thread t takes items t, t + 256, ...; lanes by a shuffle tree, waves in order
    double acc[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) acc[k] = 0.0;
    for (int it = b.item0 + t; it < b.item1; it += kLhsThreads)
#pragma unroll
      for (int k = 0; k < 21; ++k) acc[k] += partial[(size_t)it * 21 + k];
#pragma unroll
    for (int k = 0; k < 21; ++k) {
      double v = acc[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (t < 21) {
      double v = red[0][t];
#pragma unroll
      for (int w = 1; w < kLhsWaves; ++w) v += red[w][t];
      cam[t] = v;
    }
    __syncthreads();
  }
  if (t >= md * md) return;
  const int r = t / md, c = t - r * md, i = r < c ? r : c, j = r < c ? c : r;   // (r, c) and (c, r) compute the same bits
  double s = md == 6 ? cam[lhsSym6(i, j)] : 0.0;
  for (int f = b.fac0; f < b.fac1; ++f) {
    const int2 e = facs[f];
    const FactorLin& L = p.linCur[e.x];
    const int m = L.m, nc = L.ncols;
    const double* Ji = L.J + e.y + i;
    const double* Jj = L.J + e.y + j;
    double sf = 0.0;
    for (int q = 0; q < m; ++q) sf += Ji[q * nc] * Jj[q * nc];
    s += sf;
  }
  if (b.priorMd > 0) s += p.priorH[(size_t)(b.priorOrd + i) * p.priorM + b.priorOrd + j];
  out[(size_t)b.out + t] = s;
}

}  // namespace

void launchLhsAll(const DeviceProblem& p, const LhsItem* items, int nItems, const LhsBlock* blocks, int nBlocks, const int2* facs,
                  double* partial, double* out, size_t lmOut, hipStream_t s) {
  if (p.obsS) {
    launch(k_lhs_cam<true>, dim3(nItems), dim3(kLhsThreads), 0, s, p, items, partial);
    launch(k_lhs_landmarks<true>, dim3((p.L + 15) / 16), dim3(256), 0, s, p, out + lmOut);
  } else {
    launch(k_lhs_cam<false>, dim3(nItems), dim3(kLhsThreads), 0, s, p, items, partial);
    launch(k_lhs_landmarks<false>, dim3((p.L + 15) / 16), dim3(256), 0, s, p, out + lmOut);
  }
  launch(k_lhs_blocks, dim3(nBlocks), dim3(kLhsThreads), 0, s, p, blocks, facs, (const double*)partial, out);
}

}  // namespace svin
