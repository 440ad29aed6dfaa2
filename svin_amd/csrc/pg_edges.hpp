// svin_amd: host side of the pose graph's caller-given edges (svin_pg_add_edge, posegraph.hip) -- validation of an edge's
// information matrix and loss, the factor the device applies, the weights an edge gets without a matrix, and the table of
// destination blocks that three or more edges share.  HIP-free (tests/test_pg_edges_host.py runs it on the CPU through
// tests/csrc/pg_edges_shim.cpp).
//
// The factor.  information = L L^T (Cholesky, L lower triangular); the device applies S = L^T, upper triangular, to the
// unit-weight residual u and its Jacobians: r = S u, |r|^2 = u^T information u -- the convention of
// svin_ba_map_add_reprojection_error.  S is kept packed by rows: row k holds S[k][k .. D - 1], D (D + 1) / 2 doubles (10 / 21).
//
// Shared destination blocks.  The off-diagonal block of a pair of free keyframes is the sum of J_b^T J_a over the edges between
// them.  One or two edges on a pair are added atomically (two adds onto a zeroed block commute exactly); three or more are summed
// by one thread per entry in the order of the edge list and stored once (k_pg_assemble_shared), so the bits do not depend on the
// order the atomics would have landed in.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace svin {

constexpr int kPgSharedMin = 3;   // edges on one pair from which the pair's block is summed in a fixed order
constexpr int pgEdgeFactorSize(int D) { return D * (D + 1) / 2; }
// position of S[k][j], j >= k, in the packed factor
constexpr int pgEdgeFactorAt(int D, int k, int j) { return k * D - k * (k - 1) / 2 + (j - k); }

enum PgInfoStatus : int { PG_INFO_OK = 0, PG_INFO_NOT_FINITE = 1, PG_INFO_NOT_SYMMETRIC = 2, PG_INFO_NOT_POSITIVE_DEFINITE = 3 };
inline const char* pgInfoStatusText(int s) {
  switch (s) {
    case PG_INFO_OK: return "ok";
    case PG_INFO_NOT_FINITE: return "the information matrix is not finite";
    case PG_INFO_NOT_SYMMETRIC: return "the information matrix is not symmetric";
    default: return "the information matrix is not positive definite";
  }
}

// information (D x D row-major) -> packed S = L^T.  Refused: an entry that is not finite, I[i][j] != I[j][i], a pivot that is
// not above D eps times its diagonal entry (an indefinite or semi-definite matrix, to working precision).  S is only written on
// PG_INFO_OK.
inline int pgEdgeFactor(const double* info, int D, double* S) {
  for (int i = 0; i < D * D; ++i)
    if (!std::isfinite(info[i])) return PG_INFO_NOT_FINITE;
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < i; ++j)
      if (info[i * D + j] != info[j * D + i]) return PG_INFO_NOT_SYMMETRIC;
  double L[36] = {0};
  const double tol = D * 2.220446049250313e-16;
  for (int j = 0; j < D; ++j) {
    double d = info[j * D + j];
    for (int m = 0; m < j; ++m) d -= L[j * D + m] * L[j * D + m];
    if (!(d > tol * info[j * D + j])) return PG_INFO_NOT_POSITIVE_DEFINITE;
    const double ljj = std::sqrt(d);
    L[j * D + j] = ljj;
    for (int i = j + 1; i < D; ++i) {
      double v = info[i * D + j];
      for (int m = 0; m < j; ++m) v -= L[i * D + m] * L[j * D + m];
      L[i * D + j] = v / ljj;
    }
  }
  for (int k = 0; k < D; ++k)
    for (int j = k; j < D; ++j) S[pgEdgeFactorAt(D, k, j)] = L[j * D + k];
  return PG_INFO_OK;
}

// the weights of an edge given without a matrix: those of the loop edge of its DoF (FourDOFWeightError: 1, 1, 1 and yaw / 10;
// PoseGraph3dErrorTerm's loop sqrt-information 20, 20, 20, 100, 100, 100)
inline void pgEdgeDefaultFactor(bool six, double* S) {
  const int D = six ? 6 : 4;
  for (int i = 0; i < pgEdgeFactorSize(D); ++i) S[i] = 0.0;
  for (int k = 0; k < D; ++k) S[pgEdgeFactorAt(D, k, k)] = six ? (k < 3 ? 20.0 : 100.0) : (k < 3 ? 1.0 : 0.1);
}
// packed S -> D x D row-major (zeros below the diagonal); S^T S -> D x D row-major
inline void pgEdgeFactorFull(const double* S, int D, double* full) {
  for (int k = 0; k < D; ++k)
    for (int j = 0; j < D; ++j) full[k * D + j] = j >= k ? S[pgEdgeFactorAt(D, k, j)] : 0.0;
}
inline void pgEdgeFactorGram(const double* S, int D, double* info) {
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) {
      double s = 0;
      for (int k = 0; k <= std::min(i, j); ++k) s += S[pgEdgeFactorAt(D, k, i)] * S[pgEdgeFactorAt(D, k, j)];
      info[i * D + j] = s;
    }
}

// loss kinds: the values of svin_ba.h's SVIN_LOSS_NONE / _CAUCHY / _HUBER; the scale finite and > 0 except for NONE
inline bool pgEdgeLossValid(int kind, double scale) {
  if (kind == 0) return true;
  return (kind == 1 || kind == 2) && std::isfinite(scale) && scale > 0.0;
}

// pairs of free keyframes that carry kPgSharedMin or more edges: ptr (groups + 1), the edges of a group in the order of the
// edge list; groups in the order of their first edge.  off[k] < 0: constant keyframe (its edges have no off-diagonal block).
struct PgSharedDst {
  std::vector<int> ptr{0}, edge;
  std::vector<int> lo, hi;   // the group's pair, lo < hi (local keyframes)
  int groups() const { return (int)lo.size(); }
};
inline PgSharedDst pgSharedDestinations(int ne, const int* ea, const int* eb, const int* off, int minCount = kPgSharedMin) {
  struct Item { long long key; int e; };
  std::vector<Item> items;
  for (int e = 0; e < ne; ++e) {
    if (off[ea[e]] < 0 || off[eb[e]] < 0 || ea[e] == eb[e]) continue;
    const int lo = std::min(ea[e], eb[e]), hi = std::max(ea[e], eb[e]);
    items.push_back({((long long)lo << 32) | (unsigned)hi, e});
  }
  std::stable_sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.key < y.key; });
  std::vector<std::pair<int, std::pair<size_t, size_t>>> found;   // first edge, [begin, end) in items
  for (size_t i = 0; i < items.size();) {
    size_t j = i;
    while (j < items.size() && items[j].key == items[i].key) ++j;
    if ((int)(j - i) >= minCount) found.push_back({items[i].e, {i, j}});
    i = j;
  }
  std::sort(found.begin(), found.end());
  PgSharedDst T;
  for (const auto& f : found) {
    for (size_t i = f.second.first; i < f.second.second; ++i) T.edge.push_back(items[i].e);
    T.ptr.push_back((int)T.edge.size());
    T.lo.push_back((int)(items[f.second.first].key >> 32));
    T.hi.push_back((int)(items[f.second.first].key & 0xffffffffLL));
  }
  return T;
}

}  // namespace svin
