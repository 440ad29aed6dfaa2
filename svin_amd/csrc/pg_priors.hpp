// svin_amd: host side of the pose graph's absolute keyframe measurements (svin_pg_add_prior, posegraph.hip) -- validation of a
// prior's kind, measurement, information matrix and loss, and the factor the device applies.  HIP-free
// (tests/test_pg_priors_host.py runs it on the CPU through tests/csrc/pg_priors_shim.cpp).
//
// A prior measures m of the D rows of the unit residual u of its keyframe (4-DoF [t_k - t_m, wrap(yaw_k - yaw_m)], 6-DoF
// [t_k - t_m, 2 vec(q_k q_m^-1)]): POSE all D, POSITION rows 0..2, DEPTH row 2.  Its information is m x m in the order of the rows
// it keeps; information = L L^T, r = S u_sel with S = L^T (pgEdgeFactor of pg_edges.hpp on the m x m matrix).
//
// The embedding.  S goes into the packed D x D upper-triangular form of pg_edges.hpp at the rows and columns the prior keeps;
// every other entry is zero: POSITION is blockdiag(S3, 0), DEPTH has S[2][2] alone.  pgApplyFactor then applies a prior's factor
// with the code it has for edges: the rows that are not kept come out as exact zeros (0 * finite), residual and Jacobian alike.
#pragma once
#include "pg_edges.hpp"

namespace svin {

enum PgPriorKind : int { PG_PRIOR_POSE = 0, PG_PRIOR_POSITION = 1, PG_PRIOR_DEPTH = 2 };   // svin_pg.h SVIN_PG_PRIOR_*

inline bool pgPriorKindValid(int kind) { return kind == PG_PRIOR_POSE || kind == PG_PRIOR_POSITION || kind == PG_PRIOR_DEPTH; }
// rows of u a prior keeps: m of them from row `first` on; -1 for an unknown kind
inline int pgPriorRows(int kind, int D) { return kind == PG_PRIOR_POSE ? D : kind == PG_PRIOR_POSITION ? 3 : kind == PG_PRIOR_DEPTH ? 1 : -1; }
inline int pgPriorFirstRow(int kind) { return kind == PG_PRIOR_DEPTH ? 2 : 0; }

// the numbers of the measurement a prior of this kind reads are finite: t (DEPTH: t[2] alone), POSE also q (6-DoF) or yaw (4-DoF)
inline bool pgPriorMeasurementFinite(int kind, bool six, const double* t, const double* q, double yaw) {
  if (kind == PG_PRIOR_DEPTH) return std::isfinite(t[2]);
  bool ok = std::isfinite(t[0]) && std::isfinite(t[1]) && std::isfinite(t[2]);
  if (kind == PG_PRIOR_POSE) {
    if (six) for (int c = 0; c < 4; ++c) ok = ok && std::isfinite(q[c]);
    else ok = ok && std::isfinite(yaw);
  }
  return ok;
}

// information (m x m row-major, m = pgPriorRows; nullptr = identity) -> the packed D x D factor with S = L^T embedded.  Refusals
// are pgEdgeFactor's, on the m x m matrix (D eps becomes m eps in the pivot rule).  S is only written on PG_INFO_OK.
inline int pgPriorFactor(int kind, int D, const double* info, double* S) {
  const int m = pgPriorRows(kind, D), first = pgPriorFirstRow(kind);
  double Sm[21] = {0};
  if (info) {
    const int st = pgEdgeFactor(info, m, Sm);
    if (st != PG_INFO_OK) return st;
  } else {
    for (int k = 0; k < m; ++k) Sm[pgEdgeFactorAt(m, k, k)] = 1.0;
  }
  for (int i = 0; i < pgEdgeFactorSize(D); ++i) S[i] = 0.0;
  for (int k = 0; k < m; ++k)
    for (int j = k; j < m; ++j) S[pgEdgeFactorAt(D, first + k, first + j)] = Sm[pgEdgeFactorAt(m, k, j)];
  return PG_INFO_OK;
}
// the m x m information a packed embedded factor stands for: (S^T S) at the kept rows and columns
inline void pgPriorFactorGram(int kind, int D, const double* S, double* info) {
  const int m = pgPriorRows(kind, D), first = pgPriorFirstRow(kind);
  double full[36];
  pgEdgeFactorGram(S, D, full);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) info[i * m + j] = full[(first + i) * D + first + j];
}

}  // namespace svin
