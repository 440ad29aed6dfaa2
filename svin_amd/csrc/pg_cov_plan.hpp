// svin_amd: host planning of the pose graph's marginal-covariance pass (posegraph.hip, PoseGraph::covarianceBlocks) -- which
// keyframe of a requested pair is solved as a column, how the column keyframes are dealt to batches, which pieces a batch
// touches on the way down (forward substitution) and on the way up (back substitution), and the LDS of the piece kernels against
// the 160 KiB a workgroup has.  HIP-free (tests/test_pg_cov_plan_host.py runs it on the CPU through
// tests/csrc/pg_cov_plan_shim.cpp); the launcher walks the plan.
//
// The pass.  Sigma = S A^-1 S, A = S J^T J S the undamped Jacobi-scaled normal equations in the nested factorisation of one
// svin_pg_optimize iteration (pieces, level-2 pieces, dense root).  A column keyframe contributes its D unit vectors as right-hand
// sides; kPgCovBatch column keyframes share one pass through the elimination tree:
//   k_pg_cov_units     the ones of the batch's unit vectors (interior rows in tangent order, separator rows in the separator system)
//   k_pg_cov_forward   one workgroup per piece that holds a column keyframe: the band factor in LDS, one column per thread, w = L^-1 e
//                      from the column keyframe's row on (level 2: every level-2 piece, from row 0 -- its right-hand sides come
//                      from level 1)
//   k_pg_cov_sep       separator right-hand sides -= Y_C^T w, one thread per (separator unknown, column), the touching pieces in
//                      the host's fixed order
//   k_pg_cov_root      both substitutions against the root's blocked factor (solve_plan.hpp: bigM, diagF, dinvG), 16 rows a step
//   k_pg_cov_back      one workgroup per piece that holds a row keyframe (level 2: every piece): z = w - Y_C x_S, x = L^-T z
//   k_pg_cov_write     the requested blocks, unscaled by S on both sides
// Every dependency is a launch boundary; no sum depends on the batch a column rides in.
//
// Which keyframe is the column.  A column of A^-1 comes out of two substitutions, so (A^-1)_ab read off column b and (A^-1)_ba read
// off column a differ in the last bits.  For Sigma[b, a] = Sigma[a, b]^T to hold bit for bit, whichever call asks, the column
// keyframe of a pair is a function of the unordered pair: the keyframe LATER in the range.  The block is written transposed when
// that is index_a, and a diagonal block takes its upper triangle from its lower one.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace svin {

constexpr int kPgCovBatch = 8;            // B: column keyframes per pass (32 / 48 right-hand sides)
constexpr int kPgCovThreads = 256;        // every kernel of the pass
constexpr size_t kPgCovMaxLdsBytes = 160 * 1024;
// A pivot below this fraction of its diagonal entry of the scaled normal equations (or not positive) is rank deficiency to working
// precision -- the rule svin_ba_get_covariance states (cov_plan.hpp: kCovPivotTol)
constexpr double kPgCovPivotTol = 1e-12;

// LDS of k_pg_cov_forward / k_pg_cov_back (bytes): the piece's band factor, maxRows x (BW + 1), and a ring of the last BW + 1
// values of every column, (BW + 1) x ldx (ldx = kPgCovBatch * D)
constexpr size_t pgCovPieceLdsBytes(int maxRows, int BW, int ldx) { return ((size_t)maxRows + ldx) * (BW + 1) * 8; }
constexpr bool pgCovPieceFits(int maxRows, int BW, int ldx) { return pgCovPieceLdsBytes(maxRows, BW, ldx) <= kPgCovMaxLdsBytes; }
// k_pg_cov_root works on 16 rows x NC columns a step
constexpr int kPgCovRootTile = 16;

struct PgCovPair {       // one requested block as the pass computes it
  int pair;              // position in the request
  int rowNode, colNode;  // local keyframes; colNode is the later one, -1: a constant keyframe takes part (zero block)
  int transposed;        // the request's index_a is the column keyframe
};
struct PgCovBatchPair { int pair, rowNode, slot, transposed; };
struct PgCovBatch {
  std::vector<int> slotNode;            // column slot -> local keyframe (<= kPgCovBatch)
  std::vector<PgCovBatchPair> pairs;    // the blocks this batch writes
  std::vector<int> fwdPieces;           // level-1 pieces that hold a column keyframe, ascending
  std::vector<int> active;              // per level-1 piece: 1 = in fwdPieces
  std::vector<int> backPieces;          // level-1 pieces that hold a row keyframe, ascending
};
struct PgCovPlan {
  std::vector<int> zeroPairs;           // requests with a constant keyframe
  std::vector<int> columns;             // distinct column keyframes, ascending
  std::vector<PgCovBatch> batches;      // ceil(columns / kPgCovBatch)
};

// off[k] < 0: constant keyframe
inline PgCovPair pgCovCanonical(int pair, int localA, int localB, const int* off) {
  if (off[localA] < 0 || off[localB] < 0) return PgCovPair{pair, localA, -1, 0};
  return localA > localB ? PgCovPair{pair, localB, localA, 1} : PgCovPair{pair, localA, localB, 0};
}

// nodePiece[k]: level-1 piece of an interior keyframe, -1 for a separator or a constant keyframe
inline PgCovPlan planPgCovariance(int nPairs, const int* localA, const int* localB, const int* off, const int* nodePiece, int nPieces) {
  PgCovPlan P;
  std::vector<PgCovPair> cp;
  for (int i = 0; i < nPairs; ++i) {
    const PgCovPair c = pgCovCanonical(i, localA[i], localB[i], off);
    if (c.colNode < 0) P.zeroPairs.push_back(i);
    else { cp.push_back(c); P.columns.push_back(c.colNode); }
  }
  std::sort(P.columns.begin(), P.columns.end());
  P.columns.erase(std::unique(P.columns.begin(), P.columns.end()), P.columns.end());
  const int nb = ((int)P.columns.size() + kPgCovBatch - 1) / kPgCovBatch;
  P.batches.resize(nb);
  for (int b = 0; b < nb; ++b) {
    PgCovBatch& B = P.batches[b];
    const int c0 = b * kPgCovBatch, c1 = std::min<int>(c0 + kPgCovBatch, (int)P.columns.size());
    B.slotNode.assign(P.columns.begin() + c0, P.columns.begin() + c1);
    B.active.assign(nPieces > 0 ? nPieces : 1, 0);
    for (int k : B.slotNode)
      if (nodePiece[k] >= 0) B.active[nodePiece[k]] = 1;
    std::vector<int> back;
    for (const PgCovPair& c : cp) {
      const auto it = std::lower_bound(B.slotNode.begin(), B.slotNode.end(), c.colNode);
      if (it == B.slotNode.end() || *it != c.colNode) continue;
      B.pairs.push_back(PgCovBatchPair{c.pair, c.rowNode, (int)(it - B.slotNode.begin()), c.transposed});
      if (nodePiece[c.rowNode] >= 0) back.push_back(nodePiece[c.rowNode]);
    }
    std::sort(back.begin(), back.end());
    back.erase(std::unique(back.begin(), back.end()), back.end());
    B.backPieces = back;
    for (int pi = 0; pi < nPieces; ++pi)
      if (B.active[pi]) B.fwdPieces.push_back(pi);
  }
  return P;
}

}  // namespace svin
