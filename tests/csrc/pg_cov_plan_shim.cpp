// C entry points over svin_amd/csrc/pg_cov_plan.hpp (the host planning of the pose graph's covariance pass) for
// tests/test_pg_cov_plan_host.py.  A plan is handed over as a flat list of 64-bit integers:
//   nZero, zero pairs..., nColumns, columns..., nBatches, then per batch
//   nSlots, slots..., nPairs, (pair, rowNode, slot, transposed)..., nFwd, fwd..., nActive, active..., nBack, back...
#include <cstdint>
#include "../../svin_amd/csrc/pg_cov_plan.hpp"

extern "C" {
// kPgCovBatch, kPgCovThreads, kPgCovMaxLdsBytes, kPgCovRootTile
int64_t pgcp_constant(int which) {
  const int64_t c[4] = {svin::kPgCovBatch, svin::kPgCovThreads, (int64_t)svin::kPgCovMaxLdsBytes, svin::kPgCovRootTile};
  return c[which];
}
int64_t pgcp_piece_lds(int maxRows, int BW, int ldx) { return (int64_t)svin::pgCovPieceLdsBytes(maxRows, BW, ldx); }
int pgcp_piece_fits(int maxRows, int BW, int ldx) { return svin::pgCovPieceFits(maxRows, BW, ldx) ? 1 : 0; }
// returns the number of integers the plan takes; writes at most cap of them
int64_t pgcp_plan(int nPairs, const int* la, const int* lb, const int* off, const int* nodePiece, int nPieces, int64_t* o, int64_t cap) {
  const svin::PgCovPlan P = svin::planPgCovariance(nPairs, la, lb, off, nodePiece, nPieces);
  int64_t k = 0;
  auto put = [&](int64_t v) { if (k < cap) o[k] = v; ++k; };
  auto list = [&](const std::vector<int>& v) { put((int64_t)v.size()); for (int x : v) put(x); };
  list(P.zeroPairs);
  list(P.columns);
  put((int64_t)P.batches.size());
  for (const svin::PgCovBatch& B : P.batches) {
    list(B.slotNode);
    put((int64_t)B.pairs.size());
    for (const svin::PgCovBatchPair& q : B.pairs) { put(q.pair); put(q.rowNode); put(q.slot); put(q.transposed); }
    list(B.fwdPieces);
    list(B.active);
    list(B.backPieces);
  }
  return k;
}
}
