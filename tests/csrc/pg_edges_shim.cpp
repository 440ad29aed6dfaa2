// C entry points over svin_amd/csrc/pg_edges.hpp for tests/test_pg_edges_host.py (compiled with g++ -Wall -Wextra -Werror)
#include "../../svin_amd/csrc/pg_edges.hpp"

#include <cstdint>

extern "C" {
int64_t pge_constant(int which) {
  switch (which) {
    case 0: return svin::kPgSharedMin;
    case 1: return svin::pgEdgeFactorSize(4);
    case 2: return svin::pgEdgeFactorSize(6);
    default: return -1;
  }
}
// status; S_full (D x D row-major, zeros below the diagonal) is written on PG_INFO_OK only
int pge_factor(const double* info, int D, double* S_full) {
  double S[21];
  const int st = svin::pgEdgeFactor(info, D, S);
  if (st == svin::PG_INFO_OK) svin::pgEdgeFactorFull(S, D, S_full);
  return st;
}
void pge_default(int six, double* S_full, double* info) {
  double S[21];
  svin::pgEdgeDefaultFactor(six != 0, S);
  svin::pgEdgeFactorFull(S, six ? 6 : 4, S_full);
  svin::pgEdgeFactorGram(S, six ? 6 : 4, info);
}
int pge_loss_valid(int kind, double scale) { return svin::pgEdgeLossValid(kind, scale) ? 1 : 0; }
const char* pge_status_text(int st) { return svin::pgInfoStatusText(st); }
// out: groups, then per group lo, hi, count, edges...; returns the int64 needed
int64_t pge_shared(int ne, const int* ea, const int* eb, const int* off, int minCount, int64_t* out, int64_t cap) {
  const svin::PgSharedDst T = svin::pgSharedDestinations(ne, ea, eb, off, minCount);
  int64_t n = 0;
  auto put = [&](int64_t v) { if (out && n < cap) out[n] = v; ++n; };
  put(T.groups());
  for (int g = 0; g < T.groups(); ++g) {
    put(T.lo[g]); put(T.hi[g]); put(T.ptr[g + 1] - T.ptr[g]);
    for (int i = T.ptr[g]; i < T.ptr[g + 1]; ++i) put(T.edge[i]);
  }
  return n;
}
}
