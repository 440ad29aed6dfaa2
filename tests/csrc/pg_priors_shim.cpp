// C entry points over svin_amd/csrc/pg_priors.hpp for tests/test_pg_priors_host.py (compiled with g++ -Wall -Wextra -Werror)
#include "../../svin_amd/csrc/pg_priors.hpp"

extern "C" {
int pgp_kind_valid(int kind) { return svin::pgPriorKindValid(kind) ? 1 : 0; }
int pgp_rows(int kind, int D) { return svin::pgPriorRows(kind, D); }
int pgp_first_row(int kind) { return svin::pgPriorFirstRow(kind); }
int pgp_measurement_finite(int kind, int six, const double* t, const double* q, double yaw) {
  return svin::pgPriorMeasurementFinite(kind, six != 0, t, q, yaw) ? 1 : 0;
}
// status; the packed factor (D (D + 1) / 2) and its full form (D x D row-major, zeros below the diagonal) are written on
// PG_INFO_OK only; info may be NULL
int pgp_factor(int kind, int D, const double* info, double* S_packed, double* S_full) {
  double S[21];
  const int st = svin::pgPriorFactor(kind, D, info, S);
  if (st == svin::PG_INFO_OK) {
    for (int i = 0; i < svin::pgEdgeFactorSize(D); ++i) S_packed[i] = S[i];
    svin::pgEdgeFactorFull(S, D, S_full);
  }
  return st;
}
// m x m information a packed embedded factor stands for
void pgp_gram(int kind, int D, const double* S_packed, double* info) { svin::pgPriorFactorGram(kind, D, S_packed, info); }
}
