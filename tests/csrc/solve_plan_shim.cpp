// C entry points over svin_amd/csrc/solve_plan.hpp (the host planning of the reduced solve) for tests/test_solve_plan_host.py:
// the planner takes plain integers and switches, so the routes, the layout of DeviceProblem::cholL and the size of every launch
// are checked on the CPU.  A plan is handed over as kFields 64-bit integers in the order of FIELDS in tests/helpers/solve_plan_lib.py.
#include <cstdint>
#include <initializer_list>
#include "../../svin_amd/csrc/solve_plan.hpp"

namespace {
constexpr int kFields = 61;
void put(const svin::ReducedSolvePlan& q, int64_t* o) {
  int k = 0;
  for (int v : {q.chainMode, q.chainOverflow ? 1 : 0, (int)q.route, q.dSolve, q.dpad, q.border, q.dp, q.nb, q.n, q.dK, q.ldY, q.rowsY, q.ldOut, q.dpK,
                svin::batchedSolverTakes(q) ? 1 : 0})
    o[k++] = v;
  for (const svin::ScratchRegion& r : {q.factor, q.borderScr, q.bigM, q.dinvG, q.diagF, q.ready, q.compactS, q.compactG, q.Lf, q.Y, q.tvec, q.counter}) {
    o[k++] = (int64_t)r.off;
    o[k++] = (int64_t)r.len;
  }
  o[k++] = (int64_t)q.end;
  for (const svin::PlannedLaunch& l : {q.sbFactor, q.sbForward, q.sbLoad, q.borderPrepare, q.cholLds, q.cholLL, q.bigLoad, q.bigChain, q.sbBack}) {
    o[k++] = l.grid;
    o[k++] = (int64_t)l.ldsBytes;
  }
  o[k++] = q.helperTasks;
  o[k++] = q.nBackPanels;
  o[k++] = (int64_t)q.bigBackLdsBytes;
  static_assert(15 + 24 + 1 + 18 + 3 == kFields, "FIELDS of solve_plan_lib.py");
}
}  // namespace

extern "C" {
int sp_fields() { return kFields; }
// in: rows x {d, dC, sbChain, sPadded, switches (1: SVIN_NO_LL, 2: SVIN_NO_SB_ELIM, 4: SVIN_NO_LDS_BORDER)}; out: rows x kFields
void sp_plan(int rows, const int32_t* in, int64_t* out) {
  for (int r = 0; r < rows; ++r) {
    const int32_t* a = in + (size_t)5 * r;
    put(svin::planReducedSolve(svin::SolveDims{a[0], a[1], a[2], a[3]}, svin::SolveSwitches{(a[4] & 1) != 0, (a[4] & 2) != 0, (a[4] & 4) != 0}),
        out + (size_t)kFields * r);
  }
}
int64_t sp_scratch_doubles(int d, int withChain) { return (int64_t)svin::solveReducedScratchDoubles(d, withChain != 0); }
// out: c0, c1, blocks, nChunks
void sp_back_panel(int dp, int k, int* out) {
  const svin::BackPanel b = svin::backPanel(dp, k);
  out[0] = b.c0; out[1] = b.c1; out[2] = b.blocks; out[3] = b.nChunks;
}
// kNB, kBackSpan, kCholLdsMaxTiles, kBorderMaxRows, kBorderScratchDoubles, kSbRec, kSbFlo, kSbFhi, kSbMaxChain, kSbCols
int sp_constant(int which) {
  const int c[10] = {svin::kNB, svin::kBackSpan, svin::kCholLdsMaxTiles, svin::kBorderMaxRows, svin::kBorderScratchDoubles,
                     svin::kSbRec, svin::kSbFlo, svin::kSbFhi, svin::kSbMaxChain, svin::kSbCols};
  return c[which];
}
}
