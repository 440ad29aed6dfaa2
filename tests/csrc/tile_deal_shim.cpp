// C entry point over planTileDeal (svin_amd/csrc/pack_plan.hpp: the deal of the reduced system's tile rows to the waves of the
// LDS-resident solver) for tests/test_tile_deal_host.py and tests/test_gpu_tile_deal.py: the planner takes a skyline as a flat
// integer array, so its deals are checked on the CPU, and rehearsed against a model of the solver's flag protocol, before a kernel
// ever runs one.
#include <cstdint>
#include "../../svin_amd/csrc/pack_plan.hpp"

extern "C" {
int td_max_tiles() { return svin::kTileSkylineMaxTiles; }
int td_quiet_wave() { return svin::kTileDealQuietWave; }
// hi[nT]: the skyline.  owner[11]: the wave of every tile row (0: rows 0, 1 and beyond nT).  Returns the word DeviceProblem carries.
uint64_t td_plan(int nT, const int32_t* hi, int32_t* owner) {
  int h[svin::kTileSkylineMaxTiles] = {};
  for (int k = 0; k < nT && k < svin::kTileSkylineMaxTiles; ++k) h[k] = hi[k];
  const svin::TileDeal t = svin::planTileDeal(nT, h);
  for (int I = 0; I < svin::kTileSkylineMaxTiles; ++I) owner[I] = t.owner[I];
  return t.word;
}
// the same from the packed profile (DeviceProblem::tileCut), as svin_ba_debug_solve_dense_profiled plans it
uint64_t td_plan_cut(int nT, uint64_t cut) { return svin::planTileDeal(nT, cut).word; }
int td_owner_of(uint64_t word, int nT, int I) { return svin::tileDealOwnerOf(word, nT, I); }
int td_base_owner(int nT, int I) { return svin::tileDealBaseOwner(nT, I); }
unsigned td_base_rows(int nT, int w) { return svin::tileDealBaseRows(nT, w); }
}
