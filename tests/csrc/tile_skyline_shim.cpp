// C entry point over planTileSkyline (svin_amd/csrc/pack_plan.hpp: the tile skyline of the reduced system that the LDS-resident
// solver factors inside) for tests/test_tile_skyline_host.py and tests/test_gpu_chol_skyline.py: the planner takes flat integer
// arrays, so its profiles are checked on the CPU against a symbolic Cholesky (tests/helpers/tile_skyline_lib.py).
#include <cstdint>
#include <vector>
#include "../../svin_amd/csrc/pack_plan.hpp"

extern "C" {
int ts_max_tiles() { return svin::kTileSkylineMaxTiles; }
// cliques: CSR (ptr[nCliques + 1]) over the row ranges (off, len).  out: hi[11], pre[11]; cut[2] = the two words DeviceProblem carries.
// Returns nT.
int ts_plan(int d, int dC, int nCliques, const int32_t* ptr, const int32_t* off, const int32_t* len, int recognised, int32_t* hi, int32_t* pre,
            uint64_t* cut) {
  const std::vector<int> p(ptr, ptr + nCliques + 1), o(off, off + ptr[nCliques]), l(len, len + ptr[nCliques]);
  const svin::TileSkyline t = svin::planTileSkyline(d, dC, p, o, l, recognised != 0);
  for (int k = 0; k < svin::kTileSkylineMaxTiles; ++k) { hi[k] = t.hi[k]; pre[k] = t.pre[k]; }
  cut[0] = t.cut; cut[1] = t.cutPre;
  return t.nT;
}
int ts_hi_of(uint64_t cut, int nT, int k) { return svin::tileHiOf(cut, nT, k); }
}
