// A stand-alone run of planTileSkyline (svin_amd/csrc/pack_plan.hpp) for AddressSanitizer and UndefinedBehaviorSanitizer:
// tests/test_tile_skyline_host.py compiles this file with -fsanitize=address,undefined -fno-sanitize-recover=all, hands it the
// cases of that test as a text file and holds what it prints against the shim's answers.
// One case per line:  d dC recognised nCliques  { nBlocks { off len } }   ->   "nT hi[0] .. hi[nT-1] | pre[0] .. pre[nT-1] | cut cutPre"
#include <cstdio>
#include <vector>
#include "../../svin_amd/csrc/pack_plan.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int d, dC, recognised, nC, cases = 0;
  while (std::fscanf(f, "%d %d %d %d", &d, &dC, &recognised, &nC) == 4) {
    std::vector<int> ptr(1, 0), off, len;
    for (int c = 0; c < nC; ++c) {
      int nB = 0;
      if (std::fscanf(f, "%d", &nB) != 1) return 3;
      for (int b = 0; b < nB; ++b) {
        int o, l;
        if (std::fscanf(f, "%d %d", &o, &l) != 2) return 3;
        off.push_back(o); len.push_back(l);
      }
      ptr.push_back((int)off.size());
    }
    const svin::TileSkyline t = svin::planTileSkyline(d, dC, ptr, off, len, recognised != 0);
    std::printf("%d", t.nT);
    const int n = t.nT <= svin::kTileSkylineMaxTiles ? t.nT : 0;
    for (int k = 0; k < n; ++k) {
      std::printf(" %d", t.hi[k]);
      if (svin::tileHiOf(t.cut, t.nT, k) != t.hi[k] || svin::tileHiOf(t.cutPre, t.nT, k) != t.pre[k]) return 4;
    }
    std::printf(" |");
    for (int k = 0; k < n; ++k) std::printf(" %d", t.pre[k]);
    std::printf(" | %llu %llu\n", (unsigned long long)t.cut, (unsigned long long)t.cutPre);
    ++cases;
  }
  std::fclose(f);
  return cases > 0 ? 0 : 1;
}
