// A stand-alone run of planTileDeal (svin_amd/csrc/pack_plan.hpp) for AddressSanitizer and UndefinedBehaviorSanitizer:
// tests/test_tile_deal_host.py compiles this file with -fsanitize=address,undefined -fno-sanitize-recover=all, hands it the cases of
// that test as a text file and holds what it prints against the shim's answers.
// One case per line:  nT hi[0] .. hi[nT-1]   ->   "word owner[2] .. owner[nT-1]"   (the owners decoded from the word)
#include <cstdio>
#include <vector>
#include "../../svin_amd/csrc/pack_plan.hpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int nT, cases = 0;
  while (std::fscanf(f, "%d", &nT) == 1) {
    if (nT < 0 || nT > 64) return 3;
    std::vector<int> hi((size_t)nT);   // exactly nT entries: a read beyond the profile is an error the sanitizer reports
    for (int k = 0; k < nT; ++k)
      if (std::fscanf(f, "%d", &hi[(size_t)k]) != 1) return 3;
    const svin::TileDeal t = svin::planTileDeal(nT, hi.data());
    std::printf("%llu", (unsigned long long)t.word);
    const int n = nT <= svin::kTileSkylineMaxTiles ? nT : 0;
    for (int I = 2; I < n; ++I) {
      if (svin::tileDealOwnerOf(t.word, nT, I) != t.owner[I]) return 4;
      std::printf(" %d", t.owner[I]);
    }
    if (n >= 2 && svin::planTileDeal(nT, svin::packTileCut(hi.data(), nT)).word != t.word) return 5;
    std::printf("\n");
    ++cases;
  }
  std::fclose(f);
  return cases > 0 ? 0 : 1;
}
