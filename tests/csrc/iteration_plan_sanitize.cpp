// A stand-alone run of svin_amd/csrc/iteration_plan.hpp (the accumulator ledger and the plan of a pass of Window::solve) for
// AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_iteration_plan_host.py compiles this file with
// -fsanitize=address,undefined -fno-sanitize-recover=all, hands it cases of that test as a text file and holds what it prints
// against the shim's answers.
// One case per line:  cfg[0..5] nPass event[0] .. event[nPass-1]   ->   the passes run, then their rows (iteration_plan_shim.cpp)
// A second file, if given, holds passes put together by hand, one per line:  f[0..6] prepareRadius cand   ->   ip_batch_stages' answer
// (the branches of batchStagesOf that throw are reached this way only)
#include <cstdio>
#include <vector>
#include "iteration_plan_shim.cpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int32_t cfg[6];
  int cases = 0;
  while (std::fscanf(f, "%d %d %d %d %d %d", &cfg[0], &cfg[1], &cfg[2], &cfg[3], &cfg[4], &cfg[5]) == 6) {
    int nPass;
    if (std::fscanf(f, "%d", &nPass) != 1 || nPass < 0 || nPass > 64) return 3;
    std::vector<int32_t> events((size_t)nPass);   // exactly nPass entries: a read beyond the script is an error the sanitizer reports
    for (int k = 0; k < nPass; ++k)
      if (std::fscanf(f, "%d", &events[(size_t)k]) != 1) return 3;
    std::vector<double> rows((size_t)nPass * kIpFields, 0.0);
    const int ran = ip_run(cfg, events.data(), nPass, rows.data());
    std::printf("%d", ran);
    for (double v : rows) std::printf(" %.17g", v);
    std::printf("\n");
    ++cases;
  }
  std::fclose(f);
  if (argc > 2) {
    std::FILE* h = std::fopen(argv[2], "r");
    if (!h) return 2;
    int32_t p[7];
    double radius;
    int cand;
    while (std::fscanf(h, "%d %d %d %d %d %d %d %lf %d", &p[0], &p[1], &p[2], &p[3], &p[4], &p[5], &p[6], &radius, &cand) == 9)
      std::printf("stages %d\n", ip_batch_stages(p, radius, cand));
    std::fclose(h);
  }
  return cases > 0 ? 0 : 1;
}
