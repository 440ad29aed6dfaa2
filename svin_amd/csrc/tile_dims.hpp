// svin_amd: dimensions that kernels and HIP-free host planning share and that more than one planning header needs: the 16 x 16
// tile helpers (tile16.hpp) and the reduced solve (solve_plan.hpp) share the tile stride, pack() (pack_plan.hpp) and the build's
// launchers (build_plan.hpp) the pairwise form's LDS test.  HIP-free.
#pragma once
#include <cstddef>

namespace svin {

constexpr int kPanelLd = 17;  // leading dimension of the 16x16 LDS tiles of the dense solvers
constexpr int kSymEigMaxN = 128;  // largest matrix of the prior's direct eigen-solver (symeig.hpp; planned in marg_plan.hpp)

// pairwise form of the landmark elimination (k_schur): four waves stage 64 observations each, and a workgroup keeps a private
// slab (the dC x dC block + gRed | gFull | hC) in LDS when it fits next to that.  ONE function: pack() sizes the slab buffer and
// the slab count from it, the launcher picks the kernel from it and k_reduce_slabs is told how many slabs to sum from it.
constexpr int kStage = 34;  // doubles staged per observation: Jl 6, Jp 12, Je 12, offP, offE (as double), pad
constexpr size_t kPairwiseStageBytes = (size_t)4 * 64 * kStage * 8;
constexpr size_t pairwiseSlabBytes(int dC) { return ((size_t)dC * dC + 3 * (size_t)dC) * 8; }
constexpr bool pairwiseSlabFitsLds(int dC) { return pairwiseSlabBytes(dC) + kPairwiseStageBytes <= 150 * 1024; }

}  // namespace svin
