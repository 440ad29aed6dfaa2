// svin_amd: the one dimension the 16 x 16 tile helpers (tile16.hpp) and the host planning of the reduced solve (solve_plan.hpp)
// share.  HIP-free.
#pragma once

namespace svin {

constexpr int kPanelLd = 17;  // leading dimension of the 16x16 LDS tiles of the dense solvers

}  // namespace svin
