// C entry points over svin_amd/csrc/batch_plan.hpp (the host planning of svin_ba_solve_prepared_batch) for
// tests/test_batch_plan_host.py: the group key, the per-window extents of every launch, the sort and the cut into lanes are
// HIP-free, so their rules are checked on the CPU.
#include "../../svin_amd/csrc/batch_plan.hpp"

namespace {
svin::BatchGroupFields fieldsOf(const int* v) {
  return svin::BatchGroupFields{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13]};
}
// L, N, F, nPose, nExt, nSb, priorM, ownsCamera, nSlabs
svin::BatchDims dimsOf(const int* v) { return svin::BatchDims{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]}; }
}  // namespace

extern "C" {
int bp_key_fields() { return svin::BatchGroupKey::kFields; }
// 1: the two windows belong to one group (neither key orders before the other, and they compare equal)
int bp_same_group(const int* a, const int* b) {
  const svin::BatchGroupKey ka = svin::batchGroupKey(fieldsOf(a)), kb = svin::batchGroupKey(fieldsOf(b));
  const bool eq = !(ka < kb) && !(kb < ka);
  return (eq == (ka == kb)) ? (eq ? 1 : 0) : -1;
}
int bp_slab_count(int L) { return svin::denseSlabCount(L); }
// out: buildSlabs, buildFac, buildPri, postLm, postFac, step, evalR, evalF, evalPri, build(), post(), evalRest()
void bp_extents(const int* dims, int* out) {
  const svin::BatchExtents e = svin::batchExtentsOf(dimsOf(dims));
  const int v[12] = {e.buildSlabs, e.buildFac, e.buildPri, e.postLm, e.postFac, e.step, e.evalR, e.evalF, e.evalPri, e.build(), e.post(), e.evalRest()};
  for (int k = 0; k < 12; ++k) out[k] = v[k];
}
// the grid of a lane's round: dims = n x 9, stages = n; out: build, post, step, evalR, evalRest, blocks(union) per window row,
// busy blocks of all windows
void bp_lane_grid(int n, const int* dims, const int* stages, long long* out) {
  svin::BatchGrid g;
  int uni = 0;
  long long busy = 0;
  for (int i = 0; i < n; ++i) {
    const svin::BatchExtents e = svin::batchExtentsOf(dimsOf(dims + 9 * i));
    g.include(e, stages[i]);
    busy += svin::batchBusyBlocks(e, stages[i]);
    uni |= stages[i];
  }
  out[0] = g.build; out[1] = g.post; out[2] = g.step; out[3] = g.evalR; out[4] = g.evalRest; out[5] = g.blocks(uni); out[6] = busy;
}
// order: n sorted positions -> window index; laneFirst / laneCount: up to maxLanes entries; returns the number of lanes
int bp_plan_lanes(int n, const int* L, const int* N, int maxLanes, int* order, int* laneFirst, int* laneCount) {
  std::vector<svin::BatchDims> ws((size_t)n);
  for (int i = 0; i < n; ++i) ws[(size_t)i] = svin::BatchDims{L[i], N[i], 0, 0, 0, 0, 0, 1, svin::denseSlabCount(L[i])};
  const svin::BatchLanePlan plan = svin::planBatchLanes(ws, maxLanes);
  for (int i = 0; i < n; ++i) order[i] = plan.order[(size_t)i];
  for (size_t k = 0; k < plan.lanes.size(); ++k) { laneFirst[k] = plan.lanes[k].first; laneCount[k] = plan.lanes[k].count; }
  return (int)plan.lanes.size();
}
}
