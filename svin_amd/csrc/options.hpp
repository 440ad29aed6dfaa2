// Debug / A-B options of the library: ONE table, filled from the environment ONCE (the first time anything asks, which is
// svin_ba_create at the latest) and changed afterwards only through setDebugOption (C ABI: svin_ba_debug_set_option, for tests
// and tools).  Until round 5 these were two dozen getenv() calls, several of them per solve() / pack() and on the enqueue
// thread, where they raced with a setenv of the host process (VERDICT r5 "weak" 10).  Reading an option is one
// relaxed atomic load.  Every option is named after the environment variable that initialises it; none changes results beyond
// rounding -- they select between implementations of the same arithmetic or switch diagnostics on.
#pragma once
#include <atomic>

namespace svin {

enum DebugOption : int {
  kOptNoMailbox = 0,       // SVIN_NO_MAILBOX: scalar record by memcpy + synchronise instead of the pinned-host mailbox (read at create)
  kOptHostPack,            // SVIN_HOST_PACK: never use the device-resident window
  kOptSchurPairwise,       // SVIN_SCHUR_PAIRWISE: pairwise Schur kernel instead of the Gram-matrix forms
  kOptForceDistributed,    // SVIN_FORCE_DISTRIBUTED: a one-rank RCCL communicator runs the sharded code path
  kOptNoEarlyImu,          // SVIN_NO_EARLY_IMU
  kOptPackTiming,          // SVIN_PACK_TIMING: print pack() stage times
  kOptNoZeroCopyStates,    // SVIN_NO_ZERO_COPY_STATES
  kOptSplitEval,           // SVIN_SPLIT_EVAL: factor / reprojection / prior evaluation as separate launches
  kOptNoFuseStep,          // SVIN_NO_FUSE_STEP
  kOptNoDeferLm,           // SVIN_NO_DEFER_LM
  kOptNoSpeculation,       // SVIN_NO_SPECULATION: no speculative build behind the candidate evaluation
  kOptCholTiming,          // SVIN_CHOL_TIMING: print the in-kernel stage counters of a -DSVIN_CHOL_TIMING build
  kOptPgTiming,            // SVIN_PG_TIMING
  kOptMargTiming,          // SVIN_MARG_TIMING
  kOptMargKeepPre,         // SVIN_MARG_KEEP_PRE: keep the pre-marginalisation system for svin_ba_get_marg_pre
  kOptMargSyncEnqueue,     // SVIN_MARG_SYNC_ENQUEUE: issue the marginalisation job from the calling thread
  kOptMargEig,             // SVIN_MARG_EIG: 0 default chain, 1 "direct", 2 "cholesky", 3 "jacobi"
  kOptSchurAMfma,          // SVIN_SCHUR_A_MFMA
  kOptPanelsOld,           // SVIN_PANELS_OLD: the round-5 tile form of the wide-window Schur complement (k_schur_panels)
  kOptNoLL,                // SVIN_NO_LL: no left-looking one-workgroup solver
  kOptNoSbElim,            // SVIN_NO_SB_ELIM: no speed / bias chain elimination
  kOptNoLdsBorder,         // SVIN_NO_LDS_BORDER: no border variants of the LDS-resident solver
  kOptBlkRounds,           // SVIN_BLK_ROUNDS=n: workgroups of k_schur_rows per place (two places per CU; read by pack(); default 2)
  kOptBatchLanes,          // SVIN_BATCH_LANES=n: sub-batches of svin_ba_solve_prepared_batch on streams of their own (default 4)
  kOptBatchTiming,         // SVIN_BATCH_TIMING: print the host's issue / collect times of a batched solve
  kOptNoEvalSplit,         // SVIN_NO_EVAL_SPLIT: wide windows keep the one-launch evaluation (k_eval_all) and the one-workgroup-per-CU post-solve pass
  kOptSlabChunks,          // SVIN_SLAB_CHUNKS=n: chunks of 16 landmarks per workgroup of k_schur_dense (read by pack())
  kOptNoSbEarly,           // SVIN_NO_SB_EARLY: wide windows factorise the speed / bias chain inside the reduced solve, not beside the build
  kOptNoRowSplit,          // SVIN_NO_ROW_SPLIT: k_schur_rows work list with one accumulator set per block row (read by pack())
  kOptNoEvalBuild,         // SVIN_NO_EVAL_BUILD: evaluation and the build enqueued behind it as two launches (k_eval_all, k_schur_dense), never k_eval_build
  kOptLinearizeEvalBuild,  // SVIN_LINEARIZE_EVAL_BUILD: the inspection hooks svin_ba_linearize / svin_ba_debug_reduced_solve take their evaluation and
                           // build through k_eval_build where solve() would (tests: the launch against the two it replaces, on one handle)
  kOptNoStepInEval,        // SVIN_NO_STEP_IN_EVAL: the dogleg step stays in k_post_solve's tail, never at the head of k_eval_build's blocks
  kOptStepHookInEval,      // SVIN_STEP_HOOK_IN_EVAL: the inspection hook svin_ba_debug_trust_region_step (form 3) takes its step through
                           // k_post_solve without the tail + k_eval_build where solve() would (tests: the pair against the tail, on one handle)
  kOptImuRound64,          // SVIN_IMU_ROUND64: the IMU integration runs its per-step phases in rounds of 64 steps, two per covariance block,
                           // not one round of up to 128 (read at every launch of a kernel that integrates; same bits either way)
  kOptNoTileSkyline,       // SVIN_NO_TILE_SKYLINE: the LDS-resident reduced solve factors every tile, as if the window's tile skyline
                           // (pack_plan.hpp planTileSkyline) were dense (read by pack(); same bits either way)
  kOptCheckTileSkyline,    // SVIN_CHECK_TILE_SKYLINE: launchSolveReduced first synchronises, copies S to the host and throws if a tile
                           // outside the skyline holds anything but zeros (read by pack(); tests only)
  kOptNoTileDeal,          // SVIN_NO_TILE_DEAL: the LDS-resident reduced solve keeps the closed-form deal of its tile rows to its waves
                           // instead of the one planned from the window's tile skyline (pack_plan.hpp planTileDeal; read by pack() and by
                           // svin_ba_debug_solve_dense_profiled; same bits either way)
  kOptCount
};

int debugOption(DebugOption which);                        // current value (0 = off)
int setDebugOption(const char* name, int value);           // by environment-variable name; 1, or 0 for an unknown name
int debugOptionByName(const char* name, int* value);       // 1 and *value, or 0 for an unknown name
// read-only inspection field "SVIN_LAST_BATCH_IDLE_PPM": of the blocks the last svin_ba_solve_prepared_batch launched in the kernels
// whose grid differs from window to window, the share (parts per million) that left at once -- beyond their window's own extent, or
// of a window sitting out the stage (window.cpp, batch_plan.hpp)
int lastBatchIdlePpm();
// read-only inspection fields "SVIN_SPEC_BUILD_HITS" / "SVIN_SPEC_BUILD_MISSES": speculative builds of Window::solve this process has
// kept (the step was accepted and left the damping the build assumed) and discarded (window.cpp), either strategy
void countSpecBuild(bool kept, int n = 1);
long long specBuildHits();
long long specBuildMisses();
// read-only inspection field "SVIN_EVAL_BUILD_LAUNCHES": how many times this process has launched k_eval_build (kernels.hpp)
// read-only inspection field "SVIN_STEP_IN_EVAL_LAUNCHES": how many post-solve passes this process has launched without their tail,
// the step left to the blocks of the k_eval_build launch behind them (kernels.hpp)
// read-only inspection fields "SVIN_LAST_TILE_SKYLINE_LO" / "SVIN_LAST_TILE_SKYLINE_HI": the tile skyline the LDS-resident reduced
// solve was launched with last, as nT - 1 - hi[k] in four bits per tile column -- columns 0 .. 6 / 7 .. 10 (kernels.hpp)
inline bool optOn(DebugOption which) { return debugOption(which) != 0; }

}  // namespace svin
