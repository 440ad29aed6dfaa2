// svin_amd: device data layout and kernel launch interface (host side sees plain structs).
//
// HBM layout (all FP64 unless noted; SoA so that lane i of a wave touches element i):
//   parameter tables   pose[nPose][7]  ext[nExt][7]  sb[nSb][9]  lm[L][4]   (+ candidate copies)
//   reduced-system map poseOff/extOff/sbOff: first row of the block in the reduced system or -1 (fixed)
//                      order: [poses | variable extrinsics | speed-biases]  -> the leading dC rows are
//                      the only ones reprojection factors touch
//   observations       landmark-major CSR: lmPtr[L+1]; per observation uv(2) w(1) packed index (u32)
//                      and landmark index (i32)
//   linearisation      r[2][N] Jp[12][N] Jl[6][N] Je[12][N]  (component-major: a wave writes/reads
//                      512 contiguous bytes per component) -- two sets (current / candidate)
//   small factors      DevFactor[F] + FactorLin[F] (r[15], J[15x30]) ; DevImu[nImu] pre-integration state
//   prior              H-space form of the marginalisation prior (Ht m x m, bp m, c0) + block table
//   normal equations   S[d][d], gRed[d], gFull[d], hC[d], per-landmark Vinv[6] bl[3] hL[3] scaleL[3]
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <hip/hip_runtime.h>
#include "dmath.hpp"
#include "options.hpp"
#include "batch_plan.hpp"
#include "cov_plan.hpp"
#include "pack_plan.hpp"
#include "solve_plan.hpp"
#include "build_plan.hpp"

namespace svin {

constexpr int kMaxCams = 8;
constexpr int kPriorCam = 15;   // camera field of a packed index that marks a landmark-prior pseudo-observation (HomogeneousPointError)

// packed per-observation index: pose slot (12 bit) | ext slot (12 bit) | camera (4 bit) | loss selector (4 bit, an entry of the
// window's loss table DeviceProblem::lossTab; 0 = CauchyLoss(1)).  `cam` may carry the selector in its bits 4-7 (a packed index
// shifted right by 24, as the resident kernels pass it on)
inline __host__ __device__ uint32_t packObs(int pose, int ext, int cam, int loss = 0) {
  return (uint32_t)pose | ((uint32_t)ext << 12) | ((uint32_t)cam << 24) | ((uint32_t)loss << 28);
}
// residual loss functions (Ceres' TrivialLoss, CauchyLoss(a), HuberLoss(a)): dmath.hpp residualLoss
enum LossKind : int { LOSS_NONE = 0, LOSS_CAUCHY = 1, LOSS_HUBER = 2 };
// (kMaxLosses, kLossTabBytes -- a window's reprojection loss table, entry 0 CauchyLoss(1) -- : build_plan.hpp, with the staging area they size)

struct ImuParams {
  double a_max, g_max, sigma_g_c, sigma_a_c, sigma_bg, sigma_ba, sigma_gw_c, sigma_aw_c, tau, g;
  double a0[3];
};

struct DevImu {
  int sampleStart, sampleCount;  // into the imu sample pool
  uint32_t t0[2], t1[2];
  ImuParams par;
  int redo, redoCounter;
  double Delta_t;
  double Delta_q[4], C_integral[9], C_doubleintegral[9], acc_integral[3], acc_doubleintegral[3];
  double dalpha_db_g[9], dv_db_g[9], dp_db_g[9];
  double P_delta[225], information[225], sqrtInfo[225];
  double sb_ref[9];
};

enum FactorKind : int { F_IMU = 0, F_POSE_PRIOR = 1, F_SB_PRIOR = 2, F_RELPOSE = 3, F_SONAR = 4, F_DEPTH = 5,
                        F_HOST = 6 };   // residual and minimal Jacobians computed by a callback of the host (Window::evaluateHostFactors) before every evaluation launch
enum BlockKind : int { B_POSE = 0, B_EXT = 1, B_SB = 2, B_LM = 3 };

struct DevFactor {
  int kind, nblk, m, imuIndex;
  int blkKind[4], blkSlot[4];
  int lossKind, lossPad;   // LossKind of the factor (LOSS_NONE by default) and its scale a
  double lossScale;
  double meas[9];       // pose prior: T(7); sb prior: 9; sonar: range, heading, mean(3); depth: depth, firstDepth
  double aux[8];        // sonar: T_SSo(7)
  double sqrtInfo[81];  // row-major m x m (upper-triangular L^T)
};
struct FactorLin {
  double r[15];
  double J[15 * 30];  // row-major m x ncols, blocks concatenated in order (r and J WITHOUT the loss: Map::getLhs reads them)
  double sc;          // sqrt(rho') of the factor's loss at r (1 without one): every consumer of the solve scales r and J by it
  int off[4], dim[4], m, ncols;
};

struct PriorBlock {
  int kind, slot;  // BlockKind / table slot (B_LM unsupported in the solver: priors never keep landmarks)
  int ord, mdim;   // first row in the prior, minimal dimension (0 when the block was fixed)
  double lin[9];   // linearisation point
};

// scalar results of one iteration, read back by the host once per iteration
struct SolverScalars {
  // --- group A (8 summable scalars): produced by the step (retraction) and the candidate evaluation
  double cost;            // cost at the evaluated point (current or candidate)
  double costReproj, costFactors, costPrior;
  double stepNormSq, xNormSq;
  double spareA0, spareA1;
  // --- group B (8 summable scalars): produced once per linearisation by the post-solve pass.  With
  // v = g / htil (steepest descent) and y = Gauss-Newton solution, J*delta is linear in the dogleg
  // coefficients, so the five J sums below price ANY dogleg step of this linearisation.
  double gHatSq;          // |g_hat|^2
  double jgSq;            // |J v|^2                    (Cauchy point)
  double gnHatSq;         // |gn_hat|^2
  double gDotGn;          // g_hat . gn_hat
  double jySq;            // |J y|^2
  double jvDotJy;         // (J v).(J y)
  double jvDotR;          // (J v).r
  double jyDotR;          // (J y).r
  // --- sharded mode: every rank's (gradMax, failMax) pair in its own slot, the other slots zero, so that the SUM all-reduce
  // of [group B | gather] in ONE message gathers them and the host takes the max (a max all-reduce of its own before)
  double gather[16];
  // --- 2 max-reduced scalars (one GPU: written directly; sharded: the host fills them from `gather`)
  double gradMax;         // max |g_full|
  double failMax;         // (double)cholFail
  // --- derived on the device from the (all-reduced) sums and the trust-region radius
  double jdSq, jdDotR;    // |J delta|^2 , (J delta).r   (model cost change)
  double doglegStepNorm;
  int cholFail;           // bits 1 | 2: S or a landmark block is not positive definite (numerical: the mu ladder retries);
                          // bits 4 | 8 (kCholFailSync): a bounded device-side wait of a solver kernel gave up (a fault: solve() throws)
  int pad;
};
// pinned-host mailbox: the kernel that sums the cost publishes all scalars + the sequence number of that evaluation
struct ScalarMailbox {
  SolverScalars scal;
  unsigned long long seq;
};
constexpr int kCholFailSync = 4 | 8;
constexpr int kScalGroupA = 0, kScalGroupB = 8, kScalGather = 16, kScalGatherSlots = 16;  // offsets (doubles) of the all-reduced groups

// kPanelChunksPerBlock, kBlk* (the work lists of the wide-window Schur kernels) and kDensePoseCap: pack_plan.hpp, with the host
// code that builds those lists

struct DeviceProblem {
  // sizes
  int nPose, nExt, nSb, L, N, F, nImu, d, dC, priorM, priorBlocks, nCam;
  int anyExtVariable;
  int ownsCamera;   // landmark-sharded mode: only one rank takes the marginalisation prior and the camera-side norms (the small
                    // factors are dealt to the ranks frame by frame at pack() time: each rank's F counts its own)
  int rank, world;  // sharded mode (0, 1 otherwise)
  // tables
  double *pose, *ext, *sb, *lm;
  double *poseC, *extC, *sbC, *lmC;
  int *poseOff, *extOff, *sbOff;
  CameraModel* cams;
  // observations
  int* lmPtr;
  int schurDense;                            // narrow window: Schur complement as a Gram matrix on MFMA
  int schurPanels, nPanelBlocks, nPanelPairs;  // wide window: the same per 96-row panel pair (k_schur_panels)
  const int4* panelWork;                     // per workgroup: panel I, panel J, first chunk entry, chunk count
  const int* panelChunks;                    // chunk ids (16 landmarks each) of the work list
  const int* panelPairPtr;                   // per panel pair: first workgroup (nPanelPairs + 1 entries)
  // wide window, block-pair form (round 6: k_blocks_slots / k_schur_rows): a SLOT is a (landmark, distinct variable pose) pair
  int schurBlocks, nSlots;                   // 1: the panel work list is processed by k_schur_rows (0: the tile form k_schur_panels)
  const int* slotPtr;                        // per landmark: first slot (L + 1 entries); a landmark's slots ascend with the pose
  const unsigned short* slotBlk;             // per slot: pose block of the reduced camera system (poseOff / 6)
  const int* slotObsPtr;                     // per slot: its observations (nSlots + 1 entries into slotObs)
  const int* slotObs;                        // observation numbers
  const int* slotLm;                         // per slot: its landmark
  double* slotRec;                           // per slot kBlkRec doubles, written once per build: E = (sum Jp^T Jl) L^-T (kernels.hip)
  // work list of k_schur_rows (host-built, pack_plan.hpp buildSchurRowsWorkList): panelWork.z / .w = first batch / batches of the workgroup
  const int4* blkOwn;                        // per workgroup: the two block rows of wave w in bytes 2 w, 2 w + 1 (255: none)
  const int2* blkBatch;                      // per batch: first entry of blkRecSlot, records
  const int4* blkWaveTab;                    // per (batch, wave): first pair word, pair words of its first / second row (multiples of 8, together at most kBlkBatchWords)
  const int* blkRecSlot;                     // per staged record: its slot
  const uint32_t* blkPairs;                  // pair words: 2 x pose block in J | B record's byte offset << 8 | A record << 24; words 2 j and 2 j + 1 share their A record
  double* blkPartial;                        // per workgroup of k_blocks_slots: (dC / 6) x 28 sums of Jp^T Jp (21) and Jp^T r (6)
  double *obsUv, *obsW;
  uint32_t* obsIdx;
  int dCPose, aBlocks;   // rows of the variable poses in the reduced camera system; dense Schur: A accumulated block-wise in LDS (aBlocks:
                         // zero in a window's own problem at all times -- the build launchers set it in their copy, the batched loop in the slot's)
  const int* obsOrder;   // dense Schur with the A part on MFMA: the observations of every 16-landmark chunk sorted by pose (or null)
  int* obsLm;
  // linearisation buffers (cur = accepted point, cand = candidate)
  double *rCur, *JpCur, *JlCur, *JeCur;
  double *rCand, *JpCand, *JlCand, *JeCand;
  // factors
  DevFactor* factors;
  FactorLin *linCur, *linCand;
  DevImu* imus;
  uint32_t* imuT;    // [M][2]
  double* imuMeas;   // [M][6]
  // prior (H-space)
  double *priorH, *priorBp;
  const double* priorC0;                     // e0.e0 of the prior (device scalar)
  PriorBlock* priorBlk;
  double *priorDchi, *priorGrad, *priorM3;      // linearisation of the prior at the accepted point: m, m, 9 per block
  double *priorDchiC, *priorGradC, *priorM3C;   // ... at the candidate (swapped on acceptance)
  double *priorMv, *priorMy;                    // scratch m
  // normal equations
  double *S, *gRed, *gFull, *hC, *htilC, *scaleC;
  int sPadded;   // S has ((d + 15) / 16) * 16 rows of ldS doubles, zero beyond row / column d (the window's own buffer)
  int ldS;   // leading dimension of S.  The window sets it to d rounded up to 16 doubles (every 16-column tile row segment is then ONE
             // 128-byte cache line: the tile loads of the solvers touch half as many lines); 0 = d for a caller that only uses
             // launchSolveReduced on a principal block of its own matrix (pose graph root)
  double *Vinv, *bl, *hL, *scaleL;           // per landmark 6 / 3 / 3 / 3
  double *slabs; int nSlabs;                 // per-workgroup private copies of the leading dC x dC block (+2 dC vectors)
  double *yC, *yL;                           // Gauss-Newton solution (cam d, landmarks 3L)
  double *deltaC, *deltaL;                   // trust-region step
  double *vC, *vL;                           // generic vector for J*v passes
  double *cholL;                             // factor of S
  SolverScalars* scal;
  double* partial;                           // reduction scratch
  unsigned int* tickets;                     // last-block-done counters of the fused reductions
  // What ONE launch is told besides the window (PassArgs, below): null / zero in a window's own problem at all times, set by the
  // launcher in the copy it launches with (withPassArgs), by the batched loop in the slot's copy
  ScalarMailbox* mailbox;                    // host-visible copy of the scalars (nullptr: disabled)
  unsigned long long mailboxSeq;             // sequence number to publish with this evaluation
  int lmDeferred;                            // fused step: the landmark part of the retraction is taken by the candidate evaluation
  int padDeferred;
  const double* lmPrior;                     // landmark priors: 12 doubles each (measurement xyz, upper-triangular sqrt information row-major)
  double* lmFactor;                          // wide windows: per landmark L^-1 of (V + mu D) (6) and c = L^-1 b (3), written by
                                             // k_panels_landmarks once per build, read by every panel pair of k_schur_panels
  int sbChain;                               // > 0: the rows dC .. d are sbChain variable speed / bias blocks (9 rows each) that
                                             // couple only with their neighbours in this order (IMU factors) and with the kept rows:
                                             // the blocked solver eliminates them as a chain first (k_sb_factor ...)
  // poses / extrinsics on a reduced manifold (Map::Pose3d / Pose4d / Pose2d, PoseManifold.cpp:173-466): the rows of the reduced
  // system that belong to their LOCKED tangent directions.  launchSolveReduced turns each into an identity row with a zero
  // right-hand side first (k_lock_rows) -- the same system as with those Jacobian columns removed, the step stays zero there
  const int* lockedRows;
  int nLocked;
  int nHostFactors;   // factors of kind F_HOST in `factors` (such a window is not batched: the host evaluates between the launches)
  int reservedZero;   // always zero, never read (a host flag once travelled here): the slot stays so that the device code compares equal
  const double* lossTab;   // reprojection loss table: (kind, a) per selector of the packed index; nullptr = every selector 0 (CauchyLoss(1))
  // General 2x2 information on reprojection residuals: the upper-triangular square-root information S = (s00, s01, s11) of every
  // observation, component-major with stride N like the Jacobian arrays (obsS[c * N + o]).  nullptr = every observation is
  // isotropic: the evaluation reads obsW alone and takes the scalar arithmetic.  When set, |obsW| = s00 and only its sign
  // (constant landmark) is read.  Host-packed windows only (the device-resident window's records carry one weight).
  const double* obsS;
  // Tile skyline of S for the LDS-resident solver (pack_plan.hpp planTileSkyline): four bits per tile column k, nT - 1 - hi[k], hi[k]
  // the last tile row of the column that can hold a non-zero -- after the fill of the factorisation (tileCut: k_chol_solve_lds<0>
  // leaves the tiles below it alone) and before it (tileCutPre: what SVIN_CHECK_TILE_SKYLINE holds S against).  0 -- a cleared
  // problem, every caller but Window::pack() -- is the dense profile.  kTileCheckBit of tileCutPre: SVIN_CHECK_TILE_SKYLINE was on at pack().
  unsigned long long tileCut, tileCutPre;
  // The deal of the tile rows to the waves of that solver (pack_plan.hpp planTileDeal): four bits per tile row I >= 2, the wave that
  // owns the row; 0 -- a cleared problem, every caller but Window::pack() -- is the closed form for that row (tileDealBaseOwner).
  unsigned long long tileDeal;
};
constexpr unsigned long long kTileCheckBit = 1ull << 63;
// What a single launch is told besides the window.  A window's problem is constant from one pack() to the next, apart from the set
// swap of an accepted step; the launchers that can publish the scalars or read lmDeferred take this record and launch with a copy.
struct PassArgs {
  ScalarMailbox* mailbox = nullptr;      // where the launch's cost sum publishes the scalars (nullptr: it does not)
  unsigned long long mailboxSeq = 0;     // ... with this sequence number
  int lmDeferred = 0;                    // DeviceProblem::lmDeferred
};
inline DeviceProblem withPassArgs(const DeviceProblem& p, const PassArgs& a) {
  DeviceProblem q = p;
  q.mailbox = a.mailbox; q.mailboxSeq = a.mailboxSeq; q.lmDeferred = a.lmDeferred;
  return q;
}
unsigned long long lastTileCut();   // tileCut of the last launch of k_chol_solve_lds<0> / _batch<0> (options.hpp SVIN_LAST_TILE_SKYLINE_LO / _HI)

// ---- batched solve (svin_ba_solve_prepared_batch: B independent windows through ONE launch sequence per trust-region round, the
// window as blockIdx.y).  The windows of a batch agree in what the launcher computes once per launch (batch_plan.hpp
// BatchGroupFields: reduced system, factors, prior, cameras); their landmark and observation counts may differ.  One slot per
// window, refilled by the host every round: the window's problem as it stands (buffer sets swapped by its accepted steps,
// mailbox sequence number of this round's evaluation), the scalars its own trust region hands the kernels, and the window's
// OWN extent of every launch (`ext`: the grid the single-window launcher would take) -- a block finds its role from it and leaves
// at once when blockIdx.x lies beyond it; `stages` (kBatchFull / kBatchReuse / kBatchEval) says which launches of the round the
// window takes part in.
struct BatchSlot {
  DeviceProblem p;
  double mu, radius;
  int initScale, stages;
  BatchExtents ext;
};
inline BatchDims batchDimsOf(const DeviceProblem& p) { return BatchDims{p.L, p.N, p.F, p.nPose, p.nExt, p.nSb, p.priorM, p.ownsCamera, p.nSlabs}; }
// the integers the planners of build_plan.hpp take
inline BuildDims buildDimsOf(const DeviceProblem& p) {
  return BuildDims{p.dC, p.dCPose, p.L, p.N, p.F, p.priorM, p.ownsCamera, p.anyExtVariable, p.schurDense, p.schurPanels, p.schurBlocks, p.nSlabs,
                   p.nSlots, p.nPanelBlocks, p.nPanelPairs};
}
inline EvalDims evalDimsOf(const DeviceProblem& p) { return EvalDims{p.nPose, p.nExt, p.nCam, p.L, p.N, p.F, p.priorM}; }
// `p` as it looks after an accepted step: the candidate sets (parameter tables, linearisation buffers, the factors' and the
// prior's linearisation) are the current ones and the other way round
inline DeviceProblem withSetsSwapped(const DeviceProblem& p) {
  DeviceProblem q = p;
  std::swap(q.pose, q.poseC); std::swap(q.ext, q.extC); std::swap(q.sb, q.sbC); std::swap(q.lm, q.lmC);
  std::swap(q.rCur, q.rCand); std::swap(q.JpCur, q.JpCand); std::swap(q.JlCur, q.JlCand); std::swap(q.JeCur, q.JeCand);
  std::swap(q.linCur, q.linCand);
  std::swap(q.priorDchi, q.priorDchiC); std::swap(q.priorGrad, q.priorGradC); std::swap(q.priorM3, q.priorM3C);
  return q;
}
// the plans of a window as it stands (the debug options are read here, once per call)
BuildPlan buildPlanOf(const DeviceProblem& p);
EvalPlan evalPlanOf(const DeviceProblem& p);
StepMode stepModeOf(const DeviceProblem& p, bool sharded);
void releaseSideLane(hipStream_t s);   // frees the side stream / events kernels.hip keeps for solver stream `s` (before `s` is destroyed)
bool batchSupported(const DeviceProblem& p);   // the geometry the batched kernels cover (otherwise the window is solved on its own)
// one round for the `n` windows of dSlots (device copy of the slot table); `geom` = any window of the batch (what the launcher reads
// of it is equal in all of them), `grid` = gridDim.x of every launch (the largest extent among the windows taking part),
// `stagesUnion` = OR of the slots' stages, `cand` as for launchEvalAll
// `anyObsS`: a window of the batch has DeviceProblem::obsS set (the reprojection blocks then run the kernel that can read it)
void launchBatchRound(const BatchSlot* dSlots, const DeviceProblem& geom, const BatchGrid& grid, int n, int stagesUnion, bool cand, hipStream_t s,
                      bool anyObsS = false);
int schurDenseABlocks(const DeviceProblem& p);   // DeviceProblem::aBlocks as launchAccumulateNormalEquations chooses it (BuildPlan::aBlocks)
// Which landmark-elimination form launchAccumulateNormalEquations launched last in this process (read-only inspection field,
// svin_ba_debug_get_option("SVIN_LAST_SCHUR_FORM")): 0 none yet; 1000 + 10 MAXT + a for k_schur_dense<MAXT, ...> (a = 0: A in per-wave
// block copies, 1: A on MFMA block-wise, 2: A on MFMA tile-wise); 2000 k_blocks_slots + k_schur_rows; 3000 k_schur_panels;
// 4000 / 4001 pairwise k_schur with LDS slabs / global atomics; 5000 small factors only.
int lastSchurForm();
// Evaluation and the build of the normal equations AT THE EVALUATED POINT in one launch (k_eval_build) + k_reduce_slabs: what
// launchEvalAll(p, a, cand, true, s) followed by launchAccumulateNormalEquations(view, mu, initScale, s, false) computes, `view` being
// `p` itself for cand = false and `p` with its current / candidate sets swapped for cand = true.  The accumulators are clean.
// Returns false, having launched nothing, for a window the launch does not take (build_plan.hpp evalBuildTaken: any form but the
// narrow dense one with fixed extrinsics, a sharded window, more workgroups than compute units): the caller issues the two launches.
// factorsCommute: no entry of S receives more than two of the small factors' / the prior's atomic additions (they start from zero,
// so their order does not matter): the factor blocks of the launch add their factor themselves.  Otherwise the factors and the
// prior keep a launch of their own (k_factors_only) behind it, where their blocks start together as they do in k_schur_dense --
// sums of three and more terms then come out the same from run to run as far as they did before.
// stepRadius > 0 (cand only, behind launchDoglegPrepare(..., noTail = true)): every evaluation and chunk block first takes the dogleg
// step of that radius itself, from the partials of the post-solve pass (stepHead, kernels.hip), and evaluates at the candidate it
// holds in its own LDS; the first reprojection block stores the candidate blocks and the step's record.
bool launchEvalBuild(const DeviceProblem& p, const PassArgs& a, bool cand, double mu, bool initScale, bool factorsCommute, int computeUnits,
                     hipStream_t s, double stepRadius = -1.0);
int evalBuildLaunches();   // launches of k_eval_build in this process so far (svin_ba_debug_get_option("SVIN_EVAL_BUILD_LAUNCHES"))
int stepInEvalLaunches();  // post-solve passes launched without their tail so far (svin_ba_debug_get_option("SVIN_STEP_IN_EVAL_LAUNCHES"))
// Whether the step of this window moves from k_post_solve's tail to the head of k_eval_build's blocks (build_plan.hpp stepInEvalTaken)
bool stepInEvalTaken(const DeviceProblem& p, bool sharded, bool buildWanted, bool reuse, bool hostFactors, int computeUnits);

// ---- launch wrappers (kernels.hip).  `cand` selects candidate tables/buffers; `a`: what this launch publishes and defers (a launch
// that sums no cost publishes nothing: PassArgs{}).  launchEvalReproj hands its kernel single fields, none of them the record's.
void launchEvalReproj(const DeviceProblem& p, bool cand, bool robust, hipStream_t s);
void launchEvalFactors(const DeviceProblem& p, const PassArgs& a, bool cand, hipStream_t s, bool sumCost = false);
void launchEvalPrior(const DeviceProblem& p, const PassArgs& a, bool cand, hipStream_t s, bool sumCost = false, int reprojBlocks = -1);
// fused evaluation (small factors + reprojection residuals in one launch, 256 observations per block)
bool canFuseEvaluation(const DeviceProblem& p);   // EvalPlan::fusable
void launchEvalAll(const DeviceProblem& p, const PassArgs& a, bool cand, bool sumCost, hipStream_t s);
int costSummedBy(const DeviceProblem& p);  // 2 = prior evaluation, 1 = factor evaluation, 0 = separate launchCost
void launchBuildNormalEquations(const DeviceProblem& p, double mu, bool initScale, hipStream_t s);
// the same in two halves, so that a landmark-sharded solve can all-reduce [S | gRed | gFull | hC] in between
// sideLane (a one-GPU solve: Window::solve hands one value to every build and to the reduced solve behind it): launches may fork onto
// the side stream of the solver's stream (kernels.hip sideLaneOf).  Wide windows: the build also launches the small factors and the
// speed / bias chain's factorisation and forward substitution (k_factors_only, k_sb_factor, k_sb_forward) there, beside the landmark
// elimination, whose results they do not read, and launchSolveReduced skips them -- build and solve of an iteration must then see the
// same mu / initScale, which is what the trust-region loop does anyway.
void launchAccumulateNormalEquations(const DeviceProblem& p, double mu, bool initScale, hipStream_t s, bool zeroFirst = true, bool sideLane = false);
void launchZeroBuild(const DeviceProblem& p, hipStream_t s);
// Staged upload: the host arrays of a window arrive as ONE block (one DMA from pinned memory); the segment table at
// the head of the block tells this kernel where each array belongs.  Offsets and sizes are multiples of 16 bytes.
struct StageSegment { unsigned long long srcOff, bytes; void* dst; };
constexpr unsigned long long kStageClear = ~0ull;   // srcOff of a segment that clears `bytes` (a multiple of 16) at dst instead of copying
void launchScatterStaged(const void* block, int nSeg, hipStream_t s);
// the reverse for the read-back: up to 8 device arrays gathered into one block (offsets / sizes multiples of 16 bytes,
// sizes rounded up: the sources are over-allocated accordingly)
struct GatherArgs { const void* src[8]; unsigned long long off[8], bytes[8]; int n; };
void launchGatherStaged(void* block, const GatherArgs& a, hipStream_t s);
void launchFinalizeNormalEquations(const DeviceProblem& p, double mu, bool initScale, hipStream_t s);
// Cholesky + GN step of the reduced system; fuseFinalize applies k_finalize_diag (metric + damping) while loading S
// sideLane: as the build in front was told (launchAccumulateNormalEquations)
void launchSolveReduced(const DeviceProblem& p, hipStream_t s, double mu = 0.0, bool initScale = false, bool fuseFinalize = false, bool sideLane = false);
// the blocked route's factorisation alone, at any size; the factor stays in p.cholL at the returned plan's bigM / dinvG / diagF
ReducedSolvePlan launchFactorBlocked(const DeviceProblem& p, hipStream_t s);
// grants a kernel `bytes` of dynamic LDS (hipFuncSetAttribute) once per (device, kernel) and only ever upwards: the attribute
// belongs to the function for the whole process, so the bookkeeping is process-wide and mutex-protected, not per handle
void ensureDynamicLds(const void* fn, size_t bytes);

// a HIP call that is not a launch: its error becomes an exception (every C entry point turns it into its error return)
#define HIP_OK(expr)                                                                                      \
  do {                                                                                                    \
    const hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)

[[noreturn]] void launchFailed(const void* kernel, dim3 grid, dim3 block, size_t ldsBytes, hipError_t e);
// The one way the library launches a kernel: the arguments converted to the kernel's parameter types, dynamic LDS granted when
// the launch asks for any, an empty grid a no-op, and a refused launch an exception.  It reads the status hipLaunchKernel
// returns, not the sticky hipGetLastError(): that one also holds errors of other calls on this thread (RCCL's polling leaves
// hipErrorNotReady behind), and whoever reads it clears it for everyone else.
template <typename... P, typename... A>
void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t ldsBytes, hipStream_t s, A&&... args) {
  if (grid.x == 0 || grid.y == 0 || grid.z == 0) return;
  if (ldsBytes > 0) ensureDynamicLds((const void*)kernel, ldsBytes);
  std::tuple<P...> params(std::forward<A>(args)...);
  const hipError_t e = std::apply([&](P&... a) {
    void* argv[] = {(void*)&a..., nullptr};
    return hipLaunchKernel((const void*)kernel, grid, block, argv, ldsBytes, s);
  }, params);
  if (e != hipSuccess) launchFailed((const void*)kernel, grid, block, ldsBytes, e);
}
// (solveReducedScratchDoubles, the doubles DeviceProblem::cholL must hold: solve_plan.hpp)
// post-solve pass (back-substitution, J*v / J*y sums, norms); fuseRadius > 0: its last block also takes the dogleg
// step with that radius and retracts (single GPU, narrow windows) -- launchDoglegStep is then not needed
// noTail: the blocks store their partials, y_l and v_l and return -- no ticket, no reduction, no step; the launch behind it is
// launchEvalBuild with the same radius as stepRadius
void launchDoglegPrepare(const DeviceProblem& p, const PassArgs& a, hipStream_t s, double fuseRadius = -1.0, bool noTail = false);
void launchDoglegStep(const DeviceProblem& p, double radius, hipStream_t s);  // delta, J*delta pass, candidate, norms
// sharded mode: the (all-reduced) scalars + sequence number into the pinned-host mailbox, as one wave-wide store
void launchPublishScalars(const SolverScalars* scal, ScalarMailbox* mailbox, unsigned long long seq, hipStream_t s);
void launchSetStopVote(SolverScalars* scal, double vote, hipStream_t s);
// sharded mode: [lower triangle of S | gRed | gFull | hC] <-> one contiguous message in p.cholL (packedSystemDoubles long)
size_t packedSystemDoubles(const DeviceProblem& p);
void launchPackSystem(const DeviceProblem& p, bool unpack, hipStream_t s);
void launchCost(const DeviceProblem& p, const PassArgs& a, hipStream_t s);   // sums partial costs into scal->cost
void launchImuPropagation(const DevImu* im /*device*/, const uint32_t* T, const double* M, double* io, double* jac, double* cov,
                          int* used, hipStream_t s);
void launchLandmarkQuality(const DeviceProblem& p, double* quality, hipStream_t s);
// ---- Map::getLhs of every parameter block in one pass (lhs.hip).  Items: (camera-side block, observation range) -- key < nPose a
// pose slot, else extrinsics slot key - nPose; partial[item] gets its 21 upper-triangle sums.  Blocks: one per pose / extrinsics /
// speed-bias block, result at out[out .. out + md * md) (row-major, full); facs: (factor index, first column of the block in the
// factor's FactorLin::J) per small factor touching it.  The landmark blocks go to out[lmOut + 9 l] in CSR order.
struct LhsItem { int key, begin, end, pad; };
struct LhsBlock {
  int out, md;
  int item0, item1;      // its work items [item0, item1) (pose / extrinsics blocks)
  int fac0, fac1;        // its entries of facs
  int priorOrd, priorMd; // its rows of the prior (priorMd 0: not in the prior, or fixed when it was marginalised)
};
void launchLhsAll(const DeviceProblem& p, const LhsItem* items, int nItems, const LhsBlock* blocks, int nBlocks, const int2* facs,
                  double* partial, double* out, size_t lmOut, hipStream_t s);
// ---- marginal covariances (cov.hip; layout of `buf` and launch sizes: cov_plan.hpp planCovariance).  The pass reads what a build
// with mu = 0 left in `p` (S, the Jacobian arrays of the current point) and fills Sigma_cc, every landmark's diagonal block and the
// flags (int 0: bit 1 a landmark block / bit 2 the reduced system is not positive definite; int 1: L - the first such landmark).
// A pair: kind 0 (landmark lm, camera-side or speed / bias block at reduced row `other`, md columns) -> 3 x md; kind 1
// (landmarks lm, other) -> 3 x 3 WITHOUT the delta term; row-major at out[out ..).
struct CovPair { int kind, lm, other, md, out, pad; };
void launchCovariancePass(const DeviceProblem& p, const CovPlan& q, double* buf, hipStream_t s);
void launchCovariancePairs(const DeviceProblem& p, const CovPlan& q, const double* buf, const CovPair* pairs, int nPairs, double* out,
                           hipStream_t s);
// Jacobian-evaluation micro-benchmark entry: B independent copies of the observation set
void launchEvalReprojBatched(const DeviceProblem& p, int copies, double* rOut, double* JpOut, double* JlOut,
                             double* JeOut, hipStream_t s);

}  // namespace svin
