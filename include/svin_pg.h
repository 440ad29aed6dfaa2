/* svin_pg.h -- C ABI of the MI355X-native global pose-graph optimisation.
 *
 * Replaces the numerical core of pose_graph's optimisation thread in AutonomousFieldRoboticsLab/SVIn (paths relative
 * to /root/reference/pose_graph/):
 *   PoseGraph::optimize4DoFPoseGraph   src/pose_graph/PoseGraph.cpp:226-385   (yaw + translation per keyframe)
 *   PoseGraph::optimize6DoFPoseGraph   src/pose_graph/PoseGraph.cpp:387-543   (quaternion + translation)
 * i.e. building the Ceres problem from the keyframe list (sequential edges to the 2 / 4 predecessors of the same
 * sequence, loop edges with HuberLoss(0.1), first keyframe constant), ceres::Solve with SPARSE_NORMAL_CHOLESKY and
 * Levenberg-Marquardt (10 / 5 iterations), and writing the poses back.  Loop detection, BRIEF / DBoW2, the keyframe
 * container and the ROS plumbing stay in pose_graph; they hand keyframes over through svin_pg_add_keyframe.
 *
 * Conventions: opaque handle, externally synchronised (the reference holds kflistMutex_ while it builds the problem);
 * positions 3 doubles, quaternions 4 doubles [x y z w] (Eigen coeffs order); angles in degrees where the reference
 * uses degrees (PoseGraph.h:85-127).  Return 1 = ok, 0 = benign false, <0 = error; nothing throws.  There is no CPU
 * fallback: without a HIP device svin_pg_create() returns NULL.
 */
#ifndef SVIN_PG_H_
#define SVIN_PG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svin_pg svin_pg;

/* six_dof = 0: optimize4DoFPoseGraph, 1: optimize6DoFPoseGraph; max_iterations <= 0: the reference's 10 / 5 */
svin_pg* svin_pg_create(int device, int six_dof, int max_iterations);
void svin_pg_destroy(svin_pg* h);
const char* svin_pg_last_error(void);

/* keyframelist.push_back (PoseGraph.cpp addKeyframe): index, sequence, SVIn pose (Keyframe::getSVInPose);
 * loop_index < 0: no loop; otherwise Keyframe::getLoopRelativeT / getLoopRelativeQ / getLoopRelativeYaw
 * (src/pose_graph/Keyframe.cpp:576-582) */
int svin_pg_add_keyframe(svin_pg* h, int index, int sequence, const double* t, const double* q, int loop_index,
                         const double* loop_rel_t, const double* loop_rel_q, double loop_rel_yaw_deg);
int svin_pg_num_keyframes(const svin_pg* h);

/* ---- caller-given edges (no reference counterpart: pose_graph only knows the edges it builds from the keyframe list)
 *
 * A constraint between any two keyframes of the list: a second loop closure on a keyframe, an edge between two sessions or
 * vehicles, a relocalisation, an edge weighted by a measured covariance.  The measurement is the pose of keyframe b in the frame
 * of keyframe a, exactly as loop_rel_* of svin_pg_add_keyframe: rel_t = R_a^T (t_b - t_a); 6-DoF: rel_q = q_a^-1 q_b and
 * rel_yaw_deg is ignored; 4-DoF: rel_yaw_deg = yaw_b - yaw_a, rel_q may be NULL, pitch and roll are those of a's SVIn pose.
 * index_a / index_b are `index` values of keyframes already in the list (the last keyframe with that index, as for a loop edge);
 * a may come after b in the list and the sequences may differ.
 *
 * Residual.  u is the unit-weight residual of the built-in error terms: 4-DoF [R^T d - rel_t (3, metres), wrap(yaw_b - yaw_a -
 * rel_yaw) (degrees)], 6-DoF [R_a^T d - rel_t, 2 vec(rel_q conj(q_a^-1 q_b))].  r = S u with S = L^T, information = L L^T (the
 * convention of svin_ba_map_add_reprojection_error); information is D x D row-major in the order of u, D = 4 or 6; NULL = the
 * loop-edge weights of that DoF (4-DoF diag(1, 1, 1, 0.1)^2, 6-DoF diag(20, 20, 20, 100, 100, 100)^2).  The loss -- loss_kind one
 * of the numeric values of svin_ba.h's SVIN_LOSS_NONE (0) / SVIN_LOSS_CAUCHY (1) / SVIN_LOSS_HUBER (2), loss_scale = a -- acts on
 * s = |r|^2 with Ceres' corrector; the edge's cost is rho(s) / 2.  NULL information with Huber(0.1) is the built-in loop edge.
 * rel_q is used as given, like loop_rel_q: rel_q and -rel_q are the same rotation but flip the sign of the rotation rows of u.
 * That is without effect under an information that does not couple rotation with translation (the built-in weights); with one
 * that does, hand over the rel_q of the hemisphere of q_a^-1 q_b (their dot product positive).
 *
 * An edge takes part in svin_pg_optimize(earliest, cur), svin_pg_debug_step and svin_pg_get_covariance_blocks when both its
 * keyframes are in the range.  It stands in the edge list at the turn of its later keyframe (list order), after that keyframe's
 * sequential and loop edges, in the order of the add_edge calls.  With one constant end it contributes to the other end's block
 * and to the cost, with two to the cost only.  Pairs of keyframes that carry three or more edges have their block of the normal
 * equations summed in the order of the edge list: results are the same bits from run to run.
 *
 * svin_pg_add_edge returns the edge id (>= 1, never reused within a handle); -1 for a NULL handle, NULL rel_t, NULL rel_q in
 * 6-DoF, index_a == index_b, numbers that are not finite, an unknown loss kind, a loss_scale that is not finite and > 0 (ignored
 * for NONE), an information that is not symmetric (I[i][j] != I[j][i]), not finite or not positive definite (a Cholesky pivot not
 * above D eps of its diagonal entry); -2 for an unknown keyframe index or edge id; svin_pg_last_error() has the text.  A refused
 * call changes nothing.  add_edge and remove_edge drop the kept covariance factor like svin_pg_add_keyframe.  svin_pg_get_edge
 * fills whichever outputs are not NULL; information is the matrix in force (the default weights squared where NULL was given). */
int svin_pg_add_edge(svin_pg* h, int index_a, int index_b, const double* rel_t, const double* rel_q, double rel_yaw_deg,
                     const double* information, int loss_kind, double loss_scale);
int svin_pg_remove_edge(svin_pg* h, int edge_id);
int svin_pg_num_edges(const svin_pg* h);
int svin_pg_get_edge(const svin_pg* h, int edge_id, int* index_a, int* index_b, double* rel_t, double* rel_q,
                     double* rel_yaw_deg, double* information, int* loss_kind, double* loss_scale);

/* ---- absolute keyframe measurements and the gauge (no reference counterpart: pose_graph only knows relative constraints)
 *
 * A prior says where ONE keyframe is: a depth from the pressure sensor, a GPS / USBL fix, a surveyed marker, a full pose.  The
 * measurement is in the frame of the variables the optimisation moves -- the frame svin_pg_get_pose answers in.  kind:
 * SVIN_PG_PRIOR_POSE (m = D rows: t, and q in 6-DoF or yaw_deg in 4-DoF), SVIN_PG_PRIOR_POSITION (m = 3 rows: t),
 * SVIN_PG_PRIOR_DEPTH (m = 1 row: t[2]; t[0], t[1], q and yaw_deg are not read).  q and yaw_deg are only read by POSE (q may be
 * NULL otherwise, and always in 4-DoF); q is a unit quaternion [x y z w], its conjugate is taken for its inverse.
 *
 * Residual.  u follows the order of the edges' u: 4-DoF [t_k - t (metres), wrap(yaw_k - yaw_deg) (degrees)], 6-DoF [t_k - t,
 * 2 vec(q_k q^-1)]; POSITION keeps rows 0..2, DEPTH row 2.  r = S u_sel with S = L^T, information = L L^T: m x m row-major in the
 * order of the kept rows, NULL = identity.  The loss (kinds and scale as for svin_pg_add_edge) acts on s = |r|^2, the prior's cost
 * is rho(s) / 2.  Jacobians in the solver's tangent (4-DoF [yaw, t], 6-DoF [t, dq] with q <- [sin|d| d/|d|, cos|d|] q): identity
 * on t, 1 on yaw, 2 (e_w I - [e_v]x) on dq with e = q_k q^-1.  q is used with the sign given: q and -q are the same rotation but
 * flip the sign of the rotation rows of u.  That is without effect under an information that does not couple rotation with
 * translation; with one that does, hand over the q of the hemisphere of q_k (their dot product positive).
 *
 * `index` resolves to the last keyframe of the list with that index when a problem is built.  A prior joins
 * svin_pg_optimize(earliest, cur), svin_pg_debug_step and svin_pg_get_covariance_blocks when its keyframe is in the range; it
 * stands in the list at its keyframe's turn, after that keyframe's sequential, loop and caller-given edges, in the order of the
 * add_prior calls.  A prior on a constant keyframe adds to the cost only.  A keyframe may be held by priors alone.
 *
 * The gauge.  gauge = 0 (default) keeps the reference's constant keyframes: the first of the range, and in 6-DoF every keyframe of
 * sequence 0.  gauge = 1 holds none constant; the priors then have to tie the graph to the world.  Enough for a connected graph:
 * 6-DoF position on three keyframes that are not collinear, or one POSE; 4-DoF (pitch and roll are not variables) position on two
 * keyframes that differ horizontally, or one POSE.  DEPTH priors alone never are.  With too few, svin_pg_optimize still runs (the
 * Levenberg-Marquardt diagonal makes every system solvable) and svin_pg_get_covariance_blocks answers SVIN_PG_ERR_SINGULAR
 * through its pivot test.  Covariances are relative to whatever ties the graph: the constant keyframes at gauge 0, the priors at
 * gauge 1, where no block is zero.
 *
 * svin_pg_add_prior returns the prior id (>= 1, a space of its own, never reused within a handle); -1 for a NULL handle, an unknown
 * kind, NULL t, NULL q for a 6-DoF POSE, numbers that are not finite, an unknown loss kind, a loss_scale that is not finite and > 0
 * (ignored for NONE), an information that is not symmetric entry by entry, not finite or not positive definite (the pivot rule of
 * svin_pg_add_edge on the m x m matrix); -2 for an unknown keyframe index or prior id; svin_pg_set_gauge -1 for a gauge other than
 * 0 / 1.  A refused call changes nothing.  add_prior, remove_prior and set_gauge drop the kept covariance factor.
 * svin_pg_get_prior fills whichever outputs are not NULL: t (3; zeros where not read), q (4; identity where not read), information
 * m x m (the identity where NULL was given). */
#define SVIN_PG_PRIOR_POSE     0
#define SVIN_PG_PRIOR_POSITION 1
#define SVIN_PG_PRIOR_DEPTH    2
int svin_pg_add_prior(svin_pg* h, int index, int kind, const double* t, const double* q, double yaw_deg,
                      const double* information, int loss_kind, double loss_scale);
int svin_pg_remove_prior(svin_pg* h, int prior_id);
int svin_pg_num_priors(const svin_pg* h);
int svin_pg_get_prior(const svin_pg* h, int prior_id, int* index, int* kind, double* t, double* q, double* yaw_deg,
                      double* information, int* loss_kind, double* loss_scale);
int svin_pg_set_gauge(svin_pg* h, int gauge);   /* 0 = the reference's constant keyframes (default), 1 = free */
int svin_pg_get_gauge(const svin_pg* h);

/* one pass of the optimisation thread's loop body for cur_index (PoseGraph.cpp:236-351 / :397-516): keyframes with
 * index >= earliest_loop_index up to cur_index are optimised, their poses updated in place */
int svin_pg_optimize(svin_pg* h, int earliest_loop_index, int cur_index);

/* Keyframe::getPose (the drift-corrected / optimised pose; the SVIn pose handed in stays the optimisation's input) */
int svin_pg_get_pose(const svin_pg* h, int k, double* t, double* q);
/* the same for the first n keyframes of the list: t = n x 3, q = n x 4 (what updatePath() walks, PoseGraph.cpp:545-) */
int svin_pg_get_poses(const svin_pg* h, int n, double* t, double* q);

/* yaw_drift (degrees), r_drift (3x3 row-major), t_drift after the last optimisation (PoseGraph.cpp:356-363 /
 * :521-526); svin_pg_optimize applies them to the keyframes after cur_index, svin_pg_add_keyframe to new keyframes
 * (PoseGraph.cpp:127-132) */
int svin_pg_get_drift(const svin_pg* h, double* yaw_drift_deg, double* r_drift, double* t_drift);

/* solver layout (no reference counterpart; Ceres picks its own ordering): keyframes per piece (0 = keep, default
 * 32 for 4-DoF / 64 for 6-DoF, at most 256 / tangent size) and the free-keyframe count up to which the whole graph is solved as one dense
 * system (default 128).  svin_pg_get_partition: free keyframes, separator keyframes, pieces, largest piece (rows),
 * Schur tiles, seconds of the host-side symbolic step, separator unknowns, number of dense separator solves and their
 * total seconds (HIP events on the solver's stream) of the last svin_pg_optimize */
int svin_pg_set_partition(svin_pg* h, int piece_keyframes, int dense_keyframes);
/* 1 = eliminate the pieces only; 2 (default) = also eliminate the cut keyframes in level-2 pieces (of
 * level2_piece_keyframes cut keyframes, 0 = keep, default 16 / 32, used as max(8, min(., 256 / tangent size)) like the
 * level-1 length: the level-2 factor kernel's LDS grows with it) so that the dense root only holds the loop cover */
int svin_pg_set_levels(svin_pg* h, int levels, int level2_piece_keyframes);
/* out10: ... as above, [6] = unknowns of the dense root solve, [9] = level-2 pieces */
int svin_pg_get_partition(const svin_pg* h, double* out10);

/* ceres::Solver::Summary of the last solve: initial_cost, final_cost, iterations, termination (0 convergence,
 * 1 no convergence, 3 failure), successful steps, solve seconds (device work, inputs resident) */
int svin_pg_summary(const svin_pg* h, double* out6);

/* ---- marginal covariances of keyframes (ceres::Covariance::GetCovarianceBlockInTangentSpace on the reference's problem)
 *
 * For the local problem svin_pg_optimize(h, earliest_loop_index, cur_index) would build now (same keyframes, edges, constant
 * keyframes, HuberLoss(0.1) corrector), with J the stacked minimal Jacobian (square-root information and loss corrector applied:
 * apply_loss_function = true) at the poses svin_pg_get_pose returns -- the SVIn poses on a fresh handle, the optimised ones after
 * an optimisation; the edge measurements stay what optimize() takes them from -- Sigma = (J^T J)^-1, undamped, in the solver's
 * tangent coordinates: 4-DoF [yaw in degrees, t], 6-DoF [t, dq] with q <- [sin|d| d/|d|, cos|d|] q.  The units are those of the
 * reference's residual weights (sqrt-information 20 / 100 / 57.3 of the 6-DoF edges, unit weights and the 0.1 loop-yaw weight of
 * the 4-DoF edges), not metres and radians of a calibrated sensor model; an edge given with a measured information matrix
 * (svin_pg_add_edge) enters in the units of that matrix.  Covariances are relative to the constant keyframe(s), or at gauge 1 to the priors (svin_pg_set_gauge).
 *
 * The block of (index_a, index_b) -- the `index` values given to svin_pg_add_keyframe -- is Sigma[a, b], D x D row-major, D = 4
 * or 6.  A constant keyframe has exactly zero covariance with everything; Sigma[b, a] is Sigma[a, b]^T bit for bit; two calls
 * return the same bits.  To that end the block of a pair is read off the solve of ONE of its keyframes whoever asks: the one
 * later in the range is the pair's column keyframe.  Column keyframes are solved in batches of B = 8 (D right-hand sides each)
 * pushed through the factorisation the solver builds anyway; asking whole columns is cheap for late keyframes and costs a column
 * keyframe per later row for early ones.
 *
 * Returns: -1 for NULL arguments, n_pairs < 0, cur_index < earliest_loop_index or a capacity too small (nothing is written);
 * -2 for a keyframe outside the range or unknown; -3 for a device error; SVIN_PG_ERR_SINGULAR when J^T J is not positive definite
 * -- a pivot that is not positive or below 1e-12 of its diagonal entry of the Jacobi-scaled J^T J; svin_pg_last_error() then names
 * the keyframe index whose block met the pivot, or "root"; nothing is kept and the handle stays usable.  Nothing is written back:
 * poses, drift, summary and partition record stay as they were.  The factor of the last call is kept and reused until
 * svin_pg_add_keyframe, svin_pg_add_edge, svin_pg_remove_edge, svin_pg_add_prior, svin_pg_remove_prior, svin_pg_set_gauge, svin_pg_optimize, svin_pg_debug_step, svin_pg_set_partition or svin_pg_set_levels is called or another
 * (earliest_loop_index, cur_index) is given. */
#define SVIN_PG_ERR_SINGULAR (-5)
/* n_pairs blocks back to back; cov == NULL only sizes; returns the doubles written (n_pairs * D * D) */
long long svin_pg_get_covariance_blocks(svin_pg* h, int earliest_loop_index, int cur_index, int n_pairs,
                                        const int* index_a, const int* index_b, double* cov, long long cap_doubles);
int svin_pg_get_covariance(svin_pg* h, int earliest_loop_index, int cur_index, int index_a, int index_b,
                           double* cov, int cap);              /* returns D * D */
/* inspection: [0] factorisation passes, [1] substitution passes (batches), [2] distinct column keyframes solved, [3] spare */
int svin_pg_covariance_counters(const svin_pg* h, long long out4[4]);

/* ---- debug (tests/test_gpu_posegraph_stages.py): one Levenberg-Marquardt step kept stage by stage */

/* problem construction, symbolic step, evaluation, node pass (with the Jacobi scales), ONE solve of the damped normal
 * equations at the given trust-region radius, model cost change + candidate, candidate evaluation + final reduction --
 * the launches of svin_pg_optimize's first iteration, run by the same code; nothing is written back, the drift and the
 * keyframes stay untouched.  Returns 1, 0 when there is nothing to optimise, <0 on error. */
int svin_pg_debug_step(svin_pg* h, int earliest_loop_index, int cur_index, double radius);
/* copies the named array of the last svin_pg_debug_step (as doubles; ints converted) and returns its length, -2 for an
 * unknown name; out == NULL just returns the length.  Names: local problem ea eb (eb = ea on a prior) eloop (0 sequential, 1 loop, 2 caller-given, 3 prior) off
 * et eyaw epitch eroll eq esq (ones on caller-given edges) yaw pitch roll t q; ekind (0 sequential, 1 loop, 2 caller, 3 prior) einfo
 * (ne x D x D, the factor S applied, diagonal for the built-in edges, a prior's embedded in the rows it keeps) eloss (ne x 2: kind, scale) eid (edge or prior id, 0 = built-in) eprior (prior kind, -1 on other entries); device res Ja Jb (robustified) g scale colsq nodeBlk (nodes x D x D, lower triangle) y yS
 * cost costC gradmax model step2 x2 cholFail yawC tC qC; partition rows cols rows2 cols2 (per piece of level 1 / 2)
 * sepOff nodePiece nodeRow isCover isRoot l2PieceOf (per node) nS nR nPieces nPieces2 BW BW2 */
long long svin_pg_debug_array(const svin_pg* h, const char* name, double* out, long long cap);

#ifdef __cplusplus
}
#endif
#endif /* SVIN_PG_H_ */
