/*
 * stba.h -- C ABI of the MI355X-native nonlinear-least-squares engine ("slam-tricks bundle
 * adjustment").  This is the drop-in boundary for the one hot path of Unsigned-Long/slam-tricks:
 * the Ceres-driven NLS solve of st17-ceres / st20-g2o / st3-calibration.
 *
 * Plain C: opaque handles, caller-owned buffers, int status codes, no exceptions, no torch or
 * HIP types in any signature (a HIP stream is passed as void*).  Everything FP64.
 * All `double*`/`int*` arguments are HOST pointers unless the name ends in `_dev`.
 *
 * What each entry point replaces in the reference (paths relative to /root/reference):
 *
 *   stba_ba_create / _set_params / _get_params
 *        ceres::Problem construction for the BA factor graph: AddResidualBlock(ProjectFactor,
 *        {SO3, POS, landmark}) + AddParameterBlock(SO3, 4, LieLocalParameterization<SO3d>) +
 *        SetParameterBlockConstant               st20-g2o/src/include/test_ceres.h:109-130
 *        (same factor with constant landmarks = the PnP problems of
 *                                                st17-ceres/src/include/solver.hpp:247-385)
 *   stba_ba_evaluate      CostFunction::Evaluate over all residual blocks: residuals + Jacobians
 *                         test_ceres.h:63-80 (ProjectFactor), solver.hpp:168-212 (analytic form,
 *                         with the hat(pInC) rotation block -- SURVEY.md header fact 2),
 *                         composed with LieLocalParameterization::ComputeJacobian solver.hpp:48-54
 *   stba_ba_normal_blocks block-sparse J^T J / J^T r      solver.hpp:402-436 (H += J^T J, g += -J^T r),
 *                         block structure sim_data.h:108-159
 *   stba_ba_reduced_system / stba_ba_solve_reduced / stba_ba_back_substitute
 *                         options.linear_solver_type = SPARSE_SCHUR   test_ceres.h:145
 *                         (g2o: BlockSolver<6,3> + setMarginalized    test_g2o.h:95-100,121)
 *   stba_ba_apply_step    LieLocalParameterization::Plus solver.hpp:38-45 / oplusImpl test_g2o.h:36-39,60-63
 *   stba_ba_solve         ceres::Solve(options, &problem, &summary)   test_ceres.h:148, solver.hpp:286
 *   stba_ba_lm_iterations fixed-work LM iterations (bench mode; no reference counterpart)
 *   stba_ba_triangulate   per-landmark Triangulation solves           sim_data.cpp:299-311
 *   stba_dense_*          the small dense problems: DENSE_QR path     solver.hpp:282, ceres_bound.cpp:40
 *   stba_cholesky_*       dense SPD factor/solve used on the reduced camera system
 *                         (hMat.ldlt().solve(gMat) solver.hpp:438; calib.cpp:393)
 */
#ifndef STBA_H
#define STBA_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STBA_VERSION 6

/* status codes */
enum {
    STBA_OK = 0,
    STBA_ERR_INVALID_ARGUMENT = -1,
    STBA_ERR_NO_DEVICE = -2,       /* no HIP device / runtime failure: the product has no CPU fallback */
    STBA_ERR_HIP = -3,
    STBA_ERR_NOT_POSITIVE_DEFINITE = -4,
    STBA_ERR_ALLOC = -5,
    STBA_ERR_STATE = -6,
    STBA_ERR_CALLBACK = -7,
    STBA_ERR_NO_SOLUTION = -8      /* a closed-form initialiser found no (unique) solution */
};

const char* stba_status_string(int status);
const char* stba_last_error(void);      /* thread-local detail of the last failure */
int stba_version(void);                 /* 6: stba_pcg_options grew coarse_async, forcing_step_accuracy (append-only); 5: stba_lm_options grew function_tolerance_takes_step */
/* number of visible HIP devices (0 => every compute entry point returns STBA_ERR_NO_DEVICE) */
int stba_device_count(void);
/* device buffers the library's engines, stores and calls hold at this moment, process-wide (a count of allocations, not bytes).
 * An engine's buffers go with stba_*_destroy, a call's temporaries when it returns: the count is then what it was before.  Not
 * counted: the dense Cholesky's per-stream workspaces and the small dense step's pooled buffers, which live as long as the process */
int stba_live_device_buffers(long long* count);

/* ---- Levenberg-Marquardt options: the fields the reference sets plus Ceres' defaults --------
 * (solver.hpp:272-282, test_ceres.h:133-146; defaults: SURVEY.md 8c) */
typedef struct {
    int    max_num_iterations;            /* 50 */
    double initial_trust_region_radius;   /* 1e4 */
    double max_trust_region_radius;       /* 1e16 */
    double min_trust_region_radius;       /* 1e-32 */
    double min_relative_decrease;         /* 1e-3 */
    double min_lm_diagonal;               /* 1e-6 */
    double max_lm_diagonal;               /* 1e32 */
    double function_tolerance;            /* 1e-6 */
    double gradient_tolerance;            /* 1e-10 */
    double parameter_tolerance;           /* 1e-8 */
    int    jacobi_scaling;                /* 1 */
    int    num_threads;                   /* accepted and ignored (reference sets 1) */
    int    minimizer_progress_to_stdout;  /* solver.hpp:278 */
    int    update_state_every_iteration;  /* solver.hpp:277: copy parameters back before callbacks */
    int    phase_timing;                  /* 0 (default): no per-phase device times.  1: hipEvents between the phases of every
                                           * iteration fill stba_lm_summary::ms_* -- an event is a packet of its own on the queue
                                           * and costs ~5 us of idle GPU, ~1.5 % of a C5 iteration for the eight it takes */
    int    function_tolerance_takes_step; /* what happens to the trial step on which |cost change| <= function_tolerance * cost fires:
                                           * 1 (default): it is taken if it is a decrease (rho > min_relative_decrease), THEN convergence
                                           *    is reported;
                                           * 0: convergence is reported at once and the step is NOT taken -- the order of Ceres'
                                           *    TrustRegionMinimizer::Minimize since the refactoring of 1.12 (through 2.1):
                                           *    ComputeCandidatePointAndEvaluateCost(); if (ParameterToleranceReached()) return;
                                           *    if (FunctionToleranceReached()) return; if (IsStepSuccessful()) HandleSuccessfulStep();
                                           *    -- the candidate becomes the state only in HandleSuccessfulStep.
                                           * So 0 is Ceres' stopping state.  1 stays the default because the step that is given up is a
                                           * full Newton step of a converged model and not a small one: on the C4 pose graph it still moves
                                           * poses by 3.6e-3 (cost by < 1e-6 relative), and it is what brings a run with inexact steps back
                                           * onto the exact-step trajectory -- measured in round 6 (profiles/r6_c4_async.txt): production
                                           * against exact steps, poses 2.5e-6 apart with the step, 5.7e-5 without (north_star asks for
                                           * 1e-5).  Taking it can only lower the final cost.  Engine and oracle (orc_lm_options) carry the
                                           * same switch and agree under both settings; a caller who wants Ceres' own final state sets 0.
                                           * (No Ceres exists in this image to run against; tools/ceres_baseline.cpp on a box that has
                                           * one shows the order in num_successful_steps.) */
} stba_lm_options;

void stba_lm_default_options(stba_lm_options* opt);

/* STBA_FAILURE: the START point could not be evaluated -- a non-finite cost, i.e. a non-finite input or residual (Ceres: "Initial
 * residual and Jacobian evaluation failed"; reason STBA_TERM_SOLVER_FAIL, zero iterations, parameters untouched) -- or a callback
 * failed.  A non-finite cost at a TRIAL point is an unsuccessful step, as in Ceres: rejected, the radius shrinks, the solve goes on. */
enum { STBA_CONVERGENCE = 0, STBA_NO_CONVERGENCE = 1, STBA_FAILURE = 2 };
enum { STBA_TERM_NONE = 0, STBA_TERM_GRADIENT = 1, STBA_TERM_FUNCTION = 2, STBA_TERM_PARAMETER = 3,
       STBA_TERM_MAX_ITER = 4, STBA_TERM_MIN_RADIUS = 5, STBA_TERM_SOLVER_FAIL = 6,
       STBA_TERM_FIXED = 7, STBA_TERM_USER = 8 };

typedef struct {
    int    termination_type;
    int    termination_reason;
    int    num_iterations;
    int    num_successful_steps;
    int    num_unsuccessful_steps;
    double initial_cost;
    double final_cost;
    double final_radius;
    double final_gradient_max_norm;
    double seconds_total;
    /* device time per phase, milliseconds, summed over iterations (hipEvent); zero unless stba_lm_options::phase_timing.
     * ms_backsub: back-substitution + the manifold update to the trial point (one kernel); ms_cost: evaluation of the trial
     * point -- when the loop speculates (no callback, no progress output) that is the FULL linearisation at the trial point,
     * and ms_linearize then holds only the landmark blocks behind it */
    double ms_linearize, ms_schur, ms_solve, ms_backsub, ms_cost;
    /* several ranks: the cross-rank sums of the reduced camera system of this run -- device time between
     * events around the collective (part of ms_schur), bytes handed to it per rank, number of calls; 0 on one rank */
    double ms_allreduce, allreduce_bytes;
    int    allreduce_calls;
} stba_lm_summary;

/* iteration trace row: cost, cost_change, gradient_max_norm, step_norm, relative_decrease,
 * radius, accepted */
#define STBA_TRACE_COLS 7

/* IterationCallback (solver.hpp:215-245, test_ceres.h:83-96): return 0 to continue */
typedef int (*stba_iteration_callback)(void* user, int iteration, double cost, double cost_change,
                                       double gradient_max_norm, double step_norm, double radius,
                                       int step_is_successful);

/* cross-rank sum of `count` doubles resident on the device, enqueued on `hip_stream`
 * (landmark sharding, SURVEY.md 8e: RCCL all-reduce of the reduced camera system).  Return 0. */
typedef int (*stba_allreduce_fn)(void* user, void* buf_dev, size_t count, void* hip_stream);

/* ================================ native RCCL communicator ================================
 * One process per GPU.  What a C++ host of the reference (st20-g2o/src/src/test_ceres.cpp:7-19)
 * uses instead of a Python hook: rank 0 makes the id, hands it to the other ranks over its own side channel,
 * every rank creates its communicator and gives it to the engines (stba_ba_set_comm / stba_pg_set_comm), which
 * then call ncclAllReduce(buf, buf, count, ncclDouble, ncclSum, comm, stream) on THEIR stream.  RCCL is bound
 * lazily (dlopen): hosts that never create a communicator need no librccl.
 * device < 0: the calling thread's current device. */
#define STBA_COMM_ID_BYTES 128
typedef struct stba_comm stba_comm;
int stba_comm_unique_id(char id[STBA_COMM_ID_BYTES]);
int stba_comm_create(stba_comm** out, const char id[STBA_COMM_ID_BYTES], int rank, int world_size, int device);
int stba_comm_destroy(stba_comm* comm);
int stba_comm_rank(const stba_comm* comm, int* rank, int* world_size);
/* in-place sum of `count` doubles on the device across all ranks, enqueued on hip_stream */
int stba_comm_allreduce_sum(stba_comm* comm, void* buf_dev, size_t count, void* hip_stream);
/* the same as an stba_allreduce_fn (user = stba_comm*) */
int stba_comm_allreduce_hook(void* user, void* buf_dev, size_t count, void* hip_stream);

/* ================================ bundle-adjustment engine ================================ */
typedef struct stba_ba stba_ba;

/* cams: n_cams*7 (qx qy qz qw tx ty tz, camera-to-world); pts: n_pts*3; observations in any
 * order (the engine regroups them landmark-major); obs_feat: n_obs*2 normalised image coords.
 * cam_fixed: n_cams*6 bytes (1 = dof constant; NULL = all free; order [rot(3), pos(3)]);
 * pt_fixed: n_pts bytes (1 = landmark constant; NULL = all free).
 * hip_stream: hipStream_t to enqueue on (NULL = the engine creates its own).
 * The Schur complement has two forms (stba_ba_set_schur_mode).  PAIRS: a plan with one 16-byte record per PAIR of observations
 * of the same landmark (sum over landmarks of k (k + 1) / 2, k = cameras seeing it; 5.5 M at 1000 cameras x 100 000 landmarks x
 * 10 observations each), built once here, on the host and on the device; one 6 x 6 block accumulated in LDS per pair.  DENSE: the
 * scaled camera-landmark blocks in a dense [6 n_cams] x [3 n_pts] matrix Y and S = -(Y Y^T) as ONE symmetric rank-k product on the
 * matrix cores -- no plan, 8 x 18 n_cams n_pts bytes of device memory, the right form when most cameras see most landmarks.
 * The engine picks DENSE by itself when the plan would have more than 2^30 pairs (or would not fit half of the free device
 * memory), or more than 2^20 pairs at a visibility of 30 % and more; a problem that fits neither form is refused with
 * STBA_ERR_INVALID_ARGUMENT. */
int stba_ba_create(stba_ba** out, int n_cams, int n_pts, int n_obs, const double* cams,
                   const double* pts, const int* obs_cam, const int* obs_pt, const double* obs_feat,
                   const unsigned char* cam_fixed, const unsigned char* pt_fixed, void* hip_stream);
int stba_ba_destroy(stba_ba* ba);
/* form of the Schur complement (above): STBA_SCHUR_AUTO = what stba_ba_create chose.  STBA_SCHUR_PAIRS fails if the engine was
 * created without a pair plan (too many pairs), STBA_SCHUR_DENSE if Y does not fit the device. */
enum { STBA_SCHUR_AUTO = 0, STBA_SCHUR_PAIRS = 1, STBA_SCHUR_DENSE = 2 };
int stba_ba_set_schur_mode(stba_ba* ba, int mode);
int stba_ba_schur_mode(const stba_ba* ba, int* mode);
int stba_ba_set_params(stba_ba* ba, const double* cams, const double* pts);
int stba_ba_get_params(stba_ba* ba, double* cams, double* pts);
/* (round 6) the observations' features again, n_obs*2 in the order given to stba_ba_create: for a caller who learns them while the engine
 * is being created -- include/stba/ceres.h creates the engine (regrouping, Schur plan, uploads: ~50 ms at 10^6 observations) on a helper
 * thread while the calling thread evaluates the user's cost functions for their features, then hands them over here. */
int stba_ba_set_features(stba_ba* ba, const double* obs_feat);
/* the HIP device of the CALLING thread (a helper thread starts on device 0 whatever its parent had selected): read it on one thread,
 * set it on the other */
int stba_get_device(int* device);
int stba_set_device(int device);
/* BA-SHAPED problems whose factor is NOT the built-in reprojection (the reference's BA cost is a generic
 * DynamicAutoDiffCostFunction, test_ceres.h:56,109-121: a robustified, scaled or otherwise different 4+3+3 -> 2 factor must not
 * fall back to dense normal equations).  With a host lineariser the residuals and Jacobians of every observation come from the
 * caller -- the C++ shim evaluates the user's cost functions in bulk -- and everything behind them runs on the device
 * unchanged: landmark blocks, Schur complement, dense factorisation, back-substitution, manifold update, LM control.
 *   fn(user, cams[n_cams*7], pts[n_pts*3], r[n_obs*2], Jc, Jp) -> 0 on success
 * in the CALLER's observation order (the order given to stba_ba_create; obs_feat is not used in this mode);
 * Jc[n_obs*12]: 2x6 row-major w.r.t. the camera's LOCAL coordinates [dtheta(3) of q <- q (x) exp(dtheta), dt(3)];
 * Jp[n_obs*6]: 2x3 w.r.t. the landmark; Jc = Jp = NULL when only the cost of a trial point is wanted.
 * The callback runs on the calling thread, between kernels: the LM loop does not overlap host and device work in this mode. */
typedef int (*stba_ba_linearize_fn)(void* user, const double* cams, const double* pts, double* r, double* Jc, double* Jp);
int stba_ba_set_host_linearizer(stba_ba* ba, stba_ba_linearize_fn fn, void* user);
/* multi-GPU: this engine holds one landmark shard; all cameras are replicated.  The hook sums
 * the packed reduced system / scalars across ranks.  rank 0 owns the once-only diagonal terms. */
int stba_ba_set_allreduce(stba_ba* ba, stba_allreduce_fn fn, void* user, int rank, int world_size);
/* the same with a native communicator (NULL: back to a single rank) */
int stba_ba_set_comm(stba_ba* ba, stba_comm* comm);
/* padded order of the dense reduced system (multiple of the factorisation block) */
int stba_ba_reduced_dim(const stba_ba* ba, int* n, int* n_padded);

/* --- stage entry points (each runs the HIP kernels and optionally copies results out) ------ */
/* residuals r[n_obs*2], Jc[n_obs*12] (2x6 row-major), Jp[n_obs*6] (2x3), in the caller's
 * observation order; any output may be NULL.  cost = 1/2 sum r^2. */
int stba_ba_evaluate(stba_ba* ba, double* cost, double* r, double* Jc, double* Jp);
/* cost only (residual kernel without Jacobians), at the current parameters */
int stba_ba_cost(stba_ba* ba, double* cost);
/* needs a preceding stba_ba_evaluate.  Hcc[n_cams*36], gc[n_cams*6], Hpp[n_pts*9], gp[n_pts*3] */
int stba_ba_normal_blocks(stba_ba* ba, double* Hcc, double* gc, double* Hpp, double* gp);
/* needs normal blocks.  dc[n_cams*6], dp[n_pts*3]: diagonal damping.  S: n*n row-major with
 * n = 6*n_cams (lower triangle valid), rhs[n].  S/rhs may be NULL (device-only). */
int stba_ba_reduced_system(stba_ba* ba, const double* dc, const double* dp, double* S, double* rhs);
/* Cholesky + solve of the reduced system on the device: dxc[n_cams*6] */
int stba_ba_solve_reduced(stba_ba* ba, double* dxc);
/* dxp[n_pts*3] from the camera step currently on the device */
int stba_ba_back_substitute(stba_ba* ba, double* dxp);
/* trial point = current (+) step on the device; returns its cost; accept != 0 keeps it */
int stba_ba_apply_step(stba_ba* ba, int accept, double* new_cost);

/* --- whole solves ------------------------------------------------------------------------ */
/* trace: (max_num_iterations+1)*STBA_TRACE_COLS doubles or NULL */
int stba_ba_solve(stba_ba* ba, const stba_lm_options* opt, stba_lm_summary* summary, double* trace,
                  stba_iteration_callback cb, void* cb_user);
/* exactly `iterations` LM iterations, each re-linearising, solving and evaluating the trial
 * point; no convergence tests.  The unit of work bench.py times.  Parameters stay on the device. */
int stba_ba_lm_iterations(stba_ba* ba, const stba_lm_options* opt, int iterations,
                          stba_lm_summary* summary, double* trace);
/* per-landmark refinement with cameras fixed (sim_data.cpp:299-311) */
int stba_ba_triangulate(stba_ba* ba, int max_iter);

/* average device time (ms) of the residual+Jacobian kernel over `reps` back-to-back launches,
 * measured with hipEvents on the engine's stream (bench.py roofline leg). */
int stba_ba_time_linearize(stba_ba* ba, int reps, double* ms_avg);
/* the same for the Schur-complement kernel (linearises at the current point first); also hands back the number of LDS
 * FP64 atomics and of observation pairs of one launch (either may be NULL) */
int stba_ba_time_schur(stba_ba* ba, int reps, double* ms_avg, double* lds_atomics_per_launch, double* pairs_per_launch);

/* --- covariance (ceres::Covariance) ------------------------------------------------------- */
/* C = (J^T J)^-1 of the UNDAMPED, unscaled problem at the current parameters (not multiplied by a residual variance, as in Ceres),
 * in the engine's tangent coordinates: per camera [dtheta(3) of q <- q (x) exp(dtheta), dt(3)], per landmark its 3 coordinates.
 * Constant dofs (cam_fixed) and constant landmarks (pt_fixed) have zero rows and columns in every block.
 * stba_ba_covariance_compute re-linearises (through the host lineariser if one is set), builds the undamped reduced camera system S
 * = U - E V^-1 E^T (the explicit-damping path of stba_ba_reduced_system with zero damping, either Schur form) and inverts it on the
 * device; Sigma_cc = S^-1 (lower triangle, packed) and every V_j^-1 stay on the device until the next compute,
 * stba_ba_covariance_release or stba_ba_destroy.  It needs 4 np^2 doubles for the length of the call (np: 6 n_cams rounded up to
 * 128; 1.16 GB at 1000 cameras) and n (n + 1) / 2 afterwards.  The LM state is left as it was: a later stba_ba_solve is
 * bit-identical to one without this call.
 * rank test: rcond = smallest / largest Cholesky pivot, once for S (over the free dofs) and for every free landmark's V_j.  If any is
 * below min_rcond (Ceres' min_reciprocal_condition_number, 1e-14) the call fails with STBA_ERR_NOT_POSITIVE_DEFINITE and
 * stba_last_error() names S, or how many landmarks failed and the first.  This pivot ratio is a cheap test, NOT a condition number
 * estimate; fixing the gauge is the caller's job (see DESIGN.md for what it does on a gauge-free scene).  *rcond_out (may be NULL):
 * the smallest ratio found.  With an all-reduce hook or communicator set (several ranks): STBA_ERR_STATE. */
int stba_ba_covariance_compute(stba_ba* ba, double min_rcond, double* rcond_out);
/* out[n_pairs*36]: the 6x6 block Sigma_cc[cam_a[k], cam_b[k]] row-major per pair (b < a: the transpose of the stored block) */
int stba_ba_camera_covariance(stba_ba* ba, int n_pairs, const int* cam_a, const int* cam_b, double* out);
/* out[n*9]: the 3x3 marginal covariance of landmarks pts[0..n) (pts = NULL: all n_pts landmarks in order, n = n_pts):
 * V_j^-1 + sum over pairs of its observations F_a^T Sigma_cc[a, b] F_b, F_a = E_{a,j} V_j^-1 (covariance.hip) */
int stba_ba_point_covariance(stba_ba* ba, int n, const int* pts, double* out);
/* The off-diagonal blocks of the full inverse, from what the compute left on the device (nothing more is inverted; F_i = Jc_i^T Jp_i
 * V_j^-1 per observation i of landmark j, sums over observations):
 *   Sigma[a, j] = - sum_{i in obs(j)} Sigma_cc[a, cam(i)] F_i,   Sigma[j, k] = sum_{x in obs(j), y in obs(k)} F_x^T Sigma_cc[cam(x), cam(y)] F_y  (j != k)
 * Both need a preceding stba_ba_covariance_compute (STBA_ERR_STATE otherwise).  An index out of range, or a null array with
 * n_pairs > 0: STBA_ERR_INVALID_ARGUMENT (stba_last_error() names the position), nothing written.  n_pairs == 0: STBA_OK.  Constant
 * dofs and constant landmarks give zero rows and columns.  Sigma[k, j] is bitwise the transpose of Sigma[j, k].  STBA_VERSION is
 * unchanged: test for the symbols. */
/* out[n_pairs*18]: the 6 x 3 row-major block Sigma[cam[k], pt[k]] (rows [dtheta(3), dt(3)], columns the landmark's coordinates) */
int stba_ba_camera_point_covariance(stba_ba* ba, int n_pairs, const int* cam, const int* pt, double* out);
/* out[n_pairs*9]: the 3 x 3 row-major block Sigma[pt_a[k], pt_b[k]]; pt_a == pt_b gives the marginal of stba_ba_point_covariance, bit for bit */
int stba_ba_point_pair_covariance(stba_ba* ba, int n_pairs, const int* pt_a, const int* pt_b, double* out);
int stba_ba_covariance_release(stba_ba* ba);

/* ================================ dense SPD solver ======================================== */
/* A: n*n row-major SPD (lower triangle read), overwritten by L (lower).  Runs the blocked MFMA
 * Cholesky on the device.  Returns STBA_ERR_NOT_POSITIVE_DEFINITE if a pivot fails. */
int stba_cholesky_factor(double* A, int n, void* hip_stream);
/* solves A x = b for one right-hand side: b overwritten by x */
int stba_cholesky_solve(const double* A, int n, double* b, void* hip_stream);
/* Ainv[n*n] (row-major, exactly symmetric) = A^-1 of the SPD matrix A (n*n row-major, lower triangle read), n <= 4096, by the
 * routine behind every covariance (stba_ba_covariance_compute, stba_dense_covariance) and the pose graph's coarse operator: a
 * partial factorisation of [A .; I 0] that leaves -A^-1 in the lower right block -- not the factor-and-solve program of the two
 * calls above.  pivot_ratio (may be NULL): smallest / largest Cholesky pivot l_ii^2, the stand-in for a reciprocal condition number
 * that the covariance calls compare with min_rcond.  A failed pivot: STBA_ERR_NOT_POSITIVE_DEFINITE, stba_last_error() names it as
 * "pivot k+1" (LAPACK's info), and neither output is written.  STBA_VERSION is unchanged: test for the symbol. */
int stba_cholesky_inverse(const double* A, int n, double* Ainv, double* pivot_ratio, void* hip_stream);
/* device-resident timing of factor+solve on an n x n synthetic SPD system, ms per solve */
int stba_cholesky_time(int n, int reps, double* ms_avg, void* hip_stream);

/* the same, split by a hipEvent between the factorisation (one persistent kernel, chol_mega_kernel) and
 * the backward substitution: bench.py's MFMA roofline leg divides the n^3/3 flops by ms_factor. */
int stba_cholesky_time_split(int n, int reps, double* ms_factor, double* ms_backward, void* hip_stream);

/* diagnostic, runs on the host (no GPU): the makespan in microseconds that the host-side scheduling model
 * predicts for the persistent factorisation kernel of an n x n system on `n_xcd` XCDs with `wg_per_xcd`
 * workgroups each (MI355X: 8 x 32).  The ticket order of the kernel comes from this model. */
int stba_cholesky_schedule_model(int n, int n_xcd, int wg_per_xcd, double* makespan_us);
/* how often, in this process, the persistent factorisation gave up waiting for a dependency (its workgroups were not all
 * resident: the device is shared with another process) and the stage kernels -- one launch per stage and panel, nothing
 * resident -- took over */
int stba_cholesky_timeout_count(void);
/* how long a workgroup of the persistent factorisation waits for a dependency before the program gives up (microseconds;
 * 0 restores the automatic bound, max(100 ms, 40 x the predicted makespan)).  Process-wide. */
int stba_cholesky_set_timeout_us(double us);

/* design study, runs on the host (no GPU): the same task graph spread over `n_gpus` GPUs (the reduced
 * camera system as the next thing to shard).  Tile rows are dealt to the GPUs block-cyclically, `rows_per_group`
 * consecutive 128-row tile rows at a time (0: one per XCD, i.e. n_xcd rows); a task runs on the GPU that owns the tile
 * row it writes; a dependency that crosses GPUs costs `hop_us` (flag over xGMI) plus the transfer of one 128 x 128
 * FP64 tile (128 KiB) at `link_gb_per_s`.  Link contention is NOT modelled; remote_tiles_busiest_gpu (x 128 KiB) is
 * the ingress volume to hold against the aggregate xGMI bandwidth.  DESIGN.md tabulates it for 1/2/4/8 GPUs.
 * stba_cholesky_shard_owner returns the distribution (tile row -> GPU) the model uses. */
int stba_cholesky_shard_model(int n, int n_gpus, int n_xcd, int wg_per_xcd, int rows_per_group, double hop_us, double link_gb_per_s,
                              double* makespan_us, double* cross_gpu_dependencies, double* remote_tiles_busiest_gpu);
int stba_cholesky_shard_owner(int n_block_rows, int n_gpus, int rows_per_group, int* owner_gpu);

/* hipEvent time (ms) of one factor+solve per kernel class, with the stage-per-kernel schedule (a
 * diagnostic: the production path runs the stages as tasks of one persistent kernel): ms4 = {diagonal blocks, panel solves,
 * MFMA trailing updates, backward substitution}; algorithmic / executed flops of the trailing
 * updates and their launch count (bench.py MFMA roofline leg). */
int stba_cholesky_profile(int n, double* ms4, double* syrk_flops, double* syrk_flops_padded,
                          int* syrk_launches, void* hip_stream);

/* ================================ two-view initialiser ====================== */
/* st22-two-view/src/src/two_view_geometry.cpp:18-126 (FindFunctionalMatrix): fundamental matrix from n >= 8
 * pixel correspondences (x1^T F x2 = 0, no normalisation), essential matrix with K, the four (R, t)
 * hypotheses, the cheirality test over ALL points, DLT triangulation.  f1, f2: n*2 pixels; K: 3x3
 * row-major.  Out: F (9, row-major, unit norm, sign free; may be NULL), R (9) and t (3, unit norm): the
 * pose of frame 2 in frame 1 (p1 = R p2 + t), pts (n*3 landmarks in frame 1, for the UNIT baseline; may be
 * NULL), fails (4 counters of points failing the test per hypothesis; their order follows :61-64 but depends
 * on the sign conventions of the 3x3 SVD; may be NULL).
 * Returns STBA_ERR_NO_SOLUTION if not exactly one hypothesis passes (the reference returns an empty
 * optional).  Device: the n x 9 system is reduced to its triangular factor with Givens rotations, the
 * cheirality test and the triangulation run one correspondence per lane. */
int stba_two_view_init(int n, const double* f1, const double* f2, const double* K, double* F_out, double* R_out,
                       double* t_out, double* pts_out, int* fails_out, void* hip_stream);

/* ================================ trajectories ============================== */
/* Odometry files, st16-pcl-viewer/src/src/scene.cpp:66-110: "format ascii 1.0", "element odometryInfo N",
 * property lines, "end_header", then N lines "timeStamp qx qy qz qw x y z" (quaternion normalised on read,
 * translation parsed through float like the reference's std::stof).  poses: N*7 (qx qy qz qw x y z), the
 * layout of stba_pg_create; pass stamps = poses = NULL to query N. */
int stba_odometry_read(const char* path, int* n_poses, double* stamps, double* poses, int capacity);
int stba_odometry_write(const char* path, int n_poses, const double* stamps, const double* poses);
/* absolute trajectory error, st4-kalman/src/src/pose_simulation.cpp:198-209:
 * sqrt(mean |log(T_truth^-1 T_estimate)|^2), 6-vector SE3 logarithm */
int stba_trajectory_ate(int n_poses, const double* truth, const double* estimate, double* ate);

/* ================================ calibration data formats ================== */
/* Chessboard corner files, st3-calibration/src/src/cbcorner.cpp:34-73: header "rows,cols", then one
 * "i,j,x,y" line per corner (x, y parsed through float like the reference's std::stof; written with
 * 3 decimals).  xy: rows*cols*2 doubles, row-major by (i, j); pass xy = NULL to query the size. */
int stba_corners_read(const char* path, int* rows, int* cols, double* xy, int capacity);
int stba_corners_write(const char* path, int rows, int cols, const double* xy);
/* Zhang's closed-form start point of the refinement (st3-calibration/src/src/calib.cpp:55-173):
 * DLT homographies -> intrinsics (zero skew) -> per-view extrinsics.  obj / img: [V*C*2] board points
 * (X, Y) / pixels; params out: [alpha beta u0 v0 0 0 0 0 0 | xi_0(6) ..] in stba_calib_* layout;
 * homographies out (may be NULL): V*9 row-major, unit Frobenius norm, sign as the null vector came out. */
int stba_zhang_init(int n_views, int n_corners, const double* obj, const double* img, double* params,
                    double* homographies);

/* ================================ Zhang calibration (st3-calibration) ==================== */
/* CalibSolver::totalOptimization's residual / Jacobian blocks (st3-calibration/src/src/calib.cpp:311-391,
 * distortNormPt :254-262, normPt2ImgPt :247-252) evaluated by a HIP kernel, one corner per lane.
 * params: [alpha beta u0 v0 k1 k2 k3 p1 p2 | xi_0(6) .. xi_{V-1}(6)], xi = se3 log [rho, theta];
 * obj / img: [V*C*2] board points (X, Y) / measured pixels.  Outputs (any may be NULL):
 * sse = sum e^2, e[V*C*2], Ji[V*C*18] (2x9 intrinsics+distortion), Jx[V*C*12] (2x6 left pose perturbation). */
int stba_calib_evaluate(int n_views, int n_corners, const double* params, const double* obj, const double* img,
                        double* sse, double* e, double* Ji, double* Jx);
/* totalOptimization (calib.cpp:282-422): plain Gauss-Newton, <= max_iter iterations, stop when
 * |update| < 1e-8; additive update of the 9 shared parameters, left-multiplicative SE3 update of
 * every view.  params in/out; sse_trace[max_iter] receives sum e^2 at the start of each iteration. */
int stba_calib_gauss_newton(int n_views, int n_corners, double* params, const double* obj, const double* img,
                            int max_iter, double* sse_trace, int* iterations);

/* ================================ pose graph (BASELINE config C4) ======================== */
/* BUILD-DEFINED: the reference has no pose-graph code (SURVEY.md header fact 3).  Conventions from the
 * reference's Lie-group notes (st23-lie-group-v2/doc.tex:862-996): node pose T = (qx qy qz qw tx ty tz),
 * right-multiplicative update T <- T exp(delta), tangent [rho, theta]; edge measurement Z_ij ~ T_i^-1 T_j;
 * residual r_ij = log(Z_ij^-1 T_i^-1 T_j).  Levenberg-Marquardt; the damped normal equations are solved matrix-free by
 * conjugate gradients with a two-level preconditioner (6x6 block Jacobi + a coarse space of six rigid-body modes per group
 * of consecutive nodes, inverted densely) as an INEXACT Newton step: the PCG stops at |r| <= eta_k |g|, decided on the
 * device; eta_k follows Eisenstat & Walker's forcing sequence (eta_0 = forcing_eta0, tightening as the gradient falls). */
typedef struct stba_pg stba_pg;
typedef struct {
    int    max_iterations;       /* 1000: cap on the PCG iterations of one linear solve (stba_pcg_summary::hit_cap counts the solves that reach it) */
    double relative_tolerance;   /* 1e-12 on |residual| / |rhs|: used when forcing_eta0 <= 0 (a fixed tolerance, i.e. exact steps) */
    int    check_every;          /* 4: PCG iterations enqueued between the host's looks at the device-side convergence flag */
    double forcing_eta0;         /* 0.1: first and largest forcing term; <= 0: fixed relative_tolerance */
    double forcing_eta_min;      /* 0.01 (round 6; 1e-10 until then): the floor of the forcing sequence.  Eisenstat & Walker's sequence
                                  * falls quadratically near the solution and buys nothing there: the LM loop stops on its function
                                  * tolerance, not on the linear residual.  Measured (floor: PCG iterations | converged poses from the
                                  * exact-step run, north_star's gate 1e-5) -- C4: 1e-10: 217 | 2.9e-6, 0.01: 196 | 3.2e-6 (1444 -> 1505 LM
                                  * it/s), 0.03: 168 | 3.5e-6, 0.1 (a constant eta, Ceres' default for inexact steps): 125 | 7.4e-6; but on
                                  * a 400-node graph with twice the noise 6.8e-6 | 6.6e-6 | 1.1e-5 | 8.3e-6 and on 2000 nodes with three
                                  * times the noise 1.0e-5 | 1.1e-5 | 2.6e-5 | 4.6e-5: 0.01 is the largest floor that leaves the answers
                                  * where the sequence alone puts them (profiles/r6_pg_forcing_floor.txt, r6_c4_forcing.txt) */
    int    coarse_group;         /* nodes per group of the coarse space, a power of two; 0: automatic (<= 200 groups, >= 8 nodes);
                                  * -1: no coarse space (block Jacobi only, the round-3 preconditioner) */
    int    coarse_refresh_every; /* 1: LM iterations between re-inversions of the coarse operator (the first two iterations always make theirs; an
                                  * inverse made one iteration earlier still is a preconditioner, only a weaker one).  2 is FASTER at C4 since the PCG
                                  * iteration costs 13 us instead of 44 (1270 against 1080 LM it/s) but its inexact steps end 3.9e-5 from the
                                  * exact-step oracle's poses -- outside north_star's 1e-5 -- where 1 ends 2.5e-6 away: 1 stays the default */
    int    one_kernel_solve;     /* 1: the PCG solve of an LM iteration as ONE persistent kernel (two stamped exchanges per iteration
                                  * instead of four launches) where the graph allows: one rank, a coarse space of <= 256 groups of
                                  * <= 64 nodes; 0: always four launches per iteration; 2: as 1 with a time-out of zero, so that the way back is
                                  * taken -- a solve whose workgroups are not all resident gives up and is repeated with launches, and the
                                  * engine stays with launches (stba_version() >= 5); 3 (stba_version() >= 6): as 1 with the stamps of the
                                  * two exchanges published behind an agent-scope RELEASE fence and read in front of an ACQUIRE fence -- the
                                  * formally complete protocol; 1 orders the same accesses by the hardware's own rules (stores acknowledged
                                  * before the stamp is issued, loads issued after the stamp was seen) plus compiler barriers */
    int    coarse_async;         /* 1 (stba_version() >= 6): the coarse operator is built and inverted on a SECOND stream, next to the PCG kernel, and
                                  * applied one LM iteration late -- iteration k preconditions with the inverse of iteration k - 1's operator --
                                  * EXCEPT behind a long step (coarse_async_decrease) and in the first iteration(s) (coarse_async_after), which
                                  * wait for the inverse of their own operator.  2: lag always, and with a forcing sequence the first solve runs
                                  * on block Jacobi alone.  0: always in line, as until version 5 (coarse_refresh_every applies).  Ordered by
                                  * events: run-to-run reproducible.  MEASURED at C4 (profiles/r6_c4_async*.txt), LM it/s | distance of the
                                  * converged poses from the exact-step trajectory: in line 1075 | 2.5e-6; lag from iteration 2 on 1380 | 6.0e-5;
                                  * from 3 on 1382 | 3.9e-5; from 4 on (this rule's choice) 1341 | 2.9e-6; mode 2 1515 | 1.5e-4.  The coarse space
                                  * IS the graph's weakly constrained modes: a coarse solver that is stale by a long step leaves its error exactly
                                  * there, and north_star asks for 1e-5 on poses */
    double forcing_eta_final;    /* 0 = off (stba_version() >= 6; measured without effect on C4: profiles/r6_c4_async.txt): cap on the forcing term once the LM iteration is about to converge -- the last
                                  * accepted step changed the cost by less than 100 x function_tolerance (relative).  The error of the LAST
                                  * inexact step is what the converged poses keep (about eta x its length): Eisenstat & Walker's sequence
                                  * alone leaves eta ~ 1e-2 there.  0: no cap */
    double coarse_eta;           /* 0 (stba_version() >= 6; one-kernel solve with a forcing sequence only): the solve also runs until the COARSE
                                  * residual |P^T r| has fallen to this fraction of its start value -- the coarse space holds the smooth, weakly
                                  * constrained modes, where a small residual is a large error */
    int    coarse_async_after;   /* 1 (with coarse_async = 1): the first so many LM iterations wait for the inverse of their OWN coarse operator */
    double coarse_async_decrease;/* 0.5 (with coarse_async = 1): an iteration that follows an accepted step which took MORE than this fraction off
                                  * the cost also waits for its own inverse: the operator is stale by exactly that step */
} stba_pcg_options;
void stba_pcg_default_options(stba_pcg_options* o);
typedef struct {
    int    iterations_total;            /* PCG iterations of the whole solve */
    int    solves;                      /* linear solves (one per LM iteration) */
    int    hit_cap;                     /* solves that ran into max_iterations before reaching their tolerance */
    int    max_iterations_in_a_solve;
    int    coarse_dim;                  /* unknowns of the coarse space (0: none) */
    int    coarse_refreshes;            /* coarse operators inverted */
    double last_eta;                    /* forcing term of the last solve */
    int    coarse_failures;             /* coarse operators whose factorisation met a non-positive pivot: the coarse correction was
                                         * switched off (block Jacobi alone) until the next refresh (stba_version() >= 5) */
    int    one_kernel_solves;           /* linear solves that ran as one persistent kernel (stba_pcg_options::one_kernel_solve); a solve
                                         * whose workgroups were not all resident is repeated with launches and not counted */
    double linear_solve_ms;             /* (stba_version() >= 6) with stba_lm_options::phase_timing: device time of all linear solves of the
                                         * LM solve, hipEvents on the engine's stream around the persistent kernel (or the PCG launches); else 0 */
} stba_pcg_summary;
int stba_pg_create(stba_pg** out, int n_nodes, int n_edges, const double* poses, const int* edge_i, const int* edge_j,
                   const double* meas, const unsigned char* node_fixed, void* hip_stream);
int stba_pg_destroy(stba_pg* pg);
/* multi-GPU: this engine holds one shard of the EDGES (all nodes replicated); the hook sums the gradient and
 * diagonal blocks (42 n doubles per linearisation), every matrix-vector product of the PCG (6 n doubles) and
 * the cost scalars across ranks.  rank 0 owns the once-only damping term.
 * REQUIREMENT on the hook: every rank must receive BIT-IDENTICAL sums (what ncclAllReduce / MPI_Allreduce give: one reduction
 * order for all ranks).  The solve state is replicated and every rank decides from ITS copy of the device-side convergence
 * flag how many further products -- i.e. collectives -- to enqueue; a hook whose result differs in the last bit between ranks
 * (a reduce + broadcast is fine, a per-rank gather-and-sum in rank-dependent order is not) can make ranks disagree by one
 * chunk of PCG iterations and hang in mismatched collectives. */
int stba_pg_set_allreduce(stba_pg* pg, stba_allreduce_fn fn, void* user, int rank, int world_size);
int stba_pg_set_comm(stba_pg* pg, stba_comm* comm);
int stba_pg_get_poses(stba_pg* pg, double* poses);
/* r[n_edges*6], Ji / Jj [n_edges*36] (6x6 row-major, wrt delta_i / delta_j); any may be NULL */
int stba_pg_evaluate(stba_pg* pg, double* cost, double* r, double* Ji, double* Jj);
/* measurement: average device time (hipEvents on the engine's stream, `reps` launches each) of the residual + Jacobian
 * kernel and of one matrix-free product q = (J^T J + D) p */
int stba_pg_time_kernels(stba_pg* pg, int reps, double* ms_linearize, double* ms_matvec);
int stba_pg_solve(stba_pg* pg, const stba_lm_options* opt, const stba_pcg_options* pcg, stba_lm_summary* summary,
                  double* trace, int* pcg_iterations_total);
/* the linear-solver side of the last stba_pg_solve of this engine */
int stba_pg_last_pcg_summary(stba_pg* pg, stba_pcg_summary* out);

/* --- pose-graph edge information matrices --------------------------------------------------- */
/* An engine as created weights every edge by the identity: cost = 1/2 sum |r_e|^2.  With per-edge weights the cost is
 * 1/2 sum |W_e r_e|^2 = 1/2 sum r_e^T Omega_e r_e, Omega_e = W_e^T W_e; W_e (6 x 6, the square-root information) multiplies the
 * residual and both Jacobians of the edge inside the linearisation kernel, so everything behind it works on the weighted problem:
 *   stba_pg_evaluate               hands back the WHITENED r = W r, Ji = W Ji, Jj = W Jj and the weighted cost;
 *   stba_pg_solve                  minimises the weighted cost;
 *   stba_pg_covariance[_columns]   return (J^T Omega J)^-1;
 *   stba_pg_time_kernels           times the whitening linearisation.
 * Rows and columns are in the tangent order of the residual, [rho(3), theta(3)].
 * CONVENTION of the information form: Omega = L L^T (Cholesky, L lower triangular) and W = L^T, so that W^T W = Omega.  This is
 * NOT the matrixL() habit of Ceres' pose_graph_3d example (residual <- L r, whose cost is r^T L^T L r); the two agree only for
 * a diagonal Omega.  A caller who wants that cost passes L to stba_pg_set_sqrt_information.
 *   stba_pg_set_information       information[m*36]: a symmetric positive definite 6x6 per edge, row-major, in the order of
 *                                 stba_pg_create's edges (of THIS engine's edge shard where the edges are sharded); the lower
 *                                 triangle is factored on the device, in double-double arithmetic, so that W is the correctly
 *                                 rounded factor of the matrix given.  An edge whose matrix has a pivot that is not positive, or
 *                                 any entry that is not finite: STBA_ERR_NOT_POSITIVE_DEFINITE, stba_last_error() names the
 *                                 smallest such edge.
 *   stba_pg_set_sqrt_information  sqrt_information[m*36]: any finite W per edge, row-major (it need be neither triangular nor
 *                                 symmetric).  An entry that is not finite: STBA_ERR_INVALID_ARGUMENT, the edge named likewise.
 *   NULL for either               back to the identity: the array is released and the engine is bit for bit the one that never
 *                                 had weights (it runs the kernel without the whitening).
 *   stba_pg_has_information       *has = 1 while the engine holds weights.
 * A call that fails leaves the engine with the weights it had.  A call that succeeds invalidates the current linearisation: the
 * next solve, evaluation or covariance starts from a fresh one.  Both setters are allowed with an all-reduce hook or communicator
 * set.  STBA_VERSION is unchanged: test for the symbols. */
int stba_pg_set_information(stba_pg* pg, const double* information);
int stba_pg_set_sqrt_information(stba_pg* pg, const double* sqrt_information);
int stba_pg_has_information(const stba_pg* pg, int* has);

/* --- pose-graph robust loss functions ------------------------------------------------------- */
/* Per edge a loss rho_e: cost = 1/2 sum rho_e(s_e), s_e = |W_e r_e|^2 (W_e the edge's square-root information, the identity without
 * one).  The kinds are Ceres' (loss_function.h), with Ceres' rho, rho', rho'' and its lower clamp of rho' by DBL_MIN:
 *   TRIVIAL          rho = s
 *   HUBER(a)         s for s <= a^2, else 2 a sqrt(s) - a^2
 *   SOFTLONE(a)      2 a^2 (sqrt(1 + s / a^2) - 1)
 *   CAUCHY(a)        a^2 log(1 + s / a^2)
 *   ARCTAN(a)        a atan2(s, a)
 *   TOLERANT(a, b)   b log(1 + e^((s - a) / b)) - b log(1 + e^(-a / b)); s - a - b log(1 + e^(-a / b)) once (s - a) / b > 36.7
 *   TUKEY(a)         (a^2 / 3) (1 - (1 - s / a^2)^3) for s <= a^2, else a^2 / 3 (rho' = rho'' = 0)
 * and scale_e multiplies rho, rho' and rho'' (Ceres' ScaledLoss).  The linearisation kernel applies Ceres' corrector to the residual
 * and both Jacobians of the edge behind the whitening, so everything behind it works on the robustified problem:
 *   stba_pg_evaluate               hands back the CORRECTED r' and J' (Ceres' Problem::Evaluate with apply_loss_function = true:
 *                                  J'^T r' = rho' J^T r) and the cost 1/2 sum rho;
 *   stba_pg_solve                  minimises 1/2 sum rho;
 *   stba_pg_covariance[_columns]   return (J'^T J')^-1, as Ceres' Covariance does;
 *   stba_pg_time_kernels           times the correcting linearisation.
 *   stba_pg_set_loss   kind[m] (STBA_LOSS_*), a[m], b[m], scale[m] in the order of stba_pg_create's edges (of THIS engine's edge shard
 *                      where the edges are sharded).  b may be NULL if no edge is TOLERANT, a may be NULL if every edge is TRIVIAL,
 *                      scale == NULL means 1 for every edge.  Entries of a and b that the edge's kind does not use are not read.
 *                      Checked before anything is replaced: an unknown kind, an a (or, for TOLERANT, b) that is not finite and
 *                      positive, a scale that is not finite or is negative: STBA_ERR_INVALID_ARGUMENT, stba_last_error() names the
 *                      smallest such edge, and the engine keeps the table it had.
 *                      kind == NULL removes the table: the engine is bit for bit the one that never had a loss (it runs the
 *                      kernel without the corrector).  An edge of kind TRIVIAL and scale 1 is left untouched by the corrector.
 *   stba_pg_has_loss   *has = 1 while the engine holds a table.
 * A call that succeeds invalidates the current linearisation.  Allowed with an all-reduce hook or communicator set.  TUKEY can give
 * every edge of a node the weight zero: the solve is covered by its damping; a covariance at such a point is refused by the
 * conjugate gradient's own guards (STBA_ERR_NOT_POSITIVE_DEFINITE, or its iteration cap), the structural gauge check does not see it.  STBA_VERSION is unchanged: test for the symbols. */
enum {
    STBA_LOSS_TRIVIAL = 0, STBA_LOSS_HUBER = 1, STBA_LOSS_SOFTLONE = 2, STBA_LOSS_CAUCHY = 3, STBA_LOSS_ARCTAN = 4,
    STBA_LOSS_TOLERANT = 5, STBA_LOSS_TUKEY = 6
};
int stba_pg_set_loss(stba_pg* pg, const int* kind, const double* a, const double* b, const double* scale);
int stba_pg_has_loss(const stba_pg* pg, int* has);

/* --- pose-graph node pose priors ------------------------------------------------------------ */
/* A prior k names a node n_k, a prior pose Zh_k -- [qx, qy, qz, qw, tx, ty, tz] like the engine's poses -- and a 6 x 6 square-root
 * information W_k (row-major, in the tangent order [rho(3), theta(3)] of the engine's residuals):
 *     r_k = log(Zh_k^-1 T_n)      J_k = d r_k / d delta_n = Jr^-1(r_k)      cost += 1/2 |W_k r_k|^2
 * -- the relative-pose edge whose other end is a constant node at the identity: the same log (the short way round), the same
 * Jr^-1 = I + ad/2 + ad^2/12.  A GPS / RTK position (zero theta rows of W: a position-only prior), a surveyed start pose, a
 * map-localisation fix, the prior a marginalised window leaves on its boundary node; the gauge of a graph that fixes no node.  Any
 * number of priors, several on one node.  A constant node's prior has J = 0 and adds to the cost only.  Priors carry no robust loss;
 * edge weights and edge losses combine with them freely.
 *   stba_pg_set_priors   node[n], pose[n*7], and at most ONE of information[n*36] (symmetric positive definite; the lower triangle is
 *                      factored on the host, Omega = L L^T, W = L^T, in double-double arithmetic, as stba_ba_set_pose_priors does;
 *                      else STBA_ERR_NOT_POSITIVE_DEFINITE) and sqrt_information[n*36] (any finite W, rank-deficient included).
 *                      Both NULL: the identity.  Quaternions are normalised on the host (one that is unit to 8 eps keeps its bits).
 *                      n = 0 clears the priors: the engine then enqueues exactly what one that never had any enqueues.
 *                      STBA_ERR_INVALID_ARGUMENT, stba_last_error() naming the smallest such prior, nothing changed: a node index
 *                      out of range, an entry that is not finite, a zero quaternion; also both weight arrays given.
 *   stba_pg_prior_count  *n = the number of priors held.
 *   stba_pg_evaluate_priors   at the current poses: cost = 1/2 sum |W r|^2 of the priors alone, r[n*6] = W_k r_k, J[n*36] = W_k J_k
 *                      (6 x 6 row-major), in the caller's order; any may be NULL.
 *   stba_pg_prior_kernel_geometry   DIAGNOSTIC, NOT A STABLE INTERFACE (the tests derive their prior sets from it): priors per
 *                      workgroup of the per-prior kernel, prior-bearing nodes per workgroup of the per-node kernel.
 * With priors, stba_pg_evaluate's cost, the LM summary and trace, the gradient norm the loop stops on and
 * stba_pg_covariance[_columns] are those of the SUM, edges plus priors (r, Ji, Jj of stba_pg_evaluate stay per edge).  For the
 * covariance a connected component passes the gauge check if it holds a constant node OR a node with a prior that is not constant;
 * the check is structural -- a component held only by rank-deficient priors (one position-only prior leaves the rotation about that
 * point free) passes it, and the singular J^T J is refused by the conjugate gradient's own reports (STBA_ERR_NOT_POSITIVE_DEFINITE).
 * stba_pg_gauge_check itself keeps its meaning: it knows no priors.  A setter that succeeds invalidates the current linearisation.
 * LIMIT, refused with STBA_ERR_INVALID_ARGUMENT, the state untouched, in both orders of the two calls: an all-reduce hook or
 * communicator (several ranks); a call that clears either is never refused.  STBA_VERSION is unchanged: test for the symbols. */
int stba_pg_set_priors(stba_pg* pg, int n, const int* node, const double* pose /*[n*7]*/,
                       const double* information /*[n*36] or NULL*/, const double* sqrt_information /*[n*36] or NULL*/);
int stba_pg_prior_count(const stba_pg* pg, int* n);
int stba_pg_evaluate_priors(stba_pg* pg, double* cost, double* r /*[n*6]*/, double* J /*[n*36], 6x6 row-major*/);
int stba_pg_prior_kernel_geometry(const stba_pg* pg, int* priors_per_workgroup, int* nodes_per_workgroup);

/* --- pose-graph covariance ---------------------------------------------------------------- */
/* C = (J^T J)^-1 of the undamped, unscaled problem at the engine's current poses, in the engine's tangent coordinates (per node
 * [rho, theta] of T <- T exp(delta)); not multiplied by a residual variance (the definition of stba_ba_covariance_compute); constant
 * nodes have zero rows and columns.  The columns of the requested nodes are solved 64 at a time by a batched preconditioned
 * conjugate gradient on the device (pg_covariance.hip): memory is O(6 n_nodes x 64) whatever is asked for.  Both entry
 * points re-linearise, run on the engine's stream and leave the LM state alone: a later stba_pg_solve gives the same bits as
 * one without the call.
 * Refused, with the reason in stba_last_error() and nothing written to out:
 *   STBA_ERR_NOT_POSITIVE_DEFINITE  before any device work: a connected component of the graph without a constant node (J^T J is
 *                                   singular; the message names the component's size and first node -- stba_pg_gauge_check);
 *                                   during the solve: p^T H p <= 0, or max_iterations reached with the TRUE relative residual
 *                                   |e - H x| / |e| of a column above relative_tolerance (the message gives it and the iterations)
 *   STBA_ERR_INVALID_ARGUMENT       a node index out of range
 *   STBA_ERR_STATE                  an all-reduce hook or communicator is set (several ranks)
 * STBA_VERSION is unchanged: test for the symbols. */
typedef struct {
    size_t struct_size;          /* sizeof(stba_pg_covariance_options); fields behind struct_size are taken as their defaults */
    double relative_tolerance;   /* 1e-12, on the true residual |e - H x| / |e| of every column */
    int    max_iterations;       /* 0: 6 x the number of free nodes (the dimension of the system), per batch */
    int    check_every;          /* 4: iterations enqueued between the host's looks at the device-side flag */
} stba_pg_covariance_options;
void stba_pg_covariance_default_options(stba_pg_covariance_options* o);
typedef struct {
    size_t struct_size;          /* sizeof(stba_pg_covariance_summary); fields behind struct_size are not written */
    int    batches;              /* batches of up to 64 columns */
    int    columns;              /* columns solved (6 per distinct free node) */
    int    iterations_total;     /* PCG iterations over all batches */
    int    max_iterations_in_a_batch;
    double max_relative_residual;/* largest true |e - H x| / |e| over all columns */
    double device_ms;            /* hipEvents on the engine's stream around the whole computation */
} stba_pg_covariance_summary;
/* out[n_pairs*36]: the 6x6 row-major block C[node_a[k], node_b[k]] per pair; solves for the distinct node_b; a pair that names a
 * constant node gets zeros.  opt and summary may be NULL. */
int stba_pg_covariance(stba_pg* pg, int n_pairs, const int* node_a, const int* node_b, const stba_pg_covariance_options* opt,
                       double* out, stba_pg_covariance_summary* summary);
/* out[6*n_nodes*6] row-major: the six whole columns of C that belong to `node` -- its covariance with every pose of the graph */
int stba_pg_covariance_columns(stba_pg* pg, int node, const stba_pg_covariance_options* opt, double* out,
                               stba_pg_covariance_summary* summary);
/* the gauge check both run first, on the host and without a device: STBA_OK, or STBA_ERR_NOT_POSITIVE_DEFINITE if a connected
 * component of the graph holds no constant node (node_fixed may be NULL: no constant node at all) */
int stba_pg_gauge_check(int n_nodes, int n_edges, const int* edge_i, const int* edge_j, const unsigned char* node_fixed);

/* ================================ bundle adjustment: ITERATIVE_SCHUR ================================ */
/* Ceres' linear_solver_type = ITERATIVE_SCHUR: conjugate gradients on the reduced camera system S = (Hcc + D) - W V^-1 W^T, applied
 * implicitly (two passes over the observations per product), so that neither S (8 (6 n_cams)^2 bytes) nor a Schur plan is ever
 * made: the camera count is limited by the observations, not by S.  Same LM loop, damping, Jacobi scaling and constant dofs as the
 * dense path; the step is inexact, its model change is -(J d)^T (r + J d / 2).  DESIGN.md 7b.
 * stba_ba_create_options versions itself by struct_size: set it to sizeof(stba_ba_create_options); fields behind struct_size are
 * taken as their defaults.  opt = NULL or STBA_LINEAR_DENSE_SCHUR: exactly stba_ba_create.
 * An ITERATIVE_SCHUR engine refuses, with STBA_ERR_INVALID_ARGUMENT and its state untouched: stba_ba_reduced_system,
 * stba_ba_solve_reduced, stba_ba_set_schur_mode, stba_ba_time_schur, stba_ba_covariance_compute (it needs the explicit S) and
 * stba_ba_set_allreduce / stba_ba_set_comm (one rank only). */
enum { STBA_LINEAR_DENSE_SCHUR = 0, STBA_LINEAR_ITERATIVE_SCHUR = 1 };
typedef struct {
    size_t struct_size;          /* sizeof(stba_ba_create_options) */
    int    linear_solver;        /* STBA_LINEAR_DENSE_SCHUR (default) | STBA_LINEAR_ITERATIVE_SCHUR */
} stba_ba_create_options;
int stba_ba_create_ex(stba_ba** out, int n_cams, int n_pts, int n_obs, const double* cams, const double* pts, const int* obs_cam,
                      const int* obs_pt, const double* obs_feat, const unsigned char* cam_fixed, const unsigned char* pt_fixed,
                      void* hip_stream, const stba_ba_create_options* opt);
/* preconditioners, one 6x6 inverse per camera and LM iteration: IDENTITY (the identity in Jacobi-scaled coordinates), JACOBI (blocks
 * of Hcc + D, Ceres' ImplicitSchurComplement block_diagonal_FtF_inverse), SCHUR_JACOBI (blocks of S) */
enum { STBA_PRECOND_IDENTITY = 0, STBA_PRECOND_JACOBI = 1, STBA_PRECOND_SCHUR_JACOBI = 2 };
/* Ceres' defaults: JACOBI, eta 0.1 (q_tolerance, Nash & Sofer's test i (Q_i - Q_{i-1}) / Q_i <= eta), min 0, max 500 iterations;
 * check_every (4): iterations enqueued between the host's looks at the device-side stop flag.  Dense engines: invalid argument. */
int stba_ba_set_pcg(stba_ba* ba, int preconditioner, double eta, int min_iterations, int max_iterations, int check_every);
/* iterations_total, solves, hit_cap, max_iterations_in_a_solve, last_eta and (with phase_timing) linear_solve_ms of the last LM solve */
int stba_ba_last_pcg_summary(stba_ba* ba, stba_pcg_summary* out);
/* per_iteration[k]: PCG iterations of LM iteration k + 1 of the last solve, for k < n (0 behind its last iteration, and on a dense
 * engine) -- Ceres' IterationSummary::linear_solver_iterations */
int stba_ba_last_pcg_iterations(stba_ba* ba, int* per_iteration, int n);
/* test and diagnostic hook (needs stba_ba_normal_blocks): with explicit diagonals dc[n], dp[n_pts*3] as stba_ba_reduced_system takes
 * them, y[n] = S x (which = 0), the JACOBI (1) or SCHUR_JACOBI (2) preconditioner inverse applied to x, or the reduced right-hand
 * side -(gc - W V^-1 gp) when x == NULL.  Entries of constant dofs are zero in and out. */
int stba_ba_schur_apply(stba_ba* ba, const double* dc, const double* dp, int which, const double* x, double* y);
/* measurement: average device time (ms, hipEvents on the engine's stream) of one product S x -- the landmark and the camera pass --
 * over `reps` back-to-back products, with the blocks and the x of the last stba_ba_schur_apply */
int stba_ba_time_schur_apply(stba_ba* ba, int reps, double* ms_avg);

/* ================================ bundle adjustment: DOGLEG ================================ */
/* Ceres' trust_region_strategy_type = DOGLEG, dogleg_type = TRADITIONAL_DOGLEG (Powell's dogleg).  The reduced camera system is
 * built and factored ONCE per linearisation, at a small regularisation mu (1e-8, raised tenfold while a pivot fails and lowered
 * after every accepted step); the Gauss-Newton and the Cauchy step are kept, and a rejected step only halves the radius and mixes
 * the two again -- no Schur build, no factorisation, no back-substitution.  Same Jacobi scaling, LM diagonal bounds, constant dofs,
 * tolerances and trace as the LM loop; the trace's radius column and stba_lm_summary::final_radius carry the dogleg radius.
 * stba_ba_solve follows the engine's strategy; stba_ba_lm_iterations (the benchmark's unit) always runs LM.  DESIGN.md 7c.
 * Refused with STBA_ERR_INVALID_ARGUMENT, the state untouched: DOGLEG on an ITERATIVE_SCHUR engine (Ceres: "DOGLEG only supports
 * exact factorization based linear solvers"), DOGLEG on an engine with an all-reduce hook or communicator, stba_ba_set_allreduce /
 * stba_ba_set_comm on a DOGLEG engine (one rank only), an unknown strategy.  STBA_VERSION is unchanged: test for the symbols. */
enum { STBA_TR_LEVENBERG_MARQUARDT = 0, STBA_TR_TRADITIONAL_DOGLEG = 1 };
int stba_ba_set_trust_region(stba_ba* ba, int strategy);      /* default LM; stba_ba_solve follows it */
typedef struct {
    size_t struct_size;          /* sizeof(stba_dogleg_summary); fields behind struct_size are not written */
    int    factorizations;       /* factorisations of the reduced system (one per linearisation, plus one per mu escalation) */
    int    gauss_newton_solves;  /* Gauss-Newton steps computed (each behind a factorisation) */
    int    reused_steps;         /* steps that re-used the directions of the linearisation (every step behind a rejection) */
    int    invalid_steps;        /* steps without a valid Gauss-Newton step or with a model change that is not positive */
    int    steps_by_case[3];     /* trial steps: [0] the Gauss-Newton step, [1] the Cauchy step cut at the radius, [2] interpolated */
    double final_mu;             /* mu at the end of the solve */
} stba_dogleg_summary;
/* the last stba_ba_solve of this engine (all zero if it ran LM) */
int stba_ba_last_dogleg_summary(stba_ba* ba, stba_dogleg_summary* out);

/* ================================ bundle adjustment: inner iterations ================================ */
/* Ceres' Solver::Options::use_inner_iterations: after every valid trust-region step of stba_ba_solve / stba_ba_lm_iterations (LM,
 * dense Schur or ITERATIVE_SCHUR), one coordinate-descent sweep moves the trial point x+ to x*: the groups of the ordering in
 * ascending id, every block of a group solved on its own -- all other blocks held fixed -- by a Levenberg-Marquardt solve with
 * Ceres' DEFAULT options over the residuals that touch it.  The model cost change grows by cost(x+) - cost(x*), the step is
 * accepted if cost(x*) < cost(x) or rho > min_relative_decrease, and the trace / callback report x*.  Once a sweep improves the
 * trial cost by a relative 1 - cost(x*) / cost(x+) <= tolerance, sweeps stop for the rest of the solve.  DESIGN.md 7d.
 * Blocks: a camera's rotation (dofs 0..2) and position (dofs 3..5), and every landmark.  cam_rot_group[n_cams], cam_pos_group[n_cams],
 * pt_group[n_pts]: the group id of each (>= 0), -1 = not swept (held fixed by the sweeps); equal rotation and position ids make the
 * camera ONE 6-dof block.  All three NULL: the default ordering {cameras as 6-dof blocks}, {landmarks}; one NULL among the others:
 * none of that kind is swept.  Constant blocks (every dof of the part constant) are ignored.
 * Refused with STBA_ERR_INVALID_ARGUMENT (stba_last_error names the offending pair), the state untouched: a group that is not an
 * independent set (a camera and a landmark it observes), a negative tolerance, an engine with an all-reduce hook or communicator or a
 * host lineariser (and those setters on an engine with inner iterations).  stba_ba_solve on a DOGLEG engine with inner iterations:
 * STBA_ERR_INVALID_ARGUMENT before any device work.  enable = 0: off (exactly the engine that never enabled them).
 * STBA_VERSION is unchanged: test for the symbols. */
int stba_ba_set_inner_iterations(stba_ba* ba, int enable, double tolerance, const int* cam_rot_group, const int* cam_pos_group,
                                 const int* pt_group);
/* one sweep at the current point (the ordering set above, or the default one), which moves the engine's parameters.
 * iterations_per_block (nullable) [2 n_cams + n_pts]: the inner LM iterations (trust-region steps) of every rotation block, then
 * every position block, then every landmark, in the caller's order; a 6-dof camera block reports its count in both entries, a
 * block that is not swept 0.  cost_before / cost_after (nullable): 1/2 |r|^2 before and after the sweep. */
int stba_ba_inner_sweep(stba_ba* ba, double* cost_before, double* cost_after, int* iterations_per_block);
#define STBA_INNER_MAX_GROUPS_REPORTED 16
typedef struct {
    size_t struct_size;          /* sizeof(stba_inner_summary); fields behind struct_size are not written */
    int    sweeps;               /* sweeps run by the last solve (or by the last stba_ba_inner_sweep) */
    int    disabled_at_iteration;/* the iteration whose sweep switched inner iterations off, or -1 */
    double sweep_ms;             /* device time of the sweeps (stba_lm_options::phase_timing; else 0) */
    int    num_groups;           /* groups of the ordering used */
    int    group_size[STBA_INNER_MAX_GROUPS_REPORTED];   /* blocks of every group, ascending id (the first 16) */
} stba_inner_summary;
int stba_ba_last_inner_summary(stba_ba* ba, stba_inner_summary* out);

/* ================================ bundle adjustment: robust loss functions ================================ */
/* A loss rho_i per observation, the kinds and parameters of the pose graph's table above (STBA_LOSS_*, Ceres' rho, rho', rho'' and
 * ScaledLoss): the engine then minimises 1/2 sum_i rho_i(|r_i|^2).  A linearisation kernel of its own evaluates the loss at
 * s = |r|^2 and applies Ceres' corrector to the residual and to both Jacobian blocks of the observation; it writes them in the
 * general form that host-linearised factors use (the 2x6 camera block stored, not re-derived from the projection), so every stage
 * behind it works on the robustified problem:
 *   stba_ba_evaluate              hands back the CORRECTED r', Jc', Jp' (columns of constant dofs zero) and the cost 1/2 sum rho --
 *                                 Ceres' Problem::Evaluate with apply_loss_function = true;
 *   stba_ba_solve / _lm_iterations  LM or DOGLEG, dense Schur (both forms) or ITERATIVE_SCHUR: the step solves
 *                                 (J'^T J' + D) d = -J'^T r', the model change is that of (r', J'), the gain ratio divides the change
 *                                 of 1/2 sum rho by it;
 *   stba_ba_covariance_compute    gives (J'^T J')^-1, as Ceres' Covariance does;
 *   the stage entry points and stba_ba_time_linearize work on / time the correcting linearisation.
 *   stba_ba_set_loss   kind[n_obs] (STBA_LOSS_*), a[n_obs], b[n_obs], scale[n_obs] in the CALLER's observation order (that of
 *                      stba_ba_create).  b may be NULL if no observation is TOLERANT, a may be NULL if every one is TRIVIAL,
 *                      scale == NULL means 1 for every observation.  Entries of a and b that the observation's kind does not use are
 *                      not read.  Checked before anything is replaced: an unknown kind, an a (or, for TOLERANT, b) that is not finite
 *                      and positive, a scale that is not finite or is negative: STBA_ERR_INVALID_ARGUMENT, stba_last_error() names
 *                      the smallest such observation, and the engine keeps the table it had.
 *                      kind == NULL removes the table: the engine is bit for bit the one that never had a loss (it runs the
 *                      lossless kernels on the compact Jacobian record).  An observation of kind TRIVIAL and scale 1 is left
 *                      untouched by the corrector: what stba_ba_evaluate returns for it compares == with the lossless engine's.
 *   stba_ba_has_loss   *has = 1 while the engine holds a table.
 *   stba_ba_loss_kernel_geometry   DIAGNOSTIC, NOT A STABLE INTERFACE (the tests derive their scenes from it; the figures belong to
 *                      this build's kernel and may change or go with it; every pointer nullable): observations per workgroup tile of
 *                      the correcting kernel, whether THIS engine's cameras are staged in its LDS, the largest camera count that is.
 * A call that succeeds invalidates the current linearisation and releases a held covariance.  Refused with
 * STBA_ERR_INVALID_ARGUMENT, the state untouched, in both orders: a table on an engine with a host lineariser, with inner iterations,
 * or with an all-reduce hook / communicator (and those setters on an engine with a table).  TUKEY can give every observation of a
 * landmark the weight zero: the solve is covered by its damping (the landmark does not move); a covariance at such a point meets a
 * singular landmark block.  STBA_VERSION is unchanged: test for the symbols. */
int stba_ba_set_loss(stba_ba* ba, const int* kind, const double* a, const double* b, const double* scale);  /* [n_obs], caller's observation order */
int stba_ba_has_loss(const stba_ba* ba, int* has);
int stba_ba_loss_kernel_geometry(const stba_ba* ba, int* tile_observations, int* cameras_in_lds, int* max_cameras_in_lds);

/* ================================ bundle adjustment: per-observation information matrices ================================ */
/* A 2 x 2 square-root information W_i per observation (row-major; the identity where none is given), the pose graph's semantics
 * above restated for BA: the cost is 1/2 sum_i rho_i(s_i) with s_i = |W_i r_i|^2 = r_i^T Omega_i r_i, Omega_i = W_i^T W_i.
 * Whitening comes FIRST -- r <- W r, Jc <- W Jc, Jp <- W Jp -- and Ceres' corrector then runs on the whitened triple if the
 * observation has a loss (stba_ba_set_loss; the two combine freely, in either order, and each is removed on its own).  The kernel
 * that applies the losses does the whitening (its INFO form) and writes the general Jacobian form, so:
 *   stba_ba_evaluate              hands back the WHITENED (and corrected) r, Jc, Jp and the cost above;
 *   stba_ba_solve / _lm_iterations  minimise that cost (LM or DOGLEG, both dense Schur forms, ITERATIVE_SCHUR);
 *   stba_ba_covariance_compute    gives (J^T Omega J)^-1, with losses (J'^T J')^-1;
 *   stba_ba_triangulate           STAYS the unweighted per-landmark refinement (identity weights, no loss), as it does with losses.
 *   stba_ba_set_information       information[n_obs*4]: a symmetric positive definite 2 x 2 per observation in the CALLER's observation
 *                      order; the lower triangle (a, b, c) = ([0], [2], [3]) is factored on the host, Omega = L L^T, W = L^T (the
 *                      upper off-diagonal entry [1] must be finite and is otherwise IGNORED: a matrix that is not symmetric is
 *                      taken for the symmetric one of its lower triangle, without a message):
 *                      l11 = sqrt(a), l21 = b / l11, l22 = sqrt(c - b^2 / a), the pivot c - b^2 / a formed with error-free (FMA)
 *                      products directly from a, b, c, so that every entry of W is within 4 eps (eps = 2^-52) of the exact factor of
 *                      the matrix given, up to cond(Omega) = 1e12.  A pivot that is not positive or an entry that is not finite:
 *                      STBA_ERR_NOT_POSITIVE_DEFINITE, stba_last_error() names the smallest such observation, the old weights stay.
 *   stba_ba_set_sqrt_information   sqrt_information[n_obs*4]: any finite W (it need not be triangular or symmetric); an entry that
 *                      is not finite: STBA_ERR_INVALID_ARGUMENT, the observation named likewise.
 *                      NULL to either setter goes back to the identity and releases the array: an engine that then has no loss table
 *                      either is bit for bit one that never had weights or losses (it runs the lossless kernels).  An array whose
 *                      every W is exactly the identity (for the information form: every factor) is taken the same way: no array is
 *                      held and stba_ba_has_information reports 0.  An observation
 *                      whose W is exactly the identity is not whitened: without a loss (or TRIVIAL with scale 1) what stba_ba_evaluate
 *                      returns for it compares == with the lossless engine's.
 *   stba_ba_has_information   *has = 1 while the engine holds weights.
 *   stba_ba_get_sqrt_information   out[n_obs*4]: the W the engine holds, in the caller's order; identity rows if it holds none.
 * A setter that succeeds invalidates the current linearisation and releases a held covariance.  Refused with
 * STBA_ERR_INVALID_ARGUMENT, the state untouched, in both orders: weights on an engine with a host lineariser (the callback's
 * factors whiten themselves), with inner iterations, or with an all-reduce hook / communicator / world_size > 1 (and those setters on
 * an engine with weights).  STBA_VERSION is unchanged: test for the symbols. */
int stba_ba_set_information(stba_ba* ba, const double* information);            /* [n_obs*4], caller's observation order, or NULL */
int stba_ba_set_sqrt_information(stba_ba* ba, const double* sqrt_information);  /* [n_obs*4], caller's observation order, or NULL */
int stba_ba_has_information(const stba_ba* ba, int* has);
int stba_ba_get_sqrt_information(stba_ba* ba, double* out);                     /* [n_obs*4] */

/* ================================ bundle adjustment: camera pose priors ================================ */
/* A prior k names a camera c_k, a prior pose (qh_k, th_k) -- camera to world, [qx, qy, qz, qw, tx, ty, tz] like the engine's cameras --
 * and a 6 x 6 square-root information W_k (row-major):
 *     r_k = [ Log(qh_k^-1 (x) q_c) ; t_c - th_k ]      order [rot(3), pos(3)]: that of cam_fixed and of Jc's columns, NOT the pose
 *                                                      graph's [rho, theta]
 *     J_k = d r_k / d[dtheta, dt] = blockdiag(Jr^-1(r_theta), I)   under the engine's chart q <- q (x) exp(dtheta), t <- t + dt
 *     cost += 1/2 |W_k r_k|^2
 * Log takes the short way round (q and -q give the same bits), is exact at angle 0 and usable up to the neighbourhood of pi; Jr^-1
 * is the closed form of SO(3) (a series below 0.1 rad).  GPS / INS / odometry knowledge of a pose, the gauge of a problem that fixes
 * no camera (two priors make stba_ba_covariance_compute well defined), the prior a marginalised window leaves behind.  Any number of
 * priors, several on one camera.  Columns of a camera's constant dofs (cam_fixed) are exactly 0: a constant camera's prior adds to
 * the cost only.
 *   stba_ba_set_pose_priors   cam[n], pose[n*7], and at most ONE of information[n*36] (symmetric positive definite; the lower triangle
 *                      is factored on the host, Omega = L L^T, W = L^T, in double-double arithmetic: every entry of W within 4 eps of
 *                      the exact factor of the matrix given up to cond(Omega) = 1e12; else STBA_ERR_NOT_POSITIVE_DEFINITE) and
 *                      sqrt_information[n*36] (any finite W, rank-deficient included: zero rotation rows give a position-only prior).
 *                      Both NULL: the identity.  Quaternions are normalised on the host (one that is unit to 8 eps keeps its bits).
 *                      n = 0 clears the priors: the engine then enqueues exactly what one that never had any enqueues.
 *                      STBA_ERR_INVALID_ARGUMENT, stba_last_error() naming the smallest such prior, nothing changed: a camera index
 *                      out of range, an entry that is not finite, a zero quaternion; also both weight arrays given.
 *   stba_ba_pose_prior_count  *n = the number of priors held.
 *   stba_ba_evaluate_pose_priors   at the current parameters: cost = 1/2 sum |W r|^2 of the priors alone, r[n*6] = W_k r_k,
 *                      J[n*36] = W_k J_k (6 x 6 row-major), in the caller's order; any may be NULL.
 *   stba_ba_pose_prior_kernel_geometry   DIAGNOSTIC, NOT A STABLE INTERFACE (the tests derive their scenes from it): cameras with
 *                      priors per workgroup of the block kernel.
 * With priors, stba_ba_evaluate's and stba_ba_cost's cost, the LM summary and trace and the gradient norm are those of the SUM,
 * observations plus priors (r, Jc, Jp stay per observation); stba_ba_normal_blocks' Hcc, gc include the priors' J'^T J', J'^T r';
 * stba_ba_solve / _lm_iterations (LM; PAIRS and DENSE), the stage entry points, stba_ba_covariance_compute and its getters run on
 * the sum; losses and information matrices on the observations combine freely.  A setter that succeeds invalidates the current
 * linearisation and releases a held covariance.  LIMITS, refused with STBA_ERR_INVALID_ARGUMENT, the state untouched, in both
 * orders of the two calls: ITERATIVE_SCHUR engines (the inexact-step model term is summed from the observation records), DOGLEG
 * (its |J g|^2 is too), inner iterations, a host lineariser, an all-reduce hook / communicator / world_size > 1.
 * STBA_VERSION is unchanged: test for the symbols. */
int stba_ba_set_pose_priors(stba_ba* ba, int n, const int* cam, const double* pose /*[n*7]*/,
                            const double* information /*[n*36] or NULL*/, const double* sqrt_information /*[n*36] or NULL*/);
int stba_ba_pose_prior_count(const stba_ba* ba, int* n);
int stba_ba_evaluate_pose_priors(stba_ba* ba, double* cost, double* r /*[n*6]*/, double* J /*[n*36], 6x6 row-major*/);
int stba_ba_pose_prior_kernel_geometry(const stba_ba* ba, int* cameras_per_workgroup);

/* ================================ bundle adjustment: camera-to-camera relative-pose factors ================================ */
/* An edge k names two distinct cameras i_k, j_k, a measured relative pose (qz_k, tz_k) -- "camera j seen from camera i",
 * [qx, qy, qz, qw, tx, ty, tz]: wheel odometry, a pre-integrated IMU, ICP, a loop closure -- and a 6 x 6 square-root information W_k
 * (row-major).  Conventions of the engine and of the pose priors, NOT the pose graph's: poses camera to world, chart
 * q <- q (x) exp(dtheta), t <- t + dt, order [rot(3), pos(3)]:
 *     r_k = [ Log(qz^-1 (x) (q_i^-1 (x) q_j)) ; R_i^T (t_j - t_i) - tz ]
 *     d r_theta / d dtheta_j = Jr^-1(r_theta)        d r_theta / d dtheta_i = -Jr^-1(r_theta) R_j^T R_i
 *     d r_p / d dt_j = R_i^T      d r_p / d dt_i = -R_i^T      d r_p / d dtheta_i = hat(R_i^T (t_j - t_i))
 *     cost += 1/2 |W_k r_k|^2
 * Log and Jr^-1 are the priors': the short way round, the same bits when any one of qz, q_i, q_j is negated.  Columns of a camera's
 * constant dofs (cam_fixed) are exactly 0.  Any number of edges, several on one pair, in either direction; the two cameras need
 * not share a landmark.
 *   stba_ba_set_relative_poses   cam_i[n], cam_j[n], meas[n*7], and at most ONE of information[n*36] (symmetric positive definite,
 *                      factored on the host as stba_ba_set_pose_priors does; else STBA_ERR_NOT_POSITIVE_DEFINITE) and
 *                      sqrt_information[n*36] (any finite W, rank-deficient included).  Both NULL: the identity.  Quaternions are
 *                      normalised on the host (one that is unit to 8 eps keeps its bits).  n = 0 clears the edges: the engine then
 *                      enqueues exactly what one that never had any enqueues.  STBA_ERR_INVALID_ARGUMENT, stba_last_error() naming
 *                      the smallest such edge, nothing changed: a camera index out of range, cam_i == cam_j, an entry that is not
 *                      finite, a zero quaternion; also both weight arrays given.
 *   stba_ba_relative_pose_count  *n = the number of edges held.
 *   stba_ba_evaluate_relative_poses   at the current parameters: cost = 1/2 sum |W r|^2 of the edges alone, r[n*6] = W_k r_k,
 *                      Ji[n*36] = W_k d r_k / d[dtheta_i, dt_i], Jj[n*36] likewise (6 x 6 row-major), the caller's order; any may be NULL.
 *   stba_ba_relative_pose_kernel_geometry   DIAGNOSTIC, NOT A STABLE INTERFACE (the tests derive their scenes from it): groups
 *                      (cameras with edges, then pairs with edges) per workgroup of the block kernel.
 * With edges, stba_ba_evaluate's and stba_ba_cost's cost, the LM summary and trace and the gradient norm are those of the SUM;
 * stba_ba_normal_blocks' Hcc, gc include the edges' J_x'^T J_x', J_x'^T r' (the off-diagonal part lives in the reduced system only:
 * stba_ba_reduced_system's S carries sum J_hi'^T J_lo' in its block (hi, lo), hi > lo); stba_ba_solve / _lm_iterations (LM; PAIRS and
 * DENSE), the stage entry points, stba_ba_covariance_compute and its getters run on the sum; pose priors, losses and information
 * matrices on the observations combine freely.  A setter that succeeds invalidates the current linearisation and releases a held
 * covariance.  LIMITS, refused with STBA_ERR_INVALID_ARGUMENT, the state untouched, in both orders of the two calls: ITERATIVE_SCHUR
 * engines, DOGLEG, inner iterations, a host lineariser, an all-reduce hook / communicator / world_size > 1 (the packing of the
 * cross-rank sum knows the landmarks' sparsity only).  STBA_VERSION is unchanged: test for the symbols. */
int stba_ba_set_relative_poses(stba_ba* ba, int n, const int* cam_i, const int* cam_j, const double* meas /*[n*7]*/,
                               const double* information /*[n*36] or NULL*/, const double* sqrt_information /*[n*36] or NULL*/);
int stba_ba_relative_pose_count(const stba_ba* ba, int* n);
int stba_ba_evaluate_relative_poses(stba_ba* ba, double* cost, double* r /*[n*6]*/, double* Ji /*[n*36]*/, double* Jj /*[n*36]*/);
int stba_ba_relative_pose_kernel_geometry(const stba_ba* ba, int* groups_per_workgroup);

/* ================================ bundle adjustment: landmark position priors (control points) ================================ */
/* A prior k names a landmark j_k, a position ph_k and a 3 x 3 square-root information W_k (row-major):
 *     r_k = p_j - ph_k          J_k = d r_k / d p_j = I  (exactly 0 for a constant landmark, pt_fixed: the prior then adds to the cost only)
 *     cost += 1/2 |W_k r_k|^2
 * A surveyed ground control point with its sigma, a LiDAR or map point, a depth prior, the landmark prior a marginalised window
 * leaves behind; the gauge of a problem that fixes no camera (priors on four landmarks that are not coplanar make
 * stba_ba_covariance_compute well defined).  Any number of priors, several on one landmark, landmarks without any.
 *   stba_ba_set_landmark_priors   pt[n], position[n*3], and at most ONE of information[n*9] (symmetric positive definite; the lower
 *                      triangle is factored on the host, Omega = L L^T, W = L^T, in double-double arithmetic: every entry of W within
 *                      1 eps of the exact factor of the matrix given up to cond(Omega) = 1e12; else STBA_ERR_NOT_POSITIVE_DEFINITE)
 *                      and sqrt_information[n*9] (any finite W, rank-deficient included: one non-zero row is a height-only control
 *                      point).  Both NULL: the identity.  n = 0 clears the priors and is never refused: the engine then enqueues
 *                      exactly what one that never had any enqueues.  STBA_ERR_INVALID_ARGUMENT, stba_last_error() naming the
 *                      smallest such prior, nothing changed: a landmark index out of range, an entry that is not finite; also both
 *                      weight arrays given with n > 0 (n = 0 reads none of the arrays).
 *   stba_ba_landmark_prior_count  *n = the number of priors held.
 *   stba_ba_evaluate_landmark_priors   at the current parameters: cost = 1/2 sum |W r|^2 of the priors alone, r[n*3] = W_k r_k,
 *                      J[n*9] = W_k J_k (3 x 3 row-major), in the caller's order; any may be NULL.
 *   stba_ba_landmark_prior_kernel_geometry   DIAGNOSTIC, NOT A STABLE INTERFACE (the tests derive their scenes from it): landmarks
 *                      (with priors or without) per workgroup of the block kernel.
 * With priors, stba_ba_evaluate's and stba_ba_cost's cost, the LM summary and trace and the gradient norm are those of the SUM,
 * observations plus priors (r, Jc, Jp stay per observation); stba_ba_normal_blocks' Hpp, gp include the priors' W^T W, W^T r' (Hcc,
 * gc keep their bits, and so do the blocks of landmarks without priors); every solver path runs on the sum: stba_ba_solve /
 * _lm_iterations with LM on PAIRS and DENSE, ITERATIVE_SCHUR engines with every preconditioner (the inexact-step model gains the
 * priors' rows), DOGLEG (its three J sums do), the stage entry points, stba_ba_covariance_compute and its getters; losses,
 * information matrices, pose priors and relative-pose factors combine freely.  A setter that succeeds invalidates the current
 * linearisation and releases a held covariance.  LIMITS, refused with STBA_ERR_INVALID_ARGUMENT, the state untouched, in both
 * orders of the two calls: inner iterations (the per-landmark sweep solves from the observation records), a host lineariser, an
 * all-reduce hook / communicator / world_size > 1.  STBA_VERSION is unchanged: test for the symbols. */
int stba_ba_set_landmark_priors(stba_ba* ba, int n, const int* pt, const double* position /*[n*3]*/,
                                const double* information /*[n*9] or NULL*/, const double* sqrt_information /*[n*9] or NULL*/);
int stba_ba_landmark_prior_count(const stba_ba* ba, int* n);
int stba_ba_evaluate_landmark_priors(stba_ba* ba, double* cost, double* r /*[n*3]*/, double* J /*[n*9], 3x3 row-major*/);
int stba_ba_landmark_prior_kernel_geometry(const stba_ba* ba, int* landmarks_per_workgroup);

/* ================================ small dense LM problems ================================ */
/* Residual blocks evaluated by a HOST callback (user CostFunction::Evaluate, solver.hpp:168-212;
 * autodiff functors are differentiated on the host by the C++ shim), normal equations + LM
 * step on the device.  x: n_params ambient; J row-major n_res x n_local in LOCAL coordinates. */
typedef int (*stba_residual_fn)(void* user, const double* x, double* r, double* J);
typedef void (*stba_plus_fn)(void* user, const double* x, const double* delta, double* x_new);
int stba_dense_solve(stba_residual_fn fn, stba_plus_fn plus, void* user, int n_params, int n_local,
                     int n_res, double* x, const double* lower, const double* upper,
                     const stba_lm_options* opt, stba_lm_summary* summary, double* trace,
                     stba_iteration_callback cb, void* cb_user);

/* covariance of a small dense problem (not a bundle adjustment) at x: the callback is evaluated once, J^T J formed on the device as
 * in stba_dense_solve's general path and inverted there; cov[n_local*n_local] row-major in LOCAL coordinates.  Same limits as the
 * dense solve (4096 local parameters, 2.7e8 Jacobian entries) and the same pivot test as stba_ba_covariance_compute. */
int stba_dense_covariance(stba_residual_fn fn, void* user, int n_params, int n_local, int n_res, const double* x, double min_rcond,
                          double* cov, double* rcond_out);

#ifdef __cplusplus
}
#endif
#endif
