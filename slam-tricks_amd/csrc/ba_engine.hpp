// ba_engine.hpp -- the bundle-adjustment engine object behind the opaque stba_ba of include/stba.h, the owners of its state, and the
// host functions that cross the BA host units: stba_engine.hip (the process-wide entry points, creation and teardown, the plain
// setters and getters), ba_linear.hip (the linear algebra of one iteration: linearisation, blocks, both builds, the trial point, the
// implicit-Schur PCG), ba_allreduce.hip (the cross-rank sum of the reduced system), ba_solve.hip (the LM and DOGLEG loops, the inner
// iterations), ba_stages.hip (the stage, measurement and covariance entry points) and ba_factors.hip (the factor setters).  Private to
// these six; no kernel is declared or defined here.
#pragma once
#include <memory>
#include <vector>

#include "ba_kernels.hpp"
#include "ba_prior.hpp"
#include "ba_between.hpp"
#include "ba_landmark_prior.hpp"
#include "iterative_schur.hpp"
#include "ba_features.hpp"
#include "inner_plan.hpp"

namespace stba {

// scalar slots in the extras region behind S (summed across ranks together with S)
enum { SC_COST2 = 0, SC_GPMAX0 = 8, SC_MAX_WORLD = 64 };
// trial-point scalars: [0..3] summed across ranks (landmark shards), [4..6] camera terms
// (TS_TIMEOUT: 1.0 if this rank's persistent factorisation gave up -- it sits inside the all-reduced prefix of the block, so with
// several ranks every rank sees the NUMBER of ranks that timed out and they all take the recovery path together)
// Behind them: TS_SPEC_COST2, the cost of the speculative linearisation at the trial point (in the host's copy of the block: the
// factorisation's flag); then cost2 and |g|max of the LAST reduced-system build (ex_scalar, ex_gc), which the LM loop reads one
// iteration late -- outside the summed prefix, and equal on every rank (both come from the all-reduced extras).
enum { TS_COST2 = 0, TS_STEP2 = 1, TS_X2 = 2, TS_MODEL = 3, TS_TIMEOUT = 4, TS_CAM = 5, TS_COUNT = 8,
       TS_SPEC_COST2 = 8, TS_LIN_COST2 = 9, TS_LIN_GMAX = 10, TS_BLOCK = 11 };
// phase-timing events of a BA solve (stba_ba::ev; recorded only with stba_lm_options::phase_timing).  A pair is {X, X + 1}:
// the linearisation and the build the loop reads in the same iteration; the ends of the solve, the back-substitution and the trial
// evaluation; the two pairs the speculative linearisation alternates between; the build whose pair is read one solve later
// (ba_step_events).  stba_ba_time_linearize / _schur / _schur_apply borrow the first pair.
enum { EV_LIN = 0, EV_LIN_END, EV_BUILD, EV_BUILD_END, EV_SOLVE_END, EV_BACKSUB_END, EV_TRIAL_END,
       EV_SPEC_A, EV_SPEC_A_END, EV_SPEC_B, EV_SPEC_B_END, EV_DBUILD, EV_DBUILD_END, EV_COUNT };

// per-observation robust losses (stba_ba_set_loss): kind (STBA_LOSS_*), a, b, scale, each [n_obs] in the engine's
// order; kind null: no table.  With one, ba_linearize_robust_kernel writes the corrected r', J8 = {0, 0, Jp'} and Jc12 = Jc', and
// everything behind the linearisation runs its general form on them, as for host-linearised factors
struct LossTable {
    DevBuf<int> kind;
    DevBuf<double> a, b, scale;
};

// camera pose priors (stba_ba_set_pose_priors; ba_prior.hip): grouped by camera -- CSR over the cameras that have
// any, inside a group the caller's order -- with the poses (quaternions normalised) and the 6 x 6 square-root informations in
// that order; order: grouped position -> the caller's index
struct PriorSet {
    int n = 0, n_groups = 0;
    DevBuf<int> ptr, cam;
    DevBuf<double> pose, W;
    std::vector<int> order;
    PriorArgs args(const unsigned char* cam_fixed) const { return PriorArgs{n_groups, ptr, cam, pose, W, cam_fixed}; }
};

// camera-to-camera relative-pose factors (stba_ba_set_relative_poses; ba_between.hip): the edges in the caller's
// order and two CSRs of references into them, by camera (cg) and by unordered pair (pg)
struct BetweenSet {
    int n = 0, n_cg = 0, n_pg = 0;
    DevBuf<int> i, j, cg_ptr, cg_cam, cg_ref, pg_ptr, pg_ref;
    DevBuf<int2> pg_pair;
    DevBuf<double> meas, W;
    BetweenArgs args(const unsigned char* cam_fixed) const {
        return BetweenArgs{n, n_cg, n_pg, i, j, meas, W, cg_ptr, cg_cam, cg_ref, pg_ptr, pg_pair, pg_ref, cam_fixed};
    }
};

// landmark position priors (stba_ba_set_landmark_priors; ba_landmark_prior.hip): grouped by landmark -- start
// [n_pts + 1] over ALL landmarks, inside a group the caller's order -- with the landmark, the position and the 3 x 3 square-root
// information of every prior in that order; order: grouped position -> the caller's index; cost_part: the cost form's partials
// (landmark_prior_cost_grid(n) of them)
struct LandmarkPriorSet {
    int n = 0;
    DevBuf<int> start, pt;
    DevBuf<double> pos, W, cost_part;
    std::vector<int> order;
};

// inner iterations (stba_ba_set_inner_iterations; inner_iterations.hip): the ordering as per-group ranges of a
// camera list (with each entry's dof mask) and a landmark list, in ascending group id (plan: the host's copy, inner_plan.hpp; cam,
// pt, mask: the device's); the entries' iteration counts; the gate of the sweep behind a trial point, its two scalars {cost2 at x*,
// |x - x*|^2} and the partials of the latter; the events around a timed sweep (created by the first timed solve with inner
// iterations) and the summary of the last solve
struct InnerSet {
    bool on = false;
    double tol = 1e-3;
    InnerPlan plan;
    DevBuf<int> cam, pt, it, gate;
    DevBuf<unsigned char> mask;
    DevBuf<double> sc, part;
    DevEvent ev[2];
    stba_inner_summary sum{};
};

// ---- the owners of what used to be a flat member list.  (Hidden, like the cross-unit functions at the end of this header: the
// types are private to the BA host units, and their implicit members are no part of the library's dynamic symbols.)
#pragma GCC visibility push(hidden)

// THE layout of the cost partials, stated once: [0, lin_grid) the lineariser's workgroup partials, then ONE slot for every factor
// kind the engine holds, in this order: pose priors, relative poses, landmark priors.  The order is fixed: launch_sum_partials,
// launch_linear_finish and launch_trial_finish add the count() slots in index order, and the sums are compared bitwise.  A value
// made by stba_ba::cost_slots() for the factors held at that moment; ba_fill sizes cost_partial by capacity()
struct CostSlots {
    static constexpr int MAX_EXTRA = 3;       // one slot per factor kind
    static size_t capacity(int lin_grid) { return (size_t)lin_grid + MAX_EXTRA; }
    double* partial;
    int lin_grid;
    bool has_prior, has_between, has_lprior;
    double* pose_priors() const { return partial + lin_grid; }
    double* relative_poses() const { return pose_priors() + (has_prior ? 1 : 0); }
    double* landmark_priors() const { return relative_poses() + (has_between ? 1 : 0); }
    int count() const { return lin_grid + (has_prior ? 1 : 0) + (has_between ? 1 : 0) + (has_lprior ? 1 : 0); }
};

// The cross-rank sum of the reduced system (ba_allreduce.hip; several ranks hold one landmark shard each).  The hook, rank and world
// are stba_ba_set_allreduce's, which also forgets the pack plan: what travels is decided by the first build behind it
// (ba_plan_pack) and holds until the group changes.  Only the lower triangle of the n x n system travels (S is symmetric and only
// its lower triangle is ever read), followed by the four extras vectors: [tri n(n+1)/2 | ex_diag | ex_gc | rhs | scalars].  When the
// union over ranks of the non-zero 6x6 blocks is sparse (C5: 14 % of the camera pairs share a landmark), only those blocks travel:
// [blocks nz * 36 | extras] -- 20 MB instead of 144 MB at C5.  The event pair is created by the first timed sum; ms, bytes and
// calls accumulate over one solve (ba_solve_begin resets them, ba_solve_end reads them)
enum PackForm { PACK_UNPLANNED = 0, PACK_TRIANGLE = 1, PACK_BLOCKS = 2 };
struct CrossRankSum {
    stba_allreduce_fn fn = nullptr;
    void* user = nullptr;
    int rank = 0, world = 1;
    DevBuf<double> Spack;
    std::vector<int> h_row_col_ptr, h_row_cols;   // host copy of the local block pattern (lower triangle, by camera), from ba_fill
    PackForm form = PACK_UNPLANNED;
    int nz = 0;
    DevBuf<int2> blocks;        // (row camera, column camera) of every travelling block
    size_t pack_count(int n, int lda) const { return (form == PACK_BLOCKS ? (size_t)nz * 36 : (size_t)n * (n + 1) / 2) + 4 * (size_t)lda; }
    DevEvent ev[2];             // around the hook
    bool timing_pending = false, timing_on = false;
    double ms = 0.0, bytes = 0.0;
    int calls = 0;
    int stage_cooldown = 0;     // factorisations left that take the stage kernels (ba_on_chol_timeout: every rank counts the same ones)
};

// The Schur plan on the device: what build_schur_plan (schur_plan.hpp) made on the host, uploaded once by ba_fill and read by
// ba_schur_step ever after; the dense form's buffers come with the first dense step (ba_dense_alloc)
struct SchurDevicePlan {
    // task = (camera row, slice [lo, hi) of the row's column list)
    DevBuf<int> task_cam, cam_start, row_col_ptr, row_cols;
    DevBuf<int> task_col_lo, task_col_hi;
    int n_tasks = 0, max_cols = 0;
    // FEW camera rows (landmark-heavy problems): a task = (camera row, a RANGE of the camera's observation list), all columns of
    // the row; the slices of a row write partial blocks, ba_schur_reduce_slices_kernel adds them in order (see plan_rows, schur_plan.hpp)
    DevBuf<int> task_p_lo, task_p_hi, row_task_ptr, row_tasks;
    DevBuf<long long> task_part_off;
    DevBuf<double> part;
    bool lm_slices = false;
    std::shared_ptr<SchurPlan> create_leftovers;     // the host-side plan of ba_create, kept until the engine goes (see there)
    std::vector<unsigned char> create_omask;         // (the host copy of omask: kept, and freed, with it)
    // pair plan of the Schur kernel (see ba_schur_pairs_kernel)
    DevBuf<int> pair_begin, pair_end;      // per (task, wave)
    DevBuf<int> task_vs_ptr, vs_first;     // per task: first accumulator slot of every block of its slice (+ the slot count)
    int plan_mode = 0;                     // SchurArgs::mode the plan was built for
    DevBuf<int4> pair_rec;                 // (i, l, landmark, slot | flags)
    double pairs = 0.0, lds_atomics = 0.0;   // per launch of the Schur kernel (measurement)
    // the Schur complement as a dense symmetric product (dense visibility; ba_kernels.hip "DENSE visibility", stba_ba_set_schur_mode)
    int mode = STBA_SCHUR_PAIRS, mode_auto = STBA_SCHUR_PAIRS;
    bool have_pair_plan = false;
    DevBuf<double> Y; size_t ldy = 0, ykcols = 0;     // [lda][ldy]
    DevBuf<double> yv, yws;
    DevBuf<unsigned char> dup_run;                    // repeated (camera, landmark) pairs, per position of cam_perm (null: none)
    bool dup_overflow = false;                        // some pair has more than 255 observations: the DENSE form cannot take this problem
};

// The PCG of ITERATIVE_SCHUR (iterative_schur.hip): the options of stba_ba_set_pcg; the vectors r, z, p, q (x is dxc), one 6x6
// preconditioner inverse per camera, the chunk partials of the Schur-Jacobi blocks, three per-workgroup partial arrays and the solve's
// device state (ba_pcg_alloc, at creation); the stamped hand-off to the host (the first solve); the last solve's counts and the
// summary they are counted into once the LM loop keeps its step (ba_pcg_account)
struct PcgSet {
    int precond = STBA_PRECOND_JACOBI, min = 0, max = 500, check = 4;
    double eta = 0.1;
    stba_pcg_summary sum{};
    DevBuf<double> vec, minv, sj, part;
    DevBuf<PcgState> state;
    MappedBuffer host;
    double seq = 0.0;
    int last_it = 0, last_cap = 0;
    std::vector<int> per_iter;             // PCG iterations of every LM iteration of the last solve (1, 2, ...)
};

// DOGLEG (stba_ba_set_trust_region; dogleg.hip): the strategy stba_ba_solve runs; s .* u of cameras and landmarks, the terms
// kernel's partials, the six scalars and the step's stamped block for the host (ba_dogleg_alloc, the first DOGLEG solve); the summary
// of the last solve
struct DoglegSet {
    int trust_region = STBA_TR_LEVENBERG_MARQUARDT;
    DevBuf<double> uc, up, part, sc;
    MappedBuffer host;
    double seq = 0.0;
    stba_dogleg_summary sum{};
};

// host-linearised factors (stba_ba_set_host_linearizer): the user's cost functions make r and the 2x6 | 2x3 Jacobians on the host;
// J8 then holds {0, 0, Jp} per observation and Jc12 the camera blocks -- everything behind the linearisation is unchanged.  The
// vectors are ba_host_linearize's staging (caller order | engine order), sized by its first call
struct HostLinearizer {
    stba_ba_linearize_fn fn = nullptr;
    void* user = nullptr;
    std::vector<double> cams, pts, r, jc, jp, stage, cost_stage;
};

struct Damping {
    bool explicit_d = false;   // dc / dp were uploaded by the caller
    double radius = 1e4, dmin = 1e-6, dmax = 1e32;
    int use_scaling = 1;
};

#pragma GCC visibility pop

}  // namespace stba

using namespace stba;

// Teardown (ba_free, stba_engine.hip) is an ORDER, not ownership: the stream is synchronised first, the Cholesky's per-stream cache
// forgets it, the covariance store and the three MappedBuffers (plain data, no destructor: common.hpp) are released, an owned stream
// is destroyed, and only then `delete` runs the members' destructors.  So by the time a DevBuf or a DevEvent member destructs the
// stream has been synchronised: freeing buffers and destroying events races with nothing.  The events go AFTER the stream; that is
// fine for the same reason.  Nobody deletes an engine any other way.
struct stba_ba {
    int nc = 0, np = 0, no = 0, n = 0, lda = 0;
    hipStream_t st = nullptr;
    bool own_stream = false;
    std::vector<int> perm;   // sorted position -> caller's observation index
    // device
    DevBuf<double> cams[2], pts[2];
    int cur = 0;
    DevBuf<double2> feat;
    DevBuf<int> obs_cam, obs_pt, pt_start;
    DevBuf<int> cam_perm, chunk_begin, chunk_end, cam_chunk_start;
    int n_chunks = 0;
    SchurDevicePlan schur;
    DevBuf<unsigned char> cam_fixed, pt_fixed;
    DevBuf<double2> r;
    DevBuf<double> J8;            // compact Jacobian [n_obs][8] (ba_kernels.hip)
    HostLinearizer hl;
    DevBuf<double> Jc12;          // [n_obs][12]: the camera blocks of the general form (ba_wants_general_form)
    LossTable loss;
    // per-observation square-root information W_i (stba_ba_set_information / _sqrt_information): [n_obs][4], 2 x 2
    // row-major in the engine's order; null: the identity.  With it the same kernel whitens r, Jc, Jp in front of the corrector
    DevBuf<double> winfo;
    DevBuf<unsigned char> omask;  // per observation: constant dofs of its camera (bits 0..5) | constant landmark (bit 6); null if none
    DevBuf<double> Hpp6, gp, Hinv6, Rinv9, dp, scale_p;
    DevBuf<double> Hcc, gc, cam_partial, dc, scale_c;
    DevBuf<double> Sbuf;   // [S lda*lda | ex_diag lda | ex_gc lda | rhs lda | ex_scalar lda]
    DevBuf<double> dxc, dxp;
    DevBuf<double> cost_partial, upd_partial_c, upd_partial_p;      // (cost_partial: laid out by CostSlots)
    DevBuf<double> trial;   // TS_BLOCK doubles
    MappedBuffer ts_host;        // the trial block + the factorisation flag as a stamped block, written by a kernel
    double ts_seq = 0.0;         // sequence number of the last trial block asked for (the stamp of the block's lines)
    double ts_vals[TS_BLOCK] = {0};          // the host's copy of the last trial block (validated, or downloaded after a synchronise)
    DevBuf<int> flag;
    int lin_grid = 1;
    CrossRankSum ar;
    bool have_lin = false, have_blocks = false, have_reduced = false, have_dxc = false, have_dxp = false;
    bool scale_init = false;
    DevEvent ev[EV_COUNT];      // phase timing of a solve (the EV_ enum), created by ba_fill
    CovStore* cov = nullptr;    // the last stba_ba_covariance_compute (covariance.hip), until the next one, a release or destroy
    // ITERATIVE_SCHUR (stba_ba_create_ex; iterative_schur.hip): no S, no pair plan, no Y -- Sbuf holds only the extras tail
    bool iterative = false;
    PcgSet pcg;
    DoglegSet dl;
    InnerSet inner;
    // With priors the cost partials carry ONE more slot behind the lineariser's (CostSlots), filled by the cost form at every
    // linearisation; the block form adds to Hcc, gc behind the Schur step at lin_which, the parameter buffer the Jacobian records
    // were last made at
    PriorSet prior;
    int lin_which = 0;
    // With edges one more slot; the block form adds to Hcc, gc AND to the blocks (hi, lo) of S behind the Schur step
    BetweenSet btw;
    // With landmark priors one more slot again; the block form adds to Hpp6, gp right behind the landmark-block kernel
    // (ba_normal_blocks) and makes that kernel's max |gp| partials again, so that everything downstream sees the sum
    LandmarkPriorSet lprior;
    CostSlots cost_slots() const { return CostSlots{cost_partial, lin_grid, prior.n != 0, btw.n != 0, lprior.n != 0}; }
    int n_cost() const { return cost_slots().count(); }
    LandmarkPriorArgs landmark_prior_args() const { return LandmarkPriorArgs{lprior.n, np, lprior.start, lprior.pt, lprior.pos, lprior.W, pt_fixed}; }
    // the priors' rows for the model terms summed from the records (made at lin_which); no priors: start null, nothing is added
    LandmarkPriorRows landmark_prior_rows() const {
        return lprior.n ? LandmarkPriorRows{lprior.start, lprior.pos, lprior.W, pts[lin_which]} : LandmarkPriorRows{};
    }
    PriorArgs prior_args() const { return prior.args(cam_fixed); }
    BetweenArgs between_args() const { return btw.args(cam_fixed); }

    size_t s_count() const { return iterative ? 0 : (size_t)lda * lda; }
    double* S() const { return iterative ? nullptr : Sbuf; }
    double* ex_diag() const { return Sbuf + s_count(); }
    double* ex_gc() const { return Sbuf + s_count() + lda; }
    double* rhs() const { return Sbuf + s_count() + 2 * (size_t)lda; }
    double* ex_scalar() const { return Sbuf + s_count() + 3 * (size_t)lda; }
    size_t sbuf_count() const { return s_count() + 4 * (size_t)lda; }
};
namespace stba {

// nothing the stage entry points have made (linearisation, blocks, reduced system, steps) describes the engine any more
inline void ba_invalidate(stba_ba* b) { b->have_lin = b->have_blocks = b->have_reduced = b->have_dxc = b->have_dxp = false; }

inline void ba_drop_covariance(stba_ba* b) {
    cov_store_free(b->cov);
    b->cov = nullptr;
}

// the tail of every factor setter, in FRONT of the moves that free the old factors: nothing of the engine may still be reading them
// or what was linearised with them
inline int ba_factors_changed(stba_ba* b) {
    STBA_HIP(hipStreamSynchronize(b->st));
    ba_invalidate(b);
    ba_drop_covariance(b);
    return STBA_OK;
}

// who takes every kernel behind the linearisation in its GENERAL form (J8 = {0, 0, Jp}, Jc12 = the 2 x 6 camera blocks): host-
// linearised factors and engines with a loss table or weights.  Jc12 is allocated by the first setter that makes this true and
// released by the factor setter that makes it false (clearing the host lineariser keeps it)
inline bool ba_wants_general_form(bool host_linearizer, bool loss, bool information) { return host_linearizer || loss || information; }
inline bool ba_wants_general_form(const stba_ba* b) { return ba_wants_general_form(b->hl.fn != nullptr, b->loss.kind.get() != nullptr, b->winfo.get() != nullptr); }
// the camera blocks of the general form; null: the compact record
inline const double* ba_general_jc(const stba_ba* b) { return ba_wants_general_form(b) ? b->Jc12.get() : nullptr; }

// `who` asks for its feature (sets: it sets it, false: it clears it) on this engine: STBA_OK, or the refusal of ba_features.hpp
inline int ba_refuse(const stba_ba* b, const char* who, bool sets = true) {
    const unsigned held = ba_held_features(b->iterative, b->dl.trust_region == STBA_TR_TRADITIONAL_DOGLEG, b->inner.on,b->hl.fn != nullptr,
                                           b->ar.fn != nullptr, b->loss.kind.get() != nullptr, b->winfo.get() != nullptr, b->prior.n, b->btw.n, b->lprior.n);
    std::string why;
    const int code = ba_conflict(who, held, &why, sets);
    return code ? fail(code, why) : STBA_OK;
}

// From here on: what used to be file-local in one translation unit.  It crosses the BA host units now and stays out of the library's
// dynamic symbols all the same
#pragma GCC visibility push(hidden)

// what an ITERATIVE_SCHUR engine refuses for want of the explicit reduced system: the stage and measurement entry points, the
// covariance and stba_ba_set_schur_mode (the features it does not go together with are rows of ba_features.hpp)
inline int refuse_iterative(const stba_ba* b, const char* who, const char* why) {
    if (!b || !b->iterative) return STBA_OK;
    return fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": this engine uses ITERATIVE_SCHUR, " + why);
}

// ---- ba_linear.hip: the linear algebra of one iteration
// THE linearisation at parameter buffer `which` (host callback, robust or lossless kernel, then the three factor kinds' cost forms):
// the cost partials are left in cost_partial; with_jac: r, J8 (and Jc12) are stored
int ba_linearize_dispatch(stba_ba* b, int which, bool with_jac);
int ba_linearize(stba_ba* b, int which, double* cost2_dev);      // with Jacobians; the summed cost2 -> *cost2_dev
int ba_cost_only(stba_ba* b, int which, double* cost2_dev);      // residuals only; the summed cost2 -> *cost2_dev
int ba_linearize_lm(stba_ba* b, int which);                      // with Jacobians; ba_fill_scalar_slots adds the partials up
int ba_normal_blocks(stba_ba* b);                                // Hpp6, gp (landmark priors included)
int ba_camera_blocks(stba_ba* b);                                // Hcc, gc by the camera-side kernel (no Schur step)
int ba_prior_blocks(stba_ba* b);                                 // pose priors onto Hcc, gc
int ba_between_blocks(stba_ba* b, bool with_S);                  // relative-pose factors onto Hcc, gc (and S)
int ba_dense_alloc(stba_ba* b);                                  // Y and its workspaces, once
double* ba_rinv(stba_ba* b);
int ba_schur_step(stba_ba* b);
int ba_build_reduced(stba_ba* b, const Damping& dm);
int ba_build(stba_ba* b, const Damping& dm);                     // the explicit or the implicit build, by b->iterative
int ba_fill_scalar_slots(stba_ba* b, double* cost2_dev);
int ba_backsub_trial(stba_ba* b);
int ba_trial(stba_ba* b, double* host_out, bool updated = false, bool with_jac = false, double host_seq = 0.0);
int ba_read_linear_scalars(stba_ba* b, double* cost, double* gmax);
int ba_cov_build(stba_ba* b);
// the implicit-Schur driver (ITERATIVE_SCHUR)
PcgVecs pcg_vecs(stba_ba* b);
int ba_pcg_alloc(stba_ba* b);
int ba_is_landmark_pass(stba_ba* b, const double* x, const double* gp, PcgState* skip);
int ba_is_camera_pass(stba_ba* b, int mode, const double* p, double* y, double* pq_part, const PcgState* skip);
int ba_is_precond(stba_ba* b, int kind);
int ba_is_rhs(stba_ba* b);
int ba_pcg_solve(stba_ba* b, int* fail_out);
void ba_pcg_account(stba_ba* b, int lm_iter);

// ---- ba_allreduce.hip: the cross-rank sum of the reduced system
// S (lower triangle, or its travelling blocks) and the four extras vectors behind it, summed across ranks in place: pack, hook, unpack
int ba_allreduce_system(stba_ba* b);
void ba_collect_allreduce_time(stba_ba* b);

// ---- ba_solve.hip
void inner_summary_reset(stba_ba* b);

#pragma GCC visibility pop

}  // namespace stba
