// ba_kernels.hpp -- launch wrappers of the BA hot-path kernels (definitions in ba_kernels.hip)
#pragma once
#include "common.hpp"
#include "schur_plan.hpp"      // CAM_CHUNK and the SCHUR_* constants that the host-side plan shares with the kernels
#include "ba_landmark_prior.hpp"   // LandmarkPriorRows: the priors' rows of the two model terms summed from the records

namespace stba {

constexpr int LIN_THREADS = 1024;              // observations per workgroup tile
constexpr int LIN_MAX_LDS = 160 * 1024 - 512;  // dynamic LDS budget of the linearize kernel

struct LinArgs {
    int n_obs, n_cams;
    const double* cams;              // [n_cams][7]
    const double* pts;               // [n_pts][3]
    const double2* feat;             // [n_obs]
    const int* obs_cam;
    const int* obs_pt;
    const unsigned char* cam_fixed;  // [n_cams] bitmask (bit a = dof a constant) or null
    const unsigned char* pt_fixed;   // [n_pts] or null
    double2* r;                      // [n_obs]
    double* J8;                      // [n_obs][8] compact Jacobian {xn, yn, P 2x3} (see ba_kernels.hip)
    double* cost_partial;            // [grid]
};

// compact Jacobian of observation i -> the 2x6 camera block (d/dtheta | d/dt) and the 2x3 landmark block; columns of
// constant dofs (mask bits 0..5) and of constant landmarks (bit 6) are zero, as the stored form used to have them
// GEN (host-linearised factors, stba_ba_set_host_linearizer): the landmark block is still the record's P (so the landmark kernels
// need no second form), the camera block is NOT a function of it and comes from its own array Jc12 [n_obs][12] (2 x 6 row-major).
template <bool GEN = false>
__device__ inline void load_jc_jp(const double* __restrict__ J8, const unsigned char* __restrict__ omask, int i,
                                  double jc[12], double jp[6], const double* __restrict__ Jc12 = nullptr) {
    const double2* pj = reinterpret_cast<const double2*>(J8 + (size_t)i * 8);
    const double2 v0 = pj[0], v1 = pj[1], v2 = pj[2], v3 = pj[3];
    const unsigned m = omask ? omask[i] : 0u;
    if constexpr (GEN) {
        const double2* pc = reinterpret_cast<const double2*>(Jc12 + (size_t)i * 12);
        const double P[6] = {v1.x, v1.y, v2.x, v2.y, v3.x, v3.y};
        const bool pf = (m & 64u) != 0u;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double2 v = pc[k];
            jc[2 * k] = ((m >> ((2 * k) % 6)) & 1u) ? 0.0 : v.x;
            jc[2 * k + 1] = ((m >> ((2 * k + 1) % 6)) & 1u) ? 0.0 : v.y;
            jp[k] = pf ? 0.0 : P[k];
        }
        return;
    }
    const double xn = v0.x, yn = v0.y;
    const double P[6] = {v1.x, v1.y, v2.x, v2.y, v3.x, v3.y};
    jc[0] = (m & 1u) ? 0.0 : xn * yn;
    jc[1] = (m & 2u) ? 0.0 : -(1.0 + xn * xn);
    jc[2] = (m & 4u) ? 0.0 : yn;
    jc[6] = (m & 1u) ? 0.0 : 1.0 + yn * yn;
    jc[7] = (m & 2u) ? 0.0 : -xn * yn;
    jc[8] = (m & 4u) ? 0.0 : -xn;
    const bool pf = (m & 64u) != 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool fx = (m >> (3 + k)) & 1u;
        jc[3 + k] = fx ? 0.0 : -P[k];
        jc[9 + k] = fx ? 0.0 : -P[3 + k];
        jp[k] = pf ? 0.0 : P[k];
        jp[3 + k] = pf ? 0.0 : P[3 + k];
    }
}

size_t lin_lds_bytes(int n_cams, bool cams_in_lds, bool with_jac);
int launch_linearize(const LinArgs& a, bool with_jac, int grid, hipStream_t st);
// with a per-observation robust loss (stba_ba_set_loss): the table in the engine's observation order, and where the corrected camera
// blocks go -- the kernel writes the general form J8 = {0, 0, Jp'}, Jc12 = Jc' (ba_linearize_robust_kernel, ba_kernels.hip)
constexpr int LIN_ROBUST_THREADS = 512;        // observations per workgroup tile of the robust kernel
struct LinLoss {
    const int* kind;                 // [n_obs] STBA_LOSS_*
    const double* a;                 // [n_obs]
    const double* b;                 // [n_obs]
    const double* scale;             // [n_obs]
    double* Jc12;                    // [n_obs][12]
    const double* winfo;             // [n_obs][4] square-root information, 2 x 2 row-major; null: the identity
};
// (kind == null with winfo set: weights only, the table is not read)
size_t lin_robust_lds_bytes(int n_cams, bool cams_in_lds, bool with_jac);
bool lin_robust_cams_in_lds(int n_cams);
int launch_linearize_robust(const LinArgs& a, const LinLoss& l, bool with_jac, int grid, hipStream_t st);
int launch_sum_partials(const double* partial, int n, int stride, int K, double* out, hipStream_t st);
// (J8: compact Jacobian [n_obs][8]; omask: per-observation mask byte of constant dofs / landmarks, or null)
// (Jc12: the camera blocks of the general form -- host-linearised factors, robust losses -- or null)
int launch_expand_jacobian(int n_obs, const double* J8, const unsigned char* omask, double* Jc, double* Jp, hipStream_t st,
                           const double* Jc12 = nullptr);
// (gpmax_partial: optional, one max |gp| per workgroup of POINT_BLOCK_LANDMARKS landmarks, finished by launch_linear_finish)
constexpr int POINT_BLOCK_LANDMARKS = 32;
int point_blocks_grid(int n_pts);      // workgroups of the landmark-block kernel = entries of its gpmax partial array
int launch_point_blocks(int n_pts, const int* pt_start, const double* J8, const unsigned char* omask, const double2* r,
                        double* Hpp6, double* gp, double* gpmax_partial, hipStream_t st);
int launch_linear_finish(const double* cost_partial, int n_cost, const double* gpmax_partial, int n_gp, double* cost2_out,
                         double* slots, int n_slots, int cost_slot, int max_slot, hipStream_t st);
int launch_trial_finish(const double* cost_partial, int n_cost, const double* part_p, int n_p, const double* part_c, int n_c,
                        const int* flag, const double* lin_cost2, const double* gpmax, int n_gpmax, const double* gc, int n_g,
                        double* out, double* host_out, double host_seq, hipStream_t st);
int launch_camera_blocks(int n_cams, int n_chunks, const int* chunk_begin, const int* chunk_end,
                         const int* cam_chunk_start, const int* cam_perm, const double* J8, const unsigned char* omask,
                         const double* Jc12, const double2* r, double* partial, double* Hcc, double* gc, hipStream_t st);
int launch_lm_diagonal(int n, int bs, int bstride, int kind, const double* H, double* scale, int init_scale,
                       int use_scaling, double radius, double dmin, double dmax, double* d, hipStream_t st);
int launch_point_damp_invert(int n_pts, const double* Hpp6, const unsigned char* pt_fixed, double* scale, int init_scale,
                             int use_scaling, double radius, double dmin, double dmax, double* dp, double* Hinv6, double* Rinv9,
                             double* zero_buf, int zero_n, hipStream_t st);
// Hinv6 [n_pts][6] = (Hpp + diag(dp))^-1 packed, Rinv9 [n_pts][9] a root of it, R R^T = Hinv (row-major 3 x 3); both zero for a
// constant landmark and for a block that is not numerically positive definite (spd3_inverse, small_linalg.hpp); Rinv9 may be null (only the
// dense form of the Schur step reads it)
int launch_point_invert(int n_pts, const double* Hpp6, const double* dp, const unsigned char* pt_fixed,
                        double* Hinv6, double* Rinv9, hipStream_t st);
// Schur complement of the landmark blocks, row-wise with LDS accumulation (plan built on the host at create time:
// build_schur_plan, schur_plan.hpp, which also holds SCHUR_MAX_SLOTS, SCHUR_SPLIT_COLS, SCHUR_TASK_PAIRS and SCHUR_THREADS).
// LDS stride of one 6x6 accumulator block, in doubles: odd, so that the same entry of different blocks falls
// into different bank pairs (36 = 72 dwords = 8 mod 64 gave 8-way conflicts on every ds_add_f64: measured,
// the kernel was bound by them)
constexpr int SCHUR_BLK_LD = 37;
constexpr int SCHUR_CAM_LD = 56;      // per wave of a diagonal slice: 21 + 6 sums of the camera block, 21 + 6 of the pairs (i, i), padded
constexpr int SCHUR_ROTS = 6;        // column rotations of the Schur kernel's lanes (dealt per pair by the host: bits 16..18 of the record), see its pair loop
struct SchurArgs {
    const int* task_cam; const int* cam_start;       // camera row of the task; the camera's range of cam_perm
    const int* task_col_lo; const int* task_col_hi;  // the task's slice of its row's column list
    const int* row_col_ptr; const int* row_cols; int max_cols;
    const int* cam_perm;
    const double* J8; const unsigned char* omask;    // compact Jacobian [n_obs][8] | per-observation mask byte (or null)
    const double* Jc12 = nullptr;                    // host-linearised factors only: the camera blocks [n_obs][12] (then J8 holds {0, 0, Jp})
    const double2* r;
    const double* Hinv6; const double* gp;
    double* S; int lda; double* rhs;
    double* Hcc; double* gc;                         // camera blocks J_c^T J_c, J_c^T r: written by the slice that holds the diagonal block
    // every (observation i of the row's camera, observation l of the same landmark with camera(l) <= camera(i)) of the
    // slice, with the LDS slot of its 6x6 block resolved on the host
    const int* pair_begin; const int* pair_end;      // per (task, wave): every block is accumulated by one wave (bitwise reproducible)
    int mode = 0;                                    // 0: per-wave lists (slots dealt to waves) | 1: one list, waves add in turn (token) | 2: one list, arrival order
    const int* task_vs_ptr; const int* vs_first;     // per task: [blocks + 1] first accumulator slot of every block of the slice
    const int* obs_pt;                               // landmark of every observation
    const int4* pair_rec;                            // (i, l, landmark, slot | 0x8000 if diagonal block), l != i
    // round 6, landmark-range slices (few camera rows; null otherwise): the task's range of cam_perm, where it writes its partial
    // blocks [ncols * 36 | rhs 6 (+2) | camera sums 27 ...], and every row's tasks in the order ba_schur_reduce_slices_kernel adds them
    const int* task_p_lo = nullptr; const int* task_p_hi = nullptr; const long long* task_part_off = nullptr; double* part = nullptr;
    const int* row_task_ptr = nullptr; const int* row_tasks = nullptr; int n_cams = 0;
    int ablate = 0;
};
// the Schur complement for dense visibility as a symmetric rank-k product (ba_kernels.hip, "DENSE visibility")
struct SchurDenseArgs {
    int n_cams, n_chunks;                         // chunks of <= CAM_CHUNK observations of one camera (the camera-block machinery's)
    const int* chunk_begin; const int* chunk_end; const int* cam_chunk_start; const int* cam_perm;
    const int* obs_cam; const int* obs_pt;
    const double* J8; const unsigned char* omask; const double* Jc12; const double2* r;
    const double* Hinv6; const double* Rinv9; const double* gp;
    double* Y; size_t ldy; size_t kcols;         // [lda][ldy], kcols = 3 n_pts rounded up to 16 (<= ldy); zero where nothing is observed
    double* partial;                              // schur_dense_partial_doubles(n_chunks)
    const unsigned char* dup_run;                 // per position of cam_perm: repeated (camera, landmark) pairs (null: none), see the chunk kernel
    double* ws;                                   // workspace of chol_yyt_workspace_doubles(lda, kcols) doubles (or null)
    double* S; int lda; double* rhs; double* Hcc; double* gc;
};
size_t schur_dense_partial_doubles(int n_chunks);
int launch_schur_dense(const SchurDenseArgs& a, hipStream_t st);
size_t schur_rows_lds_bytes(int max_cols);
int launch_schur_rows(const SchurArgs& a, int n_tasks, hipStream_t st);
int launch_reduced_add_camera(int n_cams, const double* Hcc, const double* gc, double* S, int lda, double* rhs,
                              double* ex_diag, double* ex_gc, hipStream_t st);
int launch_reduced_finalize(int n_cams, int n, const double* Hcc, const double* gc, const unsigned char* cam_fixed, double* S, int lda,
                            double* rhs, double* ex_diag, double* ex_gc, double* scale, int init_scale, int use_scaling,
                            double radius, double dmin, double dmax, double* dc, int reduced, hipStream_t st);
int launch_reduced_damp(int n, const double* dc, const unsigned char* cam_fixed, double* S, int lda, double* rhs,
                        hipStream_t st);
// the landmark half of the trial point made by the back-substitution kernel itself (LM loop): pts_new = pts (+) dxp and one
// partial[4] = {|step|^2, |x|^2, model term, 0} per landmark workgroup of the launch (backsub_grid of them); all null: plain back-substitution
// (and the camera half, in extra workgroups behind the landmark ones, when cams_new is given: backsub_cam_grid partials)
struct BacksubUpdate {
    const double* pts; const unsigned char* pt_fixed; const double* dp;
    double* pts_new; double* partial_p;
    int n_cams; const double* cams; const unsigned char* cam_fixed; const double* gc; const double* dc;
    double* cams_new; double* partial_c;
    // iterative Schur (iterative_schur.hip): skip -- the PCG's device-side "done" flag (the kernel returns at once when it is set);
    // r_model -- the model change of an INEXACT step, m = -(J d)^T (r + J d / 2), from the records, r and the step (obs_pt: the
    // landmark of every record) in place of the exact-step term -1/2 g d + 1/2 d^T D d, which only holds for an exact solve
    const int* skip = nullptr;
    const double2* r_model = nullptr; const int* obs_pt = nullptr;
    // landmark priors: with r_model, their rows of that sum, -(W d_j)^T (r' + W d_j / 2) per prior; lp.start null: none
    LandmarkPriorRows lp{};
};
int backsub_grid(int n_pts);
int backsub_cam_grid(int n_cams);
int launch_backsub(int n_pts, const int* pt_start, const int* obs_cam, const double* J8, const unsigned char* omask,
                   const double* Hinv6, const double* gp, const double* dxc, double* dxp, hipStream_t st, const BacksubUpdate* up = nullptr,
                   const double* Jc12 = nullptr);
int launch_update(int n_cams, int n_pts, const double* cams, const double* pts, const double* dxc,
                  const double* dxp, const unsigned char* cam_fixed, const unsigned char* pt_fixed,
                  const double* gc, const double* dc, const double* gp, const double* dp, double* cams_new,
                  double* pts_new, double* partial_c, double* partial_p, hipStream_t st);
int launch_triangulate(int n_pts, const int* pt_start, const int* obs_cam, const double2* feat, const double* cams,
                       double* pts, const unsigned char* pt_fixed, int max_iter, hipStream_t st);

// ---- covariance (covariance.hip): Sigma_cc = S^-1 and the landmark marginals of a bundle adjustment at its current point
struct BaCovInputs {
    int nc, np, no, n, lda;
    hipStream_t st;
    const int* pt_start; const int* obs_cam;          // the engine's landmark-major observation order
    const double* J8; const double* Jc12;             // Jc12: host-linearised factors only (else null)
    const unsigned char* omask; const unsigned char* cam_fixed; const unsigned char* pt_fixed;
    const double* Hpp6; const double* Hinv6;          // undamped landmark blocks and their inverses
    const double* S;                                  // undamped reduced camera system (lower triangle), leading dimension lda
};
struct CovStore;
void cov_store_free(CovStore* c);
int cov_compute(const BaCovInputs& in, double min_rcond, CovStore** out, double* rcond_out);
int cov_camera_blocks(const CovStore* c, int n_pairs, const int* cam_a, const int* cam_b, double* out);
int cov_point_blocks(const CovStore* c, int n, const int* pts, double* out);
// the off-diagonal blocks of the full inverse: Sigma[cam[k], pt[k]] (6 x 3) and Sigma[pt_a[k], pt_b[k]] (3 x 3; pt_a == pt_b: the
// marginal of cov_point_blocks).  An index out of range: STBA_ERR_INVALID_ARGUMENT with the position named, nothing written
int cov_cam_point_blocks(const CovStore* c, int n_pairs, const int* cam, const int* pt, double* out);
int cov_point_pair_blocks(const CovStore* c, int n_pairs, const int* pt_a, const int* pt_b, double* out);
// inverse of the SPD matrix whose lower triangle is A (n x n, leading dimension lda, device) -> packed lower triangle sig (device,
// row i at i (i + 1) / 2); *rcond = smallest / largest Cholesky pivot over the rows that are not constant dofs (cam_fixed: bit a of
// byte i / 6 marks row i; may be null); *pivot_row = 0, or row + 1 of the first pivot that is not positive
int cov_spd_inverse_packed(const double* A, int lda, int n, const unsigned char* cam_fixed, double* sig, double* rcond, int* pivot_row,
                           hipStream_t st);

// ---- small dense problems (small_dense.hip): one kernel launch per LM step, pooled workspace, mapped host buffers
constexpr int SMALL_DENSE_MAX_N = 32;
struct SmallDenseWs;
bool small_dense_fits(int n_res, int n);
int small_dense_acquire(SmallDenseWs** ws, int n_res, int n);
void small_dense_release(SmallDenseWs* ws);
double* small_dense_J(SmallDenseWs* ws);     // where the residual callback writes J (n_res x n) and r (n_res): pinned, mapped
double* small_dense_r(SmallDenseWs* ws);
// H = J^T J, g = J^T r (relinearize) or the H, g of the last linearisation; Jacobi scaling fixed when `first`; solves
// (H + D(radius)) dx = -g.  dx, g: pointers into mapped host memory, valid until the next step.  pivot_flag: 0 or row + 1
int small_dense_step(SmallDenseWs* ws, int n_res, int n, bool relinearize, bool first, bool jacobi, double radius, double dmin,
                     double dmax, const double** dx, const double** g, double* model_change, int* pivot_flag);

}  // namespace stba
