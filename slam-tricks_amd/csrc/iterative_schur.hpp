// iterative_schur.hpp -- kernels of the ITERATIVE_SCHUR linear solver of the BA engine (definitions in iterative_schur.hip)
#pragma once
#include "common.hpp"

namespace stba {

// The reduced camera system S = (Hcc + D) - W V^-1 W^T is never formed.  One product y = S x is two passes over the observations:
//   landmark-major:  z_j = -V_j^-1 sum_i W_ij^T x_i   (ba_backsub_kernel with gp = 0, ba_kernels.hip)
//   camera-major:    y_i = (Hcc_i + D_i) x_i + sum_j W_ij z_j   (is_cam_gather_kernel over cam_perm chunks + is_cam_final_kernel)
// Constant camera dofs are not unknowns: their entries are zero in every vector of the solve.
constexpr int IS_CAMS_PER_WG = 32;                  // dof-parallel kernels: 6 lanes per camera, 192 lanes per workgroup
constexpr int IS_VEC_THREADS = 6 * IS_CAMS_PER_WG;
inline int is_vec_grid(int n_cams) { return (n_cams + IS_CAMS_PER_WG - 1) / IS_CAMS_PER_WG; }

// device state of one PCG solve (written by is_check_kernel alone, one workgroup; read by every other kernel of the solve)
struct PcgState {
    double rho, rho_old, q0, pad;
    int iter, done, fail, hit_cap;
};

enum { IS_FINAL_APPLY = 0, IS_FINAL_RHS = 1 };
enum { IS_VEC_INIT = 0, IS_VEC_DIR = 1, IS_VEC_UPDATE = 2, IS_VEC_PRECOND = 3 };
enum { IS_CHECK_INIT = 0, IS_CHECK_ITER = 1 };

// LM diagonal of the cameras without the reduced system: ex_diag = diag(Hcc), ex_gc = gc and (unless explicit_d) scale / dc with
// the arithmetic of ba_reduced_finalize_kernel, so that dc is bit-identical to the direct path's
int launch_is_cam_setup(int n_cams, const double* Hcc, const double* gc, double* ex_diag, double* ex_gc, double* scale, int init_scale,
                        int use_scaling, double radius, double dmin, double dmax, double* dc, int explicit_d, hipStream_t st);
// camera-major half of the product: per chunk of cam_perm the 6 sums sum Jc^T (Jp z_j) -> partial[chunk * 8 + a]
int launch_is_cam_gather(int n_chunks, const int* chunk_begin, const int* chunk_end, const int* cam_perm, const int* obs_pt,
                         const double* J8, const unsigned char* omask, const double* Jc12, const double* zp, const PcgState* state,
                         double* partial, hipStream_t st);
// APPLY: y = (Hcc + diag(dc)) p + sum of the chunk partials, pq_partial[wg] = p^T y over the workgroup's dofs;
// RHS:   y = -gc - sum of the chunk partials.  Constant dofs: y = 0.
int launch_is_cam_final(int n_cams, int mode, const int* cam_chunk_start, const double* partial, const double* Hcc, const double* dc,
                        const double* gc, const unsigned char* cam_fixed, const double* p, double* y, double* pq_partial,
                        const PcgState* state, hipStream_t st);
// per camera the Schur-Jacobi sums sum_j W_ij V_j^-1 W_ij^T (21 entries, lower triangle) of every chunk -> partial[chunk * 24 + k]
// (repeated observations of one (camera, landmark) pair are neighbours in cam_perm: W_ij is their sum)
int launch_is_sj_gather(int n_chunks, int n_obs, const int* chunk_begin, const int* chunk_end, const int* cam_perm, const int* obs_cam,
                        const int* obs_pt, const double* J8, const unsigned char* omask, const double* Jc12, const double* Hinv6,
                        double* partial, hipStream_t st);
// one 6x6 inverse per camera: IDENTITY diag(scale^2) (the identity in Jacobi-scaled coordinates), JACOBI (Hcc + D)^-1,
// SCHUR_JACOBI (Hcc + D - sum W V^-1 W^T)^-1; rows and columns of constant dofs zero
int launch_is_precond(int n_cams, int kind, const double* Hcc, const double* dc, const double* scale, const unsigned char* cam_fixed,
                      const int* cam_chunk_start, const double* sj_partial, double* Minv, hipStream_t st);
// the PCG vector steps (see iterative_schur.hip)
struct PcgVecs {
    double *x, *r, *z, *p, *q;
    const double* b;
    const double* Minv;
    double *part_rz, *part_pq, *part_q;      // one entry per workgroup of is_vec_grid(n_cams)
    PcgState* state;
};
int launch_is_vec(int n_cams, int op, const PcgVecs& v, hipStream_t st);
int launch_is_check(int n_cams, int op, const PcgVecs& v, double eta, int min_iterations, int max_iterations, hipStream_t st);
// {done, iterations, fail, hit_cap} as a stamped block in mapped host memory (common.hpp)
int launch_is_export(const PcgState* state, double* host_out, double seq, hipStream_t st);

}  // namespace stba
