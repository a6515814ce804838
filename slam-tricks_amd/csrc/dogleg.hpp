// dogleg.hpp -- kernels of the DOGLEG trust-region strategy of the BA engine (definitions in dogleg.hip)
#pragma once
#include "common.hpp"
#include "dogleg_select.hpp"
#include "ba_landmark_prior.hpp"

namespace stba {

// the step's block for the host (stamped, common.hpp): what ba_dogleg_step_kernel chose, and the six scalars it chose it from
enum { DL_KASE = 0, DL_BETA = 1, DL_ZNORM = 2, DL_MODEL = 3, DL_GG = 4, DL_GZ = 5, DL_ZZ = 6, DL_UU = 7, DL_NN = 8, DL_UN = 9,
       DL_BLOCK = 10 };

struct DoglegArgs {
    int n_cams, n_pts;
    const int* pt_start; const int* obs_cam; const int* obs_pt;
    const double* J8; const unsigned char* omask; const double* Jc12;       // Jc12: host-linearised factors only (else null)
    const unsigned char* cam_fixed; const unsigned char* pt_fixed;
    const double* hc; const double* gc; const double* scale_c;              // diag(Hcc), gc (ex_diag, ex_gc) and the camera scale
    const double* Hpp6; const double* gp; const double* scale_p;            // landmark blocks, gradient and scale
    double dmin, dmax;                                                      // min_lm_diagonal, max_lm_diagonal
    const double* dxc; const double* dxp;                                   // the Gauss-Newton step delta_gn = s .* y_gn
    double* uc; double* up;                                                 // out: s .* u, u = gamma ./ d  [6 n_cams] | [3 n_pts]
    double* partial;                                                        // dogleg_partial_doubles(n_cams, n_pts)
    double* scalars;                                                        // out: DoglegScalars (6 doubles)
    LandmarkPriorRows lp{};                                                 // landmark priors: their rows of the three J^ sums; start null: none
};
size_t dogleg_partial_doubles(int n_cams, int n_pts);
// once per linearisation, behind the Gauss-Newton back-substitution: u, and the six scalars (fixed-order sums, no atomics)
int launch_dogleg_terms(const DoglegArgs& a, hipStream_t st);

struct DoglegStepArgs {
    int n_cams, n_pts;
    const double* scalars;                                   // the six scalars of launch_dogleg_terms
    const double* uc; const double* up; const double* dxc; const double* dxp;
    const double* cams; const double* pts; const unsigned char* cam_fixed; const unsigned char* pt_fixed;
    double* cams_new; double* pts_new;                       // the trial point
    double* partial_c; double* partial_p;                    // {|step|^2, |x|^2, model} per workgroup: backsub_cam_grid / backsub_grid of them
    double* host_out; double seq;                            // the step's stamped block (DL_BLOCK doubles of payload)
};
// every trial step: the step at radius Delta, the trial point and its step statistics, for launch_trial_finish
int launch_dogleg_step(const DoglegStepArgs& a, double radius, hipStream_t st);

}  // namespace stba
