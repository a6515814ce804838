// inner_iterations.hpp -- kernels of the inner-iteration sweep of the BA engine (Ceres' use_inner_iterations: a coordinate-descent
// sweep over independent groups of parameter blocks, every block solved by its own small LM; definitions in inner_iterations.hip,
// DESIGN.md 7d)
#pragma once
#include "common.hpp"
#include "inner_policy.hpp"

namespace stba {

constexpr int INNER_CAM_THREADS = 256;     // one workgroup per camera block
constexpr int INNER_PT_THREADS = 64;       // one lane per landmark
constexpr int INNER_STEP_THREADS = 256;

// the observations, landmark-major (as the engine keeps them) and camera-major (cam_perm + the camera-block chunks)
struct InnerObs {
    int n_cams, n_pts;
    const int* pt_start; const int* obs_cam; const int* obs_pt; const double2* feat;
    const int* cam_perm; const int* chunk_begin; const int* chunk_end; const int* cam_chunk_start;
};

// one group: cameras list[k] with dof mask[k] (bits 0..2 rotation, 3..5 position, constant dofs already removed), landmarks
// list[k]; the inner LM iteration count of every entry -> it_cam[k] | it_pt[k].  gate: null, or a device int that is 0 when the
// sweep is not to run (the trial point is not valid): every workgroup returns at once.
int launch_inner_cameras(const InnerObs& o, int n, const int* list, const unsigned char* mask, double* cams, const double* pts,
                         int* it_cam, const int* gate, hipStream_t st);
int launch_inner_points(const InnerObs& o, int n, const int* list, const double* cams, double* pts, int* it_pt, const int* gate,
                        hipStream_t st);
// gate = 1 if the trial block says the step is valid: flag 0, trial[i_cost] finite, model change trial[i_m0] + trial[i_m1]
// positive and finite
int launch_inner_gate(const double* trial, const int* flag, int i_cost, int i_m0, int i_m1, int* gate, hipStream_t st);
// |x - x*|^2 over every camera (7) and landmark (3) entry -> partial[inner_step_grid()] ; added by launch_sum_partials
int inner_step_grid(int n_cams, int n_pts);
int launch_inner_step2(int n_cams, int n_pts, const double* cams0, const double* pts0, const double* cams1, const double* pts1,
                       double* partial, hipStream_t st);

}  // namespace stba
