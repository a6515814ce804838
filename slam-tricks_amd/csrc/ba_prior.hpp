// ba_prior.hpp -- camera pose priors of the bundle adjustment: the factor's maths (host and device) and the launch
// wrappers of its two kernels (definitions in ba_prior.hip)
#pragma once
#if defined(__HIPCC__)
#include "common.hpp"
#else
// a plain host compiler (tests/cpp/ba_between_driver.cpp): the factor's maths only, nothing of HIP
#include <cmath>
#define STBA_MATHS_ONLY
#ifndef __host__
#define __host__
#define __device__
#endif
#endif
#include "ba_factor_input.hpp"

namespace stba {

// A prior k on camera c: r = [Log(qh^-1 (x) q_c); t_c - th], order [rot(3), pos(3)] as cam_fixed and the columns of Jc;
// J = blockdiag(Jr^-1(r_theta), I) under the engine's chart q <- q (x) exp(d); whitened r' = W r, J' = W J, cost += |r'|^2 / 2.
//
// Log, the short way round.  dq = conj(qh) (x) q is formed WITHOUT contraction into FMAs, in a fixed order: for q == qh every
// imaginary part is then (w x - x w) + (-y z + z y) = 0 exactly (the products that cancel are paired), and q -> -q negates every product exactly, so that behind the sign
// choice the bits are the same.  theta = 2 atan2(|v|, w) with w >= 0 is well conditioned from 0 to pi (no acos, no division by a
// small sine); at w == 0 the sign of the axis is made canonical (first non-zero imaginary part positive).
// Returns in r[0..3) the rotation vector and in *cot_half = w / |v| (the cotangent of theta / 2, which the inverse Jacobian needs;
// unused below PRIOR_SERIES_THETA), in *theta the angle.
constexpr double PRIOR_SERIES_THETA = 0.1;     // below: the series of the phi^2 coefficient (its next term is 5e-20 there)
__host__ __device__ inline void prior_log(const double* qh, const double* q, double* r, double* theta, double* cot_half) {
#pragma clang fp contract(off)
    const double ax = -qh[0], ay = -qh[1], az = -qh[2], aw = qh[3];
    const double bx = q[0], by = q[1], bz = q[2], bw = q[3];
    double x = (aw * bx + ax * bw) + (ay * bz - az * by);
    double y = (aw * by + ay * bw) + (az * bx - ax * bz);
    double z = (aw * bz + az * bw) + (ax * by - ay * bx);
    double w = ((aw * bw - ax * bx) - ay * by) - az * bz;
    const double lead = x != 0.0 ? x : (y != 0.0 ? y : z);
    if (w < 0.0 || (w == 0.0 && lead < 0.0)) { x = -x; y = -y; z = -z; w = -w; }
    const double n2 = (x * x + y * y) + z * z;
    const double n = sqrt(n2);
    double k;
    if (n2 < 1e-40) { k = 2.0 / w; *cot_half = 0.0; }       // (atan2(n, w) / n = 1 / w to 1e-40 relative)
    else { k = 2.0 * atan2(n, w) / n; *cot_half = w / n; }
    r[0] = k * x; r[1] = k * y; r[2] = k * z;
    *theta = k * n;
}

// the coefficient c of Jr^-1(phi) = I + hat(phi) / 2 + c hat(phi)^2: c = 1 / th^2 - (1 + cos th) / (2 th sin th)
// = (1 - (th / 2) cot(th / 2)) / th^2, the second form free of the 0 / 0 of the first at th = pi; below PRIOR_SERIES_THETA its series
// (1 - x cot x loses th^2 / 12 of 1 to cancellation: eps / th^2 relative, which the c th^2 the matrix is made of turns into eps)
__host__ __device__ inline double prior_jrinv_coeff(double theta, double cot_half) {
#pragma clang fp contract(off)
    const double t2 = theta * theta;
    if (theta < PRIOR_SERIES_THETA)
        return 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 * (1.0 / 1209600.0 + t2 * (1.0 / 47900160.0))));
    return (1.0 - (0.5 * theta) * cot_half) / t2;
}

// Jr^-1(phi) [3][3] row-major: entry (k, a) = delta + hat(phi)(k, a) / 2 + c (phi_k phi_a - |phi|^2 delta)
__host__ __device__ inline void prior_jrinv(const double* p, double c, double* J) {
#pragma clang fp contract(off)
    const double t2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
    const double h[9] = {0.0, -p[2], p[1], p[2], 0.0, -p[0], -p[1], p[0], 0.0};
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) {
            const double d = k == a ? 1.0 : 0.0;
            J[k * 3 + a] = (d + 0.5 * h[k * 3 + a]) + c * (p[k] * p[a] - t2 * d);
        }
}

// the 6 residuals (not whitened) of one prior and Jr^-1 of its rotation part; cam, pose: [q(x, y, z, w), t]
__host__ __device__ inline void prior_residual(const double* pose, const double* cam, double* r, double* Jri) {
    double th, ch;
    prior_log(pose, cam, r, &th, &ch);
    for (int k = 0; k < 3; ++k) r[3 + k] = cam[4 + k] - pose[4 + k];
    if (Jri) prior_jrinv(r, prior_jrinv_coeff(th, ch), Jri);
}

// (the host's factorisation of a prior's information matrix, prior_information_factor, is in ba_factor_input.hpp)

#ifndef STBA_MATHS_ONLY
// the priors on the device, grouped by camera (CSR over the cameras that have any; inside a group the caller's order)
struct PriorArgs {
    int n_groups = 0;
    const int* group_ptr = nullptr;            // [n_groups + 1] into pose / W
    const int* group_cam = nullptr;            // [n_groups]
    const double* pose = nullptr;              // [n][7], quaternions normalised
    const double* W = nullptr;                 // [n][36] row-major square-root information
    const unsigned char* cam_fixed = nullptr;  // the engine's per-camera mask of constant dofs, or null
};
constexpr int PRIOR_THREADS = 256;             // both kernels
constexpr int PRIOR_CAMS_PER_WG = PRIOR_THREADS / 64;      // block form: one wave per camera that has priors
// cost form: sum over every prior of |r'|^2 at the cameras `cams` -> slot[0] (one workgroup: per group in the caller's order, the
// groups strided over the threads, one tree; no atomic)
int launch_prior_cost(const PriorArgs& a, const double* cams, double* slot, hipStream_t st);
// block form: Hcc[c] += sum J'^T J', gc[c] += sum J'^T r' at the cameras `cams` (Hcc, gc both given or both null); out_r [n][6] and
// out_J [n][36], in the grouped order, receive r' and J' when given
int launch_prior_blocks(const PriorArgs& a, const double* cams, double* Hcc, double* gc, double* out_r, double* out_J, hipStream_t st);
#endif

}  // namespace stba
