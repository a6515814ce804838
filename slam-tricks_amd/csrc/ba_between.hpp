// ba_between.hpp -- camera-to-camera relative-pose factors of the bundle adjustment: the factor's maths (host and
// device) and the launch wrappers of its two kernels (definitions in ba_between.hip)
#pragma once
#include "ba_prior.hpp"

namespace stba {

// An edge k between the cameras i and j with the measurement (qz, tz) -- "camera j seen from camera i" -- and the 6 x 6 square-root
// information W; poses camera to world, chart q <- q (x) exp(dtheta), t <- t + dt, order [rot(3), pos(3)] as the priors:
//     r   = [ Log(qz^-1 (x) (q_i^-1 (x) q_j)) ; R_i^T (t_j - t_i) - tz ]
//     J_j = [ Jr^-1(r_theta)  0 ; 0  R_i^T ]        J_i = [ -Jr^-1(r_theta) R_j^T R_i  0 ; hat(R_i^T (t_j - t_i))  -R_i^T ]
//     r' = W r,  J_i' = W J_i,  J_j' = W J_j,  cost += |r'|^2 / 2
// ONE order of operations, none contracted into an FMA, which tests/ba_between_ref.py restates:
//   m = conj(q_i) (x) q_j in the paired order of prior_log's product; Log and Jr^-1 are the prior's (prior_log(qz, m), prior_jrinv);
//   R(q) = I + (2 / |q|^2) (...), |q|^2 = ((xx + yy) + zz) + ww: every entry is even in q;  R_j^T R_i = R(m)^T;
//   every 3-term product is (a0 b0 + a1 b1) + a2 b2, every whitening dot the six terms from the left, structural zeros included.
// Negating any one of qz, q_i, q_j negates every product of m or of conj(qz) (x) m exactly, which prior_log's sign choice undoes:
// the same bits.

// R(q) [3][3] row-major of a quaternion [x, y, z, w] of any non-zero length
__host__ __device__ inline void between_rot(const double* q, double* R) {
#pragma clang fp contract(off)
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double s = 2.0 / (((x * x + y * y) + z * z) + w * w);
    R[0] = 1.0 - s * (y * y + z * z); R[1] = s * (x * y - z * w);       R[2] = s * (x * z + y * w);
    R[3] = s * (x * y + z * w);       R[4] = 1.0 - s * (x * x + z * z); R[5] = s * (y * z - x * w);
    R[6] = s * (x * z - y * w);       R[7] = s * (y * z + x * w);       R[8] = 1.0 - s * (x * x + y * y);
}

// the 6 residuals (not whitened) of one edge and, when Jri is given, what its Jacobians are made of: Jri = Jr^-1(r_theta), Rm = R(m)
// (R_j^T R_i is its transpose), Ri = R(q_i), each [3][3] row-major, and v = R_i^T (t_j - t_i);  meas, ci, cj: [q(x, y, z, w), t]
__host__ __device__ inline void between_parts(const double* meas, const double* ci, const double* cj, double* r, double* Jri, double* Rm,
                                              double* Ri, double* v) {
#pragma clang fp contract(off)
    const double ax = -ci[0], ay = -ci[1], az = -ci[2], aw = ci[3];
    const double bx = cj[0], by = cj[1], bz = cj[2], bw = cj[3];
    double m[4];
    m[0] = (aw * bx + ax * bw) + (ay * bz - az * by);
    m[1] = (aw * by + ay * bw) + (az * bx - ax * bz);
    m[2] = (aw * bz + az * bw) + (ax * by - ay * bx);
    m[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
    double th, ch;
    prior_log(meas, m, r, &th, &ch);
    between_rot(ci, Ri);
    const double d0 = cj[4] - ci[4], d1 = cj[5] - ci[5], d2 = cj[6] - ci[6];
    for (int k = 0; k < 3; ++k) {
        v[k] = (Ri[k] * d0 + Ri[3 + k] * d1) + Ri[6 + k] * d2;
        r[3 + k] = v[k] - meas[4 + k];
    }
    if (!Jri) return;
    prior_jrinv(r, prior_jrinv_coeff(th, ch), Jri);
    between_rot(m, Rm);
}

// entry (a, b) of -Jr^-1 R(m)^T from row a of Jri and row b of Rm: THE order of this product (the kernel selects the rows, this adds)
__host__ __device__ inline double between_rot_entry(double j0, double j1, double j2, double m0, double m1, double m2) {
#pragma clang fp contract(off)
    return -((j0 * m0 + j1 * m1) + j2 * m2);
}

// the residuals and, when Ji is given, the two 6 x 6 Jacobians (row-major, not whitened, no mask)
__host__ __device__ inline void between_residual(const double* meas, const double* ci, const double* cj, double* r, double* Ji, double* Jj) {
    double Jri[9], Rm[9], Ri[9], v[3];
    between_parts(meas, ci, cj, r, Ji ? Jri : nullptr, Rm, Ri, v);
    if (!Ji) return;
    for (int k = 0; k < 36; ++k) Ji[k] = Jj[k] = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            Ji[a * 6 + b] = between_rot_entry(Jri[a * 3], Jri[a * 3 + 1], Jri[a * 3 + 2], Rm[b * 3], Rm[b * 3 + 1], Rm[b * 3 + 2]);
            Jj[a * 6 + b] = Jri[a * 3 + b];
            Ji[(3 + a) * 6 + 3 + b] = -Ri[b * 3 + a];
            Jj[(3 + a) * 6 + 3 + b] = Ri[b * 3 + a];
        }
    Ji[3 * 6 + 1] = -v[2]; Ji[3 * 6 + 2] = v[1];
    Ji[4 * 6 + 0] = v[2];  Ji[4 * 6 + 2] = -v[0];
    Ji[5 * 6 + 0] = -v[1]; Ji[5 * 6 + 1] = v[0];
}

// one whitening dot: row Wi[6] of W against x[0], x[stride], ...; the six terms from the left
__host__ __device__ inline double between_dot(const double* Wi, const double* x, int stride) {
#pragma clang fp contract(off)
    return ((((Wi[0] * x[0] + Wi[1] * x[stride]) + Wi[2] * x[2 * stride]) + Wi[3] * x[3 * stride]) + Wi[4] * x[4 * stride]) + Wi[5] * x[5 * stride];
}

// the whitened edge: r'[6], Ji'[36], Jj'[36] (any of the three may be null; the Jacobians go together); fixed_i / fixed_j: the
// cameras' masks of constant dofs (bit a: dof a), whose columns are exactly 0
__host__ __device__ inline void between_eval(const double* meas, const double* W, const double* ci, const double* cj, unsigned fixed_i,
                                             unsigned fixed_j, double* rw, double* Jiw, double* Jjw) {
    double r[6], Ji[36], Jj[36];
    between_residual(meas, ci, cj, r, Jiw ? Ji : nullptr, Jj);
    for (int i = 0; i < 6; ++i) {
        if (rw) rw[i] = between_dot(W + i * 6, r, 1);
        if (!Jiw) continue;
        for (int a = 0; a < 6; ++a) {
            Jiw[i * 6 + a] = ((fixed_i >> a) & 1u) ? 0.0 : between_dot(W + i * 6, Ji + a, 6);
            Jjw[i * 6 + a] = ((fixed_j >> a) & 1u) ? 0.0 : between_dot(W + i * 6, Jj + a, 6);
        }
    }
}

#ifndef STBA_MATHS_ONLY
// the edges on the device: the caller's order, and two CSRs of references into them.  A reference is 2 * edge + side.
//   by camera: the edges incident to a camera, side = 1 where the camera is the edge's j;
//   by unordered pair (hi, lo), hi > lo: side = 1 where hi is the edge's j.
// Inside a group the caller's order (a stable sort on the host)
struct BetweenArgs {
    int n = 0, n_cam_groups = 0, n_pair_groups = 0;
    const int* cam_i = nullptr;                // [n]
    const int* cam_j = nullptr;                // [n]
    const double* meas = nullptr;              // [n][7], quaternions normalised
    const double* W = nullptr;                 // [n][36] row-major square-root information
    const int* cg_ptr = nullptr;               // [n_cam_groups + 1] into cg_ref
    const int* cg_cam = nullptr;               // [n_cam_groups]
    const int* cg_ref = nullptr;               // [2 n]
    const int* pg_ptr = nullptr;               // [n_pair_groups + 1] into pg_ref
    const int2* pg_pair = nullptr;             // [n_pair_groups] (hi, lo)
    const int* pg_ref = nullptr;               // [n]
    const unsigned char* cam_fixed = nullptr;  // the engine's per-camera mask of constant dofs, or null
};
constexpr int BETWEEN_THREADS = 256;           // both kernels
constexpr int BETWEEN_GROUPS_PER_WG = BETWEEN_THREADS / 64;      // block form: one wave per camera group or pair group
// cost form: sum over every edge of |r'|^2 at the cameras `cams` -> slot[0] (one workgroup: thread t takes the edges t, t + 256, ...
// in the caller's order, one tree; no atomic)
int launch_between_cost(const BetweenArgs& a, const double* cams, double* slot, hipStream_t st);
// block form at the cameras `cams`, one launch.  Hcc, gc given (both or neither): Hcc[c] += sum J_x'^T J_x', gc[c] += sum J_x'^T r' per
// camera group.  S given: S[(6 hi + a) lda + 6 lo + b] += sum J_hi'^T J_lo' per pair group.  out_r [n][6], out_Ji, out_Jj [n][36], in the
// caller's order, receive r', J_i', J_j' when given (by the pair groups, which then run whether S is given or not)
int launch_between_blocks(const BetweenArgs& a, const double* cams, double* Hcc, double* gc, double* S, int lda, double* out_r,
                          double* out_Ji, double* out_Jj, hipStream_t st);
#endif

}  // namespace stba
