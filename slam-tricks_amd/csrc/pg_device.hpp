// pg_device.hpp -- the device helpers that more than one pose-graph unit needs: the SE(3) helpers on 7-double poses and the
// fixed-order workgroup sums.  Everything here is inline; no kernel is declared or defined here.
// Internal linkage, as when these stood in the one unit that used them: the sums hold __shared__ arrays, which are laid out per
// kernel in the order of their mangled names -- with the names they had, every kernel keeps the LDS addresses (the code) it had.
#pragma once
#include "common.hpp"

namespace stba {
namespace {

// ---------------------------------------------------------------- SE3 helpers (7-double poses)
__host__ __device__ inline void quat_mul7(const double* a, const double* b, double* o) {
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
__host__ __device__ inline void rot_vec(const double* q, const double* v, double* o) {
    double R[9];
    quat_to_rot(q, R);
    for (int i = 0; i < 3; ++i) o[i] = R[i * 3] * v[0] + R[i * 3 + 1] * v[1] + R[i * 3 + 2] * v[2];
}
__host__ __device__ inline void se3_compose(const double* a, const double* b, double* out) {
    double q[4], t[3];
    quat_mul7(a, b, q);
    rot_vec(a, b + 4, t);
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) out[i] = q[i] / n;
    for (int i = 0; i < 3; ++i) out[4 + i] = t[i] + a[4 + i];
}
__host__ __device__ inline void se3_inverse(const double* a, double* out) {
    const double qc[4] = {-a[0], -a[1], -a[2], a[3]};
    double t[3];
    rot_vec(qc, a + 4, t);
    for (int i = 0; i < 4; ++i) out[i] = qc[i];
    for (int i = 0; i < 3; ++i) out[4 + i] = -t[i];
}
__host__ __device__ inline void hat3d(const double* v, double* M) {
    M[0] = 0; M[1] = -v[2]; M[2] = v[1]; M[3] = v[2]; M[4] = 0; M[5] = -v[0]; M[6] = -v[1]; M[7] = v[0]; M[8] = 0;
}
// Sophus SE3::log of (q, t) -> [rho, theta]
__host__ __device__ inline void se3_log7(const double* T, double* xi) {
    const double n2 = T[0] * T[0] + T[1] * T[1] + T[2] * T[2], qw = T[3];
    double k;
    if (n2 < 1e-20) k = 2.0 / qw - (2.0 / 3.0) * n2 / (qw * qw * qw);
    else { const double n = sqrt(n2); k = 2.0 * ((qw < 0) ? atan2(-n, -qw) : atan2(n, qw)) / n; }
    const double w[3] = {k * T[0], k * T[1], k * T[2]};
    double V[9];
    so3_left_jacobian(w, V);
    // rho = V^-1 t
    const double aa = V[0], bb = V[1], cc = V[2], dd = V[3], ee = V[4], ff = V[5], gg = V[6], hh = V[7], ii = V[8];
    const double C0 = ee * ii - ff * hh, C1 = ff * gg - dd * ii, C2 = dd * hh - ee * gg;
    const double inv = 1.0 / (aa * C0 + bb * C1 + cc * C2);
    const double* t = T + 4;
    xi[0] = inv * (C0 * t[0] + (cc * hh - bb * ii) * t[1] + (bb * ff - cc * ee) * t[2]);
    xi[1] = inv * (C1 * t[0] + (aa * ii - cc * gg) * t[1] + (cc * dd - aa * ff) * t[2]);
    xi[2] = inv * (C2 * t[0] + (bb * gg - aa * hh) * t[1] + (aa * ee - bb * dd) * t[2]);
    xi[3] = w[0]; xi[4] = w[1]; xi[5] = w[2];
}
__host__ __device__ inline void se3_retract(const double* T, const double* d, double* out) {
    double e[7], R[9];
    so3_exp(d + 3, e);
    se3_exp_rt(d, R, e + 4);
    se3_compose(T, e, out);
}

// ---------------------------------------------------------------- workgroup sums, fixed order
// out2 = {sum a, sum b} over a workgroup of 256 threads, in thread 0
__device__ inline void block_sum2(double a, double b, double* out2) {
    __shared__ double s[2][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if (lane == 0) { s[0][w] = a; s[1][w] = b; }
    __syncthreads();
    if (threadIdx.x == 0) { out2[0] = s[0][0] + s[0][1] + s[0][2] + s[0][3]; out2[1] = s[1][0] + s[1][1] + s[1][2] + s[1][3]; }
}

// sum of nb per-workgroup partials, by the WHOLE workgroup (256 threads): a strided share per thread, a shuffle tree per
// wave, the four waves in order -- the same order in every workgroup and on every rank, so every one of them gets the same
// bits.  (Every thread summing all partials serially -- 275 dependent loads -- made pg_pcg_update_kernel 27.5 us long, 40 %
// of a PCG iteration: profiles/r3_a_c4_kernel_stats.csv.)
__device__ inline double sum_partials_dev(const double* partial, int nb, int stride, int off) {
    __shared__ double s_w[4];
    __shared__ double s_tot;
    double v = 0.0;
    for (int k = threadIdx.x; k < nb; k += 256) v += partial[k * stride + off];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();                                     // (the shared slots may still be read from a previous call)
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) s_tot = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
    __syncthreads();
    return s_tot;
}

// sum of nb per-workgroup partials by a workgroup of NT threads, fixed order (same bits in every workgroup and on every rank)
template <int NT>
__device__ inline double sum_partials_n(const double* partial, int nb, int stride, int off) {
    __shared__ double s_w[NT / 64];
    __shared__ double s_tot;
    double v = 0.0;
    for (int k = threadIdx.x; k < nb; k += NT) v += partial[k * stride + off];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0.0; for (int w = 0; w < NT / 64; ++w) t += s_w[w]; s_tot = t; }
    __syncthreads();
    return s_tot;
}
template <int NT>
__device__ inline void block_sum2_n(double a, double b, double* out2) {
    __shared__ double s[2][NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    __syncthreads();
    if (lane == 0) { s[0][w] = a; s[1][w] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double x = 0.0, y = 0.0;
        for (int k = 0; k < NT / 64; ++k) { x += s[0][k]; y += s[1][k]; }
        out2[0] = x; out2[1] = y;
    }
}

}  // namespace
}  // namespace stba
