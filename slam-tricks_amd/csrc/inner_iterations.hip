// inner_iterations.hip -- the kernels of the inner-iteration sweep of the BA engine (Solver::Options::use_inner_iterations;
// DESIGN.md 7d), FP64, wave64.
//
// A sweep visits the groups of the ordering in ascending id; within a group every block is solved on its own, every other block
// held at its current value, by the Ceres LM of inner_policy.hpp with default options.  A group is an independent set -- no two of
// its blocks share a residual -- so its blocks run concurrently and the result is exactly the sequential one.
//   landmarks   one lane per landmark, its observations landmark-major (pt_start), the whole LM in registers
//   cameras     one workgroup per camera block (6 dof, or 3 through the dof mask), its observations camera-major (cam_perm and
//               the chunks of the camera-block kernels); every LM iteration is one pass that linearises and one pass per trial
//               cost, each reduced in LDS in a fixed order, and every lane runs the policy on the same sums
// Reproducibility: fixed-order sums, no floating-point atomics; a parameter is written by the one lane / workgroup that owns it.
#include "inner_iterations.hpp"

namespace stba {

// residual of one observation and, with J, the 2x6 camera block [d/dtheta | d/dt] (q <- q (x) exp(dtheta), t <- t + dt) and the
// 2x3 landmark block; the engine's projection (ba_linearize_kernel): p = R^T (L - t), r = p.xy / p.z - f
__device__ __forceinline__ void inner_obs(const double q[4], const double t[3], const double L[3], double2 f, double r[2],
                                          double* jc, double* jp) {
    double R[9];
    quat_to_rot(q, R);
    const double d0 = L[0] - t[0], d1 = L[1] - t[1], d2 = L[2] - t[2];
    const double x = R[0] * d0 + R[3] * d1 + R[6] * d2;
    const double y = R[1] * d0 + R[4] * d1 + R[7] * d2;
    const double z = R[2] * d0 + R[5] * d1 + R[8] * d2;
    const double iz = 1.0 / z, xn = x * iz, yn = y * iz;
    r[0] = xn - f.x; r[1] = yn - f.y;
    if (!jc && !jp) return;
    double P[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P[k] = iz * (R[k * 3 + 0] - xn * R[k * 3 + 2]);
        P[3 + k] = iz * (R[k * 3 + 1] - yn * R[k * 3 + 2]);
    }
    if (jp) for (int k = 0; k < 6; ++k) jp[k] = P[k];
    if (jc) {
        jc[0] = xn * yn; jc[1] = -(1.0 + xn * xn); jc[2] = yn;
        jc[6] = 1.0 + yn * yn; jc[7] = -xn * yn; jc[8] = -xn;
#pragma unroll
        for (int k = 0; k < 3; ++k) { jc[3 + k] = -P[k]; jc[9 + k] = -P[3 + k]; }
    }
}

// ---- landmarks: one lane per landmark of the group, cameras fixed
__global__ __launch_bounds__(INNER_PT_THREADS) void inner_points_kernel(InnerObs o, int n, const int* __restrict__ list,
                                                                        const double* __restrict__ cams, double* __restrict__ pts,
                                                                        int* __restrict__ it_pt, const int* __restrict__ gate) {
    if (gate && gate[0] == 0) return;
    const int k = blockIdx.x * INNER_PT_THREADS + threadIdx.x;
    if (k >= n) return;
    const int j = list[k];
    const int b = o.pt_start[j], e = o.pt_start[j + 1];
    if (e <= b) { it_pt[k] = 0; return; }
    double x[3] = {pts[(size_t)j * 3], pts[(size_t)j * 3 + 1], pts[(size_t)j * 3 + 2]};
    auto eval = [&](const double* L, double* H, double* g) -> double {
        double c = 0.0;
        if (H) { for (int a = 0; a < 9; ++a) H[a] = 0.0; g[0] = g[1] = g[2] = 0.0; }
        for (int i = b; i < e; ++i) {
            const double* cam = cams + (size_t)o.obs_cam[i] * 7;
            const double q[4] = {cam[0], cam[1], cam[2], cam[3]}, t[3] = {cam[4], cam[5], cam[6]};
            double r[2], jp[6];
            inner_obs(q, t, L, o.feat[i], r, nullptr, H ? jp : nullptr);
            c += r[0] * r[0] + r[1] * r[1];
            if (H) {
                for (int a = 0; a < 3; ++a) {
                    for (int bb = 0; bb < 3; ++bb) H[a * 3 + bb] += jp[a] * jp[bb] + jp[3 + a] * jp[3 + bb];
                    g[a] += jp[a] * r[0] + jp[3 + a] * r[1];
                }
            }
        }
        return 0.5 * c;
    };
    const inner::BlockOptions bo;
    const inner::BlockResult res = inner::block_lm<3, 3>(
        bo, 7u, x, [&](const double* L, double* H, double* g) { return eval(L, H, g); },
        [&](const double* L) { return eval(L, nullptr, nullptr); },
        [](const double* L, const double* d, double* Ln) { Ln[0] = L[0] + d[0]; Ln[1] = L[1] + d[1]; Ln[2] = L[2] + d[2]; },
        [](const double* L) { return L[0] * L[0] + L[1] * L[1] + L[2] * L[2]; },
        [](const double* L, const double* Ln) {
            const double a = L[0] - Ln[0], bb = L[1] - Ln[1], c = L[2] - Ln[2];
            return a * a + bb * bb + c * c;
        });
    pts[(size_t)j * 3] = x[0]; pts[(size_t)j * 3 + 1] = x[1]; pts[(size_t)j * 3 + 2] = x[2];
    it_pt[k] = res.iterations;
}

// the workgroup's sum of v[0..K) in a fixed order: wave shuffles, then the waves' sums in wave order; every lane gets the total
template <int K>
__device__ __forceinline__ void inner_wg_sum(double v[K], double (*s)[K]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double x = v[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0) s[w][k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double x = 0.0;
        for (int ww = 0; ww < INNER_CAM_THREADS / 64; ++ww) x += s[ww][k];
        v[k] = x;
    }
    __syncthreads();      // (s is reused by the next pass)
}

// ---- cameras: one workgroup per camera block of the group, landmarks fixed
__global__ __launch_bounds__(INNER_CAM_THREADS) void inner_cameras_kernel(InnerObs o, int n, const int* __restrict__ list,
                                                                          const unsigned char* __restrict__ mask,
                                                                          double* __restrict__ cams, const double* __restrict__ pts,
                                                                          int* __restrict__ it_cam, const int* __restrict__ gate) {
    if (gate && gate[0] == 0) return;
    const int k = blockIdx.x;
    if (k >= n) return;
    const int c = list[k];
    const unsigned m = mask[k];
    const int c0 = o.cam_chunk_start[c], c1 = o.cam_chunk_start[c + 1];
    if (c1 <= c0 || m == 0u) { if (threadIdx.x == 0) it_cam[k] = 0; return; }
    const int pb = o.chunk_begin[c0], pe = o.chunk_end[c1 - 1];
    __shared__ double s_lin[INNER_CAM_THREADS / 64][28];
    __shared__ double s_cost[INNER_CAM_THREADS / 64][1];
    const bool rot = (m & 7u) != 0u, pos = (m & 56u) != 0u;
    double x[7];
#pragma unroll
    for (int a = 0; a < 7; ++a) x[a] = cams[(size_t)c * 7 + a];
    // linearisation pass: H (lower triangle, 21) and g (6) of the camera's residuals, and the cost
    auto lin = [&](const double* X, double* H, double* g) -> double {
        double v[28];
#pragma unroll
        for (int a = 0; a < 28; ++a) v[a] = 0.0;
        const double q[4] = {X[0], X[1], X[2], X[3]}, t[3] = {X[4], X[5], X[6]};
        for (int p = pb + (int)threadIdx.x; p < pe; p += INNER_CAM_THREADS) {
            const int i = o.cam_perm[p];
            const int j = o.obs_pt[i];
            const double L[3] = {pts[(size_t)j * 3], pts[(size_t)j * 3 + 1], pts[(size_t)j * 3 + 2]};
            double r[2], jc[12];
            inner_obs(q, t, L, o.feat[i], r, jc, nullptr);
            int idx = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int bb = 0; bb <= a; ++bb) v[idx++] += jc[a] * jc[bb] + jc[6 + a] * jc[6 + bb];
#pragma unroll
            for (int a = 0; a < 6; ++a) v[21 + a] += jc[a] * r[0] + jc[6 + a] * r[1];
            v[27] += r[0] * r[0] + r[1] * r[1];
        }
        inner_wg_sum<28>(v, s_lin);
        int idx = 0;
        for (int a = 0; a < 6; ++a)
            for (int bb = 0; bb <= a; ++bb) { H[a * 6 + bb] = v[idx]; H[bb * 6 + a] = v[idx]; ++idx; }
        for (int a = 0; a < 6; ++a) g[a] = v[21 + a];
        return 0.5 * v[27];
    };
    // trial-cost pass
    auto cost_at = [&](const double* X) -> double {
        double v[1] = {0.0};
        const double q[4] = {X[0], X[1], X[2], X[3]}, t[3] = {X[4], X[5], X[6]};
        for (int p = pb + (int)threadIdx.x; p < pe; p += INNER_CAM_THREADS) {
            const int i = o.cam_perm[p];
            const int j = o.obs_pt[i];
            const double L[3] = {pts[(size_t)j * 3], pts[(size_t)j * 3 + 1], pts[(size_t)j * 3 + 2]};
            double r[2];
            inner_obs(q, t, L, o.feat[i], r, nullptr, nullptr);
            v[0] += r[0] * r[0] + r[1] * r[1];
        }
        inner_wg_sum<1>(v, s_cost);
        return 0.5 * v[0];
    };
    auto plus = [&](const double* X, const double* d, double* Xn) {
        if (rot) so3_plus(X, d, Xn);          // (a position-only block leaves q as it is: no renormalisation)
        else for (int a = 0; a < 4; ++a) Xn[a] = X[a];
        for (int a = 0; a < 3; ++a) Xn[4 + a] = pos ? X[4 + a] + d[3 + a] : X[4 + a];
    };
    auto norm2 = [&](const double* X) {
        double s = 0.0;
        if (rot) for (int a = 0; a < 4; ++a) s += X[a] * X[a];
        if (pos) for (int a = 4; a < 7; ++a) s += X[a] * X[a];
        return s;
    };
    auto dist2 = [&](const double* X, const double* Xn) {
        double s = 0.0;
        for (int a = 0; a < 7; ++a) { const double d = X[a] - Xn[a]; s += d * d; }
        return s;
    };
    const inner::BlockOptions bo;
    const inner::BlockResult res = inner::block_lm<6, 7>(bo, m, x, lin, cost_at, plus, norm2, dist2);
    if (threadIdx.x == 0) {
        for (int a = 0; a < 7; ++a) cams[(size_t)c * 7 + a] = x[a];
        it_cam[k] = res.iterations;
    }
}

int launch_inner_cameras(const InnerObs& o, int n, const int* list, const unsigned char* mask, double* cams, const double* pts,
                         int* it_cam, const int* gate, hipStream_t st) {
    if (n <= 0) return STBA_OK;
    hipLaunchKernelGGL(inner_cameras_kernel, dim3(n), dim3(INNER_CAM_THREADS), 0, st, o, n, list, mask, cams, pts, it_cam, gate);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

int launch_inner_points(const InnerObs& o, int n, const int* list, const double* cams, double* pts, int* it_pt, const int* gate,
                        hipStream_t st) {
    if (n <= 0) return STBA_OK;
    hipLaunchKernelGGL(inner_points_kernel, dim3((n + INNER_PT_THREADS - 1) / INNER_PT_THREADS), dim3(INNER_PT_THREADS), 0, st, o, n,
                       list, cams, pts, it_pt, gate);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

__global__ void inner_gate_kernel(const double* __restrict__ trial, const int* __restrict__ flag, int i_cost, int i_m0, int i_m1,
                                  int* __restrict__ gate) {
    if (threadIdx.x != 0) return;
    const double m = trial[i_m0] + trial[i_m1];
    gate[0] = (flag[0] == 0 && isfinite(trial[i_cost]) && isfinite(m) && m > 0.0) ? 1 : 0;
}

int launch_inner_gate(const double* trial, const int* flag, int i_cost, int i_m0, int i_m1, int* gate, hipStream_t st) {
    hipLaunchKernelGGL(inner_gate_kernel, dim3(1), dim3(64), 0, st, trial, flag, i_cost, i_m0, i_m1, gate);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

int inner_step_grid(int n_cams, int n_pts) {
    const long n = 7L * n_cams + 3L * n_pts;
    return (int)std::max(1L, std::min(256L, (n + 4 * INNER_STEP_THREADS - 1) / (4 * INNER_STEP_THREADS)));
}

__global__ __launch_bounds__(INNER_STEP_THREADS) void inner_step2_kernel(int n_cams, int n_pts, const double* __restrict__ cams0,
                                                                          const double* __restrict__ pts0, const double* __restrict__ cams1,
                                                                          const double* __restrict__ pts1, double* __restrict__ partial) {
    const long nc = 7L * n_cams, n = nc + 3L * n_pts;
    double v = 0.0;
    for (long i = (long)blockIdx.x * INNER_STEP_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * INNER_STEP_THREADS) {
        const double d = i < nc ? cams0[i] - cams1[i] : pts0[i - nc] - pts1[i - nc];
        v += d * d;
    }
    __shared__ double s[INNER_STEP_THREADS / 64];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < INNER_STEP_THREADS / 64; ++w) t += s[w];
        partial[blockIdx.x] = t;
    }
}

int launch_inner_step2(int n_cams, int n_pts, const double* cams0, const double* pts0, const double* cams1, const double* pts1,
                       double* partial, hipStream_t st) {
    hipLaunchKernelGGL(inner_step2_kernel, dim3(inner_step_grid(n_cams, n_pts)), dim3(INNER_STEP_THREADS), 0, st, n_cams, n_pts, cams0,
                       pts0, cams1, pts1, partial);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

}  // namespace stba
