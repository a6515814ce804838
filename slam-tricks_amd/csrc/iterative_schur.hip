// iterative_schur.hip -- the ITERATIVE_SCHUR linear solver of the BA engine: preconditioned conjugate gradients on the reduced
// camera system S = (Hcc + D) - W V^-1 W^T, applied implicitly (Ceres' ImplicitSchurComplement), FP64, wave64.
//
// Stop rule: Ceres' LevenbergMarquardtStrategy + ConjugateGradientsSolver -- q_tolerance = eta with Nash & Sofer's test
//   i (Q_i - Q_{i-1}) / Q_i <= eta,   Q_i = -1/2 x_i^T (b + r_i)   (the quadratic model of the reduced system at x_i),
// the residual test switched off (r_tolerance < 0), at least min and at most max iterations; p^T S p <= 0 ends the solve with the
// iterate so far (NO_CONVERGENCE), a non-finite alpha or r^T z = 0 makes it fail (FAILURE: the LM step is not ok).  The decision is
// taken on the device by is_check_kernel; the host enqueues check_every iterations at a time and reads the flag through a stamped
// block (common.hpp).  Every kernel of an iteration returns at once once the flag is set.
//
// Reproducibility: every sum is a fixed-order tree of per-workgroup partials (no floating-point atomics); a scalar that several
// workgroups need is reduced by each of them from the same partials in the same order, so they all hold the same bits.
#include "ba_kernels.hpp"
#include "iterative_schur.hpp"

namespace stba {

// sum over the IS_VEC_THREADS lanes of the workgroup (three waves, added in wave order); every lane gets the result
__device__ inline double is_block_sum(double v, double* sh) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = sh[0] + sh[1] + sh[2];
    __syncthreads();
    return s;
}
// the sum of n per-workgroup partials, in the same order in every workgroup that asks
__device__ inline double is_sum_partials(const double* __restrict__ part, int n, double* sh) {
    double v = 0.0;
    for (int k = threadIdx.x; k < n; k += IS_VEC_THREADS) v += part[k];
    return is_block_sum(v, sh);
}

__global__ __launch_bounds__(256) void is_cam_setup_kernel(int n, const double* __restrict__ Hcc, const double* __restrict__ gc,
                                                           double* __restrict__ ex_diag, double* __restrict__ ex_gc, double* __restrict__ scale,
                                                           int init_scale, int use_scaling, double radius, double dmin, double dmax,
                                                           double* __restrict__ dc, int explicit_d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = i / 6, a = i - c * 6;
    const double h = Hcc[(size_t)c * 36 + a * 7];
    ex_diag[i] = h;
    ex_gc[i] = gc[i];
    if (explicit_d) return;
    // (ba_reduced_finalize_kernel's LM diagonal, the same operations)
    double sc = 1.0;
    if (use_scaling) {
        if (init_scale) { sc = 1.0 / (1.0 + sqrt(h)); scale[i] = sc; }
        else sc = scale[i];
    } else if (init_scale) scale[i] = 1.0;
    const double s2 = sc * sc;
    const double v = fmin(fmax(h * s2, dmin), dmax);
    dc[i] = v / radius / s2;
}

int launch_is_cam_setup(int n_cams, const double* Hcc, const double* gc, double* ex_diag, double* ex_gc, double* scale, int init_scale,
                        int use_scaling, double radius, double dmin, double dmax, double* dc, int explicit_d, hipStream_t st) {
    const int n = 6 * n_cams;
    hipLaunchKernelGGL(is_cam_setup_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, Hcc, gc, ex_diag, ex_gc, scale, init_scale,
                       use_scaling, radius, dmin, dmax, dc, explicit_d);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

// one wave per chunk of <= CAM_CHUNK observations of one camera (the camera-block kernel's layout): lane-strided sums of
// Jc^T (Jp z_j), a shuffle tree, lane 0 writes the chunk's six sums.  Bytes per observation: the 64 B record, 4 B of cam_perm,
// 4 B of obs_pt and the landmark's 24 B of z (gathered; shared by the landmark's observations in the caches).
template <bool GEN>
__global__ __launch_bounds__(256) void is_cam_gather_kernel(int n_chunks, const int* __restrict__ chunk_begin, const int* __restrict__ chunk_end,
                                                            const int* __restrict__ cam_perm, const int* __restrict__ obs_pt,
                                                            const double* __restrict__ J8, const unsigned char* __restrict__ omask,
                                                            const double* __restrict__ Jc12, const double* __restrict__ zp,
                                                            const PcgState* __restrict__ state, double* __restrict__ partial) {
    if (state && state->done) return;
    const int lane = threadIdx.x & 63;
    const int ch = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ch >= n_chunks) return;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int e = chunk_end[ch];
    for (int p = chunk_begin[ch] + lane; p < e; p += 64) {
        const int i = cam_perm[p];
        const int j = obs_pt[i];
        double jc[12], jp[6];
        load_jc_jp<GEN>(J8, omask, i, jc, jp, Jc12);
        const double z0 = zp[(size_t)j * 3], z1 = zp[(size_t)j * 3 + 1], z2 = zp[(size_t)j * 3 + 2];
        const double v0 = jp[0] * z0 + jp[1] * z1 + jp[2] * z2;
        const double v1 = jp[3] * z0 + jp[4] * z1 + jp[5] * z2;
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] += jc[a] * v0 + jc[6 + a] * v1;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double v = acc[a];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        acc[a] = v;
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 6; ++a) partial[(size_t)ch * 8 + a] = acc[a];
    }
}

int launch_is_cam_gather(int n_chunks, const int* chunk_begin, const int* chunk_end, const int* cam_perm, const int* obs_pt,
                         const double* J8, const unsigned char* omask, const double* Jc12, const double* zp, const PcgState* state,
                         double* partial, hipStream_t st) {
    if (n_chunks > 0) {
        if (Jc12) hipLaunchKernelGGL(is_cam_gather_kernel<true>, dim3((n_chunks + 3) / 4), dim3(256), 0, st, n_chunks, chunk_begin, chunk_end,
                                     cam_perm, obs_pt, J8, omask, Jc12, zp, state, partial);
        else hipLaunchKernelGGL(is_cam_gather_kernel<false>, dim3((n_chunks + 3) / 4), dim3(256), 0, st, n_chunks, chunk_begin, chunk_end,
                                cam_perm, obs_pt, J8, omask, Jc12, zp, state, partial);
    }
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

// one lane per camera dof: the chunk partials of its camera in chunk order, the camera's own block, and (APPLY) p^T y of the workgroup
__global__ __launch_bounds__(IS_VEC_THREADS) void is_cam_final_kernel(int n_cams, int mode, const int* __restrict__ cam_chunk_start,
                                                                      const double* __restrict__ partial, const double* __restrict__ Hcc,
                                                                      const double* __restrict__ dc, const double* __restrict__ gc,
                                                                      const unsigned char* __restrict__ cam_fixed, const double* __restrict__ p,
                                                                      double* __restrict__ y, double* __restrict__ pq_partial,
                                                                      const PcgState* __restrict__ state) {
    __shared__ double sh[4];
    if (state && state->done) return;
    const int t = threadIdx.x;
    const int c = blockIdx.x * IS_CAMS_PER_WG + t / 6, a = t % 6;
    double yi = 0.0, pi = 0.0;
    if (c < n_cams) {
        const size_t i = (size_t)c * 6 + a;
        double s = 0.0;
        const int e = cam_chunk_start[c + 1];
        for (int ch = cam_chunk_start[c]; ch < e; ++ch) s += partial[(size_t)ch * 8 + a];
        if (mode == IS_FINAL_APPLY) {
            const double* H = Hcc + (size_t)c * 36 + a * 6;
            const double* pc = p + (size_t)c * 6;
            double h = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) h += H[k] * pc[k];
            pi = pc[a];
            yi = h + dc[i] * pi + s;
        } else {
            yi = -gc[i] - s;
        }
        if (cam_fixed && ((cam_fixed[c] >> a) & 1u)) { yi = 0.0; pi = 0.0; }
        y[i] = yi;
    }
    if (mode == IS_FINAL_APPLY && pq_partial) {
        const double v = is_block_sum(pi * yi, sh);
        if (t == 0) pq_partial[blockIdx.x] = v;
    }
}

int launch_is_cam_final(int n_cams, int mode, const int* cam_chunk_start, const double* partial, const double* Hcc, const double* dc,
                        const double* gc, const unsigned char* cam_fixed, const double* p, double* y, double* pq_partial,
                        const PcgState* state, hipStream_t st) {
    hipLaunchKernelGGL(is_cam_final_kernel, dim3(is_vec_grid(n_cams)), dim3(IS_VEC_THREADS), 0, st, n_cams, mode, cam_chunk_start, partial,
                       Hcc, dc, gc, cam_fixed, p, y, pq_partial, state);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

// Schur-Jacobi blocks, camera-major: a lane takes the first observation of every run of one (camera, landmark) pair, sums the run's
// W = Jc^T Jp (6x3) and adds W V^-1 W^T (21 entries) to its share; a shuffle tree per chunk
template <bool GEN>
__global__ __launch_bounds__(256) void is_sj_gather_kernel(int n_chunks, int n_obs, const int* __restrict__ chunk_begin,
                                                           const int* __restrict__ chunk_end, const int* __restrict__ cam_perm,
                                                           const int* __restrict__ obs_cam, const int* __restrict__ obs_pt,
                                                           const double* __restrict__ J8, const unsigned char* __restrict__ omask,
                                                           const double* __restrict__ Jc12, const double* __restrict__ Hinv6,
                                                           double* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int ch = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ch >= n_chunks) return;
    double acc[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) acc[k] = 0.0;
    const int e = chunk_end[ch];
    for (int p = chunk_begin[ch] + lane; p < e; p += 64) {
        const int i = cam_perm[p];
        const int c = obs_cam[i], j = obs_pt[i];
        if (p > 0) {
            const int i0 = cam_perm[p - 1];
            if (obs_cam[i0] == c && obs_pt[i0] == j) continue;      // (not the first of its run)
        }
        double W[18];
#pragma unroll
        for (int k = 0; k < 18; ++k) W[k] = 0.0;
        for (int q = p; q < n_obs; ++q) {
            const int iq = cam_perm[q];
            if (q > p && (obs_cam[iq] != c || obs_pt[iq] != j)) break;
            double jc[12], jp[6];
            load_jc_jp<GEN>(J8, omask, iq, jc, jp, Jc12);
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int k = 0; k < 3; ++k) W[a * 3 + k] += jc[a] * jp[k] + jc[6 + a] * jp[3 + k];
        }
        const double* h = Hinv6 + (size_t)j * 6;          // packed xx xy xz yy yz zz
        const double H[9] = {h[0], h[1], h[2], h[1], h[3], h[4], h[2], h[4], h[5]};
        double T[18];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) T[a * 3 + k] = W[a * 3] * H[k] + W[a * 3 + 1] * H[3 + k] + W[a * 3 + 2] * H[6 + k];
        int idx = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) acc[idx++] += T[a * 3] * W[b * 3] + T[a * 3 + 1] * W[b * 3 + 1] + T[a * 3 + 2] * W[b * 3 + 2];
    }
#pragma unroll
    for (int k = 0; k < 21; ++k) {
        double v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        acc[k] = v;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 21; ++k) partial[(size_t)ch * 24 + k] = acc[k];
    }
}

int launch_is_sj_gather(int n_chunks, int n_obs, const int* chunk_begin, const int* chunk_end, const int* cam_perm, const int* obs_cam,
                        const int* obs_pt, const double* J8, const unsigned char* omask, const double* Jc12, const double* Hinv6,
                        double* partial, hipStream_t st) {
    if (n_chunks > 0) {
        if (Jc12) hipLaunchKernelGGL(is_sj_gather_kernel<true>, dim3((n_chunks + 3) / 4), dim3(256), 0, st, n_chunks, n_obs, chunk_begin,
                                     chunk_end, cam_perm, obs_cam, obs_pt, J8, omask, Jc12, Hinv6, partial);
        else hipLaunchKernelGGL(is_sj_gather_kernel<false>, dim3((n_chunks + 3) / 4), dim3(256), 0, st, n_chunks, n_obs, chunk_begin,
                                chunk_end, cam_perm, obs_cam, obs_pt, J8, omask, Jc12, Hinv6, partial);
    }
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

// one camera per lane: the 6x6 block, constant dofs replaced by identity rows, Cholesky, the inverse as L^-T L^-1, constant
// rows and columns zeroed.  A block that is not positive definite (cannot happen with D > 0 in exact arithmetic) falls back to
// the inverse of its diagonal.
__global__ __launch_bounds__(64) void is_precond_kernel(int n_cams, int kind, const double* __restrict__ Hcc, const double* __restrict__ dc,
                                                        const double* __restrict__ scale, const unsigned char* __restrict__ cam_fixed,
                                                        const int* __restrict__ cam_chunk_start, const double* __restrict__ sj,
                                                        double* __restrict__ Minv) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_cams) return;
    const unsigned m = cam_fixed ? cam_fixed[c] : 0u;
    double* out = Minv + (size_t)c * 36;
    if (kind == STBA_PRECOND_IDENTITY) {
        // the identity in Jacobi-scaled coordinates (Ceres scales the Jacobian's columns; here the unknowns stay unscaled)
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double s = scale[(size_t)c * 6 + a];
#pragma unroll
            for (int b = 0; b < 6; ++b) out[a * 6 + b] = (a == b && !((m >> a) & 1u)) ? s * s : 0.0;
        }
        return;
    }
    double A[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) A[k] = Hcc[(size_t)c * 36 + k];
#pragma unroll
    for (int a = 0; a < 6; ++a) A[a * 7] += dc[(size_t)c * 6 + a];
    if (kind == STBA_PRECOND_SCHUR_JACOBI) {
        const int e = cam_chunk_start[c + 1];
        for (int ch = cam_chunk_start[c]; ch < e; ++ch) {
            int idx = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = 0; b <= a; ++b) {
                    const double v = sj[(size_t)ch * 24 + idx++];
                    A[a * 6 + b] -= v;
                    if (a != b) A[b * 6 + a] -= v;
                }
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
        if ((m >> a) & 1u) {
#pragma unroll
            for (int k = 0; k < 6; ++k) { A[a * 6 + k] = 0.0; A[k * 6 + a] = 0.0; }
            A[a * 7] = 1.0;
        }
    double L[36];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j * 7];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k];
        if (!(d > 0.0)) ok = false;
        d = sqrt(fmax(d, 1e-300));
        L[j * 7] = d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i * 6 + k] * L[j * 6 + k];
            L[i * 6 + j] = v / d;
        }
    }
    double Mo[36];
    if (ok) {
        double Li[36];          // L^-1, lower
#pragma unroll
        for (int k = 0; k < 36; ++k) Li[k] = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            Li[i * 7] = 1.0 / L[i * 7];
#pragma unroll
            for (int j = 0; j < i; ++j) {
                double v = 0.0;
#pragma unroll
                for (int k = j; k < i; ++k) v += L[i * 6 + k] * Li[k * 6 + j];
                Li[i * 6 + j] = -v / L[i * 7];
            }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b <= a; ++b) {
                double v = 0.0;
#pragma unroll
                for (int k = a; k < 6; ++k) v += Li[k * 6 + a] * Li[k * 6 + b];
                Mo[a * 6 + b] = v;
                Mo[b * 6 + a] = v;
            }
    } else {
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) Mo[a * 6 + b] = (a == b && A[a * 7] > 0.0) ? 1.0 / A[a * 7] : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) out[a * 6 + b] = (((m >> a) | (m >> b)) & 1u) ? 0.0 : Mo[a * 6 + b];
}

int launch_is_precond(int n_cams, int kind, const double* Hcc, const double* dc, const double* scale, const unsigned char* cam_fixed,
                      const int* cam_chunk_start, const double* sj_partial, double* Minv, hipStream_t st) {
    hipLaunchKernelGGL(is_precond_kernel, dim3((n_cams + 63) / 64), dim3(64), 0, st, n_cams, kind, Hcc, dc, scale, cam_fixed, cam_chunk_start,
                       sj_partial, Minv);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

// The PCG vector steps, one lane per camera dof (six lanes per camera: z = M^-1 r through LDS):
//   INIT     x = 0, r = b, z = M^-1 r;            partials r^T z, b^T b
//   DIR      p = z (first iteration) | z + beta p, beta = rho / rho_old
//   UPDATE   alpha = rho / p^T q (p^T q from the camera pass's partials); x += alpha p, r -= alpha q, z = M^-1 r;
//            partials r^T z, x^T (b + r)
//   PRECOND  z = M^-1 r (stba_ba_schur_apply)
__global__ __launch_bounds__(IS_VEC_THREADS) void is_vec_kernel(int n_cams, int op, PcgVecs v) {
    __shared__ double sh[4];
    __shared__ double rs[IS_VEC_THREADS];
    if ((op == IS_VEC_DIR || op == IS_VEC_UPDATE) && v.state->done) return;
    const int t = threadIdx.x;
    const int c0 = blockIdx.x * IS_CAMS_PER_WG;
    const size_t i = (size_t)c0 * 6 + t;
    const bool in = c0 + t / 6 < n_cams;
    if (op == IS_VEC_DIR) {
        if (!in) return;
        const int it = v.state->iter;
        v.p[i] = it == 0 ? v.z[i] : v.z[i] + (v.state->rho / v.state->rho_old) * v.p[i];
        return;
    }
    double ri = 0.0, xi = 0.0, bi = 0.0;
    if (op == IS_VEC_INIT) {
        if (in) { bi = v.b[i]; ri = bi; v.x[i] = 0.0; v.r[i] = ri; }
    } else if (op == IS_VEC_UPDATE) {
        const double pq = is_sum_partials(v.part_pq, gridDim.x, sh);
        const double alpha = v.state->rho / pq;
        const bool ok = pq > 0.0 && isfinite(pq) && isfinite(alpha);
        if (in) {
            xi = v.x[i]; ri = v.r[i]; bi = v.b[i];
            if (ok) {
                xi += alpha * v.p[i];
                ri -= alpha * v.q[i];
                v.x[i] = xi; v.r[i] = ri;
            }
        }
    } else if (in) ri = v.r[i];
    rs[t] = ri;
    __syncthreads();
    double zi = 0.0;
    if (in) {
        const int cl = t / 6, a = t % 6;
        const double* M = v.Minv + (size_t)(c0 + cl) * 36 + a * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) zi += M[k] * rs[cl * 6 + k];
        v.z[i] = zi;
    }
    if (op == IS_VEC_PRECOND) return;
    const double rz = is_block_sum(ri * zi, sh);
    const double qv = is_block_sum(op == IS_VEC_INIT ? bi * bi : xi * (bi + ri), sh);
    if (t == 0) { v.part_rz[blockIdx.x] = rz; v.part_q[blockIdx.x] = qv; }
}

int launch_is_vec(int n_cams, int op, const PcgVecs& v, hipStream_t st) {
    hipLaunchKernelGGL(is_vec_kernel, dim3(is_vec_grid(n_cams)), dim3(IS_VEC_THREADS), 0, st, n_cams, op, v);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

// the solve's scalars and its stop rule, one workgroup (the only writer of the state)
__global__ __launch_bounds__(IS_VEC_THREADS) void is_check_kernel(int n_wg, int op, PcgVecs v, double eta, int min_it, int max_it) {
    __shared__ double sh[4];
    PcgState* s = v.state;
    if (op == IS_CHECK_INIT) {
        const double bb = is_sum_partials(v.part_q, n_wg, sh), rho = is_sum_partials(v.part_rz, n_wg, sh);
        if (threadIdx.x != 0) return;
        s->iter = 0; s->fail = 0; s->hit_cap = 0; s->q0 = 0.0; s->pad = 0.0;
        s->rho = rho; s->rho_old = rho;
        int done = 0;
        if (bb == 0.0) done = 1;                                               // b = 0: x = 0 is the solution
        else if (rho == 0.0 || !isfinite(rho)) { done = 1; s->fail = 1; }
        s->done = done;
        return;
    }
    if (s->done) return;
    const double pq = is_sum_partials(v.part_pq, n_wg, sh);
    const double xbr = is_sum_partials(v.part_q, n_wg, sh);
    const double rz = is_sum_partials(v.part_rz, n_wg, sh);
    if (threadIdx.x != 0) return;
    const int it = s->iter + 1;
    s->iter = it;
    const double rho = s->rho, alpha = rho / pq;
    if (!(pq > 0.0) || !isfinite(pq)) { s->done = 1; return; }              // NO_CONVERGENCE: the iterate so far
    if (!isfinite(alpha)) { s->done = 1; s->fail = 1; return; }
    const double q1 = -0.5 * xbr;
    const double zeta = (double)it * (q1 - s->q0) / q1;
    if (zeta < eta && it >= min_it) { s->done = 1; return; }
    if (it >= max_it) { s->done = 1; s->hit_cap = 1; return; }
    if (rz == 0.0 || !isfinite(rz)) { s->done = 1; s->fail = 1; return; }
    s->q0 = q1;
    s->rho_old = rho;
    s->rho = rz;
}

int launch_is_check(int n_cams, int op, const PcgVecs& v, double eta, int min_iterations, int max_iterations, hipStream_t st) {
    hipLaunchKernelGGL(is_check_kernel, dim3(1), dim3(IS_VEC_THREADS), 0, st, is_vec_grid(n_cams), op, v, eta, min_iterations, max_iterations);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

__global__ void is_export_kernel(const PcgState* __restrict__ s, double* __restrict__ out, double seq) {
    __shared__ double hp[4];
    if (threadIdx.x == 0) { hp[0] = (double)s->done; hp[1] = (double)s->iter; hp[2] = (double)s->fail; hp[3] = (double)s->hit_cap; }
    __syncthreads();
    stamped_store_wave(out, hp, 4, seq, threadIdx.x);
}

int launch_is_export(const PcgState* state, double* host_out, double seq, hipStream_t st) {
    hipLaunchKernelGGL(is_export_kernel, dim3(1), dim3(64), 0, st, state, host_out, seq);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

}  // namespace stba
