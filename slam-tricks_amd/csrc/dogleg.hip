// dogleg.hip -- the two kernels of the DOGLEG trust-region strategy of the BA engine (Ceres' DoglegStrategy, TRADITIONAL_DOGLEG;
// DESIGN.md 7c), FP64, wave64.
//
// Once per linearisation, behind the Gauss-Newton step of the engine's own damped reduced system (radius 1/mu), the terms kernel
// makes one landmark-major pass over the observations with the compact Jacobian records and leaves six scalars on the device
// (dogleg_select.hpp).  Every trial step -- the first one of a linearisation and every one behind a rejection -- is then the step
// kernel (the case, beta and the trial point) and the engine's trial evaluation: no Schur build, no factorisation, no
// back-substitution.
//
// Everything is kept in the engine's coordinates, the UNSCALED step delta = s .* y: the kernels hold s .* u (u = gamma ./ d) next to
// the Gauss-Newton step delta_gn = dxc | dxp, and the step is delta = a (s .* u) + b delta_gn.  J^ u = J (s .* u), J^ y_gn = J delta_gn.
//
// Reproducibility: per-workgroup partials in fixed slots, added by one workgroup in index order (no floating-point atomics).
#include "ba_kernels.hpp"
#include "dogleg.hpp"

namespace stba {

// the back-substitution's shapes, so that the step kernel's partials are what launch_trial_finish adds behind ba_backsub_trial:
// DL_LM landmarks per landmark workgroup (backsub_grid), DL_THREADS cameras per camera workgroup (backsub_cam_grid)
constexpr int DL_THREADS = 128, DL_LM = 32, DL_PART = 8;
static_assert(3 * DL_LM <= DL_THREADS, "one lane per landmark dof");

__host__ __device__ inline int dl_lm_blocks(int n_pts) { return (n_pts + DL_LM - 1) / DL_LM; }
__host__ __device__ inline int dl_cam_blocks(int n_cams) { return (n_cams + DL_THREADS - 1) / DL_THREADS; }
size_t dogleg_partial_doubles(int n_cams, int n_pts) { return (size_t)(dl_lm_blocks(n_pts) + dl_cam_blocks(n_cams)) * DL_PART; }

// one free dof: d^2 = clamp(h s^2, dmin, dmax) (the LM path's clamped column norm of the scaled Jacobian), gamma = s g / d,
// z_gn = d dx / s, and s .* u = s gamma / d
__device__ __forceinline__ void dl_entry(double g, double h, double s, double dmin, double dmax, double dx, double& gam, double& zgn,
                                         double& su) {
    const double s2 = s * s;
    const double d = sqrt(fmin(fmax(h * s2, dmin), dmax));
    gam = s * g / d;
    zgn = d * dx / s;
    su = s * gam / d;
}

// the sum of v[0..5] over the workgroup (two waves, added in wave order) -> out[0..7] (entries 6, 7 zero)
__device__ __forceinline__ void dl_block_sum6(const double v[6], double* __restrict__ out) {
    __shared__ double sh[DL_THREADS / 64][6];
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double x = v[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((t & 63) == 0) sh[t >> 6][k] = x;
    }
    __syncthreads();
    if (t < DL_PART) out[t] = t < 6 ? sh[0][t] + sh[1][t] : 0.0;
}

// landmark workgroups: u of their landmarks, the landmark terms of |gamma|^2, gamma^T z_gn, |z_gn|^2, and over their observations
// |J^ u|^2, |J^ y_gn|^2, (J^ u)^T (J^ y_gn); camera workgroups behind them: u of their cameras and the camera terms of the first three
template <bool GEN>
__global__ __launch_bounds__(DL_THREADS) void ba_dogleg_terms_kernel(DoglegArgs a) {
    __shared__ int seg[DL_LM + 1];
    __shared__ double su_p[3 * DL_LM], dx_p[3 * DL_LM];
    const int t = threadIdx.x;
    const int lm_blocks = dl_lm_blocks(a.n_pts);
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if ((int)blockIdx.x >= lm_blocks) {
        const int c = ((int)blockIdx.x - lm_blocks) * DL_THREADS + t;
        if (c < a.n_cams) {
            const unsigned cm = a.cam_fixed ? a.cam_fixed[c] : 0u;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const size_t i = (size_t)c * 6 + k;
                double gam = 0.0, zgn = 0.0, su = 0.0;
                if (!((cm >> k) & 1u)) dl_entry(a.gc[i], a.hc[i], a.scale_c[i], a.dmin, a.dmax, a.dxc[i], gam, zgn, su);
                a.uc[i] = su;
                v[0] += gam * gam; v[1] += gam * zgn; v[2] += zgn * zgn;
            }
        }
        dl_block_sum6(v, a.partial + (size_t)blockIdx.x * DL_PART);
        return;
    }
    const int j0 = blockIdx.x * DL_LM, nl = min(DL_LM, a.n_pts - j0);
    if (t <= nl) seg[t] = a.pt_start[j0 + t];
    if (t < 3 * DL_LM) {
        const int lj = t / 3, k = t - 3 * lj;
        double su = 0.0, dx = 0.0;
        if (lj < nl) {
            const size_t i = (size_t)j0 * 3 + t;
            if (!(a.pt_fixed && a.pt_fixed[j0 + lj])) {
                double gam, zgn;
                dx = a.dxp[i];
                dl_entry(a.gp[i], a.Hpp6[(size_t)(j0 + lj) * 6 + (k == 0 ? 0 : (k == 1 ? 3 : 5))], a.scale_p[i], a.dmin, a.dmax, dx, gam, zgn, su);
                v[0] += gam * gam; v[1] += gam * zgn; v[2] += zgn * zgn;
            }
            a.up[i] = su;
        }
        su_p[t] = su; dx_p[t] = dx;
    }
    __syncthreads();
    const int rb = seg[0], re = seg[nl];
    for (int l = rb + t; l < re; l += DL_THREADS) {
        const int c = a.obs_cam[l], jl = a.obs_pt[l] - j0;
        double jc[12], jp[6];
        load_jc_jp<GEN>(a.J8, a.omask, l, jc, jp, a.Jc12);
        const unsigned cm = a.cam_fixed ? a.cam_fixed[c] : 0u;
        double e0 = 0.0, e1 = 0.0, n0 = 0.0, n1 = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            // (s .* u of the camera as its camera workgroup stores it: the same function of the same inputs)
            const size_t i = (size_t)c * 6 + k;
            double gam, zgn, su = 0.0;
            const double x = a.dxc[i];
            if (!((cm >> k) & 1u)) dl_entry(a.gc[i], a.hc[i], a.scale_c[i], a.dmin, a.dmax, x, gam, zgn, su);
            e0 += jc[k] * su; e1 += jc[6 + k] * su;
            n0 += jc[k] * x; n1 += jc[6 + k] * x;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double su = su_p[3 * jl + k], x = dx_p[3 * jl + k];
            e0 += jp[k] * su; e1 += jp[3 + k] * su;
            n0 += jp[k] * x; n1 += jp[3 + k] * x;
        }
        v[3] += e0 * e0 + e1 * e1;
        v[4] += n0 * n0 + n1 * n1;
        v[5] += e0 * n0 + e1 * n1;
    }
    // (landmark priors: their rows W su_j, W dx_j of the same three sums, one landmark per lane)
    if (a.lp.start && t < nl) lp_dogleg_rows(a.lp, j0 + t, su_p + 3 * t, dx_p + 3 * t, &v[3], &v[4], &v[5]);
    dl_block_sum6(v, a.partial + (size_t)blockIdx.x * DL_PART);
}

// the six scalars: the partials of every workgroup, strided shares then a halving tree (one workgroup, always the same order)
__global__ __launch_bounds__(256) void ba_dogleg_sum_kernel(const double* __restrict__ partial, int n, double* __restrict__ scalars) {
    __shared__ double s[6][256];
    const int t = threadIdx.x;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = t; i < n; i += 256) {
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] += partial[(size_t)i * DL_PART + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k][t] = v[k];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < 6; ++k) s[k][t] += s[k][t + off];
        }
        __syncthreads();
    }
    if (t < 6) scalars[t] = s[t][0];
}

int launch_dogleg_terms(const DoglegArgs& a, hipStream_t st) {
    const int grid = dl_lm_blocks(a.n_pts) + dl_cam_blocks(a.n_cams);
    if (a.Jc12) hipLaunchKernelGGL(ba_dogleg_terms_kernel<true>, dim3(grid), dim3(DL_THREADS), 0, st, a);
    else hipLaunchKernelGGL(ba_dogleg_terms_kernel<false>, dim3(grid), dim3(DL_THREADS), 0, st, a);
    hipLaunchKernelGGL(ba_dogleg_sum_kernel, dim3(1), dim3(256), 0, st, a.partial, grid, a.scalars);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

// the step at radius Delta: a one-lane prologue picks the case (dogleg_select), then every workgroup writes its share of the trial
// point with the manifold update of ba_backsub_trial and one partial {|step|^2, |x|^2, model} -- the model change m itself in the
// first camera workgroup's slot, zero elsewhere.  Workgroup 0 hands what it chose to the host as a stamped block.
__global__ __launch_bounds__(DL_THREADS) void ba_dogleg_step_kernel(DoglegStepArgs a, double radius) {
    __shared__ double hp[DL_BLOCK], ab[2];
    __shared__ double ssum[DL_THREADS / 64][3];
    const int t = threadIdx.x;
    if (t == 0) {
        const DoglegScalars s{a.scalars[0], a.scalars[1], a.scalars[2], a.scalars[3], a.scalars[4], a.scalars[5]};
        const DoglegStep o = dogleg_select(s, radius);
        // (scalars that are not finite: a = b = 0, but 0 * NaN is NaN -- the trial point is garbage, and the host discards it unseen)
        hp[DL_KASE] = (double)o.kase; hp[DL_BETA] = o.beta; hp[DL_ZNORM] = o.z_norm; hp[DL_MODEL] = o.model;
        hp[DL_GG] = s.gg; hp[DL_GZ] = s.gz; hp[DL_ZZ] = s.zz; hp[DL_UU] = s.uu; hp[DL_NN] = s.nn; hp[DL_UN] = s.un;
        ab[0] = o.a; ab[1] = o.b;
    }
    __syncthreads();
    const double ca = ab[0], cb = ab[1], model = hp[DL_MODEL];
    if (blockIdx.x == 0 && t < 64 && a.host_out) stamped_store_wave(a.host_out, hp, DL_BLOCK, a.seq, t);
    const int lm_blocks = dl_lm_blocks(a.n_pts);
    double v[3] = {0.0, 0.0, 0.0};
    double* out;
    if ((int)blockIdx.x >= lm_blocks) {
        const int cblk = (int)blockIdx.x - lm_blocks, c = cblk * DL_THREADS + t;
        if (c < a.n_cams) {
            const unsigned cm = a.cam_fixed ? a.cam_fixed[c] : 0u;
            double d[6], q[4], qn[4];
#pragma unroll
            for (int k = 0; k < 6; ++k) d[k] = ((cm >> k) & 1u) ? 0.0 : ca * a.uc[c * 6 + k] + cb * a.dxc[c * 6 + k];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = a.cams[(size_t)c * 7 + k];
            so3_plus(q, d, qn);
            const bool rot_active = (cm & 7u) != 7u, pos_active = (cm & 56u) != 56u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double o = rot_active ? qn[k] : q[k];
                a.cams_new[(size_t)c * 7 + k] = o;
                if (rot_active) { v[0] += (o - q[k]) * (o - q[k]); v[1] += q[k] * q[k]; }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double p = a.cams[(size_t)c * 7 + 4 + k];
                a.cams_new[(size_t)c * 7 + 4 + k] = p + d[3 + k];
                if (pos_active) { v[0] += d[3 + k] * d[3 + k]; v[1] += p * p; }
            }
        }
        if (cblk == 0 && t == 0) v[2] = model;
        out = a.partial_c + (size_t)cblk * 4;
    } else {
        const int j0 = blockIdx.x * DL_LM, nl = min(DL_LM, a.n_pts - j0);
        const int lj = t / 3;
        if (t < 3 * DL_LM && lj < nl) {
            const size_t i = (size_t)j0 * 3 + t;
            const bool fx = a.pt_fixed ? (a.pt_fixed[j0 + lj] != 0) : false;
            const double p = a.pts[i];
            const double dd = fx ? 0.0 : ca * a.up[i] + cb * a.dxp[i];
            a.pts_new[i] = p + dd;
            if (!fx) { v[0] = dd * dd; v[1] = p * p; }
        }
        out = a.partial_p + (size_t)blockIdx.x * 4;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double x = v[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((t & 63) == 0) ssum[t >> 6][k] = x;
    }
    __syncthreads();
    if (t < 4) {
        double sv = 0.0;
        if (t < 3) for (int w = 0; w < DL_THREADS / 64; ++w) sv += ssum[w][t];
        out[t] = sv;
    }
}

int launch_dogleg_step(const DoglegStepArgs& a, double radius, hipStream_t st) {
    if (dl_lm_blocks(a.n_pts) != backsub_grid(a.n_pts) || dl_cam_blocks(a.n_cams) != backsub_cam_grid(a.n_cams))
        return fail(STBA_ERR_STATE, "dogleg step: the partials' shape is not the back-substitution's");
    const int grid = dl_lm_blocks(a.n_pts) + dl_cam_blocks(a.n_cams);
    hipLaunchKernelGGL(ba_dogleg_step_kernel, dim3(grid), dim3(DL_THREADS), 0, st, a, radius);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

}  // namespace stba
