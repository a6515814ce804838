// ba_prior.hip -- the two kernels of the camera pose priors.  Latency-bound work (at most a few thousand 6 x 6
// products): one launch each, no atomic, every sum in a fixed order.
#include "ba_prior.hpp"

namespace stba {

// whitened residual i of a prior from its 6 residuals.  Like the factor's maths in ba_prior.hpp, the whitening is kept free of FMA
// contraction and in ONE documented order: W r cancels (a tight prior far from the iterate: |W r| << sum |W| |r|), so what a
// different order moves is not small against the result, and the numpy restatement the tests hold the blocks against states
// this order
__device__ __forceinline__ double prior_row_dot(const double* __restrict__ Wi, const double* r) {
#pragma clang fp contract(off)
    return ((((Wi[0] * r[0] + Wi[1] * r[1]) + Wi[2] * r[2]) + Wi[3] * r[3]) + Wi[4] * r[4]) + Wi[5] * r[5];
}

__device__ __forceinline__ double prior_col_dot(const double* __restrict__ Wi, double j0, double j1, double j2) {
#pragma clang fp contract(off)
    return (Wi[0] * j0 + Wi[1] * j1) + Wi[2] * j2;
}

// ---- cost form: one workgroup; thread t takes the groups t, t + 256, ...; inside a group the priors in the caller's order
__global__ __launch_bounds__(PRIOR_THREADS) void ba_prior_cost_kernel(PriorArgs a, const double* __restrict__ cams, double* __restrict__ slot) {
    __shared__ double s[PRIOR_THREADS];
    double v = 0.0;
    for (int g = threadIdx.x; g < a.n_groups; g += PRIOR_THREADS) {
        const double* cam = cams + (size_t)a.group_cam[g] * 7;
        double cq[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) cq[k] = cam[k];
        double sg = 0.0;
        for (int k = a.group_ptr[g]; k < a.group_ptr[g + 1]; ++k) {
            double r[6];
            prior_residual(a.pose + (size_t)k * 7, cq, r, nullptr);
            const double* W = a.W + (size_t)k * 36;
#pragma unroll
            for (int i = 0; i < 6; ++i) { const double w = prior_row_dot(W + i * 6, r); sg += w * w; }
        }
        v += sg;
    }
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = PRIOR_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) slot[0] = s[0];
}

// ---- block form: one wave per camera that has priors.  Lane l < 36 holds J'(l / 6, l % 6) of the current prior, lane 36 + i holds
// r'(i); the same lanes own Hcc entry (l / 6, l % 6) and gc entry l - 36 of the camera and add the prior's six products to them from
// their neighbours' registers (cross-lane reads, no LDS).  Entry (a, b) and entry (b, a) add the same products in the same order.
__global__ __launch_bounds__(PRIOR_THREADS) void ba_prior_blocks_kernel(PriorArgs a, const double* __restrict__ cams, double* __restrict__ Hcc,
                                                                        double* __restrict__ gc, double* __restrict__ out_r,
                                                                        double* __restrict__ out_J) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * PRIOR_CAMS_PER_WG + (threadIdx.x >> 6);
    if (g >= a.n_groups) return;                       // (a whole wave: the cross-lane reads below see every lane of theirs)
    const int c = a.group_cam[g];
    const unsigned mask = a.cam_fixed ? a.cam_fixed[c] : 0u;
    double cq[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) cq[k] = cams[(size_t)c * 7 + k];
    const int row = lane < 36 ? lane / 6 : (lane < 42 ? lane - 36 : 0), col = lane < 36 ? lane % 6 : 0;
    // which two lanes' values this lane multiplies for term i: Hcc (a, b): J'(i, a) J'(i, b); gc (a): J'(i, a) r'(i)
    const int ea = lane < 36 ? lane / 6 : (lane < 42 ? lane - 36 : 0);
    const int eb = lane < 36 ? lane % 6 : 0;
    double acc = 0.0;
    for (int k = a.group_ptr[g]; k < a.group_ptr[g + 1]; ++k) {
        double r[6], Jri[9];
        prior_residual(a.pose + (size_t)k * 7, cq, r, Jri);
        const double* Wi = a.W + (size_t)k * 36 + row * 6;
        double v = 0.0;
        if (lane < 36) {
            if (col < 3) {
                const double j0 = col == 0 ? Jri[0] : (col == 1 ? Jri[1] : Jri[2]);
                const double j1 = col == 0 ? Jri[3] : (col == 1 ? Jri[4] : Jri[5]);
                const double j2 = col == 0 ? Jri[6] : (col == 1 ? Jri[7] : Jri[8]);
                v = prior_col_dot(Wi, j0, j1, j2);
            } else v = Wi[col];
            if ((mask >> col) & 1u) v = 0.0;
            if (out_J) out_J[(size_t)k * 36 + lane] = v;
        } else if (lane < 42) {
            v = prior_row_dot(Wi, r);
            if (out_r) out_r[(size_t)k * 6 + row] = v;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double x = __shfl(v, i * 6 + ea, 64);
            const double y = __shfl(v, lane < 36 ? i * 6 + eb : 36 + i, 64);
            acc += x * y;
        }
    }
    if (Hcc) {
        if (lane < 36) Hcc[(size_t)c * 36 + lane] += acc;
        else if (lane < 42) gc[(size_t)c * 6 + (lane - 36)] += acc;
    }
}

int launch_prior_cost(const PriorArgs& a, const double* cams, double* slot, hipStream_t st) {
    hipLaunchKernelGGL(ba_prior_cost_kernel, dim3(1), dim3(PRIOR_THREADS), 0, st, a, cams, slot);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

int launch_prior_blocks(const PriorArgs& a, const double* cams, double* Hcc, double* gc, double* out_r, double* out_J, hipStream_t st) {
    if (a.n_groups <= 0) return STBA_OK;
    if ((Hcc == nullptr) != (gc == nullptr)) return fail(STBA_ERR_INVALID_ARGUMENT, "launch_prior_blocks: Hcc and gc go together");
    const int grid = (a.n_groups + PRIOR_CAMS_PER_WG - 1) / PRIOR_CAMS_PER_WG;
    hipLaunchKernelGGL(ba_prior_blocks_kernel, dim3(grid), dim3(PRIOR_THREADS), 0, st, a, cams, Hcc, gc, out_r, out_J);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

}  // namespace stba
