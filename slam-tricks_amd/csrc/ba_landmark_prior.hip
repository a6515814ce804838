// ba_landmark_prior.hip -- the two kernels of the landmark position priors.  A prior is 12 doubles in and nine
// products out: the kernels are bound by their loads; no atomic, every sum in a fixed order.
#include "ba_kernels.hpp"
#include "ba_landmark_prior.hpp"

namespace stba {

// ---- cost form: workgroup b takes the priors [b, b + 1) * LP_COST_PER_WG of the grouped order, thread t of it the priors t, t + 256,
// ... of that stretch, one tree; one workgroup (n <= LP_COST_PER_WG) writes the slot itself, more write one partial each, which
// ba_landmark_prior_cost_sum_kernel adds in index order.  (One workgroup for everything, the pose priors' shape, does not carry over: at 100 000
// priors its lanes walk a hundred priors each, dependent loads on ONE compute unit -- measured)
__global__ __launch_bounds__(LP_COST_THREADS) void ba_landmark_prior_cost_kernel(LandmarkPriorArgs a, const double* __restrict__ pts,
                                                                                  double* __restrict__ out) {
    __shared__ double s[LP_COST_THREADS];
    double v = 0.0;
    const int k0 = blockIdx.x * LP_COST_PER_WG, k1 = min(k0 + LP_COST_PER_WG, a.n);
#pragma unroll 4
    for (int k = k0 + threadIdx.x; k < k1; k += LP_COST_THREADS) {
        const double* pj = pts + (size_t)a.pt[k] * 3;
        const double p[3] = {pj[0], pj[1], pj[2]};
        double rw[3];
        lp_residual(a.W + (size_t)k * 9, a.pos + (size_t)k * 3, p, rw);
        v += (rw[0] * rw[0] + rw[1] * rw[1]) + rw[2] * rw[2];
    }
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = LP_COST_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(LP_COST_THREADS) void ba_landmark_prior_cost_sum_kernel(const double* __restrict__ part, int n,
                                                                                      double* __restrict__ slot) {
    __shared__ double s[LP_COST_THREADS];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += LP_COST_THREADS) v += part[i];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = LP_COST_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) slot[0] = s[0];
}

// ---- block form: one lane per LANDMARK (with priors or without), LP_LM_PER_WG consecutive landmarks per workgroup.  A lane whose
// landmark has priors adds them, in the caller's order, to the six entries of Hpp6 and the three of gp it alone owns.  Every lane
// then holds max |gp_j| of the SUM, and every POINT_BLOCK_LANDMARKS lanes write the partial of their landmark-block workgroup again:
// the partials that kernel left are stale for a landmark with priors, and a maximum cannot be mended, only made again.  (A maximum
// does not depend on the order: for a stretch without priors the bits are the ones that were there.)
static_assert(64 % POINT_BLOCK_LANDMARKS == 0 && LP_LM_PER_WG % 64 == 0, "a partial's landmarks are lanes of one wave");
__global__ __launch_bounds__(LP_THREADS) void ba_landmark_prior_blocks_kernel(LandmarkPriorArgs a, const double* __restrict__ pts,
                                                                              double* __restrict__ Hpp6, double* __restrict__ gp,
                                                                              double* __restrict__ gpmax_partial,
                                                                              double* __restrict__ out_r, double* __restrict__ out_J) {
    const int j = blockIdx.x * LP_LM_PER_WG + threadIdx.x;
    double m = 0.0;
    if (j < a.n_pts) {
        const int kb = a.start[j], ke = a.start[j + 1];
        const bool fx = a.pt_fixed && a.pt_fixed[j] != 0;
        double g[3] = {0.0, 0.0, 0.0};
        if (gp) { g[0] = gp[(size_t)j * 3]; g[1] = gp[(size_t)j * 3 + 1]; g[2] = gp[(size_t)j * 3 + 2]; }
        if (kb < ke) {
            const double p[3] = {pts[(size_t)j * 3], pts[(size_t)j * 3 + 1], pts[(size_t)j * 3 + 2]};
            double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            const bool add = Hpp6 && !fx;
            if (add) {
#pragma unroll
                for (int e = 0; e < 6; ++e) h[e] = Hpp6[(size_t)j * 6 + e];
            }
            for (int k = kb; k < ke; ++k) {
                double W[9], rw[3];
#pragma unroll
                for (int e = 0; e < 9; ++e) W[e] = a.W[(size_t)k * 9 + e];
                lp_residual(W, a.pos + (size_t)k * 3, p, rw);
                if (out_r) { out_r[(size_t)k * 3] = rw[0]; out_r[(size_t)k * 3 + 1] = rw[1]; out_r[(size_t)k * 3 + 2] = rw[2]; }
                if (out_J) {
#pragma unroll
                    for (int e = 0; e < 9; ++e) out_J[(size_t)k * 9 + e] = fx ? 0.0 : W[e];
                }
                if (add) {
                    h[0] += lp_wtw(W, 0, 0); h[1] += lp_wtw(W, 0, 1); h[2] += lp_wtw(W, 0, 2);
                    h[3] += lp_wtw(W, 1, 1); h[4] += lp_wtw(W, 1, 2); h[5] += lp_wtw(W, 2, 2);
                    g[0] += lp_wtr(W, rw, 0); g[1] += lp_wtr(W, rw, 1); g[2] += lp_wtr(W, rw, 2);
                }
            }
            if (add) {
#pragma unroll
                for (int e = 0; e < 6; ++e) Hpp6[(size_t)j * 6 + e] = h[e];
                gp[(size_t)j * 3] = g[0]; gp[(size_t)j * 3 + 1] = g[1]; gp[(size_t)j * 3 + 2] = g[2];
            }
        }
        m = fmax(fmax(fabs(g[0]), fabs(g[1])), fabs(g[2]));
    }
    if (gpmax_partial) {
        // (every lane of the wave takes part: lanes behind the last landmark hold 0, which is where the maximum starts)
        for (int off = POINT_BLOCK_LANDMARKS / 2; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, POINT_BLOCK_LANDMARKS));
        if (j < a.n_pts && (threadIdx.x % POINT_BLOCK_LANDMARKS) == 0) gpmax_partial[j / POINT_BLOCK_LANDMARKS] = m;
    }
}

int landmark_prior_cost_grid(int n) { return n > 0 ? (n + LP_COST_PER_WG - 1) / LP_COST_PER_WG : 1; }

int launch_landmark_prior_cost(const LandmarkPriorArgs& a, const double* pts, double* part, double* slot, hipStream_t st) {
    const int grid = landmark_prior_cost_grid(a.n);
    if (grid > 1 && !part) return fail(STBA_ERR_INVALID_ARGUMENT, "launch_landmark_prior_cost: more than one workgroup needs the partials' array");
    hipLaunchKernelGGL(ba_landmark_prior_cost_kernel, dim3(grid), dim3(LP_COST_THREADS), 0, st, a, pts, grid > 1 ? part : slot);
    if (grid > 1) hipLaunchKernelGGL(ba_landmark_prior_cost_sum_kernel, dim3(1), dim3(LP_COST_THREADS), 0, st, part, grid, slot);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

int launch_landmark_prior_blocks(const LandmarkPriorArgs& a, const double* pts, double* Hpp6, double* gp, double* gpmax_partial,
                                 double* out_r, double* out_J, hipStream_t st) {
    if (a.n <= 0 || a.n_pts <= 0) return STBA_OK;
    if ((Hpp6 == nullptr) != (gp == nullptr) || (Hpp6 == nullptr) != (gpmax_partial == nullptr))
        return fail(STBA_ERR_INVALID_ARGUMENT, "launch_landmark_prior_blocks: Hpp6, gp and the max partials go together");
    const int grid = (a.n_pts + LP_LM_PER_WG - 1) / LP_LM_PER_WG;
    hipLaunchKernelGGL(ba_landmark_prior_blocks_kernel, dim3(grid), dim3(LP_THREADS), 0, st, a, pts, Hpp6, gp, gpmax_partial, out_r, out_J);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

}  // namespace stba
