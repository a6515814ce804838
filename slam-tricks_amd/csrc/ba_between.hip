// ba_between.hip -- the two kernels of the camera-to-camera relative-pose factors.  Latency-bound work (a few
// thousand 6 x 6 products): one launch each, no atomic, every sum in a fixed order.
#include "ba_between.hpp"

namespace stba {

__device__ __forceinline__ double sel3(int c, double a0, double a1, double a2) { return c == 0 ? a0 : (c == 1 ? a1 : a2); }

// ---- cost form: one workgroup; thread t takes the edges t, t + 256, ... in the caller's order
__global__ __launch_bounds__(BETWEEN_THREADS) void ba_between_cost_kernel(BetweenArgs a, const double* __restrict__ cams, double* __restrict__ slot) {
    __shared__ double s[BETWEEN_THREADS];
    double v = 0.0;
    for (int k = threadIdx.x; k < a.n; k += BETWEEN_THREADS) {
        double ci[7], cj[7], me[7], rw[6];
        const double* pi = cams + (size_t)a.cam_i[k] * 7;
        const double* pj = cams + (size_t)a.cam_j[k] * 7;
#pragma unroll
        for (int q = 0; q < 7; ++q) { ci[q] = pi[q]; cj[q] = pj[q]; me[q] = a.meas[(size_t)k * 7 + q]; }
        between_eval(me, a.W + (size_t)k * 36, ci, cj, 0u, 0u, rw, nullptr, nullptr);
        double sg = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) sg += rw[i] * rw[i];
        v += sg;
    }
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = BETWEEN_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) slot[0] = s[0];
}

// ---- block form: one wave per group; the groups [g0, g1) of the list [camera groups | pair groups].  For every edge of its group
// lane l < 36 holds entry (l / 6, l % 6) of TWO whitened Jacobians, p and q, and lane 36 + i holds r'(i):
//   camera group of camera x: p = q = J_x';  the lanes own Hcc(l / 6, l % 6) and gc(l - 36) of x;
//   pair group (hi, lo):      p = J_hi', q = J_lo';  the lanes own entry (l / 6, l % 6) of the block (hi, lo) of S.
// The owner of entry (a, b) adds sum_i p(i, a) q(i, b) -- gc(a): sum_i p(i, a) r'(i) -- from its neighbours' registers (cross-lane
// reads, no LDS), edge after edge in the caller's order.  Hcc's entries (a, b) and (b, a) add the same products in the same order.
__global__ __launch_bounds__(BETWEEN_THREADS) void ba_between_blocks_kernel(BetweenArgs a, int g0, int g1, const double* __restrict__ cams,
                                                                            double* __restrict__ Hcc, double* __restrict__ gc,
                                                                            double* __restrict__ S, int lda, double* __restrict__ out_r,
                                                                            double* __restrict__ out_Ji, double* __restrict__ out_Jj) {
    const int lane = threadIdx.x & 63;
    const int g = g0 + blockIdx.x * BETWEEN_GROUPS_PER_WG + (threadIdx.x >> 6);
    if (g >= g1) return;                               // (a whole wave: the cross-lane reads below see every lane of theirs)
    const bool pair = g >= a.n_cam_groups;
    const int pgi = g - a.n_cam_groups;
    const int k0 = pair ? a.pg_ptr[pgi] : a.cg_ptr[g], k1 = pair ? a.pg_ptr[pgi + 1] : a.cg_ptr[g + 1];
    const int* refs = pair ? a.pg_ref : a.cg_ref;
    const int row = lane < 36 ? lane / 6 : (lane < 42 ? lane - 36 : 0), col = lane < 36 ? lane % 6 : 0;
    double acc = 0.0;
    for (int k = k0; k < k1; ++k) {
        const int ref = refs[k], e = ref >> 1, side = ref & 1;
        const int ei = a.cam_i[e], ej = a.cam_j[e];
        double ci[7], cj[7], me[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) { ci[q] = cams[(size_t)ei * 7 + q]; cj[q] = cams[(size_t)ej * 7 + q]; me[q] = a.meas[(size_t)e * 7 + q]; }
        double r[6], Jri[9], Rm[9], Ri[9], v[3];
        between_parts(me, ci, cj, r, Jri, Rm, Ri, v);
        const double* Wi = a.W + (size_t)e * 36 + row * 6;
        const unsigned mi = a.cam_fixed ? a.cam_fixed[ei] : 0u, mj = a.cam_fixed ? a.cam_fixed[ej] : 0u;
        double vi = 0.0, vj = 0.0;
        if (lane < 36) {
            // column `col` of J_i and of J_j, picked with selects (an array indexed by the lane would live in scratch memory); the
            // values and the whitening dot are those of between_residual / between_eval: the same bits
            const int cb = col < 3 ? col : col - 3;
            double xi[6], xj[6];
            if (col < 3) {
                const double m0 = sel3(cb, Rm[0], Rm[3], Rm[6]), m1 = sel3(cb, Rm[1], Rm[4], Rm[7]), m2 = sel3(cb, Rm[2], Rm[5], Rm[8]);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    xi[q] = between_rot_entry(Jri[q * 3], Jri[q * 3 + 1], Jri[q * 3 + 2], m0, m1, m2);
                    xj[q] = sel3(cb, Jri[q * 3], Jri[q * 3 + 1], Jri[q * 3 + 2]);
                    xj[3 + q] = 0.0;
                }
                xi[3] = sel3(cb, 0.0, -v[2], v[1]); xi[4] = sel3(cb, v[2], 0.0, -v[0]); xi[5] = sel3(cb, -v[1], v[0], 0.0);
            } else {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double rq = sel3(cb, Ri[q], Ri[3 + q], Ri[6 + q]);
                    xi[q] = xj[q] = 0.0;
                    xi[3 + q] = -rq; xj[3 + q] = rq;
                }
            }
            vi = ((mi >> col) & 1u) ? 0.0 : between_dot(Wi, xi, 1);
            vj = ((mj >> col) & 1u) ? 0.0 : between_dot(Wi, xj, 1);
            if (out_Ji) { out_Ji[(size_t)e * 36 + lane] = vi; out_Jj[(size_t)e * 36 + lane] = vj; }
        } else if (lane < 42) {
            vi = vj = between_dot(Wi, r, 1);
            if (out_r) out_r[(size_t)e * 6 + row] = vi;
        }
        // p: the group's camera (camera group) or hi (pair group), which `side` says is the edge's j; q: the same, or lo
        const double p = side ? vj : vi;
        const double q = pair ? (side ? vi : vj) : p;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double x = __shfl(p, i * 6 + row, 64);
            const double y = __shfl(lane < 36 ? q : p, lane < 36 ? i * 6 + col : 36 + i, 64);
            acc += x * y;
        }
    }
    if (pair) {
        if (S && lane < 36) {
            const int2 hl = a.pg_pair[pgi];
            S[(size_t)(6 * hl.x + row) * lda + 6 * hl.y + col] += acc;
        }
    } else if (Hcc) {
        const int c = a.cg_cam[g];
        if (lane < 36) Hcc[(size_t)c * 36 + lane] += acc;
        else if (lane < 42) gc[(size_t)c * 6 + (lane - 36)] += acc;
    }
}

int launch_between_cost(const BetweenArgs& a, const double* cams, double* slot, hipStream_t st) {
    hipLaunchKernelGGL(ba_between_cost_kernel, dim3(1), dim3(BETWEEN_THREADS), 0, st, a, cams, slot);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

int launch_between_blocks(const BetweenArgs& a, const double* cams, double* Hcc, double* gc, double* S, int lda, double* out_r, double* out_Ji,
                          double* out_Jj, hipStream_t st) {
    if (a.n <= 0) return STBA_OK;
    if ((Hcc == nullptr) != (gc == nullptr)) return fail(STBA_ERR_INVALID_ARGUMENT, "launch_between_blocks: Hcc and gc go together");
    if ((out_Ji == nullptr) != (out_Jj == nullptr)) return fail(STBA_ERR_INVALID_ARGUMENT, "launch_between_blocks: out_Ji and out_Jj go together");
    const int g0 = Hcc ? 0 : a.n_cam_groups;
    const int g1 = (S || out_r || out_Ji) ? a.n_cam_groups + a.n_pair_groups : a.n_cam_groups;
    if (g1 <= g0) return STBA_OK;
    const int grid = (g1 - g0 + BETWEEN_GROUPS_PER_WG - 1) / BETWEEN_GROUPS_PER_WG;
    hipLaunchKernelGGL(ba_between_blocks_kernel, dim3(grid), dim3(BETWEEN_THREADS), 0, st, a, g0, g1, cams, Hcc, gc, S, lda, out_r, out_Ji, out_Jj);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

}  // namespace stba
