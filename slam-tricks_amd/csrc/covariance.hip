// covariance.hip -- covariance of a least-squares problem at its current parameters (ceres::Covariance), on the device.
//
// C = (J^T J)^-1 of the UNDAMPED, unscaled problem, not multiplied by a residual variance (as in Ceres).  For a bundle adjustment
// with H = [[U, E], [E^T, V]] (cameras | landmarks) the Schur form gives
//   Sigma_cc = S^-1,  S = U - E V^-1 E^T                               (the engine's reduced camera system, zero damping)
//   Sigma_jj = V_j^-1 + sum_{a, b in cams(j)} F_a^T Sigma_cc[a, b] F_b,   F_a = E_{a,j} V_j^-1
// E_{a,j} is a sum over the observations of landmark j by camera a, so the double sum runs over PAIRS OF OBSERVATIONS of the
// landmark (F_i = Jc_i^T Jp_i V_j^-1 per observation): a camera that sees the landmark twice is the sum of its two terms.
// The off-diagonal blocks of the full inverse are made of the same pieces, nothing more is inverted:
//   Sigma[a, j] (6 x 3) = - sum_{i in obs(j)} Sigma_cc[a, cam(i)] F_i
//   Sigma[j, k] (3 x 3) =   sum_{x in obs(j)} sum_{y in obs(k)} F_x^T Sigma_cc[cam(x), cam(y)] F_y              (j != k)
//
//   cov_spd_inverse_packed   S (or a dense J^T J) -> W = [S . ; I 0] -> chol_spd_inverse_dev (dense_chol.hip) -> the lower
//                            triangle of S^-1, packed (row i at i (i + 1) / 2: 144 MB at 6000 unknowns), and the pivot ratio
//   cov_point_rcond_kernel   pivot ratio of every free V_j (3 x 3 LDL^T)
//   cov_point_kernel         the landmark marginals: one wave per landmark, F of up to 2 x 32 observations staged in LDS, the
//                            6 x 6 blocks of Sigma_cc read straight from the packed triangle, one pair of observations per lane
//                            and trip, a fixed order and a fixed shuffle reduction: bitwise reproducible, no atomics
//   cov_camera_kernel        6 x 6 blocks (a, b) of Sigma_cc, constant dofs zeroed
//   cov_cam_point_kernel     camera-landmark blocks: one wave per pair, one observation of the landmark per lane, F in registers
//   cov_point_pair_kernel    landmark-landmark blocks: one wave per pair, the staging and the per-pair product of cov_point_kernel
//                            (cov_form_F, cov_Ft_sigma_F), smaller index first and the transpose for a swapped request
// The pivot ratio (smallest pivot / largest pivot of the Cholesky factorisation) is a cheap stand-in for a reciprocal condition
// number, not an estimate of one: a ratio above the threshold does not prove the matrix well conditioned.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "ba_kernels.hpp"

namespace stba {

struct CovStore {
    int nc = 0, np = 0, n = 0;
    hipStream_t st = nullptr;
    DevBuf<double> sig;          // Sigma_cc, packed lower triangle
    DevBuf<double> vinv6;        // [np][6] V_j^-1 (xx xy xz yy yz zz), zero for constant landmarks
    DevBuf<double> J8;           // the linearisation the marginals are made from (a later solve overwrites the engine's)
    DevBuf<double> Jc12;         // host-linearised factors only
    const int* pt_start = nullptr; const int* obs_cam = nullptr;          // the engine's (fixed at its creation)
    const unsigned char* omask = nullptr; const unsigned char* cam_fixed = nullptr;
};

void cov_store_free(CovStore* c) {
    if (!c) return;
    if (c->st) (void)hipStreamSynchronize(c->st);      // (then the store: its buffers go with it)
    delete c;
}

__device__ inline double packed_at(const double* __restrict__ sig, int i, int j) {
    return i >= j ? sig[(size_t)i * (i + 1) / 2 + j] : sig[(size_t)j * (j + 1) / 2 + i];
}

// W (ldw = 2 np) = [A . ; I 0]: the lower triangle of A (n x n, leading dimension lda) in the upper left, identity on the padding
// rows [n, np), the identity below; everything else zero
__global__ __launch_bounds__(256) void cov_layout_kernel(const double* __restrict__ A, int lda, int n, int np, double* __restrict__ W) {
    const int r = blockIdx.x, ldw = 2 * np;
    double* row = W + (size_t)r * ldw;
    for (int c = threadIdx.x; c < ldw; c += 256) {
        double v = 0.0;
        if (r < np) {
            if (c <= r) v = (r < n) ? A[(size_t)r * lda + c] : (c == r ? 1.0 : 0.0);
        } else if (c == r - np) v = 1.0;
        row[c] = v;
    }
}

// smallest and largest Cholesky pivot L_ii^2 over the rows [0, n) that are not constant dofs (cam_fixed: bit a of byte i / 6
// marks row i; null: none) -> out[0], out[1]
__global__ __launch_bounds__(256) void cov_pivots_kernel(const double* __restrict__ W, int ldw, int n, const unsigned char* __restrict__ cam_fixed,
                                                         double* __restrict__ out) {
    __shared__ double smin[256], smax[256];
    double lo = INFINITY, hi = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        if (cam_fixed && ((cam_fixed[i / 6] >> (i % 6)) & 1u)) continue;
        const double l = W[(size_t)i * ldw + i], p = l * l;
        lo = (p == p) ? fmin(lo, p) : 0.0;
        hi = fmax(hi, p);
    }
    smin[threadIdx.x] = lo; smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + s]);
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = smin[0]; out[1] = smax[0]; }
}

// the lower right block of W holds -A^-1 (lower triangle) -> packed triangle of A^-1
__global__ __launch_bounds__(256) void cov_pack_kernel(const double* __restrict__ W, int np, double* __restrict__ sig) {
    const int i = blockIdx.x, ldw = 2 * np;
    const double* src = W + (size_t)(np + i) * ldw + np;
    double* dst = sig + (size_t)i * (i + 1) / 2;
    for (int c = threadIdx.x; c <= i; c += 256) dst[c] = -src[c];
}

int cov_spd_inverse_packed(const double* A, int lda, int n, const unsigned char* cam_fixed, double* sig, double* rcond, int* pivot_row,
                           hipStream_t st) {
    const int np = (n + CHOL_NB - 1) / CHOL_NB * CHOL_NB, ldw = 2 * np;
    DevBuf<double> W, work, piv;
    DevBuf<int> flag;
    STBA_TRY(W.alloc((size_t)ldw * ldw));
    STBA_TRY(work.alloc(chol_spd_inverse_workspace_doubles(np)));
    STBA_TRY(piv.alloc(2));
    STBA_TRY(flag.alloc(1));
    hipLaunchKernelGGL(cov_layout_kernel, dim3(ldw), dim3(256), 0, st, A, lda, n, np, W);
    STBA_HIP(hipGetLastError());
    STBA_TRY(chol_spd_inverse_dev(W, ldw, np, n, flag, work, st));
    hipLaunchKernelGGL(cov_pivots_kernel, dim3(1), dim3(256), 0, st, W, ldw, n, cam_fixed, piv);
    hipLaunchKernelGGL(cov_pack_kernel, dim3(n), dim3(256), 0, st, W, np, sig);
    STBA_HIP(hipGetLastError());
    double h[2] = {0.0, 0.0};
    int flag_h = 0;
    STBA_HIP(hipMemcpyAsync(h, piv, sizeof h, hipMemcpyDeviceToHost, st));
    STBA_HIP(hipMemcpyAsync(&flag_h, flag, sizeof flag_h, hipMemcpyDeviceToHost, st));
    STBA_HIP(hipStreamSynchronize(st));
    *pivot_row = flag_h;
    *rcond = flag_h ? 0.0 : (h[1] > 0.0 ? (std::isinf(h[0]) ? 1.0 : h[0] / h[1]) : 1.0);    // (no free row: 1)
    return STBA_OK;
}

// pivot ratio of V_j = Hpp_j (3 x 3 LDL^T, 0 if a pivot is not positive) for every free landmark; per workgroup of 256 landmarks:
// {landmarks below min_rcond, the first of them (n_pts if none), the smallest ratio}
__global__ __launch_bounds__(256) void cov_point_rcond_kernel(int n_pts, const double* __restrict__ Hpp6, const unsigned char* __restrict__ pt_fixed,
                                                              double min_rcond, double* __restrict__ partial) {
    __shared__ int s_cnt[256], s_first[256];
    __shared__ double s_min[256];
    const int j = blockIdx.x * 256 + threadIdx.x;
    int bad = 0, first = n_pts;
    double rc = 1.0;
    if (j < n_pts && !(pt_fixed && pt_fixed[j])) {
        const double* a = Hpp6 + (size_t)j * 6;
        const double d0 = a[0];
        const double l10 = a[1] / d0, l20 = a[2] / d0;
        const double d1 = a[3] - l10 * a[1];
        const double e12 = a[4] - l20 * a[1];
        const double d2 = a[5] - l20 * a[2] - e12 * e12 / d1;
        if (!(d0 > 0.0) || !(d1 > 0.0) || !(d2 > 0.0)) rc = 0.0;
        else rc = fmin(d0, fmin(d1, d2)) / fmax(d0, fmax(d1, d2));
        if (!(rc >= min_rcond)) { bad = 1; first = j; }
    }
    s_cnt[threadIdx.x] = bad; s_first[threadIdx.x] = first; s_min[threadIdx.x] = rc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + s];
            s_first[threadIdx.x] = min(s_first[threadIdx.x], s_first[threadIdx.x + s]);
            s_min[threadIdx.x] = fmin(s_min[threadIdx.x], s_min[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[(size_t)blockIdx.x * 3] = (double)s_cnt[0];
        partial[(size_t)blockIdx.x * 3 + 1] = (double)s_first[0];
        partial[(size_t)blockIdx.x * 3 + 2] = s_min[0];
    }
}

// Sigma_cc blocks (a, b), 6 x 6 row-major each; entries of constant dofs are zero
__global__ __launch_bounds__(256) void cov_camera_kernel(const double* __restrict__ sig, const unsigned char* __restrict__ cam_fixed, int n_pairs,
                                                         const int* __restrict__ ca, const int* __restrict__ cb, double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n_pairs * 36) return;
    const int k = (int)(e / 36), r = (int)(e % 36) / 6, c = (int)(e % 6);
    const int a = ca[k], b = cb[k];
    const bool fx = cam_fixed && (((cam_fixed[a] >> r) & 1u) || ((cam_fixed[b] >> c) & 1u));
    out[e] = fx ? 0.0 : packed_at(sig, 6 * a + r, 6 * b + c);
}

// Landmark marginals, one 64-lane workgroup (one wave) per requested landmark.  The observations of landmark j are the
// contiguous range [pt_start[j], pt_start[j + 1]) of the engine's order; they are taken in chunks of CV_CHUNK, and for every pair
// of chunks (A <= B) lanes 0..31 stage F = Jc^T Jp V^-1 (6 x 3) of chunk A and lanes 32..63 those of chunk B in LDS.  Then every
// lane takes pairs of observations (x in A, y in B, x <= y when A == B) in a fixed stride and adds X = F_x^T Sigma[c_x, c_y] F_y
// (X + X^T for x != y) to its six sums; a butterfly of shuffles adds the 64 lanes.  Per pair: one 6 x 6 block of the packed
// triangle (288 B: the whole triangle is 144 MB at C5 and stays in the Infinity Cache), 162 FMAs.
constexpr int CV_CHUNK = 32, CV_LD = 19;      // (odd stride: the 18 doubles of neighbouring observations start in different banks)

// what the three block kernels share.  F = Jc^T Jp V^-1 (6 x 3 row-major) of observation i, Vf = V^-1 of its landmark as a full 3 x 3
template <bool GEN>
__device__ __forceinline__ void cov_form_F(const double* __restrict__ J8, const unsigned char* __restrict__ omask, const double* __restrict__ Jc12,
                                           int i, const double Vf[9], double* F) {
    double jc[12], jp[6];
    load_jc_jp<GEN>(J8, omask, i, jc, jp, Jc12);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const double e0 = jc[r] * jp[0] + jc[6 + r] * jp[3];
        const double e1 = jc[r] * jp[1] + jc[6 + r] * jp[4];
        const double e2 = jc[r] * jp[2] + jc[6 + r] * jp[5];
#pragma unroll
        for (int k = 0; k < 3; ++k) F[r * 3 + k] = e0 * Vf[k] + e1 * Vf[3 + k] + e2 * Vf[6 + k];
    }
}

// T (6 x 3) = Sigma_cc[rows rx .. rx + 6, columns ry .. ry + 6] F_y, the block read straight from the packed triangle
__device__ __forceinline__ void cov_sigma_F(const double* __restrict__ sig, int rx, int ry, const double* Fy, double T[18]) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double s = packed_at(sig, rx + r, ry + c);
            t0 += s * Fy[c * 3]; t1 += s * Fy[c * 3 + 1]; t2 += s * Fy[c * 3 + 2];
        }
        T[r * 3] = t0; T[r * 3 + 1] = t1; T[r * 3 + 2] = t2;
    }
}

// X (3 x 3) = F_x^T Sigma_cc[rx .., ry ..] F_y
__device__ __forceinline__ void cov_Ft_sigma_F(const double* __restrict__ sig, const double* Fx, int rx, const double* Fy, int ry, double X[9]) {
    double T[18];
    cov_sigma_F(sig, rx, ry, Fy, T);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) s += Fx[r * 3 + k] * T[r * 3 + l];
            X[k * 3 + l] = s;
        }
}

template <bool GEN>
__global__ __launch_bounds__(64) void cov_point_kernel(const int* __restrict__ req, const int* __restrict__ pt_start, const int* __restrict__ obs_cam,
                                                       const double* __restrict__ J8, const unsigned char* __restrict__ omask,
                                                       const double* __restrict__ Jc12, const double* __restrict__ vinv6,
                                                       const double* __restrict__ sig, double* __restrict__ out) {
    __shared__ double sf[2][CV_CHUNK * CV_LD];
    __shared__ int sc[2][CV_CHUNK];
    const int t = threadIdx.x;
    const int j = req ? req[blockIdx.x] : (int)blockIdx.x;
    double V[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) V[k] = vinv6[(size_t)j * 6 + k];
    const double Vf[9] = {V[0], V[1], V[2], V[1], V[3], V[4], V[2], V[4], V[5]};
    const int o0 = pt_start[j], m = pt_start[j + 1] - o0;
    const bool constant = V[0] == 0.0 && V[3] == 0.0 && V[5] == 0.0;      // (constant landmark: V^-1 = 0, so every F is 0)
    const int nch = constant ? 0 : (m + CV_CHUNK - 1) / CV_CHUNK;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int ia = 0; ia < nch; ++ia)
        for (int ib = ia; ib < nch; ++ib) {
            __syncthreads();                 // (the previous pair of chunks has been read)
            {
                const int half = t >> 5, lt = t & 31;
                const int o = (half ? ib : ia) * CV_CHUNK + lt;
                if (o < m) {
                    cov_form_F<GEN>(J8, omask, Jc12, o0 + o, Vf, sf[half] + lt * CV_LD);
                    sc[half][lt] = obs_cam[o0 + o];
                }
            }
            __syncthreads();
            const int na = min(CV_CHUNK, m - ia * CV_CHUNK), nb = min(CV_CHUNK, m - ib * CV_CHUNK);
            const bool same = ia == ib;
            const int npairs = same ? na * (na + 1) / 2 : na * nb;
            for (int p = t; p < npairs; p += 64) {
                int x, y;
                if (same) {      // p -> (x <= y): y (y + 1) / 2 <= p < (y + 1) (y + 2) / 2
                    y = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
                    while (y * (y + 1) / 2 > p) --y;
                    while ((y + 1) * (y + 2) / 2 <= p) ++y;
                    x = p - y * (y + 1) / 2;
                } else { x = p / nb; y = p % nb; }
                const double* Fx = sf[0] + x * CV_LD;
                const double* Fy = sf[same ? 0 : 1] + y * CV_LD;
                const int rx = 6 * sc[0][x], ry = 6 * sc[same ? 0 : 1][y];
                double X[9];
                cov_Ft_sigma_F(sig, Fx, rx, Fy, ry, X);
                if (same && x == y) {
                    acc[0] += X[0]; acc[1] += X[1]; acc[2] += X[2]; acc[3] += X[4]; acc[4] += X[5]; acc[5] += X[8];
                } else {
                    acc[0] += 2.0 * X[0]; acc[1] += X[1] + X[3]; acc[2] += X[2] + X[6];
                    acc[3] += 2.0 * X[4]; acc[4] += X[5] + X[7]; acc[5] += 2.0 * X[8];
                }
            }
        }
#pragma unroll
    for (int k = 0; k < 6; ++k)
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    if (t == 0) {
        double* o = out + (size_t)blockIdx.x * 9;
        const double s[6] = {V[0] + acc[0], V[1] + acc[1], V[2] + acc[2], V[3] + acc[3], V[4] + acc[4], V[5] + acc[5]};
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
        o[3] = s[1]; o[4] = s[3]; o[5] = s[4];
        o[6] = s[2]; o[7] = s[4]; o[8] = s[5];
    }
}

// Landmark-landmark blocks Sigma[j, k] = sum_{x in obs(j), y in obs(k)} F_x^T Sigma_cc[c_x, c_y] F_y (j != k: no V^-1 term, no
// symmetry), one wave per requested pair.  It is the two-different-chunks case of cov_point_kernel: lanes 0..31 stage a chunk of
// the first landmark with its V^-1, lanes 32..63 a chunk of the second with its own, then one pair of observations per lane and
// trip.  The pair is computed with the smaller landmark index first and written transposed for a swapped request, so that
// Sigma[k, j] is bitwise Sigma[j, k]^T.  A constant landmark (V^-1 = 0) gives exact zeros.  (j == k never gets here: the host sends
// it through cov_point_kernel.)
template <bool GEN>
__global__ __launch_bounds__(64) void cov_point_pair_kernel(const int* __restrict__ req_a, const int* __restrict__ req_b, const int* __restrict__ pt_start,
                                                            const int* __restrict__ obs_cam, const double* __restrict__ J8,
                                                            const unsigned char* __restrict__ omask, const double* __restrict__ Jc12,
                                                            const double* __restrict__ vinv6, const double* __restrict__ sig, double* __restrict__ out) {
    __shared__ double sf[2][CV_CHUNK * CV_LD];
    __shared__ int sc[2][CV_CHUNK];
    const int t = threadIdx.x, half = t >> 5, lt = t & 31;
    const int ra = req_a[blockIdx.x], rb = req_b[blockIdx.x];
    const bool swapped = ra > rb;
    const int j = swapped ? rb : ra, k = swapped ? ra : rb;
    double Vj[6], Vk[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) { Vj[q] = vinv6[(size_t)j * 6 + q]; Vk[q] = vinv6[(size_t)k * 6 + q]; }
    const bool constant = (Vj[0] == 0.0 && Vj[3] == 0.0 && Vj[5] == 0.0) || (Vk[0] == 0.0 && Vk[3] == 0.0 && Vk[5] == 0.0);
    double V[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) V[q] = half ? Vk[q] : Vj[q];
    const double Vf[9] = {V[0], V[1], V[2], V[1], V[3], V[4], V[2], V[4], V[5]};
    const int oj = pt_start[j], mj = pt_start[j + 1] - oj, ok = pt_start[k], mk = pt_start[k + 1] - ok;
    const int o0 = half ? ok : oj, m = half ? mk : mj;            // (the landmark whose chunk this lane stages)
    const int nca = constant ? 0 : (mj + CV_CHUNK - 1) / CV_CHUNK, ncb = (mk + CV_CHUNK - 1) / CV_CHUNK;
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int ia = 0; ia < nca; ++ia)
        for (int ib = 0; ib < ncb; ++ib) {
            __syncthreads();                 // (the previous pair of chunks has been read)
            {
                const int o = (half ? ib : ia) * CV_CHUNK + lt;
                if (o < m) {
                    cov_form_F<GEN>(J8, omask, Jc12, o0 + o, Vf, sf[half] + lt * CV_LD);
                    sc[half][lt] = obs_cam[o0 + o];
                }
            }
            __syncthreads();
            const int na = min(CV_CHUNK, mj - ia * CV_CHUNK), nb = min(CV_CHUNK, mk - ib * CV_CHUNK);
            for (int p = t; p < na * nb; p += 64) {
                const int x = p / nb, y = p % nb;
                double X[9];
                cov_Ft_sigma_F(sig, sf[0] + x * CV_LD, 6 * sc[0][x], sf[1] + y * CV_LD, 6 * sc[1][y], X);
#pragma unroll
                for (int q = 0; q < 9; ++q) acc[q] += X[q];
            }
        }
#pragma unroll
    for (int q = 0; q < 9; ++q)
        for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_xor(acc[q], off, 64);
    if (t == 0) {
        double* o = out + (size_t)blockIdx.x * 9;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[swapped ? c * 3 + r : r * 3 + c] = acc[r * 3 + c];
    }
}

// Camera-landmark blocks Sigma[a, j] = - sum_{i in obs(j)} Sigma_cc[a, c_i] F_i (6 x 3), one wave per requested pair, one
// observation of the landmark per lane in trips of 64: F_i in registers, times the 6 x 6 block of the packed triangle; the 18 sums
// go through the same butterfly.  Rows of constant dofs of camera a are written as zero (the packed triangle is not zero there),
// a constant landmark gives exact zeros.
template <bool GEN>
__global__ __launch_bounds__(64) void cov_cam_point_kernel(const int* __restrict__ req_cam, const int* __restrict__ req_pt, const int* __restrict__ pt_start,
                                                           const int* __restrict__ obs_cam, const double* __restrict__ J8,
                                                           const unsigned char* __restrict__ omask, const double* __restrict__ Jc12,
                                                           const double* __restrict__ vinv6, const double* __restrict__ sig,
                                                           const unsigned char* __restrict__ cam_fixed, double* __restrict__ out) {
    const int t = threadIdx.x;
    const int a = req_cam[blockIdx.x], j = req_pt[blockIdx.x];
    double V[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) V[q] = vinv6[(size_t)j * 6 + q];
    const double Vf[9] = {V[0], V[1], V[2], V[1], V[3], V[4], V[2], V[4], V[5]};
    const int o0 = pt_start[j], m = pt_start[j + 1] - o0;
    const bool constant = V[0] == 0.0 && V[3] == 0.0 && V[5] == 0.0;
    double acc[18];
#pragma unroll
    for (int q = 0; q < 18; ++q) acc[q] = 0.0;
    for (int o = t; o < (constant ? 0 : m); o += 64) {
        double F[18], T[18];
        cov_form_F<GEN>(J8, omask, Jc12, o0 + o, Vf, F);
        cov_sigma_F(sig, 6 * a, 6 * obs_cam[o0 + o], F, T);
#pragma unroll
        for (int q = 0; q < 18; ++q) acc[q] += T[q];
    }
#pragma unroll
    for (int q = 0; q < 18; ++q)
        for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_xor(acc[q], off, 64);
    if (t == 0) {
        double* o = out + (size_t)blockIdx.x * 18;
        const unsigned fx = cam_fixed ? cam_fixed[a] : 0u;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[r * 3 + c] = ((fx >> r) & 1u) ? 0.0 : 0.0 - acc[r * 3 + c];
    }
}

// ---------------------------------------------------------------------------------------------
int cov_compute(const BaCovInputs& in, double min_rcond, CovStore** out, double* rcond_out) {
    *out = nullptr;
    hipStream_t st = in.st;
    // landmarks first: a singular V_j makes S meaningless
    double rc_pts = 1.0;
    if (in.np > 0) {
        const int nb = (in.np + 255) / 256;
        DevBuf<double> dpart;
        STBA_TRY(dpart.alloc((size_t)nb * 3));
        std::vector<double> part((size_t)nb * 3);
        hipLaunchKernelGGL(cov_point_rcond_kernel, dim3(nb), dim3(256), 0, st, in.np, in.Hpp6, in.pt_fixed, min_rcond, dpart);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(part.data(), dpart, part.size() * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        dpart.reset();
        if (e != hipSuccess) return fail(STBA_ERR_HIP, std::string("covariance: landmark pivots: ") + hipGetErrorString(e));
        long bad = 0;
        int first = in.np;
        for (int b = 0; b < nb; ++b) {
            bad += (long)part[(size_t)b * 3];
            first = std::min(first, (int)part[(size_t)b * 3 + 1]);
            rc_pts = std::min(rc_pts, part[(size_t)b * 3 + 2]);
        }
        if (bad > 0) {
            char buf[32];
            snprintf(buf, sizeof buf, "%.3e", min_rcond);
            return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, "covariance: " + std::to_string(bad) + " free landmark(s) with a pivot ratio of V_j below " +
                        buf + " (rank deficient or nearly so), the first is landmark " + std::to_string(first));
        }
    }
    std::unique_ptr<CovStore, void (*)(CovStore*)> c(new CovStore, cov_store_free);
    c->nc = in.nc; c->np = in.np; c->n = in.n; c->st = st;
    c->pt_start = in.pt_start; c->obs_cam = in.obs_cam; c->omask = in.omask; c->cam_fixed = in.cam_fixed;
    double rc_s = 1.0;
    if (in.n > 0) {
        STBA_TRY(c->sig.alloc((size_t)in.n * (in.n + 1) / 2));
        int piv = 0;
        STBA_TRY(cov_spd_inverse_packed(in.S, in.lda, in.n, in.cam_fixed, c->sig, &rc_s, &piv, st));
        if (piv)
            return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, "covariance: the reduced camera system S is not positive definite (pivot of row " +
                        std::to_string(piv - 1) + ", camera " + std::to_string((piv - 1) / 6) + ")");
        if (!(rc_s >= min_rcond)) {
            char buf[64];
            snprintf(buf, sizeof buf, "%.3e", rc_s);
            return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, std::string("covariance: the reduced camera system S has a pivot ratio of ") + buf +
                        ", below min_reciprocal_condition_number (is the gauge fixed?)");
        }
    }
    STBA_TRY(c->vinv6.alloc((size_t)std::max(in.np, 1) * 6));
    STBA_TRY(c->J8.alloc((size_t)std::max(in.no, 1) * 8));
    if (in.np) STBA_HIP(hipMemcpyAsync(c->vinv6, in.Hinv6, (size_t)in.np * 6 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (in.no) STBA_HIP(hipMemcpyAsync(c->J8, in.J8, (size_t)in.no * 8 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (in.Jc12) {
        STBA_TRY(c->Jc12.alloc((size_t)std::max(in.no, 1) * 12));
        if (in.no) STBA_HIP(hipMemcpyAsync(c->Jc12, in.Jc12, (size_t)in.no * 12 * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    STBA_HIP(hipStreamSynchronize(st));
    if (rcond_out) *rcond_out = std::min(rc_s, rc_pts);
    *out = c.release();
    return STBA_OK;
}

int cov_camera_blocks(const CovStore* c, int n_pairs, const int* cam_a, const int* cam_b, double* out) {
    if (n_pairs <= 0) return STBA_OK;
    for (int k = 0; k < n_pairs; ++k)
        if (cam_a[k] < 0 || cam_a[k] >= c->nc || cam_b[k] < 0 || cam_b[k] >= c->nc)
            return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_camera_covariance: camera index out of range in pair " + std::to_string(k));
    DevBuf<int> da, db;
    DevBuf<double> dout;
    STBA_TRY(da.alloc((size_t)n_pairs)); STBA_TRY(db.alloc((size_t)n_pairs)); STBA_TRY(dout.alloc((size_t)n_pairs * 36));
    STBA_HIP(hipMemcpyAsync(da, cam_a, (size_t)n_pairs * sizeof(int), hipMemcpyHostToDevice, c->st));
    STBA_HIP(hipMemcpyAsync(db, cam_b, (size_t)n_pairs * sizeof(int), hipMemcpyHostToDevice, c->st));
    const size_t ne = (size_t)n_pairs * 36;
    hipLaunchKernelGGL(cov_camera_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, c->st, c->sig, c->cam_fixed, n_pairs, da, db, dout);
    STBA_HIP(hipGetLastError());
    STBA_HIP(hipMemcpyAsync(out, dout, ne * sizeof(double), hipMemcpyDeviceToHost, c->st));
    STBA_HIP(hipStreamSynchronize(c->st));
    return STBA_OK;
}

int cov_point_blocks(const CovStore* c, int n, const int* pts, double* out) {
    if (n <= 0) return STBA_OK;
    if (pts)
        for (int k = 0; k < n; ++k)
            if (pts[k] < 0 || pts[k] >= c->np)
                return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_point_covariance: landmark index out of range at position " + std::to_string(k));
    if (!pts && n != c->np) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_point_covariance: pts = NULL asks for all n_pts landmarks");
    DevBuf<int> dreq;
    DevBuf<double> dout;
    if (pts) {
        STBA_TRY(dreq.alloc((size_t)n));
        STBA_HIP(hipMemcpyAsync(dreq, pts, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->st));
    }
    STBA_TRY(dout.alloc((size_t)n * 9));
    if (c->Jc12)
        hipLaunchKernelGGL(cov_point_kernel<true>, dim3(n), dim3(64), 0, c->st, dreq, c->pt_start, c->obs_cam, c->J8, c->omask, c->Jc12, c->vinv6, c->sig, dout);
    else
        hipLaunchKernelGGL(cov_point_kernel<false>, dim3(n), dim3(64), 0, c->st, dreq, c->pt_start, c->obs_cam, c->J8, c->omask, c->Jc12, c->vinv6, c->sig, dout);
    STBA_HIP(hipGetLastError());
    STBA_HIP(hipMemcpyAsync(out, dout, (size_t)n * 9 * sizeof(double), hipMemcpyDeviceToHost, c->st));
    STBA_HIP(hipStreamSynchronize(c->st));
    return STBA_OK;
}

int cov_cam_point_blocks(const CovStore* c, int n_pairs, const int* cam, const int* pt, double* out) {
    if (n_pairs <= 0) return STBA_OK;
    for (int k = 0; k < n_pairs; ++k) {
        if (cam[k] < 0 || cam[k] >= c->nc)
            return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_camera_point_covariance: camera index out of range in pair " + std::to_string(k));
        if (pt[k] < 0 || pt[k] >= c->np)
            return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_camera_point_covariance: landmark index out of range in pair " + std::to_string(k));
    }
    DevBuf<int> da, db;
    DevBuf<double> dout;
    STBA_TRY(da.alloc((size_t)n_pairs)); STBA_TRY(db.alloc((size_t)n_pairs)); STBA_TRY(dout.alloc((size_t)n_pairs * 18));
    STBA_HIP(hipMemcpyAsync(da, cam, (size_t)n_pairs * sizeof(int), hipMemcpyHostToDevice, c->st));
    STBA_HIP(hipMemcpyAsync(db, pt, (size_t)n_pairs * sizeof(int), hipMemcpyHostToDevice, c->st));
    if (c->Jc12)
        hipLaunchKernelGGL(cov_cam_point_kernel<true>, dim3(n_pairs), dim3(64), 0, c->st, da, db, c->pt_start, c->obs_cam, c->J8, c->omask, c->Jc12, c->vinv6, c->sig, c->cam_fixed, dout);
    else
        hipLaunchKernelGGL(cov_cam_point_kernel<false>, dim3(n_pairs), dim3(64), 0, c->st, da, db, c->pt_start, c->obs_cam, c->J8, c->omask, c->Jc12, c->vinv6, c->sig, c->cam_fixed, dout);
    STBA_HIP(hipGetLastError());
    STBA_HIP(hipMemcpyAsync(out, dout, (size_t)n_pairs * 18 * sizeof(double), hipMemcpyDeviceToHost, c->st));
    STBA_HIP(hipStreamSynchronize(c->st));
    return STBA_OK;
}

int cov_point_pair_blocks(const CovStore* c, int n_pairs, const int* pt_a, const int* pt_b, double* out) {
    if (n_pairs <= 0) return STBA_OK;
    for (int k = 0; k < n_pairs; ++k)
        if (pt_a[k] < 0 || pt_a[k] >= c->np || pt_b[k] < 0 || pt_b[k] >= c->np)
            return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_point_pair_covariance: landmark index out of range in pair " + std::to_string(k));
    // a landmark with itself is the marginal (it has the V_j^-1 term): those go through cov_point_kernel, the rest in one launch here
    std::vector<int> off_pos, off_a, off_b, diag_pos, diag_pt;
    for (int k = 0; k < n_pairs; ++k) {
        if (pt_a[k] == pt_b[k]) { diag_pos.push_back(k); diag_pt.push_back(pt_a[k]); }
        else { off_pos.push_back(k); off_a.push_back(pt_a[k]); off_b.push_back(pt_b[k]); }
    }
    const int n_off = (int)off_pos.size(), n_diag = (int)diag_pos.size();
    std::vector<double> res((size_t)n_pairs * 9);          // (out is written only once everything has come home)
    if (n_off > 0) {
        DevBuf<int> da, db;
        DevBuf<double> dout;
        STBA_TRY(da.alloc((size_t)n_off)); STBA_TRY(db.alloc((size_t)n_off)); STBA_TRY(dout.alloc((size_t)n_off * 9));
        STBA_HIP(hipMemcpyAsync(da, off_a.data(), (size_t)n_off * sizeof(int), hipMemcpyHostToDevice, c->st));
        STBA_HIP(hipMemcpyAsync(db, off_b.data(), (size_t)n_off * sizeof(int), hipMemcpyHostToDevice, c->st));
        if (c->Jc12)
            hipLaunchKernelGGL(cov_point_pair_kernel<true>, dim3(n_off), dim3(64), 0, c->st, da, db, c->pt_start, c->obs_cam, c->J8, c->omask, c->Jc12, c->vinv6, c->sig, dout);
        else
            hipLaunchKernelGGL(cov_point_pair_kernel<false>, dim3(n_off), dim3(64), 0, c->st, da, db, c->pt_start, c->obs_cam, c->J8, c->omask, c->Jc12, c->vinv6, c->sig, dout);
        STBA_HIP(hipGetLastError());
        STBA_HIP(hipMemcpyAsync(res.data(), dout, (size_t)n_off * 9 * sizeof(double), hipMemcpyDeviceToHost, c->st));
        STBA_HIP(hipStreamSynchronize(c->st));
    }
    if (n_diag > 0) STBA_TRY(cov_point_blocks(c, n_diag, diag_pt.data(), res.data() + (size_t)n_off * 9));
    for (int q = 0; q < n_off; ++q) std::copy(res.begin() + (size_t)q * 9, res.begin() + (size_t)(q + 1) * 9, out + (size_t)off_pos[q] * 9);
    for (int q = 0; q < n_diag; ++q)
        std::copy(res.begin() + (size_t)(n_off + q) * 9, res.begin() + (size_t)(n_off + q + 1) * 9, out + (size_t)diag_pos[q] * 9);
    return STBA_OK;
}

}  // namespace stba
