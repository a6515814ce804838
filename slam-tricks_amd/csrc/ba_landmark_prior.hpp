// ba_landmark_prior.hpp -- landmark position priors (control points) of the bundle adjustment: the factor's maths
// (host and device), the host's check of one prior's weight, and the launch wrappers of its two kernels (definitions in
// ba_landmark_prior.hip)
#pragma once
#if defined(__HIPCC__)
#include "common.hpp"
#else
// a plain host compiler (tests/cpp/ba_landmark_prior_driver.cpp): the factor's maths only, nothing of HIP
#include <cmath>
#ifndef STBA_MATHS_ONLY
#define STBA_MATHS_ONLY
#endif
#ifndef __host__
#define __host__
#define __device__
#endif
#endif
#include "ba_factor_input.hpp"

namespace stba {

// A prior k on landmark j: r = p_j - ph, J = I (0 for a constant landmark: the prior then only costs); whitened r' = W r, J' = W J,
// cost += |r'|^2 / 2, W any 3 x 3 (row-major).
//
// Like ba_prior.hpp's, the whitening is kept free of FMA contraction and in ONE order: W r cancels for a tight prior far from the
// iterate (|W r| << sum |W| |r|), so what another order moves is not small against the result, and the numpy restatement the tests
// hold the kernels against states this order.
// clang (hipcc, for the device and the host) honours the pragma inside each function.  GCC does not know it and contracts by default
// (-ffp-contract=fast) wherever the target has FMA (-march=native, -mfma): there the functions carry the optimize attribute instead,
// which also keeps GCC from inlining them into a caller that contracts (tests/test_ba_landmark_prior_reference_cpu.py reads the
// assembly of a -mfma build)
#ifndef STBA_LP_NO_CONTRACT          // (the test defines it empty to see that the compiler at hand WOULD contract)
#if defined(__GNUC__) && !defined(__clang__)
#define STBA_LP_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define STBA_LP_NO_CONTRACT
#endif
#endif
STBA_LP_NO_CONTRACT __host__ __device__ inline double lp_row_dot(const double* Wi, const double* r) {
#pragma clang fp contract(off)
    return (Wi[0] * r[0] + Wi[1] * r[1]) + Wi[2] * r[2];
}
// r' [3] of one prior at the landmark position p
STBA_LP_NO_CONTRACT __host__ __device__ inline void lp_residual(const double* W, const double* pos, const double* p, double* rw) {
#pragma clang fp contract(off)
    const double r[3] = {p[0] - pos[0], p[1] - pos[1], p[2] - pos[2]};
    for (int i = 0; i < 3; ++i) rw[i] = lp_row_dot(W + 3 * i, r);
}
// entry (a, b) of W^T W: the three products in row order.  (a, b) and (b, a) are the same products in the same order
STBA_LP_NO_CONTRACT __host__ __device__ inline double lp_wtw(const double* W, int a, int b) {
#pragma clang fp contract(off)
    return (W[a] * W[b] + W[3 + a] * W[3 + b]) + W[6 + a] * W[6 + b];
}
// entry a of W^T r'
STBA_LP_NO_CONTRACT __host__ __device__ inline double lp_wtr(const double* W, const double* rw, int a) {
#pragma clang fp contract(off)
    return (W[a] * rw[0] + W[3 + a] * rw[1]) + W[6 + a] * rw[2];
}

// Omega = L L^T, W = L^T of ONE symmetric positive definite 3 x 3 (row-major; the lower triangle is factored): the tree's one
// factorisation (information6_factor, dd6.hpp: double-double), on the 3 x 3 embedded in a 6 x 6 with an identity tail -- the leading
// 3 x 3 of that factor is the factor of the 3 x 3, the tail's pivots are 1.  false: an entry that is not finite, or a pivot that
// is not a positive finite number
inline bool landmark_information_factor(const double* A, double* W) {
    double A6[36], W6[36];
    for (int k = 0; k < 36; ++k) A6[k] = (k % 7 == 0) ? 1.0 : 0.0;
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) A6[a * 6 + c] = A[a * 3 + c];
    if (!information6_factor(A6, W6)) return false;
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) W[a * 3 + c] = W6[a * 6 + c];
    return true;
}

// the 3 x 3 square-root information W [9] of one prior: the caller's square root as it is (any finite matrix, rank-deficient ones
// included: a height-only control point is one non-zero row), the factor of the caller's information matrix, or -- neither given
// -- the identity
inline int sqrt_information3(const double* information_k, const double* sqrt_information_k, double* W, std::string* why) {
    if (sqrt_information_k) {
        for (int j = 0; j < 9; ++j) {
            if (!std::isfinite(sqrt_information_k[j])) { *why = "the square-root information has an entry that is not finite"; return STBA_ERR_INVALID_ARGUMENT; }
            W[j] = sqrt_information_k[j];
        }
    } else if (information_k) {
        for (int j = 0; j < 9; ++j)
            if (!std::isfinite(information_k[j])) { *why = "the information matrix has an entry that is not finite"; return STBA_ERR_INVALID_ARGUMENT; }
        if (!landmark_information_factor(information_k, W)) { *why = "the information matrix is not positive definite"; return STBA_ERR_NOT_POSITIVE_DEFINITE; }
    } else {
        for (int j = 0; j < 9; ++j) W[j] = (j % 4 == 0) ? 1.0 : 0.0;
    }
    return 0;
}

// one prior's row checked: the landmark index, the position, the weight -> W [9]
inline int landmark_prior_check(int pt, int n_pts, const double* position, const double* information_k, const double* sqrt_information_k,
                                double* W, std::string* why) {
    if (pt < 0 || pt >= n_pts) { *why = "landmark index " + std::to_string(pt) + " out of range"; return STBA_ERR_INVALID_ARGUMENT; }
    for (int j = 0; j < 3; ++j)
        if (!std::isfinite(position[j])) { *why = "the position has an entry that is not finite"; return STBA_ERR_INVALID_ARGUMENT; }
    return sqrt_information3(information_k, sqrt_information_k, W, why);
}

// the priors grouped by landmark (group_csr: a stable sort, inside a group the caller's order) and the groups spread over ALL
// landmarks: start [n_pts + 1], landmark j owns the grouped positions [start[j], start[j + 1]) -- empty for a landmark without
// priors.  order: grouped position -> the caller's index
inline void landmark_prior_group(size_t n, const int* pt, int n_pts, std::vector<int>& order, std::vector<int>& start) {
    order.resize(n);
    for (size_t k = 0; k < n; ++k) order[k] = (int)k;
    std::vector<int> gptr, gpt;
    group_csr(n, [pt](int k) { return pt[k]; }, order, gptr, gpt);
    start.assign((size_t)n_pts + 1, (int)n);
    size_t g = 0;
    for (int j = 0; j <= n_pts; ++j) {
        while (g < gpt.size() && gpt[g] < j) ++g;
        start[(size_t)j] = g < gpt.size() ? gptr[g] : (int)n;
    }
}

#ifndef STBA_MATHS_ONLY
// the priors on the device, in the grouped order
struct LandmarkPriorArgs {
    int n = 0, n_pts = 0;
    const int* start = nullptr;                // [n_pts + 1] into pt / pos / W
    const int* pt = nullptr;                   // [n] landmark of every prior
    const double* pos = nullptr;               // [n][3]
    const double* W = nullptr;                 // [n][9] row-major square-root information
    const unsigned char* pt_fixed = nullptr;   // the engine's per-landmark constant flag, or null
};
constexpr int LP_COST_THREADS = 256, LP_COST_PER_WG = 4 * LP_COST_THREADS;      // cost form: priors per workgroup
constexpr int LP_THREADS = 256;                // block form: one lane per landmark
constexpr int LP_LM_PER_WG = LP_THREADS;
// cost form: sum over every prior of |r'|^2 at the landmarks `pts` -> slot[0]: a workgroup per LP_COST_PER_WG priors of the grouped
// order, each one tree; one workgroup writes the slot, more write part[landmark_prior_cost_grid(n)] and a second launch adds those
// in index order (no atomic; the bits do not depend on anything but the priors and their order)
int landmark_prior_cost_grid(int n);
int launch_landmark_prior_cost(const LandmarkPriorArgs& a, const double* pts, double* part, double* slot, hipStream_t st);
// block form: Hpp6[j] += sum W^T W, gp[j] += sum W^T r' at the landmarks `pts`, a landmark's priors in the caller's order (nothing for
// a constant landmark), and the max |gp| partials of the landmark-block kernel (one per POINT_BLOCK_LANDMARKS landmarks) made again
// from the sums.  Hpp6, gp and gpmax_partial all given or all null; out_r [n][3] and out_J [n][9], in the grouped order, receive
// r' and J' when given
int launch_landmark_prior_blocks(const LandmarkPriorArgs& a, const double* pts, double* Hpp6, double* gp, double* gpmax_partial,
                                 double* out_r, double* out_J, hipStream_t st);

// what the two kernels that sum a model term from the observation records (ba_backsub_kernel's inexact-step model, ba_dogleg_terms_
// kernel) need to add the priors' rows of their landmarks; start == null: no priors
struct LandmarkPriorRows {
    const int* start = nullptr;
    const double* pos = nullptr;
    const double* W = nullptr;
    const double* pts = nullptr;               // the landmarks the records were made at
};
// the priors' rows of landmark j for a step d [3] of it (zero for a constant landmark): the inexact-step model term
// -(W d)^T (r' + W d / 2), summed over the landmark's priors in the caller's order
__device__ inline double lp_model_rows(const LandmarkPriorRows& lp, int j, const double* d) {
    double m = 0.0;
    const double p[3] = {lp.pts[(size_t)j * 3], lp.pts[(size_t)j * 3 + 1], lp.pts[(size_t)j * 3 + 2]};
    for (int k = lp.start[j]; k < lp.start[j + 1]; ++k) {
        const double* W = lp.W + (size_t)k * 9;
        double rw[3];
        lp_residual(W, lp.pos + (size_t)k * 3, p, rw);
        for (int i = 0; i < 3; ++i) {
            const double wd = lp_row_dot(W + 3 * i, d);
            m -= wd * (rw[i] + 0.5 * wd);
        }
    }
    return m;
}
// ... and DOGLEG's three sums over them: |W u|^2, |W y|^2, (W u)^T (W y)
__device__ inline void lp_dogleg_rows(const LandmarkPriorRows& lp, int j, const double* u, const double* y, double* uu, double* nn, double* un) {
    for (int k = lp.start[j]; k < lp.start[j + 1]; ++k) {
        const double* W = lp.W + (size_t)k * 9;
        for (int i = 0; i < 3; ++i) {
            const double e = lp_row_dot(W + 3 * i, u), n = lp_row_dot(W + 3 * i, y);
            *uu += e * e; *nn += n * n; *un += e * n;
        }
    }
}
#endif

}  // namespace stba
