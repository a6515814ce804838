// inner_policy.hpp -- the Levenberg-Marquardt solve of ONE small parameter block of an inner-iteration sweep:
// Ceres' CoordinateDescentMinimizer hands every block of a group to a TrustRegionMinimizer with DEFAULT Solver::Options, and this
// header restates that minimiser for a block of N <= 6 local dofs.  Usable from host and device: it includes nothing but <cmath>,
// so that a plain C++ compiler tests it against the numpy reference (tests/cpp/test_inner_policy.cpp).
//
// The caller gives three callables and keeps the block's parameters:
//   lin(x, H, g)        -> cost = 1/2 sum r^2 of the block's residuals at x, H = J^T J (N x N, row-major), g = J^T r
//   cost_at(x)          -> the cost alone
//   plus(x, d, xn)      x (+) d into xn (ambient A doubles)
// and two ambient measures, norm2(x) = |x|^2 and dist2(x, xn) = |x - xn|^2, over the ambient entries of the block's active
// parts.  `mask` (bit a: dof a is swept) removes the other dofs from the subproblem: their rows and columns of the damped system
// are the identity with a zero right-hand side, so their step is exactly 0.
// On the device the callables of the camera kernel are workgroup-wide passes (every lane runs this policy on the same reduced
// values, so control flow stays uniform and every barrier inside a callable is reached by all lanes).
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STBA_HD __host__ __device__
#else
#define STBA_HD
#endif

namespace stba {
namespace inner {

// Solver::Options defaults (and TrustRegionStrategy::Options::max_radius) of the block's minimiser -- not the caller's options
struct BlockOptions {
    int max_num_iterations = 50;
    double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
    double initial_trust_region_radius = 1e4, max_trust_region_radius = 1e32, min_trust_region_radius = 1e-32;
    double min_relative_decrease = 1e-3, min_lm_diagonal = 1e-6, max_lm_diagonal = 1e32;
    int max_consecutive_invalid = 5;
};

// why a block's minimiser stopped (the numbering of include/stba.h's STBA_TERM_*, plus SKIPPED / INVALID)
enum { STOP_SKIPPED = 0, STOP_GRADIENT = 1, STOP_FUNCTION = 2, STOP_PARAMETER = 3, STOP_MAX_ITER = 4, STOP_MIN_RADIUS = 5,
       STOP_INVALID = 6 };

struct BlockResult {
    int iterations = 0;     // trust-region steps computed (accepted, rejected, invalid, and the one that met a tolerance)
    int stop = STOP_SKIPPED;
    double cost0 = 0.0, cost = 0.0;
};

// (H + diag) y = b by Cholesky on the dofs of mask (the others: y = 0).  false: a pivot that is not positive and finite
template <int N>
STBA_HD inline bool damped_solve(const double* A, const double* b, unsigned mask, double* y) {
    double L[N * N];
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            const bool act = ((mask >> i) & 1u) && ((mask >> j) & 1u);
            L[i * N + j] = act ? A[i * N + j] : (i == j ? 1.0 : 0.0);
        }
    for (int j = 0; j < N; ++j) {
        double d = L[j * N + j];
        for (int k = 0; k < j; ++k) d -= L[j * N + k] * L[j * N + k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double ljj = std::sqrt(d);
        L[j * N + j] = ljj;
        for (int i = j + 1; i < N; ++i) {
            double s = L[i * N + j];
            for (int k = 0; k < j; ++k) s -= L[i * N + k] * L[j * N + k];
            L[i * N + j] = s / ljj;
        }
    }
    double z[N];
    for (int i = 0; i < N; ++i) {
        double s = ((mask >> i) & 1u) ? b[i] : 0.0;
        for (int k = 0; k < i; ++k) s -= L[i * N + k] * z[k];
        z[i] = s / L[i * N + i];
    }
    for (int i = N - 1; i >= 0; --i) {
        double s = z[i];
        for (int k = i + 1; k < N; ++k) s -= L[k * N + i] * y[k];
        y[i] = s / L[i * N + i];
    }
    for (int i = 0; i < N; ++i) if (!((mask >> i) & 1u)) y[i] = 0.0;
    return true;
}

// The minimiser.  x: the block's ambient parameters (A doubles), moved in place to the last accepted point.
// TrustRegionMinimizer order: iteration 0 (evaluate, gradient test), then per iteration the iteration / radius limits, the step
// (invalid: LM StepIsInvalid = a rejection), the candidate, the parameter test, the function test (its step is NOT taken),
// rho > min_relative_decrease, and after a successful step the gradient test at the new point.
template <int N, int A, class Lin, class Cost, class Plus, class Norm2, class Dist2>
STBA_HD inline BlockResult block_lm(const BlockOptions& o, unsigned mask, double* x, Lin lin, Cost cost_at, Plus plus, Norm2 norm2,
                                    Dist2 dist2) {
    BlockResult res;
    double H[N * N], g[N], s[N], xn[A];
    double cost = lin(x, H, g);
    res.cost0 = res.cost = cost;
    auto gmax_of = [&]() {
        double m = 0.0;
        for (int a = 0; a < N; ++a) if ((mask >> a) & 1u) m = std::fmax(m, std::fabs(g[a]));
        return m;
    };
    if (!std::isfinite(cost)) { res.stop = STOP_INVALID; return res; }
    for (int a = 0; a < N; ++a) s[a] = 1.0 / (1.0 + std::sqrt(H[a * N + a]));     // Jacobi scaling at the block's start point
    if (gmax_of() <= o.gradient_tolerance) { res.stop = STOP_GRADIENT; return res; }
    double radius = o.initial_trust_region_radius, decrease = 2.0;
    int invalid_run = 0;
    while (true) {
        if (res.iterations >= o.max_num_iterations) { res.stop = STOP_MAX_ITER; break; }
        if (radius < o.min_trust_region_radius) { res.stop = STOP_MIN_RADIUS; break; }
        ++res.iterations;
        // (s H s + D) y = -s g,  D_a = clamp(s_a^2 H_aa, min_lm_diagonal, max_lm_diagonal) / radius;  delta = s y
        double M[N * N], rhs[N], y[N], d[N];
        for (int i = 0; i < N; ++i) {
            for (int j = 0; j < N; ++j) M[i * N + j] = s[i] * H[i * N + j] * s[j];
            const double dd = std::fmin(std::fmax(s[i] * s[i] * H[i * N + i], o.min_lm_diagonal), o.max_lm_diagonal) / radius;
            M[i * N + i] += dd;
            rhs[i] = -s[i] * g[i];
        }
        bool valid = damped_solve<N>(M, rhs, mask, y);
        double model = 0.0;
        if (valid) {
            // model cost change -(J d)^T (r + J d / 2) = -(g^T d + d^T H d / 2)
            for (int i = 0; i < N; ++i) d[i] = s[i] * y[i];
            double gd = 0.0, dHd = 0.0;
            for (int i = 0; i < N; ++i) {
                gd += g[i] * d[i];
                double hd = 0.0;
                for (int j = 0; j < N; ++j) hd += H[i * N + j] * d[j];
                dHd += d[i] * hd;
            }
            model = -(gd + 0.5 * dHd);
            valid = model > 0.0 && std::isfinite(model);
        }
        if (!valid) {
            if (++invalid_run > o.max_consecutive_invalid) { res.stop = STOP_INVALID; break; }
            radius /= decrease; decrease *= 2.0;
            continue;
        }
        invalid_run = 0;
        plus(x, d, xn);
        double new_cost = cost_at(xn);
        if (!std::isfinite(new_cost)) new_cost = HUGE_VAL;      // (a failed evaluation: an unsuccessful step)
        const double step2 = dist2(x, xn), x2 = norm2(x);
        const double x_norm = std::sqrt(x2);
        if (std::sqrt(step2) <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) { res.stop = STOP_PARAMETER; break; }
        const double cost_change = cost - new_cost;
        if (std::fabs(cost_change) <= o.function_tolerance * cost) { res.stop = STOP_FUNCTION; break; }
        const double rho = cost_change / model;
        if (rho > o.min_relative_decrease) {
            for (int k = 0; k < A; ++k) x[k] = xn[k];
            cost = lin(x, H, g);
            const double t = 2.0 * rho - 1.0;
            radius = std::fmin(o.max_trust_region_radius, radius / std::fmax(1.0 / 3.0, 1.0 - t * t * t));
            decrease = 2.0;
            if (gmax_of() <= o.gradient_tolerance) { res.stop = STOP_GRADIENT; break; }
        } else {
            radius /= decrease; decrease *= 2.0;
        }
    }
    res.cost = cost;
    return res;
}

}  // namespace inner
}  // namespace stba
