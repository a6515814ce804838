// lm_policy.hpp -- the Levenberg-Marquardt step policy of every LM loop in the library (BA engine, pose graph, the dense loop):
// Ceres' TrustRegionMinimizer + LevenbergMarquardtStrategy decision for decision, written once.  Host code only: it includes
// nothing but include/stba.h and the standard library, so that a plain C++ compiler can test it without HIP.
// The loops keep what is theirs -- what a step costs the device, when the gradient arrives, the callback and its stops;
// this header judges a step that has been computed and evaluated, updates the trust region and writes the trace.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/stba.h"

namespace stba {

inline double wall_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline void default_options(stba_lm_options* o) {
    o->max_num_iterations = 50;
    o->initial_trust_region_radius = 1e4;
    o->max_trust_region_radius = 1e16;
    o->min_trust_region_radius = 1e-32;
    o->min_relative_decrease = 1e-3;
    o->min_lm_diagonal = 1e-6;
    o->max_lm_diagonal = 1e32;
    o->function_tolerance = 1e-6;
    o->gradient_tolerance = 1e-10;
    o->parameter_tolerance = 1e-8;
    o->jacobi_scaling = 1;
    o->num_threads = 1;
    o->minimizer_progress_to_stdout = 0;
    o->update_state_every_iteration = 0;
    o->phase_timing = 0;
    o->function_tolerance_takes_step = 1;      // (stba.h: why the step is taken by default although Ceres >= 1.12 does not)
}

// LevenbergMarquardtStrategy's radius: grown or shrunk by the outcome of every step
struct TrustRegion {
    double radius, decrease = 2.0;
    explicit TrustRegion(const stba_lm_options& o) : radius(o.initial_trust_region_radius) {}
    void accept(double rho, const stba_lm_options& o) {
        const double t = 2.0 * rho - 1.0;
        radius = std::min(o.max_trust_region_radius, radius / std::max(1.0 / 3.0, 1.0 - t * t * t));
        decrease = 2.0;
    }
    void reject() { radius /= decrease; decrease *= 2.0; }
    bool below_min(const stba_lm_options& o) const { return radius < o.min_trust_region_radius; }
};

// DoglegStrategy's state (TRADITIONAL_DOGLEG): the radius Delta, which lives in the dogleg coordinates z = d .* y,
// the regularisation mu of the Gauss-Newton solve (J^T J + mu diag(d^2)) y_gn = -g, which persists across iterations, and whether
// the next step re-uses the directions of this linearisation
struct DoglegRegion {
    static constexpr double kMinMu = 1e-8, kMaxMu = 1.0, kMuIncrease = 10.0;
    double radius, mu = kMinMu;
    bool reuse = false;
    explicit DoglegRegion(const stba_lm_options& o) : radius(o.initial_trust_region_radius) {}
    // z_norm: |z| of the accepted step
    void accept(double rho, double z_norm, const stba_lm_options& o) {
        if (rho > 0.75) radius = std::max(radius, 3.0 * z_norm);
        else if (rho < 0.25) radius *= 0.5;
        radius = std::min(o.max_trust_region_radius, radius);
        mu = std::max(kMinMu, 2.0 * mu / kMuIncrease);
        reuse = false;
    }
    void reject() { radius *= 0.5; reuse = true; }
    // a step that is not valid: no Gauss-Newton step at any mu, or a model change that is not positive and finite
    void invalid() { mu *= kMuIncrease; reuse = false; }
    // the factorisation failed (a pivot that is not positive, or a Gauss-Newton step that is not finite): true if it runs again
    // at the larger mu, false if no mu below kMaxMu is left (the step is invalid)
    bool escalate() { mu *= kMuIncrease; return mu < kMaxMu; }
    bool can_factor() const { return mu < kMaxMu; }
    bool below_min(const stba_lm_options& o) const { return radius < o.min_trust_region_radius; }
};

struct StepVerdict {
    double cost_change = 0.0, rho = 0.0;
    bool accepted = false;       // (also on a function-tolerance stop that takes the step)
    int stop = STBA_TERM_NONE;   // STBA_TERM_PARAMETER or STBA_TERM_FUNCTION: the solve has converged on this step
};

// ok: the step was computed and its trial point evaluated -- what counts as that is the caller's.  A step that is not ok is
// rejected with cost_change = rho = 0 and no test runs.  tests = false (the BA engine's fixed-iteration mode): no stop.
// inner_useful (the BA engine's inner iterations): the sweep brought the candidate below the current cost -- the step
// is taken whatever rho (Ceres IsStepSuccessful); new_cost, model_change and step_norm are then the sweep's
inline StepVerdict judge_step(const stba_lm_options& o, double cost, bool ok, double new_cost, double model_change, double step_norm,
                              double x_norm, bool tests = true, bool inner_useful = false) {
    StepVerdict v;
    if (!ok) return v;
    v.cost_change = cost - new_cost;
    v.rho = v.cost_change / model_change;
    if (tests) {
        if (step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) {
            v.stop = STBA_TERM_PARAMETER;
            return v;
        }
        if (std::fabs(v.cost_change) <= o.function_tolerance * cost) {
            // (function_tolerance_takes_step, stba.h: 1 = the decreasing step is taken before convergence is reported; 0 = not)
            v.accepted = o.function_tolerance_takes_step && (inner_useful || v.rho > o.min_relative_decrease);
            v.stop = STBA_TERM_FUNCTION;
            return v;
        }
    }
    v.accepted = inner_useful || v.rho > o.min_relative_decrease;
    return v;
}

// trace rows (stba.h, STBA_TRACE_COLS): cost, cost_change, gradient_max_norm, step_norm, relative_decrease, radius, accepted.
// Row 0 is the start point; row iter is the step of iteration iter, at the cost it left (the trial cost if ok)
inline void trace_start(double* trace, double cost, double gmax, double radius) {
    if (!trace) return;
    memset(trace, 0, sizeof(double) * STBA_TRACE_COLS);
    trace[0] = cost; trace[2] = gmax; trace[5] = radius; trace[6] = 1;
}
inline void trace_step(double* trace, int iter, bool ok, double cost, double new_cost, const StepVerdict& v, double gmax,
                       double step_norm, double radius) {
    if (!trace) return;
    double* tr = trace + (size_t)iter * STBA_TRACE_COLS;
    tr[0] = ok ? new_cost : cost; tr[1] = v.cost_change; tr[2] = gmax; tr[3] = ok ? step_norm : 0.0; tr[4] = v.rho; tr[5] = radius;
    tr[6] = v.accepted ? 1 : 0;
}

// minimizer_progress_to_stdout
inline void progress_start(double cost, double gmax, double radius) {
    printf("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius\n"
           "%4d  %.6e    0.00e+00    %.2e   0.00e+00   0.00e+00  %.2e\n", 0, cost, gmax, radius);
}
inline void progress_step(int iter, double cost, const StepVerdict& v, double gmax, double step_norm, double radius, const char* tail = "") {
    printf("%4d  %.6e   % .2e    %.2e   %.2e  % .2e  %.2e%s\n", iter, cost, v.cost_change, gmax, step_norm, v.rho, radius, tail);
}

inline void finish_summary(stba_lm_summary* s, int iterations, double cost, double radius, double gmax, double t_start) {
    s->num_iterations = iterations;
    s->final_cost = cost;
    s->final_radius = radius;
    s->final_gradient_max_norm = gmax;
    s->seconds_total = wall_s() - t_start;
}

}  // namespace stba
