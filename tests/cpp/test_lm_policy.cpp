// The Levenberg-Marquardt step policy (slam-tricks_amd/csrc/lm_policy.hpp) that the BA engine, the pose graph and the dense loop
// share: the stop tests, the acceptance test, the radius on acceptance and rejection, and the trace rows.  No device needed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../slam-tricks_amd/csrc/lm_policy.hpp"

using namespace stba;

int main() {
    int bad = 0;
    auto expect = [&](bool cond, const char* what) { if (!cond) { std::printf("FAILED: %s\n", what); ++bad; } };
    stba_lm_options o;
    stba::default_options(&o);
    expect(o.function_tolerance_takes_step == 1 && o.initial_trust_region_radius == 1e4 && o.max_trust_region_radius == 1e16 &&
           o.min_relative_decrease == 1e-3 && o.function_tolerance == 1e-6 && o.parameter_tolerance == 1e-8 && o.max_num_iterations == 50,
           "default options");

    // parameter tolerance: |step| <= tol (|x| + tol) stops, whatever rho; the step is not taken
    StepVerdict v = judge_step(o, 10.0, true, 5.0, 5.0, 1e-8 * (1.0 + 1e-8), 1.0);
    expect(v.stop == STBA_TERM_PARAMETER && !v.accepted && v.cost_change == 5.0 && v.rho == 1.0, "parameter tolerance stop");
    v = judge_step(o, 10.0, true, 5.0, 5.0, 1.1e-8, 1.0);
    expect(v.stop == STBA_TERM_NONE && v.accepted, "a step just above the parameter tolerance goes on");

    // function tolerance: |cost_change| <= tol * cost stops; with takes_step = 1 a step with rho > min_relative_decrease is taken
    const double c = 1.0, dc = std::ldexp(1.0, -21);                    // (4.8e-7: exact in binary, under the tolerance)
    v = judge_step(o, c, true, c - dc, dc, 1.0, 1.0);
    expect(v.stop == STBA_TERM_FUNCTION && v.accepted && v.rho == 1.0, "function tolerance, takes_step = 1, good rho: taken");
    v = judge_step(o, c, true, c - dc, dc * 2048.0, 1.0, 1.0);          // rho = 1/2048 <= min_relative_decrease
    expect(v.stop == STBA_TERM_FUNCTION && !v.accepted, "function tolerance, takes_step = 1, rho below min_relative_decrease: not taken");
    v = judge_step(o, c, true, c + dc, dc, 1.0, 1.0);                    // an increase within the tolerance
    expect(v.stop == STBA_TERM_FUNCTION && !v.accepted && v.rho == -1.0, "function tolerance on an increase: stop, not taken");
    stba_lm_options o0 = o;
    o0.function_tolerance_takes_step = 0;
    v = judge_step(o0, c, true, c - dc, dc, 1.0, 1.0);
    expect(v.stop == STBA_TERM_FUNCTION && !v.accepted, "function tolerance, takes_step = 0, good rho: not taken");
    v = judge_step(o0, c, true, c - dc, dc * 2048.0, 1.0, 1.0);
    expect(v.stop == STBA_TERM_FUNCTION && !v.accepted, "function tolerance, takes_step = 0, poor rho: not taken");
    v = judge_step(o, c, true, c - 2e-6, 2e-6, 1.0, 1.0);
    expect(v.stop == STBA_TERM_NONE && v.accepted, "a change above the function tolerance goes on");

    // acceptance: rho > min_relative_decrease
    v = judge_step(o, 10.0, true, 10.0 - 1e-3, 1.0, 1.0, 1.0);          // rho = 1e-3: not greater
    expect(v.stop == STBA_TERM_NONE && !v.accepted, "rho == min_relative_decrease is rejected");
    v = judge_step(o, 10.0, true, 10.0 - 2e-3, 1.0, 1.0, 1.0);
    expect(v.stop == STBA_TERM_NONE && v.accepted, "rho above min_relative_decrease is accepted");

    // the radius on acceptance: radius / max(1/3, 1 - (2 rho - 1)^3), at most max_trust_region_radius
    TrustRegion tr(o);
    expect(tr.radius == 1e4 && tr.decrease == 2.0, "trust region starts at the initial radius");
    tr.accept(1.0, o);                                                    // 1 - 1 = 0 -> the 1/3 floor: x3
    expect(tr.radius == 1e4 / (1.0 / 3.0), "rho = 1: radius x 3 (the 1/3 floor)");
    tr.radius = 1e4; tr.accept(0.5, o);                                   // t = 0: radius / 1
    expect(tr.radius == 1e4, "rho = 0.5: radius unchanged");
    tr.radius = 1e4; tr.accept(0.25, o);                                  // t = -0.5: radius / 1.125
    expect(tr.radius == 1e4 / 1.125, "rho = 0.25: radius / (1 - (2 rho - 1)^3)");
    tr.radius = 0.9e16; tr.accept(1.0, o);
    expect(tr.radius == 1e16, "the radius is capped at max_trust_region_radius");

    // three rejections in a row (/2, /4, /8), then an acceptance resets the decrease
    tr.radius = 64.0; tr.decrease = 2.0;
    tr.reject(); expect(tr.radius == 32.0 && tr.decrease == 4.0, "first rejection: /2");
    tr.reject(); expect(tr.radius == 8.0 && tr.decrease == 8.0, "second rejection: /4");
    tr.reject(); expect(tr.radius == 1.0 && tr.decrease == 16.0, "third rejection: /8");
    tr.accept(0.5, o); expect(tr.radius == 1.0 && tr.decrease == 2.0, "an acceptance resets the decrease");
    tr.reject(); expect(tr.radius == 0.5, "and the next rejection halves again");

    // the min-radius test
    tr.radius = o.min_trust_region_radius; expect(!tr.below_min(o), "radius == min is not below");
    tr.radius = 0.5 * o.min_trust_region_radius; expect(tr.below_min(o), "radius < min is below");

    // a step that was not computed or evaluated: rejected, no test, zeros
    v = judge_step(o, 10.0, false, 0.0, 0.0, 0.0, 1.0);
    expect(v.stop == STBA_TERM_NONE && !v.accepted && v.cost_change == 0.0 && v.rho == 0.0, "ok == false: rejected, no test");
    // a NaN trial cost judged as ok (the dense loop): no stop, rejected, NaN cost change and rho
    const double nan = std::numeric_limits<double>::quiet_NaN();
    v = judge_step(o, 10.0, true, nan, 1.0, 1.0, 1.0);
    expect(v.stop == STBA_TERM_NONE && !v.accepted && std::isnan(v.cost_change) && std::isnan(v.rho), "NaN new cost: rejected");
    v = judge_step(o, 10.0, true, nan, 1.0, 0.0, 1.0);
    expect(v.stop == STBA_TERM_PARAMETER && !v.accepted, "NaN new cost with a zero step: the parameter test still stops");

    // fixed mode: no test stops, acceptance by rho alone
    v = judge_step(o, 10.0, true, 5.0, 5.0, 0.0, 1.0, false);
    expect(v.stop == STBA_TERM_NONE && v.accepted, "fixed mode: no parameter stop");
    v = judge_step(o, c, true, c - dc, dc, 1.0, 1.0, false);
    expect(v.stop == STBA_TERM_NONE && v.accepted, "fixed mode: no function stop");
    v = judge_step(o, 10.0, true, 11.0, 1.0, 1.0, 1.0, false);
    expect(v.stop == STBA_TERM_NONE && !v.accepted && v.rho == -1.0, "fixed mode: an increase is rejected");

    // trace rows: row 0 and row iter (cost, cost_change, |g|max, |step|, rho, radius, accepted)
    std::vector<double> t(3 * STBA_TRACE_COLS, 7.0);
    trace_start(t.data(), 4.0, 0.5, 1e4);
    const double row0[STBA_TRACE_COLS] = {4.0, 0.0, 0.5, 0.0, 0.0, 1e4, 1.0};
    bool same = true;
    for (int k = 0; k < STBA_TRACE_COLS; ++k) same = same && t[(size_t)k] == row0[k];
    expect(same && t[STBA_TRACE_COLS] == 7.0, "trace row 0, and nothing behind it");
    v = judge_step(o, 4.0, true, 3.0, 2.0, 0.25, 1.0);
    trace_step(t.data(), 1, true, 4.0, 3.0, v, 0.125, 0.25, 3e4);
    const double row1[STBA_TRACE_COLS] = {3.0, 1.0, 0.125, 0.25, 0.5, 3e4, 1.0};
    same = true;
    for (int k = 0; k < STBA_TRACE_COLS; ++k) same = same && t[(size_t)STBA_TRACE_COLS + k] == row1[k];
    expect(same, "trace row of an accepted step");
    v = judge_step(o, 4.0, false, 0.0, 0.0, 0.25, 1.0);
    trace_step(t.data(), 2, false, 4.0, 99.0, v, 0.125, 0.25, 5e3);
    const double row2[STBA_TRACE_COLS] = {4.0, 0.0, 0.125, 0.0, 0.0, 5e3, 0.0};
    same = true;
    for (int k = 0; k < STBA_TRACE_COLS; ++k) same = same && t[(size_t)2 * STBA_TRACE_COLS + k] == row2[k];
    expect(same, "trace row of a step that is not ok: [cost, 0, |g|, 0, 0, radius, 0]");
    trace_start(nullptr, 1.0, 1.0, 1.0);
    trace_step(nullptr, 1, true, 1.0, 1.0, v, 1.0, 1.0, 1.0);            // (no trace: nothing written)

    std::printf(bad ? "lm_policy FAILED %d\n" : "lm_policy ok\n", bad);
    return bad ? 1 : 0;
}
