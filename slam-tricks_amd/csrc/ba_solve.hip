// ba_solve.hip -- the solves of the bundle-adjustment engine: the state of one call (BaSolve) and the steps over it, the
// Levenberg-Marquardt loop (ba_run_lm) and the DOGLEG loop (ba_run_dogleg), the inner-iteration driver, and the entry points
// stba_ba_solve, stba_ba_lm_iterations, stba_ba_inner_sweep and stba_ba_triangulate.
// The Levenberg-Marquardt control flow follows Ceres' TrustRegionMinimizer +
// LevenbergMarquardtStrategy (the solver behind ceres::Solve at
// st20-g2o/src/include/test_ceres.h:148 and st17-ceres/src/include/solver.hpp:286) with the
// defaults listed in SURVEY.md 8c; all arithmetic on problem-sized data runs in HIP kernels (what the loops enqueue is ba_linear.hip).
#include <algorithm>
#include <vector>

#include "ba_engine.hpp"
#include "dogleg.hpp"
#include "inner_iterations.hpp"
#include "lm_policy.hpp"

namespace stba {

// ---- inner iterations (Solver::Options::use_inner_iterations; inner_iterations.hip)
static InnerObs inner_obs_args(const stba_ba* b) {
    InnerObs o;
    o.n_cams = b->nc; o.n_pts = b->np;
    o.pt_start = b->pt_start; o.obs_cam = b->obs_cam; o.obs_pt = b->obs_pt; o.feat = b->feat;
    o.cam_perm = b->cam_perm; o.chunk_begin = b->chunk_begin; o.chunk_end = b->chunk_end; o.cam_chunk_start = b->cam_chunk_start;
    return o;
}
// one sweep of the ordering over parameter buffer `which`, in place: the groups in ascending id, in each the camera blocks, then the
// landmarks (a group is an independent set: the two launches see nothing of each other's blocks).  gate: null, or the device's
// verdict on the trial point (0: every workgroup returns at once)
static int ba_inner_sweep_enqueue(stba_ba* b, int which, const int* gate) {
    const InnerObs o = inner_obs_args(b);
    const int n_cam_entries = (int)b->inner.plan.cam.size();
    for (const auto& g : b->inner.plan.groups) {
        STBA_TRY(launch_inner_cameras(o, g.cam_hi - g.cam_lo, b->inner.cam + g.cam_lo, b->inner.mask + g.cam_lo, b->cams[which],
                                      b->pts[which], b->inner.it + g.cam_lo, gate, b->st));
        STBA_TRY(launch_inner_points(o, g.pt_hi - g.pt_lo, b->inner.pt + g.pt_lo, b->cams[which], b->pts[which],
                                     b->inner.it + n_cam_entries + g.pt_lo, gate, b->st));
    }
    return STBA_OK;
}
// behind the trial point x+ in buffer cur ^ 1 (enqueued before the host reads the trial block): the gate, the sweep x+ -> x*, the
// cost at x* by the trial pass's residual kernel -> inner.sc[0] (cost2), and the ambient |x - x*|^2 -> inner.sc[1]
static int ba_inner_after_trial(stba_ba* b) {
    const int cur = b->cur, nxt = cur ^ 1;
    STBA_TRY(launch_inner_gate(b->trial, b->flag, TS_COST2, TS_MODEL, TS_CAM + 2, b->inner.gate, b->st));
    STBA_TRY(ba_inner_sweep_enqueue(b, nxt, b->inner.gate));
    STBA_TRY(ba_cost_only(b, nxt, b->inner.sc));
    STBA_TRY(launch_inner_step2(b->nc, b->np, b->cams[cur], b->pts[cur], b->cams[nxt], b->pts[nxt], b->inner.part, b->st));
    return launch_sum_partials(b->inner.part, inner_step_grid(b->nc, b->np), 1, 1, b->inner.sc + 1, b->st);
}
void inner_summary_reset(stba_ba* b) {
    b->inner.sum = stba_inner_summary{};
    b->inner.sum.struct_size = sizeof(stba_inner_summary);
    b->inner.sum.disabled_at_iteration = -1;
    b->inner.sum.num_groups = (int)b->inner.plan.groups.size();
    for (int g = 0; g < b->inner.sum.num_groups && g < STBA_INNER_MAX_GROUPS_REPORTED; ++g) {
        const auto& r = b->inner.plan.groups[(size_t)g];
        b->inner.sum.group_size[g] = (r.cam_hi - r.cam_lo) + (r.pt_hi - r.pt_lo);
    }
}

// ---- the steps of a BA solve (ba_run_lm, ba_run_dogleg).  BaSolve is the state of ONE call; what outlives a call (the parameter
// buffers and which is current, the Jacobi scale, the stage cool-down, the stamped blocks' sequence numbers, the events, the PCG,
// dogleg and inner summaries) stays in stba_ba.  The two strategies share steps, not a loop: each keeps its trust region and its
// own order of enqueues.  No step captures anything.
struct BaPending {             // (cost, |g|max) of the linearisation behind iteration `iter`: they arrive with the next trial block
    bool on = false, accepted = false;
    int iter = 0, lin_ev = EV_SPEC_A;     // lin_ev: the event pair around that linearisation
};
struct BaSolve {
    stba_lm_options opt;
    // derived once
    bool fixed = false, timing = false;
    bool deferred_ok = false;   // deferred read of (cost, |g|max) of a freshly linearised point: only when nobody watches the iterations
    int max_iter = 0;
    Damping dm;
    stba_lm_summary s;
    double t_start = 0.0;
    // the loop
    double cost = 0.0, gmax = 0.0;
    int iter = 0, chol_timeouts = 0;
    bool need_build = true;      // reduced system must be (re)built before the next solve
    BaPending pending;
    // phase timing: is the start point's linearisation pair still to be read, the speculation's pair of this iteration, and
    // the end event of the last build (the start of the solve that follows it)
    bool lin_timing_pending = true;
    int spec_ev = EV_SPEC_B, build_end_ev = EV_BUILD_END;
    double* trace = nullptr;
    stba_iteration_callback cb = nullptr;
    void* cb_user = nullptr;
};
struct TrialScalars { double new_cost = 0.0, step_norm = 0.0, x_norm = 0.0, model_change = 0.0; };

static void stop(BaSolve& sv, int type, int reason) { sv.s.termination_type = type; sv.s.termination_reason = reason; }

// (see stba_lm_options::phase_timing: every event costs ~5 us of idle GPU -- with timing off none is enqueued)
static int ba_stamp(stba_ba* b, bool on, int ev) {
    if (on) STBA_HIP(hipEventRecord(b->ev[ev], b->st));
    return STBA_OK;
}
static void ba_add_ms(stba_ba* b, int ev_begin, int ev_end, double* total) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->ev[ev_begin], b->ev[ev_end]) == hipSuccess) *total += ms;
}

// options, summary, the per-solve resets of the engine, the damping's constants.  timed: the strategy has phase events at all
static void ba_solve_begin(stba_ba* b, BaSolve& sv, const stba_lm_options* opt_in, int fixed_iterations, bool timed, double* trace,
                           stba_iteration_callback cb, void* cb_user) {
    if (opt_in) sv.opt = *opt_in; else default_options(&sv.opt);
    memset(&sv.s, 0, sizeof sv.s);
    stop(sv, STBA_NO_CONVERGENCE, STBA_TERM_MAX_ITER);
    sv.t_start = wall_s();
    sv.fixed = fixed_iterations > 0;
    sv.max_iter = sv.fixed ? fixed_iterations : sv.opt.max_num_iterations;
    sv.timing = timed && sv.opt.phase_timing != 0;
    sv.deferred_ok = (cb == nullptr) && !sv.opt.minimizer_progress_to_stdout;
    sv.trace = trace; sv.cb = cb; sv.cb_user = cb_user;
    b->ar.timing_on = sv.timing;
    b->scale_init = false;
    b->ar.ms = 0.0; b->ar.bytes = 0.0; b->ar.calls = 0; b->ar.timing_pending = false;
    memset(&b->pcg.sum, 0, sizeof b->pcg.sum);
    b->pcg.per_iter.clear();
    sv.dm.dmin = sv.opt.min_lm_diagonal; sv.dm.dmax = sv.opt.max_lm_diagonal; sv.dm.use_scaling = sv.opt.jacobi_scaling;
}

// linearisation at parameter buffer `which`: residuals + Jacobians, the landmark blocks, and the cost -> *cost_slot with the
// scalar slots.  jac_done: a with_jac trial pass has made the residuals and Jacobians there already (the speculation).
// timed: the pair ev_pair, ev_pair + 1 is recorded around everything but the scalar fill
static int ba_linearize_point(stba_ba* b, int which, double* cost_slot, bool timed = false, int ev_pair = EV_LIN, bool jac_done = false) {
    STBA_TRY(ba_stamp(b, timed, ev_pair));
    if (!jac_done) STBA_TRY(ba_linearize_lm(b, which));
    STBA_TRY(ba_normal_blocks(b));
    STBA_TRY(ba_stamp(b, timed, ev_pair + 1));
    return ba_fill_scalar_slots(b, cost_slot);
}

// the reduced system at `radius`, inside the event pair ev_pair when the solve is timed
static int ba_build_at(stba_ba* b, BaSolve& sv, double radius, int ev_pair = EV_BUILD) {
    sv.dm.radius = radius;
    STBA_TRY(ba_stamp(b, sv.timing, ev_pair));
    STBA_TRY(ba_build(b, sv.dm));
    STBA_TRY(ba_stamp(b, sv.timing, ev_pair + 1));
    sv.build_end_ev = ev_pair + 1;
    sv.need_build = false;
    return STBA_OK;
}

// the start point, behind its first build: cost and |g|max, row 0, the header.  *go = false: the solve ends here
static int ba_first_point(stba_ba* b, BaSolve& sv, double radius, bool* go) {
    *go = false;
    STBA_TRY(ba_read_linear_scalars(b, &sv.cost, &sv.gmax));
    sv.s.initial_cost = sv.cost;
    trace_start(sv.trace, sv.cost, sv.gmax, radius);
    if (sv.opt.minimizer_progress_to_stdout) progress_start(sv.cost, sv.gmax, radius);     // (the BA loops alone print a header)
    // Ceres: a residual block that returns a non-finite value fails its evaluation, and a failed evaluation of the START
    // point ends the solve as FAILURE before any step ("Initial residual and Jacobian evaluation failed"); at a trial
    // point it is an unsuccessful step -- the rho test rejects a non-finite cost.  (oracle.c: orc_ba_solve)
    if (!std::isfinite(sv.cost)) stop(sv, STBA_FAILURE, STBA_TERM_SOLVER_FAIL);
    else if (!sv.fixed && sv.gmax <= sv.opt.gradient_tolerance) stop(sv, STBA_CONVERGENCE, STBA_TERM_GRADIENT);
    else *go = sv.max_iter > 0;
    return STBA_OK;
}

// the pending read: (cost, |g|max) of the linearisation behind iteration pending.iter have arrived.  true: that iteration had
// converged on its gradient -- the test comes first, whatever the loop has done since
static bool ba_take_pending(BaSolve& sv, double cost, double gmax) {
    sv.gmax = gmax;
    if (sv.pending.accepted) sv.cost = cost;
    if (sv.trace) sv.trace[(size_t)sv.pending.iter * STBA_TRACE_COLS + 2] = gmax;
    sv.pending.on = false;
    return sv.pending.accepted && !sv.fixed && gmax <= sv.opt.gradient_tolerance;
}
// behind the loop (the stream is idle): the loop ended (iteration / radius limit) before the last linearisation's scalars were read
static int ba_take_pending_at_end(stba_ba* b, BaSolve& sv) {
    if (!sv.pending.on) return STBA_OK;
    double c2, g2;
    STBA_TRY(ba_read_linear_scalars(b, &c2, &g2));
    if (ba_take_pending(sv, c2, g2) && (sv.s.termination_reason == STBA_TERM_MAX_ITER || sv.s.termination_reason == STBA_TERM_MIN_RADIUS))
        stop(sv, STBA_CONVERGENCE, STBA_TERM_GRADIENT);
    return STBA_OK;
}

static TrialScalars trial_scalars(const double* ts) {
    return {0.5 * ts[TS_COST2], std::sqrt(ts[TS_STEP2] + ts[TS_CAM + 0]), std::sqrt(ts[TS_X2] + ts[TS_CAM + 1]), ts[TS_MODEL] + ts[TS_CAM + 2]};
}

// The persistent factorisation gave up waiting for a dependency: some of its workgroups were not resident (the
// device is shared with another process).  S is half factored; it is rebuilt from the blocks -- the engine owns
// them -- and this iteration runs again, the factorisation through the stage kernels, which need nothing
// resident (chol_note_timeout: so do the next ones on this device).
// relinearize: a speculative linearisation overwrote the current point's residuals, Jacobians and blocks
static int ba_on_chol_timeout(stba_ba* b, BaSolve& sv, int flag_h, bool relinearize) {
    // One rank: the DEVICE is marked (it is shared with somebody: the next 64 factorisations of anybody on it take the stage
    // kernels).  Several ranks: every rank -- the one that gave up and its peers -- starts the same cool-down of ITS ENGINE, so
    // that all of them factor the identical system with the identical schedule for the same 64 factorisations (the two
    // schedules differ in the last bits, and every rank must hold the same camera blocks); a counter in the shared
    // per-device state (round 5) was decremented by whoever else factored on that device (advisor, round 5).
    if (b->ar.fn) { b->ar.stage_cooldown = 64; if (flag_h == CHOL_FLAG_TIMEOUT) chol_count_timeout(); }
    else chol_note_timeout();
    // (a device that keeps timing out is shared for good: the cool-down is renewed every time, so a long run goes on through
    // the stage kernels instead of failing; only time-outs that come back-to-back without a good iteration in between --
    // the stage kernels cannot time out -- end the solve)
    if (++sv.chol_timeouts > 8) return fail(STBA_ERR_HIP, "dense Cholesky: the persistent program timed out repeatedly");
    if (relinearize) STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2));
    sv.need_build = true;
    --sv.iter;
    return STBA_OK;
}

static int ba_notify(const BaSolve& sv, const StepVerdict& v, double step_norm, double radius) {
    return sv.cb ? sv.cb(sv.cb_user, sv.iter, sv.cost, v.cost_change, sv.gmax, step_norm, radius, v.accepted ? 1 : 0) : 0;
}
// a judged step: the accepted point becomes the current one; the iteration's trace row (its |g|max and radius follow, ba_end_iteration).
// true: the step ended the solve on the parameter or the function tolerance (the callback hears of it; its answer no longer matters)
static bool ba_apply_verdict(stba_ba* b, BaSolve& sv, const StepVerdict& v, bool step_ok, const TrialScalars& t, double radius) {
    if (v.accepted) {
        b->cur ^= 1;
        sv.cost = t.new_cost;
        ++sv.s.num_successful_steps;
    }
    trace_step(sv.trace, sv.iter, step_ok, sv.cost, t.new_cost, v, sv.gmax, t.step_norm, radius);
    if (!v.stop) return false;
    stop(sv, STBA_CONVERGENCE, v.stop);
    (void)ba_notify(sv, v, t.step_norm, radius);
    return true;
}
// the iteration's row is complete: |g|max and the new radius into it, the progress line, the callback.  true: the solve ends here
static bool ba_end_iteration(BaSolve& sv, const StepVerdict& v, double step_norm, double radius) {
    if (sv.trace) { sv.trace[(size_t)sv.iter * STBA_TRACE_COLS + 2] = sv.gmax; sv.trace[(size_t)sv.iter * STBA_TRACE_COLS + 5] = radius; }
    if (sv.opt.minimizer_progress_to_stdout) progress_step(sv.iter, sv.cost, v, sv.gmax, step_norm, radius);
    if (ba_notify(sv, v, step_norm, radius) != 0) { stop(sv, STBA_CONVERGENCE, STBA_TERM_USER); return true; }
    if (!sv.pending.on && v.accepted && !sv.fixed && sv.gmax <= sv.opt.gradient_tolerance) {
        stop(sv, STBA_CONVERGENCE, STBA_TERM_GRADIENT);
        return true;
    }
    return false;
}

static int ba_solve_end(stba_ba* b, BaSolve& sv, double radius, stba_lm_summary* sum) {
    STBA_HIP(hipStreamSynchronize(b->st));
    STBA_TRY(ba_take_pending_at_end(b, sv));
    ba_collect_allreduce_time(b);
    sv.s.ms_allreduce = b->ar.ms; sv.s.allreduce_bytes = b->ar.bytes; sv.s.allreduce_calls = b->ar.calls;
    finish_summary(&sv.s, sv.iter, sv.cost, radius, sv.gmax, sv.t_start);
    b->pcg.sum.linear_solve_ms = b->iterative ? sv.s.ms_solve : 0.0;
    ba_invalidate(b);
    if (sum) *sum = sv.s;
    return STBA_OK;
}

// ---- ba_run_lm's own steps
// factor + solve into dxc: the PCG (*pcg_fail: the step is not ok), or the dense Cholesky -- the persistent program, or the stage kernels
static int ba_factor_solve(stba_ba* b, int* pcg_fail) {
    if (b->iterative) return ba_pcg_solve(b, pcg_fail);
    // (several ranks behind a time-out of ANY rank: this engine's own cool-down -- every rank counts the same factorisations
    // through the stage kernels, whatever else shares its device or its process)
    if (b->ar.stage_cooldown > 0) { --b->ar.stage_cooldown; return chol_factor_solve_stages(b->S(), b->lda, b->n, b->dxc, b->flag, b->st); }
    return chol_factor_solve_dev(b->S(), b->lda, b->n, b->dxc, b->flag, b->st);
}

// the sweep ran behind a valid step (its gate saw the same valid step): the candidate becomes x* (Ceres DoInnerIterationsIfNeeded),
// isc = {cost2 at x*, |x - x*|^2}.  Returns whether the sweep brought the candidate below the current cost
static bool ba_inner_verdict(stba_ba* b, const BaSolve& sv, const double* isc, TrialScalars& t, bool* inner_active) {
    const double inner_cost = 0.5 * isc[0];
    ++b->inner.sum.sweeps;
    t.model_change += t.new_cost - inner_cost;
    const double progress = 1.0 - inner_cost / t.new_cost;
    t.new_cost = inner_cost;
    t.step_norm = std::sqrt(isc[1]);
    if (!(progress > b->inner.tol)) { *inner_active = false; b->inner.sum.disabled_at_iteration = sv.iter; }
    return inner_cost < sv.cost;
}

// Which event pairs the linearisation and the build behind a judged step belong to.  Watched, the loop reads both at once: its
// own pairs.  Deferred, the host reads them one solve later, with the next trial block: the build has a pair of its own, and the
// linearisation's is the pair the speculation used LAST -- recorded by the speculation itself if the step it ran ahead of was
// accepted, by the re-linearisation otherwise; the next iteration's speculation records into the other one, so the pair is
// still intact when the host reads it.
struct BaStepEvents { int lin, build; };
static BaStepEvents ba_step_events(const BaSolve& sv) {
    return sv.deferred_ok ? BaStepEvents{sv.spec_ev, EV_DBUILD} : BaStepEvents{EV_LIN, EV_BUILD};
}

// everything behind a judged step that has not ended the solve: the linearisation at the (new) current point -- unless the stream
// has done so already --, the reduced system at the new radius, and the pending or immediate read of its cost and |g|max
static int ba_advance(stba_ba* b, BaSolve& sv, double radius, bool accepted, bool speculated) {
    sv.need_build = true;
    if ((accepted || sv.fixed) && !(sv.fixed && sv.iter >= sv.max_iter)) {
        const BaStepEvents e = ba_step_events(sv);
        if (!(speculated && accepted)) STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2, sv.timing, e.lin));
        // gradient of the new point is needed for the convergence test: it arrives with the
        // next reduced-system build (one collective per iteration); build it now.
        STBA_TRY(ba_build_at(b, sv, radius, e.build));
        sv.lin_timing_pending = false;
        if (sv.deferred_ok) {
            // (cost, |g|max) of the new point arrive with the next iteration's trial block
            sv.pending.on = true; sv.pending.accepted = accepted; sv.pending.iter = sv.iter; sv.pending.lin_ev = e.lin;
        } else {
            double c2, g2;
            STBA_TRY(ba_read_linear_scalars(b, &c2, &g2));
            if (sv.timing) { ba_add_ms(b, e.lin, e.lin + 1, &sv.s.ms_linearize); ba_add_ms(b, e.build, e.build + 1, &sv.s.ms_schur); }
            sv.gmax = g2;
            if (accepted) sv.cost = c2;   // same value as new_cost up to summation order
        }
    } else if (speculated && !accepted) {
        // the speculative linearisation overwrote the residuals, Jacobians and blocks of the current point
        STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2));
    }
    return STBA_OK;
}

static int ba_run_lm(stba_ba* b, const stba_lm_options* opt_in, int fixed_iterations, stba_lm_summary* sum,
                     double* trace, stba_iteration_callback cb, void* cb_user) {
    if (b->ar.world > SC_MAX_WORLD) return fail(STBA_ERR_INVALID_ARGUMENT, "world size too large");
    BaSolve sv;
    ba_solve_begin(b, sv, opt_in, fixed_iterations, true, trace, cb, cb_user);
    const stba_lm_options& opt = sv.opt;
    stba_lm_summary& s = sv.s;
    TrustRegion region(opt);
    // inner iterations: on while the engine has them and no sweep has switched them off (rule 6)
    bool inner_active = b->inner.on;
    if (b->inner.on) {
        inner_summary_reset(b);
        if (sv.timing) for (auto& e : b->inner.ev) if (!e) STBA_TRY(e.create());
    }
    static const bool SPECULATE = knob_int("STBA_LM_SPECULATE", 1) != 0;

    // ---- iteration 0: linearise at the start point
    STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2, sv.timing, EV_LIN));
    bool first = true;
    while (true) {
        if (!first) {
            if (sv.iter >= sv.max_iter) {
                stop(sv, sv.fixed ? STBA_CONVERGENCE : STBA_NO_CONVERGENCE, sv.fixed ? STBA_TERM_FIXED : STBA_TERM_MAX_ITER);
                break;
            }
            if (!sv.fixed && region.below_min(opt)) { stop(sv, STBA_CONVERGENCE, STBA_TERM_MIN_RADIUS); break; }
        }
        // ---- reduced system for the current radius
        // (an event record is a packet of its own on the queue, ~5 us of idle GPU between two kernels: none is recorded that
        // is not needed -- when the system was built behind the previous iteration, that build's end event is the start of
        // this solve)
        const bool built_here = sv.need_build;
        if (sv.need_build) STBA_TRY(ba_build_at(b, sv, region.radius));
        const int solve_start_ev = sv.build_end_ev;
        if (first) {
            bool go = false;
            first = false;
            STBA_TRY(ba_first_point(b, sv, region.radius, &go));
            if (!go) break;
        }
        ++sv.iter;
        // ---- factor + solve, back-substitute, trial point
        int flag_h = 0, pcg_fail = 0;
        STBA_TRY(ba_factor_solve(b, &pcg_fail));
        STBA_TRY(ba_stamp(b, sv.timing, EV_SOLVE_END));
        STBA_TRY(ba_backsub_trial(b));
        STBA_TRY(ba_stamp(b, sv.timing, EV_BACKSUB_END));
        // Nobody watches the iterations and there is one rank: the host learns the trial point's scalars through a stamped
        // block in mapped memory, and meanwhile the stream already linearises AT THE TRIAL POINT -- a step is accepted far
        // more often than not, and the host's round trip (wake-up, decision, enqueue: ~35 us) would otherwise be a
        // bubble on the GPU in every iteration.  A rejected step costs one linearisation at the old point (ba_advance).
        // (With several ranks too: every rank takes the same decision from the same all-reduced block, and the collectives of
        // the speculative build are enqueued on the stream like everything else.)
        // (host-linearised factors: the callback is synchronous host work; iterative Schur: the PCG hands its state to the host
        // anyway, and this path does not speculate -- DESIGN.md 7b)
        // (inner iterations: the sweep moves the trial point before anything is linearised there -- no speculation)
        const bool fast = sv.deferred_ok && SPECULATE && !b->hl.fn && !b->iterative && !inner_active;
        if (fast && !b->ts_host.host) STBA_TRY(b->ts_host.alloc((size_t)stamped_doubles(TS_BLOCK)));
        // (the speculative linearisation IS the evaluation of the trial point: one pass over the observations, not two)
        const bool speculate = fast && !(sv.fixed && sv.iter >= sv.max_iter);
        const double seq = fast ? (b->ts_seq += 1.0) : 0.0;
        STBA_TRY(ba_trial(b, fast ? b->ts_host.dev : nullptr, true, speculate, seq));
        STBA_TRY(ba_stamp(b, sv.timing, EV_TRIAL_END));
        double isc[2] = {0.0, 0.0};
        if (inner_active) {
            if (sv.timing) STBA_HIP(hipEventRecord(b->inner.ev[0], b->st));
            STBA_TRY(ba_inner_after_trial(b));
            if (sv.timing) STBA_HIP(hipEventRecord(b->inner.ev[1], b->st));
        }
        const double* ts = b->ts_vals;
        if (fast) {
            if (speculate) {
                // (its own pair of events, alternating: the previous linearisation's pair is read behind the wait below)
                sv.spec_ev = (sv.spec_ev == EV_SPEC_A) ? EV_SPEC_B : EV_SPEC_A;
                STBA_TRY(ba_linearize_point(b, b->cur ^ 1, b->trial + TS_SPEC_COST2, sv.timing, sv.spec_ev, true));
            }
            // (a polled stamped block, no event: a record between two kernels costs the GPU ~5 us, and the stream goes straight on)
            STBA_TRY(stamped_wait(b->ts_host.host, TS_BLOCK, [seq](double st) { return st == seq; }, b->ts_vals, hip_stream_state(b->st),
                                  "trial point", 120.0));
            flag_h = (int)ts[TS_SPEC_COST2];           // (the host's block carries the flag in that slot)
        } else {
            STBA_TRY(download(b->ts_vals, b->trial, TS_BLOCK, b->st));
            STBA_TRY(download(&flag_h, b->flag, 1, b->st));
            if (inner_active) STBA_TRY(download(isc, b->inner.sc, 2, b->st));
            STBA_HIP(hipStreamSynchronize(b->st));
            if (inner_active && sv.timing) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, b->inner.ev[0], b->inner.ev[1]) == hipSuccess) b->inner.sum.sweep_ms += ms;
            }
        }
        if (pcg_fail) flag_h = 1;            // (the PCG failed: the step is not ok)
        if (sv.pending.on) {
            // (cost2 and |g|max of the build behind the previous iteration: trial_finish_kernel read them on the way)
            if (sv.timing) {
                ba_add_ms(b, sv.pending.lin_ev, sv.pending.lin_ev + 1, &s.ms_linearize);
                ba_add_ms(b, EV_DBUILD, EV_DBUILD_END, &s.ms_schur);
            }
            if (ba_take_pending(sv, 0.5 * ts[TS_LIN_COST2], ts[TS_LIN_GMAX])) {
                // converged at the previous iteration: the trial step just computed is discarded
                --sv.iter;
                stop(sv, STBA_CONVERGENCE, STBA_TERM_GRADIENT);
                break;
            }
        }
        if (b->iterative) ba_pcg_account(b, sv.iter);
        // (several ranks: the decision is COLLECTIVE -- ts[TS_TIMEOUT] is the all-reduced count of ranks whose factorisation timed
        // out, the same number on every rank.  A rank-local decision would leave one rank re-running the iteration, with its
        // all-reduces of a system linearised at the old point, while the others move on: mismatched collectives.)
        if (flag_h == CHOL_FLAG_TIMEOUT || ts[TS_TIMEOUT] > 0.0) {
            STBA_TRY(ba_on_chol_timeout(b, sv, flag_h, speculate));
            continue;
        }
        if (sv.timing) {
            if (sv.lin_timing_pending) ba_add_ms(b, EV_LIN, EV_LIN_END, &s.ms_linearize);
            if (built_here) ba_add_ms(b, EV_BUILD, EV_BUILD_END, &s.ms_schur);
            ba_add_ms(b, solve_start_ev, EV_SOLVE_END, &s.ms_solve);
            ba_add_ms(b, EV_SOLVE_END, EV_BACKSUB_END, &s.ms_backsub);
            // (a polled trial block can reach the host before the event recorded behind its kernel has fired: wait for that one)
            if (fast) (void)hipEventSynchronize(b->ev[EV_TRIAL_END]);
            ba_add_ms(b, EV_BACKSUB_END, EV_TRIAL_END, &s.ms_cost);
        }
        sv.lin_timing_pending = false;
        sv.chol_timeouts = 0;

        TrialScalars t = trial_scalars(ts);
        // (a non-finite trial cost makes the step not ok: row [cost, 0, ., 0, 0], no stop test)
        const bool step_ok = flag_h == 0 && t.model_change > 0.0 && std::isfinite(t.model_change) && std::isfinite(t.new_cost);
        const bool inner_useful = inner_active && step_ok && ba_inner_verdict(b, sv, isc, t, &inner_active);
        const StepVerdict v = judge_step(opt, sv.cost, step_ok, t.new_cost, t.model_change, t.step_norm, t.x_norm, !sv.fixed, inner_useful);
        if (ba_apply_verdict(b, sv, v, step_ok, t, region.radius)) break;
        if (v.accepted) region.accept(v.rho, opt);
        else {
            ++s.num_unsuccessful_steps;
            region.reject();
        }
        STBA_TRY(ba_advance(b, sv, region.radius, v.accepted, speculate));
        if (ba_end_iteration(sv, v, t.step_norm, region.radius)) break;
    }
    return ba_solve_end(b, sv, region.radius, sum);
}

// ---- DOGLEG (Ceres' TrustRegionMinimizer + DoglegStrategy, TRADITIONAL_DOGLEG).  One rank, the dense Schur path.
// Per linearisation: the reduced system at radius 1/mu (ba_build), the persistent Cholesky, the Gauss-Newton back-substitution and
// the terms kernel.  Per trial step: the step kernel at Delta and the trial evaluation, whose stamped block is the host's one wait;
// a rejected step is nothing else.  No speculative linearisation: a rejection re-uses the linearisation, which a speculation at the
// trial point would have overwritten.  The cost and |g|max of a new linearisation arrive with its first trial block (as in
// ba_run_lm), unless somebody watches the iterations.
static int ba_dogleg_alloc(stba_ba* b) {
    if (b->dl.sc) return STBA_OK;
    STBA_TRY(b->dl.uc.alloc((size_t)std::max(b->n, 1)));
    STBA_TRY(b->dl.up.alloc((size_t)std::max(b->np, 1) * 3));
    STBA_TRY(b->dl.part.alloc(dogleg_partial_doubles(b->nc, b->np)));
    STBA_TRY(b->dl.sc.alloc(8));
    return b->dl.host.alloc((size_t)stamped_doubles(DL_BLOCK));
}

// the Gauss-Newton side of a linearisation: factor, back-substitute, the six scalars (the reduced system is built)
static int ba_dogleg_gauss_newton(stba_ba* b, const Damping& dm) {
    STBA_TRY(chol_factor_solve_dev(b->S(), b->lda, b->n, b->dxc, b->flag, b->st));
    STBA_TRY(launch_backsub(b->np, b->pt_start, b->obs_cam, b->J8, b->omask, b->Hinv6, b->gp, b->dxc, b->dxp, b->st, nullptr,
                            ba_general_jc(b)));
    DoglegArgs a;
    a.n_cams = b->nc; a.n_pts = b->np;
    a.pt_start = b->pt_start; a.obs_cam = b->obs_cam; a.obs_pt = b->obs_pt;
    a.J8 = b->J8; a.omask = b->omask; a.Jc12 = ba_general_jc(b);
    a.cam_fixed = b->cam_fixed; a.pt_fixed = b->pt_fixed;
    a.hc = b->ex_diag(); a.gc = b->ex_gc(); a.scale_c = b->scale_c;
    a.Hpp6 = b->Hpp6; a.gp = b->gp; a.scale_p = b->scale_p;
    a.dmin = dm.dmin; a.dmax = dm.dmax;
    a.dxc = b->dxc; a.dxp = b->dxp; a.uc = b->dl.uc; a.up = b->dl.up;
    a.partial = b->dl.part; a.scalars = b->dl.sc;
    a.lp = b->landmark_prior_rows();
    return launch_dogleg_terms(a, b->st);
}

static int ba_dogleg_step(stba_ba* b, double radius, double seq) {
    DoglegStepArgs a;
    a.n_cams = b->nc; a.n_pts = b->np;
    a.scalars = b->dl.sc; a.uc = b->dl.uc; a.up = b->dl.up; a.dxc = b->dxc; a.dxp = b->dxp;
    a.cams = b->cams[b->cur]; a.pts = b->pts[b->cur]; a.cam_fixed = b->cam_fixed; a.pt_fixed = b->pt_fixed;
    a.cams_new = b->cams[b->cur ^ 1]; a.pts_new = b->pts[b->cur ^ 1];
    a.partial_c = b->upd_partial_c; a.partial_p = b->upd_partial_p;
    a.host_out = b->dl.host.dev; a.seq = seq;
    return launch_dogleg_step(a, radius, b->st);
}

constexpr int kMaxConsecutiveInvalidSteps = 5;      // Ceres' Solver::Options::max_num_consecutive_invalid_steps

static int ba_run_dogleg(stba_ba* b, const stba_lm_options* opt_in, stba_lm_summary* sum, double* trace, stba_iteration_callback cb,
                         void* cb_user) {
    STBA_TRY(ba_dogleg_alloc(b));
    if (!b->ts_host.host) STBA_TRY(b->ts_host.alloc((size_t)stamped_doubles(TS_BLOCK)));
    BaSolve sv;
    ba_solve_begin(b, sv, opt_in, 0, false, trace, cb, cb_user);
    const stba_lm_options& opt = sv.opt;
    stba_lm_summary& s = sv.s;
    stba_dogleg_summary ds{};
    ds.struct_size = sizeof ds;
    DoglegRegion region(opt);

    STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2));
    bool need_gn = true, first = true;
    int invalid_in_a_row = 0;
    double hd[DL_BLOCK] = {0.0};

    while (true) {
        if (!first) {
            if (sv.iter >= sv.max_iter) break;
            if (region.below_min(opt)) { stop(sv, STBA_CONVERGENCE, STBA_TERM_MIN_RADIUS); break; }
        }
        if (sv.need_build) STBA_TRY(ba_build_at(b, sv, 1.0 / region.mu));
        if (first) {
            bool go = false;
            first = false;
            STBA_TRY(ba_first_point(b, sv, region.radius, &go));
            if (!go) break;
        }
        ++sv.iter;
        // ---- the Gauss-Newton side, once per linearisation (and per mu escalation); mu >= 1: no solve, the step is invalid
        bool have_gn = true, reused = !need_gn;
        if (need_gn) {
            if (region.can_factor()) {
                STBA_TRY(ba_dogleg_gauss_newton(b, sv.dm));
                ++ds.factorizations; ++ds.gauss_newton_solves;
                need_gn = false;
            } else have_gn = false;
        }
        const double* ts = b->ts_vals;
        if (have_gn) {
            // ---- the trial step: the step kernel at Delta and the trial evaluation, read through the trial block (the one wait)
            const double dseq = (b->dl.seq += 1.0), seq = (b->ts_seq += 1.0);
            STBA_TRY(ba_dogleg_step(b, region.radius, dseq));
            STBA_TRY(ba_trial(b, b->ts_host.dev, true, false, seq));
            STBA_TRY(stamped_wait(b->ts_host.host, TS_BLOCK, [seq](double x) { return x == seq; }, b->ts_vals, hip_stream_state(b->st),
                                  "trial point", 120.0));
            // (the step kernel wrote its block before the trial evaluation began: it is there)
            STBA_TRY(stamped_wait(b->dl.host.host, DL_BLOCK, [dseq](double x) { return x == dseq; }, hd, hip_stream_state(b->st),
                                  "dogleg step", 120.0));
            const int flag_h = (int)ts[TS_SPEC_COST2];
            if (flag_h == CHOL_FLAG_TIMEOUT) {
                // the persistent factorisation gave up (the device is shared): S is rebuilt and factored again through the stage
                // kernels, as in ba_run_lm
                STBA_TRY(ba_on_chol_timeout(b, sv, flag_h, false));
                --ds.factorizations; --ds.gauss_newton_solves;
                need_gn = true;
                continue;
            }
            sv.chol_timeouts = 0;
            // cost and |g|max of the linearisation behind the previous iteration (trial_finish_kernel read them on the way)
            if (sv.pending.on && ba_take_pending(sv, 0.5 * ts[TS_LIN_COST2], ts[TS_LIN_GMAX])) {
                --sv.iter;           // converged at the previous iteration: this trial step is discarded
                stop(sv, STBA_CONVERGENCE, STBA_TERM_GRADIENT);
                break;
            }
            if (flag_h != 0 || (int)hd[DL_KASE] == DOGLEG_INVALID_GN) {
                // no Gauss-Newton step at this mu: the same linearisation again at 10 mu
                if (region.escalate()) { sv.need_build = need_gn = true; --sv.iter; continue; }
                have_gn = false;
            }
        }
        const TrialScalars t = have_gn ? trial_scalars(ts) : TrialScalars{sv.cost, 0.0, 0.0, 0.0};
        // a step without a Gauss-Newton step, or whose model change is not positive and finite, is invalid; a trial point whose cost
        // is not finite is rejected.  Neither is judged (row [cost, 0, ., 0, 0], no stop test).
        const bool valid = have_gn && t.model_change > 0.0 && std::isfinite(t.model_change);
        const bool step_ok = valid && std::isfinite(t.new_cost);
        if (have_gn) {
            const int kase = (int)hd[DL_KASE];
            if (kase >= 0 && kase < 3) ++ds.steps_by_case[kase];
            if (reused) ++ds.reused_steps;
        }
        const StepVerdict v = judge_step(opt, sv.cost, step_ok, t.new_cost, t.model_change, t.step_norm, t.x_norm, true);
        if (ba_apply_verdict(b, sv, v, step_ok, t, region.radius)) break;
        if (v.accepted) region.accept(v.rho, hd[DL_ZNORM], opt);
        else {
            ++s.num_unsuccessful_steps;
            if (!valid) { region.invalid(); ++ds.invalid_steps; sv.need_build = need_gn = true; }
            else region.reject();
        }
        invalid_in_a_row = valid ? 0 : invalid_in_a_row + 1;
        if (invalid_in_a_row >= kMaxConsecutiveInvalidSteps) {
            // Ceres' max_num_consecutive_invalid_steps (5): mu has only grown, and nothing lowers it but an accepted step
            stop(sv, STBA_FAILURE, STBA_TERM_SOLVER_FAIL);
            break;
        }
        if (v.accepted) {
            // a new linearisation: the next iteration builds and factors it at the new mu
            STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2));
            sv.need_build = need_gn = true;
            if (sv.deferred_ok) {
                sv.pending.on = true; sv.pending.accepted = true; sv.pending.iter = sv.iter;
            } else {
                STBA_TRY(ba_build_at(b, sv, 1.0 / region.mu));
                STBA_TRY(ba_read_linear_scalars(b, &sv.cost, &sv.gmax));
            }
        }
        if (ba_end_iteration(sv, v, t.step_norm, region.radius)) break;
    }
    // (a pending read behind the loop needs the reduced system of the last linearisation: the gradient comes with its build)
    if (sv.pending.on && sv.need_build) STBA_TRY(ba_build_at(b, sv, 1.0 / region.mu));
    STBA_TRY(ba_solve_end(b, sv, region.radius, sum));
    ds.final_mu = region.mu;
    b->dl.sum = ds;
    return STBA_OK;
}

}  // namespace stba

extern "C" {

int stba_ba_solve(stba_ba* b, const stba_lm_options* opt, stba_lm_summary* summary, double* trace,
                  stba_iteration_callback cb, void* cb_user) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    b->dl.sum = stba_dogleg_summary{};
    STBA_TRY(ba_refuse(b, "stba_ba_solve"));
    if (b->dl.trust_region == STBA_TR_TRADITIONAL_DOGLEG) return ba_run_dogleg(b, opt, summary, trace, cb, cb_user);
    return ba_run_lm(b, opt, 0, summary, trace, cb, cb_user);
}

int stba_ba_lm_iterations(stba_ba* b, const stba_lm_options* opt, int iterations, stba_lm_summary* summary,
                          double* trace) {
    if (!b || iterations <= 0) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    return ba_run_lm(b, opt, iterations, summary, trace, nullptr, nullptr);
}

int stba_ba_inner_sweep(stba_ba* b, double* cost_before, double* cost_after, int* iterations_per_block) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    STBA_TRY(ba_refuse(b, "stba_ba_inner_sweep"));
    const bool was_on = b->inner.on;
    if (!b->inner.sc) STBA_TRY(stba_ba_set_inner_iterations(b, 1, b->inner.tol, nullptr, nullptr, nullptr));   // (never set: the default ordering)
    STBA_TRY(ba_cost_only(b, b->cur, b->inner.sc + 2));
    STBA_TRY(ba_inner_sweep_enqueue(b, b->cur, nullptr));
    STBA_TRY(ba_cost_only(b, b->cur, b->inner.sc));
    double sc[3];
    STBA_TRY(download(sc, b->inner.sc, 3, b->st));
    const size_t ncl = b->inner.plan.cam.size(), npl = b->inner.plan.pt.size();
    std::vector<int> it(ncl + npl);
    if (!it.empty()) STBA_TRY(download(it.data(), b->inner.it, it.size(), b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    ba_invalidate(b);
    inner_summary_reset(b);
    b->inner.sum.sweeps = 1;
    b->inner.on = was_on;
    if (cost_before) *cost_before = 0.5 * sc[2];
    if (cost_after) *cost_after = 0.5 * sc[0];
    if (iterations_per_block) {
        const int nc = b->nc;
        memset(iterations_per_block, 0, sizeof(int) * ((size_t)2 * nc + b->np));
        for (size_t k = 0; k < ncl; ++k) {
            const int c = b->inner.plan.cam[k];
            if (b->inner.plan.kind[k] & 1u) iterations_per_block[c] = it[k];
            if (b->inner.plan.kind[k] & 2u) iterations_per_block[nc + c] = it[k];
        }
        for (size_t k = 0; k < npl; ++k) iterations_per_block[2 * nc + b->inner.plan.pt[k]] = it[ncl + k];
    }
    return STBA_OK;
}

int stba_ba_triangulate(stba_ba* b, int max_iter) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    STBA_TRY(launch_triangulate(b->np, b->pt_start, b->obs_cam, b->feat, b->cams[b->cur], b->pts[b->cur], b->pt_fixed,
                                max_iter, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    ba_invalidate(b);
    return STBA_OK;
}

}  // extern "C"
