// pg_engine.hip -- pose-graph SLAM on gfx950 (BASELINE config C4: 10k SE3 nodes, 40k relative-pose
// edges).  BUILD-DEFINED: the reference has no pose-graph code (SURVEY.md header fact 3); the
// conventions are the reference's Lie-group notes: right-multiplicative update T <- T exp(delta),
// tangent order [rho, theta] (st23-lie-group-v2/doc.tex:862-996, st21-lie/lie-group.tex:218-278),
// trajectory shape and ATE from st4-kalman/src/src/pose_simulation.cpp:17-88,198-209.
//
//   residual   r_ij = log(Z_ij^-1 T_i^-1 T_j)  in R^6
//   Jacobians  d r/d delta_j = Jr^-1(r),  d r/d delta_i = -Jr^-1(r) Ad(T_j^-1 T_i),
//              Jr^-1(r) = I + ad(r)/2 + ad(r)^2/12
//   solver     Levenberg-Marquardt (same control flow as the BA engine); the damped normal equations
//              (6 n_nodes unknowns, block-sparse) are solved matrix-free by preconditioned conjugate
//              gradients as an INEXACT Newton step: the PCG stops at |r| <= eta |g| with a forcing
//              sequence eta_k (Eisenstat-Walker), decided on the device.
//   preconditioner  M^-1 = blockdiag(H_ii + D_i)^-1 + P (P^T (J^T J + D) P)^-1 P^T: two levels, additive.
//              The coarse space holds six rigid-body modes per GROUP of consecutive nodes (a stretch of
//              the trajectory moved as one body): delta_k = Ad(T_k^-1 T_ref(group)) xi.  Block Jacobi alone
//              leaves the long, smooth error modes of the chain (drift) to the Krylov iteration -- 939
//              iterations to 1e-12 at C4, the cap of 1000 on every LM iteration in round 3; a block
//              TRIDIAGONAL preconditioner (the odometry chain factored exactly) was measured first and
//              hardly helps (812: its diagonal carries the loop closures' stiffness, which the smooth
//              modes do not feel); the rigid-body coarse space cuts it to 67-109 (groups of 16-64
//              nodes), and with the forcing sequence a C4 LM iteration takes ~24 PCG iterations.
//              The coarse matrix (942 unknowns at C4) is inverted explicitly once per LM iteration
//              (dense_chol.hip, chol_spd_inverse_dev: the only MFMA work of this engine) and applied
//              as a dense product.
//
// Data in HBM: poses [n][7] (two copies), edges (i, j) int32, meas [m][7], r [m][6], Ji/Jj [36][m] (COMPONENT-major: entry k
// of edge e at k m + e, so that the lanes of a wave -- consecutive edges -- read and write consecutive addresses; edge-major
// [m][36] made every load instruction touch 64 cache lines: the matrix-free product took 24 us for 25 MB),
// g [6n], Hd [n][36] (diagonal blocks), Minv [n][36], PCG vectors x r z p q [6n].
//
// This unit holds the engine's creation and destruction, the LM loop (stba_pg_solve) with the steps that belong to no other unit --
// the set-up of a solve, the linearisation's enqueue and scalars, the trial point, and the kernels that finish, export and update
// them --, what pg_covariance.hip sees of the engine, and the rest of the stba_pg_* entry points.  The engine object and the
// functions that cross units: pg_engine.hpp; the linearisation: pg_linearize.hip; the coarse space: pg_coarse.hip; the PCG: pg_pcg.hip;
// node pose priors: pg_prior.hip.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pg_covariance.hpp"
#include "pg_device.hpp"
#include "pg_engine.hpp"

namespace stba {
namespace {

// |g|^2 and |g|_inf as per-workgroup partials {sum, max} (behind the cross-rank sum of g when there are several ranks)
__global__ __launch_bounds__(256) void pg_gnorm_kernel(int N, const double* __restrict__ g, double* __restrict__ part) {
    __shared__ double sm[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double v = i < N ? g[i] : 0.0;
    double s = v * v, mx = fabs(v);
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o, 64); mx = fmax(mx, __shfl_down(mx, o, 64)); }
    __shared__ double ss[4];
    if ((threadIdx.x & 63) == 0) { ss[threadIdx.x >> 6] = s; sm[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) { part[blockIdx.x * 2] = (ss[0] + ss[1]) + (ss[2] + ss[3]); part[blockIdx.x * 2 + 1] = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3])); }
}

// trial point of an LM iteration: the scalars the host decides on, summed on the device and written to mapped host memory
// (one rank) or to a device block the cross-rank sum goes over first.  out: {cost2_new, |J x|^2, g.x, |dx|^2, |x|^2, seq}
__global__ __launch_bounds__(256) void pg_trial_finish_kernel(int nb_e, const double* __restrict__ part_e, int nb_tt,
                                                              const double* __restrict__ part_tt, int nb_u, const double* __restrict__ part_u,
                                                              const PgPcgState* __restrict__ state, double* __restrict__ out, double seq) {
    const double c2 = sum_partials_dev(part_e, nb_e, 1, 0);
    const double tt = sum_partials_dev(part_tt, nb_tt, 2, 0);
    const double gx = sum_partials_dev(part_u, nb_u, 4, 0);
    const double s2 = sum_partials_dev(part_u, nb_u, 4, 1);
    const double x2 = sum_partials_dev(part_u, nb_u, 4, 2);
    __shared__ double hp[8];
    if (threadIdx.x == 0) {
        hp[0] = c2; hp[1] = tt; hp[2] = gx; hp[3] = s2; hp[4] = x2;
        hp[5] = state ? (double)state->iters : 0.0; hp[6] = state ? (double)state->hit_cap : 0.0; hp[7] = state ? state->rr0 : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < 64) stamped_store_wave(out, hp, 8, seq, threadIdx.x);       // (a stamped block: common.hpp)
}
// linearisation: {cost2, |g|_inf, seq}
__global__ __launch_bounds__(256) void pg_linear_finish_kernel(int nb_e, const double* __restrict__ part_e, int nb_g, const double* __restrict__ part_g,
                                                               double* __restrict__ out, double seq) {
    const double c2 = sum_partials_dev(part_e, nb_e, 1, 0);
    const double g2 = sum_partials_dev(part_g, nb_g, 2, 0);
    __shared__ double sq[256];
    double mx = 0.0;
    for (int k = threadIdx.x; k < nb_g; k += 256) mx = fmax(mx, part_g[2 * k + 1]);
    sq[threadIdx.x] = mx;
    __syncthreads();
    __shared__ double hp[3];
    if (threadIdx.x == 0) {
        for (int k = 1; k < 256; ++k) mx = fmax(mx, sq[k]);
        hp[0] = c2; hp[1] = mx; hp[2] = g2;
    }
    __syncthreads();
    if (threadIdx.x < 64) stamped_store_wave(out, hp, 3, seq, threadIdx.x);
}
__global__ void pg_export_kernel(int cnt, const double* __restrict__ src, double* __restrict__ out, double seq) {
    stamped_store_wave(out, src, cnt, seq, threadIdx.x);      // (one wave; src is device memory the previous kernel or collective left)
}

// trial poses + statistics of the step: partial[b] = {g.x, |x_new - x|^2, |x|^2, 0}
__global__ __launch_bounds__(256) void pg_update4_kernel(int n_nodes, const double* __restrict__ poses, const double* __restrict__ dx,
                                                         const double* __restrict__ g, const unsigned char* __restrict__ fixed,
                                                         double* __restrict__ poses_new, double* __restrict__ partial) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double a = 0.0, b = 0.0, c = 0.0;
    if (i < n_nodes) {
        double T[7], d[6], Tn[7];
        for (int k = 0; k < 7; ++k) T[k] = poses[(size_t)i * 7 + k];
        const bool fx = fixed && fixed[i];
        for (int k = 0; k < 6; ++k) { d[k] = fx ? 0.0 : dx[(size_t)i * 6 + k]; c += g[(size_t)i * 6 + k] * d[k]; }
        if (fx) for (int k = 0; k < 7; ++k) Tn[k] = T[k];
        else se3_retract(T, d, Tn);
        for (int k = 0; k < 7; ++k) {
            poses_new[(size_t)i * 7 + k] = Tn[k];
            if (!fx) { a += (Tn[k] - T[k]) * (Tn[k] - T[k]); b += T[k] * T[k]; }
        }
    }
    double out2[2], out3[2];
    block_sum2(a, b, out2);
    __syncthreads();
    block_sum2(c, 0.0, out3);
    if (threadIdx.x == 0) { partial[blockIdx.x * 4] = out3[0]; partial[blockIdx.x * 4 + 1] = out2[0]; partial[blockIdx.x * 4 + 2] = out2[1]; partial[blockIdx.x * 4 + 3] = 0.0; }
}

// Everything of an engine that is not memory, then the engine: its DevBuf members free themselves in `delete`.  Both streams are
// synchronised FIRST (nothing on the device reads a buffer that is about to go); then the Cholesky's per-stream cache forgets the
// second one, then the events, the mapped blocks and the streams, and the buffers last.
void pg_free(stba_pg* g) {
    PgCoarseJob& j = g->job;
    if (g->st) (void)hipStreamSynchronize(g->st);
    (void)j.quiesce();
    if (j.st2) chol_forget_stream(j.st2);
    for (DevEvent* e : {&j.ev_in, &j.ev_read, &j.ev_job[0], &j.ev_job[1], &g->ev_t[0], &g->ev_t[1]}) e->reset();
    g->exp.release();
    g->fin.release();
    if (j.st2) (void)hipStreamDestroy(j.st2);
    if (g->own && g->st) (void)hipStreamDestroy(g->st);
    delete g;
}

// the tail of the two finish kernels.  One rank: the kernel has written the stamped block itself.  Several: it wrote g->scal_dev, the
// hook sums the first n_summed scalars and a kernel exports the n_payload of them with the stamp.  Then the host reads g->fin_vals.
int pg_read_block(stba_pg* g, int n_summed, int n_payload) {
    if (g->ar) {
        STBA_TRY(pg_hook(g, g->scal_dev, (size_t)n_summed));
        hipLaunchKernelGGL(pg_export_kernel, dim3(1), dim3(64), 0, g->st, n_payload, g->scal_dev, g->fin.dev, g->seq);
    }
    STBA_HIP(hipGetLastError());
    const double seq = g->seq;
    return stamped_wait(g->fin.host, n_payload, [seq](double st) { return st == seq; }, g->fin_vals, hip_stream_state(g->st), "pose graph", 120.0);
}

// ---- set-up of a solve: the coarse space for this group size, the second stream, the flags derived once
int pg_solve_begin(stba_pg* g, PgSolve& sv) {
    const stba_pcg_options& pcg = sv.pcg;
    STBA_TRY(pg_setup_coarse(g, pcg.coarse_group));
    sv.coarse = g->coarse.agg > 0;
    // the second stream of the coarse inverse (pg_coarse_refresh); a job of the previous solve may still be in flight: it is awaited here,
    // where it costs nothing, instead of at the end of that solve, where it would have been the last 0.3 ms of its wall time
    sv.async_inv = sv.coarse && pcg.coarse_async != 0;
    if (sv.async_inv) {
        STBA_TRY(g->job.ensure());
        if (g->job.in_flight) STBA_TRY(g->job.quiesce());      // (only then: a synchronise of an idle stream still costs the host)
    }
    sv.build_on_st2 = sv.async_inv && !g->ar;
    if (sv.coarse) STBA_HIP(hipMemsetAsync(g->cflag + 1, 0, sizeof(int), g->st));      // this solve's count of failed coarse operators
    sv.multi = (g->ar != nullptr);
    sv.chunk = std::max(1, pcg.check_every);
    sv.forcing = pcg.forcing_eta0 > 0.0;
    sv.eta = pcg.forcing_eta0;
    sv.ps.coarse_dim = sv.coarse ? g->coarse.nc : 0;
    sv.pp_ok = pg_one_kernel_eligible(g, sv);
    // (stba_lm_options::phase_timing: hipEvents around the linear solve -- the persistent kernel, or the launches of the PCG loop --
    // for bench.py's roofline of the C4 line; an event is a packet of its own on the queue, so only on request)
    sv.timing = sv.opt.phase_timing != 0;
    return STBA_OK;
}

// ---- linearisation at the current point: residuals, Jacobians, gradient | diagonal blocks, the coarse basis and matrix
int pg_linearize_enqueue(stba_pg* g, const PgSolve& sv) {
    STBA_TRY(pg_wait_for_job_reads(g));
    STBA_TRY(pg_linearize(g, g->cur, true));
    pg_gather_blocks(g);
    STBA_TRY(pg_hook(g, g->g, (size_t)g->n * 42));
    hipLaunchKernelGGL(pg_gnorm_kernel, dim3(g->nb_vec), dim3(256), 0, g->st, 6 * g->n, g->g, g->part_c);
    if (sv.coarse) STBA_TRY(pg_coarse_linearized(g, sv));
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

// cost and |g|_inf of that linearisation: one kernel sums, the host reads mapped memory (several ranks: the cost goes over the hook)
int pg_linearize_finish(stba_pg* g, double* cost, double* gmax, double* g2) {
    g->seq += 1.0;
    hipLaunchKernelGGL(pg_linear_finish_kernel, dim3(1), dim3(256), 0, g->st, pg_cost_slots(g), g->part_e, g->nb_vec, g->part_c, g->ar ? g->scal_dev : g->fin.dev, g->seq);
    STBA_TRY(pg_read_block(g, 1, 3));
    *cost = 0.5 * g->fin_vals[0]; *gmax = g->fin_vals[1]; *g2 = g->fin_vals[2];
    return STBA_OK;
}

// ---- model change, trial point: |J x|^2 from the edge kernel (its |t_e|^2 sums), g.x and the step norms from the update kernel;
// the trial block (cost, x^T H x, g.x, |step|^2, |x|^2, PCG iterations, capped / timed out, |r_0|^2) comes home in g->fin_vals
int pg_trial_point(stba_pg* g) {
    const int nxt = g->cur ^ 1;
    pg_edge_product(g, g->x, g->part_b, nullptr);
    hipLaunchKernelGGL(pg_update4_kernel, dim3(g->nb_nodes), dim3(256), 0, g->st, g->n, g->poses[g->cur], g->x, g->g, g->fixed, g->poses[nxt], g->part_u);
    STBA_TRY(pg_linearize(g, nxt, false, g->x));      // (priors: their cost, and their |J' x|^2 behind the edge product's slots of part_b)
    g->seq += 1.0;
    hipLaunchKernelGGL(pg_trial_finish_kernel, dim3(1), dim3(256), 0, g->st, pg_cost_slots(g), g->part_e, pg_cost_slots(g), g->part_b, g->nb_nodes, g->part_u,
                       g->state, g->ar ? g->scal_dev : g->fin.dev, g->seq);
    return pg_read_block(g, 2, 8);      // (several ranks: cost and |J x|^2 summed over the edge shards)
}

}  // namespace

// the all-reduce hook over `count` doubles at `buf`, on the engine's stream (one rank: nothing)
int pg_hook(stba_pg* g, double* buf, size_t count) {
    if (g->ar && g->ar(g->ar_user, buf, count, g->st) != 0) return fail(STBA_ERR_CALLBACK, "all-reduce hook failed");
    return STBA_OK;
}

// ---- what pg_covariance.hip sees of the engine (pg_covariance.hpp)
void pg_cov_graph(const stba_pg* g, PgCovGraph* out) {
    out->n = g->n; out->m = g->m;
    out->ei = g->h_ei.data(); out->ej = g->h_ej.data();
    out->fixed = g->h_fixed.empty() ? nullptr : g->h_fixed.data();
    out->several_ranks = g->ar != nullptr || g->world > 1;
    out->anchored = g->pr.n ? g->pr.anchored.data() : nullptr;
}
int pg_cov_linearize(stba_pg* g, PgCovDevice* out) {
    // (a coarse inverse of the last solve may still be reading the diagonal blocks on the second stream)
    if (g->job.in_flight) STBA_TRY(g->job.quiesce());
    STBA_TRY(pg_linearize(g, g->cur, true));
    pg_gather_blocks(g);
    STBA_HIP(hipGetLastError());
    out->st = g->st; out->node_start = g->node_start; out->end_code = g->end_code; out->end_rem = g->end_rem;
    out->Ji = g->Ji; out->Jj = g->Jj; out->Hd = g->Hd; out->fixed = g->fixed;
    out->node_slot = g->pr.n ? g->pr.node_slot.get() : nullptr; out->Hp = g->pr.n ? g->pr.Hp.get() : nullptr;
    return STBA_OK;
}
}  // namespace stba

extern "C" {

void stba_pcg_default_options(stba_pcg_options* o) {
    if (!o) return;
    o->max_iterations = 1000;
    o->relative_tolerance = 1e-12;
    o->check_every = 4;
    o->forcing_eta0 = 0.1;
    o->forcing_eta_min = 0.01;          // (stba.h: the measured reason)
    o->coarse_group = 0;
    o->coarse_refresh_every = 1;
    o->one_kernel_solve = 1;
    o->coarse_async = 1;
    o->forcing_eta_final = 0.0;
    o->coarse_eta = 0.0;
    o->coarse_async_after = 1;
    o->coarse_async_decrease = 0.5;
}

// everything of stba_pg_create behind the engine object and its stream: the buffers and their contents.  A failure leaves a partly
// filled engine, which stba_pg_create frees
static int pg_fill(stba_pg* g, int n_nodes, int n_edges, const double* poses, const int* edge_i, const int* edge_j, const double* meas,
                   const unsigned char* node_fixed) {
    const size_t n = (size_t)n_nodes, m = (size_t)n_edges;
    STBA_TRY(g->poses[0].alloc(n * 7)); STBA_TRY(g->poses[1].alloc(n * 7)); STBA_TRY(g->ei.alloc(m)); STBA_TRY(g->ej.alloc(m));
    STBA_TRY(g->meas.alloc(m * 7)); STBA_TRY(g->r.alloc(m * 6)); STBA_TRY(g->Ji.alloc(m * 36)); STBA_TRY(g->Jj.alloc(m * 36));
    STBA_TRY(g->g.alloc(n * 42)); g->Hd = g->g + n * 6;      // [gradient 6n | diagonal blocks 36n]: one cross-rank sum
    STBA_TRY(g->Minv.alloc(n * 36)); STBA_TRY(g->d.alloc(n * 6)); STBA_TRY(g->scalar.alloc(1));
    STBA_TRY(g->scale.alloc(n * 6)); STBA_TRY(g->x.alloc(n * 6)); STBA_TRY(g->rr.alloc(n * 6)); STBA_TRY(g->z.alloc(n * 6));
    STBA_TRY(g->p.alloc(n * 6)); STBA_TRY(g->q.alloc(n * 6));
    const size_t np_ = (size_t)std::max(g->nb_vec, std::max(g->nb_nodes, g->nb_edges)) * 2 + 2;
    STBA_TRY(g->part_e.alloc(np_)); STBA_TRY(g->part_a.alloc(np_)); STBA_TRY(g->part_b.alloc(np_)); STBA_TRY(g->part_c.alloc(np_));
    STBA_TRY(g->part_d.alloc(np_));
    g->part_cap = np_;
    if (node_fixed) STBA_TRY(g->fixed.alloc(n));
    STBA_TRY(g->node_start.alloc(n + 1)); STBA_TRY(g->end_code.alloc(2 * m)); STBA_TRY(g->u.alloc(12 * m));
    STBA_TRY(g->end_node.alloc(2 * m)); STBA_TRY(g->contrib.alloc(2 * m * 28));
    STBA_TRY(g->end_pos.alloc(2 * m)); STBA_TRY(g->end_rem.alloc(2 * m)); STBA_TRY(g->Bend.alloc(72 * m)); STBA_TRY(g->ubuf.alloc(12 * n));
    STBA_TRY(g->pbuf.alloc((size_t)2 * PP_GROUPS_MAX * PP_SLOT)); STBA_TRY(g->ustamp.alloc((size_t)PP_GROUPS_MAX * PP_STAMP)); STBA_TRY(g->pstamp.alloc((size_t)PP_GROUPS_MAX * PP_STAMP));
    if (hipMemsetAsync(g->ustamp, 0, PP_GROUPS_MAX * PP_STAMP * sizeof(int), g->st) != hipSuccess ||
        hipMemsetAsync(g->pstamp, 0, PP_GROUPS_MAX * PP_STAMP * sizeof(int), g->st) != hipSuccess)
        return fail(STBA_ERR_HIP, "stba_pg_create: memset");
    g->nb_nodes4 = (n_nodes + PG_NPW - 1) / PG_NPW;
    STBA_TRY(g->part_u.alloc((size_t)g->nb_nodes * 4 + 4)); STBA_TRY(g->scal_dev.alloc(16)); STBA_TRY(g->state.alloc(1)); STBA_TRY(g->cflag.alloc(2));
    if (g->exp.alloc((size_t)stamped_doubles(PX_COUNT)) != STBA_OK || g->fin.alloc(16) != STBA_OK)
        return fail(STBA_ERR_ALLOC, "stba_pg_create: mapped host memory");
    memset(&g->last_pcg, 0, sizeof g->last_pcg);
    {   // the edge ends sorted by node (pg_plan.hpp)
        PgEnds ends;
        pg_build_ends(n_nodes, n_edges, edge_i, edge_j, &ends);
        if (upload(g->end_pos, ends.end_pos.data(), 2 * m, g->st) != STBA_OK || upload(g->end_rem, ends.end_rem.data(), 2 * m, g->st) != STBA_OK ||
            upload(g->node_start, ends.node_start.data(), n + 1, g->st) != STBA_OK || upload(g->end_code, ends.end_code.data(), 2 * m, g->st) != STBA_OK ||
            upload(g->end_node, ends.end_node.data(), 2 * m, g->st) != STBA_OK || hipStreamSynchronize(g->st) != hipSuccess)
            return fail(STBA_ERR_HIP, "stba_pg_create: upload failed");
        g->node_start_host.swap(ends.node_start);
    }
    if (upload(g->poses[0], poses, n * 7, g->st) != STBA_OK || upload(g->ei, edge_i, m, g->st) != STBA_OK ||
        upload(g->ej, edge_j, m, g->st) != STBA_OK || upload(g->meas, meas, m * 7, g->st) != STBA_OK ||
        (node_fixed && upload(g->fixed, node_fixed, n, g->st) != STBA_OK) || hipStreamSynchronize(g->st) != hipSuccess)
        return fail(STBA_ERR_HIP, "stba_pg_create: upload failed");
    // The buffers of the default coarse space, the second stream and its events are made HERE: a solve used to begin with
    // a dozen allocations (the 33 MB inversion workspace among them), a stream and four events -- ~ 0.4 ms of a 6.4 ms C4 solve
    // on a fresh engine, inside the time every caller and bench.py measure.  (A solve with another group size makes its own; a
    // graph too large for the default space is told so by the solve, not here.)
    if (pg_setup_coarse(g, 0) == STBA_OK && g->coarse.agg > 0) (void)g->job.ensure();
    (void)hipStreamSynchronize(g->st);
    return STBA_OK;
}

int stba_pg_create(stba_pg** out, int n_nodes, int n_edges, const double* poses, const int* edge_i, const int* edge_j,
                   const double* meas, const unsigned char* node_fixed, void* hip_stream) {
    if (!out) return fail(STBA_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (n_nodes <= 0 || n_edges <= 0 || !poses || !edge_i || !edge_j || !meas)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_create: null or empty input");
    if (pg_check_edges(n_nodes, n_edges, edge_i, edge_j) >= 0) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_create: bad edge");
    STBA_TRY(require_device());
    stba_pg* g = new stba_pg();
    g->n = n_nodes; g->m = n_edges;
    g->h_ei.assign(edge_i, edge_i + n_edges); g->h_ej.assign(edge_j, edge_j + n_edges);
    if (node_fixed) g->h_fixed.assign(node_fixed, node_fixed + n_nodes);
    if (hip_stream) g->st = reinterpret_cast<hipStream_t>(hip_stream);
    else { if (hipStreamCreate(&g->st) != hipSuccess) { delete g; return fail(STBA_ERR_HIP, "hipStreamCreate"); } g->own = true; }
    g->nb_nodes = (n_nodes + 255) / 256; g->nb_vec = (6 * n_nodes + 255) / 256; g->nb_edges = (n_edges + 255) / 256;
    const int rc = pg_fill(g, n_nodes, n_edges, poses, edge_i, edge_j, meas, node_fixed);
    if (rc != STBA_OK) { pg_free(g); return rc; }
    *out = g;
    return STBA_OK;
}

int stba_pg_set_allreduce(stba_pg* g, stba_allreduce_fn fn, void* user, int rank, int world_size) {
    if (!g || rank < 0 || world_size < 1 || rank >= world_size) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    if (!fn && world_size > 1) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_set_allreduce: world_size > 1 needs a hook");
    // (node pose priors are one rank's: their terms are summed on this device only.  A call that clears the hook is never refused)
    if (g->pr.n && (fn || world_size > 1))
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_set_allreduce: the engine holds node pose priors, which are implemented for one rank only (clear them first)");
    g->ar = (world_size > 1 || fn) ? fn : nullptr;
    g->ar_user = user; g->rank = rank; g->world = world_size;
    return STBA_OK;
}

int stba_pg_destroy(stba_pg* g) {
    if (!g) return STBA_OK;
    pg_free(g);
    return STBA_OK;
}

int stba_pg_get_poses(stba_pg* g, double* poses) {
    if (!g || !poses) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    STBA_HIP(hipMemcpyAsync(poses, g->poses[g->cur], (size_t)g->n * 7 * sizeof(double), hipMemcpyDeviceToHost, g->st));
    STBA_HIP(hipStreamSynchronize(g->st));
    return STBA_OK;
}

int stba_pg_solve(stba_pg* g, const stba_lm_options* opt_in, const stba_pcg_options* pcg_in, stba_lm_summary* summary,
                  double* trace, int* pcg_iterations_total) {
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    stba_lm_options opt;
    if (opt_in) opt = *opt_in; else stba_lm_default_options(&opt);
    stba_pcg_options pcg;
    if (pcg_in) pcg = *pcg_in; else stba_pcg_default_options(&pcg);
    stba_lm_summary s;
    memset(&s, 0, sizeof s);
    const double t0 = wall_s();
    // ---- options and set-up
    PgSolve sv(opt, pcg);
    STBA_TRY(pg_solve_begin(g, sv));
    stba_pcg_summary& ps = sv.ps;
    TrustRegion& region = sv.region;
    const double* fin = g->fin_vals;          // (the validated copy of the mapped block g->fin)

    // ---- first linearisation
    STBA_TRY(pg_linearize_enqueue(g, sv));
    STBA_TRY(pg_linearize_finish(g, &sv.cost, &sv.gmax, &sv.g2));
    s.initial_cost = sv.cost;
    trace_start(trace, sv.cost, sv.gmax, region.radius);
    s.termination_type = STBA_NO_CONVERGENCE; s.termination_reason = STBA_TERM_MAX_ITER;
    bool done = sv.gmax <= opt.gradient_tolerance;
    if (done) { s.termination_type = STBA_CONVERGENCE; s.termination_reason = STBA_TERM_GRADIENT; }
    if (!std::isfinite(sv.cost)) { s.termination_type = STBA_FAILURE; s.termination_reason = STBA_TERM_SOLVER_FAIL; done = true; }   // (Ceres: initial evaluation failed, see stba_ba_solve)
    while (!done) {
        if (sv.iter >= opt.max_num_iterations) break;
        if (region.below_min(opt)) { s.termination_type = STBA_CONVERGENCE; s.termination_reason = STBA_TERM_MIN_RADIUS; break; }
        ++sv.iter;
        // ---- preconditioner (behind an accepted step it and the job's head are already on their way)
        const bool head_was_done = sv.head_done;
        if (!sv.head_done) {
            STBA_TRY(pg_wait_for_job_reads(g));      // (a rejected step: no linearisation in between)
            pg_precond(g, sv);
        }
        sv.head_done = false;
        PgCoarseUse cu;
        STBA_TRY(pg_coarse_refresh(g, sv, head_was_done, &cu));
        // ---- PCG and trial point.  A deferred job goes BEHIND the launch of the one-kernel PCG, so that the host enqueues it while
        // the kernel runs, but in FRONT of the launch path's, which talks to the host all along (pg_job_rest: the measured reason)
        const double eta_k = sv.forcing ? sv.eta : pcg.relative_tolerance;
        const int nxt = g->cur ^ 1;
        const bool one_kernel = sv.pp_ok && !g->pp_disabled;
        if (sv.timing && !g->ev_t[0]) { STBA_TRY(g->ev_t[0].create()); STBA_TRY(g->ev_t[1].create()); }
        if (sv.timing) STBA_HIP(hipEventRecord(g->ev_t[0], g->st));
        if (!one_kernel && cu.job_deferred) { STBA_TRY(pg_job_rest(g, sv, cu.job)); cu.job_deferred = false; }
        if (one_kernel) STBA_TRY(pg_pcg_one_kernel(g, sv, cu.Ainv, eta_k)); else STBA_TRY(pg_pcg_by_launches(g, sv, cu.Ainv, eta_k));
        if (sv.timing) STBA_HIP(hipEventRecord(g->ev_t[1], g->st));
        if (cu.job_deferred) { STBA_TRY(pg_job_rest(g, sv, cu.job)); cu.job_deferred = false; }
        STBA_TRY(pg_trial_point(g));
        if (sv.timing) {
            float ms = 0.f;
            STBA_HIP(hipEventSynchronize(g->ev_t[1]));
            STBA_HIP(hipEventElapsedTime(&ms, g->ev_t[0], g->ev_t[1]));
            ps.linear_solve_ms += (double)ms;
        }
        if (one_kernel && fin[6] != (double)PP_TIMED_OUT) ++ps.one_kernel_solves;
        if (one_kernel && fin[6] == (double)PP_TIMED_OUT) {
            // a stamp never came: the workgroups were not all resident (another process on the device).  Once is enough: this
            // engine solves with launches from here on, starting with this very iteration.
            g->pp_disabled = true;
            STBA_TRY(pg_pcg_by_launches(g, sv, cu.Ainv, eta_k));
            STBA_TRY(pg_trial_point(g));
        }
        // ---- verdict
        const double new_cost = 0.5 * fin[0], xhx = fin[1], gx = fin[2], step2 = fin[3], x2 = fin[4];
        const int k = (int)fin[5];
        const bool capped = fin[6] != 0.0;
        const double rr0 = fin[7];
        ps.iterations_total += k; ++ps.solves; ps.hit_cap += capped ? 1 : 0; ps.max_iterations_in_a_solve = std::max(ps.max_iterations_in_a_solve, k);
        ps.last_eta = eta_k;
        bool ok = std::isfinite(rr0);
        const double model_change = -gx - 0.5 * xhx;
        const double step_norm = std::sqrt(step2), x_norm = std::sqrt(x2);
        ok = ok && model_change > 0.0 && std::isfinite(model_change) && std::isfinite(new_cost);
        const StepVerdict v = judge_step(opt, sv.cost, ok, new_cost, model_change, step_norm, x_norm);
        trace_step(trace, sv.iter, ok, sv.cost, new_cost, v, sv.gmax, step_norm, region.radius);
        if (v.stop) {        // (no progress line)
            s.termination_type = STBA_CONVERGENCE; s.termination_reason = v.stop;
            if (v.accepted) { g->cur = nxt; sv.cost = new_cost; ++s.num_successful_steps; g->coarse_valid = false; }
            break;
        }
        if (v.accepted) {
            g->cur = nxt;
            ++s.num_successful_steps;
            sv.last_rel_decrease = sv.cost > 0.0 ? v.cost_change / sv.cost : 1.0;
            region.accept(v.rho, opt);
            double g2_new = 0.0;
            STBA_TRY(pg_linearize_enqueue(g, sv));
            if (sv.async_inv && sv.build_on_st2) {        // the next iteration's preconditioner kernel and the head of its job, at once (pg_job_head)
                pg_precond(g, sv);
                STBA_HIP(hipEventRecord(g->job.ev_in, g->st));
                STBA_TRY(pg_job_head(g));
                sv.head_done = true;
            }
            STBA_TRY(pg_linearize_finish(g, &sv.cost, &sv.gmax, &g2_new));
            sv.eta = pg_next_eta(pcg, opt, sv.eta, sv.g2, g2_new, v.cost_change, sv.cost);
            sv.g2 = g2_new;
            if (trace) { trace[(size_t)sv.iter * STBA_TRACE_COLS + 2] = sv.gmax; trace[(size_t)sv.iter * STBA_TRACE_COLS + 5] = region.radius; }
            // (the gradient is tested here, before the progress line: none is printed for the converging iteration)
            if (sv.gmax <= opt.gradient_tolerance) { s.termination_type = STBA_CONVERGENCE; s.termination_reason = STBA_TERM_GRADIENT; break; }
        } else {
            ++s.num_unsuccessful_steps;
            region.reject();
            if (trace) trace[(size_t)sv.iter * STBA_TRACE_COLS + 5] = region.radius;
        }
        if (opt.minimizer_progress_to_stdout) {
            char tail[64];
            snprintf(tail, sizeof tail, "  pcg %d eta %.1e%s", k, eta_k, capped ? " CAP" : "");
            progress_step(sv.iter, sv.cost, v, sv.gmax, step_norm, region.radius, tail);
        }
    }
    // ---- summary
    finish_summary(&s, sv.iter, sv.cost, region.radius, sv.gmax, t0);
    if (summary) *summary = s;
    if (pcg_iterations_total) *pcg_iterations_total = ps.iterations_total;
    if (sv.coarse) {        // (how many coarse operators could not be factored: counted on the device, read once per solve)
        int cf = 0;
        if (hipMemcpyAsync(&cf, g->cflag + 1, sizeof(int), hipMemcpyDeviceToHost, g->st) == hipSuccess && hipStreamSynchronize(g->st) == hipSuccess)
            ps.coarse_failures = cf;
    }
    g->last_pcg = ps;
    return STBA_OK;
}

int stba_pg_last_pcg_summary(stba_pg* g, stba_pcg_summary* out) {
    if (!g || !out) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    *out = g->last_pcg;
    return STBA_OK;
}

}  // extern "C"

