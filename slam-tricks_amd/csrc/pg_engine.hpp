// pg_engine.hpp -- the pose-graph engine object behind the opaque stba_pg of include/stba.h, the state of one stba_pg_solve call,
// and the few host functions that cross the pose-graph units: pg_linearize.hip (linearisation, weights and losses), pg_coarse.hip (the
// coarse space and its second-stream job), pg_pcg.hip (the two forms of the PCG solve), pg_prior.hip (node pose priors) and pg_engine.hip
// (creation, the LM loop and the rest of the stba_pg_* entry points).  No kernel is declared or defined here.
#pragma once
#include <vector>

#include "common.hpp"
#include "lm_policy.hpp"
#include "pg_plan.hpp"

namespace stba {

// device-resident scalars of one PCG solve; every kernel of iteration k reads rz[k & 1], the direction kernel writes rz[(k + 1) & 1]
struct PgPcgState {
    double rz[2];
    double rr0, rr, tol2;
    int iters, done, hit_cap, ticks;
};
// what the launch-path PCG shows the polling host: a STAMPED block (common.hpp) of one line -- payload {rr0, rr, iters, done, hit_cap},
// stamp = the tick count
enum { PX_RR0 = 0, PX_RR = 1, PX_ITERS = 2, PX_DONE = 3, PX_HIT_CAP = 4, PX_COUNT = 5 };

constexpr int PP_TIMED_OUT = 2;      // PgPcgState::hit_cap: a stamp never came (the workgroups were not all resident): the caller repeats the solve with launches

// The coarse inverse OFF the critical path (stba_pcg_options::coarse_async): a second stream inverts the coarse operator of LM
// iteration k while the first runs iteration k's PCG with the inverse made during iteration k - 1 (pg_coarse.hip: pg_job_head,
// pg_job_rest, pg_wait_for_job_reads, pg_coarse_refresh).  The job's stream, events, buffer pair and flags have this one owner.
// reads_pending implies in_flight: both are set by the job's head, and only quiesce() clears in_flight.
struct PgCoarseJob {
    hipStream_t st2 = nullptr;
    DevEvent ev_in, ev_read, ev_job[2];   // the job may start | it has read its inputs | it has written Ainv[0 / 1]
    DevBuf<double> Ainv[2];               // the pair the jobs alternate between ([0] alone: the synchronous form's inverse)
    bool in_flight = false;               // work may still be running on st2
    bool reads_pending = false;           // ev_read guards inputs that the first stream has not waited for yet
    bool ac0_valid = false;               // Ac0 belongs to the current linearisation
    // the stream and its events (once)
    int ensure() {
        if (st2) return STBA_OK;
        STBA_HIP(hipStreamCreateWithFlags(&st2, hipStreamNonBlocking));
        for (DevEvent* e : {&ev_in, &ev_read, &ev_job[0], &ev_job[1]}) STBA_TRY(e->create(hipEventDisableTiming));
        return STBA_OK;
    }
    // nothing of a job runs any more, and nothing is left to wait for: whoever frees or overwrites what a job reads or writes calls
    // this first (behind a synchronised st2 every event has fired, so a wait for ev_read would enqueue nothing)
    int quiesce() {
        if (st2) STBA_HIP(hipStreamSynchronize(st2));
        in_flight = false; reads_pending = false;
        return STBA_OK;
    }
};

// Node pose priors (stba_pg_set_priors; kernels and setter: pg_prior.hip).  Prior k names a node, a pose Z_k and a square-root
// information W_k: r_k = log(Z_k^-1 T_node), the j side of pg_edge with T_i = I.  Held SORTED by node (stably: a node's priors in the
// caller's order), with a CSR over the prior-bearing nodes, each of which has a compact SLOT.  n == 0: nothing is held, and the
// engine enqueues what one that never had priors enqueues.
constexpr int PG_PRIOR_NT = 256;             // the per-prior kernel: one lane per prior
constexpr int PG_PRIOR_NODES_PER_WG = 32;    // the per-node kernel: eight lanes per prior-bearing node
struct PgPriors {
    int n = 0, n_slots = 0, nb = 0;          // priors | prior-bearing nodes | workgroups of the per-prior kernel
    DevBuf<int> node;                        // [n]  node of the prior at a sorted position
    DevBuf<double> pose, W;                  // [n][7], [n][36] (row-major), sorted like node
    DevBuf<int> slot_node, slot_start;       // [n_slots] the slot's node | [n_slots + 1] its priors (CSR into the sorted order)
    DevBuf<int> node_slot;                   // [n_nodes] the node's slot, or -1
    DevBuf<double> r, J;                     // [n][6], [n][36]: W r and W J of the last linearisation (J == 0 on a constant node)
    DevBuf<double> Hp;                       // [n_slots][36]: sum of J'^T J' over the slot's priors, for the matrix-free products
    std::vector<int> order;                  // sorted position -> the caller's index
    std::vector<unsigned char> anchored;     // [n_nodes] host: the node holds a prior and is not constant (the covariance's gauge)
};

}  // namespace stba

using namespace stba;

struct stba_pg {
    int n = 0, m = 0;
    hipStream_t st = nullptr;
    bool own = false;
    DevBuf<double> poses[2];
    int cur = 0;
    DevBuf<int> ei, ej;
    DevBuf<double> meas, r, Ji, Jj, g, Minv, d, scale, x, rr, z, p, q, part_e, part_a, part_b, part_c, part_d;
    double* Hd = nullptr;               // (inside g)
    DevBuf<unsigned char> fixed;
    int nb_nodes = 1, nb_vec = 1, nb_edges = 1;
    // one rank: the edge ends (edge * 2 + side) of every node as a CSR, and the per-edge products u = (Ji^T t | Jj^T t) [12][m]
    DevBuf<int> node_start, end_code;
    DevBuf<double> u;
    // multi-GPU: this engine holds one shard of the EDGES, all nodes are replicated; the hook sums the
    // gradient | diagonal blocks, every matrix-vector product and the cost across ranks
    stba_allreduce_fn ar = nullptr;
    void* ar_user = nullptr;
    int rank = 0, world = 1;
    DevBuf<double> scalar;              // one device double for the cost sums
    // ---- coarse space of the two-level preconditioner (pg_engine.hip's header) and the device-side PCG control
    PgCoarsePlan coarse;                                 // its sizes (pg_plan.hpp); agg 0: none planned yet, -1: off
    DevBuf<int> end_node;                                // owner node of every edge end of the CSR
    DevBuf<double> AdP, Ac0, W, inv_work, rc_part, zc, part_cz, part_u, scal_dev, contrib, Dc;
    DevBuf<int> cflag;               // [0]: pivot flag of the coarse factorisation, [1]: coarse operators that failed (this solve)
    DevBuf<PgPcgState> state;
    MappedBuffer exp;                                    // the launch-path PCG's stamped block (PX_*)
    double fin_vals[8] = {0};                            // the host's validated copy of the last trial / linearisation block
    MappedBuffer fin;                                    // the trial / linearisation scalars' stamped block
    double seq = 0.0;
    int nb_nodes4 = 1;
    // ---- the PCG solve as one persistent kernel (pg_pcg_persistent_kernel)
    DevBuf<int> end_pos, end_rem;                        // CSR position of the edge end 2 e + side | remote node of the end at a CSR position
    DevBuf<double> Bend, ubuf, pbuf;
    DevBuf<int> ustamp, pstamp;
    int pp_base = 0;                                     // stamps only grow: the next solve starts behind the last one's
    bool bend_valid = false, pp_disabled = false;
    std::vector<int> node_start_host;                    // what the engine keeps of its PgEnds: node_start, for pg_plan_coarse
    bool coarse_valid = false;
    double coarse_radius = 0.0;
    PgCoarseJob job;                 // the second stream's inversion of the coarse operator, and the inverse(s) it leaves
    DevEvent ev_t[2];                // stba_lm_options::phase_timing: around the linear solve (created with the first timed solve)
    stba_pcg_summary last_pcg;
    // host copies of the graph for stba_pg_covariance's gauge check (pg_covariance.hip), which runs before any device work
    std::vector<int> h_ei, h_ej;
    std::vector<unsigned char> h_fixed;
    // per-edge square-root information W_e, component-major [36][m] like Ji (stba_pg_set_information / _sqrt_information); NULL: every
    // edge weighted by the identity, and pg_linearize launches the kernel without the whitening
    DevBuf<double> Winfo;
    // per-edge robust losses (stba_pg_set_loss): kind (STBA_LOSS_*), a, b, scale, each [m]; all NULL: no edge has a loss, and
    // pg_linearize launches a kernel without the corrector
    DevBuf<int> loss_kind;
    DevBuf<double> loss_a, loss_b, loss_scale;
    // node pose priors (n == 0: none).  part_cap: doubles in part_e and part_b, which grow with the priors' partial slots
    PgPriors pr;
    size_t part_cap = 0;
};

namespace stba {

// ---- stba_pg_solve's steps.  PgSolve is the state of ONE call; what outlives a call (the job's flags, bend_valid, coarse_valid,
// pp_base, pp_disabled, seq) stays in stba_pg.  No step captures anything; every launch is written once.
struct PgSolve {
    stba_lm_options opt;
    stba_pcg_options pcg;
    // derived once
    bool coarse = false, async_inv = false, build_on_st2 = false, multi = false, forcing = false, pp_ok = false, timing = false;
    int chunk = 1;
    // the loop
    TrustRegion region;
    double cost = 0.0, gmax = 0.0, g2 = 0.0, eta = 0.0;
    double last_rel_decrease = 1.0;      // of the last accepted step: (cost before - cost after) / cost before
    int iter = 0, jobs = 0, since_refresh = 0;
    bool scale_init = false;
    bool head_done = false;              // the preconditioner and the job's head of the NEXT iteration are already on their way
    stba_pcg_summary ps;
    PgSolve(const stba_lm_options& o, const stba_pcg_options& p) : opt(o), pcg(p), region(o) { memset(&ps, 0, sizeof ps); }
};

// the rest of a second-stream job, for whoever enqueues it: the buffer of the pair it writes, and whether its head is already out
struct PgJob { int wbuf = 0; bool head_was_done = false; };
// what pg_coarse_refresh leaves to the iteration: the inverse its PCG reads, and a job that is still to be enqueued
struct PgCoarseUse { const double* Ainv = nullptr; bool job_deferred = false; PgJob job; };

// what a setter resets that replaces an input of the linearisation (weights, losses): the edge-end blocks, the coarse inverse and
// the coarse matrix made from the last one are stale.  (pg_linearize and the solve's linearisation reset the same.)
inline void pg_invalidate_linearisation(stba_pg* g) { g->bend_valid = false; g->coarse_valid = false; g->job.ac0_valid = false; }

// ---- pg_engine.hip
// the all-reduce hook over `count` doubles at `buf`, on the engine's stream (one rank: nothing)
int pg_hook(stba_pg* g, double* buf, size_t count);

// ---- pg_linearize.hip
// residuals (and, with jac, Jacobians and the per-end contributions) at poses[which]; part_e gets the cost's partial sums -- the
// edges' in its first nb_edges slots, the priors' behind them (pg_cost_slots).  trial_x: the step of a trial point (jac == false): the
// priors' share of |J x|^2 goes into part_b behind the edge product's slots
int pg_linearize(stba_pg* g, int which, bool jac, const double* trial_x = nullptr);
// gradient | diagonal blocks of the last pg_linearize(jac), gathered per node, the priors' J'^T r' and J'^T J' included
void pg_gather_blocks(stba_pg* g);
// partial sums of a linearisation's cost in part_e (and of a trial point's |J x|^2 in part_b): the edge workgroups, then the priors'
inline int pg_cost_slots(const stba_pg* g) { return g->nb_edges + g->pr.nb; }

// ---- pg_prior.hip (an engine without priors: both return at once)
// W r, W J (jac) and the cost partials of the priors at `poses`, behind the edges' slots of part_e; trial_x as for pg_linearize
void pg_prior_linearize(stba_pg* g, const double* poses, bool jac, const double* trial_x);
// g += sum J'^T r', Hd += sum J'^T J' per prior-bearing node, right behind pg_gather_blocks_kernel; Hp keeps the blocks
void pg_prior_gather(stba_pg* g, bool accumulate);

// ---- pg_coarse.hip
int pg_setup_coarse(stba_pg* g, int group_opt);
void pg_offdiag_if_stale(stba_pg* g);
int pg_coarse_linearized(stba_pg* g, const PgSolve& sv);
int pg_wait_for_job_reads(stba_pg* g);
int pg_job_head(stba_pg* g);
int pg_job_rest(stba_pg* g, const PgSolve& sv, const PgJob& job);
int pg_coarse_refresh(stba_pg* g, PgSolve& sv, bool head_was_done, PgCoarseUse* use);

// ---- pg_pcg.hip
void pg_precond(stba_pg* g, PgSolve& sv);
// the edge kernel of the matrix-free product on v: u_e = J_e^T (J_e v), |J_e v|^2 summed per workgroup into part[2 b]
void pg_edge_product(stba_pg* g, const double* v, double* part, const PgPcgState* state);
bool pg_one_kernel_eligible(stba_pg* g, const PgSolve& sv);
int pg_pcg_by_launches(stba_pg* g, const PgSolve& sv, const double* Ainv_use, double eta_k);
int pg_pcg_one_kernel(stba_pg* g, const PgSolve& sv, const double* Ainv_use, double eta_k);

}  // namespace stba
