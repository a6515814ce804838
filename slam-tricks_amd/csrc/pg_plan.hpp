// pg_plan.hpp -- the host decisions of the pose-graph engine (pg_engine.hip and its units) that fix what its kernels may assume: the layout
// constants and LDS sizes that host and kernels share, the check of the edges, the CSR of the edge ends, the sizes of the coarse
// space, whether the PCG solve may run as one kernel, the two policies of the solve loop (forcing sequence, lagged coarse inverse)
// and the gauge check of the covariance.  A function returns 0, or a status of include/stba.h with the reason in *why.
// Host only: the standard library and include/stba.h, nothing of HIP (tests/cpp/pg_plan_driver.cpp; the kernels include this header
// for the constants).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/stba.h"

namespace stba {

// ---------------------------------------------------------------- layout shared by the host and the kernels
constexpr int PG_NT = 1024;             // node kernels of the PCG: 1024 threads = 128 nodes x 8 lanes
constexpr int PG_NPW = PG_NT / 8;       // nodes per workgroup
// the PCG solve as ONE kernel (pg_pcg_persistent_kernel)
constexpr int PP_T = 512;            // threads of a group's workgroup (384 = 64 nodes x 6 components carry the vectors)
constexpr int PP_VCAP = 1536;        // edge ends of one group whose products fit the LDS buffer
constexpr int PP_NCMAX = 1536;       // coarse unknowns: three columns of the group's six inverse rows per thread
constexpr int PP_SLOT = 16;          // doubles per group in the all-gather block (9 used)
constexpr int PP_STAMP = 16;         // ints between two stamps (a 64-byte line each)
constexpr int PP_GROUPS_MAX = 256;   // groups, one workgroup each: the all-gather block and the stamps are allocated for this many
constexpr int PP_GROUP_NODES_MAX = 64;                      // nodes of a group: six components each in 384 of the PP_T threads
constexpr size_t PP_LDS_MAX = (size_t)160 * 1024 - 64;      // the dynamic LDS the persistent kernel is allowed (its attribute)
// the dynamic LDS of pg_pcg_persistent_kernel: rc, pts [nc] | gat [na][PP_SLOT] | ul, rl [384] | vbuf [PP_VCAP][6] | red [128] | 16
inline size_t pp_lds_bytes(int na, int nc) { return ((size_t)2 * nc + (size_t)na * PP_SLOT + 768 + (size_t)PP_VCAP * 6 + 128 + 16) * sizeof(double); }
// the dynamic LDS of pg_coarse_build_kernel: six coarse columns and the edge ends of the largest group; what a launch may ask for
// at the most (+ 20 KB static in the kernel)
constexpr size_t PG_COARSE_BUILD_LDS_MAX = 136 * 1024;
inline size_t pg_coarse_build_lds(int nc, int max_group_ends) { return (size_t)6 * nc * sizeof(double) + (size_t)4 * max_group_ends * sizeof(int); }

// ---------------------------------------------------------------- the edges
// the index of the first bad edge -- an end outside [0, n_nodes), or both ends at one node --, or -1
inline int pg_check_edges(int n_nodes, int n_edges, const int* ei, const int* ej) {
    for (int e = 0; e < n_edges; ++e)
        if (ei[e] < 0 || ei[e] >= n_nodes || ej[e] < 0 || ej[e] >= n_nodes || ei[e] == ej[e]) return e;
    return -1;
}

// The edge ENDS (2 * edge + side; side 0: the end at i, 1: at j) sorted by their node, as a CSR: node k owns the positions
// node_start[k] .. node_start[k + 1], in edge order (the sort is stable).
struct PgEnds {
    std::vector<int> node_start;       // [n + 1]
    std::vector<int> end_code;         // [2 m]  2 * edge + side at a position
    std::vector<int> end_node;         // [2 m]  the node that owns the position
    std::vector<int> end_pos;          // [2 m]  the position of end 2 * edge + side: the inverse of end_code
    std::vector<int> end_rem;          // [2 m]  the node at the other end of the position's edge
};
// (the edges have passed pg_check_edges)
inline void pg_build_ends(int n_nodes, int n_edges, const int* edge_i, const int* edge_j, PgEnds* out) {
    const size_t m = (size_t)n_edges;
    // edge ends sorted by node (counting sort; stable: a node's ends in edge order)
    std::vector<int> start((size_t)n_nodes + 1, 0), code(2 * m);
    for (int e = 0; e < n_edges; ++e) { ++start[(size_t)edge_i[e] + 1]; ++start[(size_t)edge_j[e] + 1]; }
    for (int i = 0; i < n_nodes; ++i) start[(size_t)i + 1] += start[(size_t)i];
    std::vector<int> fill(start.begin(), start.end() - 1), owner(2 * m), pos(2 * m), rem(2 * m);
    for (int e = 0; e < n_edges; ++e) {
        owner[(size_t)fill[(size_t)edge_i[e]]] = edge_i[e];
        rem[(size_t)fill[(size_t)edge_i[e]]] = edge_j[e];
        pos[(size_t)2 * e] = fill[(size_t)edge_i[e]];
        code[(size_t)fill[(size_t)edge_i[e]]++] = 2 * e;
        owner[(size_t)fill[(size_t)edge_j[e]]] = edge_j[e];
        rem[(size_t)fill[(size_t)edge_j[e]]] = edge_i[e];
        pos[(size_t)2 * e + 1] = fill[(size_t)edge_j[e]];
        code[(size_t)fill[(size_t)edge_j[e]]++] = 2 * e + 1;
    }
    out->node_start.swap(start); out->end_code.swap(code); out->end_node.swap(owner); out->end_pos.swap(pos); out->end_rem.swap(rem);
}

// ---------------------------------------------------------------- the coarse space of the two-level preconditioner
// six rigid-body modes per GROUP of `agg` consecutive nodes (the last group may be short)
struct PgCoarsePlan {
    int agg = 0;                       // nodes per group, a power of two >= 2; -1: no coarse space (the other members keep these defaults)
    int na = 0, nc = 0, np = 0;        // groups, coarse unknowns 6 na, padded to a multiple of 128
    int parts = 1;                     // workgroups of the node kernels per group
    int max_group_ends = 0;            // edge ends of the largest group
    size_t build_lds_bytes = 0;        // dynamic LDS of pg_coarse_build_kernel, <= PG_COARSE_BUILD_LDS_MAX
};
// group_opt: stba_pcg_options::coarse_group (0: automatic, -1: off).  node_start: PgEnds' [n + 1]
inline int pg_plan_coarse(int n, const std::vector<int>& node_start, int group_opt, PgCoarsePlan* plan, std::string* why) {
    *plan = PgCoarsePlan();
    int agg = group_opt;
    if (agg == 0) {            // auto: about 160 groups (C4: 64 nodes per group, 942 coarse unknowns), at least 8 nodes per group
        agg = 8;
        while ((n + agg - 1) / agg > 200) agg *= 2;
    }
    if (agg < 0) { plan->agg = -1; return 0; }
    if (agg < 2 || (agg & (agg - 1)) != 0) { *why = "stba_pg_solve: coarse_group must be a power of two >= 2 (0: automatic, -1: off)"; return STBA_ERR_INVALID_ARGUMENT; }
    const int na = (n + agg - 1) / agg, nc = 6 * na, np = ((nc + 127) / 128) * 128, parts = std::max(1, agg / PG_NPW);
    int max_ends = 0;
    for (int a = 0; a < na; ++a)
        max_ends = std::max(max_ends, node_start[(size_t)std::min(n, (a + 1) * agg)] - node_start[(size_t)std::min(n, a * agg)]);
    if (pg_coarse_build_lds(nc, max_ends) > PG_COARSE_BUILD_LDS_MAX) { *why = "stba_pg_solve: coarse space too large for this group size"; return STBA_ERR_INVALID_ARGUMENT; }
    plan->agg = agg; plan->na = na; plan->nc = nc; plan->np = np; plan->parts = parts; plan->max_group_ends = max_ends;
    plan->build_lds_bytes = pg_coarse_build_lds(nc, max_ends);
    return 0;
}

// what the device says of itself: compute units, and the LDS a workgroup may opt in to (bytes)
struct PgDeviceLimits { int cus; int lds_max_optin; };
// the PCG solve as one kernel: one rank, a coarse space whose groups fit a workgroup (<= 64 nodes, all their edge-end products
// in LDS) and are all resident at once (one per CU)
inline bool pg_one_kernel_fits(const PgCoarsePlan& c, int one_kernel_solve, bool several_ranks, PgDeviceLimits dev) {
    return one_kernel_solve != 0 && !several_ranks && c.agg > 0 && c.agg <= PP_GROUP_NODES_MAX && c.na <= PP_GROUPS_MAX && c.nc <= PP_NCMAX &&
           pp_lds_bytes(c.na, c.nc) <= PP_LDS_MAX && c.na <= dev.cus &&
           pp_lds_bytes(c.na, c.nc) <= (size_t)std::max(0, dev.lds_max_optin - 64) && c.max_group_ends <= PP_VCAP;
}

// ---------------------------------------------------------------- the two policies of the solve loop
// forcing sequence (Eisenstat & Walker, choice 2) behind an accepted step: eta_{k+1} = 0.9 (|g_{k+1}| / |g_k|)^2 with their
// safeguard, kept in [eta_min, eta0]; after a rejected step the gradient has not moved and eta stays
inline double pg_next_eta(const stba_pcg_options& pcg, const stba_lm_options& opt, double eta, double g2, double g2_new, double cost_change,
                          double new_cost) {
    if (!(pcg.forcing_eta0 > 0.0 && g2 > 0.0 && std::isfinite(g2_new))) return eta;
    double e2 = 0.9 * g2_new / g2;
    if (0.9 * eta * eta > 0.1) e2 = std::max(e2, 0.9 * eta * eta);
    eta = std::min(pcg.forcing_eta0, std::max(pcg.forcing_eta_min, e2));
    // (round 6) about to converge -- the step just taken changed the cost by less than 100 x the function tolerance: the
    // error of the LAST inexact step is what the converged poses keep (about eta x its length; on C4 the last step still
    // moves poses by 3.6e-3, and Eisenstat & Walker leave eta ~ 1e-2 there: 4e-5 in the poses, north_star asks for 1e-5)
    if (pcg.forcing_eta_final > 0.0 && cost_change <= 100.0 * opt.function_tolerance * (new_cost + cost_change))
        eta = std::max(pcg.forcing_eta_min, std::min(eta, pcg.forcing_eta_final));
    return eta;
}

// does this iteration's PCG wait for the inverse of its OWN operator (or take the one made an LM iteration earlier)?
// The first solve(s) wait (coarse_async = 2: not with a forcing sequence; coarse_async_after: how many LM iterations do -- the
// operator changes most in the first iterations) -- and every solve that follows a LONG step: the operator is stale by exactly the
// step that was just taken.  At C4 (profiles/r6_c4_async.txt) the steps of the first three iterations take 98 %, 97 % and 45 % off
// the cost, the later ones 1 % and less; preconditioning iteration 3 with iteration 2's operator ends 3.9e-5 from the exact-step
// poses, iterations 4 .. 9 with their predecessors' 2.9e-6 (in line: 2.5e-6).  Rule: lag only behind a step that took at most
// coarse_async_decrease (0.5) off the cost.
// (also measured, profiles/r6_c4_async_coarse_tolerance_behind_long_steps.txt: not waiting behind a long step either and
// giving THAT solve a tolerance on the coarse residual instead -- 3e-4 is what the poses need (2.4e-6), and then the extra
// PCG iterations cost more than the wait: 1323 against 1411 LM it/s)
inline bool pg_waits_for_own_inverse(const stba_pcg_options& pcg, bool forcing, int jobs, int iter, double last_rel_decrease) {
    const bool long_step = iter <= pcg.coarse_async_after || last_rel_decrease > pcg.coarse_async_decrease;
    return (jobs == 0 && (!forcing || pcg.coarse_async != 2)) || (pcg.coarse_async != 2 && long_step);
}

// ---------------------------------------------------------------- the gauge (pg_covariance.hip)
// union-find over the edges: the first connected component without a constant (or anchored) node.  true: every component has one.
// Otherwise *size and *first_node describe the offending component (the one whose smallest node index is smallest).
// fixed: [n], or null (no node is constant).  anchored: [n], or null: nodes that hold a pose prior and are not constant -- a component
// passes if it holds a constant node OR an anchored one
inline bool pg_gauge_fixed(int n, int m, const int* ei, const int* ej, const unsigned char* fixed, int* size, int* first_node,
                           const unsigned char* anchored = nullptr) {
    std::vector<int> parent((size_t)n);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int a) { while (parent[(size_t)a] != a) { parent[(size_t)a] = parent[(size_t)parent[(size_t)a]]; a = parent[(size_t)a]; } return a; };
    for (int e = 0; e < m; ++e) {
        const int a = find(ei[e]), b = find(ej[e]);
        if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);      // (the root is the component's smallest node)
    }
    std::vector<int> count((size_t)n, 0);
    std::vector<unsigned char> has((size_t)n, 0);
    for (int k = 0; k < n; ++k) { const int r = find(k); ++count[(size_t)r]; if ((fixed && fixed[k]) || (anchored && anchored[k])) has[(size_t)r] = 1; }
    for (int k = 0; k < n; ++k)
        if (find(k) == k && !has[(size_t)k]) { *size = count[(size_t)k]; *first_node = k; return false; }
    return true;
}

}  // namespace stba
