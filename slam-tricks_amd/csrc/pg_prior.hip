// pg_prior.hip -- node pose priors of the pose-graph engine: absolute knowledge of a node's pose -- a GPS / RTK fix, a
// surveyed start, a map-localisation fix, the prior a marginalised window leaves on its boundary node.
//
//   prior k:   node n_k, pose Z_k, square-root information W_k (6 x 6 row-major, tangent order [rho, theta])
//   residual   r_k = log(Z_k^-1 T_n)            -- pg_edge with T_i = I, the j side: the same log, the same short way round
//   Jacobian   J_k = d r_k / d delta_n = Jr^-1(r_k) = I + ad/2 + ad^2/12   (a constant node: 0, the prior adds to the cost only)
//   cost       += 1/2 |W_k r_k|^2, no robust loss
//
// A prior is block-diagonal in its node.  Whoever applies the matrix ASSEMBLED (the persistent PCG kernel, the block-Jacobi
// preconditioner, the coarse space, the covariance's block inverse) reads Hd and g, into which pg_prior_gather_kernel adds the priors'
// J'^T J' and J'^T r' right behind pg_gather_blocks_kernel; whoever is matrix-free over the EDGES (the launch-path PCG's product and
// p.q, the trial point's |J x|^2, the covariance's product) takes the summed block Hp[slot] or the per-prior J' from here.
// Two kernels, no atomics, fixed orders: two runs give the same bits.  This unit also holds the setter and the priors' entry points.
#include <cstring>
#include <vector>

#include "ba_factor_input.hpp"
#include "pg_device.hpp"
#include "pg_edge.hpp"
#include "pg_engine.hpp"

namespace stba {
namespace {

// One lane per prior (sorted by node).  with_jac: W r and W J are stored ([n][6], [n][36] row-major; J = 0 on a constant node), and
// part_cost[workgroup] gets the sum of |W r|^2.  Without: the cost alone -- the trial point -- and, with x, the priors' share of the
// model term: part_tt[2 workgroup] = sum |J' x_n|^2 with the J' the LAST linearisation stored (non-negative by construction).
__global__ __launch_bounds__(PG_PRIOR_NT) void pg_prior_linearize_kernel(int n_priors, const double* __restrict__ poses, const int* __restrict__ pnode,
                                                                         const double* __restrict__ ppose, const double* __restrict__ pW,
                                                                         const unsigned char* __restrict__ fixed, int with_jac,
                                                                         double* __restrict__ r, double* __restrict__ J,
                                                                         double* __restrict__ part_cost, const double* __restrict__ x,
                                                                         double* __restrict__ part_tt) {
    const int k = blockIdx.x * PG_PRIOR_NT + threadIdx.x;
    double c = 0.0, tt = 0.0;
    if (k < n_priors) {
        const int node = pnode[k];
        const double I7[7] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
        double T[7], Z[7], W[36], re[6], ji[36], jj[36];
        for (int q = 0; q < 7; ++q) { T[q] = poses[(size_t)node * 7 + q]; Z[q] = ppose[(size_t)k * 7 + q]; }
        for (int q = 0; q < 36; ++q) W[q] = pW[(size_t)k * 36 + q];
        pg_edge(I7, T, Z, re, with_jac ? ji : nullptr, jj);        // (ji: the virtual end's, not used)
        pg_whiten_cols(W, re, 1, 1);
        for (int q = 0; q < 6; ++q) c += re[q] * re[q];
        if (with_jac) {
            pg_whiten_cols(W, jj, 6, 6);
            const bool fx = fixed && fixed[node];
            for (int q = 0; q < 6; ++q) r[(size_t)k * 6 + q] = re[q];
            for (int q = 0; q < 36; ++q) J[(size_t)k * 36 + q] = fx ? 0.0 : jj[q];
        } else if (x) {
            double xl[6];
            for (int q = 0; q < 6; ++q) xl[q] = x[(size_t)node * 6 + q];
            for (int a = 0; a < 6; ++a) {
                double s = 0.0;
                for (int q = 0; q < 6; ++q) s += J[(size_t)k * 36 + a * 6 + q] * xl[q];
                tt += s * s;
            }
        }
    }
    double out2[2];
    block_sum2(c, tt, out2);
    if (threadIdx.x == 0) {
        part_cost[blockIdx.x] = out2[0];
        if (part_tt) { part_tt[blockIdx.x * 2] = out2[1]; part_tt[blockIdx.x * 2 + 1] = 0.0; }
    }
}

// Eight lanes per prior-bearing node (slot); lane k < 6 owns component k of the gradient and row k of the block.  The node's priors are
// summed serially in ascending (sorted) index: gk = sum_p (J'^T r')[k], row[b] = sum_p (J'^T J')[k][b] -- entry (k, b) and entry
// (b, k) are the same products in the same order, so the block is symmetric to the bit.  accumulate: g and Hd of the node gain the
// sums (the kernel runs right behind pg_gather_blocks_kernel, which wrote them); Hp[slot] keeps the block either way.
__global__ __launch_bounds__(PG_PRIOR_NODES_PER_WG * 8) void pg_prior_gather_kernel(int n_slots, const int* __restrict__ slot_node,
                                                                                    const int* __restrict__ slot_start, const double* __restrict__ r,
                                                                                    const double* __restrict__ J, int accumulate,
                                                                                    double* __restrict__ g, double* __restrict__ Hd,
                                                                                    double* __restrict__ Hp) {
    const int t = threadIdx.x, k = t & 7;
    const int slot = blockIdx.x * PG_PRIOR_NODES_PER_WG + (t >> 3);
    if (slot >= n_slots || k >= 6) return;
    double gk = 0.0, row[6] = {0, 0, 0, 0, 0, 0};
    const int p1 = slot_start[slot + 1];
    for (int p = slot_start[slot]; p < p1; ++p) {
        const double* Jp = J + (size_t)p * 36;
        const double* rp = r + (size_t)p * 6;
        double gs = 0.0, hs[6] = {0, 0, 0, 0, 0, 0};
        for (int a = 0; a < 6; ++a) {
            const double jak = Jp[a * 6 + k];
            gs += jak * rp[a];
            for (int b = 0; b < 6; ++b) hs[b] += jak * Jp[a * 6 + b];
        }
        gk += gs;
        for (int b = 0; b < 6; ++b) row[b] += hs[b];
    }
    for (int b = 0; b < 6; ++b) Hp[(size_t)slot * 36 + k * 6 + b] = row[b];
    if (accumulate) {
        const int node = slot_node[slot];
        g[(size_t)node * 6 + k] += gk;
        for (int b = 0; b < 6; ++b) Hd[(size_t)node * 36 + k * 6 + b] += row[b];
    }
}

}  // namespace

void pg_prior_linearize(stba_pg* g, const double* poses, bool jac, const double* trial_x) {
    const PgPriors& pr = g->pr;
    if (!pr.n) return;
    const bool trial = !jac && trial_x;
    hipLaunchKernelGGL(pg_prior_linearize_kernel, dim3(pr.nb), dim3(PG_PRIOR_NT), 0, g->st, pr.n, poses, pr.node.get(), pr.pose.get(), pr.W.get(),
                       g->fixed.get(), jac ? 1 : 0, pr.r.get(), pr.J.get(), g->part_e + g->nb_edges, trial ? trial_x : nullptr,
                       trial ? g->part_b + (size_t)2 * g->nb_edges : nullptr);
}

void pg_prior_gather(stba_pg* g, bool accumulate) {
    const PgPriors& pr = g->pr;
    if (!pr.n) return;
    hipLaunchKernelGGL(pg_prior_gather_kernel, dim3((pr.n_slots + PG_PRIOR_NODES_PER_WG - 1) / PG_PRIOR_NODES_PER_WG), dim3(PG_PRIOR_NODES_PER_WG * 8), 0,
                       g->st, pr.n_slots, pr.slot_node.get(), pr.slot_start.get(), pr.r.get(), pr.J.get(), accumulate ? 1 : 0, g->g.get(), g->Hd, pr.Hp.get());
}

}  // namespace stba

extern "C" {

// Everything is checked -- and, for the information form, factored -- on the host BEFORE anything is replaced (the checks and the
// double-double factorisation are the bundle adjustment's: ba_factor_input.hpp); the priors are grouped by node (a stable sort: inside a
// node the caller's order), uploaded into NEW arrays that are swapped in.  n == 0 releases them.
int stba_pg_set_priors(stba_pg* g, int n, const int* node, const double* pose, const double* information, const double* sqrt_information) {
    const std::string who = "stba_pg_set_priors";
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": null engine");
    if (n < 0) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": n is negative");
    if (information && sqrt_information) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": give information or sqrt_information, not both");
    PgPriors fresh;
    DevBuf<double> part_e_new, part_b_new;
    size_t cap_new = g->part_cap;
    if (n > 0) {
        if (!node || !pose) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": null node or pose array");
        if (g->ar || g->world > 1)
            return fail(STBA_ERR_INVALID_ARGUMENT, who + ": node pose priors are implemented for one rank only, and this engine has an all-reduce hook or communicator set");
        const size_t m = (size_t)n;
        std::vector<double> hp(m * 7), hw(m * 36);
        for (size_t k = 0; k < m; ++k) {
            std::string why;
            int rc = 0;
            if (node[k] < 0 || node[k] >= g->n) { why = "node index " + std::to_string(node[k]) + " out of range"; rc = STBA_ERR_INVALID_ARGUMENT; }
            if (!rc) rc = pose7_check_normalise(pose + k * 7, &hp[k * 7], "the pose", &why);
            if (!rc) rc = sqrt_information6(information ? information + k * 36 : nullptr, sqrt_information ? sqrt_information + k * 36 : nullptr, &hw[k * 36], &why);
            if (rc) return fail(rc, who + ": prior " + std::to_string(k) + ": " + why);
        }
        fresh.order.resize(m);
        for (size_t k = 0; k < m; ++k) fresh.order[k] = (int)k;
        std::vector<int> gptr, gnode;
        group_csr(m, [node](int k) { return node[k]; }, fresh.order, gptr, gnode);
        std::vector<int> snode(m), nslot((size_t)g->n, -1);
        std::vector<double> gp(m * 7), gw(m * 36);
        for (size_t p = 0; p < m; ++p) {
            const size_t k = (size_t)fresh.order[p];
            snode[p] = node[k];
            memcpy(&gp[p * 7], &hp[k * 7], 7 * sizeof(double));
            memcpy(&gw[p * 36], &hw[k * 36], 36 * sizeof(double));
        }
        fresh.anchored.assign((size_t)g->n, 0);
        for (size_t s = 0; s < gnode.size(); ++s) {
            nslot[(size_t)gnode[s]] = (int)s;
            fresh.anchored[(size_t)gnode[s]] = (g->h_fixed.empty() || !g->h_fixed[(size_t)gnode[s]]) ? 1 : 0;
        }
        fresh.n = n; fresh.n_slots = (int)gnode.size(); fresh.nb = (n + PG_PRIOR_NT - 1) / PG_PRIOR_NT;
        STBA_TRY(to_device(who, fresh.node, snode, g->st)); STBA_TRY(to_device(who, fresh.pose, gp, g->st)); STBA_TRY(to_device(who, fresh.W, gw, g->st));
        STBA_TRY(to_device(who, fresh.slot_node, gnode, g->st)); STBA_TRY(to_device(who, fresh.slot_start, gptr, g->st));
        STBA_TRY(to_device(who, fresh.node_slot, nslot, g->st));
        STBA_TRY(fresh.r.alloc(m * 6)); STBA_TRY(fresh.J.alloc(m * 36)); STBA_TRY(fresh.Hp.alloc((size_t)fresh.n_slots * 36));
        // the priors' partial sums sit behind the edges' in part_e (cost) and part_b (|J x|^2, two doubles per slot)
        const size_t need = (size_t)(g->nb_edges + fresh.nb) * 2 + 2;
        if (need > g->part_cap) { STBA_TRY(part_e_new.alloc(need)); STBA_TRY(part_b_new.alloc(need)); cap_new = need; }
        if (hipStreamSynchronize(g->st) != hipSuccess) return fail(STBA_ERR_HIP, who + ": upload failed");
    }
    // (nothing of the engine may still be reading the old priors or what was linearised with them: the moves below free them)
    STBA_HIP(hipStreamSynchronize(g->st));
    STBA_TRY(g->job.quiesce());
    g->pr = std::move(fresh);
    if (part_e_new) { g->part_e = std::move(part_e_new); g->part_b = std::move(part_b_new); g->part_cap = cap_new; }
    pg_invalidate_linearisation(g);
    return STBA_OK;
}

int stba_pg_prior_count(const stba_pg* g, int* n) {
    if (!g || !n) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_prior_count: null argument");
    *n = g->pr.n;
    return STBA_OK;
}

int stba_pg_prior_kernel_geometry(const stba_pg* g, int* priors_per_workgroup, int* nodes_per_workgroup) {
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_prior_kernel_geometry: null engine");
    if (priors_per_workgroup) *priors_per_workgroup = PG_PRIOR_NT;
    if (nodes_per_workgroup) *nodes_per_workgroup = PG_PRIOR_NODES_PER_WG;
    return STBA_OK;
}

// the whitened residuals and Jacobians of the priors at the current poses by the two kernels themselves (the second one without adding
// to g and Hd), in the caller's order; the cost from the first kernel's partial sums.  The engine's linearisation is left as it is:
// what the kernels overwrite (r', J', Hp at the same poses) gets the values it had
int stba_pg_evaluate_priors(stba_pg* g, double* cost, double* r, double* J) {
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_evaluate_priors: null engine");
    if (cost) *cost = 0.0;
    const PgPriors& pr = g->pr;
    if (!pr.n) return STBA_OK;
    const size_t m = (size_t)pr.n;
    pg_prior_linearize(g, g->poses[g->cur], true, nullptr);
    pg_prior_gather(g, false);
    STBA_HIP(hipGetLastError());
    std::vector<double> part((size_t)pr.nb), hr, hj;
    STBA_TRY(download(part.data(), g->part_e + g->nb_edges, part.size(), g->st));
    if (r) { hr.resize(m * 6); STBA_TRY(download(hr.data(), pr.r.get(), hr.size(), g->st)); }
    if (J) { hj.resize(m * 36); STBA_TRY(download(hj.data(), pr.J.get(), hj.size(), g->st)); }
    STBA_HIP(hipStreamSynchronize(g->st));
    double c2 = 0.0;
    for (double v : part) c2 += v;
    if (cost) *cost = 0.5 * c2;
    for (size_t p = 0; p < m; ++p) {
        const size_t k = (size_t)pr.order[p];
        if (r) memcpy(r + k * 6, &hr[p * 6], 6 * sizeof(double));
        if (J) memcpy(J + k * 36, &hj[p * 36], 36 * sizeof(double));
    }
    return STBA_OK;
}

}  // extern "C"
