// pg_pcg.hip -- the preconditioned conjugate gradient on the damped normal equations of the pose graph (J^T J + D) x = -g, in its
// two forms: by launches (three or four kernels per iteration, stopped on the device, watched by the host through a stamped block;
// the only form for several ranks) and as ONE persistent kernel (one rank, all groups resident).  Holds the block-Jacobi
// preconditioner kernel, the kernels of the launch path, the persistent kernel with its argument block and exchange helpers, and the
// host code that launches them.  The method and the preconditioner: pg_engine.hip's header.
// Node pose priors (pg_prior.hip) are block-diagonal: the persistent kernel applies the matrix ASSEMBLED -- Hd, which holds them, plus d
// and the edge ends' off-diagonal blocks -- and needs nothing; the launch path is matrix-free over the edges and takes the priors'
// summed blocks Hp in the PRIOR instantiations of its two node kernels.
// (PG_NT = 1024 threads = PG_NPW = 128 nodes x 8 lanes: pg_plan.hpp)
#include <algorithm>
#include <atomic>
#include <climits>

#include "pg_device.hpp"
#include "pg_engine.hpp"

namespace stba {
namespace {

// LM diagonal + block-Jacobi preconditioner M_i = (Hd_i + diag(d_i))^-1 (6x6 Gauss-Jordan on an SPD block)
__global__ __launch_bounds__(256) void pg_precond_kernel(int n_nodes, const double* __restrict__ Hd, double* __restrict__ scale,
                                                         int init_scale, int use_scaling, double radius, double dmin, double dmax,
                                                         const unsigned char* __restrict__ fixed, double* __restrict__ d,
                                                         double* __restrict__ Minv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_nodes) return;
    double A[36], B[36];
    for (int k = 0; k < 36; ++k) { A[k] = Hd[(size_t)i * 36 + k]; B[k] = 0.0; }
    const bool fx = fixed && fixed[i];
    for (int a = 0; a < 6; ++a) {
        const double h = A[a * 7];
        double s = 1.0;
        if (use_scaling) { if (init_scale) { s = 1.0 / (1.0 + sqrt(h)); scale[(size_t)i * 6 + a] = s; } else s = scale[(size_t)i * 6 + a]; }
        else if (init_scale) scale[(size_t)i * 6 + a] = 1.0;
        const double s2 = s * s;
        const double dv = fmin(fmax(h * s2, dmin), dmax) / radius / s2;
        d[(size_t)i * 6 + a] = dv;
        A[a * 7] += dv;
        B[a * 7] = 1.0;
    }
    if (fx) { for (int k = 0; k < 36; ++k) Minv[(size_t)i * 36 + k] = 0.0; return; }
    for (int c = 0; c < 6; ++c) {          // Gauss-Jordan without pivoting (SPD + damping)
        const double inv = 1.0 / A[c * 7];
        for (int k = 0; k < 6; ++k) { A[c * 6 + k] *= inv; B[c * 6 + k] *= inv; }
        for (int rr = 0; rr < 6; ++rr) {
            if (rr == c) continue;
            const double f = A[rr * 6 + c];
            for (int k = 0; k < 6; ++k) { A[rr * 6 + k] -= f * A[c * 6 + k]; B[rr * 6 + k] -= f * B[c * 6 + k]; }
        }
    }
    for (int k = 0; k < 36; ++k) Minv[(size_t)i * 36 + k] = B[k];
}

// q = D p   (then the edge kernel adds J^T J p)
__global__ __launch_bounds__(256) void pg_diag_mul_kernel(int n, const double* __restrict__ d, const double* __restrict__ p,
                                                          double* __restrict__ q, int use_d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) q[i] = use_d ? d[i] * p[i] : 0.0;
}

__global__ __launch_bounds__(256) void pg_matvec_kernel(int n_edges, const int* __restrict__ ei, const int* __restrict__ ej,
                                                        const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                        const double* __restrict__ p, double* __restrict__ q) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    const int i = ei[e], j = ej[e];
    double A[36], B[36];
    for (int k = 0; k < 36; ++k) { A[k] = Ji[(size_t)k * n_edges + e]; B[k] = Jj[(size_t)k * n_edges + e]; }
    double pi[6], pj[6], t[6];
    for (int k = 0; k < 6; ++k) { pi[k] = p[(size_t)i * 6 + k]; pj[k] = p[(size_t)j * 6 + k]; }
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += A[a * 6 + k] * pi[k] + B[a * 6 + k] * pj[k];
        t[a] = s;
    }
    for (int k = 0; k < 6; ++k) {
        double si = 0.0, sj = 0.0;
        for (int a = 0; a < 6; ++a) { si += A[a * 6 + k] * t[a]; sj += B[a * 6 + k] * t[a]; }
        if (si != 0.0) unsafeAtomicAdd(&q[(size_t)i * 6 + k], si);
        if (sj != 0.0) unsafeAtomicAdd(&q[(size_t)j * 6 + k], sj);
    }
}

// partial[b] = {dot(a, b2), dot(a, a)}
__global__ __launch_bounds__(256) void pg_dot_kernel(int n, const double* __restrict__ a, const double* __restrict__ b2,
                                                     double* __restrict__ partial) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double x = 0.0, y = 0.0;
    if (i < n) { x = a[i] * b2[i]; y = a[i] * a[i]; }
    double out2[2];
    block_sum2(x, y, out2);
    if (threadIdx.x == 0) { partial[blockIdx.x * 2] = out2[0]; partial[blockIdx.x * 2 + 1] = out2[1]; }
}

// ---------------------------------------------------------------- one rank: a PCG iteration in THREE launches, no atomics
// (1) p^T q = p^T D p + |J p|^2 = sum_i d_i p_i^2 + sum_e |t_e|^2 with t_e = J_e [p_i; p_j]: the dot product needs no pass over
//     the finished q -- the edge kernel adds up |t_e|^2, the kernel that makes the direction p adds up d p^2.
// (2) q is never scattered: the edge kernel stores u_e = (Ji^T t_e | Jj^T t_e), 12 doubles per edge, component-major, and the
//     node kernel GATHERS q_i = d_i p_i + sum over the node's edge ends of u (a CSR of the ends built at create time) while it
//     updates x, r, z.  The scatter with FP64 atomics was the bound of the product: 480 k device-scope atomics per product
//     retire at ~20 G/s whatever the access pattern -- the product scaled linearly with the edge count at 1.65 G edges/s
//     (24.7 us at 40 k edges, 95 us at 160 k, 387 us at 640 k).  Measured on the way: one lane per edge END with a segmented
//     scan over a node's lanes and 6 atomics per node instead of 12 per edge (21.1 against 23.8 us: fewer atomics, but every
//     edge read twice and no coalescing); the whole loop as ONE persistent kernel with four grid barriers per iteration
//     (correct, 59 us per iteration against 40 us for the launches: a barrier across eight XCDs costs more than a kernel
//     boundary).
//     (Also measured: the direction p = z + beta p_old formed on the fly by the edge kernel and again by the node kernel, the
//     node term of the dot product added up by the edge ends -- TWO launches per iteration: 32 us against 30 us for three.
//     Every kernel that needs a scalar of the loop adds up its partial sums first, ~2 us each; two kernels that need three
//     each lose more than the launch they save.)
__global__ __launch_bounds__(256) void pg_edge_product_kernel(int n_edges, const int* __restrict__ ei, const int* __restrict__ ej,
                                                              const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                              const double* __restrict__ p, double* __restrict__ u,
                                                              double* __restrict__ part_tt, const PgPcgState* __restrict__ state) {
    if (state && state->done) return;          // (the solve has converged: see pg_pcg_dir4_kernel)
    const int e = blockIdx.x * 256 + threadIdx.x;
    double tt2 = 0.0;
    if (e < n_edges) {
        const int i = ei[e], j = ej[e];
        double A[36], B[36];
        for (int k = 0; k < 36; ++k) { A[k] = Ji[(size_t)k * n_edges + e]; B[k] = Jj[(size_t)k * n_edges + e]; }
        double pi[6], pj[6], t[6];
        for (int k = 0; k < 6; ++k) { pi[k] = p[(size_t)i * 6 + k]; pj[k] = p[(size_t)j * 6 + k]; }
        for (int a = 0; a < 6; ++a) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += A[a * 6 + k] * pi[k] + B[a * 6 + k] * pj[k];
            t[a] = s;
            tt2 += s * s;
        }
        // u edge-major, 12 doubles per edge (i-side | j-side): the node kernel's gather then reads 48 contiguous bytes per edge end
        // (component-major u -- better for these stores -- made it six scattered 8-byte loads per end: 14 us for the node kernel)
        double ue[12];
        for (int k = 0; k < 6; ++k) {
            double si = 0.0, sj = 0.0;
            for (int a = 0; a < 6; ++a) { si += A[a * 6 + k] * t[a]; sj += B[a * 6 + k] * t[a]; }
            ue[k] = si; ue[6 + k] = sj;
        }
        double2* dst = reinterpret_cast<double2*>(u + (size_t)e * 12);
        for (int k = 0; k < 6; ++k) dst[k] = make_double2(ue[2 * k], ue[2 * k + 1]);
    }
    double out2[2];
    block_sum2(tt2, 0.0, out2);
    if (threadIdx.x == 0) { part_tt[blockIdx.x * 2] = out2[0]; part_tt[blockIdx.x * 2 + 1] = 0.0; }
}

// restriction of a workgroup's 128 nodes: w[node][u] = (P_node^T r_node)[u] sits in LDS; the groups that END in this
// workgroup's range are summed serially in node order (fixed order: same bits everywhere).  Groups of up to 128 nodes lie
// inside one workgroup (128 % agg == 0); larger ones (agg = 256, 512, ...) span agg / 128 workgroups, each of which writes
// its own partial row of rc_part -- the coarse kernel adds the parts in order.
__device__ inline void pg_restrict_store(const double (*wsm)[6], int n, int agg, int node0, double* __restrict__ rc_part) {
    const int t = threadIdx.x;
    if (agg <= PG_NPW) {
        const int ng = PG_NPW / agg;
        if (t < 6 * ng) {
            const int gl = t / 6, u = t % 6;
            const int kb = gl * agg;
            if (node0 + kb < n) {
                double s = 0.0;
                for (int k = 0; k < agg && node0 + kb + k < n; ++k) s += wsm[kb + k][u];
                rc_part[(size_t)((node0 + kb) / agg) * 6 + u] = s;
            }
        }
    } else if (t < 6) {
        double s = 0.0;
        for (int k = 0; k < PG_NPW && node0 + k < n; ++k) s += wsm[k][t];
        rc_part[(size_t)(node0 / PG_NPW) * 6 + t] = s;
    }
}

// PCG start: r = -g, x = 0, z0 = Minv r (into z), restriction of r; partial -> {r.z0, r.r}
__global__ __launch_bounds__(PG_NT) void pg_pcg_init4_kernel(int n, int agg, const double* __restrict__ g, const double* __restrict__ Minv,
                                                            const double* __restrict__ AdP, double* __restrict__ x, double* __restrict__ r,
                                                            double* __restrict__ z, double* __restrict__ rc_part, double* __restrict__ part) {
    __shared__ double wsm[PG_NPW][6];
    const int t = threadIdx.x, nl = t >> 3, k = t & 7;
    const int node0 = blockIdx.x * PG_NPW, node = node0 + nl;
    double a = 0.0, b = 0.0;
    if (node < n && k < 6) {
        double rl[6];
        for (int q = 0; q < 6; ++q) rl[q] = -g[(size_t)node * 6 + q];
        double z0 = 0.0, w = 0.0;
        for (int q = 0; q < 6; ++q) { z0 += Minv[(size_t)node * 36 + k * 6 + q] * rl[q]; if (AdP) w += AdP[(size_t)node * 36 + q * 6 + k] * rl[q]; }
        r[(size_t)node * 6 + k] = rl[k]; x[(size_t)node * 6 + k] = 0.0; z[(size_t)node * 6 + k] = z0;
        wsm[nl][k] = w;
        a = rl[k] * z0; b = rl[k] * rl[k];
    }
    __syncthreads();
    if (AdP) pg_restrict_store(wsm, n, agg, node0, rc_part);
    double out2[2];
    block_sum2_n<PG_NT>(a, b, out2);
    if (t == 0) { part[blockIdx.x * 2] = out2[0]; part[blockIdx.x * 2 + 1] = out2[1]; }
}

// one PCG step on the nodes: q (GATHERED from the edge kernel's u on one rank, read from the all-reduced product with several),
// alpha = rz / p.q, x += alpha p, r -= alpha q, z0 = Minv r, restriction; partial -> {r.z0, r.r}.  Eight lanes per node: lane j takes
// the node's edge ends j, j + 8, ... (all loads of the gather in flight at once -- one lane per node walking its ends was a
// chain of dependent round trips, 19 us for 10 000 nodes in round 3), the six components are summed over the lanes with a
// butterfly, lanes 0..5 then own one component each.
// PRIOR = false: the engine holds no node pose priors -- the kernel as it was before there were any; node_slot and Hp are not read.
// PRIOR = true (one rank, GATHER): q = (J^T J + D + Hp) p -- a node with a slot adds Hp_i p_i, Hp_i the summed J'^T J' of its priors
// (pg_prior.hip); lane k holds row k of the block, the lanes of a node exchange p through shuffles.  Two instantiations and not a
// runtime branch, as INFO / ROBUST in pg_linearize_kernel: an engine without priors runs the instruction stream it ran before.
template <bool GATHER, bool PRIOR = false>
__global__ __launch_bounds__(PG_NT) void pg_pcg_update4_kernel(int n, int m, int agg, int slot, const PgPcgState* __restrict__ state,
                                                              int nb_a, const double* __restrict__ part_a, int nb_b,
                                                              const double* __restrict__ part_b, const double* __restrict__ Minv,
                                                              const double* __restrict__ AdP, const double* __restrict__ d,
                                                              const int* __restrict__ node_start, const int* __restrict__ end_code,
                                                              const double* __restrict__ u, const double* __restrict__ qin,
                                                              const double* __restrict__ p, double* __restrict__ x, double* __restrict__ r,
                                                              double* __restrict__ z, double* __restrict__ rc_part, double* __restrict__ part_out,
                                                              const int* __restrict__ node_slot, const double* __restrict__ Hp) {
    __shared__ double wsm[PG_NPW][6];
    __shared__ double s_red[2][PG_NT / 64];
    const int t = threadIdx.x, nl = t >> 3, k = t & 7;
    const int node0 = blockIdx.x * PG_NPW, node = node0 + nl;
    // Everything that does not depend on alpha is REQUESTED first, in one go: the kernel is a chain of memory round trips
    // (~1 us each on a machine this empty), and in program order -- state, partial sums, CSR, edge products, vectors, blocks --
    // it took 14 us for 10 000 nodes.  The `done` flag is looked at only after the requests are out.
    const int done = state->done;
    const double rz = state->rz[slot];
    double pa = 0.0, pb = 0.0;
    for (int q = t; q < nb_a; q += PG_NT) pa += part_a[q * 2];
    if (part_b) for (int q = t; q < nb_b; q += PG_NT) pb += part_b[q * 2];
    double ql[6] = {0, 0, 0, 0, 0, 0};
    double pk = 0.0, rk = 0.0, dk = 0.0, xk = 0.0, mrow[6] = {0, 0, 0, 0, 0, 0}, pcol[6] = {0, 0, 0, 0, 0, 0};
    const bool act = node < n && k < 6;
    const size_t o = (size_t)node * 6 + k;
    if (act) {
        pk = p[o]; rk = r[o]; xk = x[o];
        if (GATHER) dk = d[o]; else dk = qin[o];
        for (int q = 0; q < 6; ++q) mrow[q] = Minv[(size_t)node * 36 + k * 6 + q];
        if (AdP) for (int q = 0; q < 6; ++q) pcol[q] = AdP[(size_t)node * 36 + q * 6 + k];
    }
    double hprow[6] = {0, 0, 0, 0, 0, 0};
    if (PRIOR && act) {
        const int sl = node_slot[node];
        if (sl >= 0) for (int q = 0; q < 6; ++q) hprow[q] = Hp[(size_t)sl * 36 + k * 6 + q];
    }
    if (GATHER && node < n) {
        const int e1 = node_start[node + 1];
        for (int c = node_start[node] + k; c < e1; c += 8) {
            const int code = end_code[c];                              // = 2 e + side: the end's six doubles start at u + 6 code
            const double2* ue = reinterpret_cast<const double2*>(u + (size_t)code * 6);
            const double2 a0 = ue[0], a1 = ue[1], a2 = ue[2];
            ql[0] += a0.x; ql[1] += a0.y; ql[2] += a1.x; ql[3] += a1.y; ql[4] += a2.x; ql[5] += a2.y;
        }
    }
    if (done) return;
    // p.q: one rank: sum |t_e|^2 (edge kernel) + sum d p^2 (direction kernel); several: the dot-product kernel's partials.
    // Fixed order: every workgroup (and every rank) gets the same bits.
    for (int off = 32; off > 0; off >>= 1) { pa += __shfl_down(pa, off, 64); pb += __shfl_down(pb, off, 64); }
    if ((t & 63) == 0) { s_red[0][t >> 6] = pa; s_red[1][t >> 6] = pb; }
    __syncthreads();
    double pq = 0.0, pq2 = 0.0;
    for (int w = 0; w < PG_NT / 64; ++w) { pq += s_red[0][w]; pq2 += s_red[1][w]; }
    pq += pq2;
    const double alpha = (pq > 0.0) ? rz / pq : 0.0;
    if (GATHER) {
        for (int q = 0; q < 6; ++q) {
            ql[q] += __shfl_xor(ql[q], 1, 8);
            ql[q] += __shfl_xor(ql[q], 2, 8);
            ql[q] += __shfl_xor(ql[q], 4, 8);
        }
    }
    double hp_p = 0.0;                   // (Hp_i p_i)[k]; a node without a slot has a zero row
    if (PRIOR) for (int q = 0; q < 6; ++q) hp_p += hprow[q] * __shfl(pk, q, 8);
    if (act) {
        double qk;
        if (GATHER) {
            qk = ql[0];
            if (k == 1) qk = ql[1]; else if (k == 2) qk = ql[2]; else if (k == 3) qk = ql[3]; else if (k == 4) qk = ql[4]; else if (k == 5) qk = ql[5];
            qk += dk * pk;
            if (PRIOR) qk += hp_p;
        } else qk = dk;
        x[o] = xk + alpha * pk;
        rk = rk - alpha * qk;
        r[o] = rk;
    } else rk = 0.0;
    double rl[6];
    for (int q = 0; q < 6; ++q) rl[q] = __shfl(rk, q, 8);
    double a = 0.0, b = 0.0;
    if (act) {
        double z0 = 0.0, w = 0.0;
        for (int q = 0; q < 6; ++q) { z0 += mrow[q] * rl[q]; w += pcol[q] * rl[q]; }
        z[o] = z0;
        wsm[nl][k] = w;
        a = rk * z0; b = rk * rk;
    }
    __syncthreads();
    if (AdP) pg_restrict_store(wsm, n, agg, node0, rc_part);
    double out2[2];
    block_sum2_n<PG_NT>(a, b, out2);
    if (t == 0) { part_out[blockIdx.x * 2] = out2[0]; part_out[blockIdx.x * 2 + 1] = out2[1]; }
}

// coarse correction: zc = Ainv rc (one wave per row; rc = the parts of its group added in order); partial -> rc.zc
__global__ __launch_bounds__(256) void pg_coarse_solve_kernel(int nc, int parts, const PgPcgState* __restrict__ state, const double* __restrict__ Ainv,
                                                              const double* __restrict__ rc_part, double* __restrict__ zc,
                                                              double* __restrict__ part_cz) {
    __shared__ double sw[4];
    const int done = state ? state->done : 0;           // (looked at below, behind the row's first loads)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + w;
    auto rc = [&](int c) {
        const int a = c / 6, u = c % 6;
        double s = 0.0;
        for (int j = 0; j < parts; ++j) s += rc_part[(size_t)(a * parts + j) * 6 + u];
        return s;
    };
    double acc = 0.0;
    if (row < nc)
        for (int c = lane; c < nc; c += 64) acc += Ainv[(size_t)row * nc + c] * rc(c);
    if (done) return;
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) {
        double prod = 0.0;
        if (row < nc) { zc[row] = acc; prod = rc(row) * acc; }
        sw[w] = prod;
    }
    __syncthreads();
    if (threadIdx.x == 0) { part_cz[blockIdx.x * 2] = (sw[0] + sw[1]) + (sw[2] + sw[3]); part_cz[blockIdx.x * 2 + 1] = 0.0; }
}

// z = z0 + P zc; rz_new = sum r.z0 + rc.zc; beta = rz_new / rz_old (first: p = z); p = z + beta p; partial -> sum d p^2.
// Workgroup 0 also keeps the books of the solve: rz for the next iteration, the iteration count, and the STOPPING TEST
// |r|^2 <= eta^2 |b|^2 (or the iteration cap) -- once `done` is set every later kernel of the solve returns at once, so the
// host can enqueue iterations ahead of what it knows (it polls the exported block in mapped memory).
// PRIOR (as in pg_pcg_update4_kernel): the partial gains p_i^T Hp_i p_i of the nodes that hold pose priors -- p.q = sum |t_e|^2 +
// sum d p^2 + sum p^T Hp p.
template <bool PRIOR = false>
__global__ __launch_bounds__(PG_NT) void pg_pcg_dir4_kernel(int n, int agg, int slot, int first, double eta, int max_iters, PgPcgState* __restrict__ state,
                                                           double* __restrict__ exp_, int nb_rz, const double* __restrict__ part_rz, int nb_cz,
                                                           const double* __restrict__ part_cz, const double* __restrict__ AdP,
                                                           const double* __restrict__ zc, const double* __restrict__ z, const double* __restrict__ d,
                                                           double* __restrict__ p, double* __restrict__ part_dp,
                                                           const int* __restrict__ node_slot, const double* __restrict__ Hp) {
    __shared__ double s_red[3][PG_NT / 64];
    const int t = threadIdx.x;
    // (as in the update kernel: every load that does not depend on beta is requested before anything is waited for)
    const int was_done = first ? 0 : state->done;
    const double rzo = first ? 1.0 : state->rz[slot];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int q = t; q < nb_rz; q += PG_NT) { s0 += part_rz[q * 2]; s2 += part_rz[q * 2 + 1]; }
    if (part_cz) for (int q = t; q < nb_cz; q += PG_NT) s1 += part_cz[q * 2];
    const int nl = t >> 3, k = t & 7;
    const int node = blockIdx.x * PG_NPW + nl;
    const bool act = node < n && k < 6;
    const size_t o = (size_t)node * 6 + k;
    double zk = 0.0, pold = 0.0, dk = 0.0;
    if (act) {
        zk = z[o]; dk = d[o];
        if (!first) pold = p[o];
        if (AdP) {
            const int a = node / agg;
            for (int q = 0; q < 6; ++q) zk += AdP[(size_t)node * 36 + k * 6 + q] * zc[(size_t)a * 6 + q];
        }
    }
    double hprow[6] = {0, 0, 0, 0, 0, 0};
    if (PRIOR && act) {
        const int sl = node_slot[node];
        if (sl >= 0) for (int q = 0; q < 6; ++q) hprow[q] = Hp[(size_t)sl * 36 + k * 6 + q];
    }
    if (was_done) {
        if (blockIdx.x == 0 && t == 0) {
            const int tk = state->ticks + 1;
            state->ticks = tk;
            if (exp_) {        // (the same block again under the new tick)
                const double px[PX_COUNT] = {state->rr0, state->rr, (double)state->iters, (double)state->done, (double)state->hit_cap};
                stamped_store_thread(exp_, px, PX_COUNT, (double)tk);
            }
        }
        return;
    }
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_down(s0, off, 64); s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
    if ((t & 63) == 0) { s_red[0][t >> 6] = s0; s_red[1][t >> 6] = s1; s_red[2][t >> 6] = s2; }
    __syncthreads();
    double rzn = 0.0, rcz = 0.0, rr = 0.0;
    for (int w = 0; w < PG_NT / 64; ++w) { rzn += s_red[0][w]; rcz += s_red[1][w]; rr += s_red[2][w]; }
    rzn += rcz;
    const double beta = first ? 0.0 : ((rzo > 0.0) ? rzn / rzo : 0.0);
    double dp2 = 0.0;
    if (!PRIOR) {
        if (act) {
            const double pv = first ? zk : zk + beta * pold;
            p[o] = pv;
            dp2 = dk * pv * pv;
        }
    } else {
        // (every lane takes part in the shuffles; the lanes that carry no component hold a zero)
        const double pv = act ? (first ? zk : zk + beta * pold) : 0.0;
        double hp_p = 0.0;
        for (int q = 0; q < 6; ++q) hp_p += hprow[q] * __shfl(pv, q, 8);
        if (act) {
            p[o] = pv;
            dp2 = dk * pv * pv + pv * hp_p;
        }
    }
    double out2[2];
    block_sum2_n<PG_NT>(dp2, 0.0, out2);
    if (t == 0) { part_dp[blockIdx.x * 2] = out2[0]; part_dp[blockIdx.x * 2 + 1] = 0.0; }
    if (blockIdx.x == 0 && t == 0) {
        int iters, done, cap = 0, tk;
        double rr0, tol2;
        if (first) {
            rr0 = rr; tol2 = eta * eta * rr0; iters = 0; tk = 1;
            done = !(rr0 > 0.0) || !isfinite(rr0) || !isfinite(rzn);
        } else {
            rr0 = state->rr0; tol2 = state->tol2; iters = state->iters + 1; tk = state->ticks + 1;
            done = !(rr > tol2);                              // (also ends the solve on a NaN)
            if (!done && iters >= max_iters) { done = 1; cap = 1; }
        }
        state->rz[slot ^ 1] = rzn;
        state->rr0 = rr0; state->tol2 = tol2; state->rr = rr; state->iters = iters; state->done = done; state->hit_cap = cap; state->ticks = tk;
        if (exp_) {
            const double px[PX_COUNT] = {rr0, rr, (double)iters, (double)done, (double)cap};
            stamped_store_thread(exp_, px, PX_COUNT, (double)tk);
        }
    }
}

// ================================================================= the PCG solve of an LM iteration as ONE kernel
// Four launches per PCG iteration cost ~44 us for ~34 us of kernels (C4), every kernel a chain of three memory round trips on an
// empty machine.  Round 3's persistent loop (four grid BARRIERS per iteration, 59 us) was slower still; what a barrier costs is not
// the exchange but the counter: arrive, wait for the count, then fetch the data.  Here nothing is counted.  One workgroup per
// GROUP of the coarse space (<= 64 nodes, <= 256 groups: all resident, one per CU) keeps its nodes' x, r, p, s, u, w and its six rows
// of the coarse inverse in REGISTERS for the whole solve, and an iteration has two exchanges, each a block of data with a STAMP
// behind it (agent-scope write-through stores, agent-scope loads: no fence, no cache invalidate):
//   A  the group's slice of u = M^-1 r; an edge end waits for the stamp of the ONE group that owns its remote node, reads 48 bytes;
//   B  nine doubles per group -- the partial sums of (r, u), (w, u), (r, r) and the group's six entries of P^T w -- which every
//      group reads from every group: an all-gather of 157 x 72 bytes at C4.
// Two exchanges suffice because the iteration is the Chronopoulos-Gear form of PCG (w = A u instead of q = A p; p and s = A p by
// recurrence; both dot products of a step in ONE reduction), and because the coarse residual is carried by recurrence, replicated
// in every group: r_c <- r_c - alpha P^T s, P^T s = P^T w + beta P^T s -- so the restriction never needs a gather of its own.
// Measured skeleton (tools/exp/pcg_skeleton.hip, no arithmetic): 6.0 us per iteration (A 2.6, B 3.8).
// The matrix is applied ASSEMBLED: (H_ii + D_i) u_i from the diagonal blocks the linearisation leaves, plus one 6 x 6 block
// B_e = Ji^T Jj per edge END (its transpose for the other end), written once per linearisation in the order the groups read
// them (pg_offdiag_kernel), 36 coalesced loads per end and iteration out of the XCD's L2.
// Several ranks (edge shards) keep the launch-per-kernel path: their product needs a cross-rank sum in every iteration.
// (PP_T, PP_VCAP, PP_NCMAX, PP_SLOT, PP_STAMP and pp_lds_bytes, the layout the host sizes and this kernel indexes: pg_plan.hpp)

struct PpArgs {
    int n, agg, log2agg, na, nc, base, max_iters;
    double eta;
    const int *node_start, *end_rem;
    const double *Bend, *Hd, *d, *Minv, *AdP, *Ainv, *g;
    double *x, *ubuf, *pbuf;
    int *ustamp, *pstamp;
    PgPcgState* state;
    long long spin_limit; // how long a workgroup waits for a stamp, in ticks of wall_clock64 (100 MHz); 0: not at all (the test of the way back)
    double eta_c;         // tolerance on |P^T r| / |P^T r_0| in the stopping test (<= 0: none)
    int fences;           // 1: the stamps are published behind a RELEASE fence and read in front of an ACQUIRE fence (agent scope); 0: compiler barriers only
    long long* tdbg;      // debug builds: time per phase (group 0), else null
};

__device__ __forceinline__ int pp_ld_i(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double pp_ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pp_st(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// THE MEMORY ORDER OF THE TWO EXCHANGES.  Producer: data with agent-scope stores (write-through), s_waitcnt
// vmcnt(0) -- every store acknowledged --, workgroup barrier, then the stamp.  Consumer: polls the stamp, then loads the data with
// agent-scope loads (never from the L1).  What the hardware orders by itself (a load is ISSUED after the poll's branch has seen the
// stamp; stores are acknowledged before the stamp is issued) the COMPILER must not undo: both sides carry a compiler barrier.
// With PpArgs::fences the stamp is also stored behind an agent-scope release fence and the data loaded behind an acquire fence --
// the formally complete protocol; measured against the barrier-only form in tools/dbg/c4_async.py.
__device__ __forceinline__ void pp_publish(int* stamp, int value, int fences) {
    if (fences) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    else asm volatile("" ::: "memory");
    __hip_atomic_store(stamp, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// waits until *stamp >= want; the limit is WALL-CLOCK time (a slow but live peer must not send the engine to the launch path for
// good: until round 5 the limit was a count of polls), looked at every 32 polls
__device__ __forceinline__ bool pp_await(const int* stamp, int want, long long limit_ticks, int fences) {
    bool ok = true;
    if (pp_ld_i(stamp) - want < 0) {
        const long long t0 = wall_clock64();
        unsigned spins = 0;
        while (pp_ld_i(stamp) - want < 0) {
            __builtin_amdgcn_s_sleep(1);
            if (limit_ticks <= 0 || ((++spins & 31u) == 0 && wall_clock64() - t0 > limit_ticks)) { ok = false; break; }
        }
    }
    if (fences) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    else asm volatile("" ::: "memory");
    return ok;
}

#ifdef STBA_DEBUG_KNOBS
#define PP_STAMP_T(i) do { if (a.tdbg && grp == 0 && t == 0) { const long long now_ = wall_clock64(); a.tdbg[i] += now_ - tlast; tlast = now_; } } while (0)
#else
#define PP_STAMP_T(i) do { } while (0)
#endif
__global__ __launch_bounds__(PP_T) void pg_pcg_persistent_kernel(PpArgs a) {
    extern __shared__ double pp_sm[];
    __shared__ int s_abort;
    const int t = threadIdx.x, grp = blockIdx.x;
    const int n = a.n, agg = a.agg, na = a.na, nc = a.nc;
    double* rc = pp_sm;                       // [nc]   coarse residual P^T r, replicated in every group
    double* pts = rc + nc;                    // [nc]   P^T s
    double* gat = pts + nc;                   // [na][PP_SLOT]  the gathered block of exchange B
    double* ul = gat + (size_t)na * PP_SLOT;  // [384]  this group's u (the diagonal term reads it)
    double* rl = ul + 384;                    // [384]  this group's r (block Jacobi reads a node's six)
    double* vbuf = rl + 384;                  // [PP_VCAP][6]  products of the edge ends
    double* red = vbuf + (size_t)PP_VCAP * 6; // [128] scratch of the gathered sums
    double* sc = red + 128;                   // [16]  the group's sums | zc at 8..13
    if (t == 0) s_abort = 0;
    // ---- what a thread keeps for the whole solve
    const int nl = t / 6, q = t - nl * 6;
    const int node = grp * agg + nl;
    const bool act = t < agg * 6 && node < n;
    const size_t o = (size_t)node * 6 + q;
    double mrow[6] = {0, 0, 0, 0, 0, 0}, hrow[6] = {0, 0, 0, 0, 0, 0}, prow[6] = {0, 0, 0, 0, 0, 0};
    double r = 0.0, x = 0.0, p = 0.0, s = 0.0, u = 0.0, w = 0.0;
    int e0 = 0, e1 = 0;
    const int c0 = a.node_start[min(n, grp * agg)], c1 = a.node_start[min(n, (grp + 1) * agg)];
    if (act) {
        for (int b = 0; b < 6; ++b) {
            mrow[b] = a.Minv[(size_t)node * 36 + q * 6 + b];
            hrow[b] = a.Hd[(size_t)node * 36 + q * 6 + b];
            prow[b] = a.AdP[(size_t)node * 36 + q * 6 + b];
        }
        hrow[q] += a.d[o];
        r = -a.g[o];
        e0 = a.node_start[node] - c0; e1 = a.node_start[node + 1] - c0;
    }
    double acol[3][6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int c = t + j * PP_T;
#pragma unroll
        for (int rr_ = 0; rr_ < 6; ++rr_) acol[j][rr_] = (c < nc) ? a.Ainv[(size_t)(grp * 6 + rr_) * nc + c] : 0.0;
    }
    const size_t m2 = (size_t)a.node_start[n];        // edge ends = 2 m
    const int rem0 = (c0 + t < c1) ? a.end_rem[c0 + t] : 0;
    __syncthreads();

    // K values per thread -> the group's sums in sc[off .. off + K).  Through LDS in three fixed steps (512 -> 32 -> 1 per value): a
    // shuffle tree is a chain of ds_bpermute round trips, 6 per value -- 54 of them for the nine sums took 2 us of a 15 us iteration.
    // The buffer is the edge ends' product buffer, which is spent whenever sums are made.
    auto group_sum = [&](const double* v, int K, int off) {
        double* tr = vbuf;                       // [K][PP_T]
        double* p2 = vbuf + 9 * PP_T;            // [K][33]
        __syncthreads();                         // (the last reader of the products is through)
        for (int k = 0; k < K; ++k) tr[k * PP_T + t] = v[k];
        __syncthreads();
        if (t < K * 32) {
            const int k = t >> 5, j = t & 31;
            double y = 0.0;
#pragma unroll
            for (int i = 0; i < PP_T / 32; ++i) y += tr[k * PP_T + j + 32 * i];
            p2[k * 33 + j] = y;
        }
        __syncthreads();
        if (t < K) {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < 32; ++j) y += p2[t * 33 + j];
            sc[off + t] = y;
        }
        __syncthreads();
    };
    // exchange B: sc[0 .. K) of every group -> gat[group][0 .. K)
    auto all_gather = [&](int round, int K) {
        double* mine = a.pbuf + ((size_t)(round & 1) * na + grp) * PP_SLOT;
        if (t < K) { pp_st(mine + t, sc[t]); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        __syncthreads();
        if (t == 0) pp_publish(&a.pstamp[grp * PP_STAMP], a.base + round + 1, a.fences);
        if (t < na) {
            const bool ok = pp_await(&a.pstamp[t * PP_STAMP], a.base + round + 1, a.spin_limit, a.fences);
            if (!ok) s_abort = 1;
            if (ok) {
                const double* src = a.pbuf + ((size_t)(round & 1) * na + t) * PP_SLOT;
                for (int k = 0; k < K; ++k) gat[t * PP_SLOT + k] = pp_ld(src + k);
            }
        }
        __syncthreads();
    };
    // the first K entries of the gathered block summed over the groups (the same order in every group: every group gets the same bits)
    auto gathered_sums = [&](int K) {
        double* p2 = red;                        // [K][33]
        if (t < K * 32) {
            const int k = t >> 5, j = t & 31;
            double y = 0.0;
            for (int i = j; i < na; i += 32) y += gat[i * PP_SLOT + k];
            p2[k * 33 + j] = y;
        }
        __syncthreads();
        if (t < K) {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < 32; ++j) y += p2[t * 33 + j];
            sc[t] = y;
        }
        __syncthreads();
    };
    double rc2 = 0.0;                  // |P^T r|^2 of the current residual (the same bits in every group)
    auto coarse_and_u = [&]() {        // zc = (own six rows of the inverse) rc; u = Minv r + P zc
        double zp[7];
#pragma unroll
        for (int rr_ = 0; rr_ < 6; ++rr_) {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) { const int c = t + j * PP_T; if (c < nc) y += acol[j][rr_] * rc[c]; }
            zp[rr_] = y;
        }
        {
            double y = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) { const int c = t + j * PP_T; if (c < nc) y += rc[c] * rc[c]; }
            zp[6] = y;
        }
        if (t < 384) rl[t] = r;
        group_sum(zp, 7, 8);
        rc2 = sc[14];
        double z0 = 0.0;
        if (act) {
            for (int b = 0; b < 6; ++b) z0 += mrow[b] * rl[nl * 6 + b];
            for (int b = 0; b < 6; ++b) z0 += prow[b] * sc[8 + b];
        }
        u = z0;
    };
    auto finish = [&](int iters, int cap, double rr0, double rr, double tol2) {
        if (act) a.x[o] = x;
        if (grp == 0 && t == 0) {
            a.state->rr0 = rr0; a.state->rr = rr; a.state->tol2 = tol2; a.state->iters = iters; a.state->done = 1; a.state->hit_cap = cap;
        }
    };

    // ---- start: x = 0, r = -g; |r|^2 and P^T r gathered; u = M^-1 r
    {
        double v[7];
        v[0] = r * r;
        for (int b = 0; b < 6; ++b) v[1 + b] = prow[b] * r;
        group_sum(v, 7, 0);
        all_gather(0, 7);
        if (s_abort) { finish(0, PP_TIMED_OUT, 0.0, 0.0, 0.0); return; }
        for (int c = t; c < nc; c += PP_T) { rc[c] = gat[(c / 6) * PP_SLOT + 1 + (c % 6)]; pts[c] = 0.0; }
        gathered_sums(1);
    }
    const double rr0 = sc[0];
    __syncthreads();
    if (!(rr0 > 0.0) || !isfinite(rr0)) { finish(0, 0, rr0, rr0, 0.0); return; }
    const double tol2 = a.eta * a.eta * rr0;
    coarse_and_u();
    // the COARSE residual has a tolerance of its own: the coarse space holds the smooth, weakly constrained modes of the
    // graph, where a residual of eta |g| is a large error -- with the inverse of the PREVIOUS operator as coarse solver (coarse_async)
    // that error is what moves the LM trajectory away from the exact-step one.  eta_c <= 0: no such test
    const double tolc2 = a.eta_c > 0.0 ? a.eta_c * a.eta_c * rc2 : -1.0;
    double gamma_old = 1.0, alpha_old = 1.0;
    const size_t N6 = (size_t)n * 6;
    long long tlast = wall_clock64();
    (void)tlast;
    for (int k = 0;; ++k) {
        PP_STAMP_T(6);
        // ---- exchange A: publish the group's u
        double* ub = a.ubuf + (size_t)(k & 1) * N6;
        if (act) { pp_st(ub + o, u); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        if (t < 384) ul[t] = u;
        __syncthreads();
        if (t == 0) pp_publish(&a.ustamp[grp * PP_STAMP], a.base + k + 1, a.fences);
        PP_STAMP_T(0);
        // ---- off-diagonal blocks times the remote ends' u
        for (int c = c0 + t, pass = 0; c < c1; c += PP_T, ++pass) {
            double B[36];
#pragma unroll
            for (int b = 0; b < 36; ++b) B[b] = a.Bend[(size_t)b * m2 + c];
            // (the first pass's remote node is kept: one round trip less in front of the poll.  Half the groups have more than 512 ends
            // at C4 and make a second trip; measured and not kept: both trips' stamps polled together and the block loads behind the
            // poll, 1070 against 1090 LM it/s -- the loads no longer overlap the wait; both ends' blocks in flight at once: 184-472
            // bytes of scratch per lane, 780 LM it/s)
            const int rem = pass == 0 ? rem0 : a.end_rem[c];
            const int* stamp = &a.ustamp[(rem >> a.log2agg) * PP_STAMP];
            const bool ok = pp_await(stamp, a.base + k + 1, a.spin_limit, a.fences);
            if (!ok) s_abort = 1;
            double ur[6] = {0, 0, 0, 0, 0, 0};
            if (ok) for (int b = 0; b < 6; ++b) ur[b] = pp_ld(ub + (size_t)rem * 6 + b);
#pragma unroll
            for (int aa = 0; aa < 6; ++aa) {
                double y = 0.0;
#pragma unroll
                for (int b = 0; b < 6; ++b) y += B[aa * 6 + b] * ur[b];
                vbuf[(size_t)(c - c0) * 6 + aa] = y;
            }
        }
        __syncthreads();
        if (s_abort) { finish(k, PP_TIMED_OUT, rr0, 0.0, tol2); return; }
        PP_STAMP_T(1);
        w = 0.0;
        if (act) {
            for (int b = 0; b < 6; ++b) w += hrow[b] * ul[nl * 6 + b];
            for (int e = e0; e < e1; ++e) w += vbuf[(size_t)e * 6 + q];
        }
        // ---- exchange B: (r, u), (w, u), (r, r), P^T w
        {
            double v[9];
            v[0] = r * u; v[1] = w * u; v[2] = r * r;
            for (int b = 0; b < 6; ++b) v[3 + b] = prow[b] * w;
            group_sum(v, 9, 0);
            PP_STAMP_T(2);
            all_gather(k + 1, 9);
            PP_STAMP_T(3);
            if (s_abort) { finish(k, PP_TIMED_OUT, rr0, 0.0, tol2); return; }
            gathered_sums(3);
        }
        const double gamma = sc[0], delta = sc[1], rr = sc[2];
        // the residual of k updates: the stopping test (the first iteration always runs, as with the launches)
        if (k > 0 && !(rr > tol2) && !(tolc2 >= 0.0 && rc2 > tolc2)) { finish(k, 0, rr0, rr, tol2); return; }
        if (k >= a.max_iters) { finish(k, 1, rr0, rr, tol2); return; }
        const double beta = (k == 0) ? 0.0 : gamma / gamma_old;
        const double den = (k == 0) ? delta : delta - beta * gamma / alpha_old;
        if (!(den > 0.0) || !isfinite(den) || !isfinite(gamma)) { finish(k, 1, rr0, rr, tol2); return; }     // (breakdown: never seen; reported as a capped solve)
        const double alpha = gamma / den;
        p = u + beta * p; s = w + beta * s;
        x += alpha * p; r -= alpha * s;
        for (int c = t; c < nc; c += PP_T) {
            const double ps = gat[(c / 6) * PP_SLOT + 3 + (c % 6)] + beta * pts[c];
            pts[c] = ps;
            rc[c] -= alpha * ps;
        }
        gamma_old = gamma; alpha_old = alpha;
        __syncthreads();
        PP_STAMP_T(4);
        coarse_and_u();
        PP_STAMP_T(5);
    }
}

// q = (J^T J [+ D]) v.  Sharded: every rank applies its edges, rank 0 alone adds the diagonal term, and the
// hook sums the 6n-vector (the only data-path collective of a PCG iteration: every other vector operation
// is replicated and bit-identical on all ranks).
int pg_apply(stba_pg* g, const double* v, double* q, bool with_d) {
    hipLaunchKernelGGL(pg_diag_mul_kernel, dim3(g->nb_vec), dim3(256), 0, g->st, 6 * g->n, g->d, v, q,
                       (with_d && g->rank == 0) ? 1 : 0);
    hipLaunchKernelGGL(pg_matvec_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->ei, g->ej, g->Ji, g->Jj, v, q);
    STBA_HIP(hipGetLastError());
    return pg_hook(g, q, (size_t)6 * g->n);
}

}  // namespace

// LM diagonal d and the block-Jacobi preconditioner at the current trust-region radius (the first call of a solve also makes the scaling)
void pg_precond(stba_pg* g, PgSolve& sv) {
    hipLaunchKernelGGL(pg_precond_kernel, dim3(g->nb_nodes), dim3(256), 0, g->st, g->n, g->Hd, g->scale, sv.scale_init ? 0 : 1,
                       sv.opt.jacobi_scaling, sv.region.radius, sv.opt.min_lm_diagonal, sv.opt.max_lm_diagonal, g->fixed, g->d, g->Minv);
    sv.scale_init = true;
}

void pg_edge_product(stba_pg* g, const double* v, double* part, const PgPcgState* state) {
    hipLaunchKernelGGL(pg_edge_product_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->ei, g->ej, g->Ji, g->Jj, v, g->u, part, state);
}

// the PCG solve as one kernel: one rank, a coarse space whose groups fit a workgroup (<= 64 nodes, all their edge-end products
// in LDS) and are all resident at once (one per CU)
bool pg_one_kernel_eligible(stba_pg* g, const PgSolve& sv) {
    // the clauses that need no device first: a solve they rule out (several ranks, one_kernel_solve = 0, no coarse space) asks it nothing
    if (!pg_one_kernel_fits(g->coarse, sv.pcg.one_kernel_solve, sv.multi, PgDeviceLimits{INT_MAX, INT_MAX})) return false;
    // (the compute units, and the LDS a workgroup may opt in to, are properties of the device and the driver: asked, not assumed)
    int dev = 0;
    PgDeviceLimits lim{0, 0};
    bool pp_ok = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&lim.cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
                 hipDeviceGetAttribute(&lim.lds_max_optin, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess &&
                 pg_one_kernel_fits(g->coarse, sv.pcg.one_kernel_solve, sv.multi, lim);
    if (pp_ok) {
        static DeviceOnce attr;
        // a device that refuses the attribute takes the launch path; that is not a failed solve
        if (attr.run([]() -> int {
                STBA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pg_pcg_persistent_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PP_LDS_MAX));
                return STBA_OK;
            }) != STBA_OK) { pp_ok = false; g->pp_disabled = true; (void)hipGetLastError(); }
    }
    return pp_ok;
}

// ---- PCG on (J^T J + D) x = -g, stopped on the device at |r| <= eta_k |g|: four launches per iteration, watched by the host
int pg_pcg_by_launches(stba_pg* g, const PgSolve& sv, const double* Ainv_use, double eta_k) {
    const stba_pcg_options& pcg = sv.pcg;
    const bool coarse = sv.coarse;
    const double* AdP = coarse ? g->AdP : nullptr;
    // (every kernel of the previous solve has finished -- the host has read the trial block behind them -- so the exported
    // block can be taken back: the wait below must not see the previous solve's tick count and `done`)
    g->exp.zero();
    std::atomic_thread_fence(std::memory_order_seq_cst);
    hipLaunchKernelGGL(pg_pcg_init4_kernel, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->coarse.agg, g->g, g->Minv, AdP, g->x, g->rr, g->z,
                       g->rc_part, g->part_a);
    if (coarse)
        hipLaunchKernelGGL(pg_coarse_solve_kernel, dim3((g->coarse.nc + 3) / 4), dim3(256), 0, g->st, g->coarse.nc, g->coarse.parts, (const PgPcgState*)nullptr, Ainv_use, g->rc_part,
                           g->zc, g->part_cz);
    // (an engine that holds node pose priors runs the PRIOR instantiations of the node kernels, every other one the kernels as they were:
    // no launch more per iteration either way)
    const bool prior = g->pr.n > 0;
    const int* node_slot = prior ? g->pr.node_slot.get() : nullptr;
    const double* Hp = prior ? g->pr.Hp.get() : nullptr;
    auto direction = [&](int slot, int first) {
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->coarse.agg, slot, first, eta_k, pcg.max_iterations, g->state, g->exp.dev,
                               g->nb_nodes4, g->part_a, (g->coarse.nc + 3) / 4, coarse ? g->part_cz : nullptr, AdP, g->zc, g->z, g->d, g->p, g->part_d,
                               node_slot, Hp);
        };
        if (prior) launch(pg_pcg_dir4_kernel<true>); else launch(pg_pcg_dir4_kernel<false>);
    };
    direction(1, 1);
    STBA_HIP(hipGetLastError());
    int enq = 0;
    bool pcg_done = false;
    double px[PX_COUNT];
    STBA_TRY(stamped_wait(g->exp.host, PX_COUNT, [](double st) { return st >= 1.0; }, px, hip_stream_state(g->st), "pose graph",
                          120.0));          // (also: the previous solve's ticks are gone)
    if (px[PX_DONE] != 0.0) pcg_done = true;
    while (!pcg_done && enq < pcg.max_iterations) {
        const int todo = std::min(sv.chunk, pcg.max_iterations - enq);
        for (int c = 0; c < todo; ++c, ++enq) {
            const int slot = enq & 1;
            if (!sv.multi) {
                pg_edge_product(g, g->p, g->part_c, g->state);
                auto update = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->m, g->coarse.agg, slot, g->state, g->nb_edges,
                                       g->part_c, g->nb_nodes4, g->part_d, g->Minv, AdP, g->d, g->node_start, g->end_code, g->u, (const double*)nullptr,
                                       g->p, g->x, g->rr, g->z, g->rc_part, g->part_a, node_slot, Hp);
                };
                if (prior) update(pg_pcg_update4_kernel<true, true>); else update(pg_pcg_update4_kernel<true, false>);
            } else {
                STBA_TRY(pg_apply(g, g->p, g->q, true));
                hipLaunchKernelGGL(pg_dot_kernel, dim3(g->nb_vec), dim3(256), 0, g->st, 6 * g->n, g->p, g->q, g->part_c);
                hipLaunchKernelGGL(pg_pcg_update4_kernel<false>, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->m, g->coarse.agg, slot, g->state, g->nb_vec,
                                   g->part_c, 0, (const double*)nullptr, g->Minv, AdP, g->d, g->node_start, g->end_code, g->u, g->q,
                                   g->p, g->x, g->rr, g->z, g->rc_part, g->part_a, (const int*)nullptr, (const double*)nullptr);
            }
            if (coarse)
                hipLaunchKernelGGL(pg_coarse_solve_kernel, dim3((g->coarse.nc + 3) / 4), dim3(256), 0, g->st, g->coarse.nc, g->coarse.parts, g->state, Ainv_use, g->rc_part, g->zc,
                                   g->part_cz);
            direction(slot, 0);
        }
        STBA_HIP(hipGetLastError());
        // one rank: the host looks at the chunk BEFORE the one it has just enqueued (the stream never runs dry; the kernels of a
        // chunk enqueued past convergence return at once).  Several ranks: every rank must enqueue the same collectives, so the
        // decision waits for the chunk itself -- the solve state is replicated and every rank sees the same `done`.
        const double want = 1 + (sv.multi ? enq : enq - todo);
        STBA_TRY(stamped_wait(g->exp.host, PX_COUNT, [want](double st) { return st >= want; }, px, hip_stream_state(g->st), "pose graph",
                              120.0));
        if (px[PX_DONE] != 0.0) pcg_done = true;
    }
    return STBA_OK;
}

// the same solve as ONE kernel (see pg_pcg_persistent_kernel): nothing for the host to watch, the trial point follows on the stream
int pg_pcg_one_kernel(stba_pg* g, const PgSolve& sv, const double* Ainv_use, double eta_k) {
    const stba_pcg_options& pcg = sv.pcg;
    pg_offdiag_if_stale(g);
    if (g->pp_base > (1 << 30)) {        // (stamps only grow; long before they wrap they are taken back to zero)
        STBA_HIP(hipMemsetAsync(g->ustamp, 0, PP_GROUPS_MAX * PP_STAMP * sizeof(int), g->st));
        STBA_HIP(hipMemsetAsync(g->pstamp, 0, PP_GROUPS_MAX * PP_STAMP * sizeof(int), g->st));
        g->pp_base = 0;
    }
    PpArgs a;
    a.n = g->n; a.agg = g->coarse.agg; a.log2agg = 0; while ((1 << a.log2agg) < g->coarse.agg) ++a.log2agg;
    a.na = g->coarse.na; a.nc = g->coarse.nc; a.base = g->pp_base; a.max_iters = pcg.max_iterations; a.eta = eta_k;
    a.node_start = g->node_start; a.end_rem = g->end_rem; a.Bend = g->Bend; a.Hd = g->Hd; a.d = g->d; a.Minv = g->Minv; a.AdP = g->AdP;
    a.Ainv = Ainv_use; a.g = g->g; a.x = g->x; a.ubuf = g->ubuf; a.pbuf = g->pbuf; a.ustamp = g->ustamp; a.pstamp = g->pstamp;
    a.state = g->state; a.spin_limit = pcg.one_kernel_solve == 2 ? 0 : 25000000ll;      // (a quarter of a second of wall_clock64 ticks; 2: the test of the way back)
    a.fences = pcg.one_kernel_solve == 3 ? 1 : 0;
    a.eta_c = sv.forcing ? pcg.coarse_eta : 0.0;
    a.tdbg = nullptr;
#ifdef STBA_DEBUG_KNOBS
    static long long* tdbg_dev = nullptr;
    if (knob_int("STBA_PP_TIMING", 0)) {
        if (!tdbg_dev) { STBA_HIP(hipMalloc(&tdbg_dev, 8 * sizeof(long long))); STBA_HIP(hipMemset(tdbg_dev, 0, 8 * sizeof(long long))); }
        a.tdbg = tdbg_dev;
    }
#endif
    hipLaunchKernelGGL(pg_pcg_persistent_kernel, dim3(g->coarse.na), dim3(PP_T), pp_lds_bytes(g->coarse.na, g->coarse.nc), g->st, a);
#ifdef STBA_DEBUG_KNOBS
    if (a.tdbg) {
        long long h[8];
        STBA_HIP(hipMemcpyAsync(h, tdbg_dev, sizeof h, hipMemcpyDeviceToHost, g->st)); STBA_HIP(hipStreamSynchronize(g->st));
        fprintf(stderr, "pp phases (x 10 ns, cumulative): publish %lld | ends %lld | w+sum9 %lld | all-gather %lld | scalars+update %lld | coarse+u %lld | loop top %lld\n",
                h[0], h[1], h[2], h[3], h[4], h[5], h[6]);
    }
#endif
    STBA_HIP(hipGetLastError());
    g->pp_base += pcg.max_iterations + 8;
    return STBA_OK;
}

}  // namespace stba
