// pg_coarse.hip -- the coarse space of the pose graph's two-level preconditioner (six rigid-body modes per group of consecutive
// nodes: pg_engine.hip's header): the kernels that make the basis, the Galerkin matrix P^T J^T J P from the assembled blocks, its
// damping term, the inversion workspace and the inverse, and pg_offdiag_kernel, whose blocks the coarse matrix shares with the
// persistent PCG kernel; on the host the buffers for a group size, the steps of an LM iteration's coarse operator, and the
// second-stream job (PgCoarseJob, pg_engine.hpp) that takes the inversion off the critical path.
#include <algorithm>

#include "pg_device.hpp"
#include "pg_engine.hpp"

namespace stba {
namespace {

// damping term of the coarse matrix: Dc[group] = sum over the group's nodes of P_k^T diag(d_k) P_k (6 x 6), one workgroup per group
__global__ __launch_bounds__(256) void pg_coarse_dc_kernel(int n, int agg, const double* __restrict__ AdP, const double* __restrict__ d,
                                                           double* __restrict__ Dc) {
    __shared__ double sw[4][36];
    const int a = blockIdx.x, t = threadIdx.x;
    const int k0 = a * agg, k1 = min(n, k0 + agg);
    double acc[36];
    for (int q = 0; q < 36; ++q) acc[q] = 0.0;
    for (int item = t; item < (k1 - k0) * 6; item += 256) {          // (node, tangent component)
        const int k = k0 + item / 6, c = item % 6;
        const double dv = d[(size_t)k * 6 + c];
        double row[6];
        for (int u = 0; u < 6; ++u) row[u] = AdP[(size_t)k * 36 + c * 6 + u];
        for (int u = 0; u < 6; ++u)
            for (int w = 0; w < 6; ++w) acc[u * 6 + w] += row[u] * dv * row[w];
    }
    for (int q = 0; q < 36; ++q) {
        double v = acc[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((t & 63) == 0) sw[t >> 6][q] = v;
    }
    __syncthreads();
    if (t < 36) Dc[(size_t)a * 36 + t] = (sw[0][t] + sw[1][t]) + (sw[2][t] + sw[3][t]);
}

// coarse basis: P_k = Ad(T_k^-1 T_ref), T_ref = the pose in the middle of the node's group; zero for constant nodes.
// Ad(R, t) = [[R, hat(t) R], [0, R]] for the tangent order [rho, theta] (st23-lie-group-v2/doc.tex:945-963)
__global__ __launch_bounds__(256) void pg_coarse_basis_kernel(int n, int agg, const double* __restrict__ poses,
                                                              const unsigned char* __restrict__ fixed, double* __restrict__ AdP) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    double M[36];
    for (int q = 0; q < 36; ++q) M[q] = 0.0;
    if (!(fixed && fixed[k])) {
        const int ref = min((k / agg) * agg + agg / 2, n - 1);
        double Tk[7], Tr[7], Tki[7], rel[7], R[9], Hh[9];
        for (int q = 0; q < 7; ++q) { Tk[q] = poses[(size_t)k * 7 + q]; Tr[q] = poses[(size_t)ref * 7 + q]; }
        se3_inverse(Tk, Tki);
        se3_compose(Tki, Tr, rel);
        quat_to_rot(rel, R);
        hat3d(rel + 4, Hh);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double s = 0.0;
                for (int q = 0; q < 3; ++q) s += Hh[i * 3 + q] * R[q * 3 + j];
                M[i * 6 + j] = R[i * 3 + j]; M[i * 6 + 3 + j] = s; M[(3 + i) * 6 + 3 + j] = R[i * 3 + j];
            }
    }
    for (int q = 0; q < 36; ++q) AdP[(size_t)k * 36 + q] = M[q];
}

// Galerkin coarse matrix without the damping term, Ac0 = P^T J^T J P (nc x nc, dense): one workgroup per group of nodes
// = six rows of Ac0, from the ASSEMBLED blocks (until then every edge end re-made G = J P from two scattered Jacobians, 71 us):
//   the diagonal block of the group gets  sum over its nodes of P_i^T Hd_i P_i  (Hd_i = the node's diagonal block of J^T J, which
//   the linearisation leaves) and, for every edge end whose other node lies in the same group, P_s^T B P_o;
//   block (group, group of the other node) gets P_s^T B P_o for every other end -- B = J_s^T J_o is the end's block of
//   pg_offdiag_kernel, read coalesced in CSR order.  The other end does the same from its side, so the four blocks of an edge are
//   all made and no workgroup writes another one's rows.
// The row panel is accumulated in LDS and written once, zeros included: no global atomics, no memset.
// REPRODUCIBLE sums (until then the four waves added to the panel in arrival order and the preconditioner -- hence every
// PCG iterate -- differed in the last bits from run to run): every block of the panel is added to by ONE wave, the wave
// (other group) mod 4, whose adds meet an LDS address in program and lane order.  Each wave first collects ITS ends, in CSR order,
// into a list of its own (ballot + prefix count), then works through the list with all lanes.
// Several ranks (edge shards): Hd is the cross-rank sum, so only rank 0 adds the nodes' term (add_nodes).
__global__ __launch_bounds__(256) void pg_coarse_build_kernel(int n, int agg, int nc, int add_nodes, const int* __restrict__ node_start,
                                                              const int* __restrict__ end_node, const int* __restrict__ end_rem,
                                                              const double* __restrict__ Bend, const double* __restrict__ Hd,
                                                              const double* __restrict__ AdP, double* __restrict__ Ac0) {
    extern __shared__ double rowp[];            // [6][nc] | four lists of edge ends (int)
    __shared__ double dgp[4][36];
    __shared__ double dnode[64][37];
    const int a = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int q = t; q < 6 * nc; q += 256) rowp[q] = 0.0;
    const int k0 = a * agg, k1 = min(n, k0 + agg);
    const int c0 = node_start[k0], c1 = node_start[k1];
    const size_t m2 = (size_t)node_start[n];
    int* mylist = reinterpret_cast<int*>(rowp + (size_t)6 * nc) + (size_t)wv * (c1 - c0);
    int cnt = 0;
    for (int cb = c0; cb < c1; cb += 64) {
        const int c = cb + lane;
        const bool mine = c < c1 && ((end_rem[c] / agg) & 3) == wv;
        const unsigned long long bal = __ballot(mine);
        if (mine) mylist[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = c;
        cnt += __popcll(bal);
    }
    // the nodes' term: one node per thread (groups of more than 64 nodes: in rounds), summed over the nodes in order below
    double dsum = 0.0;                          // thread q < 36: entry q of the diagonal block
    for (int base = k0; base < k1; base += 64) {
        __syncthreads();
        const int node = base + t;
        if (t < 64) {
            double M[36];
            for (int q = 0; q < 36; ++q) M[q] = 0.0;
            if (node < k1 && add_nodes) {
                double H[36], P[36], T[36];
                for (int q = 0; q < 36; ++q) { H[q] = Hd[(size_t)node * 36 + q]; P[q] = AdP[(size_t)node * 36 + q]; }
                for (int i = 0; i < 6; ++i)
                    for (int j = 0; j < 6; ++j) {
                        double s2 = 0.0;
                        for (int q = 0; q < 6; ++q) s2 += H[i * 6 + q] * P[q * 6 + j];
                        T[i * 6 + j] = s2;
                    }
                for (int u = 0; u < 6; ++u)
                    for (int v = 0; v < 6; ++v) {
                        double s2 = 0.0;
                        for (int q = 0; q < 6; ++q) s2 += P[q * 6 + u] * T[q * 6 + v];
                        M[u * 6 + v] = s2;
                    }
            }
            for (int q = 0; q < 36; ++q) dnode[t][q] = M[q];
        }
        __syncthreads();
        if (t < 36) for (int i = 0; i < 64; ++i) dsum += dnode[i][t];
    }
    __syncthreads();
    double dg[36];
    for (int q = 0; q < 36; ++q) dg[q] = 0.0;
    for (int idx = lane; idx < cnt; idx += 64) {
        const int c = mylist[idx];
        const int self = end_node[c], other = end_rem[c];
        double B[36], P[36], T[36];
        for (int q = 0; q < 36; ++q) { B[q] = Bend[(size_t)q * m2 + c]; P[q] = AdP[(size_t)other * 36 + q]; }
        for (int i = 0; i < 6; ++i)               // T = B P_o
            for (int j = 0; j < 6; ++j) {
                double s2 = 0.0;
                for (int q = 0; q < 6; ++q) s2 += B[i * 6 + q] * P[q * 6 + j];
                T[i * 6 + j] = s2;
            }
        for (int q = 0; q < 36; ++q) P[q] = AdP[(size_t)self * 36 + q];
        const int ao = other / agg;
        for (int u = 0; u < 6; ++u)
            for (int v = 0; v < 6; ++v) {
                double so = 0.0;
                for (int q = 0; q < 6; ++q) so += P[q * 6 + u] * T[q * 6 + v];
                if (ao == a) dg[u * 6 + v] += so;
                else unsafeAtomicAdd(&rowp[u * nc + 6 * ao + v], so);
            }
    }
    // the diagonal block: the waves' register sums through a shuffle tree each, the four waves in order, then the nodes' term
    for (int q = 0; q < 36; ++q) {
        double v = dg[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) dgp[wv][q] = v;
    }
    __syncthreads();
    if (t < 36) rowp[(t / 6) * nc + 6 * a + (t % 6)] = ((dgp[0][t] + dgp[1][t]) + (dgp[2][t] + dgp[3][t])) + dsum;
    __syncthreads();
    for (int q = t; q < 6 * nc; q += 256) Ac0[(size_t)(6 * a + q / nc) * nc + (q % nc)] = rowp[q];
}

// the inversion workspace of an LM iteration: W = [Ac0 + P^T D P (identity-padded to np) | . ; I | 0], see chol_spd_inverse_dev
__global__ __launch_bounds__(256) void pg_coarse_assemble_kernel(int nc, int np, const double* __restrict__ Ac0,
                                                                 const double* __restrict__ Dc, double* __restrict__ W) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)np * np;
    if (idx >= 3 * per) return;
    const int quad = (int)(idx / per);
    const int r = (int)((idx % per) / np), c = (int)(idx % np);
    const size_t ldw = 2 * (size_t)np;
    if (quad == 1) { W[(np + r) * ldw + c] = (r == c) ? 1.0 : 0.0; return; }
    if (quad == 2) { W[(np + r) * ldw + np + c] = 0.0; return; }
    double v = (r == c) ? 1.0 : 0.0;
    if (r < nc && c < nc) {
        v = Ac0[(size_t)r * nc + c];
        if (r / 6 == c / 6) {
            v += Dc[(size_t)(r / 6) * 36 + (r % 6) * 6 + (c % 6)];
            if (r == c && !(v > 0.0)) v = 1.0;          // a group of constant nodes
        }
    }
    W[r * ldw + c] = v;
}

// Ainv = -(lower right block of W), symmetric, full.  cflag: the pivot flag of the partial factorisation that made W -- a non-positive
// pivot (or a NaN) in P^T (J^T J + D) P leaves garbage there: the coarse correction is then switched OFF for this operator (Ainv = 0:
// z = z0, block Jacobi alone, still a symmetric positive definite preconditioner) and counted (stba_pcg_summary::coarse_failures),
// instead of sending the PCG into NaNs and the LM step into a rejection nobody can explain.
__global__ __launch_bounds__(256) void pg_coarse_finish_kernel(int nc, int np, const double* __restrict__ W, double* __restrict__ Ainv,
                                                               const int* __restrict__ cflag, int* __restrict__ fail_count) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = cflag[0] != 0;
    if (idx == 0 && bad) atomicAdd(fail_count, 1);
    if (idx >= (size_t)nc * nc) return;
    const int r = (int)(idx / nc), c = (int)(idx % nc);
    const int hi = max(r, c), lo = min(r, c);
    Ainv[idx] = bad ? 0.0 : -W[((size_t)np + hi) * (2 * (size_t)np) + np + lo];
}

// B_e = Ji^T Jj of every edge, stored COMPONENT-major over the CSR positions of the edge ENDS ([36][2 m]): column end_pos[2 e] (the
// end at i, which multiplies u_j) gets B_e, column end_pos[2 e + 1] (the end at j, which multiplies u_i) its transpose
__global__ __launch_bounds__(256) void pg_offdiag_kernel(int m, const double* __restrict__ Ji, const double* __restrict__ Jj,
                                                         const int* __restrict__ end_pos, double* __restrict__ Bend) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m) return;
    double A[36], B[36];
    for (int k = 0; k < 36; ++k) { A[k] = Ji[(size_t)k * m + e]; B[k] = Jj[(size_t)k * m + e]; }
    const size_t m2 = 2 * (size_t)m;
    const size_t c0 = (size_t)end_pos[2 * e], c1 = (size_t)end_pos[2 * e + 1];
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) {
            double s = 0.0;
            for (int r = 0; r < 6; ++r) s += A[r * 6 + a] * B[r * 6 + b];
            Bend[(size_t)(a * 6 + b) * m2 + c0] = s;
            Bend[(size_t)(b * 6 + a) * m2 + c1] = s;
        }
}

// the first stream waits for an event of the second one only if the event has NOT fired yet when the dependent work is enqueued: a
// wait packet costs ~10 us of idle GPU even when its event has long fired (dense_chol.hip's note on the same), and here it nearly
// always has -- the job it guards started a whole PCG solve earlier.  The data flow is the same either way: same bits.
int pg_wait_if_pending(hipStream_t st, hipEvent_t ev) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return STBA_OK;
    if (q != hipErrorNotReady) { (void)hipGetLastError(); }
    STBA_HIP(hipStreamWaitEvent(st, ev, 0));
    return STBA_OK;
}

// the coarse matrix P^T J^T J P from the blocks; add_nodes: with the diagonal blocks' part (several ranks: rank 0 alone)
void pg_coarse_build(stba_pg* g, hipStream_t st, int add_nodes) {
    hipLaunchKernelGGL(pg_coarse_build_kernel, dim3(g->coarse.na), dim3(256), g->coarse.build_lds_bytes, st, g->n, g->coarse.agg, g->coarse.nc,
                       add_nodes, g->node_start, g->end_node, g->end_rem, g->Bend, g->Hd, g->AdP, g->Ac0);
}

// its damping term P^T D P, and W = the padded sum of the two
void pg_coarse_damped(stba_pg* g, hipStream_t st) {
    const size_t cnt = (size_t)3 * g->coarse.np * g->coarse.np;
    hipLaunchKernelGGL(pg_coarse_dc_kernel, dim3(g->coarse.na), dim3(256), 0, st, g->n, g->coarse.agg, g->AdP, g->d, g->Dc);
    hipLaunchKernelGGL(pg_coarse_assemble_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, g->coarse.nc, g->coarse.np, g->Ac0, g->Dc, g->W);
}

// W^-1 -> Aout
int pg_coarse_invert(stba_pg* g, hipStream_t st, double* Aout) {
    STBA_TRY(chol_spd_inverse_dev(g->W, 2 * g->coarse.np, g->coarse.np, g->coarse.nc, g->cflag, g->inv_work, st));
    hipLaunchKernelGGL(pg_coarse_finish_kernel, dim3((unsigned)(((size_t)g->coarse.nc * g->coarse.nc + 255) / 256)), dim3(256), 0, st, g->coarse.nc, g->coarse.np, g->W, Aout,
                       g->cflag, g->cflag + 1);
    return STBA_OK;
}

}  // namespace

// ---- coarse space: the sizes (pg_plan_coarse) and the buffers for a group size (lazily: the group size is an option of the solve)
int pg_setup_coarse(stba_pg* g, int group_opt) {
    PgCoarsePlan plan;
    std::string why;
    const int rc = pg_plan_coarse(g->n, g->node_start_host, group_opt, &plan, &why);
    if (rc != 0) return fail(rc, why);
    if (plan.agg < 0) { g->coarse.agg = -1; g->coarse_valid = false; return STBA_OK; }
    if (plan.agg == g->coarse.agg) return STBA_OK;
    const int na = plan.na, nc = plan.nc, np = plan.np, parts = plan.parts;
    STBA_TRY(g->job.quiesce());       // (a job of the last solve may still be writing W / an inverse)
    for (auto* buf : {&g->AdP, &g->Ac0, &g->W, &g->job.Ainv[0], &g->job.Ainv[1], &g->inv_work, &g->rc_part, &g->zc, &g->part_cz, &g->Dc}) buf->reset();
    g->coarse.agg = 0;
    STBA_TRY(g->AdP.alloc((size_t)g->n * 36)); STBA_TRY(g->Ac0.alloc((size_t)nc * nc)); STBA_TRY(g->W.alloc((size_t)4 * np * np));
    STBA_TRY(g->job.Ainv[0].alloc((size_t)nc * nc)); STBA_TRY(g->job.Ainv[1].alloc((size_t)nc * nc)); STBA_TRY(g->Dc.alloc((size_t)na * 36)); STBA_TRY(g->inv_work.alloc(chol_spd_inverse_workspace_doubles(np)));
    STBA_TRY(g->rc_part.alloc((size_t)na * parts * 6)); STBA_TRY(g->zc.alloc((size_t)nc)); STBA_TRY(g->part_cz.alloc((size_t)((nc + 3) / 4) * 2 + 2));
    STBA_HIP(hipMemsetAsync(g->rc_part, 0, (size_t)na * parts * 6 * sizeof(double), g->st));
    static DeviceOnce attr;
    STBA_TRY(attr.run([]() -> int {
        STBA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pg_coarse_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PG_COARSE_BUILD_LDS_MAX));
        return STBA_OK;
    }));
    g->coarse = plan;
    g->coarse_valid = false;
    return STBA_OK;
}

void pg_offdiag_if_stale(stba_pg* g) {
    if (g->bend_valid) return;
    hipLaunchKernelGGL(pg_offdiag_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->Ji, g->Jj, g->end_pos, g->Bend);
    g->bend_valid = true;
}

// ---- what a new linearisation means for the coarse space: its basis at the new poses, the edge-end blocks, and the coarse matrix
int pg_coarse_linearized(stba_pg* g, const PgSolve& sv) {
    hipLaunchKernelGGL(pg_coarse_basis_kernel, dim3(g->nb_nodes), dim3(256), 0, g->st, g->n, g->coarse.agg, g->poses[g->cur], g->fixed, g->AdP);
    pg_offdiag_if_stale(g);
    // (one rank with the coarse inverse on its second stream: the coarse MATRIX is only read by that job, and is built there --
    // 55 us of every LM iteration off the critical path; several ranks sum it with the hook, on the engine's stream)
    if (!sv.build_on_st2) {
        pg_coarse_build(g, g->st, (!g->ar || g->rank == 0) ? 1 : 0);
        STBA_TRY(pg_hook(g, g->Ac0, (size_t)g->coarse.nc * g->coarse.nc));
    }
    g->coarse_valid = false;
    g->job.ac0_valid = false;
    return STBA_OK;
}

// (the job of the second stream reads the blocks, the coarse basis and the damping of the linearisation it belongs to: whatever
// overwrites them -- the next linearisation, or the preconditioner kernel -- waits until it has: an event that has long fired by then)
int pg_wait_for_job_reads(stba_pg* g) {
    if (g->job.reads_pending) { STBA_TRY(pg_wait_if_pending(g->st, g->job.ev_read)); g->job.reads_pending = false; }
    return STBA_OK;
}

// the HEAD of the second stream's job (one rank): everything the inverse needs -- the coarse matrix from the blocks, the diagonal
// blocks and the basis of THIS linearisation, its damping term, the workspace; READ_k tells the first stream when its next
// linearisation / preconditioner kernel may overwrite those inputs.  Three launches: behind an accepted step they are enqueued
// at once (the preconditioner kernel in front of them), so that they run under the host's wait for the new point's scalars
// instead of at the start of the PCG kernel, with which the inversion then competes for CUs.
int pg_job_head(stba_pg* g) {
    PgCoarseJob& j = g->job;
    STBA_HIP(hipStreamWaitEvent(j.st2, j.ev_in, 0));
    if (!j.ac0_valid) {
        pg_coarse_build(g, j.st2, 1);
        j.ac0_valid = true;
    }
    pg_coarse_damped(g, j.st2);
    STBA_HIP(hipEventRecord(j.ev_read, j.st2));
    j.reads_pending = true;
    j.in_flight = true;
    return STBA_OK;
}

// THE JOB: ~ 30 launches on the second stream.  Enqueueing them takes the HOST ~ 250 us -- so when the iteration does not
// wait for them (the usual case), the PCG kernel is launched FIRST and the job is enqueued while it runs: with the job in
// front, the kernel timeline showed the first stream idle for 277 us of every 760 us iteration, waiting for the host
// (profiles/r6_c4_iter_trace.txt)
int pg_job_rest(stba_pg* g, const PgSolve& sv, const PgJob& job) {
    PgCoarseJob& j = g->job;
    if (!job.head_was_done) { if (sv.build_on_st2) STBA_TRY(pg_job_head(g)); else STBA_HIP(hipStreamWaitEvent(j.st2, j.ev_in, 0)); }
    STBA_TRY(pg_coarse_invert(g, j.st2, j.Ainv[job.wbuf]));
    STBA_HIP(hipEventRecord(j.ev_job[job.wbuf], j.st2));
    j.in_flight = true;
    return STBA_OK;
}

// ---- coarse operator (P^T (J^T J + D) P)^-1 of an LM iteration
int pg_coarse_refresh(stba_pg* g, PgSolve& sv, bool head_was_done, PgCoarseUse* use) {
    PgCoarseJob& j = g->job;
    use->Ainv = j.Ainv[0];
    use->job_deferred = false;
    if (sv.coarse && sv.async_inv) {
        // Off the critical path.  The inversion (eight panels of a ~45 us chain on a handful of CUs: 0.39 of a 0.92 ms LM
        // iteration at C4) runs on a SECOND stream, next to this iteration's PCG kernel (157 workgroups on 256 CUs), and is applied one LM
        // iteration LATE: iteration k preconditions with the inverse of iteration k - 1's operator -- an inverse made at the
        // previous linearisation / damping still is a preconditioner, only a weaker one (coarse_refresh_every = 2 had measured
        // + 9 % PCG iterations).  The very first solve has no predecessor: it waits for its own inverse (coarse_async = 2 with a
        // forcing sequence: it runs on block Jacobi alone, Ainv = 0 -- 3 PCG iterations at eta_0 = 0.1, but a first step that
        // leaves the cost at 1021 where the two-level step leaves 258 and the exact one 48: the whole trajectory moves).
        // Everything is ordered by events, so the result does not depend on timing: run to run the same bits.
        //   stream 1: precond_k | wait job_{k-1} | record IN_k | PCG_k (Ainv of job_{k-1}) | trial | wait READ_k | linearise ...
        //   stream 2:                              wait IN_k   | coarse matrix, Dc_k, assemble W_k | record READ_k | invert -> Ainv[k & 1] | record job_k
        // (several ranks: coarse matrix -- summed by the hook --, Dc_k and W_k stay on stream 1, IN_k is recorded behind them)
        const int wbuf = sv.jobs & 1;
        double* Aw = j.Ainv[wbuf];
        double* Ar = j.Ainv[wbuf ^ 1];        // written by the previous job (or zeroed below)
        if (sv.jobs == 0) STBA_HIP(hipMemsetAsync(Ar, 0, (size_t)g->coarse.nc * g->coarse.nc * sizeof(double), g->st));
        else STBA_TRY(pg_wait_if_pending(g->st, j.ev_job[(sv.jobs - 1) & 1]));
        const bool own = pg_waits_for_own_inverse(sv.pcg, sv.forcing, sv.jobs, sv.iter, sv.last_rel_decrease);
        if (!sv.build_on_st2) pg_coarse_damped(g, g->st);
        if (!head_was_done) STBA_HIP(hipEventRecord(j.ev_in, g->st));
        use->job.wbuf = wbuf;
        use->job.head_was_done = head_was_done;
        use->Ainv = Ar;
        if (own) {
            STBA_TRY(pg_job_rest(g, sv, use->job));
            STBA_HIP(hipStreamWaitEvent(g->st, j.ev_job[wbuf], 0));
            use->Ainv = Aw;
        } else use->job_deferred = true;
        ++sv.jobs;
        g->coarse_valid = true;
        ++sv.ps.coarse_refreshes;
    } else if (sv.coarse && (sv.ps.coarse_refreshes < 2 || sv.since_refresh >= std::max(1, sv.pcg.coarse_refresh_every))) {
        // (synchronous form, coarse_async = 0) rebuilt when the linearisation or (every coarse_refresh_every-th time) the damping changed
        // (the inverse is a preconditioner: one made at an earlier linearisation / damping still is one, only weaker -- with
        // coarse_refresh_every = k it is re-made every k-th LM iteration; the first two iterations always make theirs)
        pg_coarse_damped(g, g->st);
        STBA_TRY(pg_coarse_invert(g, g->st, j.Ainv[0]));
        g->coarse_valid = true;
        sv.since_refresh = 0;
        ++sv.ps.coarse_refreshes;
    }
    ++sv.since_refresh;
    return STBA_OK;
}

}  // namespace stba
