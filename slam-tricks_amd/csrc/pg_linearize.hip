// pg_linearize.hip -- the linearisation of the pose graph and everything that feeds it: the edge's residual and Jacobians and the
// whitening by per-edge square-root information (pg_edge, pg_whiten_cols: pg_edge.hpp, shared with pg_prior.hip), the robust
// corrector, the kernel that writes r, Ji, Jj and the per-end contributions, the gather of the gradient and the diagonal blocks, the
// conversion of the caller's weights; on the host pg_linearize, pg_gather_blocks, the setters of weights and losses, stba_pg_evaluate
// and stba_pg_time_kernels (which times this unit's kernel and the edge product of pg_pcg.hip).  The method: pg_engine.hip's header.
#include <climits>
#include <vector>

#include "dd6.hpp"
#include "pg_device.hpp"
#include "pg_edge.hpp"
#include "pg_engine.hpp"
#include "robust_loss.hpp"

namespace stba {
namespace {

// J <- sqrt(rho') (J - k r (r^T J)) for the 6 x 6 row-major J of one edge end, one column at a time (k = alpha / s of Ceres' corrector;
// k == 0: the scaling alone)
__device__ inline void pg_correct_cols(const double* re, double* J, double sq, double k) {
    for (int c = 0; c < 6; ++c) {
        if (k != 0.0) {
            double t = 0.0;
            for (int a = 0; a < 6; ++a) t += re[a] * J[a * 6 + c];
            t *= k;
            for (int a = 0; a < 6; ++a) J[a * 6 + c] = sq * (J[a * 6 + c] - re[a] * t);
        } else {
            for (int a = 0; a < 6; ++a) J[a * 6 + c] = sq * J[a * 6 + c];
        }
    }
}

// INFO = false: every edge weighted by the identity -- the kernel as it was before edges had information matrices; Winfo is not
// read.  INFO = true: the residual and both Jacobians are whitened by the edge's square-root information W_e (Winfo[k * n_edges + e],
// laid out like Ji) right behind pg_edge: cost, stores, the constant-node zeroing and the contrib block below all see W r, W Ji,
// W Jj, and so does every consumer of what this kernel writes.  Two instantiations and not a runtime branch: an engine without
// weights runs the instruction stream it ran before.
// ROBUST = false: no edge has a loss, the kernel as it was before (lkind, la, lb, lscale are not read).  ROBUST = true: behind the
// whitening the edge's loss (lkind[e], la[e], lb[e], lscale[e]: read by edge index) is evaluated at s = |r|^2 and Ceres' corrector
// turns r and both Jacobians into r', J' with J'^T r' = rho' J^T r and J'^T J' the Triggs approximation of the robustified Hessian;
// the edge's cost term is rho(s).  Every store and the contrib block see r', J'.  An edge of kind TRIVIAL and scale 1 is left alone:
// what it stores compares == to the ROBUST = false kernel's.  The kind is a runtime switch: lanes of a wave may differ.
template <bool INFO, bool ROBUST>
__global__ __launch_bounds__(256) void pg_linearize_kernel(int n_edges, const double* __restrict__ poses,
                                                           const int* __restrict__ ei, const int* __restrict__ ej,
                                                           const double* __restrict__ meas,
                                                           const unsigned char* __restrict__ fixed, int with_jac,
                                                           double* __restrict__ r, double* __restrict__ Ji,
                                                           double* __restrict__ Jj, double* __restrict__ partial,
                                                           double* __restrict__ contrib, const double* __restrict__ Winfo,
                                                           const int* __restrict__ lkind, const double* __restrict__ la,
                                                           const double* __restrict__ lb, const double* __restrict__ lscale) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    double c = 0.0;
    if (e < n_edges) {
        const int i = ei[e], j = ej[e];
        double Ti[7], Tj[7], Z[7], re[6], ji[36], jj[36];
        for (int k = 0; k < 7; ++k) { Ti[k] = poses[(size_t)i * 7 + k]; Tj[k] = poses[(size_t)j * 7 + k]; Z[k] = meas[(size_t)e * 7 + k]; }
        pg_edge(Ti, Tj, Z, re, with_jac ? ji : nullptr, jj);
        if (INFO) {
            double We[36];
            for (int k = 0; k < 36; ++k) We[k] = Winfo[(size_t)k * n_edges + e];
            pg_whiten_cols(We, re, 1, 1);
            if (with_jac) { pg_whiten_cols(We, ji, 6, 6); pg_whiten_cols(We, jj, 6, 6); }
        }
        for (int k = 0; k < 6; ++k) c += re[k] * re[k];
        if (ROBUST) {
            const int kind = lkind[e];
            const double sc = lscale[e];
            if (kind != STBA_LOSS_TRIVIAL || sc != 1.0) {
                const double s = c;
                double rho[3];
                robust_loss(kind, la[e], lb[e], s, rho);
                for (int k = 0; k < 3; ++k) rho[k] *= sc;
                c = rho[0];
                const double sq = sqrt(rho[1]);
                double rs = sq, ak = 0.0;                     // residual scaling, alpha / s
                if (s != 0.0 && rho[2] > 0.0) {
                    const double alpha = 1.0 - sqrt(1.0 + 2.0 * s * rho[2] / rho[1]);
                    rs = sq / (1.0 - alpha);
                    ak = alpha / s;
                }
                if (with_jac) { pg_correct_cols(re, ji, sq, ak); pg_correct_cols(re, jj, sq, ak); }
                for (int k = 0; k < 6; ++k) re[k] *= rs;
            }
        }
        if (r) for (int k = 0; k < 6; ++k) r[(size_t)e * 6 + k] = re[k];
        if (with_jac) {
            const bool fi = fixed && fixed[i], fj = fixed && fixed[j];
            for (int k = 0; k < 36; ++k) { ji[k] = fi ? 0.0 : ji[k]; jj[k] = fj ? 0.0 : jj[k]; Ji[(size_t)k * n_edges + e] = ji[k]; Jj[(size_t)k * n_edges + e] = jj[k]; }
            // what this edge adds to its two nodes' gradient and diagonal block, 27 doubles per end {J^T r (6), upper triangle of J^T J (21)}:
            // pg_gather_blocks_kernel sums a node's ends in a fixed order -- no atomics (the scatter with 42 FP64 atomics per edge
            // end took 156 us per linearisation at C4, 9 % of an LM iteration; rocprofv3, profiles/r4_b_c4_kernel_stats.csv)
            if (contrib) {
                for (int side = 0; side < 2; ++side) {
                    const double* J = side ? jj : ji;
                    double* out = contrib + ((size_t)e * 2 + side) * 28;
                    int w = 0;
                    for (int a = 0; a < 6; ++a) {
                        double sg = 0.0;
                        for (int k = 0; k < 6; ++k) sg += J[k * 6 + a] * re[k];
                        out[w++] = sg;
                    }
                    for (int a = 0; a < 6; ++a)
                        for (int b = a; b < 6; ++b) {
                            double h = 0.0;
                            for (int k = 0; k < 6; ++k) h += J[k * 6 + a] * J[k * 6 + b];
                            out[w++] = h;
                        }
                    out[27] = 0.0;
                }
            }
        }
    }
    double out2[2];
    block_sum2(c, 0.0, out2);
    if (threadIdx.x == 0) partial[blockIdx.x] = out2[0];
}

// ---- per-edge weights: what the caller gives ([m][36] row-major) -> the component-major array the linearisation reads
// One edge per lane.  sqrt_form = 0: `in` holds an information matrix Omega_e (symmetric positive definite; the lower triangle is
// factored), Omega = L L^T by an unblocked Cholesky in double-double, W_e = L^T rounded to FP64 (information6_factor, dd6.hpp: the
// one the bundle adjustment's factor setters call on the host).  sqrt_form = 1: `in` holds W_e itself, which is only transposed into
// the component-major array.  A non-finite entry anywhere in the 36, or a pivot that is not a positive finite number, refuses the
// edge: the smallest such edge index ends up in *bad (which the host set to INT_MAX), and the host throws the whole array away.
__global__ __launch_bounds__(256) void pg_information_kernel(int n_edges, const double* __restrict__ in, int sqrt_form,
                                                             double* __restrict__ Wout, int* __restrict__ bad) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    double A[36];
    bool ok = true;
    for (int k = 0; k < 36; ++k) { A[k] = in[(size_t)e * 36 + k]; ok = ok && isfinite(A[k]); }
    double Wl[36];
    if (sqrt_form) {
        for (int k = 0; k < 36; ++k) Wl[k] = A[k];
    } else {
        ok = ok && information6_factor(A, Wl);
    }
    if (!ok) { atomicMin(bad, e); return; }
    for (int k = 0; k < 36; ++k) Wout[(size_t)k * n_edges + e] = Wl[k];
}

// gradient and diagonal blocks: g_i += Ji^T r, Hd_i += Ji^T Ji (same for j), FP64 atomics
__global__ __launch_bounds__(256) void pg_accumulate_kernel(int n_edges, const int* __restrict__ ei, const int* __restrict__ ej,
                                                            const double* __restrict__ r, const double* __restrict__ Ji,
                                                            const double* __restrict__ Jj, double* __restrict__ g,
                                                            double* __restrict__ Hd) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int e = gid >> 1, side = gid & 1;
    if (e >= n_edges) return;
    const int node = side ? ej[e] : ei[e];
    const double* J = (side ? Jj : Ji) + e;
    const double* re = r + (size_t)e * 6;
    double Jl[36], rl[6];
    bool any = false;
    for (int k = 0; k < 36; ++k) { Jl[k] = J[(size_t)k * n_edges]; any |= (Jl[k] != 0.0); }
    if (!any) return;   // constant node
    for (int k = 0; k < 6; ++k) rl[k] = re[k];
    for (int a = 0; a < 6; ++a) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += Jl[k * 6 + a] * rl[k];
        unsafeAtomicAdd(&g[(size_t)node * 6 + a], s);
        for (int b = 0; b <= a; ++b) {
            double h = 0.0;
            for (int k = 0; k < 6; ++k) h += Jl[k * 6 + a] * Jl[k * 6 + b];
            unsafeAtomicAdd(&Hd[(size_t)node * 36 + a * 6 + b], h);
            if (b != a) unsafeAtomicAdd(&Hd[(size_t)node * 36 + b * 6 + a], h);
        }
    }
}

// gradient and diagonal blocks of a node = sum over its edge ends of the 27 doubles the linearise kernel left per end (fixed order: no
// atomics, same bits every run).  Eight lanes per node, one end each per trip, a butterfly over the eight lanes.
__global__ __launch_bounds__(PG_NT) void pg_gather_blocks_kernel(int n, const int* __restrict__ node_start, const int* __restrict__ end_code,
                                                                const double* __restrict__ contrib, double* __restrict__ g, double* __restrict__ Hd) {
    const int t = threadIdx.x, nl = t >> 3, k = t & 7;
    const int node = blockIdx.x * PG_NPW + nl;
    double acc[27];
    for (int q = 0; q < 27; ++q) acc[q] = 0.0;
    if (node < n) {
        const int e1 = node_start[node + 1];
        for (int c = node_start[node] + k; c < e1; c += 8) {
            const double2* src = reinterpret_cast<const double2*>(contrib + (size_t)end_code[c] * 28);
            for (int q = 0; q < 13; ++q) { const double2 v = src[q]; acc[2 * q] += v.x; acc[2 * q + 1] += v.y; }
            acc[26] += src[13].x;
        }
    }
    for (int q = 0; q < 27; ++q) {
        acc[q] += __shfl_xor(acc[q], 1, 8);
        acc[q] += __shfl_xor(acc[q], 2, 8);
        acc[q] += __shfl_xor(acc[q], 4, 8);
    }
    if (node < n && k < 6) {
        // row k of the symmetric block from the packed upper triangle: entry (a, b), a <= b, at 6 + a (13 - a) / 2 + (b - a)
        double gk = 0.0, row[6];
        for (int a = 0; a < 6; ++a) if (a == k) gk = acc[a];
        for (int b = 0; b < 6; ++b) {
            double v = 0.0;
            for (int a = 0; a < 6; ++a) {
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                if (a == k) v = acc[6 + lo * (13 - lo) / 2 + (hi - lo)];
            }
            row[b] = v;
        }
        g[(size_t)node * 6 + k] = gk;
        for (int b = 0; b < 6; ++b) Hd[(size_t)node * 36 + k * 6 + b] = row[b];
    }
}

double host_sum(hipStream_t st, const double* dev, int n, int stride, int off, std::vector<double>& buf) {
    buf.resize((size_t)n * stride);
    (void)hipMemcpyAsync(buf.data(), dev, buf.size() * sizeof(double), hipMemcpyDeviceToHost, st);
    (void)hipStreamSynchronize(st);
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += buf[(size_t)k * stride + off];
    return s;
}

// sum of a host scalar across ranks (through one device double and the hook)
int pg_sum_ranks(stba_pg* g, double* v) {
    if (!g->ar) return STBA_OK;
    STBA_HIP(hipMemcpyAsync(g->scalar, v, sizeof(double), hipMemcpyHostToDevice, g->st));
    STBA_TRY(pg_hook(g, g->scalar, 1));
    STBA_HIP(hipMemcpyAsync(v, g->scalar, sizeof(double), hipMemcpyDeviceToHost, g->st));
    STBA_HIP(hipStreamSynchronize(g->st));
    return STBA_OK;
}

}  // namespace

int pg_linearize(stba_pg* g, int which, bool jac, const double* trial_x) {
    // (an engine that holds square-root information runs a whitening instantiation, one that holds a loss table a robust one, every
    // other one the kernel without either)
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, g->poses[which], g->ei, g->ej,
                           g->meas, g->fixed, jac ? 1 : 0, jac ? g->r : nullptr, g->Ji, g->Jj, g->part_e, jac ? g->contrib : nullptr,
                           (const double*)g->Winfo, (const int*)g->loss_kind, (const double*)g->loss_a, (const double*)g->loss_b,
                           (const double*)g->loss_scale);
    };
    if (g->loss_kind) { if (g->Winfo) launch(pg_linearize_kernel<true, true>); else launch(pg_linearize_kernel<false, true>); }
    else if (g->Winfo) launch(pg_linearize_kernel<true, false>);
    else launch(pg_linearize_kernel<false, false>);
    pg_prior_linearize(g, g->poses[which], jac, trial_x);
    STBA_HIP(hipGetLastError());
    if (jac) g->bend_valid = false;
    return STBA_OK;
}

// gradient | diagonal blocks of the last pg_linearize(jac), gathered per node; then the priors' terms on top
void pg_gather_blocks(stba_pg* g) {
    hipLaunchKernelGGL(pg_gather_blocks_kernel, dim3(g->nb_nodes4), dim3(PG_NT), 0, g->st, g->n, g->node_start, g->end_code, g->contrib, g->g, g->Hd);
    pg_prior_gather(g, true);
}

}  // namespace stba

extern "C" {

// the two setters of the per-edge weights: `in` [m][36] -> a NEW component-major array on the device; only a call that succeeds
// swaps it in (a refused one leaves the engine with the weights it had), NULL releases the array
static int pg_set_weights(stba_pg* g, const double* in, int sqrt_form, const char* who) {
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": null engine");
    DevBuf<double> Wnew;
    if (in) {
        const size_t cnt = (size_t)g->m * 36;
        DevBuf<double> stage;
        DevBuf<int> bad;
        int bad_h = INT_MAX;
        STBA_TRY(Wnew.alloc(cnt)); STBA_TRY(stage.alloc(cnt)); STBA_TRY(bad.alloc(1));
        if (upload(stage, in, cnt, g->st) != STBA_OK || upload(bad, &bad_h, 1, g->st) != STBA_OK)
            return fail(STBA_ERR_HIP, std::string(who) + ": upload failed");
        hipLaunchKernelGGL(pg_information_kernel, dim3(g->nb_edges), dim3(256), 0, g->st, g->m, (const double*)stage, sqrt_form, Wnew.get(), bad.get());
        if (hipGetLastError() != hipSuccess || download(&bad_h, bad, 1, g->st) != STBA_OK || hipStreamSynchronize(g->st) != hipSuccess)
            return fail(STBA_ERR_HIP, std::string(who) + ": the conversion kernel failed");
        if (bad_h != INT_MAX)
            return sqrt_form ? fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": edge " + std::to_string(bad_h) + ": the square-root information has an entry that is not finite")
                             : fail(STBA_ERR_NOT_POSITIVE_DEFINITE, std::string(who) + ": edge " + std::to_string(bad_h) + ": the information matrix is not positive definite (or has an entry that is not finite)");
    }
    // (nothing of the engine may still be reading the old array or what was linearised with it: the move below frees it)
    STBA_HIP(hipStreamSynchronize(g->st));
    STBA_TRY(g->job.quiesce());
    g->Winfo = std::move(Wnew);
    pg_invalidate_linearisation(g);
    return STBA_OK;
}

int stba_pg_set_information(stba_pg* g, const double* information) { return pg_set_weights(g, information, 0, "stba_pg_set_information"); }
int stba_pg_set_sqrt_information(stba_pg* g, const double* sqrt_information) { return pg_set_weights(g, sqrt_information, 1, "stba_pg_set_sqrt_information"); }
int stba_pg_has_information(const stba_pg* g, int* has) {
    if (!g || !has) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    *has = g->Winfo ? 1 : 0;
    return STBA_OK;
}

// the per-edge loss table: checked on the host BEFORE anything is replaced (a refused call leaves the engine with the table it had),
// then uploaded into NEW arrays that are swapped in; kind == NULL releases the table
int stba_pg_set_loss(stba_pg* g, const int* kind, const double* a, const double* b, const double* scale) {
    const char* who = "stba_pg_set_loss";
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": null engine");
    DevBuf<int> k_new;
    DevBuf<double> a_new, b_new, s_new;
    if (kind) {
        const size_t m = (size_t)g->m;
        std::vector<double> ha, hb, hs;
        STBA_TRY(loss_table_check(who, "edge", m, kind, a, b, scale, ha, hb, hs));
        STBA_TRY(k_new.alloc(m)); STBA_TRY(a_new.alloc(m)); STBA_TRY(b_new.alloc(m)); STBA_TRY(s_new.alloc(m));
        if (upload(k_new, kind, m, g->st) != STBA_OK || upload(a_new, ha.data(), m, g->st) != STBA_OK ||
            upload(b_new, hb.data(), m, g->st) != STBA_OK || upload(s_new, hs.data(), m, g->st) != STBA_OK ||
            hipStreamSynchronize(g->st) != hipSuccess)
            return fail(STBA_ERR_HIP, std::string(who) + ": upload failed");
    }
    // (nothing of the engine may still be reading the old table or what was linearised with it: the moves below free it)
    STBA_HIP(hipStreamSynchronize(g->st));
    STBA_TRY(g->job.quiesce());
    g->loss_kind = std::move(k_new); g->loss_a = std::move(a_new); g->loss_b = std::move(b_new); g->loss_scale = std::move(s_new);
    pg_invalidate_linearisation(g);
    return STBA_OK;
}

int stba_pg_has_loss(const stba_pg* g, int* has) {
    if (!g || !has) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    *has = g->loss_kind ? 1 : 0;
    return STBA_OK;
}

int stba_pg_evaluate(stba_pg* g, double* cost, double* r, double* Ji, double* Jj) {
    if (!g) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    STBA_TRY(pg_linearize(g, g->cur, true));
    std::vector<double> buf;
    double c2 = host_sum(g->st, g->part_e, pg_cost_slots(g), 1, 0, buf);      // (edges plus priors)
    STBA_TRY(pg_sum_ranks(g, &c2));
    if (cost) *cost = 0.5 * c2;
    if (r) STBA_HIP(hipMemcpyAsync(r, g->r, (size_t)g->m * 6 * sizeof(double), hipMemcpyDeviceToHost, g->st));
    // (the device keeps the Jacobians component-major, [36][m]; the caller gets them edge-major, [m][6][6])
    std::vector<double> ti, tj;
    if (Ji) { ti.resize((size_t)g->m * 36); STBA_HIP(hipMemcpyAsync(ti.data(), g->Ji, ti.size() * sizeof(double), hipMemcpyDeviceToHost, g->st)); }
    if (Jj) { tj.resize((size_t)g->m * 36); STBA_HIP(hipMemcpyAsync(tj.data(), g->Jj, tj.size() * sizeof(double), hipMemcpyDeviceToHost, g->st)); }
    STBA_HIP(hipStreamSynchronize(g->st));
    for (int k = 0; k < 36; ++k)
        for (int e = 0; e < g->m; ++e) {
            if (Ji) Ji[(size_t)e * 36 + k] = ti[(size_t)k * g->m + e];
            if (Jj) Jj[(size_t)e * 36 + k] = tj[(size_t)k * g->m + e];
        }
    return STBA_OK;
}

// measurement (bench.py --config c4): hipEvent-timed averages of the two kernels a solve is made of -- the residual +
// Jacobian kernel and one matrix-free product q = (J^T J + D) p (diagonal term + edge kernel) -- on the engine's stream
int stba_pg_time_kernels(stba_pg* g, int reps, double* ms_linearize, double* ms_matvec) {
    if (!g || reps <= 0 || !ms_linearize || !ms_matvec) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    DevEvent e0, e1, e2;
    STBA_TRY(e0.create()); STBA_TRY(e1.create()); STBA_TRY(e2.create());
    STBA_TRY(pg_linearize(g, g->cur, true));            // warm-up; also makes the Jacobians the products use
    // (a non-zero direction and damping -- the gradient of this linearisation, unit damping -- so that the product does the
    // atomics a real one does)
    STBA_HIP(hipMemsetAsync(g->g, 0, (size_t)g->n * 42 * sizeof(double), g->st));
    hipLaunchKernelGGL(pg_accumulate_kernel, dim3((2 * g->m + 255) / 256), dim3(256), 0, g->st, g->m, g->ei, g->ej, g->r, g->Ji, g->Jj, g->g, g->Hd);
    STBA_HIP(hipMemcpyAsync(g->p, g->g, (size_t)6 * g->n * sizeof(double), hipMemcpyDeviceToDevice, g->st));
    STBA_HIP(hipMemcpyAsync(g->d, g->g, (size_t)6 * g->n * sizeof(double), hipMemcpyDeviceToDevice, g->st));
    // the product as the one-rank solve runs it: the edge kernel (t_e, u_e = J_e^T t_e, |t_e|^2) -- the node kernel gathers u
    // while it updates x, r, z and is not a product kernel of its own
    pg_edge_product(g, g->p, g->part_c, nullptr);
    STBA_HIP(hipEventRecord(e0, g->st));
    for (int k = 0; k < reps; ++k) STBA_TRY(pg_linearize(g, g->cur, true));
    STBA_HIP(hipEventRecord(e1, g->st));
    for (int k = 0; k < reps; ++k) pg_edge_product(g, g->p, g->part_c, nullptr);
    STBA_HIP(hipEventRecord(e2, g->st));
    STBA_HIP(hipStreamSynchronize(g->st));
    float a = 0.f, b = 0.f;
    (void)hipEventElapsedTime(&a, e0, e1); (void)hipEventElapsedTime(&b, e1, e2);
    *ms_linearize = a / reps; *ms_matvec = b / reps;
    return STBA_OK;
}

}  // extern "C"
