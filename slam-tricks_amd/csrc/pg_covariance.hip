// pg_covariance.hip -- covariance of a pose graph on gfx950: columns of C = (J^T J)^-1 by a BATCHED preconditioned conjugate gradient.
//
//   C is the inverse of the undamped, unscaled Gauss-Newton matrix H = J^T J at the engine's current poses, in the engine's tangent
//   coordinates (pg_engine.hip: per node [rho, theta] of T <- T exp(delta)); constant nodes have zero rows and columns.  The six
//   columns of C that belong to node b solve H x = e_{6 b + k}; PGC_K = 64 such systems are solved at once.
//
//   layout     every vector of the solve (X R Z P Q) holds K columns per scalar row: [node][6][K].  The 64 lanes of a wave are the
//              64 columns, so every load and store of a vector is one contiguous 512-byte row, and everything that belongs to the
//              NODE -- its edge list, the 6x6 Jacobians, the block of the preconditioner -- is wave-uniform: read once, through
//              scalar loads, for all 64 columns.
//   product    Q = H P by node-gather: a wave takes a node, walks its edge ends through the engine's CSR (node_start / end_code /
//              end_rem) and sums J_self^T (J_self p_self + J_other p_other) in that order.  Every edge is visited from both ends;
//              no atomics, so the bits do not depend on arrival order.  The Jacobians are repacked edge-major ([m][72]: Ji | Jj)
//              once per call, so that a wave fetches them as a few wide scalar loads instead of 72 lines of the engine's
//              component-major layout.  A node that holds pose priors adds Hp_v p_v, Hp_v the summed J'^T J' of its priors (wave-uniform
//              like the Jacobians); the preconditioner's diagonal blocks hold the priors already.
//   PCG        K independent recurrences that share the three kernels of an iteration (product | update | direction): alpha, beta,
//              |r|^2 are per column, reduced over the nodes by per-workgroup partial rows [workgroup][K] that every workgroup adds up
//              in the same fixed order.  A column whose recurrence residual reaches the tolerance FREEZES (no more updates, p = 0),
//              hence a column's bits do not depend on which other columns share its batch.  The flag `done` lives on the device;
//              the host looks at a stamped block (common.hpp) every check_every iterations.
//   re-check   the recurrence's residual is not trusted: when every column is frozen, one more product gives the TRUE residual
//              e - H x of every column; columns above the tolerance restart from it (p = z = M r), within the iteration cap.
//   precond    M = blockdiag(H_ii)^-1, undamped (6x6 Gauss-Jordan as pg_precond_kernel's); zero for constant nodes.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "pg_covariance.hpp"

namespace stba {

namespace {

constexpr int PGC_K = 64;          // columns of a batch = lanes of a wave
constexpr int PGC_NT = 256;        // four waves
constexpr int PGC_NPV = 4;         // nodes per wave
constexpr int PGC_NPW = 4 * PGC_NPV;

// device-resident state of a batch.  Per-column values are double-buffered: the direction kernel of iteration k reads slot k & 1 and
// (its workgroup 0) writes the other one, so no workgroup reads what another one of the same kernel writes.
struct PgcCtrl {
    double rz[2][PGC_K];
    int frozen[2][PGC_K];
    double rr0[PGC_K];             // |e|^2: 1, or 0 for a column of the batch that is not used
    int col_node[PGC_K], col_k[PGC_K];
    int iters, done, hit_cap, bad;
    double rho;                    // largest true relative residual at the last re-check
};
enum { CX_ITERS = 0, CX_DONE = 1, CX_HIT_CAP = 2, CX_BAD = 3, CX_RHO = 4, CX_COUNT = 5 };

__device__ inline int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// column `lane` of the sum of nb partial rows: wave w adds rows w, w + 4, ... in order, the four waves are added in order
__device__ inline double pgc_sum_rows(const double* __restrict__ part, int nb, int lane, int w, double (*s)[PGC_K]) {
    double v = 0.0;
    for (int b = w; b < nb; b += 4) v += part[(size_t)b * PGC_K + lane];
    __syncthreads();
    s[w][lane] = v;
    __syncthreads();
    return (s[0][lane] + s[1][lane]) + (s[2][lane] + s[3][lane]);
}
// this workgroup's partial row from the four waves' sums
__device__ inline void pgc_store_row(double v, double* __restrict__ part, int lane, int w, double (*s)[PGC_K]) {
    __syncthreads();
    s[w][lane] = v;
    __syncthreads();
    if (w == 0) part[(size_t)blockIdx.x * PGC_K + lane] = (s[0][lane] + s[1][lane]) + (s[2][lane] + s[3][lane]);
}

// Jacobians edge-major: Jp[e][0..36) = Ji, [36..72) = Jj (row-major 6x6), from the engine's component-major [36][m]
__global__ __launch_bounds__(256) void pgc_pack_kernel(int m, const double* __restrict__ Ji, const double* __restrict__ Jj, double* __restrict__ Jp) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)m * 72) return;
    const int e = (int)(idx / 72), k = (int)(idx % 72);
    Jp[idx] = k < 36 ? Ji[(size_t)k * m + e] : Jj[(size_t)(k - 36) * m + e];
}

// M_i = Hd_i^-1: Gauss-Jordan without pivoting on the undamped SPD block (the elimination of pg_precond_kernel, zero damping);
// a constant node, or a block with a pivot that is not positive, gives a zero block
__global__ __launch_bounds__(256) void pgc_block_inverse_kernel(int n, const double* __restrict__ Hd, const unsigned char* __restrict__ fixed,
                                                                double* __restrict__ Minv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double A[36], B[36];
    for (int k = 0; k < 36; ++k) { A[k] = Hd[(size_t)i * 36 + k]; B[k] = 0.0; }
    for (int a = 0; a < 6; ++a) B[a * 7] = 1.0;
    bool ok = !(fixed && fixed[i]);
    for (int c = 0; c < 6 && ok; ++c) {
        if (!(A[c * 7] > 0.0)) { ok = false; break; }
        const double inv = 1.0 / A[c * 7];
        for (int k = 0; k < 6; ++k) { A[c * 6 + k] *= inv; B[c * 6 + k] *= inv; }
        for (int rr = 0; rr < 6; ++rr) {
            if (rr == c) continue;
            const double f = A[rr * 6 + c];
            for (int k = 0; k < 6; ++k) { A[rr * 6 + k] -= f * A[c * 6 + k]; B[rr * 6 + k] -= f * B[c * 6 + k]; }
        }
    }
    for (int k = 0; k < 36; ++k) Minv[(size_t)i * 36 + k] = ok ? B[k] : 0.0;
}

// Q = H P and the partial rows of p^T q.  A wave per node (four nodes in turn), a lane per column.
__global__ __launch_bounds__(PGC_NT) void pgc_product_kernel(int n, const int* __restrict__ node_start, const int* __restrict__ end_code,
                                                             const int* __restrict__ end_rem, const double* __restrict__ Jp,
                                                             const int* __restrict__ node_slot, const double* __restrict__ Hp,
                                                             const double* __restrict__ P, double* __restrict__ Q,
                                                             double* __restrict__ part_pq, const PgcCtrl* __restrict__ ctrl, int obey_done) {
    if (obey_done && ctrl->done) return;
    __shared__ double s[4][PGC_K];
    const int lane = threadIdx.x & 63, w = wave_id();
    double acc = 0.0;
    for (int t = 0; t < PGC_NPV; ++t) {
        const int v = blockIdx.x * PGC_NPW + w * PGC_NPV + t;          // wave-uniform
        if (v >= n) break;
        double ps[6], q[6];
        for (int r = 0; r < 6; ++r) { ps[r] = P[((size_t)v * 6 + r) * PGC_K + lane]; q[r] = 0.0; }
        const int c0 = node_start[v], c1 = node_start[v + 1];
        for (int c = c0; c < c1; ++c) {
            const int code = end_code[c], o = end_rem[c];
            const double* __restrict__ Js = Jp + (size_t)(code >> 1) * 72 + (code & 1) * 36;
            const double* __restrict__ Jo = Jp + (size_t)(code >> 1) * 72 + ((code & 1) ^ 1) * 36;
            double po[6], te[6];
            for (int r = 0; r < 6; ++r) po[r] = P[((size_t)o * 6 + r) * PGC_K + lane];
            for (int a = 0; a < 6; ++a) {
                double sa = 0.0;
                for (int k = 0; k < 6; ++k) sa += Js[a * 6 + k] * ps[k];
                for (int k = 0; k < 6; ++k) sa += Jo[a * 6 + k] * po[k];
                te[a] = sa;
            }
            for (int k = 0; k < 6; ++k) {
                double sk = 0.0;
                for (int a = 0; a < 6; ++a) sk += Js[a * 6 + k] * te[a];
                q[k] += sk;
            }
        }
        // (node pose priors: the node's summed block, behind its edge ends; node_slot null: the engine holds none)
        const int slot = node_slot ? node_slot[v] : -1;
        if (slot >= 0) {
            const double* __restrict__ H = Hp + (size_t)slot * 36;
            for (int k = 0; k < 6; ++k) {
                double sk = 0.0;
                for (int a = 0; a < 6; ++a) sk += H[k * 6 + a] * ps[a];
                q[k] += sk;
            }
        }
        for (int r = 0; r < 6; ++r) { Q[((size_t)v * 6 + r) * PGC_K + lane] = q[r]; acc += ps[r] * q[r]; }
    }
    pgc_store_row(acc, part_pq, lane, w, s);
}

// start and re-check: r = e - q (q = H x; the start has x = 0 and no product), z = M r; partial rows of r.z and r.r
__global__ __launch_bounds__(PGC_NT) void pgc_residual_kernel(int n, int first, const PgcCtrl* __restrict__ ctrl, const double* __restrict__ Minv,
                                                              const double* __restrict__ Q, double* __restrict__ X, double* __restrict__ R,
                                                              double* __restrict__ Z, double* __restrict__ part_rz, double* __restrict__ part_rr) {
    __shared__ double s[4][PGC_K];
    const int lane = threadIdx.x & 63, w = wave_id();
    const int cn = ctrl->col_node[lane], ck = ctrl->col_k[lane];
    double arz = 0.0, arr = 0.0;
    for (int t = 0; t < PGC_NPV; ++t) {
        const int v = blockIdx.x * PGC_NPW + w * PGC_NPV + t;
        if (v >= n) break;
        const double* __restrict__ M = Minv + (size_t)v * 36;
        double r[6];
        for (int k = 0; k < 6; ++k) {
            const size_t at = ((size_t)v * 6 + k) * PGC_K + lane;
            r[k] = ((cn == v && ck == k) ? 1.0 : 0.0) - (first ? 0.0 : Q[at]);
            R[at] = r[k];
            if (first) X[at] = 0.0;
        }
        for (int k = 0; k < 6; ++k) {
            double z = 0.0;
            for (int j = 0; j < 6; ++j) z += M[k * 6 + j] * r[j];
            Z[((size_t)v * 6 + k) * PGC_K + lane] = z;
            arz += r[k] * z; arr += r[k] * r[k];
        }
    }
    pgc_store_row(arz, part_rz, lane, w, s);
    pgc_store_row(arr, part_rr, lane, w, s);
}

// alpha = r.z / p.q per column; x += alpha p, r -= alpha q, z = M r; partial rows of r.z and r.r.  A frozen column keeps x and r.
__global__ __launch_bounds__(PGC_NT) void pgc_update_kernel(int n, int slot, PgcCtrl* __restrict__ ctrl, int nb, const double* __restrict__ part_pq,
                                                            const double* __restrict__ Minv, const double* __restrict__ P,
                                                            const double* __restrict__ Q, double* __restrict__ X, double* __restrict__ R,
                                                            double* __restrict__ Z, double* __restrict__ part_rz, double* __restrict__ part_rr) {
    if (ctrl->done) return;
    __shared__ double s[4][PGC_K];
    const int lane = threadIdx.x & 63, w = wave_id();
    const double pq = pgc_sum_rows(part_pq, nb, lane, w, s);
    const bool frozen = ctrl->frozen[slot][lane] != 0;
    const bool bad = !frozen && !(pq > 0.0);                 // (also a NaN)
    const double alpha = (frozen || bad) ? 0.0 : ctrl->rz[slot][lane] / pq;
    if (blockIdx.x == 0 && bad) ctrl->bad = 1;               // (read by the direction kernel that follows)
    double arz = 0.0, arr = 0.0;
    for (int t = 0; t < PGC_NPV; ++t) {
        const int v = blockIdx.x * PGC_NPW + w * PGC_NPV + t;
        if (v >= n) break;
        const double* __restrict__ M = Minv + (size_t)v * 36;
        double r[6];
        for (int k = 0; k < 6; ++k) {
            const size_t at = ((size_t)v * 6 + k) * PGC_K + lane;
            r[k] = R[at];
            if (!frozen) {
                X[at] += alpha * P[at];
                r[k] -= alpha * Q[at];
                R[at] = r[k];
            }
        }
        for (int k = 0; k < 6; ++k) {
            double z = 0.0;
            for (int j = 0; j < 6; ++j) z += M[k * 6 + j] * r[j];
            if (!frozen) Z[((size_t)v * 6 + k) * PGC_K + lane] = z;
            arz += r[k] * z; arr += r[k] * r[k];
        }
    }
    pgc_store_row(arz, part_rz, lane, w, s);
    pgc_store_row(arr, part_rr, lane, w, s);
}

// beta = r.z / (r.z)_old per column, p = z + beta p (restart: p = z, every column thawed and judged anew); a column with
// |r| <= tol |e| freezes.  Workgroup 0 writes the other slot of the state, counts the iteration, decides `done` and
// hands {iterations, done, hit_cap, bad, rho} to the host with the stamp `seq`.
__global__ __launch_bounds__(PGC_NT) void pgc_direction_kernel(int n, int slot, int restart, int cap, double tol, double seq,
                                                               PgcCtrl* __restrict__ ctrl, int nb, const double* __restrict__ part_rz,
                                                               const double* __restrict__ part_rr, const double* __restrict__ Z,
                                                               double* __restrict__ P, double* __restrict__ exp) {
    __shared__ double s[4][PGC_K];
    __shared__ double pay[CX_COUNT];
    const int lane = threadIdx.x & 63, w = wave_id();
    // (`done` is written by workgroup 0 of this very kernel: a workgroup that starts late may see it and skip its p, which nobody
    // reads any more -- the re-check makes every p anew)
    if (!restart && ctrl->done) {
        if (blockIdx.x == 0 && w == 0) {
            pay[CX_ITERS] = ctrl->iters; pay[CX_DONE] = 1.0; pay[CX_HIT_CAP] = ctrl->hit_cap; pay[CX_BAD] = ctrl->bad; pay[CX_RHO] = ctrl->rho;
            stamped_store_wave(exp, pay, CX_COUNT, seq, lane);
        }
        return;
    }
    const double rzn = pgc_sum_rows(part_rz, nb, lane, w, s);
    const double rr = pgc_sum_rows(part_rr, nb, lane, w, s);
    const double rr0 = ctrl->rr0[lane];
    const bool was = !restart && ctrl->frozen[slot][lane] != 0;
    double rel = rr0 > 0.0 ? sqrt(rr / rr0) : 0.0;          // (the number the host reports as rho: one criterion)
    const bool frozen = was || rel <= tol;
    const double beta = restart ? 0.0 : rzn / ctrl->rz[slot][lane];
    for (int t = 0; t < PGC_NPV; ++t) {
        const int v = blockIdx.x * PGC_NPW + w * PGC_NPV + t;
        if (v >= n) break;
        for (int k = 0; k < 6; ++k) {
            const size_t at = ((size_t)v * 6 + k) * PGC_K + lane;
            if (frozen) { if (!was) P[at] = 0.0; }
            else P[at] = restart ? Z[at] : Z[at] + beta * P[at];
        }
    }
    if (blockIdx.x != 0) return;
    if (w == 0) {
        ctrl->rz[slot ^ 1][lane] = rzn;
        ctrl->frozen[slot ^ 1][lane] = frozen ? 1 : 0;
        const bool all = __all(frozen ? 1 : 0) != 0;
        if (!(rel == rel)) rel = INFINITY;                 // (a NaN must not vanish in fmax)
        for (int o = 32; o > 0; o >>= 1) rel = fmax(rel, __shfl_xor(rel, o, 64));
        // (every lane computes and stores the same payload, so that each reads back its own stores; lane 0 writes the state)
        const int it = ctrl->iters + (restart ? 0 : 1);
        const int bad = ctrl->bad;
        int cap_hit = ctrl->hit_cap;
        if (!all && !bad && it >= cap) cap_hit = 1;
        const int dn = (all || bad || cap_hit) ? 1 : 0;
        const double rho = restart ? rel : ctrl->rho;
        pay[CX_ITERS] = it; pay[CX_DONE] = dn; pay[CX_HIT_CAP] = cap_hit; pay[CX_BAD] = bad; pay[CX_RHO] = rho;
        if (lane == 0) { ctrl->rho = rho; ctrl->iters = it; ctrl->hit_cap = cap_hit; ctrl->done = dn; }
        stamped_store_wave(exp, pay, CX_COUNT, seq, lane);
    }
}

// out[dst[k]] = X[src[k]]: the requested blocks of a finished batch
__global__ __launch_bounds__(256) void pgc_extract_kernel(int count, const long long* __restrict__ src, const long long* __restrict__ dst,
                                                          const double* __restrict__ X, double* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < count) out[dst[k]] = X[src[k]];
}

// everything a call allocates, freed on every way out
struct Workspace {
    DevBuf<double> Jp, Minv, X, R, Z, P, Q, part, out;
    DevBuf<long long> src, dst;
    DevBuf<PgcCtrl> ctrl;
    MappedBuffer exp;
    DevEvent ev[2];
    ~Workspace() { exp.release(); }
};

struct Request {
    int n_pairs = 0;
    const int* a = nullptr; const int* b = nullptr;      // pairs, or
    int column_node = -1;                                // the whole columns of one node
};

int pgc_options(const stba_pg_covariance_options* in, stba_pg_covariance_options* o) {
    stba_pg_covariance_default_options(o);
    if (!in) return STBA_OK;
    if (in->struct_size < sizeof(size_t)) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_covariance: options without struct_size");
    const size_t have = in->struct_size;
    auto has = [&](size_t off, size_t sz) { return have >= off + sz; };
    if (has(offsetof(stba_pg_covariance_options, relative_tolerance), sizeof(double))) o->relative_tolerance = in->relative_tolerance;
    if (has(offsetof(stba_pg_covariance_options, max_iterations), sizeof(int))) o->max_iterations = in->max_iterations;
    if (has(offsetof(stba_pg_covariance_options, check_every), sizeof(int))) o->check_every = in->check_every;
    if (!(o->relative_tolerance > 0.0) || o->max_iterations < 0 || o->check_every < 1)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_covariance: relative_tolerance > 0, max_iterations >= 0 and check_every >= 1 are required");
    return STBA_OK;
}

// every connected component holds a constant node, or one ANCHORED by a pose prior (a structural check: a component anchored only by
// rank-deficient priors passes, and a singular H is then the conjugate gradient's to report)
int pgc_gauge(int n, int m, const int* ei, const int* ej, const unsigned char* fixed, const unsigned char* anchored) {
    int size = 0, first = 0;
    if (pg_gauge_fixed(n, m, ei, ej, fixed, &size, &first, anchored)) return STBA_OK;
    return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, "pose-graph covariance: a connected component of " + std::to_string(size) + " node" + (size == 1 ? "" : "s") +
                                                    " (first node " + std::to_string(first) + ") contains no constant node" +
                                                    (anchored ? " and no node with a pose prior" : "") + ": J^T J is singular (gauge freedom)");
}

int pgc_run(stba_pg* g, const Request& rq, const stba_pg_covariance_options* opt_in, double* out, stba_pg_covariance_summary* summary) {
    stba_pg_covariance_options opt;
    STBA_TRY(pgc_options(opt_in, &opt));
    PgCovGraph gr;
    pg_cov_graph(g, &gr);
    const int n = gr.n;
    // ---- refusals, before any device work
    if (rq.n_pairs == 0 && (rq.column_node < 0 || rq.column_node >= n))
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_covariance_columns: node " + std::to_string(rq.column_node) + " out of range (" + std::to_string(n) + " nodes)");
    for (int k = 0; k < rq.n_pairs; ++k)
        if (rq.a[k] < 0 || rq.a[k] >= n || rq.b[k] < 0 || rq.b[k] >= n)
            return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_covariance: pair " + std::to_string(k) + " (" + std::to_string(rq.a[k]) + ", " + std::to_string(rq.b[k]) +
                                                       ") names a node out of range (" + std::to_string(n) + " nodes)");
    if (gr.several_ranks) return fail(STBA_ERR_STATE, "stba_pg_covariance: not available with an all-reduce hook or communicator set (one rank only)");
    STBA_TRY(pgc_gauge(n, gr.m, gr.ei, gr.ej, gr.fixed, gr.anchored));
    auto is_fixed = [&](int v) { return gr.fixed && gr.fixed[v]; };
    int n_free = 0;
    for (int v = 0; v < n; ++v) n_free += is_fixed(v) ? 0 : 1;
    const int cap = opt.max_iterations > 0 ? opt.max_iterations : 6 * n_free;

    // ---- the distinct free nodes whose columns are wanted, ascending; column c of the request = (nodes[c / 6], c % 6)
    std::vector<int> nodes;
    const bool whole = rq.n_pairs == 0;
    if (whole) { if (!is_fixed(rq.column_node)) nodes.push_back(rq.column_node); }
    else {
        for (int k = 0; k < rq.n_pairs; ++k) if (!is_fixed(rq.a[k]) && !is_fixed(rq.b[k])) nodes.push_back(rq.b[k]);
        std::sort(nodes.begin(), nodes.end());
        nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
    }
    const size_t out_count = whole ? (size_t)36 * n : (size_t)36 * rq.n_pairs;
    stba_pg_covariance_summary sm;
    memset(&sm, 0, sizeof sm);
    std::vector<double> host_out(out_count, 0.0);
    const int n_cols = 6 * (int)nodes.size();
    if (n_cols > 0) {
        PgCovDevice dv;
        STBA_TRY(pg_cov_linearize(g, &dv));
        hipStream_t st = dv.st;
        Workspace ws;
        const size_t vec = (size_t)6 * n * PGC_K;
        const int nb = (n + PGC_NPW - 1) / PGC_NPW;
        STBA_TRY(ws.Jp.alloc((size_t)gr.m * 72)); STBA_TRY(ws.Minv.alloc((size_t)n * 36));
        STBA_TRY(ws.X.alloc(vec)); STBA_TRY(ws.R.alloc(vec)); STBA_TRY(ws.Z.alloc(vec)); STBA_TRY(ws.P.alloc(vec)); STBA_TRY(ws.Q.alloc(vec));
        STBA_TRY(ws.part.alloc((size_t)3 * nb * PGC_K)); STBA_TRY(ws.ctrl.alloc(1));
        if (!whole) { STBA_TRY(ws.out.alloc(out_count)); STBA_TRY(ws.src.alloc((size_t)36 * rq.n_pairs)); STBA_TRY(ws.dst.alloc((size_t)36 * rq.n_pairs)); }
        STBA_TRY(ws.exp.alloc((size_t)stamped_doubles(CX_COUNT)));
        STBA_TRY(ws.ev[0].create()); STBA_TRY(ws.ev[1].create());
        double* part_pq = ws.part; double* part_rz = ws.part + (size_t)nb * PGC_K; double* part_rr = ws.part + (size_t)2 * nb * PGC_K;
        STBA_HIP(hipEventRecord(ws.ev[0], st));
        hipLaunchKernelGGL(pgc_pack_kernel, dim3((unsigned)(((size_t)gr.m * 72 + 255) / 256)), dim3(256), 0, st, gr.m, dv.Ji, dv.Jj, ws.Jp);
        hipLaunchKernelGGL(pgc_block_inverse_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, dv.Hd, dv.fixed, ws.Minv);
        STBA_HIP(hipGetLastError());
        // pairs grouped by the column node, so that a batch finds its blocks
        std::vector<int> order;
        if (!whole) {
            order.resize((size_t)rq.n_pairs);
            std::iota(order.begin(), order.end(), 0);
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return rq.b[x] < rq.b[y]; });
        }
        const double tol = opt.relative_tolerance;
        const int chunk = opt.check_every;
        double seq = 0.0;
        double px[CX_COUNT];
        size_t next_pair = 0;
        for (int c0 = 0; c0 < n_cols; c0 += PGC_K) {
            const int c1 = std::min(n_cols, c0 + PGC_K);
            PgcCtrl hc;
            memset(&hc, 0, sizeof hc);
            for (int c = 0; c < PGC_K; ++c) {
                const bool used = c0 + c < c1;
                hc.col_node[c] = used ? nodes[(size_t)(c0 + c) / 6] : -1;
                hc.col_k[c] = used ? (c0 + c) % 6 : 0;
                hc.rr0[c] = used ? 1.0 : 0.0;
            }
            STBA_HIP(hipMemcpyAsync(ws.ctrl, &hc, sizeof hc, hipMemcpyHostToDevice, st));
            STBA_HIP(hipStreamSynchronize(st));          // (hc is a local of this loop; also: the last batch is over before its block is zeroed)
            ws.exp.zero();
            seq = 0.0;
            int slot = 0;
            auto direction = [&](int restart) {
                seq += 1.0;
                hipLaunchKernelGGL(pgc_direction_kernel, dim3(nb), dim3(PGC_NT), 0, st, n, slot, restart, cap, tol, seq, ws.ctrl, nb, part_rz, part_rr, ws.Z, ws.P, ws.exp.dev);
                slot ^= 1;
            };
            auto wait_for = [&](double want) -> int {
                return stamped_wait(ws.exp.host, CX_COUNT, [want](double s) { return s >= want; }, px, hip_stream_state(st), "pose graph covariance", 120.0);
            };
            hipLaunchKernelGGL(pgc_residual_kernel, dim3(nb), dim3(PGC_NT), 0, st, n, 1, ws.ctrl, ws.Minv, ws.Q, ws.X, ws.R, ws.Z, part_rz, part_rr);
            direction(1);
            STBA_HIP(hipGetLastError());
            STBA_TRY(wait_for(seq));
            for (;;) {
                // ---- the recurrences, check_every iterations per look; the host looks at the chunk BEFORE the one it has just enqueued
                // (the kernels of a chunk enqueued past `done` return at once)
                double prev = seq;
                while (px[CX_DONE] == 0.0) {
                    for (int k = 0; k < chunk; ++k) {
                        hipLaunchKernelGGL(pgc_product_kernel, dim3(nb), dim3(PGC_NT), 0, st, n, dv.node_start, dv.end_code, dv.end_rem, ws.Jp, dv.node_slot, dv.Hp, ws.P, ws.Q, part_pq, ws.ctrl, 1);
                        hipLaunchKernelGGL(pgc_update_kernel, dim3(nb), dim3(PGC_NT), 0, st, n, slot, ws.ctrl, nb, part_pq, ws.Minv, ws.P, ws.Q, ws.X, ws.R, ws.Z, part_rz, part_rr);
                        direction(0);
                    }
                    STBA_HIP(hipGetLastError());
                    STBA_TRY(wait_for(prev));
                    prev = seq;
                }
                STBA_TRY(wait_for(seq));        // (everything enqueued has run: the slot the host tracks is the device's)
                char msg[256];
                if (px[CX_BAD] != 0.0) {
                    snprintf(msg, sizeof msg, "stba_pg_covariance: p^T H p <= 0 after %d iterations (last true relative residual %.3e): J^T J is not positive definite",
                             (int)px[CX_ITERS], px[CX_RHO]);
                    return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, msg);
                }
                // ---- the true residual e - H x of every column; columns above the tolerance go on from it
                hipLaunchKernelGGL(pgc_product_kernel, dim3(nb), dim3(PGC_NT), 0, st, n, dv.node_start, dv.end_code, dv.end_rem, ws.Jp, dv.node_slot, dv.Hp, ws.X, ws.Q, part_pq, ws.ctrl, 0);
                hipLaunchKernelGGL(pgc_residual_kernel, dim3(nb), dim3(PGC_NT), 0, st, n, 0, ws.ctrl, ws.Minv, ws.Q, ws.X, ws.R, ws.Z, part_rz, part_rr);
                direction(1);
                STBA_HIP(hipGetLastError());
                STBA_TRY(wait_for(seq));
                if (!std::isfinite(px[CX_RHO])) {
                    snprintf(msg, sizeof msg, "stba_pg_covariance: the residual is not finite after %d iterations", (int)px[CX_ITERS]);
                    return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, msg);
                }
                if (px[CX_HIT_CAP] != 0.0 && px[CX_RHO] > tol) {
                    snprintf(msg, sizeof msg, "stba_pg_covariance: the conjugate gradients reached %d iterations (the cap) with a true relative residual of %.3e > %.3e",
                             (int)px[CX_ITERS], px[CX_RHO], opt.relative_tolerance);
                    return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, msg);
                }
                if (px[CX_DONE] != 0.0) break;          // (every column's true residual is within the tolerance -- or the cap was met by a batch that is)
            }
            ++sm.batches;
            sm.columns += c1 - c0;
            sm.iterations_total += (int)px[CX_ITERS];
            sm.max_iterations_in_a_batch = std::max(sm.max_iterations_in_a_batch, (int)px[CX_ITERS]);
            sm.max_relative_residual = std::max(sm.max_relative_residual, px[CX_RHO]);
            // ---- the requested blocks of this batch
            if (whole) {
                STBA_HIP(hipMemcpy2DAsync(host_out.data(), 6 * sizeof(double), ws.X, PGC_K * sizeof(double), 6 * sizeof(double), (size_t)6 * n, hipMemcpyDeviceToHost, st));
            } else {
                std::vector<long long> src, dst;
                const int node_lo = nodes[(size_t)c0 / 6], node_hi = nodes[(size_t)(c1 - 1) / 6];
                // (a node's six columns may lie in two batches: every batch takes the columns it holds)
                size_t p = next_pair;
                while (p < order.size() && rq.b[order[p]] < node_lo) ++p;
                next_pair = p;
                for (; p < order.size() && rq.b[order[p]] <= node_hi; ++p) {
                    const int pr = order[p], a = rq.a[pr], b = rq.b[pr];
                    if (is_fixed(a) || is_fixed(b)) continue;
                    const int cb = 6 * (int)(std::lower_bound(nodes.begin(), nodes.end(), b) - nodes.begin());
                    for (int k = 0; k < 6; ++k) {
                        if (cb + k < c0 || cb + k >= c1) continue;
                        for (int r = 0; r < 6; ++r) {
                            src.push_back(((long long)a * 6 + r) * PGC_K + (cb + k - c0));
                            dst.push_back((long long)pr * 36 + r * 6 + k);
                        }
                    }
                }
                if (!src.empty()) {
                    STBA_HIP(hipMemcpyAsync(ws.src, src.data(), src.size() * sizeof(long long), hipMemcpyHostToDevice, st));
                    STBA_HIP(hipMemcpyAsync(ws.dst, dst.data(), dst.size() * sizeof(long long), hipMemcpyHostToDevice, st));
                    hipLaunchKernelGGL(pgc_extract_kernel, dim3((unsigned)((src.size() + 255) / 256)), dim3(256), 0, st, (int)src.size(), ws.src, ws.dst, ws.X, ws.out);
                    STBA_HIP(hipGetLastError());
                    STBA_HIP(hipStreamSynchronize(st));      // (src / dst are locals)
                }
            }
        }
        if (!whole) {
            // (blocks of pairs with a constant node were never written on the device: they stay zero in host_out)
            std::vector<double> got(out_count);
            STBA_HIP(hipMemcpyAsync(got.data(), ws.out, out_count * sizeof(double), hipMemcpyDeviceToHost, st));
            STBA_HIP(hipStreamSynchronize(st));
            for (int k = 0; k < rq.n_pairs; ++k)
                if (!is_fixed(rq.a[k]) && !is_fixed(rq.b[k])) memcpy(&host_out[(size_t)k * 36], &got[(size_t)k * 36], 36 * sizeof(double));
        }
        STBA_HIP(hipEventRecord(ws.ev[1], st));
        STBA_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        STBA_HIP(hipEventElapsedTime(&ms, ws.ev[0], ws.ev[1]));
        sm.device_ms = ms;
    }
    memcpy(out, host_out.data(), out_count * sizeof(double));
    if (summary) {
        const size_t have = summary->struct_size;
        if (have >= sizeof(size_t)) {
            sm.struct_size = have;
            memcpy(summary, &sm, std::min(have, sizeof sm));
        }
    }
    return STBA_OK;
}

}  // namespace
}  // namespace stba

using namespace stba;

extern "C" {

void stba_pg_covariance_default_options(stba_pg_covariance_options* o) {
    if (!o) return;
    o->struct_size = sizeof(stba_pg_covariance_options);
    o->relative_tolerance = 1e-12;
    o->max_iterations = 0;
    o->check_every = 4;
}

int stba_pg_gauge_check(int n_nodes, int n_edges, const int* edge_i, const int* edge_j, const unsigned char* node_fixed) {
    if (n_nodes <= 0 || n_edges < 0 || (n_edges > 0 && (!edge_i || !edge_j))) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_gauge_check: null or empty input");
    for (int e = 0; e < n_edges; ++e)
        if (edge_i[e] < 0 || edge_i[e] >= n_nodes || edge_j[e] < 0 || edge_j[e] >= n_nodes) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_gauge_check: bad edge");
    return pgc_gauge(n_nodes, n_edges, edge_i, edge_j, node_fixed, nullptr);
}

int stba_pg_covariance(stba_pg* pg, int n_pairs, const int* node_a, const int* node_b, const stba_pg_covariance_options* opt, double* out,
                       stba_pg_covariance_summary* summary) {
    if (!pg || n_pairs <= 0 || !node_a || !node_b || !out) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_covariance: null or empty argument");
    Request rq;
    rq.n_pairs = n_pairs; rq.a = node_a; rq.b = node_b;
    return pgc_run(pg, rq, opt, out, summary);
}

int stba_pg_covariance_columns(stba_pg* pg, int node, const stba_pg_covariance_options* opt, double* out, stba_pg_covariance_summary* summary) {
    if (!pg || !out) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_pg_covariance_columns: null argument");
    Request rq;
    rq.column_node = node;
    return pgc_run(pg, rq, opt, out, summary);
}

}  // extern "C"
