// dense_engine.hip -- the dense entry points of the C ABI (include/stba.h) that are no bundle adjustment: the SPD factorisation,
// solve and inverse on a matrix the caller holds (stba_cholesky_*, over dense_chol.hip and covariance.hip's inverse) with their
// timing entry points on a synthetic matrix, and the dense Levenberg-Marquardt loop over host callbacks (stba_dense_solve,
// stba_dense_covariance) with the kernel of its normal equations.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ba_kernels.hpp"
#include "lm_policy.hpp"

namespace stba {

// ===========================================================================================
// dense normal equations for the small problems: H = J^T J (n x n, n <= 256), g = J^T r
// one workgroup per (a, b-chunk): plain, these problems are tiny (6..129 unknowns)
// ===========================================================================================
__global__ __launch_bounds__(256) void dense_normal_kernel(int n_res, int n, const double* __restrict__ J,
                                                           const double* __restrict__ r, double* __restrict__ H,
                                                           int ldh, double* __restrict__ g) {
    // block (a): computes row a of H (lower part) and g[a]
    const int a = blockIdx.x;
    __shared__ double s[256];
    for (int b = 0; b <= a + 1; ++b) {     // b == a+1 -> gradient
        double v = 0.0;
        for (int i = threadIdx.x; i < n_res; i += 256) {
            const double ja = J[(size_t)i * n + a];
            v += ja * ((b <= a) ? J[(size_t)i * n + b] : r[i]);
        }
        s[threadIdx.x] = v;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (b <= a) H[(size_t)a * ldh + b] = s[0];
            else g[a] = s[0];
        }
        __syncthreads();
    }
}

int launch_dense_normal(int n_res, int n, const double* J, const double* r, double* H, int ldh, double* g,
                        hipStream_t st) {
    hipLaunchKernelGGL(dense_normal_kernel, dim3(n), dim3(256), 0, st, n_res, n, J, r, H, ldh, g);
    STBA_HIP(hipGetLastError());
    return STBA_OK;
}

}  // namespace stba

using namespace stba;

extern "C" {

// ---------------------------------------------------------------------------------------------
// dense SPD solver entry points
// ---------------------------------------------------------------------------------------------
__global__ void synth_spd_kernel(double* A, int lda, int n) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)lda * lda) return;
    const int i = (int)(idx / lda), j = (int)(idx % lda);
    double v = 0.0;
    if (i < n && j < n) {
        const unsigned h = (unsigned)(i * 2654435761u) ^ (unsigned)(j * 40503u);
        const unsigned g = (unsigned)(j * 2654435761u) ^ (unsigned)(i * 40503u);
        v = ((double)((h ^ g) & 1023u) / 1024.0 - 0.5);   // symmetric in (i,j)
        if (i == j) v += (double)n;
    }
    A[idx] = v;
}

}  // extern "C"

namespace {

struct DenseWs {
    int n = 0, lda = 0;
    DevBuf<double> A, x, rhs;
    DevBuf<int> flag;
    hipStream_t st = nullptr;
    bool own = false;
    ~DenseWs() {          // (the stream is synchronised here; the buffers go behind it, with the members)
        if (st) { (void)hipStreamSynchronize(st); chol_forget_stream(st); }
        if (own && st) (void)hipStreamDestroy(st);
    }
    int init(int n_, void* stream) {
        n = n_; lda = chol_padded_dim(n);
        if (stream) st = reinterpret_cast<hipStream_t>(stream);
        else { STBA_HIP(hipStreamCreate(&st)); own = true; }
        STBA_TRY(A.alloc((size_t)lda * lda)); STBA_TRY(x.alloc((size_t)lda));
        STBA_TRY(rhs.alloc((size_t)lda)); STBA_TRY(flag.alloc(1));
        return STBA_OK;
    }
    // host A (n x n, lower used) -> padded device matrix
    int load(const double* hostA, const double* host_rhs) {
        STBA_HIP(hipMemsetAsync(A, 0, (size_t)lda * lda * sizeof(double), st));
        STBA_HIP(hipMemcpy2DAsync(A, (size_t)lda * sizeof(double), hostA, (size_t)n * sizeof(double),
                                  (size_t)n * sizeof(double), (size_t)n, hipMemcpyHostToDevice, st));
        STBA_HIP(hipMemsetAsync(rhs, 0, (size_t)lda * sizeof(double), st));
        if (host_rhs) STBA_TRY(upload(rhs, host_rhs, (size_t)n, st));
        return chol_prepare_padding_dev(A, lda, n, rhs, st);
    }
    // factor + solve of the system the host holds; synchronises the stream and hands back the pivot flag.  If the persistent
    // program gives up (CHOL_FLAG_TIMEOUT: not all of its workgroups were resident, the device is shared with another
    // process), the matrix is loaded again and the stage kernels -- which need nothing resident -- do the same job.
    int load_factor_solve(const double* hostA, const double* host_rhs, int* flag_h) {
        STBA_TRY(load(hostA, host_rhs));
        STBA_TRY(chol_factor_solve_dev(A, lda, n, x, flag, st));
        STBA_TRY(download(flag_h, flag, 1, st));
        STBA_HIP(hipStreamSynchronize(st));
        if (*flag_h == CHOL_FLAG_TIMEOUT) {
            chol_note_timeout();
            STBA_TRY(load(hostA, host_rhs));
            STBA_TRY(chol_factor_solve_stages(A, lda, n, x, flag, st));
            STBA_TRY(download(flag_h, flag, 1, st));
            STBA_HIP(hipStreamSynchronize(st));
        }
        return STBA_OK;
    }
    // the synthetic matrix of the timing entry points in place of a caller's (zero_rhs false: the right-hand side stays as it is)
    int synthesize(bool zero_rhs = true) {
        const size_t cnt = (size_t)lda * lda;
        hipLaunchKernelGGL(synth_spd_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, A, lda, n);
        if (zero_rhs) STBA_HIP(hipMemsetAsync(rhs, 0, (size_t)lda * sizeof(double), st));
        return chol_prepare_padding_dev(A, lda, n, rhs, st);
    }
};

// packed lower triangle (row i at i (i + 1) / 2) -> the full symmetric n x n matrix
void unpack_symmetric(const std::vector<double>& packed, int n, double* full) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) full[(size_t)i * n + j] = full[(size_t)j * n + i] = packed[(size_t)i * (i + 1) / 2 + j];
}

}  // namespace

extern "C" {

int stba_cholesky_factor(double* A, int n, void* hip_stream) {
    if (!A || n <= 0) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    STBA_TRY(require_device());
    DenseWs w;
    STBA_TRY(w.init(n, hip_stream));
    int flag_h = 0;
    STBA_TRY(w.load_factor_solve(A, nullptr, &flag_h));
    STBA_HIP(hipMemcpy2DAsync(A, (size_t)n * sizeof(double), w.A, (size_t)w.lda * sizeof(double),
                              (size_t)n * sizeof(double), (size_t)n, hipMemcpyDeviceToHost, w.st));
    STBA_HIP(hipStreamSynchronize(w.st));
    STBA_TRY(chol_flag_status(flag_h));
    if (flag_h) return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, "pivot " + std::to_string(flag_h));
    return STBA_OK;
}

int stba_cholesky_solve(const double* A, int n, double* bvec, void* hip_stream) {
    if (!A || !bvec || n <= 0) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    STBA_TRY(require_device());
    DenseWs w;
    STBA_TRY(w.init(n, hip_stream));
    int flag_h = 0;
    STBA_TRY(w.load_factor_solve(A, bvec, &flag_h));
    STBA_TRY(download(bvec, w.x, (size_t)n, w.st));
    STBA_HIP(hipStreamSynchronize(w.st));
    STBA_TRY(chol_flag_status(flag_h));
    if (flag_h) return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, "pivot " + std::to_string(flag_h));
    return STBA_OK;
}

// A^-1 through covariance.hip's cov_spd_inverse_packed -- the partial factorisation of [A .; I 0] behind every covariance and the
// pose graph's coarse operator -- on a matrix the caller holds: the seam its accuracy is tested through.  Nothing is written to
// Ainv or pivot_ratio unless the factorisation succeeded.
int stba_cholesky_inverse(const double* A, int n, double* Ainv, double* pivot_ratio, void* hip_stream) {
    if (!A || !Ainv || n <= 0) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    if (n > 4096) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_cholesky_inverse: limited to n = 4096");
    STBA_TRY(require_device());
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);      // (null: the default stream)
    const size_t np = (size_t)n * (n + 1) / 2;
    DevBuf<double> dA, sig;
    STBA_TRY(dA.alloc((size_t)n * n));
    STBA_TRY(sig.alloc(np));
    STBA_TRY(upload(dA, A, (size_t)n * n, st));
    double rc = 0.0;
    int piv = 0;
    STBA_TRY(cov_spd_inverse_packed(dA, n, n, nullptr, sig, &rc, &piv, st));
    if (piv) return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, "pivot " + std::to_string(piv));
    std::vector<double> packed(np);
    STBA_TRY(download(packed.data(), sig, np, st));
    STBA_HIP(hipStreamSynchronize(st));
    unpack_symmetric(packed, n, Ainv);
    if (pivot_ratio) *pivot_ratio = rc;
    return STBA_OK;
}

int stba_cholesky_time(int n, int reps, double* ms_avg, void* hip_stream) {
    if (n <= 0 || reps <= 0 || !ms_avg) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    STBA_TRY(require_device());
    DenseWs w;
    STBA_TRY(w.init(n, hip_stream));
    DevEvent e0, e1;
    STBA_TRY(e0.create()); STBA_TRY(e1.create());
    double total = 0.0;
    for (int k = 0; k < reps + 1; ++k) {
        STBA_TRY(w.synthesize());
        STBA_HIP(hipEventRecord(e0, w.st));
        STBA_TRY(chol_factor_solve_dev(w.A, w.lda, n, w.x, w.flag, w.st));
        STBA_HIP(hipEventRecord(e1, w.st));
        STBA_HIP(hipStreamSynchronize(w.st));
        float ms = 0.f;
        STBA_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (k > 0) total += ms;
    }
    *ms_avg = total / reps;
    return STBA_OK;
}

int stba_cholesky_schedule_model(int n, int n_xcd, int wg_per_xcd, double* makespan_us) {
    if (n <= 0 || n_xcd <= 0 || n_xcd > 16 || wg_per_xcd < 4 || !makespan_us) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    const int lda = ((n + 1 + 127) / 128) * 128;      // the padded system carries the right-hand side as one more row
    *makespan_us = chol_schedule_makespan(lda / 128, n_xcd, wg_per_xcd);
    return STBA_OK;
}

int stba_cholesky_timeout_count(void) { return chol_timeout_count(); }
int stba_cholesky_set_timeout_us(double us) {
    if (!(us >= 0.0)) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    chol_set_spin_limit_us(us);
    return STBA_OK;
}

int stba_cholesky_shard_model(int n, int n_gpus, int n_xcd, int wg_per_xcd, int rows_per_group, double hop_us, double link_gb_per_s,
                              double* makespan_us, double* cross_gpu_dependencies, double* remote_tiles_busiest_gpu) {
    if (n <= 0 || n_gpus < 1 || n_gpus > 32 || n_xcd <= 0 || n_xcd > 16 || wg_per_xcd < 4 || rows_per_group < 0 || hop_us < 0 ||
        !(link_gb_per_s > 0) || !makespan_us)
        return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    const int lda = ((n + 1 + 127) / 128) * 128;
    double out3[3];
    chol_shard_model(lda / 128, n_gpus, n_xcd, wg_per_xcd, rows_per_group, hop_us, 128.0 * 128.0 * 8.0 / (link_gb_per_s * 1e3), out3);
    *makespan_us = out3[0];
    if (cross_gpu_dependencies) *cross_gpu_dependencies = out3[1];
    if (remote_tiles_busiest_gpu) *remote_tiles_busiest_gpu = out3[2];
    return STBA_OK;
}

int stba_cholesky_shard_owner(int n_block_rows, int n_gpus, int rows_per_group, int* owner_gpu) {
    if (n_block_rows <= 0 || n_gpus < 1 || rows_per_group < 1 || !owner_gpu) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    for (int r = 0; r < n_block_rows; ++r) owner_gpu[r] = chol_shard_row_owner(r, n_gpus, rows_per_group);
    return STBA_OK;
}

int stba_cholesky_time_split(int n, int reps, double* ms_factor, double* ms_backward, void* hip_stream) {
    if (n <= 0 || reps <= 0 || !ms_factor || !ms_backward) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    STBA_TRY(require_device());
    DenseWs w;
    STBA_TRY(w.init(n, hip_stream));
    DevEvent e0, ep, e1, e2;
    STBA_TRY(e0.create()); STBA_TRY(ep.create()); STBA_TRY(e1.create()); STBA_TRY(e2.create());
    // ms_factor = the MEDIAN over the repetitions of the persistent kernel's own duration (an event right in front of it and one
    // right behind: what rocprofv3 reports for chol_mega_kernel; the flag reset in front, 5 us, is not in it) -- when a
    // factorisation went through the stage kernels instead (time-out fallback, cool-down) the whole of it, from e0
    std::vector<double> tf, tb;
    for (int k = 0; k < reps + 1; ++k) {
        STBA_TRY(w.synthesize());
        STBA_HIP(hipEventRecord(e0, w.st));
        STBA_HIP(hipEventRecord(ep, w.st));          // (re-recorded in front of the persistent kernel when that is what runs)
        STBA_TRY(chol_factor_solve_split(w.A, w.lda, n, w.x, w.flag, w.st, e1, ep));
        STBA_HIP(hipEventRecord(e2, w.st));
        STBA_HIP(hipStreamSynchronize(w.st));
        float a = 0.f, b = 0.f;
        STBA_HIP(hipEventElapsedTime(&a, ep, e1));
        STBA_HIP(hipEventElapsedTime(&b, e1, e2));
        if (k > 0) { tf.push_back(a); tb.push_back(b); }
    }
    auto median = [](std::vector<double>& v) { std::sort(v.begin(), v.end()); const size_t h = v.size() / 2; return (v.size() & 1) ? v[h] : 0.5 * (v[h - 1] + v[h]); };
    *ms_factor = median(tf);
    *ms_backward = median(tb);
    return STBA_OK;
}

int stba_cholesky_profile(int n, double* ms4, double* syrk_flops, double* syrk_flops_padded, int* syrk_launches,
                          void* hip_stream) {
    if (n <= 0 || !ms4) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    STBA_TRY(require_device());
    DenseWs w;
    STBA_TRY(w.init(n, hip_stream));
    STBA_TRY(w.synthesize());
    CholProfile prof;
    // warm-up pass inside, then the timed pass on a fresh matrix
    STBA_TRY(chol_factor_solve_dev(w.A, w.lda, n, w.x, w.flag, w.st));
    STBA_TRY(w.synthesize(false));
    // the profiled routine factors once un-timed (on this matrix) and once timed: re-synthesise between
    // is not possible from outside, so time a factorisation of the already-factored-then-refilled buffer:
    STBA_TRY(chol_factor_solve_profiled(w.A, w.lda, n, w.x, w.flag, w.st, &prof));
    ms4[0] = prof.ms_diag; ms4[1] = prof.ms_trsm; ms4[2] = prof.ms_syrk; ms4[3] = prof.ms_bwd;
    if (syrk_flops) *syrk_flops = prof.syrk_flops;
    if (syrk_flops_padded) *syrk_flops_padded = prof.syrk_flops_padded;
    if (syrk_launches) *syrk_launches = prof.syrk_launches;
    return STBA_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Dense LM problems: residual blocks evaluated by a host callback (the user's CostFunction::Evaluate), the damped normal equations
// solved on the device.  One loop (dense_lm) over two step providers:
//  - SmallDenseSteps, <= 32 local parameters (the reference's PnP call sites, its per-landmark triangulation, the bounds demo, the
//    curve fit): one kernel launch per step (small_dense.hip), no allocation, no copy and no synchronise per solve -- the published
//    workload of the reference is 0.12-0.22 ms per Solve() (st17-ceres/img/release.png), the general path took 3.5 ms;
//  - GeneralDenseSteps: normal equations on the device, damping and model change on the host, the dense Cholesky of DenseWs.
// A provider holds r and J (where the callback writes), g and dx of the last linearisation / step, and
//   linearize(radius): r and J hold the callback's output at x -- make g (and on the small path the step at `radius`);
//   step(radius, &model_change, &flag_ok): the step at `radius` for the current linearisation.
// ---------------------------------------------------------------------------------------------
namespace stba {
namespace {

struct SmallDenseSteps {
    static constexpr bool linearizes_failed_start = false;     // (a non-finite start cost: no device step, row 0's gradient is 0)
    const stba_lm_options& opt;
    const int n_res, n;
    SmallDenseWs* ws = nullptr;
    double *r = nullptr, *J = nullptr;
    double dx[SMALL_DENSE_MAX_N], g[SMALL_DENSE_MAX_N];
    double model_change = 0.0;
    int flag_h = 0;
    bool first = true, have_step = false;
    SmallDenseSteps(const stba_lm_options& o, int n_res_, int n_) : opt(o), n_res(n_res_), n(n_) {}
    ~SmallDenseSteps() { if (ws) small_dense_release(ws); }
    int init() {
        STBA_TRY(small_dense_acquire(&ws, n_res, n));
        r = small_dense_r(ws); J = small_dense_J(ws);
        return STBA_OK;
    }
    int run(bool relinearize, double radius) {     // (H + D) dx = -g on the device; g refreshed when relinearised
        const double *dxp = nullptr, *gp = nullptr;
        STBA_TRY(small_dense_step(ws, n_res, n, relinearize, first, opt.jacobi_scaling != 0, radius, opt.min_lm_diagonal,
                                  opt.max_lm_diagonal, &dxp, &gp, &model_change, &flag_h));
        first = false;
        for (int a = 0; a < n; ++a) { dx[a] = dxp[a]; g[a] = gp[a]; }
        return STBA_OK;
    }
    int linearize(double radius) {      // the next iteration's step rides along with the new linearisation
        STBA_TRY(run(true, radius));
        have_step = true;
        return STBA_OK;
    }
    int step(double radius, double* mc, bool* flag_ok) {
        if (!have_step) STBA_TRY(run(false, radius));
        have_step = false;
        *mc = model_change;
        *flag_ok = flag_h == 0;
        return STBA_OK;
    }
};

struct GeneralDenseSteps {
    static constexpr bool linearizes_failed_start = true;      // (a non-finite start cost: linearised all the same, row 0 has its gradient)
    const stba_lm_options& opt;
    const int n_res, n;
    DenseWs w;
    DevBuf<double> dJ, dr, dH, dg;
    std::vector<double> rv, Jv, H, Hd, gv, dxv, scale, dvec;
    double *r = nullptr, *J = nullptr, *g = nullptr, *dx = nullptr;
    bool first = true;
    GeneralDenseSteps(const stba_lm_options& o, int n_res_, int n_) : opt(o), n_res(n_res_), n(n_) {}
    int init() {
        STBA_TRY(w.init(n, nullptr));
        STBA_TRY(dJ.alloc((size_t)n_res * n)); STBA_TRY(dr.alloc((size_t)n_res));
        STBA_TRY(dH.alloc((size_t)n * n)); STBA_TRY(dg.alloc((size_t)n));
        rv.resize(n_res); Jv.resize((size_t)n_res * n); H.resize((size_t)n * n); Hd.resize((size_t)n * n);
        gv.resize(n); dxv.resize(n); scale.resize(n); dvec.resize(n);
        r = rv.data(); J = Jv.data(); g = gv.data(); dx = dxv.data();
        return STBA_OK;
    }
    int linearize(double) {     // H = J^T J, g = J^T r on the device; the Jacobi scale from the first linearisation
        STBA_TRY(upload(dJ, J, Jv.size(), w.st)); STBA_TRY(upload(dr, r, rv.size(), w.st));
        STBA_HIP(hipMemsetAsync(dH, 0, (size_t)n * n * sizeof(double), w.st));
        STBA_TRY(launch_dense_normal(n_res, n, dJ, dr, dH, n, dg, w.st));
        STBA_TRY(download(H.data(), dH, H.size(), w.st)); STBA_TRY(download(g, dg, gv.size(), w.st));
        STBA_HIP(hipStreamSynchronize(w.st));
        if (first)
            for (int a = 0; a < n; ++a) scale[a] = opt.jacobi_scaling ? 1.0 / (1.0 + std::sqrt(H[(size_t)a * n + a])) : 1.0;
        first = false;
        return STBA_OK;
    }
    int step(double radius, double* model_change, bool* flag_ok) {
        Hd = H;
        for (int a = 0; a < n; ++a) {
            const double s2 = scale[a] * scale[a];
            const double d = std::min(std::max(H[(size_t)a * n + a] * s2, opt.min_lm_diagonal), opt.max_lm_diagonal);
            dvec[a] = d / radius / s2;
            Hd[(size_t)a * n + a] += dvec[a];
            dx[a] = -g[a];
        }
        int flag_h = 0;
        STBA_TRY(w.load_factor_solve(Hd.data(), dx, &flag_h));
        STBA_TRY(download(dx, w.x, (size_t)n, w.st));
        STBA_HIP(hipStreamSynchronize(w.st));
        STBA_TRY(chol_flag_status(flag_h));
        *model_change = 0.0;
        *flag_ok = flag_h == 0;
        if (*flag_ok)
            for (int a = 0; a < n; ++a) *model_change += -0.5 * g[a] * dx[a] + 0.5 * dvec[a] * dx[a] * dx[a];
        return STBA_OK;
    }
};

template <class Steps>
int dense_lm(Steps& S, stba_residual_fn fn, stba_plus_fn plus, void* user, int n_params, int n, int n_res, double* x,
             const double* lower, const double* upper, const stba_lm_options& opt, stba_lm_summary* summary, double* trace,
             stba_iteration_callback cb, void* cb_user) {
    std::vector<double> xn((size_t)n_params), rn((size_t)n_res);
    stba_lm_summary s;
    memset(&s, 0, sizeof s);
    const double t_start = wall_s();
    const bool bounded = lower || upper;
    auto gmax_of = [&]() {
        double m = 0.0;
        for (int a = 0; a < n; ++a) {
            if (!bounded) m = std::max(m, std::fabs(S.g[a]));
            else {
                double y = x[a] - S.g[a];
                if (lower && y < lower[a]) y = lower[a];
                if (upper && y > upper[a]) y = upper[a];
                m = std::max(m, std::fabs(x[a] - y));
            }
        }
        return m;
    };
    auto norm_of = [&](const double* v, int k) { double q = 0; for (int a = 0; a < k; ++a) q += v[a] * v[a]; return std::sqrt(q); };

    if (fn(user, x, S.r, S.J) != 0) return fail(STBA_ERR_CALLBACK, "residual callback failed");
    double cost = 0.0;
    for (int i = 0; i < n_res; ++i) cost += S.r[i] * S.r[i];
    cost *= 0.5;
    s.initial_cost = cost;
    TrustRegion region(opt);
    double x_norm = norm_of(x, n_params), gmax = 0.0;
    if (std::isfinite(cost) || Steps::linearizes_failed_start) {
        STBA_TRY(S.linearize(region.radius));
        gmax = gmax_of();
    }
    trace_start(trace, cost, gmax, region.radius);
    int iter = 0;
    bool done = false;
    s.termination_type = STBA_NO_CONVERGENCE; s.termination_reason = STBA_TERM_MAX_ITER;
    if (!std::isfinite(cost)) { s.termination_type = STBA_FAILURE; s.termination_reason = STBA_TERM_SOLVER_FAIL; done = true; }    // (Ceres: initial evaluation failed, see stba_ba_solve)
    else if (gmax <= opt.gradient_tolerance) { s.termination_type = STBA_CONVERGENCE; s.termination_reason = STBA_TERM_GRADIENT; done = true; }
    while (!done) {
        if (iter >= opt.max_num_iterations) { s.termination_type = STBA_NO_CONVERGENCE; s.termination_reason = STBA_TERM_MAX_ITER; break; }
        if (region.below_min(opt)) { s.termination_type = STBA_CONVERGENCE; s.termination_reason = STBA_TERM_MIN_RADIUS; break; }
        ++iter;
        double model_change = 0.0, new_cost = 0.0, step_norm = 0.0;
        bool ok = false;
        STBA_TRY(S.step(region.radius, &model_change, &ok));
        if (ok && (!(model_change > 0.0) || !std::isfinite(model_change))) ok = false;
        if (ok) {
            if (plus) plus(user, x, S.dx, xn.data());
            else for (int a = 0; a < n_params; ++a) xn[a] = x[a] + S.dx[a];
            if (bounded)
                for (int a = 0; a < n_params; ++a) {
                    if (lower && xn[a] < lower[a]) xn[a] = lower[a];
                    if (upper && xn[a] > upper[a]) xn[a] = upper[a];
                }
            if (fn(user, xn.data(), rn.data(), nullptr) != 0) ok = false;
        }
        if (ok) {
            for (double v : rn) new_cost += v * v;
            new_cost *= 0.5;
            for (int a = 0; a < n_params; ++a) step_norm += (xn[a] - x[a]) * (xn[a] - x[a]);
            step_norm = std::sqrt(step_norm);
        }
        // (a non-finite trial cost stays ok here, unlike BA and the pose graph: it is judged, and its NaN rho reaches the trace)
        const StepVerdict v = judge_step(opt, cost, ok, new_cost, model_change, step_norm, x_norm);
        if (v.accepted) { memcpy(x, xn.data(), sizeof(double) * n_params); cost = new_cost; ++s.num_successful_steps; }
        if (v.stop) {
            s.termination_type = STBA_CONVERGENCE; s.termination_reason = v.stop;
            trace_step(trace, iter, ok, cost, new_cost, v, gmax, step_norm, region.radius);
            if (cb) (void)cb(cb_user, iter, cost, v.cost_change, gmax, step_norm, region.radius, v.accepted ? 1 : 0);
            break;
        }
        if (v.accepted) {
            x_norm = norm_of(x, n_params);
            if (fn(user, x, S.r, S.J) != 0) return fail(STBA_ERR_CALLBACK, "residual callback failed");
            region.accept(v.rho, opt);
            STBA_TRY(S.linearize(region.radius));
            gmax = gmax_of();
        } else {
            ++s.num_unsuccessful_steps;
            region.reject();
        }
        trace_step(trace, iter, ok, cost, new_cost, v, gmax, step_norm, region.radius);
        if (opt.minimizer_progress_to_stdout) progress_step(iter, cost, v, gmax, step_norm, region.radius);
        if (cb && cb(cb_user, iter, cost, v.cost_change, gmax, step_norm, region.radius, v.accepted ? 1 : 0) != 0) {
            s.termination_type = STBA_CONVERGENCE; s.termination_reason = STBA_TERM_USER; break;
        }
        if (v.accepted && gmax <= opt.gradient_tolerance) { s.termination_type = STBA_CONVERGENCE; s.termination_reason = STBA_TERM_GRADIENT; break; }
    }
    finish_summary(&s, iter, cost, region.radius, gmax, t_start);
    if (summary) *summary = s;
    return STBA_OK;
}

}  // namespace
}  // namespace stba

extern "C" {

int stba_dense_solve(stba_residual_fn fn, stba_plus_fn plus, void* user, int n_params, int n_local, int n_res,
                     double* x, const double* lower, const double* upper, const stba_lm_options* opt_in,
                     stba_lm_summary* summary, double* trace, stba_iteration_callback cb, void* cb_user) {
    if (!fn || !x || n_params <= 0 || n_local <= 0 || n_res <= 0)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_dense_solve: bad argument");
    if ((lower || upper) && plus)
        return fail(STBA_ERR_INVALID_ARGUMENT, "bounds are only supported on Euclidean parameter blocks");
    if (!plus && n_params != n_local)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_dense_solve: n_params != n_local needs a plus() callback");
    STBA_TRY(require_device());
    stba_lm_options opt;
    if (opt_in) opt = *opt_in; else default_options(&opt);
    const int n = n_local;
    if (small_dense_fits(n_res, n)) {
        SmallDenseSteps S(opt, n_res, n);
        STBA_TRY(S.init());
        return dense_lm(S, fn, plus, user, n_params, n, n_res, x, lower, upper, opt, summary, trace, cb, cb_user);
    }
    GeneralDenseSteps S(opt, n_res, n);
    STBA_TRY(S.init());
    return dense_lm(S, fn, plus, user, n_params, n, n_res, x, lower, upper, opt, summary, trace, cb, cb_user);
}

// (J^T J)^-1 at x: one evaluation of the callback, J^T J formed on the device by GeneralDenseSteps::linearize -- the normal
// equations of the general dense solve -- and inverted by covariance.hip's cov_spd_inverse_packed
int stba_dense_covariance(stba_residual_fn fn, void* user, int n_params, int n_local, int n_res, const double* x, double min_rcond,
                          double* cov, double* rcond_out) {
    if (!fn || !x || !cov || n_params <= 0 || n_local <= 0 || n_res <= 0)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_dense_covariance: bad argument");
    if (n_local > 4096 || (double)n_local * n_res > 2.7e8)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_dense_covariance: limited to 4096 local parameters and 2.7e8 Jacobian entries");
    STBA_TRY(require_device());
    stba_lm_options opt;
    default_options(&opt);
    const int n = n_local;
    GeneralDenseSteps S(opt, n_res, n);
    STBA_TRY(S.init());
    std::vector<double> xv(x, x + n_params);
    if (fn(user, xv.data(), S.r, S.J) != 0) return fail(STBA_ERR_CALLBACK, "residual callback failed");
    for (int i = 0; i < n_res; ++i)
        if (!std::isfinite(S.r[i])) return fail(STBA_ERR_CALLBACK, "stba_dense_covariance: non-finite residual");
    STBA_TRY(S.linearize(0.0));
    DevBuf<double> sig;
    STBA_TRY(sig.alloc((size_t)n * (n + 1) / 2));
    double rc = 0.0;
    int piv = 0;
    STBA_TRY(cov_spd_inverse_packed(S.dH, n, n, nullptr, sig, &rc, &piv, S.w.st));
    if (rcond_out) *rcond_out = rc;
    if (piv) return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, "stba_dense_covariance: J^T J is not positive definite (pivot of row " + std::to_string(piv - 1) + ")");
    if (!(rc >= min_rcond)) {
        char buf[64];
        snprintf(buf, sizeof buf, "%.3e", rc);
        return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, std::string("stba_dense_covariance: J^T J has a pivot ratio of ") + buf + ", below min_reciprocal_condition_number");
    }
    std::vector<double> packed((size_t)n * (n + 1) / 2);
    STBA_TRY(download(packed.data(), sig, packed.size(), S.w.st));
    STBA_HIP(hipStreamSynchronize(S.w.st));
    unpack_symmetric(packed, n, cov);
    return STBA_OK;
}

}  // extern "C"
