// stba_engine.hip -- the bundle-adjustment engine of the MI355X NLS library as an object: the process-wide entry points of the C ABI
// (include/stba.h: status strings, the last error, the version, the device functions, the default LM options), creation and
// teardown of an engine (ba_fill, ba_create, stba_ba_create[_ex], stba_ba_destroy) and its plain setters and getters.  What an
// engine DOES is in the other BA host units over ba_engine.hpp: ba_linear.hip, ba_allreduce.hip, ba_solve.hip, ba_stages.hip and
// ba_factors.hip.  The dense entry points are dense_engine.hip, calibration is calib.hip.
// There is no CPU fallback: without a HIP device every compute entry point fails.
#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>

#include "ba_engine.hpp"
#include "inner_iterations.hpp"
#include "lm_policy.hpp"

namespace stba {

thread_local std::string g_last_error;

int require_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(STBA_ERR_NO_DEVICE, std::string("no HIP device visible (") +
                                            (e == hipSuccess ? "count=0" : hipGetErrorString(e)) +
                                            "); libstba has no CPU fallback");
    return STBA_OK;
}

}  // namespace stba

static_assert(sizeof(PairRec) == sizeof(int4) && alignof(int4) % alignof(PairRec) == 0, "the Schur kernel reads a pair record as one int4");
static_assert(SCHUR_FORM_PAIRS == STBA_SCHUR_PAIRS && SCHUR_FORM_DENSE == STBA_SCHUR_DENSE, "schur_plan.hpp mirrors include/stba.h");

namespace stba {

// The part of an engine's end that is an order and not ownership (the contract is stated on stba_ba, ba_engine.hpp): the stream is
// synchronised FIRST, then everything that has no destructor goes, then the stream, and `delete` lets the members free themselves.
static void ba_free(stba_ba* b) {
    if (b->st) { (void)hipStreamSynchronize(b->st); chol_forget_stream(b->st); }
    cov_store_free(b->cov);
    b->pcg.host.release();
    b->dl.host.release();
    b->ts_host.release();
    if (b->own_stream && b->st) (void)hipStreamDestroy(b->st);
    delete b;
}

}  // namespace stba

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* stba_status_string(int status) {
    switch (status) {
        case STBA_OK: return "ok";
        case STBA_ERR_INVALID_ARGUMENT: return "invalid argument";
        case STBA_ERR_NO_DEVICE: return "no HIP device (no CPU fallback)";
        case STBA_ERR_HIP: return "HIP runtime error";
        case STBA_ERR_NOT_POSITIVE_DEFINITE: return "matrix not positive definite";
        case STBA_ERR_ALLOC: return "device allocation failed";
        case STBA_ERR_STATE: return "call order / state error";
        case STBA_ERR_CALLBACK: return "callback failed";
        case STBA_ERR_NO_SOLUTION: return "no (unique) solution";
        default: return "unknown";
    }
}

const char* stba_last_error(void) { return g_last_error.c_str(); }
int stba_version(void) { return STBA_VERSION; }
int stba_live_device_buffers(long long* count) {
    if (!count) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_live_device_buffers: null argument");
    *count = g_live_device_buffers.load(std::memory_order_relaxed);
    return STBA_OK;
}

int stba_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void stba_lm_default_options(stba_lm_options* opt) { if (opt) default_options(opt); }

// everything of ba_create behind the engine object and its stream: the plan, the buffers, their contents.  A failure leaves a partly
// filled engine, which ba_create frees
static int ba_fill(stba_ba* b, int n_cams, int n_pts, int n_obs, const double* cams, const double* pts, const int* obs_cam,
                   const int* obs_pt, const double* obs_feat, const unsigned char* cam_fixed, const unsigned char* pt_fixed) {
    const bool iterative = b->iterative;
    static const bool TIMING = knob_int("STBA_CREATE_TIMING", 0) != 0;
    // (declared before the plan's vectors: destroyed after them, so its message includes what freeing them costs)
    struct TotalTimer { bool on; std::chrono::steady_clock::time_point t; ~TotalTimer() { if (on) fprintf(stderr, "stba_ba_create: %-28s %8.2f ms\n", "total, temporaries freed", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count()); } } total_timer{TIMING, std::chrono::steady_clock::now()};
    auto tc0 = std::chrono::steady_clock::now();
    auto tmark = [&](const char* what) {
        if (!TIMING) return;
        auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "stba_ba_create: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t1 - tc0).count());
        tc0 = t1;
    };
    for (auto& e : b->ev) {
        if (e.create() != STBA_OK) return fail(STBA_ERR_HIP, "hipEventCreate");
    }
    hipDeviceProp_t prop;
    int dev = 0;
    (void)hipGetDevice(&dev);
    int num_cu = 256;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) num_cu = prop.multiProcessorCount;
    tmark("events, device properties");

    SchurPlanOptions popt;
    popt.iterative = iterative;
    popt.lda = b->lda;
    size_t total_b = 0;
    if (!iterative) popt.have_mem_info = hipMemGetInfo(&popt.free_bytes, &total_b) == hipSuccess;
    static const int TASK_PAIRS = knob_int("STBA_SCHUR_TASK_PAIRS", SCHUR_TASK_PAIRS);
    popt.task_pairs = TASK_PAIRS;
    popt.plan_knob = knob_int("STBA_SCHUR_PLAN", SCHUR_PLAN_DEFAULT);
    popt.plan_runs = knob_int("STBA_SCHUR_RUNS", 1) != 0;
    popt.rot_by_rank = knob_int("STBA_SCHUR_ROT_RANK", 1) != 0;
    popt.lm_slices_allowed = knob_int("STBA_SCHUR_LM_SLICES", 1) != 0;
    popt.phase = tmark;
    // the whole host-side plan (schur_plan.hpp); the engine keeps it until it is destroyed, see the end of this function
    auto plan = std::make_shared<SchurPlan>();
    std::string why;
    if (build_schur_plan(n_cams, n_pts, n_obs, obs_cam, obs_pt, obs_feat, popt, plan.get(), &why) != 0)
        return fail(STBA_ERR_INVALID_ARGUMENT, why);
    const SchurPlan& P = *plan;
    b->n_chunks = (int)P.chunk_begin.size();
    b->schur.dup_overflow = P.dup_overflow;
    b->schur.mode = b->schur.mode_auto = P.schur_mode;
    b->schur.have_pair_plan = P.have_pair_plan;
    b->schur.lm_slices = P.lm_slices;
    b->schur.n_tasks = P.n_tasks; b->schur.max_cols = P.max_cols;
    b->schur.plan_mode = P.plan_mode;
    b->schur.pairs = (double)P.pairs; b->schur.lds_atomics = P.lds_atomics;
    std::vector<unsigned char> cmask;
    if (cam_fixed) {
        cmask.resize(n_cams);
        for (int c = 0; c < n_cams; ++c) {
            unsigned m = 0;
            for (int a = 0; a < 6; ++a) if (cam_fixed[c * 6 + a]) m |= (1u << a);
            cmask[c] = (unsigned char)m;
        }
    }
    const int n_tiles = (n_obs + LIN_THREADS - 1) / LIN_THREADS;
    const size_t lds = lin_lds_bytes(n_cams, lin_lds_bytes(n_cams, true, true) <= (size_t)LIN_MAX_LDS, true);
    const int per_cu = std::max(1, std::min(4, (int)((160 * 1024) / std::max<size_t>(lds, 1))));
    b->lin_grid = std::max(1, std::min(n_tiles, num_cu * per_cu));

    tmark("masks");
    const size_t no = (size_t)n_obs, np = (size_t)n_pts, nc = (size_t)n_cams;
    // ---- what comes from the host: every array is named once, allocated at its source's length and its copy enqueued (to_device)
    const std::string who = "stba_ba_create";
    STBA_TRY(to_device(who, b->cams[0], cams, nc * 7, b->st)); STBA_TRY(to_device(who, b->pts[0], pts, np * 3, b->st));
    STBA_TRY(b->cams[1].alloc(nc * 7)); STBA_TRY(b->pts[1].alloc(np * 3));
    STBA_TRY(b->feat.alloc(no));            // (double2 on the device, pairs of doubles in the plan)
    STBA_TRY(upload(reinterpret_cast<double*>(b->feat.get()), P.s_feat.data(), no * 2, b->st));
    STBA_TRY(to_device(who, b->obs_cam, P.s_cam, b->st)); STBA_TRY(to_device(who, b->obs_pt, P.s_pt, b->st));
    STBA_TRY(to_device(who, b->pt_start, P.pt_start, b->st)); STBA_TRY(to_device(who, b->cam_perm, P.cam_perm, b->st));
    STBA_TRY(to_device(who, b->chunk_begin, P.chunk_begin, b->st)); STBA_TRY(to_device(who, b->chunk_end, P.chunk_end, b->st));
    STBA_TRY(to_device(who, b->cam_chunk_start, P.cam_chunk_start, b->st));
    STBA_TRY(to_device(who, b->schur.task_cam, P.task_cam, b->st)); STBA_TRY(to_device(who, b->schur.cam_start, P.cam_start, b->st));
    STBA_TRY(to_device(who, b->schur.task_col_lo, P.task_col_lo, b->st)); STBA_TRY(to_device(who, b->schur.task_col_hi, P.task_col_hi, b->st));
    b->ar.h_row_col_ptr = P.row_col_ptr; b->ar.h_row_cols = P.row_cols;
    STBA_TRY(to_device(who, b->schur.row_col_ptr, P.row_col_ptr, b->st)); STBA_TRY(to_device(who, b->schur.row_cols, P.row_cols, b->st));
    STBA_TRY(to_device(who, b->schur.pair_begin, P.pair_begin, b->st)); STBA_TRY(to_device(who, b->schur.pair_end, P.pair_end, b->st));
    STBA_TRY(b->schur.pair_rec.alloc(P.pairs));          // (the plan holds them as PairRec, not in a vector)
    if (P.pairs > 0) STBA_TRY(upload(b->schur.pair_rec, reinterpret_cast<const int4*>(P.pair_rec.get()), P.pairs, b->st));
    STBA_TRY(to_device(who, b->schur.task_vs_ptr, P.task_vs_ptr, b->st)); STBA_TRY(to_device(who, b->schur.vs_first, P.vs_first, b->st));
    if (cam_fixed) STBA_TRY(to_device(who, b->cam_fixed, cmask, b->st));
    if (pt_fixed) STBA_TRY(to_device(who, b->pt_fixed, pt_fixed, np, b->st));
    if (b->schur.lm_slices) {
        STBA_TRY(to_device(who, b->schur.task_p_lo, P.task_p_lo, b->st)); STBA_TRY(to_device(who, b->schur.task_p_hi, P.task_p_hi, b->st));
        STBA_TRY(to_device(who, b->schur.task_part_off, P.task_part_off, b->st));
        STBA_TRY(to_device(who, b->schur.row_task_ptr, P.row_task_ptr, b->st)); STBA_TRY(to_device(who, b->schur.row_tasks, P.row_tasks, b->st));
        STBA_TRY(b->schur.part.alloc(P.part_doubles));
    }
    if (!P.dup_run.empty()) STBA_TRY(to_device(who, b->schur.dup_run, P.dup_run, b->st));
    std::vector<unsigned char>& omask = b->schur.create_omask;
    if (cam_fixed || pt_fixed) {
        omask.resize(no);
        for (size_t p2 = 0; p2 < no; ++p2)
            omask[p2] = (unsigned char)((cam_fixed ? cmask[(size_t)P.s_cam[p2]] : 0u) | ((pt_fixed && pt_fixed[(size_t)P.s_pt[p2]]) ? 64u : 0u));
        STBA_TRY(to_device(who, b->omask, omask, b->st));
    }
    // ---- what the kernels fill
    STBA_TRY(b->r.alloc(no)); STBA_TRY(b->J8.alloc(no * 8));
    STBA_TRY(b->Hpp6.alloc(np * 6)); STBA_TRY(b->gp.alloc(np * 3)); STBA_TRY(b->Hinv6.alloc(np * 6)); STBA_TRY(b->Rinv9.alloc(np * 9));
    STBA_TRY(b->dp.alloc(np * 3)); STBA_TRY(b->scale_p.alloc(np * 3));
    STBA_TRY(b->Hcc.alloc(nc * 36)); STBA_TRY(b->gc.alloc(nc * 6)); STBA_TRY(b->cam_partial.alloc((size_t)b->n_chunks * 28));
    STBA_TRY(b->dc.alloc(nc * 6)); STBA_TRY(b->scale_c.alloc(nc * 6));
    STBA_TRY(b->Sbuf.alloc(b->sbuf_count()));
    STBA_TRY(b->dxc.alloc((size_t)b->lda)); STBA_TRY(b->dxp.alloc(np * 3));
    STBA_TRY(b->cost_partial.alloc(CostSlots::capacity(b->lin_grid)));
    STBA_TRY(b->upd_partial_c.alloc((size_t)backsub_cam_grid(n_cams) * 4));    // (>= (n_cams + 255) / 256 blocks of 4)
    STBA_TRY(b->upd_partial_p.alloc((size_t)(point_blocks_grid(n_pts) + 1) * 4));    // (>= (n_pts + 255) / 256 + 1 blocks of 4)
    STBA_TRY(b->trial.alloc((size_t)TS_BLOCK)); STBA_TRY(b->flag.alloc(1));
    if (iterative) STBA_TRY(ba_pcg_alloc(b));

    if (hipMemsetAsync(b->dxc, 0, (size_t)b->lda * sizeof(double), b->st) != hipSuccess ||
        hipMemsetAsync(b->Sbuf, 0, b->sbuf_count() * sizeof(double), b->st) != hipSuccess ||
        hipStreamSynchronize(b->st) != hipSuccess)
        return fail(STBA_ERR_HIP, "stba_ba_create: initial memset/sync failed");
    tmark("device arrays, uploads + sync");
    // The plan's host-side temporaries -- 16 bytes per pair, the regrouped observations: ~110 MB at C5 -- cost 11 of the 43 ms of this
    // function just to FREE (measured: STBA_CREATE_TIMING in a debug build).  The engine keeps them and frees them when it is destroyed:
    // the caller gets its engine that much sooner, and the operator API destroys its engine on a helper thread next to its end-point
    // check anyway.  (Freed by a thread of their own right here: 10 ms off this function as well, but 2 ms ON a drop-in Solve() -- the
    // munmap of 110 MB holds the process's address-space lock while the calling thread faults pages in.)
    b->perm = std::move(plan->perm);
    b->schur.create_leftovers = std::move(plan);
    return STBA_OK;
}

// (iterative: ITERATIVE_SCHUR -- no Schur plan, no dense Y, no S: see stba_ba_create_ex)
static int ba_create(stba_ba** out, int n_cams, int n_pts, int n_obs, const double* cams, const double* pts,
                     const int* obs_cam, const int* obs_pt, const double* obs_feat, const unsigned char* cam_fixed,
                     const unsigned char* pt_fixed, void* hip_stream, bool iterative) {
    if (!out) return fail(STBA_ERR_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (n_cams <= 0 || n_pts < 0 || n_obs < 0 || !cams || (n_pts > 0 && !pts) ||
        (n_obs > 0 && (!obs_cam || !obs_pt || !obs_feat)))
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_create: null or empty input");
    for (int i = 0; i < n_obs; ++i)
        if (obs_cam[i] < 0 || obs_cam[i] >= n_cams || obs_pt[i] < 0 || obs_pt[i] >= n_pts)
            return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_create: observation index out of range");
    STBA_TRY(require_device());
    stba_ba* b = new stba_ba();
    b->iterative = iterative;
    b->nc = n_cams; b->np = n_pts; b->no = n_obs; b->n = 6 * n_cams; b->lda = chol_padded_dim(b->n);
    if (hip_stream) b->st = reinterpret_cast<hipStream_t>(hip_stream);
    else {
        hipError_t e = hipStreamCreate(&b->st);
        if (e != hipSuccess) { delete b; return fail(STBA_ERR_HIP, hipGetErrorString(e)); }
        b->own_stream = true;
    }
    const int rc = ba_fill(b, n_cams, n_pts, n_obs, cams, pts, obs_cam, obs_pt, obs_feat, cam_fixed, pt_fixed);
    if (rc != STBA_OK) { ba_free(b); return rc; }
    *out = b;
    return STBA_OK;
}

int stba_ba_create(stba_ba** out, int n_cams, int n_pts, int n_obs, const double* cams, const double* pts,
                   const int* obs_cam, const int* obs_pt, const double* obs_feat, const unsigned char* cam_fixed,
                   const unsigned char* pt_fixed, void* hip_stream) {
    return ba_create(out, n_cams, n_pts, n_obs, cams, pts, obs_cam, obs_pt, obs_feat, cam_fixed, pt_fixed, hip_stream, false);
}

int stba_ba_create_ex(stba_ba** out, int n_cams, int n_pts, int n_obs, const double* cams, const double* pts,
                      const int* obs_cam, const int* obs_pt, const double* obs_feat, const unsigned char* cam_fixed,
                      const unsigned char* pt_fixed, void* hip_stream, const stba_ba_create_options* opt) {
    if (out) *out = nullptr;
    int solver = STBA_LINEAR_DENSE_SCHUR;
    if (opt) {
        if (opt->struct_size < offsetof(stba_ba_create_options, linear_solver) + sizeof(int))
            return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_create_ex: options.struct_size is smaller than any version of the struct");
        solver = opt->linear_solver;
    }
    if (solver != STBA_LINEAR_DENSE_SCHUR && solver != STBA_LINEAR_ITERATIVE_SCHUR)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_create_ex: unknown linear_solver " + std::to_string(solver));
    return ba_create(out, n_cams, n_pts, n_obs, cams, pts, obs_cam, obs_pt, obs_feat, cam_fixed, pt_fixed, hip_stream,
                     solver == STBA_LINEAR_ITERATIVE_SCHUR);
}

int stba_ba_set_pcg(stba_ba* b, int preconditioner, double eta, int min_iterations, int max_iterations, int check_every) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (!b->iterative) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_pcg: the engine uses the dense Schur solver (stba_ba_create_ex)");
    if (preconditioner < STBA_PRECOND_IDENTITY || preconditioner > STBA_PRECOND_SCHUR_JACOBI || !(eta >= 0.0) || min_iterations < 0 ||
        max_iterations < 1 || min_iterations > max_iterations || check_every < 1)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_pcg: bad argument");
    b->pcg.precond = preconditioner; b->pcg.eta = eta; b->pcg.min = min_iterations; b->pcg.max = max_iterations; b->pcg.check = check_every;
    return STBA_OK;
}

int stba_ba_last_pcg_summary(stba_ba* b, stba_pcg_summary* out) {
    if (!b || !out) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    *out = b->pcg.sum;
    return STBA_OK;
}

int stba_ba_last_pcg_iterations(stba_ba* b, int* per_iteration, int n) {
    if (!b || n < 0 || (n > 0 && !per_iteration)) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_last_pcg_iterations: bad argument");
    for (int k = 0; k < n; ++k) per_iteration[k] = (size_t)k < b->pcg.per_iter.size() ? b->pcg.per_iter[(size_t)k] : 0;
    return STBA_OK;
}

int stba_ba_set_schur_mode(stba_ba* ba, int mode) {
    STBA_TRY(refuse_iterative(ba, "stba_ba_set_schur_mode", "which forms no Schur complement"));
    if (!ba || mode < STBA_SCHUR_AUTO || mode > STBA_SCHUR_DENSE) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_schur_mode: bad argument");
    if (mode == STBA_SCHUR_AUTO) mode = ba->schur.mode_auto;
    if (mode == STBA_SCHUR_PAIRS && !ba->schur.have_pair_plan)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_schur_mode: this engine was created without a pair plan (too many observation pairs)");
    if (mode == STBA_SCHUR_DENSE && ba->schur.dup_overflow)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_schur_mode: more than 255 observations of one (camera, landmark) pair: the dense form cannot take this problem");
    if (mode == STBA_SCHUR_DENSE) STBA_TRY(ba_dense_alloc(ba));
    ba->schur.mode = mode;
    ba->have_reduced = ba->have_dxc = ba->have_dxp = false;
    return STBA_OK;
}
int stba_ba_schur_mode(const stba_ba* ba, int* mode) {
    if (!ba || !mode) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_schur_mode: bad argument");
    *mode = ba->schur.mode;
    return STBA_OK;
}

int stba_ba_destroy(stba_ba* ba) {
    if (!ba) return STBA_OK;
    ba_free(ba);
    return STBA_OK;
}

int stba_ba_set_params(stba_ba* b, const double* cams, const double* pts) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (cams) STBA_TRY(upload(b->cams[b->cur], cams, (size_t)b->nc * 7, b->st));
    if (pts) STBA_TRY(upload(b->pts[b->cur], pts, (size_t)b->np * 3, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    ba_invalidate(b);
    return STBA_OK;
}

int stba_ba_set_features(stba_ba* b, const double* obs_feat) {
    if (!b || (!obs_feat && b->no > 0)) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_features: null argument");
    if (b->no == 0) return STBA_OK;
    std::vector<double> s_feat((size_t)b->no * 2);          // (the engine's order: landmark-major, b->perm = position -> the caller's index)
    for (int p = 0; p < b->no; ++p) {
        const size_t i = (size_t)b->perm[(size_t)p];
        s_feat[2 * (size_t)p] = obs_feat[2 * i]; s_feat[2 * (size_t)p + 1] = obs_feat[2 * i + 1];
    }
    STBA_TRY(upload(reinterpret_cast<double*>(b->feat.get()), s_feat.data(), (size_t)b->no * 2, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    ba_invalidate(b);
    return STBA_OK;
}

int stba_get_device(int* device) {
    if (!device) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_get_device: null argument");
    STBA_TRY(require_device());
    STBA_HIP(hipGetDevice(device));
    return STBA_OK;
}
int stba_set_device(int device) {
    STBA_TRY(require_device());
    STBA_HIP(hipSetDevice(device));
    return STBA_OK;
}

int stba_ba_get_params(stba_ba* b, double* cams, double* pts) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (cams) STBA_TRY(download(cams, b->cams[b->cur], (size_t)b->nc * 7, b->st));
    if (pts) STBA_TRY(download(pts, b->pts[b->cur], (size_t)b->np * 3, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    return STBA_OK;
}

int stba_ba_set_allreduce(stba_ba* b, stba_allreduce_fn fn, void* user, int rank, int world_size) {
    if (b) STBA_TRY(ba_refuse(b, "stba_ba_set_allreduce", fn || world_size > 1));
    if (!b || world_size < 1 || rank < 0 || rank >= world_size || world_size > SC_MAX_WORLD)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_allreduce: bad rank/world");
    if (!fn && world_size > 1) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_allreduce: world_size > 1 needs a hook");
    b->ar.fn = fn; b->ar.user = user; b->ar.rank = rank; b->ar.world = world_size;
    // what travels is decided again with the new group (the union pattern belongs to the group)
    b->ar.form = PACK_UNPLANNED; b->ar.nz = 0;
    b->ar.blocks.reset();
    b->ar.Spack.reset();
    return STBA_OK;
}

int stba_ba_reduced_dim(const stba_ba* b, int* n, int* n_padded) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (n) *n = b->n;
    if (n_padded) *n_padded = b->lda;
    return STBA_OK;
}

int stba_ba_set_trust_region(stba_ba* b, int strategy) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (strategy != STBA_TR_LEVENBERG_MARQUARDT && strategy != STBA_TR_TRADITIONAL_DOGLEG)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_trust_region: unknown strategy " + std::to_string(strategy));
    STBA_TRY(ba_refuse(b, "stba_ba_set_trust_region", strategy == STBA_TR_TRADITIONAL_DOGLEG));
    b->dl.trust_region = strategy;
    return STBA_OK;
}

int stba_ba_last_dogleg_summary(stba_ba* b, stba_dogleg_summary* out) {
    if (!b || !out) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    const size_t want = out->struct_size;
    if (want < offsetof(stba_dogleg_summary, factorizations) + sizeof(int))
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_last_dogleg_summary: out->struct_size is smaller than any version of the struct");
    stba_dogleg_summary s = b->dl.sum;
    s.struct_size = want;
    memcpy(out, &s, std::min(want, sizeof s));
    return STBA_OK;
}

int stba_ba_set_inner_iterations(stba_ba* b, int enable, double tolerance, const int* cam_rot_group, const int* cam_pos_group,
                                 const int* pt_group) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (!enable) {
        b->inner.on = false;
        return STBA_OK;
    }
    if (!(tolerance >= 0.0) || !std::isfinite(tolerance))
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_inner_iterations: the tolerance must be finite and >= 0");
    STBA_TRY(ba_refuse(b, "stba_ba_set_inner_iterations"));
    const int nc = b->nc, np = b->np, no = b->no;
    // constant parts, from the device's masks (cam_fixed: bit a = dof a constant)
    std::vector<unsigned char> cf((size_t)nc, 0), pf((size_t)np, 0);
    if (b->cam_fixed) STBA_TRY(download(cf.data(), b->cam_fixed, (size_t)nc, b->st));
    if (b->pt_fixed) STBA_TRY(download(pf.data(), b->pt_fixed, (size_t)np, b->st));
    std::vector<int> oc((size_t)no), op((size_t)no);
    STBA_TRY(download(oc.data(), b->obs_cam, (size_t)no, b->st));
    STBA_TRY(download(op.data(), b->obs_pt, (size_t)no, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    InnerPlan plan;
    std::string why;
    if (build_inner_plan(nc, np, no, oc.data(), op.data(), cf.data(), pf.data(), cam_rot_group, cam_pos_group, pt_group, &plan, &why) != 0)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_inner_iterations: " + why);
    // device lists: the new ones are allocated and filled first and swapped in only when all of them are there, so that a failed
    // allocation leaves the engine's state (and an earlier ordering) as it was
    const size_t n_it = std::max<size_t>(plan.cam.size() + plan.pt.size(), 1);
    DevBuf<int> n_cam, n_pt, n_itb, n_gate;
    DevBuf<unsigned char> n_mask;
    DevBuf<double> n_sc, n_part;
    STBA_TRY(n_cam.alloc(plan.cam.size())); STBA_TRY(n_mask.alloc(plan.mask.size())); STBA_TRY(n_pt.alloc(plan.pt.size())); STBA_TRY(n_itb.alloc(n_it));
    if (!b->inner.gate) STBA_TRY(n_gate.alloc(1));
    if (!b->inner.sc) STBA_TRY(n_sc.alloc(4));
    if (!b->inner.part) STBA_TRY(n_part.alloc((size_t)inner_step_grid(nc, np)));
    STBA_TRY(upload(n_cam, plan.cam.data(), plan.cam.size(), b->st));
    STBA_TRY(upload(n_mask, plan.mask.data(), plan.mask.size(), b->st));
    STBA_TRY(upload(n_pt, plan.pt.data(), plan.pt.size(), b->st));
    if (hipMemsetAsync(n_itb, 0, n_it * sizeof(int), b->st) != hipSuccess || hipStreamSynchronize(b->st) != hipSuccess)
        return fail(STBA_ERR_HIP, "stba_ba_set_inner_iterations: upload failed");
    // (the stream is idle: the moves free the earlier ordering)
    b->inner.cam = std::move(n_cam); b->inner.pt = std::move(n_pt); b->inner.it = std::move(n_itb); b->inner.mask = std::move(n_mask);
    if (n_gate) b->inner.gate = std::move(n_gate);
    if (n_sc) b->inner.sc = std::move(n_sc);
    if (n_part) b->inner.part = std::move(n_part);
    b->inner.plan = std::move(plan);
    b->inner.tol = tolerance;
    b->inner.on = true;
    inner_summary_reset(b);
    return STBA_OK;
}

int stba_ba_last_inner_summary(stba_ba* b, stba_inner_summary* out) {
    if (!b || !out || out->struct_size < offsetof(stba_inner_summary, sweeps) + sizeof(int)) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_last_inner_summary: bad argument");
    const size_t n = std::min(out->struct_size, sizeof(stba_inner_summary));
    stba_inner_summary s = b->inner.sum;
    s.struct_size = out->struct_size;
    memcpy(out, &s, n);
    return STBA_OK;
}

}  // extern "C"
