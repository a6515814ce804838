// stba_engine.hip -- host side of the bundle-adjustment engine of the MI355X NLS library: the stba_ba_* part of the C ABI
// (include/stba.h; the factor setters are ba_factors.hip) and the process-wide entry points (status strings, the last error, the
// version, the device functions, the default LM options).  The dense entry points are dense_engine.hip, calibration is calib.hip.
// The Levenberg-Marquardt control flow follows Ceres' TrustRegionMinimizer +
// LevenbergMarquardtStrategy (the solver behind ceres::Solve at
// st20-g2o/src/include/test_ceres.h:148 and st17-ceres/src/include/solver.hpp:286) with the
// defaults listed in SURVEY.md 8c; all arithmetic on problem-sized data runs in HIP kernels.
// There is no CPU fallback: without a HIP device every compute entry point fails.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <thread>
#include <vector>

#include "ba_engine.hpp"
#include "dogleg.hpp"
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

// Everything of an engine that is not memory, then the engine: its DevBuf members free themselves in `delete`.  The order: the
// stream is synchronised FIRST (nothing on the device reads a buffer that is about to go), then the Cholesky's per-stream cache
// forgets it, then the events, the mapped blocks and the stream itself, and the buffers last.
static void ba_free(stba_ba* b) {
    if (b->st) { (void)hipStreamSynchronize(b->st); chol_forget_stream(b->st); }
    b->create_leftovers.reset();                        // (what ba_create's plan left on the host)
    std::vector<unsigned char>().swap(b->create_omask);
    cov_store_free(b->cov);
    for (auto& e : b->inner.ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : b->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : b->ev_ar) if (e) (void)hipEventDestroy(e);
    b->pcg_host.release();
    b->dl_host.release();
    b->ts_host.release();
    if (b->own_stream && b->st) (void)hipStreamDestroy(b->st);
    delete b;
}

static LinArgs lin_args(stba_ba* b, int which, bool store_r) {
    LinArgs a;
    a.n_obs = b->no; a.n_cams = b->nc;
    a.cams = b->cams[which]; a.pts = b->pts[which];
    a.feat = b->feat; a.obs_cam = b->obs_cam; a.obs_pt = b->obs_pt;
    a.cam_fixed = b->cam_fixed; a.pt_fixed = b->pt_fixed;
    a.r = store_r ? b->r : nullptr; a.J8 = b->J8; a.cost_partial = b->cost_partial;
    return a;
}

// Host-linearised factors: parameters of buffer `which` -> host, the caller's callback makes r (and, with_jac, the 2x6 | 2x3
// Jacobians in LOCAL camera coordinates [dtheta, dt]) in ITS observation order, the engine regroups them landmark-major and
// uploads them where the device kernel would have put them: r, J8 = {0, 0, Jp}, Jc12, and sum r^2 as the first cost partial.
// Synchronous by nature (the callback is host code); the LM loop does not speculate in this mode.
static int ba_host_linearize(stba_ba* b, int which, bool with_jac) {
    const size_t no = (size_t)b->no;
    b->hl_cams.resize((size_t)b->nc * 7); b->hl_pts.resize((size_t)b->np * 3); b->hl_r.resize(no * 2);
    if (with_jac) { b->hl_jc.resize(no * 12); b->hl_jp.resize(no * 6); }
    STBA_TRY(download(b->hl_cams.data(), b->cams[which], b->hl_cams.size(), b->st));
    STBA_TRY(download(b->hl_pts.data(), b->pts[which], b->hl_pts.size(), b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    if (b->hl_fn(b->hl_user, b->hl_cams.data(), b->hl_pts.data(), b->hl_r.data(), with_jac ? b->hl_jc.data() : nullptr,
                 with_jac ? b->hl_jp.data() : nullptr) != 0)
        return fail(STBA_ERR_CALLBACK, "host lineariser failed (a cost function returned false)");
    double c2 = 0.0;
    for (size_t k = 0; k < no * 2; ++k) c2 += b->hl_r[k] * b->hl_r[k];
    if (!std::isfinite(c2)) return fail(STBA_ERR_CALLBACK, "host lineariser: non-finite residual");
    // (the cost partials have a staging buffer of their own: the copy is asynchronous, and the big staging buffer below is
    // resized and overwritten right behind it -- in the cost-only call nothing waits for it before the next call refills it)
    b->hl_cost_stage.assign((size_t)b->lin_grid, 0.0);
    b->hl_cost_stage[0] = c2;
    STBA_TRY(upload(b->cost_partial, b->hl_cost_stage.data(), b->hl_cost_stage.size(), b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    std::vector<double>& st = b->hl_stage;
    if (with_jac) {
        st.resize(no * 12);
        for (size_t p = 0; p < no; ++p) { const size_t i = (size_t)b->perm[p]; memcpy(&st[p * 2], &b->hl_r[i * 2], 2 * sizeof(double)); }
        STBA_TRY(upload(reinterpret_cast<double*>(b->r.get()), st.data(), no * 2, b->st));
        STBA_HIP(hipStreamSynchronize(b->st));              // (the staging buffer is reused)
        for (size_t p = 0; p < no; ++p) {
            const size_t i = (size_t)b->perm[p];
            st[p * 8] = 0.0; st[p * 8 + 1] = 0.0;
            memcpy(&st[p * 8 + 2], &b->hl_jp[i * 6], 6 * sizeof(double));
        }
        STBA_TRY(upload(b->J8, st.data(), no * 8, b->st));
        STBA_HIP(hipStreamSynchronize(b->st));
        for (size_t p = 0; p < no; ++p) memcpy(&st[p * 12], &b->hl_jc[(size_t)b->perm[p] * 12], 12 * sizeof(double));
        STBA_TRY(upload(b->Jc12, st.data(), no * 12, b->st));
        STBA_HIP(hipStreamSynchronize(b->st));
    }
    return STBA_OK;
}

// THE linearisation at parameter buffer `which`: the host's callback, the robust kernel (a loss table and / or weights are set: its
// INFO / LOSS pair follows from which of the two the engine holds) or the lossless kernel.  The cost partials (sum r^2, or sum rho with a table) are left in cost_partial; with_jac: r, J8 (and Jc12) are stored
static int ba_linearize_dispatch(stba_ba* b, int which, bool with_jac) {
    if (b->hl_fn) return ba_host_linearize(b, which, with_jac);
    const LinArgs a = lin_args(b, which, with_jac);
    if (with_jac) b->lin_which = which;
    if (b->loss.kind || b->winfo)
        STBA_TRY(launch_linearize_robust(a, LinLoss{b->loss.kind, b->loss.a, b->loss.b, b->loss.scale, b->Jc12, b->winfo}, with_jac, b->lin_grid, b->st));
    else
        STBA_TRY(launch_linearize(a, with_jac, b->lin_grid, b->st));
    // pose priors: their cost at the same parameters into the slot behind the lineariser's partials (one launch; n_cost counts it)
    if (b->prior.n) STBA_TRY(launch_prior_cost(b->prior_args(), b->cams[which], b->cost_partial + b->lin_grid, b->st));
    // relative-pose factors: theirs into the next slot
    if (b->btw.n) STBA_TRY(launch_between_cost(b->between_args(), b->cams[which], b->cost_partial + b->lin_grid + (b->prior.n ? 1 : 0), b->st));
    // landmark priors: theirs into the last slot
    if (b->lprior.n) STBA_TRY(launch_landmark_prior_cost(b->landmark_prior_args(), b->pts[which], b->lprior.cost_part, b->cost_partial + b->n_cost() - 1, b->st));
    return STBA_OK;
}

// pose priors: sum J'^T J' into Hcc and sum J'^T r' into gc, at the parameters the Jacobian records were made at (one launch; none
// without priors).  Behind whatever has just WRITTEN the camera blocks: the Schur step or the camera-block kernel
static int ba_prior_blocks(stba_ba* b) {
    if (!b->prior.n) return STBA_OK;
    return launch_prior_blocks(b->prior_args(), b->cams[b->lin_which], b->Hcc, b->gc, nullptr, nullptr, b->st);
}

// relative-pose factors: sum J_x'^T J_x' into Hcc, sum J_x'^T r' into gc and -- with_S -- sum J_hi'^T J_lo' onto the block (hi, lo) of S,
// which the Schur step has just zeroed and written (every build: nothing accumulates from one build to the next).  One launch; none
// without edges
static int ba_between_blocks(stba_ba* b, bool with_S) {
    if (!b->btw.n) return STBA_OK;
    return launch_between_blocks(b->between_args(), b->cams[b->lin_which], b->Hcc, b->gc, with_S ? b->S() : nullptr, b->lda, nullptr, nullptr,
                                 nullptr, b->st);
}

// residuals + Jacobians at parameter buffer `which`; sum r^2 -> *cost2_dev
static int ba_linearize(stba_ba* b, int which, double* cost2_dev) {
    STBA_TRY(ba_linearize_dispatch(b, which, true));
    return launch_sum_partials(b->cost_partial, b->n_cost(), 1, 1, cost2_dev, b->st);
}

// residual-only kernel (nothing stored): sum r^2 -> *cost2_dev
static int ba_cost_only(stba_ba* b, int which, double* cost2_dev) {
    STBA_TRY(ba_linearize_dispatch(b, which, false));
    return launch_sum_partials(b->cost_partial, b->n_cost(), 1, 1, cost2_dev, b->st);
}

// landmark blocks Hpp, gp.  The CAMERA blocks Hcc, gc are made by the Schur kernel on the way (ba_build_reduced: the
// workgroup of a camera row has that camera's Jacobian records in its caches anyway); only the stage entry point
// stba_ba_normal_blocks, which hands them out without building the reduced system, runs the camera-side kernel.
// Landmark priors: sum W^T W into Hpp6 and sum W^T r' into gp right behind the kernel that has just written both, at the parameters
// the Jacobian records were made at -- every reader downstream (damping and scale, the inverses, both Schur forms, the back-
// substitution, the covariance, the implicit build) sees the sum -- and that kernel's max |gp| partials made again from it (one
// launch; none without priors)
static int ba_normal_blocks(stba_ba* b) {
    STBA_TRY(launch_point_blocks(b->np, b->pt_start, b->J8, b->omask, b->r, b->Hpp6, b->gp, b->upd_partial_p, b->st));
    if (!b->lprior.n) return STBA_OK;
    return launch_landmark_prior_blocks(b->landmark_prior_args(), b->pts[b->lin_which], b->Hpp6, b->gp, b->upd_partial_p, nullptr, nullptr, b->st);
}
// residuals + Jacobians of the LM loop: the cost partial sums stay in cost_partial and are added up by
// ba_fill_scalar_slots behind the landmark blocks (one launch less than ba_linearize)
static int ba_linearize_lm(stba_ba* b, int which) {
    return ba_linearize_dispatch(b, which, true);
}
static int ba_camera_blocks(stba_ba* b) {
    return launch_camera_blocks(b->nc, b->n_chunks, b->chunk_begin, b->chunk_end, b->cam_chunk_start, b->cam_perm,
                                b->J8, b->omask, ba_general_jc(b), b->r, b->cam_partial, b->Hcc, b->gc, b->st);
}

struct Damping {
    bool explicit_d = false;   // dc / dp were uploaded by the caller
    double radius = 1e4, dmin = 1e-6, dmax = 1e32;
    int use_scaling = 1;
};

// S (damped, padded, rhs row in place) on the device.  One cross-rank sum carries S, diag(Hcc),
// gc, rhs and the scalar slots.
// row r < n: S[r][0..r] <-> tri[r(r+1)/2 ..]; block n: the four extras vectors behind S <-> behind tri
__global__ __launch_bounds__(256) void tri_pack_kernel(double* __restrict__ Sbuf, int lda, int n, double* __restrict__ pack, int to_pack) {
    const int r = blockIdx.x;
    if (r < n) {
        double* row = Sbuf + (size_t)r * lda;
        double* dst = pack + (size_t)r * (r + 1) / 2;
        for (int c = threadIdx.x; c <= r; c += 256) {
            if (to_pack) dst[c] = row[c]; else row[c] = dst[c];
        }
    } else {
        double* ex = Sbuf + (size_t)lda * lda;
        double* dst = pack + (size_t)n * (n + 1) / 2;
        for (int c = threadIdx.x; c < 4 * lda; c += 256) {
            if (to_pack) dst[c] = ex[c]; else ex[c] = dst[c];
        }
    }
}

// the travelling 6x6 blocks <-> the packed buffer; the four extras vectors behind S <-> behind the blocks
__global__ __launch_bounds__(256) void blk_pack_kernel(double* __restrict__ Sbuf, int lda, const int2* __restrict__ blocks, int nz,
                                                       double* __restrict__ pack, int to_pack) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nel = (size_t)nz * 36;
    if (e < nel) {
        const int blk = (int)(e / 36), k = (int)(e % 36);
        const int2 ij = blocks[blk];
        double* p = Sbuf + (size_t)(6 * ij.x + k / 6) * lda + 6 * ij.y + k % 6;
        if (to_pack) pack[e] = *p; else *p = pack[e];
    } else if (e < nel + 4 * (size_t)lda) {
        double* p = Sbuf + (size_t)lda * lda + (e - nel);
        if (to_pack) pack[e] = *p; else *p = pack[e];
    }
}

// decides once per engine what travels in the cross-rank sum of the reduced system: the union over ranks of the
// non-zero blocks (a 0/1 mask of the nc(nc+1)/2 lower blocks, summed with the same hook) if it is sparse
static int ba_plan_pack(stba_ba* b) {
    const size_t nb = (size_t)b->nc * (b->nc + 1) / 2;
    static const bool SPARSE = knob_int("STBA_PACK_BLOCKS", 1) != 0;
    b->pk_state = 1;
    if (SPARSE && !b->h_row_col_ptr.empty()) {
        std::vector<double> mask(nb, 0.0);
        for (int c = 0; c < b->nc; ++c) {
            mask[(size_t)c * (c + 1) / 2 + c] = 1.0;                 // the diagonal block always travels (Hcc)
            for (int k = b->h_row_col_ptr[(size_t)c]; k < b->h_row_col_ptr[(size_t)c + 1]; ++k)
                mask[(size_t)c * (c + 1) / 2 + b->h_row_cols[(size_t)k]] = 1.0;
        }
        DevBuf<double> dmask;
        STBA_TRY(dmask.alloc(nb));
        STBA_TRY(upload(dmask, mask.data(), nb, b->st));
        if (b->ar(b->ar_user, dmask, nb, b->st) != 0) return fail(STBA_ERR_CALLBACK, "all-reduce hook failed");
        if (hipMemcpyAsync(mask.data(), dmask, nb * sizeof(double), hipMemcpyDeviceToHost, b->st) != hipSuccess ||
            hipStreamSynchronize(b->st) != hipSuccess)
            return fail(STBA_ERR_HIP, "mask download failed");
        dmask.reset();
        std::vector<int2> blocks;
        for (int c = 0; c < b->nc; ++c)
            for (int c2 = 0; c2 <= c; ++c2)
                if (mask[(size_t)c * (c + 1) / 2 + c2] > 0.5) blocks.push_back(make_int2(c, c2));
        if (blocks.size() * 36 * 2 < (size_t)b->n * (b->n + 1) / 2) {      // worth it below 50 % of the triangle
            STBA_TRY(b->pk_blocks.alloc(blocks.size()));
            STBA_TRY(upload(b->pk_blocks, blocks.data(), blocks.size(), b->st));
            STBA_HIP(hipStreamSynchronize(b->st));
            b->pk_nz = (int)blocks.size();
            b->pk_state = 2;
        }
    }
    STBA_TRY(b->Spack.alloc(b->pack_count()));
    return STBA_OK;
}

// device time of the last cross-rank sum of the reduced system: read once its events have completed (after a
// synchronisation of the stream; a pair still in flight is waited for -- only on the multi-rank path)
static void ba_collect_allreduce_time(stba_ba* b) {
    if (!b->ar_timing_pending) return;
    float ms = 0.f;
    if (hipEventSynchronize(b->ev_ar[1]) == hipSuccess && hipEventElapsedTime(&ms, b->ev_ar[0], b->ev_ar[1]) == hipSuccess) b->ar_ms += ms;
    b->ar_timing_pending = false;
}

// Y for the dense form of the Schur complement: [lda][ldy] doubles, zeroed once (the visibility pattern is static)
static int ba_dense_alloc(stba_ba* b) {
    if (b->Y) return STBA_OK;
    const size_t kcols = ((size_t)3 * b->np + 15) / 16 * 16;
    const size_t ldy = kcols + ((kcols % 512 == 0) ? 16 : 0);          // (not a multiple of 4 KB: rows would alias in the memory channels)
    const size_t ycount = (size_t)b->lda * ldy;
    const size_t wcount = chol_yyt_workspace_doubles(b->lda, kcols);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (ycount + wcount + kcols) * sizeof(double) > free_b / 10 * 9)
        return fail(STBA_ERR_INVALID_ARGUMENT, "the dense form of the Schur complement needs " + std::to_string((ycount + wcount) * 8 / (1 << 20)) +
                    " MiB (6 cameras x 3 landmarks doubles, padded), more than the device has free");
    STBA_TRY(b->Y.alloc(ycount));
    STBA_TRY(b->yv.alloc(schur_dense_partial_doubles(b->n_chunks)));      // (the chunk partials of the camera sums)
    if (wcount) STBA_TRY(b->yws.alloc(wcount));
    STBA_HIP(hipMemsetAsync(b->Y, 0, ycount * sizeof(double), b->st));
    b->ldy = ldy; b->ykcols = kcols;
    return STBA_OK;
}

// where the landmark inversion in front of a Schur step puts the root of the inverse: only the dense form reads it
static double* ba_rinv(stba_ba* b) { return b->schur_mode == STBA_SCHUR_DENSE ? b->Rinv9.get() : nullptr; }

// S (lower triangle), rhs, Hcc, gc from the linearisation and the inverse landmark blocks: the pair plan or the dense product
static int ba_schur_step(stba_ba* b) {
    if (b->schur_mode == STBA_SCHUR_DENSE) {
        STBA_TRY(ba_dense_alloc(b));
        SchurDenseArgs da;
        da.n_cams = b->nc; da.n_chunks = b->n_chunks;
        da.chunk_begin = b->chunk_begin; da.chunk_end = b->chunk_end; da.cam_chunk_start = b->cam_chunk_start; da.cam_perm = b->cam_perm;
        da.obs_cam = b->obs_cam; da.obs_pt = b->obs_pt;
        da.J8 = b->J8; da.omask = b->omask; da.Jc12 = ba_general_jc(b); da.r = b->r; da.Hinv6 = b->Hinv6; da.Rinv9 = b->Rinv9; da.gp = b->gp;
        da.Y = b->Y; da.ldy = b->ldy; da.kcols = b->ykcols; da.partial = b->yv; da.ws = b->yws; da.dup_run = b->dup_run;
        da.S = b->S(); da.lda = b->lda; da.rhs = b->rhs(); da.Hcc = b->Hcc; da.gc = b->gc;
        return launch_schur_dense(da, b->st);
    }
    SchurArgs sa;
    sa.task_cam = b->task_cam; sa.cam_start = b->cam_start; sa.task_col_lo = b->task_col_lo; sa.task_col_hi = b->task_col_hi;
    sa.row_col_ptr = b->row_col_ptr; sa.row_cols = b->row_cols; sa.max_cols = b->max_cols; sa.cam_perm = b->cam_perm;
    sa.J8 = b->J8; sa.omask = b->omask; sa.Jc12 = ba_general_jc(b); sa.r = b->r; sa.Hinv6 = b->Hinv6; sa.gp = b->gp;
    sa.S = b->S(); sa.lda = b->lda; sa.rhs = b->rhs(); sa.Hcc = b->Hcc; sa.gc = b->gc;
    sa.obs_pt = b->obs_pt; sa.pair_begin = b->pair_begin; sa.pair_end = b->pair_end; sa.pair_rec = b->pair_rec;
    sa.task_vs_ptr = b->task_vs_ptr; sa.vs_first = b->vs_first; sa.mode = b->schur_plan_mode;
    if (b->lm_slices) {
        sa.task_p_lo = b->task_p_lo; sa.task_p_hi = b->task_p_hi; sa.task_part_off = b->task_part_off; sa.part = b->schur_part;
        sa.row_task_ptr = b->row_task_ptr; sa.row_tasks = b->row_tasks; sa.n_cams = b->nc;
    }
    sa.ablate = knob_int("STBA_SCHUR_ABLATE", 0);
    return launch_schur_rows(sa, b->n_tasks, b->st);
}

static int ba_build_reduced(stba_ba* b, const Damping& dm) {
    const int init_scale = b->scale_init ? 0 : 1;
    // (the three extras vectors behind S -- diag, gc, rhs -- are zeroed on the way; the scalar slots are kept)
    double* extras = b->Sbuf + (size_t)b->lda * b->lda;
    if (!dm.explicit_d)
        STBA_TRY(launch_point_damp_invert(b->np, b->Hpp6, b->pt_fixed, b->scale_p, init_scale, dm.use_scaling, dm.radius, dm.dmin,
                                          dm.dmax, b->dp, b->Hinv6, ba_rinv(b), extras, 3 * b->lda, b->st));
    else {
        STBA_TRY(launch_point_invert(b->np, b->Hpp6, b->dp, b->pt_fixed, b->Hinv6, ba_rinv(b), b->st));
        STBA_HIP(hipMemsetAsync(extras, 0, 3 * (size_t)b->lda * sizeof(double), b->st));
    }
    // S is zeroed (pair plan) or overwritten (dense product) by the Schur step itself
    STBA_TRY(ba_schur_step(b));
    STBA_TRY(ba_prior_blocks(b));
    STBA_TRY(ba_between_blocks(b, true));
    if (!b->ar && !dm.explicit_d && b->n == 6 * b->nc) {
        // one rank: camera blocks, LM diagonal, damping and padding in one launch
        STBA_TRY(launch_reduced_finalize(b->nc, b->n, b->Hcc, b->gc, b->cam_fixed, b->S(), b->lda, b->rhs(), b->ex_diag(), b->ex_gc(),
                                         b->scale_c, init_scale, dm.use_scaling, dm.radius, dm.dmin, dm.dmax, b->dc, 0, b->st));
        b->scale_init = true;
        return STBA_OK;
    }
    STBA_TRY(launch_reduced_add_camera(b->nc, b->Hcc, b->gc, b->S(), b->lda, b->rhs(), b->ex_diag(), b->ex_gc(),
                                       b->st));
    if (b->ar) {
        // pack the lower triangle + extras (half the bytes on the wire: 144 MB instead of 288 MB at C5),
        // sum across ranks, unpack
        if (b->pk_state == 0) STBA_TRY(ba_plan_pack(b));
        const unsigned pgrid = (unsigned)((b->pack_count() + 255) / 256);
        if (b->pk_state == 2) hipLaunchKernelGGL(blk_pack_kernel, dim3(pgrid), dim3(256), 0, b->st, b->Sbuf, b->lda, b->pk_blocks, b->pk_nz, b->Spack, 1);
        else hipLaunchKernelGGL(tri_pack_kernel, dim3(b->n + 1), dim3(256), 0, b->st, b->Sbuf, b->lda, b->n, b->Spack, 1);
        ba_collect_allreduce_time(b);                     // (a previous build's pair, if nobody has read it yet)
        if (b->ar_timing_on) {
            if (!b->ev_ar[0]) { STBA_HIP(hipEventCreate(&b->ev_ar[0])); STBA_HIP(hipEventCreate(&b->ev_ar[1])); }
            STBA_HIP(hipEventRecord(b->ev_ar[0], b->st));
        }
        if (b->ar(b->ar_user, b->Spack, b->pack_count(), b->st) != 0)
            return fail(STBA_ERR_CALLBACK, "all-reduce hook failed");
        if (b->ar_timing_on) { STBA_HIP(hipEventRecord(b->ev_ar[1], b->st)); b->ar_timing_pending = true; }
        b->ar_bytes += (double)b->pack_count() * sizeof(double);
        b->ar_calls += 1;
        if (b->pk_state == 2) hipLaunchKernelGGL(blk_pack_kernel, dim3(pgrid), dim3(256), 0, b->st, b->Sbuf, b->lda, b->pk_blocks, b->pk_nz, b->Spack, 0);
        else hipLaunchKernelGGL(tri_pack_kernel, dim3(b->n + 1), dim3(256), 0, b->st, b->Sbuf, b->lda, b->n, b->Spack, 0);
        STBA_HIP(hipGetLastError());
    }
    if (!dm.explicit_d && b->n == 6 * b->nc) {
        // behind the cross-rank sum: LM diagonal of the summed diag(Hcc), damping and padding in ONE launch, as on one rank
        STBA_TRY(launch_reduced_finalize(b->nc, b->n, b->Hcc, b->gc, b->cam_fixed, b->S(), b->lda, b->rhs(), b->ex_diag(), b->ex_gc(),
                                         b->scale_c, init_scale, dm.use_scaling, dm.radius, dm.dmin, dm.dmax, b->dc, 1, b->st));
        b->scale_init = true;
        return STBA_OK;
    }
    if (!dm.explicit_d)
        STBA_TRY(launch_lm_diagonal(b->n, 1, 1, 2, b->ex_diag(), b->scale_c, init_scale, dm.use_scaling, dm.radius,
                                    dm.dmin, dm.dmax, b->dc, b->st));
    b->scale_init = true;
    STBA_TRY(launch_reduced_damp(b->n, b->dc, b->cam_fixed, b->S(), b->lda, b->rhs(), b->st));
    return chol_prepare_padding_dev(b->S(), b->lda, b->n, b->rhs(), b->st);
}

// cost slot + per-rank |gp|_inf slot, filled before the reduced system is built
// (behind ba_linearize_lm + ba_normal_blocks: the cost of the linearisation point -> *cost2_dev and the cost slot, the
// |gp| maxima of the landmark-block workgroups -> this rank's slot, the rest of the scalar block zeroed)
static int ba_fill_scalar_slots(stba_ba* b, double* cost2_dev) {
    return launch_linear_finish(b->cost_partial, b->n_cost(), b->upd_partial_p, point_blocks_grid(b->np), cost2_dev, b->ex_scalar(), b->lda,
                                SC_COST2, SC_GPMAX0 + b->rank, b->st);
}

// the trial block and the factorisation's flag into mapped host memory (several ranks; one rank: trial_finish_kernel does it)
__global__ void export_trial_kernel(const double* __restrict__ trial, const int* __restrict__ flag, double* __restrict__ out, double seq) {
    __shared__ double hp[TS_BLOCK];
    const int k = threadIdx.x;
    if (k == TS_SPEC_COST2) hp[k] = (double)flag[0];
    else if (k < TS_BLOCK) hp[k] = trial[k];
    __syncthreads();
    stamped_store_wave(out, hp, TS_BLOCK, seq, k);      // (one wave of 64; a stamped block: the host validates every line)
}

// back-substitution of the LM loop: dxp, and on the way the trial point (landmarks and cameras) + its step statistics
static int ba_backsub_trial(stba_ba* b) {
    BacksubUpdate up{b->pts[b->cur], b->pt_fixed, b->dp, b->pts[b->cur ^ 1], b->upd_partial_p,
                     b->nc, b->cams[b->cur], b->cam_fixed, b->ex_gc(), b->dc, b->cams[b->cur ^ 1], b->upd_partial_c};
    // (an inexact step: m = -(J d)^T (r + J d / 2), the landmark priors' rows included)
    if (b->iterative) { up.r_model = b->r; up.obs_pt = b->obs_pt; up.lp = b->landmark_prior_rows(); }
    return launch_backsub(b->np, b->pt_start, b->obs_cam, b->J8, b->omask, b->Hinv6, b->gp, b->dxc, b->dxp, b->st, &up, ba_general_jc(b));
}

// trial point: both manifold updates (one launch), the residual-only kernel, and ONE launch that finishes every sum of
// the trial block -- and, when host_out is given (nobody watching), writes the block and the factorisation's flag straight
// into mapped host memory as a stamped block: the host polls it instead of a device-to-host copy + stream synchronisation,
// and the stream can go on
// (updated: the back-substitution kernel has made the trial point and the partial sums of its step already, see ba_backsub_trial)
// (with_jac: the stream is going to linearise at the trial point anyway (speculation, see ba_run_lm) -- then THAT kernel
// evaluates the trial point: residuals, Jacobian records and the cost partials in one pass instead of a residual-only pass
// followed by the full one)
static int ba_trial(stba_ba* b, double* host_out, bool updated = false, bool with_jac = false, double host_seq = 0.0) {
    const int cur = b->cur, nxt = cur ^ 1;
    const int cb = updated ? backsub_cam_grid(b->nc) : (b->nc + 255) / 256, pb = updated ? backsub_grid(b->np) : (b->np + 255) / 256;
    if (!updated)
        STBA_TRY(launch_update(b->nc, b->np, b->cams[cur], b->pts[cur], b->dxc, b->dxp, b->cam_fixed, b->pt_fixed,
                               b->ex_gc(), b->dc, b->gp, b->dp, b->cams[nxt], b->pts[nxt], b->upd_partial_c,
                               b->upd_partial_p, b->st));
    static_assert(TS_COST2 == 0 && TS_STEP2 == 1 && TS_X2 == 2 && TS_MODEL == 3 && TS_TIMEOUT == 4 && TS_CAM == 5 && TS_COUNT == 8 &&
                  TS_SPEC_COST2 == 8 && TS_LIN_COST2 == 9 && TS_LIN_GMAX == 10 && TS_BLOCK == 11, "trial_finish_kernel writes this layout");
    if (with_jac) STBA_TRY(ba_linearize_lm(b, nxt));
    else STBA_TRY(ba_linearize_dispatch(b, nxt, false));
    STBA_TRY(launch_trial_finish(b->cost_partial, b->n_cost(), b->upd_partial_p, b->np > 0 ? pb : 0, b->upd_partial_c, cb, b->flag,
                                 b->ex_scalar() + SC_COST2, b->ex_scalar() + SC_GPMAX0, b->world, b->ex_gc(), b->n, b->trial,
                                 b->ar ? nullptr : host_out, host_seq, b->st));
    if (b->ar) {
        if (b->ar(b->ar_user, b->trial, TS_TIMEOUT + 1, b->st) != 0) return fail(STBA_ERR_CALLBACK, "all-reduce hook failed");
        // (several ranks: the block goes to the host behind the cross-rank sum of its first five entries)
        if (host_out) hipLaunchKernelGGL(export_trial_kernel, dim3(1), dim3(64), 0, b->st, b->trial, b->flag, host_out, host_seq);
        STBA_HIP(hipGetLastError());
    }
    return STBA_OK;
}

// reads {cost2, gpmax slots, gc} after a reduced-system build and returns cost / gradient max norm
static int ba_read_linear_scalars(stba_ba* b, double* cost, double* gmax) {
    std::vector<double> h((size_t)SC_GPMAX0 + b->world);
    std::vector<double> g((size_t)b->n);
    STBA_TRY(download(h.data(), b->ex_scalar(), h.size(), b->st));
    STBA_TRY(download(g.data(), b->ex_gc(), g.size(), b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    *cost = 0.5 * h[SC_COST2];
    double m = 0.0;
    for (int k = 0; k < b->world; ++k) m = std::max(m, h[SC_GPMAX0 + k]);
    for (double v : g) m = std::max(m, std::fabs(v));
    *gmax = m;
    return STBA_OK;
}

// covariance (covariance.hip): linearisation, landmark blocks and the UNDAMPED reduced system at the current parameters, through the
// explicit-damping path of stba_ba_reduced_system with dc = dp = 0 (constant dofs get their 1 on the diagonal as always).  The LM
// state stays as it was: parameters and their buffers, the Jacobi scale (ba_build_reduced marks it made; this path made none) and
// the speculation's stamped block; every solve starts with a linearisation of its own.
static int ba_cov_build(stba_ba* b) {
    const bool scale_init = b->scale_init;
    STBA_TRY(ba_linearize(b, b->cur, b->trial + TS_COST2));
    STBA_TRY(ba_normal_blocks(b));
    STBA_HIP(hipMemsetAsync(b->dc, 0, (size_t)b->n * sizeof(double), b->st));
    STBA_HIP(hipMemsetAsync(b->dp, 0, (size_t)b->np * 3 * sizeof(double), b->st));
    STBA_HIP(hipMemsetAsync(b->ex_scalar(), 0, (size_t)b->lda * sizeof(double), b->st));
    Damping dm;
    dm.explicit_d = true;
    const int rc = ba_build_reduced(b, dm);
    b->scale_init = scale_init;
    STBA_TRY(rc);
    b->have_lin = b->have_blocks = true;
    b->have_reduced = b->have_dxc = b->have_dxp = false;
    return STBA_OK;
}

// ---- ITERATIVE_SCHUR: the reduced camera system applied implicitly and solved by PCG (iterative_schur.hip).
// Same unknowns, damping and constant dofs as the direct path: with eta -> 0 the step is the direct path's step.
static PcgVecs pcg_vecs(stba_ba* b) {
    PcgVecs v;
    const size_t L = (size_t)b->lda, nw = (size_t)is_vec_grid(b->nc);
    v.x = b->dxc; v.r = b->pcg_vec; v.z = b->pcg_vec + L; v.p = b->pcg_vec + 2 * L; v.q = b->pcg_vec + 3 * L;
    v.b = b->rhs(); v.Minv = b->pcg_minv;
    v.part_rz = b->pcg_part; v.part_pq = b->pcg_part + nw; v.part_q = b->pcg_part + 2 * nw;
    v.state = b->pcg_state;
    return v;
}

static int ba_pcg_alloc(stba_ba* b) {
    STBA_TRY(b->pcg_vec.alloc(4 * (size_t)b->lda));
    STBA_TRY(b->pcg_minv.alloc((size_t)b->nc * 36));
    STBA_TRY(b->pcg_sj.alloc((size_t)std::max(b->n_chunks, 1) * 24));
    STBA_TRY(b->pcg_part.alloc(3 * (size_t)is_vec_grid(b->nc)));
    STBA_TRY(b->pcg_state.alloc(1));
    STBA_HIP(hipMemsetAsync(b->pcg_vec, 0, 4 * (size_t)b->lda * sizeof(double), b->st));
    STBA_HIP(hipMemsetAsync(b->pcg_state, 0, sizeof(PcgState), b->st));
    STBA_HIP(hipMemsetAsync(b->flag, 0, sizeof(int), b->st));       // (no factorisation: the trial block's flag stays 0)
    return STBA_OK;
}

// landmark pass of one product: zp (in dxp) = V^-1 (-gp - W^T x); gp = null for S x.  skip: the PCG's state (null: always run)
static int ba_is_landmark_pass(stba_ba* b, const double* x, const double* gp, PcgState* skip) {
    BacksubUpdate up{};
    up.skip = skip ? &skip->done : nullptr;
    return launch_backsub(b->np, b->pt_start, b->obs_cam, b->J8, b->omask, b->Hinv6, gp, x, b->dxp, b->st, &up, ba_general_jc(b));
}
// camera pass: y = (Hcc + D) p + W zp (IS_FINAL_APPLY, p^T y partials into pq_part) | y = -gc - W zp (IS_FINAL_RHS)
static int ba_is_camera_pass(stba_ba* b, int mode, const double* p, double* y, double* pq_part, const PcgState* skip) {
    STBA_TRY(launch_is_cam_gather(b->n_chunks, b->chunk_begin, b->chunk_end, b->cam_perm, b->obs_pt, b->J8, b->omask, ba_general_jc(b),
                                  b->dxp, skip, b->cam_partial, b->st));
    return launch_is_cam_final(b->nc, mode, b->cam_chunk_start, b->cam_partial, b->Hcc, b->dc, b->gc, b->cam_fixed, p, y, pq_part, skip, b->st);
}
static int ba_is_precond(stba_ba* b, int kind) {
    if (kind == STBA_PRECOND_SCHUR_JACOBI)
        STBA_TRY(launch_is_sj_gather(b->n_chunks, b->no, b->chunk_begin, b->chunk_end, b->cam_perm, b->obs_cam, b->obs_pt, b->J8, b->omask,
                                     ba_general_jc(b), b->Hinv6, b->pcg_sj, b->st));
    return launch_is_precond(b->nc, kind, b->Hcc, b->dc, b->scale_c, b->cam_fixed, b->cam_chunk_start, b->pcg_sj, b->pcg_minv, b->st);
}
// reduced right-hand side rhs = -(gc - W V^-1 gp): the landmark pass with x = 0, then the camera pass
static int ba_is_rhs(stba_ba* b) {
    STBA_HIP(hipMemsetAsync(b->dxc, 0, (size_t)b->n * sizeof(double), b->st));
    STBA_TRY(ba_is_landmark_pass(b, b->dxc, b->gp, nullptr));
    return ba_is_camera_pass(b, IS_FINAL_RHS, nullptr, b->rhs(), nullptr, nullptr);
}
// what ba_build_reduced makes, without S: damped landmark inverses, camera blocks, the LM diagonal, the right-hand side and the
// preconditioner of this iteration
static int ba_build_implicit(stba_ba* b, const Damping& dm) {
    const int init_scale = b->scale_init ? 0 : 1;
    if (!dm.explicit_d)
        STBA_TRY(launch_point_damp_invert(b->np, b->Hpp6, b->pt_fixed, b->scale_p, init_scale, dm.use_scaling, dm.radius, dm.dmin,
                                          dm.dmax, b->dp, b->Hinv6, nullptr, b->ex_diag(), 3 * b->lda, b->st));
    else {
        STBA_TRY(launch_point_invert(b->np, b->Hpp6, b->dp, b->pt_fixed, b->Hinv6, nullptr, b->st));
        STBA_HIP(hipMemsetAsync(b->ex_diag(), 0, 3 * (size_t)b->lda * sizeof(double), b->st));
    }
    STBA_TRY(ba_camera_blocks(b));
    STBA_TRY(launch_is_cam_setup(b->nc, b->Hcc, b->gc, b->ex_diag(), b->ex_gc(), b->scale_c, init_scale, dm.use_scaling, dm.radius, dm.dmin,
                                 dm.dmax, b->dc, dm.explicit_d ? 1 : 0, b->st));
    if (!dm.explicit_d) b->scale_init = true;
    STBA_TRY(ba_is_rhs(b));
    return ba_is_precond(b, b->pcg_precond);
}
static int ba_build(stba_ba* b, const Damping& dm) { return b->iterative ? ba_build_implicit(b, dm) : ba_build_reduced(b, dm); }

// PCG on the reduced system into dxc.  check_every iterations are enqueued at a time, then the solve's state travels to the host
// as a stamped block; every kernel of an iteration behind the device's decision returns at once.  *fail: Ceres' FAILURE (the LM
// step is not ok)
static int ba_pcg_solve(stba_ba* b, int* fail_out) {
    const PcgVecs v = pcg_vecs(b);
    STBA_TRY(launch_is_vec(b->nc, IS_VEC_INIT, v, b->st));
    STBA_TRY(launch_is_check(b->nc, IS_CHECK_INIT, v, b->pcg_eta, b->pcg_min, b->pcg_max, b->st));
    if (!b->pcg_host.host) STBA_TRY(b->pcg_host.alloc((size_t)stamped_doubles(4)));
    double hs[4] = {0.0, 0.0, 0.0, 0.0};
    long enqueued = 0;
    while (true) {
        for (int k = 0; k < b->pcg_check; ++k) {
            STBA_TRY(launch_is_vec(b->nc, IS_VEC_DIR, v, b->st));
            STBA_TRY(ba_is_landmark_pass(b, v.p, nullptr, b->pcg_state));
            STBA_TRY(ba_is_camera_pass(b, IS_FINAL_APPLY, v.p, v.q, v.part_pq, b->pcg_state));
            STBA_TRY(launch_is_vec(b->nc, IS_VEC_UPDATE, v, b->st));
            STBA_TRY(launch_is_check(b->nc, IS_CHECK_ITER, v, b->pcg_eta, b->pcg_min, b->pcg_max, b->st));
        }
        enqueued += b->pcg_check;
        const double seq = (b->pcg_seq += 1.0);
        STBA_TRY(launch_is_export(b->pcg_state, b->pcg_host.dev, seq, b->st));
        STBA_TRY(stamped_wait(b->pcg_host.host, 4, [seq](double st) { return st == seq; }, hs, hip_stream_state(b->st), "PCG state", 120.0));
        if (hs[0] != 0.0) break;
        if (enqueued > (long)b->pcg_max + b->pcg_check) return fail(STBA_ERR_HIP, "PCG: the device did not stop at max_iterations");
    }
    b->pcg_last_it = (int)hs[1];
    b->pcg_last_cap = hs[3] != 0.0 ? 1 : 0;
    *fail_out = hs[2] != 0.0 ? 1 : 0;
    return STBA_OK;
}
// the last solve belongs to an LM iteration (not to a trial step the loop discards behind a late convergence test)
static void ba_pcg_account(stba_ba* b, int lm_iter) {
    if (lm_iter >= 1) { b->pcg_per_iter.resize((size_t)lm_iter, 0); b->pcg_per_iter[(size_t)lm_iter - 1] = b->pcg_last_it; }
    b->pcg_sum.iterations_total += b->pcg_last_it;
    b->pcg_sum.solves += 1;
    b->pcg_sum.hit_cap += b->pcg_last_cap;
    b->pcg_sum.max_iterations_in_a_solve = std::max(b->pcg_sum.max_iterations_in_a_solve, b->pcg_last_it);
    b->pcg_sum.last_eta = b->pcg_eta;
}

// ---- inner iterations (Solver::Options::use_inner_iterations; inner_iterations.hip)
static InnerObs inner_obs_args(const stba_ba* b) {
    InnerObs o;
    o.n_cams = b->nc; o.n_pts = b->np;
    o.pt_start = b->pt_start; o.obs_cam = b->obs_cam; o.obs_pt = b->obs_pt; o.feat = b->feat;
    o.cam_perm = b->cam_perm; o.chunk_begin = b->chunk_begin; o.chunk_end = b->chunk_end; o.cam_chunk_start = b->cam_chunk_start;
    return o;
}
// one sweep of the ordering over parameter buffer `which`, in place: the groups in ascending id, in each the camera blocks, then the
// landmarks (a group is an independent set: the two launches see nothing of each other's blocks).  gate: null, or the device's
// verdict on the trial point (0: every workgroup returns at once)
static int ba_inner_sweep_enqueue(stba_ba* b, int which, const int* gate) {
    const InnerObs o = inner_obs_args(b);
    const int n_cam_entries = (int)b->inner.plan.cam.size();
    for (const auto& g : b->inner.plan.groups) {
        STBA_TRY(launch_inner_cameras(o, g.cam_hi - g.cam_lo, b->inner.cam + g.cam_lo, b->inner.mask + g.cam_lo, b->cams[which],
                                      b->pts[which], b->inner.it + g.cam_lo, gate, b->st));
        STBA_TRY(launch_inner_points(o, g.pt_hi - g.pt_lo, b->inner.pt + g.pt_lo, b->cams[which], b->pts[which],
                                     b->inner.it + n_cam_entries + g.pt_lo, gate, b->st));
    }
    return STBA_OK;
}
// behind the trial point x+ in buffer cur ^ 1 (enqueued before the host reads the trial block): the gate, the sweep x+ -> x*, the
// cost at x* by the trial pass's residual kernel -> inner.sc[0] (cost2), and the ambient |x - x*|^2 -> inner.sc[1]
static int ba_inner_after_trial(stba_ba* b) {
    const int cur = b->cur, nxt = cur ^ 1;
    STBA_TRY(launch_inner_gate(b->trial, b->flag, TS_COST2, TS_MODEL, TS_CAM + 2, b->inner.gate, b->st));
    STBA_TRY(ba_inner_sweep_enqueue(b, nxt, b->inner.gate));
    STBA_TRY(ba_cost_only(b, nxt, b->inner.sc));
    STBA_TRY(launch_inner_step2(b->nc, b->np, b->cams[cur], b->pts[cur], b->cams[nxt], b->pts[nxt], b->inner.part, b->st));
    return launch_sum_partials(b->inner.part, inner_step_grid(b->nc, b->np), 1, 1, b->inner.sc + 1, b->st);
}
static void inner_summary_reset(stba_ba* b) {
    b->inner.sum = stba_inner_summary{};
    b->inner.sum.struct_size = sizeof(stba_inner_summary);
    b->inner.sum.disabled_at_iteration = -1;
    b->inner.sum.num_groups = (int)b->inner.plan.groups.size();
    for (int g = 0; g < b->inner.sum.num_groups && g < STBA_INNER_MAX_GROUPS_REPORTED; ++g) {
        const auto& r = b->inner.plan.groups[(size_t)g];
        b->inner.sum.group_size[g] = (r.cam_hi - r.cam_lo) + (r.pt_hi - r.pt_lo);
    }
}

// ---- the steps of a BA solve (ba_run_lm, ba_run_dogleg).  BaSolve is the state of ONE call; what outlives a call (the parameter
// buffers and which is current, the Jacobi scale, the stage cool-down, the stamped blocks' sequence numbers, the events, the PCG,
// dogleg and inner summaries) stays in stba_ba.  The two strategies share steps, not a loop: each keeps its trust region and its
// own order of enqueues.  No step captures anything.
struct BaPending {             // (cost, |g|max) of the linearisation behind iteration `iter`: they arrive with the next trial block
    bool on = false, accepted = false;
    int iter = 0, lin_ev = EV_SPEC_A;     // lin_ev: the event pair around that linearisation
};
struct BaSolve {
    stba_lm_options opt;
    // derived once
    bool fixed = false, timing = false;
    bool deferred_ok = false;   // deferred read of (cost, |g|max) of a freshly linearised point: only when nobody watches the iterations
    int max_iter = 0;
    Damping dm;
    stba_lm_summary s;
    double t_start = 0.0;
    // the loop
    double cost = 0.0, gmax = 0.0;
    int iter = 0, chol_timeouts = 0;
    bool need_build = true;      // reduced system must be (re)built before the next solve
    BaPending pending;
    // phase timing: is the start point's linearisation pair still to be read, the speculation's pair of this iteration, and
    // the end event of the last build (the start of the solve that follows it)
    bool lin_timing_pending = true;
    int spec_ev = EV_SPEC_B, build_end_ev = EV_BUILD_END;
    double* trace = nullptr;
    stba_iteration_callback cb = nullptr;
    void* cb_user = nullptr;
};
struct TrialScalars { double new_cost = 0.0, step_norm = 0.0, x_norm = 0.0, model_change = 0.0; };

static void stop(BaSolve& sv, int type, int reason) { sv.s.termination_type = type; sv.s.termination_reason = reason; }

// (see stba_lm_options::phase_timing: every event costs ~5 us of idle GPU -- with timing off none is enqueued)
static int ba_stamp(stba_ba* b, bool on, int ev) {
    if (on) STBA_HIP(hipEventRecord(b->ev[ev], b->st));
    return STBA_OK;
}
static void ba_add_ms(stba_ba* b, int ev_begin, int ev_end, double* total) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->ev[ev_begin], b->ev[ev_end]) == hipSuccess) *total += ms;
}

// options, summary, the per-solve resets of the engine, the damping's constants.  timed: the strategy has phase events at all
static void ba_solve_begin(stba_ba* b, BaSolve& sv, const stba_lm_options* opt_in, int fixed_iterations, bool timed, double* trace,
                           stba_iteration_callback cb, void* cb_user) {
    if (opt_in) sv.opt = *opt_in; else default_options(&sv.opt);
    memset(&sv.s, 0, sizeof sv.s);
    stop(sv, STBA_NO_CONVERGENCE, STBA_TERM_MAX_ITER);
    sv.t_start = wall_s();
    sv.fixed = fixed_iterations > 0;
    sv.max_iter = sv.fixed ? fixed_iterations : sv.opt.max_num_iterations;
    sv.timing = timed && sv.opt.phase_timing != 0;
    sv.deferred_ok = (cb == nullptr) && !sv.opt.minimizer_progress_to_stdout;
    sv.trace = trace; sv.cb = cb; sv.cb_user = cb_user;
    b->ar_timing_on = sv.timing;
    b->scale_init = false;
    b->ar_ms = 0.0; b->ar_bytes = 0.0; b->ar_calls = 0; b->ar_timing_pending = false;
    memset(&b->pcg_sum, 0, sizeof b->pcg_sum);
    b->pcg_per_iter.clear();
    sv.dm.dmin = sv.opt.min_lm_diagonal; sv.dm.dmax = sv.opt.max_lm_diagonal; sv.dm.use_scaling = sv.opt.jacobi_scaling;
}

// linearisation at parameter buffer `which`: residuals + Jacobians, the landmark blocks, and the cost -> *cost_slot with the
// scalar slots.  jac_done: a with_jac trial pass has made the residuals and Jacobians there already (the speculation).
// timed: the pair ev_pair, ev_pair + 1 is recorded around everything but the scalar fill
static int ba_linearize_point(stba_ba* b, int which, double* cost_slot, bool timed = false, int ev_pair = EV_LIN, bool jac_done = false) {
    STBA_TRY(ba_stamp(b, timed, ev_pair));
    if (!jac_done) STBA_TRY(ba_linearize_lm(b, which));
    STBA_TRY(ba_normal_blocks(b));
    STBA_TRY(ba_stamp(b, timed, ev_pair + 1));
    return ba_fill_scalar_slots(b, cost_slot);
}

// the reduced system at `radius`, inside the event pair ev_pair when the solve is timed
static int ba_build_at(stba_ba* b, BaSolve& sv, double radius, int ev_pair = EV_BUILD) {
    sv.dm.radius = radius;
    STBA_TRY(ba_stamp(b, sv.timing, ev_pair));
    STBA_TRY(ba_build(b, sv.dm));
    STBA_TRY(ba_stamp(b, sv.timing, ev_pair + 1));
    sv.build_end_ev = ev_pair + 1;
    sv.need_build = false;
    return STBA_OK;
}

// the start point, behind its first build: cost and |g|max, row 0, the header.  *go = false: the solve ends here
static int ba_first_point(stba_ba* b, BaSolve& sv, double radius, bool* go) {
    *go = false;
    STBA_TRY(ba_read_linear_scalars(b, &sv.cost, &sv.gmax));
    sv.s.initial_cost = sv.cost;
    trace_start(sv.trace, sv.cost, sv.gmax, radius);
    if (sv.opt.minimizer_progress_to_stdout) progress_start(sv.cost, sv.gmax, radius);     // (the BA loops alone print a header)
    // Ceres: a residual block that returns a non-finite value fails its evaluation, and a failed evaluation of the START
    // point ends the solve as FAILURE before any step ("Initial residual and Jacobian evaluation failed"); at a trial
    // point it is an unsuccessful step -- the rho test rejects a non-finite cost.  (oracle.c: orc_ba_solve)
    if (!std::isfinite(sv.cost)) stop(sv, STBA_FAILURE, STBA_TERM_SOLVER_FAIL);
    else if (!sv.fixed && sv.gmax <= sv.opt.gradient_tolerance) stop(sv, STBA_CONVERGENCE, STBA_TERM_GRADIENT);
    else *go = sv.max_iter > 0;
    return STBA_OK;
}

// the pending read: (cost, |g|max) of the linearisation behind iteration pending.iter have arrived.  true: that iteration had
// converged on its gradient -- the test comes first, whatever the loop has done since
static bool ba_take_pending(BaSolve& sv, double cost, double gmax) {
    sv.gmax = gmax;
    if (sv.pending.accepted) sv.cost = cost;
    if (sv.trace) sv.trace[(size_t)sv.pending.iter * STBA_TRACE_COLS + 2] = gmax;
    sv.pending.on = false;
    return sv.pending.accepted && !sv.fixed && gmax <= sv.opt.gradient_tolerance;
}
// behind the loop (the stream is idle): the loop ended (iteration / radius limit) before the last linearisation's scalars were read
static int ba_take_pending_at_end(stba_ba* b, BaSolve& sv) {
    if (!sv.pending.on) return STBA_OK;
    double c2, g2;
    STBA_TRY(ba_read_linear_scalars(b, &c2, &g2));
    if (ba_take_pending(sv, c2, g2) && (sv.s.termination_reason == STBA_TERM_MAX_ITER || sv.s.termination_reason == STBA_TERM_MIN_RADIUS))
        stop(sv, STBA_CONVERGENCE, STBA_TERM_GRADIENT);
    return STBA_OK;
}

static TrialScalars trial_scalars(const double* ts) {
    return {0.5 * ts[TS_COST2], std::sqrt(ts[TS_STEP2] + ts[TS_CAM + 0]), std::sqrt(ts[TS_X2] + ts[TS_CAM + 1]), ts[TS_MODEL] + ts[TS_CAM + 2]};
}

// The persistent factorisation gave up waiting for a dependency: some of its workgroups were not resident (the
// device is shared with another process).  S is half factored; it is rebuilt from the blocks -- the engine owns
// them -- and this iteration runs again, the factorisation through the stage kernels, which need nothing
// resident (chol_note_timeout: so do the next ones on this device).
// relinearize: a speculative linearisation overwrote the current point's residuals, Jacobians and blocks
static int ba_on_chol_timeout(stba_ba* b, BaSolve& sv, int flag_h, bool relinearize) {
    // One rank: the DEVICE is marked (it is shared with somebody: the next 64 factorisations of anybody on it take the stage
    // kernels).  Several ranks: every rank -- the one that gave up and its peers -- starts the same cool-down of ITS ENGINE, so
    // that all of them factor the identical system with the identical schedule for the same 64 factorisations (the two
    // schedules differ in the last bits, and every rank must hold the same camera blocks); a counter in the shared
    // per-device state (round 5) was decremented by whoever else factored on that device (advisor, round 5).
    if (b->ar) { b->stage_cooldown = 64; if (flag_h == CHOL_FLAG_TIMEOUT) chol_count_timeout(); }
    else chol_note_timeout();
    // (a device that keeps timing out is shared for good: the cool-down is renewed every time, so a long run goes on through
    // the stage kernels instead of failing; only time-outs that come back-to-back without a good iteration in between --
    // the stage kernels cannot time out -- end the solve)
    if (++sv.chol_timeouts > 8) return fail(STBA_ERR_HIP, "dense Cholesky: the persistent program timed out repeatedly");
    if (relinearize) STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2));
    sv.need_build = true;
    --sv.iter;
    return STBA_OK;
}

static int ba_notify(const BaSolve& sv, const StepVerdict& v, double step_norm, double radius) {
    return sv.cb ? sv.cb(sv.cb_user, sv.iter, sv.cost, v.cost_change, sv.gmax, step_norm, radius, v.accepted ? 1 : 0) : 0;
}
// a judged step: the accepted point becomes the current one; the iteration's trace row (its |g|max and radius follow, ba_end_iteration).
// true: the step ended the solve on the parameter or the function tolerance (the callback hears of it; its answer no longer matters)
static bool ba_apply_verdict(stba_ba* b, BaSolve& sv, const StepVerdict& v, bool step_ok, const TrialScalars& t, double radius) {
    if (v.accepted) {
        b->cur ^= 1;
        sv.cost = t.new_cost;
        ++sv.s.num_successful_steps;
    }
    trace_step(sv.trace, sv.iter, step_ok, sv.cost, t.new_cost, v, sv.gmax, t.step_norm, radius);
    if (!v.stop) return false;
    stop(sv, STBA_CONVERGENCE, v.stop);
    (void)ba_notify(sv, v, t.step_norm, radius);
    return true;
}
// the iteration's row is complete: |g|max and the new radius into it, the progress line, the callback.  true: the solve ends here
static bool ba_end_iteration(BaSolve& sv, const StepVerdict& v, double step_norm, double radius) {
    if (sv.trace) { sv.trace[(size_t)sv.iter * STBA_TRACE_COLS + 2] = sv.gmax; sv.trace[(size_t)sv.iter * STBA_TRACE_COLS + 5] = radius; }
    if (sv.opt.minimizer_progress_to_stdout) progress_step(sv.iter, sv.cost, v, sv.gmax, step_norm, radius);
    if (ba_notify(sv, v, step_norm, radius) != 0) { stop(sv, STBA_CONVERGENCE, STBA_TERM_USER); return true; }
    if (!sv.pending.on && v.accepted && !sv.fixed && sv.gmax <= sv.opt.gradient_tolerance) {
        stop(sv, STBA_CONVERGENCE, STBA_TERM_GRADIENT);
        return true;
    }
    return false;
}

static int ba_solve_end(stba_ba* b, BaSolve& sv, double radius, stba_lm_summary* sum) {
    STBA_HIP(hipStreamSynchronize(b->st));
    STBA_TRY(ba_take_pending_at_end(b, sv));
    ba_collect_allreduce_time(b);
    sv.s.ms_allreduce = b->ar_ms; sv.s.allreduce_bytes = b->ar_bytes; sv.s.allreduce_calls = b->ar_calls;
    finish_summary(&sv.s, sv.iter, sv.cost, radius, sv.gmax, sv.t_start);
    b->pcg_sum.linear_solve_ms = b->iterative ? sv.s.ms_solve : 0.0;
    ba_invalidate(b);
    if (sum) *sum = sv.s;
    return STBA_OK;
}

// ---- ba_run_lm's own steps
// factor + solve into dxc: the PCG (*pcg_fail: the step is not ok), or the dense Cholesky -- the persistent program, or the stage kernels
static int ba_factor_solve(stba_ba* b, int* pcg_fail) {
    if (b->iterative) return ba_pcg_solve(b, pcg_fail);
    // (several ranks behind a time-out of ANY rank: this engine's own cool-down -- every rank counts the same factorisations
    // through the stage kernels, whatever else shares its device or its process)
    if (b->stage_cooldown > 0) { --b->stage_cooldown; return chol_factor_solve_stages(b->S(), b->lda, b->n, b->dxc, b->flag, b->st); }
    return chol_factor_solve_dev(b->S(), b->lda, b->n, b->dxc, b->flag, b->st);
}

// the sweep ran behind a valid step (its gate saw the same valid step): the candidate becomes x* (Ceres DoInnerIterationsIfNeeded),
// isc = {cost2 at x*, |x - x*|^2}.  Returns whether the sweep brought the candidate below the current cost
static bool ba_inner_verdict(stba_ba* b, const BaSolve& sv, const double* isc, TrialScalars& t, bool* inner_active) {
    const double inner_cost = 0.5 * isc[0];
    ++b->inner.sum.sweeps;
    t.model_change += t.new_cost - inner_cost;
    const double progress = 1.0 - inner_cost / t.new_cost;
    t.new_cost = inner_cost;
    t.step_norm = std::sqrt(isc[1]);
    if (!(progress > b->inner.tol)) { *inner_active = false; b->inner.sum.disabled_at_iteration = sv.iter; }
    return inner_cost < sv.cost;
}

// Which event pairs the linearisation and the build behind a judged step belong to.  Watched, the loop reads both at once: its
// own pairs.  Deferred, the host reads them one solve later, with the next trial block: the build has a pair of its own, and the
// linearisation's is the pair the speculation used LAST -- recorded by the speculation itself if the step it ran ahead of was
// accepted, by the re-linearisation otherwise; the next iteration's speculation records into the other one, so the pair is
// still intact when the host reads it.
struct BaStepEvents { int lin, build; };
static BaStepEvents ba_step_events(const BaSolve& sv) {
    return sv.deferred_ok ? BaStepEvents{sv.spec_ev, EV_DBUILD} : BaStepEvents{EV_LIN, EV_BUILD};
}

// everything behind a judged step that has not ended the solve: the linearisation at the (new) current point -- unless the stream
// has done so already --, the reduced system at the new radius, and the pending or immediate read of its cost and |g|max
static int ba_advance(stba_ba* b, BaSolve& sv, double radius, bool accepted, bool speculated) {
    sv.need_build = true;
    if ((accepted || sv.fixed) && !(sv.fixed && sv.iter >= sv.max_iter)) {
        const BaStepEvents e = ba_step_events(sv);
        if (!(speculated && accepted)) STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2, sv.timing, e.lin));
        // gradient of the new point is needed for the convergence test: it arrives with the
        // next reduced-system build (one collective per iteration); build it now.
        STBA_TRY(ba_build_at(b, sv, radius, e.build));
        sv.lin_timing_pending = false;
        if (sv.deferred_ok) {
            // (cost, |g|max) of the new point arrive with the next iteration's trial block
            sv.pending.on = true; sv.pending.accepted = accepted; sv.pending.iter = sv.iter; sv.pending.lin_ev = e.lin;
        } else {
            double c2, g2;
            STBA_TRY(ba_read_linear_scalars(b, &c2, &g2));
            if (sv.timing) { ba_add_ms(b, e.lin, e.lin + 1, &sv.s.ms_linearize); ba_add_ms(b, e.build, e.build + 1, &sv.s.ms_schur); }
            sv.gmax = g2;
            if (accepted) sv.cost = c2;   // same value as new_cost up to summation order
        }
    } else if (speculated && !accepted) {
        // the speculative linearisation overwrote the residuals, Jacobians and blocks of the current point
        STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2));
    }
    return STBA_OK;
}

static int ba_run_lm(stba_ba* b, const stba_lm_options* opt_in, int fixed_iterations, stba_lm_summary* sum,
                     double* trace, stba_iteration_callback cb, void* cb_user) {
    if (b->world > SC_MAX_WORLD) return fail(STBA_ERR_INVALID_ARGUMENT, "world size too large");
    BaSolve sv;
    ba_solve_begin(b, sv, opt_in, fixed_iterations, true, trace, cb, cb_user);
    const stba_lm_options& opt = sv.opt;
    stba_lm_summary& s = sv.s;
    TrustRegion region(opt);
    // inner iterations: on while the engine has them and no sweep has switched them off (rule 6)
    bool inner_active = b->inner.on;
    if (b->inner.on) {
        inner_summary_reset(b);
        if (sv.timing) for (auto& e : b->inner.ev) if (!e) STBA_HIP(hipEventCreate(&e));
    }
    static const bool SPECULATE = knob_int("STBA_LM_SPECULATE", 1) != 0;

    // ---- iteration 0: linearise at the start point
    STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2, sv.timing, EV_LIN));
    bool first = true;
    while (true) {
        if (!first) {
            if (sv.iter >= sv.max_iter) {
                stop(sv, sv.fixed ? STBA_CONVERGENCE : STBA_NO_CONVERGENCE, sv.fixed ? STBA_TERM_FIXED : STBA_TERM_MAX_ITER);
                break;
            }
            if (!sv.fixed && region.below_min(opt)) { stop(sv, STBA_CONVERGENCE, STBA_TERM_MIN_RADIUS); break; }
        }
        // ---- reduced system for the current radius
        // (an event record is a packet of its own on the queue, ~5 us of idle GPU between two kernels: none is recorded that
        // is not needed -- when the system was built behind the previous iteration, that build's end event is the start of
        // this solve)
        const bool built_here = sv.need_build;
        if (sv.need_build) STBA_TRY(ba_build_at(b, sv, region.radius));
        const int solve_start_ev = sv.build_end_ev;
        if (first) {
            bool go = false;
            first = false;
            STBA_TRY(ba_first_point(b, sv, region.radius, &go));
            if (!go) break;
        }
        ++sv.iter;
        // ---- factor + solve, back-substitute, trial point
        int flag_h = 0, pcg_fail = 0;
        STBA_TRY(ba_factor_solve(b, &pcg_fail));
        STBA_TRY(ba_stamp(b, sv.timing, EV_SOLVE_END));
        STBA_TRY(ba_backsub_trial(b));
        STBA_TRY(ba_stamp(b, sv.timing, EV_BACKSUB_END));
        // Nobody watches the iterations and there is one rank: the host learns the trial point's scalars through a stamped
        // block in mapped memory, and meanwhile the stream already linearises AT THE TRIAL POINT -- a step is accepted far
        // more often than not, and the host's round trip (wake-up, decision, enqueue: ~35 us) would otherwise be a
        // bubble on the GPU in every iteration.  A rejected step costs one linearisation at the old point (ba_advance).
        // (With several ranks too: every rank takes the same decision from the same all-reduced block, and the collectives of
        // the speculative build are enqueued on the stream like everything else.)
        // (host-linearised factors: the callback is synchronous host work; iterative Schur: the PCG hands its state to the host
        // anyway, and this path does not speculate -- DESIGN.md 7b)
        // (inner iterations: the sweep moves the trial point before anything is linearised there -- no speculation)
        const bool fast = sv.deferred_ok && SPECULATE && !b->hl_fn && !b->iterative && !inner_active;
        if (fast && !b->ts_host.host) STBA_TRY(b->ts_host.alloc((size_t)stamped_doubles(TS_BLOCK)));
        // (the speculative linearisation IS the evaluation of the trial point: one pass over the observations, not two)
        const bool speculate = fast && !(sv.fixed && sv.iter >= sv.max_iter);
        const double seq = fast ? (b->ts_seq += 1.0) : 0.0;
        STBA_TRY(ba_trial(b, fast ? b->ts_host.dev : nullptr, true, speculate, seq));
        STBA_TRY(ba_stamp(b, sv.timing, EV_TRIAL_END));
        double isc[2] = {0.0, 0.0};
        if (inner_active) {
            if (sv.timing) STBA_HIP(hipEventRecord(b->inner.ev[0], b->st));
            STBA_TRY(ba_inner_after_trial(b));
            if (sv.timing) STBA_HIP(hipEventRecord(b->inner.ev[1], b->st));
        }
        const double* ts = b->ts_vals;
        if (fast) {
            if (speculate) {
                // (its own pair of events, alternating: the previous linearisation's pair is read behind the wait below)
                sv.spec_ev = (sv.spec_ev == EV_SPEC_A) ? EV_SPEC_B : EV_SPEC_A;
                STBA_TRY(ba_linearize_point(b, b->cur ^ 1, b->trial + TS_SPEC_COST2, sv.timing, sv.spec_ev, true));
            }
            // (a polled stamped block, no event: a record between two kernels costs the GPU ~5 us, and the stream goes straight on)
            STBA_TRY(stamped_wait(b->ts_host.host, TS_BLOCK, [seq](double st) { return st == seq; }, b->ts_vals, hip_stream_state(b->st),
                                  "trial point", 120.0));
            flag_h = (int)ts[TS_SPEC_COST2];           // (the host's block carries the flag in that slot)
        } else {
            STBA_TRY(download(b->ts_vals, b->trial, TS_BLOCK, b->st));
            STBA_TRY(download(&flag_h, b->flag, 1, b->st));
            if (inner_active) STBA_TRY(download(isc, b->inner.sc, 2, b->st));
            STBA_HIP(hipStreamSynchronize(b->st));
            if (inner_active && sv.timing) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, b->inner.ev[0], b->inner.ev[1]) == hipSuccess) b->inner.sum.sweep_ms += ms;
            }
        }
        if (pcg_fail) flag_h = 1;            // (the PCG failed: the step is not ok)
        if (sv.pending.on) {
            // (cost2 and |g|max of the build behind the previous iteration: trial_finish_kernel read them on the way)
            if (sv.timing) {
                ba_add_ms(b, sv.pending.lin_ev, sv.pending.lin_ev + 1, &s.ms_linearize);
                ba_add_ms(b, EV_DBUILD, EV_DBUILD_END, &s.ms_schur);
            }
            if (ba_take_pending(sv, 0.5 * ts[TS_LIN_COST2], ts[TS_LIN_GMAX])) {
                // converged at the previous iteration: the trial step just computed is discarded
                --sv.iter;
                stop(sv, STBA_CONVERGENCE, STBA_TERM_GRADIENT);
                break;
            }
        }
        if (b->iterative) ba_pcg_account(b, sv.iter);
        // (several ranks: the decision is COLLECTIVE -- ts[TS_TIMEOUT] is the all-reduced count of ranks whose factorisation timed
        // out, the same number on every rank.  A rank-local decision would leave one rank re-running the iteration, with its
        // all-reduces of a system linearised at the old point, while the others move on: mismatched collectives.)
        if (flag_h == CHOL_FLAG_TIMEOUT || ts[TS_TIMEOUT] > 0.0) {
            STBA_TRY(ba_on_chol_timeout(b, sv, flag_h, speculate));
            continue;
        }
        if (sv.timing) {
            if (sv.lin_timing_pending) ba_add_ms(b, EV_LIN, EV_LIN_END, &s.ms_linearize);
            if (built_here) ba_add_ms(b, EV_BUILD, EV_BUILD_END, &s.ms_schur);
            ba_add_ms(b, solve_start_ev, EV_SOLVE_END, &s.ms_solve);
            ba_add_ms(b, EV_SOLVE_END, EV_BACKSUB_END, &s.ms_backsub);
            // (a polled trial block can reach the host before the event recorded behind its kernel has fired: wait for that one)
            if (fast) (void)hipEventSynchronize(b->ev[EV_TRIAL_END]);
            ba_add_ms(b, EV_BACKSUB_END, EV_TRIAL_END, &s.ms_cost);
        }
        sv.lin_timing_pending = false;
        sv.chol_timeouts = 0;

        TrialScalars t = trial_scalars(ts);
        // (a non-finite trial cost makes the step not ok: row [cost, 0, ., 0, 0], no stop test)
        const bool step_ok = flag_h == 0 && t.model_change > 0.0 && std::isfinite(t.model_change) && std::isfinite(t.new_cost);
        const bool inner_useful = inner_active && step_ok && ba_inner_verdict(b, sv, isc, t, &inner_active);
        const StepVerdict v = judge_step(opt, sv.cost, step_ok, t.new_cost, t.model_change, t.step_norm, t.x_norm, !sv.fixed, inner_useful);
        if (ba_apply_verdict(b, sv, v, step_ok, t, region.radius)) break;
        if (v.accepted) region.accept(v.rho, opt);
        else {
            ++s.num_unsuccessful_steps;
            region.reject();
        }
        STBA_TRY(ba_advance(b, sv, region.radius, v.accepted, speculate));
        if (ba_end_iteration(sv, v, t.step_norm, region.radius)) break;
    }
    return ba_solve_end(b, sv, region.radius, sum);
}

// ---- DOGLEG (Ceres' TrustRegionMinimizer + DoglegStrategy, TRADITIONAL_DOGLEG).  One rank, the dense Schur path.
// Per linearisation: the reduced system at radius 1/mu (ba_build), the persistent Cholesky, the Gauss-Newton back-substitution and
// the terms kernel.  Per trial step: the step kernel at Delta and the trial evaluation, whose stamped block is the host's one wait;
// a rejected step is nothing else.  No speculative linearisation: a rejection re-uses the linearisation, which a speculation at the
// trial point would have overwritten.  The cost and |g|max of a new linearisation arrive with its first trial block (as in
// ba_run_lm), unless somebody watches the iterations.
static int ba_dogleg_alloc(stba_ba* b) {
    if (b->dl_sc) return STBA_OK;
    STBA_TRY(b->dl_uc.alloc((size_t)std::max(b->n, 1)));
    STBA_TRY(b->dl_up.alloc((size_t)std::max(b->np, 1) * 3));
    STBA_TRY(b->dl_part.alloc(dogleg_partial_doubles(b->nc, b->np)));
    STBA_TRY(b->dl_sc.alloc(8));
    return b->dl_host.alloc((size_t)stamped_doubles(DL_BLOCK));
}

// the Gauss-Newton side of a linearisation: factor, back-substitute, the six scalars (the reduced system is built)
static int ba_dogleg_gauss_newton(stba_ba* b, const Damping& dm) {
    STBA_TRY(chol_factor_solve_dev(b->S(), b->lda, b->n, b->dxc, b->flag, b->st));
    STBA_TRY(launch_backsub(b->np, b->pt_start, b->obs_cam, b->J8, b->omask, b->Hinv6, b->gp, b->dxc, b->dxp, b->st, nullptr,
                            ba_general_jc(b)));
    DoglegArgs a;
    a.n_cams = b->nc; a.n_pts = b->np;
    a.pt_start = b->pt_start; a.obs_cam = b->obs_cam; a.obs_pt = b->obs_pt;
    a.J8 = b->J8; a.omask = b->omask; a.Jc12 = ba_general_jc(b);
    a.cam_fixed = b->cam_fixed; a.pt_fixed = b->pt_fixed;
    a.hc = b->ex_diag(); a.gc = b->ex_gc(); a.scale_c = b->scale_c;
    a.Hpp6 = b->Hpp6; a.gp = b->gp; a.scale_p = b->scale_p;
    a.dmin = dm.dmin; a.dmax = dm.dmax;
    a.dxc = b->dxc; a.dxp = b->dxp; a.uc = b->dl_uc; a.up = b->dl_up;
    a.partial = b->dl_part; a.scalars = b->dl_sc;
    a.lp = b->landmark_prior_rows();
    return launch_dogleg_terms(a, b->st);
}

static int ba_dogleg_step(stba_ba* b, double radius, double seq) {
    DoglegStepArgs a;
    a.n_cams = b->nc; a.n_pts = b->np;
    a.scalars = b->dl_sc; a.uc = b->dl_uc; a.up = b->dl_up; a.dxc = b->dxc; a.dxp = b->dxp;
    a.cams = b->cams[b->cur]; a.pts = b->pts[b->cur]; a.cam_fixed = b->cam_fixed; a.pt_fixed = b->pt_fixed;
    a.cams_new = b->cams[b->cur ^ 1]; a.pts_new = b->pts[b->cur ^ 1];
    a.partial_c = b->upd_partial_c; a.partial_p = b->upd_partial_p;
    a.host_out = b->dl_host.dev; a.seq = seq;
    return launch_dogleg_step(a, radius, b->st);
}

constexpr int kMaxConsecutiveInvalidSteps = 5;      // Ceres' Solver::Options::max_num_consecutive_invalid_steps

static int ba_run_dogleg(stba_ba* b, const stba_lm_options* opt_in, stba_lm_summary* sum, double* trace, stba_iteration_callback cb,
                         void* cb_user) {
    STBA_TRY(ba_dogleg_alloc(b));
    if (!b->ts_host.host) STBA_TRY(b->ts_host.alloc((size_t)stamped_doubles(TS_BLOCK)));
    BaSolve sv;
    ba_solve_begin(b, sv, opt_in, 0, false, trace, cb, cb_user);
    const stba_lm_options& opt = sv.opt;
    stba_lm_summary& s = sv.s;
    stba_dogleg_summary ds{};
    ds.struct_size = sizeof ds;
    DoglegRegion region(opt);

    STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2));
    bool need_gn = true, first = true;
    int invalid_in_a_row = 0;
    double hd[DL_BLOCK] = {0.0};

    while (true) {
        if (!first) {
            if (sv.iter >= sv.max_iter) break;
            if (region.below_min(opt)) { stop(sv, STBA_CONVERGENCE, STBA_TERM_MIN_RADIUS); break; }
        }
        if (sv.need_build) STBA_TRY(ba_build_at(b, sv, 1.0 / region.mu));
        if (first) {
            bool go = false;
            first = false;
            STBA_TRY(ba_first_point(b, sv, region.radius, &go));
            if (!go) break;
        }
        ++sv.iter;
        // ---- the Gauss-Newton side, once per linearisation (and per mu escalation); mu >= 1: no solve, the step is invalid
        bool have_gn = true, reused = !need_gn;
        if (need_gn) {
            if (region.can_factor()) {
                STBA_TRY(ba_dogleg_gauss_newton(b, sv.dm));
                ++ds.factorizations; ++ds.gauss_newton_solves;
                need_gn = false;
            } else have_gn = false;
        }
        const double* ts = b->ts_vals;
        if (have_gn) {
            // ---- the trial step: the step kernel at Delta and the trial evaluation, read through the trial block (the one wait)
            const double dseq = (b->dl_seq += 1.0), seq = (b->ts_seq += 1.0);
            STBA_TRY(ba_dogleg_step(b, region.radius, dseq));
            STBA_TRY(ba_trial(b, b->ts_host.dev, true, false, seq));
            STBA_TRY(stamped_wait(b->ts_host.host, TS_BLOCK, [seq](double x) { return x == seq; }, b->ts_vals, hip_stream_state(b->st),
                                  "trial point", 120.0));
            // (the step kernel wrote its block before the trial evaluation began: it is there)
            STBA_TRY(stamped_wait(b->dl_host.host, DL_BLOCK, [dseq](double x) { return x == dseq; }, hd, hip_stream_state(b->st),
                                  "dogleg step", 120.0));
            const int flag_h = (int)ts[TS_SPEC_COST2];
            if (flag_h == CHOL_FLAG_TIMEOUT) {
                // the persistent factorisation gave up (the device is shared): S is rebuilt and factored again through the stage
                // kernels, as in ba_run_lm
                STBA_TRY(ba_on_chol_timeout(b, sv, flag_h, false));
                --ds.factorizations; --ds.gauss_newton_solves;
                need_gn = true;
                continue;
            }
            sv.chol_timeouts = 0;
            // cost and |g|max of the linearisation behind the previous iteration (trial_finish_kernel read them on the way)
            if (sv.pending.on && ba_take_pending(sv, 0.5 * ts[TS_LIN_COST2], ts[TS_LIN_GMAX])) {
                --sv.iter;           // converged at the previous iteration: this trial step is discarded
                stop(sv, STBA_CONVERGENCE, STBA_TERM_GRADIENT);
                break;
            }
            if (flag_h != 0 || (int)hd[DL_KASE] == DOGLEG_INVALID_GN) {
                // no Gauss-Newton step at this mu: the same linearisation again at 10 mu
                if (region.escalate()) { sv.need_build = need_gn = true; --sv.iter; continue; }
                have_gn = false;
            }
        }
        const TrialScalars t = have_gn ? trial_scalars(ts) : TrialScalars{sv.cost, 0.0, 0.0, 0.0};
        // a step without a Gauss-Newton step, or whose model change is not positive and finite, is invalid; a trial point whose cost
        // is not finite is rejected.  Neither is judged (row [cost, 0, ., 0, 0], no stop test).
        const bool valid = have_gn && t.model_change > 0.0 && std::isfinite(t.model_change);
        const bool step_ok = valid && std::isfinite(t.new_cost);
        if (have_gn) {
            const int kase = (int)hd[DL_KASE];
            if (kase >= 0 && kase < 3) ++ds.steps_by_case[kase];
            if (reused) ++ds.reused_steps;
        }
        const StepVerdict v = judge_step(opt, sv.cost, step_ok, t.new_cost, t.model_change, t.step_norm, t.x_norm, true);
        if (ba_apply_verdict(b, sv, v, step_ok, t, region.radius)) break;
        if (v.accepted) region.accept(v.rho, hd[DL_ZNORM], opt);
        else {
            ++s.num_unsuccessful_steps;
            if (!valid) { region.invalid(); ++ds.invalid_steps; sv.need_build = need_gn = true; }
            else region.reject();
        }
        invalid_in_a_row = valid ? 0 : invalid_in_a_row + 1;
        if (invalid_in_a_row >= kMaxConsecutiveInvalidSteps) {
            // Ceres' max_num_consecutive_invalid_steps (5): mu has only grown, and nothing lowers it but an accepted step
            stop(sv, STBA_FAILURE, STBA_TERM_SOLVER_FAIL);
            break;
        }
        if (v.accepted) {
            // a new linearisation: the next iteration builds and factors it at the new mu
            STBA_TRY(ba_linearize_point(b, b->cur, b->trial + TS_COST2));
            sv.need_build = need_gn = true;
            if (sv.deferred_ok) {
                sv.pending.on = true; sv.pending.accepted = true; sv.pending.iter = sv.iter;
            } else {
                STBA_TRY(ba_build_at(b, sv, 1.0 / region.mu));
                STBA_TRY(ba_read_linear_scalars(b, &sv.cost, &sv.gmax));
            }
        }
        if (ba_end_iteration(sv, v, t.step_norm, region.radius)) break;
    }
    // (a pending read behind the loop needs the reduced system of the last linearisation: the gradient comes with its build)
    if (sv.pending.on && sv.need_build) STBA_TRY(ba_build_at(b, sv, 1.0 / region.mu));
    STBA_TRY(ba_solve_end(b, sv, region.radius, sum));
    ds.final_mu = region.mu;
    b->dl_sum = ds;
    return STBA_OK;
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
        if (hipEventCreate(&e) != hipSuccess) return fail(STBA_ERR_HIP, "hipEventCreate");
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
    b->dup_overflow = P.dup_overflow;
    b->schur_mode = b->schur_mode_auto = P.schur_mode;
    b->have_pair_plan = P.have_pair_plan;
    b->lm_slices = P.lm_slices;
    b->n_tasks = P.n_tasks; b->max_cols = P.max_cols;
    b->schur_plan_mode = P.plan_mode;
    b->schur_pairs = (double)P.pairs; b->schur_lds_atomics = P.lds_atomics;
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
    for (int k = 0; k < 2; ++k) { STBA_TRY(b->cams[k].alloc(nc * 7)); STBA_TRY(b->pts[k].alloc(np * 3)); }
    STBA_TRY(b->feat.alloc(no)); STBA_TRY(b->obs_cam.alloc(no)); STBA_TRY(b->obs_pt.alloc(no));
    STBA_TRY(b->pt_start.alloc(np + 1)); STBA_TRY(b->cam_perm.alloc(no));
    STBA_TRY(b->chunk_begin.alloc((size_t)b->n_chunks)); STBA_TRY(b->chunk_end.alloc((size_t)b->n_chunks));
    STBA_TRY(b->cam_chunk_start.alloc(nc + 1));
    STBA_TRY(b->task_cam.alloc(P.task_cam.size())); STBA_TRY(b->cam_start.alloc(nc + 1));
    STBA_TRY(b->task_col_lo.alloc(P.task_cam.size())); STBA_TRY(b->task_col_hi.alloc(P.task_cam.size()));
    STBA_TRY(b->row_col_ptr.alloc(nc + 1)); STBA_TRY(b->row_cols.alloc(P.row_cols.size()));
    STBA_TRY(b->pair_begin.alloc(P.pair_begin.size())); STBA_TRY(b->pair_end.alloc(P.pair_end.size()));
    STBA_TRY(b->pair_rec.alloc(P.pairs));
    STBA_TRY(b->task_vs_ptr.alloc(P.task_vs_ptr.size())); STBA_TRY(b->vs_first.alloc(P.vs_first.size()));
    if (cam_fixed) STBA_TRY(b->cam_fixed.alloc(nc));
    if (pt_fixed) STBA_TRY(b->pt_fixed.alloc(np));
    if (b->lm_slices) {
        STBA_TRY(b->task_p_lo.alloc(P.task_p_lo.size())); STBA_TRY(b->task_p_hi.alloc(P.task_p_hi.size())); STBA_TRY(b->task_part_off.alloc(P.task_part_off.size()));
        STBA_TRY(b->row_task_ptr.alloc(P.row_task_ptr.size())); STBA_TRY(b->row_tasks.alloc(P.row_tasks.size()));
        STBA_TRY(b->schur_part.alloc(P.part_doubles));
        STBA_TRY(upload(b->task_p_lo, P.task_p_lo.data(), P.task_p_lo.size(), b->st)); STBA_TRY(upload(b->task_p_hi, P.task_p_hi.data(), P.task_p_hi.size(), b->st));
        STBA_TRY(upload(b->task_part_off, P.task_part_off.data(), P.task_part_off.size(), b->st));
        STBA_TRY(upload(b->row_task_ptr, P.row_task_ptr.data(), P.row_task_ptr.size(), b->st)); STBA_TRY(upload(b->row_tasks, P.row_tasks.data(), P.row_tasks.size(), b->st));
    }
    if (!P.dup_run.empty()) { STBA_TRY(b->dup_run.alloc(no)); STBA_TRY(upload(b->dup_run, P.dup_run.data(), no, b->st)); }
    STBA_TRY(b->r.alloc(no)); STBA_TRY(b->J8.alloc(no * 8));
    if (cam_fixed || pt_fixed) STBA_TRY(b->omask.alloc(no));
    STBA_TRY(b->Hpp6.alloc(np * 6)); STBA_TRY(b->gp.alloc(np * 3)); STBA_TRY(b->Hinv6.alloc(np * 6)); STBA_TRY(b->Rinv9.alloc(np * 9));
    STBA_TRY(b->dp.alloc(np * 3)); STBA_TRY(b->scale_p.alloc(np * 3));
    STBA_TRY(b->Hcc.alloc(nc * 36)); STBA_TRY(b->gc.alloc(nc * 6)); STBA_TRY(b->cam_partial.alloc((size_t)b->n_chunks * 28));
    STBA_TRY(b->dc.alloc(nc * 6)); STBA_TRY(b->scale_c.alloc(nc * 6));
    STBA_TRY(b->Sbuf.alloc(b->sbuf_count()));
    STBA_TRY(b->dxc.alloc((size_t)b->lda)); STBA_TRY(b->dxp.alloc(np * 3));
    STBA_TRY(b->cost_partial.alloc((size_t)b->lin_grid + 3));     // (+ 3: the pose priors' slot, the relative-pose factors' and the landmark priors', see n_cost)
    STBA_TRY(b->upd_partial_c.alloc((size_t)backsub_cam_grid(n_cams) * 4));    // (>= (n_cams + 255) / 256 blocks of 4)
    STBA_TRY(b->upd_partial_p.alloc((size_t)(point_blocks_grid(n_pts) + 1) * 4));    // (>= (n_pts + 255) / 256 + 1 blocks of 4)
    STBA_TRY(b->trial.alloc((size_t)TS_BLOCK)); STBA_TRY(b->flag.alloc(1));
    if (iterative) STBA_TRY(ba_pcg_alloc(b));

    tmark("device allocations");
    STBA_TRY(upload(b->cams[0], cams, nc * 7, b->st)); STBA_TRY(upload(b->pts[0], pts, np * 3, b->st));
    STBA_TRY(upload(reinterpret_cast<double*>(b->feat.get()), P.s_feat.data(), no * 2, b->st));
    STBA_TRY(upload(b->obs_cam, P.s_cam.data(), no, b->st)); STBA_TRY(upload(b->obs_pt, P.s_pt.data(), no, b->st));
    STBA_TRY(upload(b->pt_start, P.pt_start.data(), np + 1, b->st)); STBA_TRY(upload(b->cam_perm, P.cam_perm.data(), no, b->st));
    STBA_TRY(upload(b->chunk_begin, P.chunk_begin.data(), (size_t)b->n_chunks, b->st));
    STBA_TRY(upload(b->chunk_end, P.chunk_end.data(), (size_t)b->n_chunks, b->st));
    STBA_TRY(upload(b->cam_chunk_start, P.cam_chunk_start.data(), nc + 1, b->st));
    STBA_TRY(upload(b->task_cam, P.task_cam.data(), P.task_cam.size(), b->st));
    STBA_TRY(upload(b->cam_start, P.cam_start.data(), nc + 1, b->st));
    STBA_TRY(upload(b->task_col_lo, P.task_col_lo.data(), P.task_cam.size(), b->st));
    STBA_TRY(upload(b->task_col_hi, P.task_col_hi.data(), P.task_cam.size(), b->st));
    b->h_row_col_ptr = P.row_col_ptr; b->h_row_cols = P.row_cols;
    STBA_TRY(upload(b->row_col_ptr, P.row_col_ptr.data(), nc + 1, b->st));
    if (!P.row_cols.empty()) STBA_TRY(upload(b->row_cols, P.row_cols.data(), P.row_cols.size(), b->st));
    STBA_TRY(upload(b->pair_begin, P.pair_begin.data(), P.pair_begin.size(), b->st)); STBA_TRY(upload(b->pair_end, P.pair_end.data(), P.pair_end.size(), b->st));
    if (P.pairs > 0) STBA_TRY(upload(b->pair_rec, reinterpret_cast<const int4*>(P.pair_rec.get()), P.pairs, b->st));
    STBA_TRY(upload(b->task_vs_ptr, P.task_vs_ptr.data(), P.task_vs_ptr.size(), b->st)); STBA_TRY(upload(b->vs_first, P.vs_first.data(), P.vs_first.size(), b->st));
    if (cam_fixed) STBA_TRY(upload(b->cam_fixed, cmask.data(), nc, b->st));
    std::vector<unsigned char>& omask = b->create_omask;
    if (b->omask) {
        omask.resize(no);
        for (size_t p2 = 0; p2 < no; ++p2)
            omask[p2] = (unsigned char)((cam_fixed ? cmask[(size_t)P.s_cam[p2]] : 0u) | ((pt_fixed && pt_fixed[(size_t)P.s_pt[p2]]) ? 64u : 0u));
        STBA_TRY(upload(b->omask, omask.data(), no, b->st));
    }
    if (pt_fixed) STBA_TRY(upload(b->pt_fixed, pt_fixed, np, b->st));
    if (hipMemsetAsync(b->dxc, 0, (size_t)b->lda * sizeof(double), b->st) != hipSuccess ||
        hipMemsetAsync(b->Sbuf, 0, b->sbuf_count() * sizeof(double), b->st) != hipSuccess ||
        hipStreamSynchronize(b->st) != hipSuccess)
        return fail(STBA_ERR_HIP, "stba_ba_create: initial memset/sync failed");
    tmark("uploads + sync");
    // The plan's host-side temporaries -- 16 bytes per pair, the regrouped observations: ~110 MB at C5 -- cost 11 of the 43 ms of this
    // function just to FREE (measured: STBA_CREATE_TIMING in a debug build).  The engine keeps them and frees them when it is destroyed:
    // the caller gets its engine that much sooner, and the operator API destroys its engine on a helper thread next to its end-point
    // check anyway.  (Freed by a thread of their own right here: 10 ms off this function as well, but 2 ms ON a drop-in Solve() -- the
    // munmap of 110 MB holds the process's address-space lock while the calling thread faults pages in.)
    b->perm = std::move(plan->perm);
    b->create_leftovers = std::move(plan);
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

// what an ITERATIVE_SCHUR engine refuses for want of the explicit reduced system: the stage and measurement entry points and the
// covariance (the features it does not go together with are rows of ba_features.hpp)
static int refuse_iterative(const stba_ba* b, const char* who, const char* why) {
    if (!b || !b->iterative) return STBA_OK;
    return fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": this engine uses ITERATIVE_SCHUR, " + why);
}

int stba_ba_set_pcg(stba_ba* b, int preconditioner, double eta, int min_iterations, int max_iterations, int check_every) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (!b->iterative) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_pcg: the engine uses the dense Schur solver (stba_ba_create_ex)");
    if (preconditioner < STBA_PRECOND_IDENTITY || preconditioner > STBA_PRECOND_SCHUR_JACOBI || !(eta >= 0.0) || min_iterations < 0 ||
        max_iterations < 1 || min_iterations > max_iterations || check_every < 1)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_pcg: bad argument");
    b->pcg_precond = preconditioner; b->pcg_eta = eta; b->pcg_min = min_iterations; b->pcg_max = max_iterations; b->pcg_check = check_every;
    return STBA_OK;
}

int stba_ba_last_pcg_summary(stba_ba* b, stba_pcg_summary* out) {
    if (!b || !out) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    *out = b->pcg_sum;
    return STBA_OK;
}

int stba_ba_last_pcg_iterations(stba_ba* b, int* per_iteration, int n) {
    if (!b || n < 0 || (n > 0 && !per_iteration)) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_last_pcg_iterations: bad argument");
    for (int k = 0; k < n; ++k) per_iteration[k] = (size_t)k < b->pcg_per_iter.size() ? b->pcg_per_iter[(size_t)k] : 0;
    return STBA_OK;
}

int stba_ba_time_schur_apply(stba_ba* b, int reps, double* ms_avg) {
    if (!b || reps <= 0 || !ms_avg) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_time_schur_apply: bad argument");
    if (!b->iterative) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_time_schur_apply: the engine uses the dense Schur solver");
    if (!b->have_blocks) return fail(STBA_ERR_STATE, "stba_ba_time_schur_apply needs stba_ba_schur_apply first");
    const PcgVecs v = pcg_vecs(b);
    STBA_HIP(hipEventRecord(b->ev[EV_LIN], b->st));
    for (int k = 0; k < reps; ++k) {
        STBA_TRY(ba_is_landmark_pass(b, v.p, nullptr, nullptr));
        STBA_TRY(ba_is_camera_pass(b, IS_FINAL_APPLY, v.p, v.q, nullptr, nullptr));
    }
    STBA_HIP(hipEventRecord(b->ev[EV_LIN_END], b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    float ms = 0.f;
    STBA_HIP(hipEventElapsedTime(&ms, b->ev[EV_LIN], b->ev[EV_LIN_END]));
    *ms_avg = (double)ms / reps;
    return STBA_OK;
}

int stba_ba_schur_apply(stba_ba* b, const double* dc, const double* dp, int which, const double* x, double* y) {
    if (!b || !dc || !dp || !y || which < 0 || which > 2) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_schur_apply: bad argument");
    if (!b->iterative) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_schur_apply: the engine uses the dense Schur solver (stba_ba_reduced_system)");
    if (!b->have_blocks) return fail(STBA_ERR_STATE, "stba_ba_schur_apply needs stba_ba_normal_blocks first");
    STBA_TRY(upload(b->dc, dc, (size_t)b->n, b->st));
    STBA_TRY(upload(b->dp, dp, (size_t)b->np * 3, b->st));
    Damping dm;
    dm.explicit_d = true;
    STBA_TRY(launch_point_invert(b->np, b->Hpp6, b->dp, b->pt_fixed, b->Hinv6, nullptr, b->st));
    STBA_TRY(ba_camera_blocks(b));
    double* out_dev = b->rhs();
    if (!x) STBA_TRY(ba_is_rhs(b));
    else {
        const PcgVecs v = pcg_vecs(b);
        STBA_TRY(upload(which == 0 ? v.p : v.r, x, (size_t)b->n, b->st));
        if (which == 0) {
            STBA_TRY(ba_is_landmark_pass(b, v.p, nullptr, nullptr));
            STBA_TRY(ba_is_camera_pass(b, IS_FINAL_APPLY, v.p, v.q, nullptr, nullptr));
            out_dev = v.q;
        } else {
            STBA_TRY(ba_is_precond(b, which == 1 ? STBA_PRECOND_JACOBI : STBA_PRECOND_SCHUR_JACOBI));
            STBA_TRY(launch_is_vec(b->nc, IS_VEC_PRECOND, v, b->st));
            out_dev = v.z;
        }
    }
    STBA_TRY(download(y, out_dev, (size_t)b->n, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    b->have_reduced = b->have_dxc = b->have_dxp = false;
    return STBA_OK;
}

int stba_ba_set_schur_mode(stba_ba* ba, int mode) {
    STBA_TRY(refuse_iterative(ba, "stba_ba_set_schur_mode", "which forms no Schur complement"));
    if (!ba || mode < STBA_SCHUR_AUTO || mode > STBA_SCHUR_DENSE) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_schur_mode: bad argument");
    if (mode == STBA_SCHUR_AUTO) mode = ba->schur_mode_auto;
    if (mode == STBA_SCHUR_PAIRS && !ba->have_pair_plan)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_schur_mode: this engine was created without a pair plan (too many observation pairs)");
    if (mode == STBA_SCHUR_DENSE && ba->dup_overflow)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_schur_mode: more than 255 observations of one (camera, landmark) pair: the dense form cannot take this problem");
    if (mode == STBA_SCHUR_DENSE) STBA_TRY(ba_dense_alloc(ba));
    ba->schur_mode = mode;
    ba->have_reduced = ba->have_dxc = ba->have_dxp = false;
    return STBA_OK;
}
int stba_ba_schur_mode(const stba_ba* ba, int* mode) {
    if (!ba || !mode) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_schur_mode: bad argument");
    *mode = ba->schur_mode;
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
    b->ar = fn; b->ar_user = user; b->rank = rank; b->world = world_size;
    // what travels is decided again with the new group (the union pattern belongs to the group)
    b->pk_state = 0; b->pk_nz = 0;
    b->pk_blocks.reset();
    b->Spack.reset();
    return STBA_OK;
}

int stba_ba_reduced_dim(const stba_ba* b, int* n, int* n_padded) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (n) *n = b->n;
    if (n_padded) *n_padded = b->lda;
    return STBA_OK;
}

int stba_ba_evaluate(stba_ba* b, double* cost, double* r, double* Jc, double* Jp) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    STBA_TRY(ba_linearize(b, b->cur, b->trial + TS_COST2));
    double c2 = 0.0;
    STBA_TRY(download(&c2, b->trial + TS_COST2, 1, b->st));
    const size_t no = (size_t)b->no;
    std::vector<double> tr, tjc, tjp;
    if (r) { tr.resize(no * 2); STBA_TRY(download(tr.data(), reinterpret_cast<double*>(b->r.get()), no * 2, b->st)); }
    DevBuf<double> djc, djp;     // the device holds the compact Jacobian; the 2x6 | 2x3 form is expanded for the caller
    if ((Jc || Jp) && b->hl_fn) return fail(STBA_ERR_STATE, "stba_ba_evaluate: with a host lineariser the Jacobians are the caller's own");
    if (Jc || Jp) {
        if (Jc) STBA_TRY(djc.alloc(no * 12));
        if (Jp) STBA_TRY(djp.alloc(no * 6));
        STBA_TRY(launch_expand_jacobian(b->no, b->J8, b->omask, djc, djp, b->st, ba_general_jc(b)));
        if (Jc) { tjc.resize(no * 12); STBA_TRY(download(tjc.data(), djc, no * 12, b->st)); }
        if (Jp) { tjp.resize(no * 6); STBA_TRY(download(tjp.data(), djp, no * 6, b->st)); }
    }
    STBA_HIP(hipStreamSynchronize(b->st));
    for (size_t p = 0; p < no; ++p) {   // back to the caller's observation order
        const size_t i = (size_t)b->perm[p];
        if (r) memcpy(r + i * 2, tr.data() + p * 2, 2 * sizeof(double));
        if (Jc) memcpy(Jc + i * 12, tjc.data() + p * 12, 12 * sizeof(double));
        if (Jp) memcpy(Jp + i * 6, tjp.data() + p * 6, 6 * sizeof(double));
    }
    if (cost) *cost = 0.5 * c2;
    b->have_lin = true;
    b->have_blocks = b->have_reduced = b->have_dxc = b->have_dxp = false;
    return STBA_OK;
}

int stba_ba_cost(stba_ba* b, double* cost) {
    if (!b || !cost) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    STBA_TRY(ba_cost_only(b, b->cur, b->trial + TS_COST2));
    double c2 = 0.0;
    STBA_TRY(download(&c2, b->trial + TS_COST2, 1, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    *cost = 0.5 * c2;
    return STBA_OK;
}

int stba_ba_normal_blocks(stba_ba* b, double* Hcc, double* gc, double* Hpp, double* gp) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (!b->have_lin) return fail(STBA_ERR_STATE, "stba_ba_normal_blocks needs stba_ba_evaluate first");
    STBA_TRY(ba_normal_blocks(b));
    STBA_TRY(ba_camera_blocks(b));
    STBA_TRY(ba_prior_blocks(b));
    STBA_TRY(ba_between_blocks(b, false));
    std::vector<double> h6;
    if (Hcc) STBA_TRY(download(Hcc, b->Hcc, (size_t)b->nc * 36, b->st));
    if (gc) STBA_TRY(download(gc, b->gc, (size_t)b->nc * 6, b->st));
    if (Hpp) { h6.resize((size_t)b->np * 6); STBA_TRY(download(h6.data(), b->Hpp6, h6.size(), b->st)); }
    if (gp) STBA_TRY(download(gp, b->gp, (size_t)b->np * 3, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    if (Hpp)
        for (size_t j = 0; j < (size_t)b->np; ++j) {
            const double* s = h6.data() + j * 6;
            double* d = Hpp + j * 9;
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[1]; d[4] = s[3]; d[5] = s[4]; d[6] = s[2]; d[7] = s[4]; d[8] = s[5];
        }
    b->have_blocks = true;
    return STBA_OK;
}

int stba_ba_reduced_system(stba_ba* b, const double* dc, const double* dp, double* S, double* rhs) {
    STBA_TRY(refuse_iterative(b, "stba_ba_reduced_system", "which never forms the reduced system (stba_ba_schur_apply applies it)"));
    if (!b || !dc || !dp) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    if (!b->have_blocks) return fail(STBA_ERR_STATE, "stba_ba_reduced_system needs stba_ba_normal_blocks first");
    STBA_TRY(upload(b->dc, dc, (size_t)b->n, b->st));
    STBA_TRY(upload(b->dp, dp, (size_t)b->np * 3, b->st));
    Damping dm;
    dm.explicit_d = true;
    STBA_HIP(hipMemsetAsync(b->ex_scalar(), 0, (size_t)b->lda * sizeof(double), b->st));
    STBA_TRY(ba_build_reduced(b, dm));
    if (S) STBA_HIP(hipMemcpy2DAsync(S, (size_t)b->n * sizeof(double), b->S(), (size_t)b->lda * sizeof(double),
                                     (size_t)b->n * sizeof(double), (size_t)b->n, hipMemcpyDeviceToHost, b->st));
    if (rhs) STBA_TRY(download(rhs, b->rhs(), (size_t)b->n, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    b->have_reduced = true;
    b->have_dxc = b->have_dxp = false;
    return STBA_OK;
}

int stba_ba_solve_reduced(stba_ba* b, double* dxc) {
    STBA_TRY(refuse_iterative(b, "stba_ba_solve_reduced", "which has no reduced system to factor"));
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (!b->have_reduced) return fail(STBA_ERR_STATE, "stba_ba_solve_reduced needs stba_ba_reduced_system first");
    STBA_TRY(chol_factor_solve_dev(b->S(), b->lda, b->n, b->dxc, b->flag, b->st));
    int flag_h = 0;
    STBA_TRY(download(&flag_h, b->flag, 1, b->st));
    if (dxc) STBA_TRY(download(dxc, b->dxc, (size_t)b->n, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    b->have_reduced = false;   // S now holds the factor
    if (flag_h == CHOL_FLAG_TIMEOUT && !b->ar && b->have_blocks) {
        // the persistent factorisation gave up (shared device): start the cool-down, rebuild S from the blocks with the damping
        // the caller gave (it is still on the device) and factor through the stage kernels, as the LM loop does.  (Several ranks:
        // the rebuild is a collective and this is a rank-local decision -- the error below stands.)
        chol_note_timeout();
        Damping dm;
        dm.explicit_d = true;
        STBA_HIP(hipMemsetAsync(b->ex_scalar(), 0, (size_t)b->lda * sizeof(double), b->st));
        STBA_TRY(ba_build_reduced(b, dm));
        STBA_TRY(chol_factor_solve_stages(b->S(), b->lda, b->n, b->dxc, b->flag, b->st));
        STBA_TRY(download(&flag_h, b->flag, 1, b->st));
        if (dxc) STBA_TRY(download(dxc, b->dxc, (size_t)b->n, b->st));
        STBA_HIP(hipStreamSynchronize(b->st));
    }
    STBA_TRY(chol_flag_status(flag_h));
    if (flag_h != 0) return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, "reduced camera system: pivot " + std::to_string(flag_h));
    b->have_dxc = true;
    return STBA_OK;
}

int stba_ba_back_substitute(stba_ba* b, double* dxp) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (!b->have_dxc) return fail(STBA_ERR_STATE, "stba_ba_back_substitute needs stba_ba_solve_reduced first");
    STBA_TRY(launch_backsub(b->np, b->pt_start, b->obs_cam, b->J8, b->omask, b->Hinv6, b->gp, b->dxc, b->dxp, b->st, nullptr, ba_general_jc(b)));
    if (dxp) STBA_TRY(download(dxp, b->dxp, (size_t)b->np * 3, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    b->have_dxp = true;
    return STBA_OK;
}

int stba_ba_apply_step(stba_ba* b, int accept, double* new_cost) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (!b->have_dxp) return fail(STBA_ERR_STATE, "stba_ba_apply_step needs stba_ba_back_substitute first");
    STBA_TRY(ba_trial(b, nullptr));
    double ts[TS_COUNT];
    STBA_TRY(download(ts, b->trial, TS_COUNT, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    if (new_cost) *new_cost = 0.5 * ts[TS_COST2];
    if (accept) {
        b->cur ^= 1;
        ba_invalidate(b);
    }
    return STBA_OK;
}

int stba_ba_solve(stba_ba* b, const stba_lm_options* opt, stba_lm_summary* summary, double* trace,
                  stba_iteration_callback cb, void* cb_user) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    b->dl_sum = stba_dogleg_summary{};
    STBA_TRY(ba_refuse(b, "stba_ba_solve"));
    if (b->trust_region == STBA_TR_TRADITIONAL_DOGLEG) return ba_run_dogleg(b, opt, summary, trace, cb, cb_user);
    return ba_run_lm(b, opt, 0, summary, trace, cb, cb_user);
}

int stba_ba_set_trust_region(stba_ba* b, int strategy) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (strategy != STBA_TR_LEVENBERG_MARQUARDT && strategy != STBA_TR_TRADITIONAL_DOGLEG)
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_set_trust_region: unknown strategy " + std::to_string(strategy));
    STBA_TRY(ba_refuse(b, "stba_ba_set_trust_region", strategy == STBA_TR_TRADITIONAL_DOGLEG));
    b->trust_region = strategy;
    return STBA_OK;
}

int stba_ba_last_dogleg_summary(stba_ba* b, stba_dogleg_summary* out) {
    if (!b || !out) return fail(STBA_ERR_INVALID_ARGUMENT, "null argument");
    const size_t want = out->struct_size;
    if (want < offsetof(stba_dogleg_summary, factorizations) + sizeof(int))
        return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_last_dogleg_summary: out->struct_size is smaller than any version of the struct");
    stba_dogleg_summary s = b->dl_sum;
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

int stba_ba_inner_sweep(stba_ba* b, double* cost_before, double* cost_after, int* iterations_per_block) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    STBA_TRY(ba_refuse(b, "stba_ba_inner_sweep"));
    const bool was_on = b->inner.on;
    if (!b->inner.sc) STBA_TRY(stba_ba_set_inner_iterations(b, 1, b->inner.tol, nullptr, nullptr, nullptr));   // (never set: the default ordering)
    STBA_TRY(ba_cost_only(b, b->cur, b->inner.sc + 2));
    STBA_TRY(ba_inner_sweep_enqueue(b, b->cur, nullptr));
    STBA_TRY(ba_cost_only(b, b->cur, b->inner.sc));
    double sc[3];
    STBA_TRY(download(sc, b->inner.sc, 3, b->st));
    const size_t ncl = b->inner.plan.cam.size(), npl = b->inner.plan.pt.size();
    std::vector<int> it(ncl + npl);
    if (!it.empty()) STBA_TRY(download(it.data(), b->inner.it, it.size(), b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    ba_invalidate(b);
    inner_summary_reset(b);
    b->inner.sum.sweeps = 1;
    b->inner.on = was_on;
    if (cost_before) *cost_before = 0.5 * sc[2];
    if (cost_after) *cost_after = 0.5 * sc[0];
    if (iterations_per_block) {
        const int nc = b->nc;
        memset(iterations_per_block, 0, sizeof(int) * ((size_t)2 * nc + b->np));
        for (size_t k = 0; k < ncl; ++k) {
            const int c = b->inner.plan.cam[k];
            if (b->inner.plan.kind[k] & 1u) iterations_per_block[c] = it[k];
            if (b->inner.plan.kind[k] & 2u) iterations_per_block[nc + c] = it[k];
        }
        for (size_t k = 0; k < npl; ++k) iterations_per_block[2 * nc + b->inner.plan.pt[k]] = it[ncl + k];
    }
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

int stba_ba_lm_iterations(stba_ba* b, const stba_lm_options* opt, int iterations, stba_lm_summary* summary,
                          double* trace) {
    if (!b || iterations <= 0) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    return ba_run_lm(b, opt, iterations, summary, trace, nullptr, nullptr);
}

int stba_ba_triangulate(stba_ba* b, int max_iter) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    STBA_TRY(launch_triangulate(b->np, b->pt_start, b->obs_cam, b->feat, b->cams[b->cur], b->pts[b->cur], b->pt_fixed,
                                max_iter, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    ba_invalidate(b);
    return STBA_OK;
}

int stba_ba_time_linearize(stba_ba* b, int reps, double* ms_avg) {
    if (!b || reps <= 0 || !ms_avg) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    STBA_TRY(ba_linearize_dispatch(b, b->cur, true));   // warm
    STBA_HIP(hipEventRecord(b->ev[EV_LIN], b->st));
    for (int k = 0; k < reps; ++k) STBA_TRY(ba_linearize_dispatch(b, b->cur, true));
    STBA_HIP(hipEventRecord(b->ev[EV_LIN_END], b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    float ms = 0.f;
    STBA_HIP(hipEventElapsedTime(&ms, b->ev[EV_LIN], b->ev[EV_LIN_END]));
    *ms_avg = (double)ms / reps;
    ba_invalidate(b);
    return STBA_OK;
}

// measurement (bench.py roofline_schur): average device time of the Schur-complement kernel at the current point -- a fresh
// linearisation and landmark blocks first, then `reps` reduced-system builds timed around the kernel alone
int stba_ba_time_schur(stba_ba* b, int reps, double* ms_avg, double* lds_atomics_per_launch, double* pairs_per_launch) {
    STBA_TRY(refuse_iterative(b, "stba_ba_time_schur", "which has no Schur complement kernel"));
    if (!b || reps <= 0 || !ms_avg) return fail(STBA_ERR_INVALID_ARGUMENT, "bad argument");
    STBA_TRY(ba_linearize_lm(b, b->cur));
    STBA_TRY(ba_normal_blocks(b));
    STBA_TRY(ba_fill_scalar_slots(b, b->trial + TS_COST2));
    Damping dm;
    STBA_TRY(launch_point_damp_invert(b->np, b->Hpp6, b->pt_fixed, b->scale_p, b->scale_init ? 0 : 1, dm.use_scaling, dm.radius, dm.dmin,
                                      dm.dmax, b->dp, b->Hinv6, ba_rinv(b), b->Sbuf + (size_t)b->lda * b->lda, 3 * b->lda, b->st));
    STBA_TRY(ba_schur_step(b));      // warm
    STBA_HIP(hipEventRecord(b->ev[EV_LIN], b->st));
    for (int k = 0; k < reps; ++k) STBA_TRY(ba_schur_step(b));
    STBA_HIP(hipEventRecord(b->ev[EV_LIN_END], b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    float ms = 0.f;
    STBA_HIP(hipEventElapsedTime(&ms, b->ev[EV_LIN], b->ev[EV_LIN_END]));
    *ms_avg = (double)ms / reps;
    if (lds_atomics_per_launch) *lds_atomics_per_launch = b->schur_lds_atomics;
    if (pairs_per_launch) *pairs_per_launch = b->schur_pairs;
    ba_invalidate(b);
    return STBA_OK;
}

int stba_ba_covariance_compute(stba_ba* b, double min_rcond, double* rcond_out) {
    STBA_TRY(refuse_iterative(b, "stba_ba_covariance_compute", "and the covariance needs the explicit reduced system S"));
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (b->ar) return fail(STBA_ERR_STATE, "stba_ba_covariance_compute: the engine holds one landmark shard of several ranks; covariance needs one rank");
    ba_drop_covariance(b);
    STBA_TRY(ba_cov_build(b));
    BaCovInputs in;
    in.nc = b->nc; in.np = b->np; in.no = b->no; in.n = b->n; in.lda = b->lda; in.st = b->st;
    in.pt_start = b->pt_start; in.obs_cam = b->obs_cam; in.J8 = b->J8; in.Jc12 = ba_general_jc(b);
    in.omask = b->omask; in.cam_fixed = b->cam_fixed; in.pt_fixed = b->pt_fixed;
    in.Hpp6 = b->Hpp6; in.Hinv6 = b->Hinv6; in.S = b->S();
    return cov_compute(in, min_rcond, &b->cov, rcond_out);
}

int stba_ba_camera_covariance(stba_ba* b, int n_pairs, const int* cam_a, const int* cam_b, double* out) {
    if (!b || n_pairs < 0 || (n_pairs > 0 && (!cam_a || !cam_b || !out))) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_camera_covariance: bad argument");
    if (!b->cov) return fail(STBA_ERR_STATE, "stba_ba_camera_covariance needs stba_ba_covariance_compute first");
    return cov_camera_blocks(b->cov, n_pairs, cam_a, cam_b, out);
}

int stba_ba_point_covariance(stba_ba* b, int n, const int* pts, double* out) {
    if (!b || n < 0 || (n > 0 && !out)) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_point_covariance: bad argument");
    if (!b->cov) return fail(STBA_ERR_STATE, "stba_ba_point_covariance needs stba_ba_covariance_compute first");
    return cov_point_blocks(b->cov, n, pts, out);
}

int stba_ba_camera_point_covariance(stba_ba* b, int n_pairs, const int* cam, const int* pt, double* out) {
    if (!b || n_pairs < 0 || (n_pairs > 0 && (!cam || !pt || !out))) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_camera_point_covariance: bad argument");
    if (!b->cov) return fail(STBA_ERR_STATE, "stba_ba_camera_point_covariance needs stba_ba_covariance_compute first");
    return cov_cam_point_blocks(b->cov, n_pairs, cam, pt, out);
}

int stba_ba_point_pair_covariance(stba_ba* b, int n_pairs, const int* pt_a, const int* pt_b, double* out) {
    if (!b || n_pairs < 0 || (n_pairs > 0 && (!pt_a || !pt_b || !out))) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_point_pair_covariance: bad argument");
    if (!b->cov) return fail(STBA_ERR_STATE, "stba_ba_point_pair_covariance needs stba_ba_covariance_compute first");
    return cov_point_pair_blocks(b->cov, n_pairs, pt_a, pt_b, out);
}

int stba_ba_covariance_release(stba_ba* b) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    ba_drop_covariance(b);
    return STBA_OK;
}

}  // extern "C"
