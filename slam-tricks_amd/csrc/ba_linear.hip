// ba_linear.hip -- the linear algebra of one iteration of the bundle adjustment, host side: the linearisation dispatch (host
// callback, robust or lossless kernel, the factor kinds' cost forms), the landmark and camera blocks, the damped reduced system in
// its explicit form (pair plan or dense product; the cross-rank sum is ba_allreduce.hip) and its implicit form with the PCG that
// solves it (ITERATIVE_SCHUR), the back-substitution and the trial point, and the undamped build of the covariance.
// Every function enqueues on the engine's stream; the loops that order them are ba_solve.hip, the stage entry points ba_stages.hip.
#include <algorithm>
#include <vector>

#include "ba_engine.hpp"

namespace stba {

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
    b->hl.cams.resize((size_t)b->nc * 7); b->hl.pts.resize((size_t)b->np * 3); b->hl.r.resize(no * 2);
    if (with_jac) { b->hl.jc.resize(no * 12); b->hl.jp.resize(no * 6); }
    STBA_TRY(download(b->hl.cams.data(), b->cams[which], b->hl.cams.size(), b->st));
    STBA_TRY(download(b->hl.pts.data(), b->pts[which], b->hl.pts.size(), b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    if (b->hl.fn(b->hl.user, b->hl.cams.data(), b->hl.pts.data(), b->hl.r.data(), with_jac ? b->hl.jc.data() : nullptr,
                 with_jac ? b->hl.jp.data() : nullptr) != 0)
        return fail(STBA_ERR_CALLBACK, "host lineariser failed (a cost function returned false)");
    double c2 = 0.0;
    for (size_t k = 0; k < no * 2; ++k) c2 += b->hl.r[k] * b->hl.r[k];
    if (!std::isfinite(c2)) return fail(STBA_ERR_CALLBACK, "host lineariser: non-finite residual");
    // (the cost partials have a staging buffer of their own: the copy is asynchronous, and the big staging buffer below is
    // resized and overwritten right behind it -- in the cost-only call nothing waits for it before the next call refills it)
    b->hl.cost_stage.assign((size_t)b->lin_grid, 0.0);
    b->hl.cost_stage[0] = c2;
    STBA_TRY(upload(b->cost_partial, b->hl.cost_stage.data(), b->hl.cost_stage.size(), b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    std::vector<double>& st = b->hl.stage;
    if (with_jac) {
        st.resize(no * 12);
        for (size_t p = 0; p < no; ++p) { const size_t i = (size_t)b->perm[p]; memcpy(&st[p * 2], &b->hl.r[i * 2], 2 * sizeof(double)); }
        STBA_TRY(upload(reinterpret_cast<double*>(b->r.get()), st.data(), no * 2, b->st));
        STBA_HIP(hipStreamSynchronize(b->st));              // (the staging buffer is reused)
        for (size_t p = 0; p < no; ++p) {
            const size_t i = (size_t)b->perm[p];
            st[p * 8] = 0.0; st[p * 8 + 1] = 0.0;
            memcpy(&st[p * 8 + 2], &b->hl.jp[i * 6], 6 * sizeof(double));
        }
        STBA_TRY(upload(b->J8, st.data(), no * 8, b->st));
        STBA_HIP(hipStreamSynchronize(b->st));
        for (size_t p = 0; p < no; ++p) memcpy(&st[p * 12], &b->hl.jc[(size_t)b->perm[p] * 12], 12 * sizeof(double));
        STBA_TRY(upload(b->Jc12, st.data(), no * 12, b->st));
        STBA_HIP(hipStreamSynchronize(b->st));
    }
    return STBA_OK;
}

// THE linearisation at parameter buffer `which`: the host's callback, the robust kernel (a loss table and / or weights are set: its
// INFO / LOSS pair follows from which of the two the engine holds) or the lossless kernel.  The cost partials (sum r^2, or sum rho with a table) are left in cost_partial; with_jac: r, J8 (and Jc12) are stored
int ba_linearize_dispatch(stba_ba* b, int which, bool with_jac) {
    if (b->hl.fn) return ba_host_linearize(b, which, with_jac);
    const LinArgs a = lin_args(b, which, with_jac);
    if (with_jac) b->lin_which = which;
    if (b->loss.kind || b->winfo)
        STBA_TRY(launch_linearize_robust(a, LinLoss{b->loss.kind, b->loss.a, b->loss.b, b->loss.scale, b->Jc12, b->winfo}, with_jac, b->lin_grid, b->st));
    else
        STBA_TRY(launch_linearize(a, with_jac, b->lin_grid, b->st));
    // the factor kinds' costs at the same parameters, each into its slot behind the lineariser's partials (CostSlots; one launch each)
    const CostSlots slots = b->cost_slots();
    if (b->prior.n) STBA_TRY(launch_prior_cost(b->prior_args(), b->cams[which], slots.pose_priors(), b->st));
    if (b->btw.n) STBA_TRY(launch_between_cost(b->between_args(), b->cams[which], slots.relative_poses(), b->st));
    if (b->lprior.n) STBA_TRY(launch_landmark_prior_cost(b->landmark_prior_args(), b->pts[which], b->lprior.cost_part, slots.landmark_priors(), b->st));
    return STBA_OK;
}

// pose priors: sum J'^T J' into Hcc and sum J'^T r' into gc, at the parameters the Jacobian records were made at (one launch; none
// without priors).  Behind whatever has just WRITTEN the camera blocks: the Schur step or the camera-block kernel
int ba_prior_blocks(stba_ba* b) {
    if (!b->prior.n) return STBA_OK;
    return launch_prior_blocks(b->prior_args(), b->cams[b->lin_which], b->Hcc, b->gc, nullptr, nullptr, b->st);
}

// relative-pose factors: sum J_x'^T J_x' into Hcc, sum J_x'^T r' into gc and -- with_S -- sum J_hi'^T J_lo' onto the block (hi, lo) of S,
// which the Schur step has just zeroed and written (every build: nothing accumulates from one build to the next).  One launch; none
// without edges
int ba_between_blocks(stba_ba* b, bool with_S) {
    if (!b->btw.n) return STBA_OK;
    return launch_between_blocks(b->between_args(), b->cams[b->lin_which], b->Hcc, b->gc, with_S ? b->S() : nullptr, b->lda, nullptr, nullptr,
                                 nullptr, b->st);
}

// residuals + Jacobians at parameter buffer `which`; sum r^2 -> *cost2_dev
int ba_linearize(stba_ba* b, int which, double* cost2_dev) {
    STBA_TRY(ba_linearize_dispatch(b, which, true));
    return launch_sum_partials(b->cost_partial, b->n_cost(), 1, 1, cost2_dev, b->st);
}

// residual-only kernel (nothing stored): sum r^2 -> *cost2_dev
int ba_cost_only(stba_ba* b, int which, double* cost2_dev) {
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
int ba_normal_blocks(stba_ba* b) {
    STBA_TRY(launch_point_blocks(b->np, b->pt_start, b->J8, b->omask, b->r, b->Hpp6, b->gp, b->upd_partial_p, b->st));
    if (!b->lprior.n) return STBA_OK;
    return launch_landmark_prior_blocks(b->landmark_prior_args(), b->pts[b->lin_which], b->Hpp6, b->gp, b->upd_partial_p, nullptr, nullptr, b->st);
}
// residuals + Jacobians of the LM loop: the cost partial sums stay in cost_partial and are added up by
// ba_fill_scalar_slots behind the landmark blocks (one launch less than ba_linearize)
int ba_linearize_lm(stba_ba* b, int which) {
    return ba_linearize_dispatch(b, which, true);
}
int ba_camera_blocks(stba_ba* b) {
    return launch_camera_blocks(b->nc, b->n_chunks, b->chunk_begin, b->chunk_end, b->cam_chunk_start, b->cam_perm,
                                b->J8, b->omask, ba_general_jc(b), b->r, b->cam_partial, b->Hcc, b->gc, b->st);
}

// Y for the dense form of the Schur complement: [lda][ldy] doubles, zeroed once (the visibility pattern is static)
int ba_dense_alloc(stba_ba* b) {
    if (b->schur.Y) return STBA_OK;
    const size_t kcols = ((size_t)3 * b->np + 15) / 16 * 16;
    const size_t ldy = kcols + ((kcols % 512 == 0) ? 16 : 0);          // (not a multiple of 4 KB: rows would alias in the memory channels)
    const size_t ycount = (size_t)b->lda * ldy;
    const size_t wcount = chol_yyt_workspace_doubles(b->lda, kcols);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (ycount + wcount + kcols) * sizeof(double) > free_b / 10 * 9)
        return fail(STBA_ERR_INVALID_ARGUMENT, "the dense form of the Schur complement needs " + std::to_string((ycount + wcount) * 8 / (1 << 20)) +
                    " MiB (6 cameras x 3 landmarks doubles, padded), more than the device has free");
    STBA_TRY(b->schur.Y.alloc(ycount));
    STBA_TRY(b->schur.yv.alloc(schur_dense_partial_doubles(b->n_chunks)));      // (the chunk partials of the camera sums)
    if (wcount) STBA_TRY(b->schur.yws.alloc(wcount));
    STBA_HIP(hipMemsetAsync(b->schur.Y, 0, ycount * sizeof(double), b->st));
    b->schur.ldy = ldy; b->schur.ykcols = kcols;
    return STBA_OK;
}

// where the landmark inversion in front of a Schur step puts the root of the inverse: only the dense form reads it
double* ba_rinv(stba_ba* b) { return b->schur.mode == STBA_SCHUR_DENSE ? b->Rinv9.get() : nullptr; }

// S (lower triangle), rhs, Hcc, gc from the linearisation and the inverse landmark blocks: the pair plan or the dense product
int ba_schur_step(stba_ba* b) {
    if (b->schur.mode == STBA_SCHUR_DENSE) {
        STBA_TRY(ba_dense_alloc(b));
        SchurDenseArgs da;
        da.n_cams = b->nc; da.n_chunks = b->n_chunks;
        da.chunk_begin = b->chunk_begin; da.chunk_end = b->chunk_end; da.cam_chunk_start = b->cam_chunk_start; da.cam_perm = b->cam_perm;
        da.obs_cam = b->obs_cam; da.obs_pt = b->obs_pt;
        da.J8 = b->J8; da.omask = b->omask; da.Jc12 = ba_general_jc(b); da.r = b->r; da.Hinv6 = b->Hinv6; da.Rinv9 = b->Rinv9; da.gp = b->gp;
        da.Y = b->schur.Y; da.ldy = b->schur.ldy; da.kcols = b->schur.ykcols; da.partial = b->schur.yv; da.ws = b->schur.yws; da.dup_run = b->schur.dup_run;
        da.S = b->S(); da.lda = b->lda; da.rhs = b->rhs(); da.Hcc = b->Hcc; da.gc = b->gc;
        return launch_schur_dense(da, b->st);
    }
    SchurArgs sa;
    sa.task_cam = b->schur.task_cam; sa.cam_start = b->schur.cam_start; sa.task_col_lo = b->schur.task_col_lo; sa.task_col_hi = b->schur.task_col_hi;
    sa.row_col_ptr = b->schur.row_col_ptr; sa.row_cols = b->schur.row_cols; sa.max_cols = b->schur.max_cols; sa.cam_perm = b->cam_perm;
    sa.J8 = b->J8; sa.omask = b->omask; sa.Jc12 = ba_general_jc(b); sa.r = b->r; sa.Hinv6 = b->Hinv6; sa.gp = b->gp;
    sa.S = b->S(); sa.lda = b->lda; sa.rhs = b->rhs(); sa.Hcc = b->Hcc; sa.gc = b->gc;
    sa.obs_pt = b->obs_pt; sa.pair_begin = b->schur.pair_begin; sa.pair_end = b->schur.pair_end; sa.pair_rec = b->schur.pair_rec;
    sa.task_vs_ptr = b->schur.task_vs_ptr; sa.vs_first = b->schur.vs_first; sa.mode = b->schur.plan_mode;
    if (b->schur.lm_slices) {
        sa.task_p_lo = b->schur.task_p_lo; sa.task_p_hi = b->schur.task_p_hi; sa.task_part_off = b->schur.task_part_off; sa.part = b->schur.part;
        sa.row_task_ptr = b->schur.row_task_ptr; sa.row_tasks = b->schur.row_tasks; sa.n_cams = b->nc;
    }
    sa.ablate = knob_int("STBA_SCHUR_ABLATE", 0);
    return launch_schur_rows(sa, b->schur.n_tasks, b->st);
}

// S (damped, padded, rhs row in place) on the device.  One cross-rank sum carries S, diag(Hcc),
// gc, rhs and the scalar slots.
int ba_build_reduced(stba_ba* b, const Damping& dm) {
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
    if (!b->ar.fn && !dm.explicit_d && b->n == 6 * b->nc) {
        // one rank: camera blocks, LM diagonal, damping and padding in one launch
        STBA_TRY(launch_reduced_finalize(b->nc, b->n, b->Hcc, b->gc, b->cam_fixed, b->S(), b->lda, b->rhs(), b->ex_diag(), b->ex_gc(),
                                         b->scale_c, init_scale, dm.use_scaling, dm.radius, dm.dmin, dm.dmax, b->dc, 0, b->st));
        b->scale_init = true;
        return STBA_OK;
    }
    STBA_TRY(launch_reduced_add_camera(b->nc, b->Hcc, b->gc, b->S(), b->lda, b->rhs(), b->ex_diag(), b->ex_gc(),
                                       b->st));
    if (b->ar.fn) STBA_TRY(ba_allreduce_system(b));      // S and the extras, summed across ranks
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
int ba_fill_scalar_slots(stba_ba* b, double* cost2_dev) {
    return launch_linear_finish(b->cost_partial, b->n_cost(), b->upd_partial_p, point_blocks_grid(b->np), cost2_dev, b->ex_scalar(), b->lda,
                                SC_COST2, SC_GPMAX0 + b->ar.rank, b->st);
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
int ba_backsub_trial(stba_ba* b) {
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
int ba_trial(stba_ba* b, double* host_out, bool updated, bool with_jac, double host_seq) {
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
                                 b->ex_scalar() + SC_COST2, b->ex_scalar() + SC_GPMAX0, b->ar.world, b->ex_gc(), b->n, b->trial,
                                 b->ar.fn ? nullptr : host_out, host_seq, b->st));
    if (b->ar.fn) {
        if (b->ar.fn(b->ar.user, b->trial, TS_TIMEOUT + 1, b->st) != 0) return fail(STBA_ERR_CALLBACK, "all-reduce hook failed");
        // (several ranks: the block goes to the host behind the cross-rank sum of its first five entries)
        if (host_out) hipLaunchKernelGGL(export_trial_kernel, dim3(1), dim3(64), 0, b->st, b->trial, b->flag, host_out, host_seq);
        STBA_HIP(hipGetLastError());
    }
    return STBA_OK;
}

// reads {cost2, gpmax slots, gc} after a reduced-system build and returns cost / gradient max norm
int ba_read_linear_scalars(stba_ba* b, double* cost, double* gmax) {
    std::vector<double> h((size_t)SC_GPMAX0 + b->ar.world);
    std::vector<double> g((size_t)b->n);
    STBA_TRY(download(h.data(), b->ex_scalar(), h.size(), b->st));
    STBA_TRY(download(g.data(), b->ex_gc(), g.size(), b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    *cost = 0.5 * h[SC_COST2];
    double m = 0.0;
    for (int k = 0; k < b->ar.world; ++k) m = std::max(m, h[SC_GPMAX0 + k]);
    for (double v : g) m = std::max(m, std::fabs(v));
    *gmax = m;
    return STBA_OK;
}

// covariance (covariance.hip): linearisation, landmark blocks and the UNDAMPED reduced system at the current parameters, through the
// explicit-damping path of stba_ba_reduced_system with dc = dp = 0 (constant dofs get their 1 on the diagonal as always).  The LM
// state stays as it was: parameters and their buffers, the Jacobi scale (ba_build_reduced marks it made; this path made none) and
// the speculation's stamped block; every solve starts with a linearisation of its own.
int ba_cov_build(stba_ba* b) {
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
PcgVecs pcg_vecs(stba_ba* b) {
    PcgVecs v;
    const size_t L = (size_t)b->lda, nw = (size_t)is_vec_grid(b->nc);
    v.x = b->dxc; v.r = b->pcg.vec; v.z = b->pcg.vec + L; v.p = b->pcg.vec + 2 * L; v.q = b->pcg.vec + 3 * L;
    v.b = b->rhs(); v.Minv = b->pcg.minv;
    v.part_rz = b->pcg.part; v.part_pq = b->pcg.part + nw; v.part_q = b->pcg.part + 2 * nw;
    v.state = b->pcg.state;
    return v;
}

int ba_pcg_alloc(stba_ba* b) {
    STBA_TRY(b->pcg.vec.alloc(4 * (size_t)b->lda));
    STBA_TRY(b->pcg.minv.alloc((size_t)b->nc * 36));
    STBA_TRY(b->pcg.sj.alloc((size_t)std::max(b->n_chunks, 1) * 24));
    STBA_TRY(b->pcg.part.alloc(3 * (size_t)is_vec_grid(b->nc)));
    STBA_TRY(b->pcg.state.alloc(1));
    STBA_HIP(hipMemsetAsync(b->pcg.vec, 0, 4 * (size_t)b->lda * sizeof(double), b->st));
    STBA_HIP(hipMemsetAsync(b->pcg.state, 0, sizeof(PcgState), b->st));
    STBA_HIP(hipMemsetAsync(b->flag, 0, sizeof(int), b->st));       // (no factorisation: the trial block's flag stays 0)
    return STBA_OK;
}

// landmark pass of one product: zp (in dxp) = V^-1 (-gp - W^T x); gp = null for S x.  skip: the PCG's state (null: always run)
int ba_is_landmark_pass(stba_ba* b, const double* x, const double* gp, PcgState* skip) {
    BacksubUpdate up{};
    up.skip = skip ? &skip->done : nullptr;
    return launch_backsub(b->np, b->pt_start, b->obs_cam, b->J8, b->omask, b->Hinv6, gp, x, b->dxp, b->st, &up, ba_general_jc(b));
}
// camera pass: y = (Hcc + D) p + W zp (IS_FINAL_APPLY, p^T y partials into pq_part) | y = -gc - W zp (IS_FINAL_RHS)
int ba_is_camera_pass(stba_ba* b, int mode, const double* p, double* y, double* pq_part, const PcgState* skip) {
    STBA_TRY(launch_is_cam_gather(b->n_chunks, b->chunk_begin, b->chunk_end, b->cam_perm, b->obs_pt, b->J8, b->omask, ba_general_jc(b),
                                  b->dxp, skip, b->cam_partial, b->st));
    return launch_is_cam_final(b->nc, mode, b->cam_chunk_start, b->cam_partial, b->Hcc, b->dc, b->gc, b->cam_fixed, p, y, pq_part, skip, b->st);
}
int ba_is_precond(stba_ba* b, int kind) {
    if (kind == STBA_PRECOND_SCHUR_JACOBI)
        STBA_TRY(launch_is_sj_gather(b->n_chunks, b->no, b->chunk_begin, b->chunk_end, b->cam_perm, b->obs_cam, b->obs_pt, b->J8, b->omask,
                                     ba_general_jc(b), b->Hinv6, b->pcg.sj, b->st));
    return launch_is_precond(b->nc, kind, b->Hcc, b->dc, b->scale_c, b->cam_fixed, b->cam_chunk_start, b->pcg.sj, b->pcg.minv, b->st);
}
// reduced right-hand side rhs = -(gc - W V^-1 gp): the landmark pass with x = 0, then the camera pass
int ba_is_rhs(stba_ba* b) {
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
    return ba_is_precond(b, b->pcg.precond);
}
int ba_build(stba_ba* b, const Damping& dm) { return b->iterative ? ba_build_implicit(b, dm) : ba_build_reduced(b, dm); }

// PCG on the reduced system into dxc.  check_every iterations are enqueued at a time, then the solve's state travels to the host
// as a stamped block; every kernel of an iteration behind the device's decision returns at once.  *fail: Ceres' FAILURE (the LM
// step is not ok)
int ba_pcg_solve(stba_ba* b, int* fail_out) {
    const PcgVecs v = pcg_vecs(b);
    STBA_TRY(launch_is_vec(b->nc, IS_VEC_INIT, v, b->st));
    STBA_TRY(launch_is_check(b->nc, IS_CHECK_INIT, v, b->pcg.eta, b->pcg.min, b->pcg.max, b->st));
    if (!b->pcg.host.host) STBA_TRY(b->pcg.host.alloc((size_t)stamped_doubles(4)));
    double hs[4] = {0.0, 0.0, 0.0, 0.0};
    long enqueued = 0;
    while (true) {
        for (int k = 0; k < b->pcg.check; ++k) {
            STBA_TRY(launch_is_vec(b->nc, IS_VEC_DIR, v, b->st));
            STBA_TRY(ba_is_landmark_pass(b, v.p, nullptr, b->pcg.state));
            STBA_TRY(ba_is_camera_pass(b, IS_FINAL_APPLY, v.p, v.q, v.part_pq, b->pcg.state));
            STBA_TRY(launch_is_vec(b->nc, IS_VEC_UPDATE, v, b->st));
            STBA_TRY(launch_is_check(b->nc, IS_CHECK_ITER, v, b->pcg.eta, b->pcg.min, b->pcg.max, b->st));
        }
        enqueued += b->pcg.check;
        const double seq = (b->pcg.seq += 1.0);
        STBA_TRY(launch_is_export(b->pcg.state, b->pcg.host.dev, seq, b->st));
        STBA_TRY(stamped_wait(b->pcg.host.host, 4, [seq](double st) { return st == seq; }, hs, hip_stream_state(b->st), "PCG state", 120.0));
        if (hs[0] != 0.0) break;
        if (enqueued > (long)b->pcg.max + b->pcg.check) return fail(STBA_ERR_HIP, "PCG: the device did not stop at max_iterations");
    }
    b->pcg.last_it = (int)hs[1];
    b->pcg.last_cap = hs[3] != 0.0 ? 1 : 0;
    *fail_out = hs[2] != 0.0 ? 1 : 0;
    return STBA_OK;
}
// the last solve belongs to an LM iteration (not to a trial step the loop discards behind a late convergence test)
void ba_pcg_account(stba_ba* b, int lm_iter) {
    if (lm_iter >= 1) { b->pcg.per_iter.resize((size_t)lm_iter, 0); b->pcg.per_iter[(size_t)lm_iter - 1] = b->pcg.last_it; }
    b->pcg.sum.iterations_total += b->pcg.last_it;
    b->pcg.sum.solves += 1;
    b->pcg.sum.hit_cap += b->pcg.last_cap;
    b->pcg.sum.max_iterations_in_a_solve = std::max(b->pcg.sum.max_iterations_in_a_solve, b->pcg.last_it);
    b->pcg.sum.last_eta = b->pcg.eta;
}

}  // namespace stba
