// ba_stages.hip -- the stage, measurement and covariance entry points of the bundle-adjustment engine (include/stba.h): one LM
// iteration by hand (evaluate, cost, normal_blocks, reduced_system, solve_reduced, back_substitute, apply_step; schur_apply for
// ITERATIVE_SCHUR), the kernel timings (time_linearize, time_schur, time_schur_apply) and the six covariance calls.  Each checks the
// have_* state the one before it left and enqueues through ba_linear.hip; none of them is on the path of a solve.
#include <vector>

#include "ba_engine.hpp"

extern "C" {

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

int stba_ba_evaluate(stba_ba* b, double* cost, double* r, double* Jc, double* Jp) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    STBA_TRY(ba_linearize(b, b->cur, b->trial + TS_COST2));
    double c2 = 0.0;
    STBA_TRY(download(&c2, b->trial + TS_COST2, 1, b->st));
    const size_t no = (size_t)b->no;
    std::vector<double> tr, tjc, tjp;
    if (r) { tr.resize(no * 2); STBA_TRY(download(tr.data(), reinterpret_cast<double*>(b->r.get()), no * 2, b->st)); }
    DevBuf<double> djc, djp;     // the device holds the compact Jacobian; the 2x6 | 2x3 form is expanded for the caller
    if ((Jc || Jp) && b->hl.fn) return fail(STBA_ERR_STATE, "stba_ba_evaluate: with a host lineariser the Jacobians are the caller's own");
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
    if (flag_h == CHOL_FLAG_TIMEOUT && !b->ar.fn && b->have_blocks) {
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
    if (lds_atomics_per_launch) *lds_atomics_per_launch = b->schur.lds_atomics;
    if (pairs_per_launch) *pairs_per_launch = b->schur.pairs;
    ba_invalidate(b);
    return STBA_OK;
}

int stba_ba_covariance_compute(stba_ba* b, double min_rcond, double* rcond_out) {
    STBA_TRY(refuse_iterative(b, "stba_ba_covariance_compute", "and the covariance needs the explicit reduced system S"));
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    if (b->ar.fn) return fail(STBA_ERR_STATE, "stba_ba_covariance_compute: the engine holds one landmark shard of several ranks; covariance needs one rank");
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
