// ba_factors.hip -- the factors of the bundle adjustment through the C ABI (include/stba.h): the host lineariser, the loss table, the
// per-observation weights, the camera pose priors, the relative-pose factors and the landmark position priors -- their setters, counts, kernel geometries and
// evaluate_* entry points.  Host code only: the kernels are in ba_kernels.hip, ba_prior.hip, ba_between.hip and ba_landmark_prior.hip.
// A setter checks first (ba_features.hpp: does the engine take the factor at all; ba_factor_input.hpp: every row, into host vectors, the
// smallest bad index named), then builds and uploads a LOCAL set, then commits: ba_factors_changed and one move assignment.
#include "ba_engine.hpp"
#include "ba_factor_input.hpp"
#include "robust_loss.hpp"

namespace {

// Jc12, the camera blocks of the general form, lives from the first setter that makes ba_wants_general_form true to the factor setter
// that makes it false.  Before the commit: allocated into `fresh` (a failed allocation leaves the engine untouched) ...
int jc12_reserve(const stba_ba* b, bool general_after, DevBuf<double>& fresh) {
    if (general_after && !b->Jc12) STBA_TRY(fresh.alloc((size_t)b->no * 12));
    return STBA_OK;
}
// ... after it: taken, or released (96 B per observation nobody reads any more)
void jc12_settle(stba_ba* b, DevBuf<double>& fresh) {
    if (fresh) b->Jc12 = std::move(fresh);
    if (!ba_wants_general_form(b)) b->Jc12.reset();
}

// the rows of an SE(3) factor list checked into hp [n][7] (quaternions normalised) and hw [n][36]; `row`: "prior" or "edge", `what`:
// ba_factor_input.hpp's name of the 7 doubles.  index_check(k, &why) runs first in every row
template <class IndexCheck>
int se3_rows_check(const std::string& who, const char* row, const char* what, size_t n, const double* pose, const double* information,
                   const double* sqrt_information, IndexCheck index_check, std::vector<double>& hp, std::vector<double>& hw) {
    hp.resize(n * 7); hw.resize(n * 36);
    for (size_t k = 0; k < n; ++k) {
        std::string why;
        int rc = index_check(k, &why);
        if (!rc) rc = pose7_check_normalise(pose + k * 7, &hp[k * 7], what, &why);
        if (!rc) rc = sqrt_information6(information ? information + k * 36 : nullptr, sqrt_information ? sqrt_information + k * 36 : nullptr, &hw[k * 36], &why);
        if (rc) return fail(rc, who + ": " + row + " " + std::to_string(k) + ": " + why);
    }
    return STBA_OK;
}

}  // namespace

extern "C" {

int stba_ba_set_host_linearizer(stba_ba* b, stba_ba_linearize_fn fn, void* user) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "null engine");
    STBA_TRY(ba_refuse(b, "stba_ba_set_host_linearizer", fn != nullptr));
    // (straight into the engine: nothing else is committed; clearing the callback keeps the buffer)
    STBA_TRY(jc12_reserve(b, ba_wants_general_form(fn != nullptr, b->loss.kind.get() != nullptr, b->winfo.get() != nullptr), b->Jc12));
    b->hl.fn = fn; b->hl.user = user;
    ba_invalidate(b);
    return STBA_OK;
}

// the per-observation loss table: checked on the host BEFORE anything is replaced (a refused call leaves the engine with the table it
// had), permuted into the engine's landmark-major order, uploaded into NEW arrays that are swapped in; kind == NULL releases the table
int stba_ba_set_loss(stba_ba* b, const int* kind, const double* a, const double* lb, const double* scale) {
    const char* who = "stba_ba_set_loss";
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": null engine");
    LossTable fresh;
    DevBuf<double> jc_new;
    if (kind) {
        STBA_TRY(ba_refuse(b, who));
        const size_t m = (size_t)b->no;
        std::vector<double> ha, hb, hs;
        STBA_TRY(loss_table_check(who, "observation", m, kind, a, lb, scale, ha, hb, hs));
        std::vector<int> pk(m);
        std::vector<double> pa(m), pb(m), ps(m);
        for (size_t p = 0; p < m; ++p) {                    // the engine's order: b->perm = position -> the caller's index
            const size_t i = (size_t)b->perm[p];
            pk[p] = kind[i]; pa[p] = ha[i]; pb[p] = hb[i]; ps[p] = hs[i];
        }
        STBA_TRY(jc12_reserve(b, true, jc_new));
        STBA_TRY(to_device(who, fresh.kind, pk, b->st)); STBA_TRY(to_device(who, fresh.a, pa, b->st));
        STBA_TRY(to_device(who, fresh.b, pb, b->st)); STBA_TRY(to_device(who, fresh.scale, ps, b->st));
        if (m > 0 && hipStreamSynchronize(b->st) != hipSuccess) return fail(STBA_ERR_HIP, std::string(who) + ": upload failed");
    }
    STBA_TRY(ba_factors_changed(b));
    b->loss = std::move(fresh);
    jc12_settle(b, jc_new);
    return STBA_OK;
}

// the per-observation weights: checked (and, for the information form, factored) on the host BEFORE anything is replaced, permuted
// into the engine's landmark-major order, uploaded into a NEW array that is swapped in; in == NULL, or an array whose every W is
// exactly the identity, goes back to the identity (no array held)
static int ba_set_weights(stba_ba* b, const double* in, bool sqrt_form, const char* who) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": null engine");
    DevBuf<double> w_new, jc_new;
    const size_t m = (size_t)b->no;
    std::vector<double> hw;
    if (in) {
        // (the messages below name the row as "observation <index>:" -- include/stba/g2o.h reads the index out of that text to name the
        // edge; keep the wording)
        hw.resize(m * 4);
        bool all_identity = true;
        for (size_t e = 0; e < m; ++e) {
            if (sqrt_form) {
                for (int k = 0; k < 4; ++k) {
                    if (!std::isfinite(in[e * 4 + k]))
                        return fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": observation " + std::to_string(e) + ": the square-root information has an entry that is not finite");
                    hw[e * 4 + k] = in[e * 4 + k];
                }
            } else if (!ba_information_factor(in + e * 4, &hw[e * 4])) {
                return fail(STBA_ERR_NOT_POSITIVE_DEFINITE, std::string(who) + ": observation " + std::to_string(e) + ": the information matrix is not positive definite (or has an entry that is not finite)");
            }
            const double* w = &hw[e * 4];
            all_identity = all_identity && w[0] == 1.0 && w[1] == 0.0 && w[2] == 0.0 && w[3] == 1.0;
        }
        // every W exactly the identity IS the engine without weights: the array is not held (as for NULL), the lossless kernels run
        if (all_identity) in = nullptr;
    }
    if (in) {
        STBA_TRY(ba_refuse(b, who));
        std::vector<double> pw(m * 4);
        for (size_t p = 0; p < m; ++p) memcpy(&pw[p * 4], &hw[(size_t)b->perm[p] * 4], 4 * sizeof(double));   // the engine's order
        STBA_TRY(jc12_reserve(b, true, jc_new));
        STBA_TRY(to_device(who, w_new, pw, b->st));
        if (m > 0 && hipStreamSynchronize(b->st) != hipSuccess) return fail(STBA_ERR_HIP, std::string(who) + ": upload failed");
    }
    STBA_TRY(ba_factors_changed(b));
    b->winfo = std::move(w_new);
    jc12_settle(b, jc_new);
    return STBA_OK;
}

int stba_ba_set_information(stba_ba* b, const double* information) { return ba_set_weights(b, information, false, "stba_ba_set_information"); }
int stba_ba_set_sqrt_information(stba_ba* b, const double* sqrt_information) { return ba_set_weights(b, sqrt_information, true, "stba_ba_set_sqrt_information"); }

int stba_ba_has_information(const stba_ba* b, int* has) {
    if (!b || !has) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_has_information: null argument");
    *has = b->winfo ? 1 : 0;
    return STBA_OK;
}

int stba_ba_get_sqrt_information(stba_ba* b, double* out) {
    if (!b || !out) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_get_sqrt_information: null argument");
    const size_t m = (size_t)b->no;
    if (!b->winfo) {
        for (size_t e = 0; e < m; ++e) { out[e * 4] = 1.0; out[e * 4 + 1] = 0.0; out[e * 4 + 2] = 0.0; out[e * 4 + 3] = 1.0; }
        return STBA_OK;
    }
    std::vector<double> pw(m * 4);
    if (m > 0) STBA_TRY(download(pw.data(), b->winfo, m * 4, b->st));
    STBA_HIP(hipStreamSynchronize(b->st));
    for (size_t p = 0; p < m; ++p) memcpy(&out[(size_t)b->perm[p] * 4], &pw[p * 4], 4 * sizeof(double));
    return STBA_OK;
}

// ---- camera pose priors.  Everything is checked -- and, for the information form, factored -- on the host BEFORE
// anything is replaced; the priors are grouped by camera (a stable sort: inside a group the caller's order), uploaded into NEW arrays
// that are swapped in.  n == 0 releases them: the engine then enqueues exactly what one that never had priors enqueues
int stba_ba_set_pose_priors(stba_ba* b, int n, const int* cam, const double* pose, const double* information, const double* sqrt_information) {
    const std::string who = "stba_ba_set_pose_priors";
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": null engine");
    if (n < 0) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": n is negative");
    if (information && sqrt_information) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": give information or sqrt_information, not both");
    PriorSet fresh;
    if (n > 0) {
        if (!cam || !pose) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": null cam or pose array");
        STBA_TRY(ba_refuse(b, who.c_str()));
        const size_t m = (size_t)n;
        const int nc = b->nc;
        std::vector<double> hp, hw;
        STBA_TRY(se3_rows_check(who, "prior", "the pose", m, pose, information, sqrt_information, [cam, nc](size_t k, std::string* why) {
            if (cam[k] >= 0 && cam[k] < nc) return 0;
            *why = "camera index " + std::to_string(cam[k]) + " out of range";
            return (int)STBA_ERR_INVALID_ARGUMENT;
        }, hp, hw));
        fresh.order.resize(m);
        for (size_t k = 0; k < m; ++k) fresh.order[k] = (int)k;
        std::vector<int> gptr, gcam;
        group_csr(m, [cam](int k) { return cam[k]; }, fresh.order, gptr, gcam);
        std::vector<double> gp(m * 7), gw(m * 36);
        for (size_t p = 0; p < m; ++p) {
            const size_t k = (size_t)fresh.order[p];
            memcpy(&gp[p * 7], &hp[k * 7], 7 * sizeof(double));
            memcpy(&gw[p * 36], &hw[k * 36], 36 * sizeof(double));
        }
        fresh.n = n; fresh.n_groups = (int)gcam.size();
        STBA_TRY(to_device(who, fresh.ptr, gptr, b->st)); STBA_TRY(to_device(who, fresh.cam, gcam, b->st));
        STBA_TRY(to_device(who, fresh.pose, gp, b->st)); STBA_TRY(to_device(who, fresh.W, gw, b->st));
        if (hipStreamSynchronize(b->st) != hipSuccess) return fail(STBA_ERR_HIP, who + ": upload failed");
    }
    STBA_TRY(ba_factors_changed(b));
    b->prior = std::move(fresh);
    return STBA_OK;
}

int stba_ba_pose_prior_count(const stba_ba* b, int* n) {
    if (!b || !n) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_pose_prior_count: null argument");
    *n = b->prior.n;
    return STBA_OK;
}

int stba_ba_pose_prior_kernel_geometry(const stba_ba* b, int* cameras_per_workgroup) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_pose_prior_kernel_geometry: null engine");
    if (cameras_per_workgroup) *cameras_per_workgroup = PRIOR_CAMS_PER_WG;
    return STBA_OK;
}

// the whitened residuals and Jacobians of the priors at the current parameters, by the block kernel itself (no blocks written),
// and their cost by the cost kernel; the caller's order.  The engine's linearisation state is not touched
int stba_ba_evaluate_pose_priors(stba_ba* b, double* cost, double* r, double* J) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_evaluate_pose_priors: null engine");
    if (cost) *cost = 0.0;
    if (!b->prior.n) return STBA_OK;
    const size_t m = (size_t)b->prior.n;
    DevBuf<double> dr, dj, dcost;
    std::vector<double> hr, hj;
    double c2 = 0.0;
    if (r || J) {
        STBA_TRY(dr.alloc(m * 6));
        STBA_TRY(dj.alloc(m * 36));
        STBA_TRY(launch_prior_blocks(b->prior_args(), b->cams[b->cur], nullptr, nullptr, dr, dj, b->st));
        hr.resize(m * 6); hj.resize(m * 36);
        STBA_TRY(download(hr.data(), dr, m * 6, b->st));
        STBA_TRY(download(hj.data(), dj, m * 36, b->st));
    }
    if (cost) {
        STBA_TRY(dcost.alloc(1));
        STBA_TRY(launch_prior_cost(b->prior_args(), b->cams[b->cur], dcost, b->st));
        STBA_TRY(download(&c2, dcost, 1, b->st));
    }
    STBA_HIP(hipStreamSynchronize(b->st));
    if (cost) *cost = 0.5 * c2;
    for (size_t p = 0; p < m && (r || J); ++p) {
        const size_t k = (size_t)b->prior.order[p];
        if (r) memcpy(r + k * 6, &hr[p * 6], 6 * sizeof(double));
        if (J) memcpy(J + k * 36, &hj[p * 36], 36 * sizeof(double));
    }
    return STBA_OK;
}

// ---- camera-to-camera relative-pose factors.  As with the priors everything is checked -- and, for the information
// form, factored -- on the host BEFORE anything is replaced.  The edges stay in the caller's order; two stable sorts make the
// references by camera and by unordered pair (inside a group the caller's order).  n == 0 releases everything: the engine then
// enqueues exactly what one that never had edges enqueues
int stba_ba_set_relative_poses(stba_ba* b, int n, const int* cam_i, const int* cam_j, const double* meas, const double* information,
                               const double* sqrt_information) {
    const std::string who = "stba_ba_set_relative_poses";
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": null engine");
    if (n < 0) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": n is negative");
    if (information && sqrt_information) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": give information or sqrt_information, not both");
    BetweenSet fresh;
    if (n > 0) {
        if (!cam_i || !cam_j || !meas) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": null cam_i, cam_j or meas array");
        STBA_TRY(ba_refuse(b, who.c_str()));
        const size_t m = (size_t)n;
        const int nc = b->nc;
        std::vector<double> hm, hw;
        STBA_TRY(se3_rows_check(who, "edge", "the measurement", m, meas, information, sqrt_information, [cam_i, cam_j, nc](size_t k, std::string* why) {
            for (int c : {cam_i[k], cam_j[k]})
                if (c < 0 || c >= nc) { *why = "camera index " + std::to_string(c) + " out of range"; return (int)STBA_ERR_INVALID_ARGUMENT; }
            if (cam_i[k] != cam_j[k]) return 0;
            *why = "cam_i == cam_j (" + std::to_string(cam_i[k]) + ")";
            return (int)STBA_ERR_INVALID_ARGUMENT;
        }, hm, hw));
        // by camera: 2 n references (2 * edge + side), side 1 where the camera is the edge's j
        std::vector<int> cref(2 * m), cgp, cgc;
        for (size_t k = 0; k < 2 * m; ++k) cref[k] = (int)k;
        group_csr(2 * m, [cam_i, cam_j](int ref) { return (ref & 1) ? cam_j[ref >> 1] : cam_i[ref >> 1]; }, cref, cgp, cgc);
        // by unordered pair (hi, lo): n references, side 1 where hi is the edge's j
        std::vector<int> pref(m), pgp;
        std::vector<std::pair<int, int>> pairs;
        for (size_t k = 0; k < m; ++k) pref[k] = 2 * (int)k + (cam_j[k] > cam_i[k] ? 1 : 0);
        group_csr(m, [cam_i, cam_j](int ref) { const int e = ref >> 1; return std::make_pair(std::max(cam_i[e], cam_j[e]), std::min(cam_i[e], cam_j[e])); },
                  pref, pgp, pairs);
        std::vector<int2> pgq;
        for (const auto& hl : pairs) pgq.push_back(make_int2(hl.first, hl.second));
        fresh.n = n; fresh.n_cg = (int)cgc.size(); fresh.n_pg = (int)pgq.size();
        STBA_TRY(to_device(who, fresh.i, cam_i, m, b->st)); STBA_TRY(to_device(who, fresh.j, cam_j, m, b->st));
        STBA_TRY(to_device(who, fresh.meas, hm, b->st)); STBA_TRY(to_device(who, fresh.W, hw, b->st));
        STBA_TRY(to_device(who, fresh.cg_ptr, cgp, b->st)); STBA_TRY(to_device(who, fresh.cg_cam, cgc, b->st)); STBA_TRY(to_device(who, fresh.cg_ref, cref, b->st));
        STBA_TRY(to_device(who, fresh.pg_ptr, pgp, b->st)); STBA_TRY(to_device(who, fresh.pg_pair, pgq, b->st)); STBA_TRY(to_device(who, fresh.pg_ref, pref, b->st));
        if (hipStreamSynchronize(b->st) != hipSuccess) return fail(STBA_ERR_HIP, who + ": upload failed");
    }
    STBA_TRY(ba_factors_changed(b));
    b->btw = std::move(fresh);
    return STBA_OK;
}

int stba_ba_relative_pose_count(const stba_ba* b, int* n) {
    if (!b || !n) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_relative_pose_count: null argument");
    *n = b->btw.n;
    return STBA_OK;
}

int stba_ba_relative_pose_kernel_geometry(const stba_ba* b, int* groups_per_workgroup) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_relative_pose_kernel_geometry: null engine");
    if (groups_per_workgroup) *groups_per_workgroup = BETWEEN_GROUPS_PER_WG;
    return STBA_OK;
}

// the whitened residuals and Jacobians of the edges at the current parameters, by the pair groups of the block kernel itself (no
// blocks written), and their cost by the cost kernel; the caller's order.  The engine's linearisation state is not touched
int stba_ba_evaluate_relative_poses(stba_ba* b, double* cost, double* r, double* Ji, double* Jj) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_evaluate_relative_poses: null engine");
    if (cost) *cost = 0.0;
    if (!b->btw.n) return STBA_OK;
    const size_t m = (size_t)b->btw.n;
    DevBuf<double> dr, dji, djj, dcost;
    double c2 = 0.0;
    if (r || Ji || Jj) {
        STBA_TRY(dr.alloc(m * 6)); STBA_TRY(dji.alloc(m * 36)); STBA_TRY(djj.alloc(m * 36));
        STBA_TRY(launch_between_blocks(b->between_args(), b->cams[b->cur], nullptr, nullptr, nullptr, b->lda, dr, dji, djj, b->st));
        if (r) STBA_TRY(download(r, dr, m * 6, b->st));
        if (Ji) STBA_TRY(download(Ji, dji, m * 36, b->st));
        if (Jj) STBA_TRY(download(Jj, djj, m * 36, b->st));
    }
    if (cost) {
        STBA_TRY(dcost.alloc(1));
        STBA_TRY(launch_between_cost(b->between_args(), b->cams[b->cur], dcost, b->st));
        STBA_TRY(download(&c2, dcost, 1, b->st));
    }
    STBA_HIP(hipStreamSynchronize(b->st));
    if (cost) *cost = 0.5 * c2;
    return STBA_OK;
}

// ---- landmark position priors.  As with the pose priors everything is checked -- and, for the information form,
// factored -- on the host BEFORE anything is replaced; the priors are grouped by landmark (a stable sort: inside a group the caller's
// order), uploaded into NEW arrays that are swapped in.  n == 0 releases them and is never refused: the engine then enqueues exactly
// what one that never had priors enqueues
int stba_ba_set_landmark_priors(stba_ba* b, int n, const int* pt, const double* position, const double* information, const double* sqrt_information) {
    const std::string who = "stba_ba_set_landmark_priors";
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": null engine");
    if (n < 0) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": n is negative");
    LandmarkPriorSet fresh;
    if (n > 0) {                // (n == 0 reads none of the arrays and is never refused)
        if (information && sqrt_information) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": give information or sqrt_information, not both");
        if (!pt || !position) return fail(STBA_ERR_INVALID_ARGUMENT, who + ": null pt or position array");
        STBA_TRY(ba_refuse(b, who.c_str()));
        const size_t m = (size_t)n;
        std::vector<double> hw(m * 9);
        for (size_t k = 0; k < m; ++k) {
            std::string why;
            const int rc = landmark_prior_check(pt[k], b->np, position + k * 3, information ? information + k * 9 : nullptr,
                                                sqrt_information ? sqrt_information + k * 9 : nullptr, &hw[k * 9], &why);
            if (rc) return fail(rc, who + ": prior " + std::to_string(k) + ": " + why);
        }
        std::vector<int> start;
        landmark_prior_group(m, pt, b->np, fresh.order, start);
        std::vector<int> gpt(m);
        std::vector<double> gpos(m * 3), gw(m * 9);
        for (size_t p = 0; p < m; ++p) {
            const size_t k = (size_t)fresh.order[p];
            gpt[p] = pt[k];
            memcpy(&gpos[p * 3], position + k * 3, 3 * sizeof(double));
            memcpy(&gw[p * 9], &hw[k * 9], 9 * sizeof(double));
        }
        fresh.n = n;
        STBA_TRY(to_device(who, fresh.start, start, b->st)); STBA_TRY(to_device(who, fresh.pt, gpt, b->st));
        STBA_TRY(to_device(who, fresh.pos, gpos, b->st)); STBA_TRY(to_device(who, fresh.W, gw, b->st));
        STBA_TRY(fresh.cost_part.alloc((size_t)landmark_prior_cost_grid(n)));
        if (hipStreamSynchronize(b->st) != hipSuccess) return fail(STBA_ERR_HIP, who + ": upload failed");
    }
    STBA_TRY(ba_factors_changed(b));
    b->lprior = std::move(fresh);
    return STBA_OK;
}

int stba_ba_landmark_prior_count(const stba_ba* b, int* n) {
    if (!b || !n) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_landmark_prior_count: null argument");
    *n = b->lprior.n;
    return STBA_OK;
}

int stba_ba_landmark_prior_kernel_geometry(const stba_ba* b, int* landmarks_per_workgroup) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_landmark_prior_kernel_geometry: null engine");
    if (landmarks_per_workgroup) *landmarks_per_workgroup = LP_LM_PER_WG;
    return STBA_OK;
}

// the whitened residuals and Jacobians of the priors at the current parameters, by the block kernel itself (no blocks written),
// and their cost by the cost kernel; the caller's order.  The engine's linearisation state is not touched
int stba_ba_evaluate_landmark_priors(stba_ba* b, double* cost, double* r, double* J) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_evaluate_landmark_priors: null engine");
    if (cost) *cost = 0.0;
    if (!b->lprior.n) return STBA_OK;
    const size_t m = (size_t)b->lprior.n;
    DevBuf<double> dr, dj, dcost;
    std::vector<double> hr, hj;
    double c2 = 0.0;
    if (r || J) {
        STBA_TRY(dr.alloc(m * 3));
        STBA_TRY(dj.alloc(m * 9));
        STBA_TRY(launch_landmark_prior_blocks(b->landmark_prior_args(), b->pts[b->cur], nullptr, nullptr, nullptr, dr, dj, b->st));
        hr.resize(m * 3); hj.resize(m * 9);
        STBA_TRY(download(hr.data(), dr, m * 3, b->st));
        STBA_TRY(download(hj.data(), dj, m * 9, b->st));
    }
    if (cost) {
        STBA_TRY(dcost.alloc(1));
        STBA_TRY(launch_landmark_prior_cost(b->landmark_prior_args(), b->pts[b->cur], b->lprior.cost_part, dcost, b->st));
        STBA_TRY(download(&c2, dcost, 1, b->st));
    }
    STBA_HIP(hipStreamSynchronize(b->st));
    if (cost) *cost = 0.5 * c2;
    for (size_t p = 0; p < m && (r || J); ++p) {
        const size_t k = (size_t)b->lprior.order[p];
        if (r) memcpy(r + k * 3, &hr[p * 3], 3 * sizeof(double));
        if (J) memcpy(J + k * 9, &hj[p * 9], 9 * sizeof(double));
    }
    return STBA_OK;
}

int stba_ba_has_loss(const stba_ba* b, int* has) {
    if (!b || !has) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_has_loss: null argument");
    *has = b->loss.kind ? 1 : 0;
    return STBA_OK;
}

int stba_ba_loss_kernel_geometry(const stba_ba* b, int* tile_observations, int* cameras_in_lds, int* max_cameras_in_lds) {
    if (!b) return fail(STBA_ERR_INVALID_ARGUMENT, "stba_ba_loss_kernel_geometry: null engine");
    if (tile_observations) *tile_observations = LIN_ROBUST_THREADS;
    if (cameras_in_lds) *cameras_in_lds = lin_robust_cams_in_lds(b->nc) ? 1 : 0;
    if (max_cameras_in_lds) *max_cameras_in_lds = (int)(((size_t)LIN_MAX_LDS - lin_robust_lds_bytes(0, true, true)) / (7 * sizeof(double)));
    return STBA_OK;
}

}  // extern "C"
