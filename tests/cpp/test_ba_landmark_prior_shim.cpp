// Driver of tests/test_ba_landmark_prior_shim_cpu.py (no argument: host only) and tests/test_gpu_ba_landmark_prior_shim.py
// ("device <scene> <mode>").
// Host mode: ceres::LandmarkPriorFactor::Evaluate.
//   stdin:  n, then n times: position[3] p[3] has_w W[9]
//   stdout: per case one line: r'[3], then J'[9] row-major; then the line "detect a b c d e f": internal::DetectBa on a two-camera BA
//           problem (a) without a prior block, (b) with two on landmark 1 and one on landmark 0 (and the residual <-> observation
//           bookkeeping checked), (c) with one that carries a LossFunction, (d) with one on a 3-block no observation names, (e) with
//           one on a camera's position block, (f) with one on a landmark and a PosePriorFactor on a camera
// Device mode: the reference's BA call site (test_ceres.h:98-152) with LandmarkPriorFactor blocks instead of SetParameterBlockConstant.
//   scene:  nc np no nlp ccov pcov / cams[nc][7] / pts[np][3] / no x (cam pt fx fy) / nlp x (pt position[3] W[9])
//   mode:   lm | iterative | dogleg | inner | callback, each also with "_tight" behind it: function, parameter and gradient tolerance
//           1e-15, at most 60 iterations
//   stdout: "ba <path> <termination> <iterations> <initial cost> <final cost>", "msg <message>", "untouched <0|1>", "cams ...",
//           "pts ...", "cov <path> <ok>", "P <9>", "Q <9>": the covariance of camera ccov's position block and of landmark pcov at the
//           end point
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "stba/ceres.h"

namespace ceres = stba_ceres;

static int device_mode(const char* path, const std::string& mode) {
    FILE* f = std::fopen(path, "r");
    if (!f) return 2;
    int nc, np, no, nlp, ccov, pcov;
    if (std::fscanf(f, "%d %d %d %d %d %d", &nc, &np, &no, &nlp, &ccov, &pcov) != 6) return 2;
    std::vector<double> cams((size_t)nc * 7), pts((size_t)np * 3), feat((size_t)no * 2), pos((size_t)nlp * 3), W((size_t)nlp * 9);
    std::vector<int> oc((size_t)no), op((size_t)no), lp((size_t)nlp);
    for (double& v : cams) if (std::fscanf(f, "%lf", &v) != 1) return 2;
    for (double& v : pts) if (std::fscanf(f, "%lf", &v) != 1) return 2;
    for (int i = 0; i < no; ++i) if (std::fscanf(f, "%d %d %lf %lf", &oc[i], &op[i], &feat[2 * i], &feat[2 * i + 1]) != 4) return 2;
    for (int k = 0; k < nlp; ++k) {
        if (std::fscanf(f, "%d", &lp[k]) != 1) return 2;
        for (int j = 0; j < 3; ++j) if (std::fscanf(f, "%lf", &pos[(size_t)k * 3 + j]) != 1) return 2;
        for (int j = 0; j < 9; ++j) if (std::fscanf(f, "%lf", &W[(size_t)k * 9 + j]) != 1) return 2;
    }
    std::fclose(f);
    const std::vector<double> cams0 = cams, pts0 = pts;
    ceres::Problem problem;
    for (int c = 0; c < nc; ++c) {
        problem.AddParameterBlock(&cams[(size_t)c * 7], 4, new ceres::QuaternionRightPlus);
        problem.AddParameterBlock(&cams[(size_t)c * 7 + 4], 3);
    }
    // the prior blocks sit BETWEEN the observations' blocks (every 7th residual block from the 3rd on, the rest behind them)
    int kp = 0;
    auto add_prior = [&]() {
        problem.AddResidualBlock(ceres::LandmarkPriorFactor::Create(&pos[(size_t)kp * 3], &W[(size_t)kp * 9]), nullptr, &pts[(size_t)lp[kp] * 3]);
        ++kp;
    };
    for (int i = 0; i < no; ++i) {
        if (i >= 3 && i % 7 == 3 && kp < nlp) add_prior();
        problem.AddResidualBlock(ceres::ReprojectionFactor::Create(&feat[2 * i]), nullptr, &cams[(size_t)oc[i] * 7], &cams[(size_t)oc[i] * 7 + 4],
                                 &pts[(size_t)op[i] * 3]);
    }
    while (kp < nlp) add_prior();
    ceres::Solver::Options o;
    o.num_threads = 1;
    const bool tight = mode.size() > 6 && mode.compare(mode.size() - 6, 6, "_tight") == 0;
    const std::string base = tight ? mode.substr(0, mode.size() - 6) : mode;
    if (base == "iterative") o.linear_solver_type = ceres::ITERATIVE_SCHUR;
    if (base == "dogleg") o.trust_region_strategy_type = ceres::DOGLEG;
    if (base == "inner") o.use_inner_iterations = true;
    if (base == "callback") o.force_callback_path = true;
    // (tight: every strategy runs to the minimiser itself, not to its own first point inside Ceres' default function tolerance)
    if (tight) { o.function_tolerance = 1e-15; o.parameter_tolerance = 1e-15; o.gradient_tolerance = 1e-15; o.max_num_iterations = 60; }
    ceres::Solver::Summary sum;
    ceres::Solve(o, &problem, &sum);
    std::printf("ba %s %d %d %.17g %.17g\n", sum.execution_path.empty() ? "none" : sum.execution_path.c_str(), (int)sum.termination_type,
                (int)sum.iterations.size() - 1, sum.initial_cost, sum.final_cost);
    std::printf("msg %s\n", sum.message.c_str());
    std::printf("untouched %d\n", (cams == cams0 && pts == pts0) ? 1 : 0);
    std::printf("cams");
    for (double v : cams) std::printf(" %.17g", v);
    std::printf("\npts");
    for (double v : pts) std::printf(" %.17g", v);
    std::printf("\n");
    if (mode == "lm") {
        ceres::Covariance::Options co;
        ceres::Covariance cov(co);
        const double* t = &cams[(size_t)ccov * 7 + 4];
        const double* l = &pts[(size_t)pcov * 3];
        std::vector<std::pair<const double*, const double*>> blocks = {{t, t}, {l, l}};
        const bool ok = cov.Compute(blocks, &problem);
        std::printf("cov %s %d\n", cov.execution_path().empty() ? "none" : cov.execution_path().c_str(), ok ? 1 : 0);
        double P[9], Q[9];
        if (ok && cov.GetCovarianceBlock(t, t, P) && cov.GetCovarianceBlock(l, l, Q)) {
            std::printf("P"); for (double v : P) std::printf(" %.17g", v);
            std::printf("\nQ"); for (double v : Q) std::printf(" %.17g", v);
            std::printf("\n");
        }
    }
    std::printf("device ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && std::string(argv[1]) == "device") return device_mode(argv[2], argv[3]);
    int n = 0;
    if (std::scanf("%d", &n) != 1) return 2;
    for (int c = 0; c < n; ++c) {
        double pos[3], p[3], W[9];
        int has_w = 0;
        for (double& v : pos) if (std::scanf("%lf", &v) != 1) return 2;
        for (double& v : p) if (std::scanf("%lf", &v) != 1) return 2;
        if (std::scanf("%d", &has_w) != 1) return 2;
        for (double& v : W) if (std::scanf("%lf", &v) != 1) return 2;
        ceres::CostFunction* f = ceres::LandmarkPriorFactor::Create(pos, has_w ? W : nullptr);
        const double* prm[1] = {p};
        double r[3], r2[3], Jp[9];
        double* J[1] = {Jp};
        if (!f->Evaluate(prm, r, J) || !f->Evaluate(prm, r2, nullptr)) return 3;
        for (int i = 0; i < 3; ++i) if (r[i] != r2[i]) return 4;
        for (int i = 0; i < 3; ++i) std::printf("%.17g ", r[i]);
        for (int i = 0; i < 9; ++i) std::printf("%.17g ", Jp[i]);
        std::printf("\n");
        delete f;
    }
    int detect[6];
    for (int variant = 0; variant < 6; ++variant) {
        double q[2][4] = {{0, 0, 0, 1}, {0, 0.1, 0, 0.99498743710662}}, t[2][3] = {{0, 0, 0}, {1, 0, 0}};
        double Lm[2][3] = {{0.1, 0.2, 4}, {-0.3, 0.1, 5}}, lone[3] = {1, 2, 3};
        const double feat[4][2] = {{0.01, 0.02}, {0.03, 0.04}, {0.05, 0.06}, {0.07, 0.08}};
        const double w[9] = {2, 0, 0, 0, 3, 0, 0, 0, 4};
        ceres::Problem problem;
        for (int c = 0; c < 2; ++c) {
            problem.AddParameterBlock(q[c], 4, new ceres::QuaternionRightPlus);
            problem.AddParameterBlock(t[c], 3);
        }
        if (variant == 3) problem.AddParameterBlock(lone, 3);
        int nb = 0;
        for (int c = 0; c < 2; ++c)
            for (int j = 0; j < 2; ++j) {
                problem.AddResidualBlock(ceres::ReprojectionFactor::Create(feat[c * 2 + j]), nullptr, q[c], t[c], Lm[j]);
                ++nb;
                if (variant == 1 && nb == 2) {       // (behind the second observation: both landmarks have been named)
                    problem.AddResidualBlock(ceres::LandmarkPriorFactor::Create(Lm[1], w), nullptr, Lm[1]);
                    problem.AddResidualBlock(ceres::LandmarkPriorFactor::Create(Lm[0]), nullptr, Lm[0]);
                }
                if (nb != 1) continue;               // (the other variants' block sits behind the first observation's)
                if (variant == 2) problem.AddResidualBlock(ceres::LandmarkPriorFactor::Create(Lm[0]), new ceres::HuberLoss(1.0), Lm[0]);
                if (variant == 3) problem.AddResidualBlock(ceres::LandmarkPriorFactor::Create(lone), nullptr, lone);
                if (variant == 4) problem.AddResidualBlock(ceres::LandmarkPriorFactor::Create(t[0]), nullptr, t[0]);
                if (variant == 5) {
                    problem.AddResidualBlock(ceres::LandmarkPriorFactor::Create(Lm[1]), nullptr, Lm[1]);   // (named only later: resolved behind the loop)
                    problem.AddResidualBlock(ceres::PosePriorFactor::Create(q[0], t[0]), nullptr, q[0], t[0]);
                }
            }
        if (variant == 1) problem.AddResidualBlock(ceres::LandmarkPriorFactor::Create(lone, w), nullptr, Lm[1]);
        ceres::internal::BaLayout L;
        bool ok = ceres::internal::DetectBa(problem, &L);
        if (ok && variant == 0) ok = L.obs_res.empty() && L.lp_pt.empty() && L.obs_cam.size() == 4;
        if (ok && variant == 1) {
            // four observations at residual blocks 0, 1, 4, 5 with their features in place; priors on landmarks 1, 0, 1 in that order
            ok = L.obs_cam.size() == 4 && L.obs_res == std::vector<int>({0, 1, 4, 5}) && L.lp_pt == std::vector<int>({1, 0, 1}) &&
                 L.lp_pos.size() == 9 && L.lp_w.size() == 27 && L.feat.size() == 8 && L.user.size() == 4 && L.prior_cam.empty();
            for (int i = 0; ok && i < 4; ++i) ok = L.feat[2 * i] == feat[i][0] && L.feat[2 * i + 1] == feat[i][1] && L.obs_cam[i] == i / 2 && L.obs_pt[i] == i % 2;
            for (int i = 0; ok && i < 9; ++i) ok = L.lp_w[i] == w[i] && L.lp_w[9 + i] == (i % 4 == 0 ? 1.0 : 0.0) && L.lp_w[18 + i] == w[i];
            for (int i = 0; ok && i < 3; ++i) ok = L.lp_pos[i] == Lm[1][i] && L.lp_pos[3 + i] == Lm[0][i] && L.lp_pos[6 + i] == lone[i];
        }
        if (ok && variant == 5) ok = L.lp_pt == std::vector<int>({1}) && L.prior_cam == std::vector<int>({0}) && L.obs_res == std::vector<int>({0, 3, 4, 5});
        detect[variant] = ok ? 1 : 0;
    }
    std::printf("detect %d %d %d %d %d %d\n", detect[0], detect[1], detect[2], detect[3], detect[4], detect[5]);
    // the route decision (no device work: SolveDispatch's own first two calls), one "route <variant> <option> <stage> <path>" line each.
    // Variants: lp -- built-in factors and a landmark prior; loss -- the prior block carries a loss; user -- the observations are a user's
    // cost functions that are NOT the reprojection factor (shape only: "gpu-ba-hostjac" without the prior) and a landmark prior
    struct Doubled : ceres::SizedCostFunction<2, 4, 3, 3> {
        ceres::ReprojectionFactor f;
        explicit Doubled(const double* feat) : f(feat[0], feat[1]) {}
        bool Evaluate(double const* const* p, double* r, double** J) const override {
            if (!f.Evaluate(p, r, J)) return false;
            r[0] *= 2; r[1] *= 2;
            const int n[3] = {8, 6, 6};
            if (J) for (int b = 0; b < 3; ++b) if (J[b]) for (int i = 0; i < n[b]; ++i) J[b][i] *= 2;
            return true;
        }
    };
    for (const char* variant : {"lp", "loss", "user", "user_plain"})
        for (const char* option : {"default", "iterative", "dogleg", "inner"}) {
            double q[2][4] = {{0, 0, 0, 1}, {0, 0.1, 0, 0.99498743710662}}, t[2][3] = {{0, 0, 0}, {1, 0, 0}};
            double Lm[2][3] = {{0.1, 0.2, 4}, {-0.3, 0.1, 5}};
            const double feat[4][2] = {{0.01, 0.02}, {0.03, 0.04}, {0.05, 0.06}, {0.07, 0.08}};
            const std::string v = variant, opt = option;
            ceres::Problem problem;
            for (int c = 0; c < 2; ++c) {
                problem.AddParameterBlock(q[c], 4, new ceres::QuaternionRightPlus);
                problem.AddParameterBlock(t[c], 3);
            }
            for (int c = 0; c < 2; ++c)
                for (int j = 0; j < 2; ++j) {
                    if (v == "user" || v == "user_plain") problem.AddResidualBlock(new Doubled(feat[c * 2 + j]), nullptr, q[c], t[c], Lm[j]);
                    else problem.AddResidualBlock(ceres::ReprojectionFactor::Create(feat[c * 2 + j]), nullptr, q[c], t[c], Lm[j]);
                }
            if (v != "user_plain")
                problem.AddResidualBlock(ceres::LandmarkPriorFactor::Create(Lm[0]), v == "loss" ? new ceres::HuberLoss(1.0) : nullptr, Lm[0]);
            ceres::Solver::Options o;
            o.num_threads = 1;
            if (opt == "iterative") o.linear_solver_type = ceres::ITERATIVE_SCHUR;
            if (opt == "dogleg") o.trust_region_strategy_type = ceres::DOGLEG;
            if (opt == "inner") o.use_inner_iterations = true;
            ceres::internal::Recognition r;
            ceres::internal::Recognise(problem, false, o.bundle_adjustment_losses && !o.use_inner_iterations, o.num_threads, &r);
            ceres::internal::InnerGroups inner;
            const ceres::internal::Decision d = ceres::internal::DecideSolve(o, r, &inner);
            std::printf("route %s %s %d %s | %s\n", variant, option, (int)d.stage, d.stage == ceres::internal::Decision::GO ? ceres::internal::RouteName(d.route) : "-",
                        d.why.c_str());
        }
    return 0;
}
