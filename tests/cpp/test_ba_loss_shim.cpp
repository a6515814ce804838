// Solver::Options::bundle_adjustment_losses / Covariance::Options::bundle_adjustment_losses of include/stba/ceres.h, for
// tests/test_ba_loss_shim.py (host mode, no device) and tests/test_gpu_ba_loss_shim.py:
//   test_ba_loss_shim host   -- what is let through and what is refused, before any device work: a bundle-adjustment problem of
//       ReprojectionFactors whose blocks mix built-in losses, a ScaledLoss and no loss is let through with the option set (and its
//       per-observation table is the expected one) and refused without it; with the option set a user subclass, a ScaledLoss around a
//       ScaledLoss, inner iterations, the forced callback path, a BA-shaped problem of another factor ("gpu-ba-hostjac") and a dense
//       problem are refused by Solve and by Covariance::Compute with the "LossFunction ... not implemented" message, parameters untouched
//   test_ba_loss_shim device <file>  -- the scene of <file>: nc np no n_cam_pairs n_pts | nc x 7 cameras | nc fixed flags | np x 3 landmarks |
//       no x (camera landmark fx fy) | no x (kind a b scale; kind -1: no loss if scale is 1, else ScaledLoss(nullptr, scale)) |
//       n_cam_pairs x (a b) | n_pts landmark indices.  ceres::Solve with the option set, then ceres::Covariance at the solution.
//       Prints "ba path <execution_path> term <t> iters <k> initial <c0> final <c>", "ba_cams ...", "ba_pts ...", "cov path ...", a
//       "R" / "P" line per camera pair (rotation | position 3 x 3 block) and an "L" line per landmark.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "stba/ceres.h"
namespace ceres = stba_ceres;

static ceres::LossFunction* MakeLoss(int kind, double a, double b, double scale) {
    ceres::LossFunction* inner = nullptr;
    switch (kind) {
    case STBA_LOSS_TRIVIAL: inner = new ceres::TrivialLoss(); break;
    case STBA_LOSS_HUBER: inner = new ceres::HuberLoss(a); break;
    case STBA_LOSS_SOFTLONE: inner = new ceres::SoftLOneLoss(a); break;
    case STBA_LOSS_CAUCHY: inner = new ceres::CauchyLoss(a); break;
    case STBA_LOSS_ARCTAN: inner = new ceres::ArctanLoss(a); break;
    case STBA_LOSS_TOLERANT: inner = new ceres::TolerantLoss(a, b); break;
    case STBA_LOSS_TUKEY: inner = new ceres::TukeyLoss(a); break;
    default: break;
    }
    if (scale != 1.0 || !inner) return new ceres::ScaledLoss(inner, scale, ceres::TAKE_OWNERSHIP);
    return inner;
}

struct UserLoss : ceres::LossFunction {};

// BA-shaped ({4, 3, 3} -> 2) but not the reprojection factor: twice its residual
struct TwiceReprojection : ceres::SizedCostFunction<2, 4, 3, 3> {
    ceres::ReprojectionFactor inner;
    TwiceReprojection(double fx, double fy) : inner(fx, fy) {}
    bool Evaluate(double const* const* p, double* r, double** J) const override {
        if (!inner.Evaluate(p, r, J)) return false;
        r[0] *= 2.0; r[1] *= 2.0;
        const int sizes[3] = {4, 3, 3};
        if (J) for (int k = 0; k < 3; ++k) if (J[k]) for (int q = 0; q < 2 * sizes[k]; ++q) J[k][q] *= 2.0;
        return true;
    }
};

// two cameras, two landmarks, four observations; block k gets losses[k] (nullptr: none)
struct Small {
    double q[8] = {0, 0, 0, 1, 0, 0, 0, 1}, t[6] = {0, 0, 0, 1, 0, 0}, lm[6] = {0.1, 0.2, 4.0, -0.3, 0.1, 5.0};
    ceres::Problem problem;
    Small(const std::vector<ceres::LossFunction*>& losses, bool twice) {
        for (int c = 0; c < 2; ++c) problem.AddParameterBlock(&q[4 * c], 4, new ceres::QuaternionRightPlus());
        int k = 0;
        for (int c = 0; c < 2; ++c)
            for (int l = 0; l < 2; ++l, ++k) {
                ceres::CostFunction* f = twice ? static_cast<ceres::CostFunction*>(new TwiceReprojection(0.01 * c, 0.02 * l))
                                               : static_cast<ceres::CostFunction*>(new ceres::ReprojectionFactor(0.01 * c, 0.02 * l));
                problem.AddResidualBlock(f, losses[(size_t)k], &q[4 * c], &t[3 * c], &lm[3 * l]);
            }
        problem.SetParameterBlockConstant(&q[0]);
        problem.SetParameterBlockConstant(&t[0]);
    }
    bool Untouched() const {
        const Small ref({nullptr, nullptr, nullptr, nullptr}, false);
        return std::memcmp(q, ref.q, sizeof q) == 0 && std::memcmp(t, ref.t, sizeof t) == 0 && std::memcmp(lm, ref.lm, sizeof lm) == 0;
    }
};

static bool RefusedMessage(const std::string& m) { return m.find("LossFunction") != std::string::npos && m.find("not implemented") != std::string::npos; }

static bool Refused(const char* what, Small& s, ceres::Solver::Options options, bool cov_option) {
    ceres::Solver::Summary summary;
    ceres::Solve(options, &s.problem, &summary);
    bool ok = summary.termination_type == ceres::FAILURE && RefusedMessage(summary.message) && s.Untouched() && summary.execution_path.empty();
    ceres::Covariance::Options co;
    co.bundle_adjustment_losses = cov_option;
    ceres::Covariance cov{co};
    ok = ok && !cov.Compute({{&s.q[4], &s.q[4]}}, &s.problem) && RefusedMessage(cov.message()) && cov.execution_path().empty();
    std::printf("%s: %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED");
    return ok;
}

static int Host() {
    bool ok = true;
    ceres::Solver::Options on;
    on.bundle_adjustment_losses = true;
    {   // the table of a mixed problem: none | Huber(0.5) | ScaledLoss(Cauchy(2), 3) | Tolerant(0.3, 0.02)
        Small s({nullptr, new ceres::HuberLoss(0.5), new ceres::ScaledLoss(new ceres::CauchyLoss(2.0), 3.0, ceres::TAKE_OWNERSHIP), new ceres::TolerantLoss(0.3, 0.02)}, false);
        ceres::internal::BaLayout L;
        if (!ceres::internal::BaWithKnownLosses(&s.problem, 1, &L)) { std::printf("the problem or its losses were not recognised\n"); return 1; }
        const int kind[4] = {STBA_LOSS_TRIVIAL, STBA_LOSS_HUBER, STBA_LOSS_CAUCHY, STBA_LOSS_TOLERANT};
        const double a[4] = {1.0, 0.5, 2.0, 0.3}, b[4] = {1.0, 1.0, 1.0, 0.02}, sc[4] = {1.0, 1.0, 3.0, 1.0};
        const int oc[4] = {0, 0, 1, 1}, op[4] = {0, 1, 0, 1};
        if (L.loss_kind.size() != 4 || L.obs_cam.size() != 4) { std::printf("table has %zu rows\n", L.loss_kind.size()); return 1; }
        for (int e = 0; e < 4; ++e)
            if (L.loss_kind[e] != kind[e] || L.loss_a[e] != a[e] || L.loss_b[e] != b[e] || L.loss_scale[e] != sc[e] || L.obs_cam[e] != oc[e] || L.obs_pt[e] != op[e]) {
                std::printf("table row %d is wrong\n", e); ok = false;
            }
        if (!ceres::internal::LossesGoToBa(on, &s.problem)) { std::printf("a bundle adjustment of built-in losses was not let through with the option set\n"); ok = false; }
        if (ceres::internal::LossesGoToBa(ceres::Solver::Options(), &s.problem)) { std::printf("let through without the option\n"); ok = false; }
        if (ok) std::printf("option set: let through, table of 4 rows\n");
        ok = Refused("option unset", s, ceres::Solver::Options(), false) && ok;
        ceres::Solver::Options inner = on;
        inner.use_inner_iterations = true;
        ok = Refused("option set, inner iterations", s, inner, false) && ok;
        ceres::Solver::Options forced = on;
        forced.force_callback_path = true;
        ok = Refused("option set, callback path forced", s, forced, false) && ok;
        Small plain({nullptr, nullptr, nullptr, nullptr}, false);
        ceres::internal::BaLayout L0;
        if (!ceres::internal::BaWithKnownLosses(&plain.problem, 1, &L0) || !L0.loss_kind.empty()) { std::printf("a table without a loss\n"); ok = false; }
    }
    {
        Small s({nullptr, new UserLoss(), nullptr, nullptr}, false);
        ok = Refused("option set, user subclass", s, on, true) && ok;
    }
    {
        Small s({nullptr, nullptr, nullptr, new ceres::ScaledLoss(new ceres::ScaledLoss(new ceres::HuberLoss(1.0), 2.0, ceres::TAKE_OWNERSHIP), 2.0, ceres::TAKE_OWNERSHIP)}, false);
        ok = Refused("option set, ScaledLoss around a ScaledLoss", s, on, true) && ok;
    }
    {
        Small s({nullptr, new ceres::HuberLoss(0.5), nullptr, nullptr}, true);
        ok = Refused("option set, another factor (gpu-ba-hostjac)", s, on, true) && ok;
    }
    {   // a built-in loss on a dense problem
        struct Line : ceres::SizedCostFunction<1, 1> {
            bool Evaluate(double const* const* p, double* r, double** J) const override { r[0] = p[0][0] - 2.0; if (J && J[0]) J[0][0] = 1.0; return true; }
        };
        double x = 0.5;
        ceres::Problem p;
        p.AddResidualBlock(new Line(), new ceres::CauchyLoss(1.0), &x);
        ceres::Solver::Summary summary;
        ceres::Solve(on, &p, &summary);
        ceres::Covariance::Options co;
        co.bundle_adjustment_losses = true;
        ceres::Covariance cov{co};
        const bool r = summary.termination_type == ceres::FAILURE && RefusedMessage(summary.message) && x == 0.5 && !cov.Compute({{&x, &x}}, &p) && RefusedMessage(cov.message());
        std::printf("option set, dense problem: %s\n", r ? "refused" : "NOT REFUSED AS EXPECTED");
        ok = ok && r;
    }
    if (ok) std::printf("host ok\n");
    return ok ? 0 : 1;
}

static int Device(const char* file) {
    std::ifstream in(file);
    int nc = 0, np = 0, no = 0, ncp = 0, nlp = 0;
    if (!(in >> nc >> np >> no >> ncp >> nlp)) return 2;
    std::vector<double> cams((size_t)nc * 7), pts((size_t)np * 3), fx((size_t)no), fy((size_t)no), la((size_t)no), lb((size_t)no), ls((size_t)no);
    std::vector<int> fixed((size_t)nc), oc((size_t)no), op((size_t)no), kind((size_t)no), pa((size_t)ncp), pb((size_t)ncp), lp((size_t)nlp);
    for (auto& v : cams) in >> v;
    for (auto& v : fixed) in >> v;
    for (auto& v : pts) in >> v;
    for (int k = 0; k < no; ++k) in >> oc[k] >> op[k] >> fx[k] >> fy[k];
    for (int k = 0; k < no; ++k) in >> kind[k] >> la[k] >> lb[k] >> ls[k];
    for (int k = 0; k < ncp; ++k) in >> pa[k] >> pb[k];
    for (auto& v : lp) in >> v;
    if (!in) return 2;
    // (quaternion and position of a camera are separate blocks: [qx qy qz qw] and [tx ty tz])
    std::vector<double> q((size_t)nc * 4), t((size_t)nc * 3);
    for (int c = 0; c < nc; ++c) { std::memcpy(&q[4 * (size_t)c], &cams[7 * (size_t)c], 4 * sizeof(double)); std::memcpy(&t[3 * (size_t)c], &cams[7 * (size_t)c + 4], 3 * sizeof(double)); }
    ceres::Problem problem;
    for (int c = 0; c < nc; ++c) problem.AddParameterBlock(&q[4 * (size_t)c], 4, new ceres::QuaternionRightPlus());
    for (int k = 0; k < no; ++k)
        problem.AddResidualBlock(new ceres::ReprojectionFactor(fx[k], fy[k]), (kind[k] < 0 && ls[k] == 1.0) ? nullptr : MakeLoss(kind[k], la[k], lb[k], ls[k]),
                                 &q[4 * (size_t)oc[k]], &t[3 * (size_t)oc[k]], &pts[3 * (size_t)op[k]]);
    for (int c = 0; c < nc; ++c) if (fixed[c]) { problem.SetParameterBlockConstant(&q[4 * (size_t)c]); problem.SetParameterBlockConstant(&t[3 * (size_t)c]); }
    ceres::Solver::Options options;
    options.num_threads = 1;
    options.bundle_adjustment_losses = true;
    ceres::Solver::Summary summary;
    ceres::Solve(options, &problem, &summary);
    std::printf("ba path %s term %d iters %d initial %.17g final %.17g\n", summary.execution_path.c_str(), (int)summary.termination_type,
                (int)summary.iterations.size() - 1, summary.initial_cost, summary.final_cost);
    if (summary.termination_type != ceres::CONVERGENCE) { std::printf("ba message %s\n", summary.message.c_str()); return 1; }
    std::printf("ba_cams");
    for (int c = 0; c < nc; ++c) { for (int k = 0; k < 4; ++k) std::printf(" %.17g", q[4 * (size_t)c + k]); for (int k = 0; k < 3; ++k) std::printf(" %.17g", t[3 * (size_t)c + k]); }
    std::printf("\nba_pts");
    for (double v : pts) std::printf(" %.17g", v);
    std::printf("\n");
    std::vector<std::pair<const double*, const double*>> pairs;
    for (int k = 0; k < ncp; ++k) { pairs.push_back({&q[4 * (size_t)pa[k]], &q[4 * (size_t)pb[k]]}); pairs.push_back({&t[3 * (size_t)pa[k]], &t[3 * (size_t)pb[k]]}); }
    for (int k = 0; k < nlp; ++k) pairs.push_back({&pts[3 * (size_t)lp[k]], &pts[3 * (size_t)lp[k]]});
    ceres::Covariance::Options co;
    co.bundle_adjustment_losses = true;
    ceres::Covariance cov{co};
    const bool ok = cov.Compute(pairs, &problem);
    std::printf("cov path %s\n", cov.execution_path().c_str());
    if (!ok) { std::printf("covariance failed: %s\n", cov.message().c_str()); return 1; }
    for (size_t k = 0; k < pairs.size(); ++k) {
        double b[9];
        if (!cov.GetCovarianceBlockInTangentSpace(pairs[k].first, pairs[k].second, b)) return 1;
        const bool cam = k < 2 * (size_t)ncp;
        std::printf("%s %d", cam ? (k % 2 ? "P" : "R") : "L", cam ? (int)(k / 2) : (int)(k - 2 * (size_t)ncp));
        for (int e = 0; e < 9; ++e) std::printf(" %.17g", b[e]);
        std::printf("\n");
    }
    std::printf("device ok\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "host") return Host();
    if (mode == "device" && argc > 2) return Device(argv[2]);
    std::fprintf(stderr, "usage: test_ba_loss_shim host | device <file>\n");
    return 2;
}
