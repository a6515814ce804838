// The loss classes of include/stba/ceres.h, for tests/test_pg_loss_shim.py / test_pg_loss_cpu.py (host modes, no device) and
// tests/test_gpu_pg_loss_shim.py:
//   test_pg_loss_shim eval <kind> <a> <b> <scale> <s>...  -- rho, rho', rho'' of the class of STBA_LOSS_* <kind> at every s, one line
//       "E <s> <rho> <rho'> <rho''>" each; scale != 1: through ScaledLoss(inner, scale, TAKE_OWNERSHIP); kind -1: ScaledLoss(nullptr, scale)
//   test_pg_loss_shim host   -- what is let through and what is refused, before any device work: the per-edge table of a pose graph whose
//       blocks mix built-in losses, a ScaledLoss and no loss; a user subclass, a bare LossFunction and a ScaledLoss around a
//       ScaledLoss on a pose graph; a built-in loss on a bundle-adjustment problem, on a dense problem and on a pose graph sent down
//       the callback path -- each refused by Solve and by Covariance::Compute with the "LossFunction ... not implemented" message,
//       parameters untouched
//   test_pg_loss_shim device <file>  -- the graph of <file>: n m n_pairs | n x 7 poses | n fixed flags | m x (i j) | m x 7 measurements |
//       m x (kind a b scale; kind -1: the block gets no loss if scale is 1, else ScaledLoss(nullptr, scale)) | n_pairs x (a b).  ceres::Solve, then ceres::Covariance at the solution.
//       Prints "pg path <execution_path> term <t> iters <k> initial <c0> final <c>", "pg_poses ...", "cov path ..." and a "T" line per pair.
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

static void EvaluateAny(const ceres::LossFunction* l, double s, double rho[3]) {
    if (auto* p = dynamic_cast<const ceres::TrivialLoss*>(l)) p->Evaluate(s, rho);
    else if (auto* p = dynamic_cast<const ceres::HuberLoss*>(l)) p->Evaluate(s, rho);
    else if (auto* p = dynamic_cast<const ceres::SoftLOneLoss*>(l)) p->Evaluate(s, rho);
    else if (auto* p = dynamic_cast<const ceres::CauchyLoss*>(l)) p->Evaluate(s, rho);
    else if (auto* p = dynamic_cast<const ceres::ArctanLoss*>(l)) p->Evaluate(s, rho);
    else if (auto* p = dynamic_cast<const ceres::TolerantLoss*>(l)) p->Evaluate(s, rho);
    else if (auto* p = dynamic_cast<const ceres::TukeyLoss*>(l)) p->Evaluate(s, rho);
    else if (auto* p = dynamic_cast<const ceres::ScaledLoss*>(l)) p->Evaluate(s, rho);
    else rho[0] = rho[1] = rho[2] = NAN;
}

static int Eval(int argc, char** argv) {
    const int kind = std::atoi(argv[2]);
    const double a = std::strtod(argv[3], nullptr), b = std::strtod(argv[4], nullptr), scale = std::strtod(argv[5], nullptr);
    ceres::LossFunction* l = MakeLoss(kind, a, b, scale);
    for (int k = 6; k < argc; ++k) {
        const double s = std::strtod(argv[k], nullptr);
        double rho[3];
        EvaluateAny(l, s, rho);
        std::printf("E %.17g %.17g %.17g %.17g\n", s, rho[0], rho[1], rho[2]);
    }
    delete l;
    return 0;
}

struct UserLoss : ceres::LossFunction {};

// a chain of four edges over five poses; block e gets losses[e] (nullptr: none)
struct Chain {
    std::vector<double> poses;
    ceres::Problem problem;
    explicit Chain(const std::vector<ceres::LossFunction*>& losses) {
        const double z[7] = {0.05, -0.02, 0.03, 0.9979, 0.4, -0.1, 0.2};
        for (int k = 0; k < 5; ++k) { const double p[7] = {0, 0, 0, 1, 0.5 * k, 0, 0}; poses.insert(poses.end(), p, p + 7); }
        for (int k = 0; k < 5; ++k) problem.AddParameterBlock(&poses[7 * k], 7, new ceres::SE3RightPlus());
        for (int e = 0; e < 4; ++e) problem.AddResidualBlock(ceres::RelativePoseFactor::Create(z), losses[e], {&poses[7 * e], &poses[7 * (e + 1)]});
        problem.SetParameterBlockConstant(&poses[0]);
    }
};

static bool RefusedMessage(const std::string& m) { return m.find("LossFunction") != std::string::npos && m.find("not implemented") != std::string::npos; }

static bool ChainRefused(const char* what, const std::vector<ceres::LossFunction*>& losses, bool force_callback) {
    Chain c(losses);
    const std::vector<double> before = c.poses;
    ceres::Solver::Options options;
    options.force_callback_path = force_callback;
    ceres::Solver::Summary summary;
    ceres::Solve(options, &c.problem, &summary);
    bool ok = summary.termination_type == ceres::FAILURE && RefusedMessage(summary.message) && c.poses == before && summary.execution_path.empty();
    if (!force_callback) {
        ceres::Covariance cov{ceres::Covariance::Options()};
        ok = ok && !cov.Compute({{&c.poses[7], &c.poses[7]}}, &c.problem) && RefusedMessage(cov.message()) && cov.execution_path().empty();
    }
    std::printf("%s: %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED");
    return ok;
}

static int Host() {
    bool ok = true;
    {   // the table of a mixed problem: none | Huber(0.5) | ScaledLoss(Cauchy(2), 3) | Tolerant(0.3, 0.02)
        Chain c({nullptr, new ceres::HuberLoss(0.5), new ceres::ScaledLoss(new ceres::CauchyLoss(2.0), 3.0, ceres::TAKE_OWNERSHIP), new ceres::TolerantLoss(0.3, 0.02)});
        ceres::internal::PoseGraphLayout L;
        if (!ceres::internal::DetectPoseGraph(&c.problem, &L) || !L.losses_known) { std::printf("the graph or its losses were not recognised\n"); return 1; }
        const int kind[4] = {STBA_LOSS_TRIVIAL, STBA_LOSS_HUBER, STBA_LOSS_CAUCHY, STBA_LOSS_TOLERANT};
        const double a[4] = {1.0, 0.5, 2.0, 0.3}, b[4] = {1.0, 1.0, 1.0, 0.02}, sc[4] = {1.0, 1.0, 3.0, 1.0};
        if (L.loss_kind.size() != 4) { std::printf("table has %zu rows\n", L.loss_kind.size()); return 1; }
        for (int e = 0; e < 4; ++e)
            if (L.loss_kind[e] != kind[e] || L.loss_a[e] != a[e] || L.loss_b[e] != b[e] || L.loss_scale[e] != sc[e]) { std::printf("table row %d is wrong\n", e); ok = false; }
        if (c.problem.NumLossFunctions() != 3) ok = false;
        if (!ceres::internal::LossesGoToPoseGraph(ceres::Solver::Options(), &c.problem)) { std::printf("a pose graph of built-in losses was not let through\n"); ok = false; }
        Chain plain({nullptr, nullptr, nullptr, nullptr});
        ceres::internal::PoseGraphLayout L0;
        if (!ceres::internal::DetectPoseGraph(&plain.problem, &L0) || !L0.loss_kind.empty()) { std::printf("a table without a loss\n"); ok = false; }
        Chain scaled_null({new ceres::ScaledLoss(nullptr, 2.5, ceres::TAKE_OWNERSHIP), nullptr, nullptr, nullptr});
        ceres::internal::PoseGraphLayout L1;
        if (!ceres::internal::DetectPoseGraph(&scaled_null.problem, &L1) || !L1.losses_known || L1.loss_kind[0] != STBA_LOSS_TRIVIAL || L1.loss_scale[0] != 2.5) ok = false;
    }
    ok = ChainRefused("user subclass on a pose graph", {nullptr, new UserLoss(), nullptr, nullptr}, false) && ok;
    ok = ChainRefused("bare LossFunction on a pose graph", {new ceres::LossFunction(), nullptr, nullptr, nullptr}, false) && ok;
    ok = ChainRefused("ScaledLoss around a ScaledLoss", {nullptr, nullptr, nullptr,
                      new ceres::ScaledLoss(new ceres::ScaledLoss(new ceres::HuberLoss(1.0), 2.0, ceres::TAKE_OWNERSHIP), 2.0, ceres::TAKE_OWNERSHIP)}, false) && ok;
    ok = ChainRefused("ScaledLoss around a user subclass", {new ceres::ScaledLoss(new UserLoss(), 2.0, ceres::TAKE_OWNERSHIP), nullptr, nullptr, nullptr}, false) && ok;
    ok = ChainRefused("built-in loss, callback path forced", {new ceres::HuberLoss(0.5), nullptr, nullptr, nullptr}, true) && ok;
    {   // a built-in loss on a bundle-adjustment problem
        double q[8] = {0, 0, 0, 1, 0, 0, 0, 1}, t[6] = {0, 0, 0, 1, 0, 0}, Lm[6] = {0.1, 0.2, 4.0, -0.3, 0.1, 5.0};
        const double q0[8] = {0, 0, 0, 1, 0, 0, 0, 1};
        ceres::Problem p;
        for (int c = 0; c < 2; ++c) p.AddParameterBlock(&q[4 * c], 4, new ceres::QuaternionRightPlus());
        for (int c = 0; c < 2; ++c)
            for (int l = 0; l < 2; ++l)
                p.AddResidualBlock(new ceres::ReprojectionFactor(0.01 * c, 0.02 * l), (c == 1 && l == 0) ? new ceres::HuberLoss(1.0) : nullptr, &q[4 * c], &t[3 * c], &Lm[3 * l]);
        ceres::Solver::Options options;
        ceres::Solver::Summary summary;
        ceres::Solve(options, &p, &summary);
        ceres::Covariance cov{ceres::Covariance::Options()};
        const bool r = summary.termination_type == ceres::FAILURE && RefusedMessage(summary.message) && std::memcmp(q, q0, sizeof q) == 0 && Lm[2] == 4.0 &&
                       !cov.Compute({{&q[4], &q[4]}}, &p) && RefusedMessage(cov.message());
        std::printf("built-in loss on a bundle-adjustment problem: %s\n", r ? "refused" : "NOT REFUSED AS EXPECTED");
        ok = ok && r;
    }
    {   // a built-in loss on a dense problem
        struct Line : ceres::SizedCostFunction<1, 1> {
            bool Evaluate(double const* const* p, double* r, double** J) const override { r[0] = p[0][0] - 2.0; if (J && J[0]) J[0][0] = 1.0; return true; }
        };
        double x = 0.5;
        ceres::Problem p;
        p.AddResidualBlock(new Line(), new ceres::CauchyLoss(1.0), &x);
        ceres::Solver::Options options;
        ceres::Solver::Summary summary;
        ceres::Solve(options, &p, &summary);
        ceres::Covariance cov{ceres::Covariance::Options()};
        const bool r = summary.termination_type == ceres::FAILURE && RefusedMessage(summary.message) && x == 0.5 && !cov.Compute({{&x, &x}}, &p) && RefusedMessage(cov.message());
        std::printf("built-in loss on a dense problem: %s\n", r ? "refused" : "NOT REFUSED AS EXPECTED");
        ok = ok && r;
    }
    if (ok) std::printf("host ok\n");
    return ok ? 0 : 1;
}

static int Device(const char* file) {
    std::ifstream in(file);
    int n = 0, m = 0, np = 0;
    if (!(in >> n >> m >> np)) return 2;
    std::vector<double> poses((size_t)n * 7), meas((size_t)m * 7), la((size_t)m), lb((size_t)m), ls((size_t)m);
    std::vector<int> fixed((size_t)n), ei((size_t)m), ej((size_t)m), kind((size_t)m), pa((size_t)np), pb((size_t)np);
    for (auto& v : poses) in >> v;
    for (auto& v : fixed) in >> v;
    for (int e = 0; e < m; ++e) in >> ei[e] >> ej[e];
    for (auto& v : meas) in >> v;
    for (int e = 0; e < m; ++e) in >> kind[e] >> la[e] >> lb[e] >> ls[e];
    for (int k = 0; k < np; ++k) in >> pa[k] >> pb[k];
    if (!in) return 2;
    ceres::Problem problem;
    for (int k = 0; k < n; ++k) problem.AddParameterBlock(&poses[7 * (size_t)k], 7, new ceres::SE3RightPlus());
    for (int e = 0; e < m; ++e)
        problem.AddResidualBlock(ceres::RelativePoseFactor::Create(&meas[7 * (size_t)e]), (kind[e] < 0 && ls[e] == 1.0) ? nullptr : MakeLoss(kind[e], la[e], lb[e], ls[e]),
                                 {&poses[7 * (size_t)ei[e]], &poses[7 * (size_t)ej[e]]});
    for (int k = 0; k < n; ++k) if (fixed[k]) problem.SetParameterBlockConstant(&poses[7 * (size_t)k]);
    ceres::Solver::Options options;
    options.num_threads = 1;
    options.function_tolerance = 1e-12;
    options.parameter_tolerance = 1e-11;
    ceres::Solver::Summary summary;
    ceres::Solve(options, &problem, &summary);
    std::printf("pg path %s term %d iters %d initial %.17g final %.17g\n", summary.execution_path.c_str(), (int)summary.termination_type,
                (int)summary.iterations.size() - 1, summary.initial_cost, summary.final_cost);
    if (summary.termination_type != ceres::CONVERGENCE) { std::printf("pg message %s\n", summary.message.c_str()); return 1; }
    std::printf("pg_poses");
    for (double v : poses) std::printf(" %.17g", v);
    std::printf("\n");
    std::vector<std::pair<const double*, const double*>> pairs;
    for (int k = 0; k < np; ++k) pairs.push_back({&poses[7 * (size_t)pa[k]], &poses[7 * (size_t)pb[k]]});
    ceres::Covariance cov{ceres::Covariance::Options()};
    const bool ok = cov.Compute(pairs, &problem);
    std::printf("cov path %s\n", cov.execution_path().c_str());
    if (!ok) { std::printf("covariance failed: %s\n", cov.message().c_str()); return 1; }
    for (int k = 0; k < np; ++k) {
        double t[36];
        if (!cov.GetCovarianceBlockInTangentSpace(pairs[k].first, pairs[k].second, t)) return 1;
        std::printf("T %d", k);
        for (int q = 0; q < 36; ++q) std::printf(" %.17g", t[q]);
        std::printf("\n");
    }
    std::printf("device ok\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "eval" && argc > 6) return Eval(argc, argv);
    if (mode == "host") return Host();
    if (mode == "device" && argc > 2) return Device(argv[2]);
    std::fprintf(stderr, "usage: test_pg_loss_shim eval <kind> <a> <b> <scale> <s>... | host | device <file>\n");
    return 2;
}
