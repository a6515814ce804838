// ReprojectionFactor::Create(feature, sqrt_information) of include/stba/ceres.h, for tests/test_ba_information_shim_cpu.py (host mode,
// no device) and tests/test_gpu_ba_information_shim.py:
//   test_ba_information_shim host   -- the factory and the accessor; the weighted factor's Evaluate is W times the unweighted one's
//       (residual and the three Jacobian blocks); DetectBa gathers the W of a mixed problem (the identity for a factor made without one)
//       and nothing for a problem without weighted factors; use_inner_iterations with a weighted factor is refused with a message,
//       parameters untouched, before any device work
//   test_ba_information_shim device <file> [callback]  -- the scene of <file>: nc np no n_cam_pairs n_pts | nc x 7 cameras | nc fixed flags |
//       np x 3 landmarks | no x (camera landmark fx fy) | no x (kind a b scale; kind -1: no loss if scale is 1) | no x (has_w w00 w01 w10 w11) |
//       n_cam_pairs x (a b) | n_pts landmark indices.  ceres::Solve (bundle_adjustment_losses set; "callback": force_callback_path), then
//       ceres::Covariance at the solution.  Prints "ba path <execution_path> term <t> iters <k> initial <c0> final <c>", "ba_cams ...",
//       "ba_pts ...", "cov path ...", an "R" / "P" line per camera pair (rotation | position 3 x 3 block) and an "L" line per landmark.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "stba/ceres.h"
namespace ceres = stba_ceres;

static ceres::LossFunction* MakeLoss(int kind, double a, double scale) {
    ceres::LossFunction* inner = nullptr;
    if (kind == STBA_LOSS_HUBER) inner = new ceres::HuberLoss(a);
    else if (kind == STBA_LOSS_CAUCHY) inner = new ceres::CauchyLoss(a);
    if (scale != 1.0 || !inner) return new ceres::ScaledLoss(inner, scale, ceres::TAKE_OWNERSHIP);
    return inner;
}

// two cameras, two landmarks, four observations; block k is weighted by W[k] if weighted[k]
struct Small {
    double q[8] = {0.01, -0.02, 0.03, 1, 0, 0, 0, 1}, t[6] = {0, 0, 0, 1, 0, 0}, lm[6] = {0.1, 0.2, 4.0, -0.3, 0.1, 5.0};
    ceres::Problem problem;
    Small(const bool* weighted, const double (*W)[4]) {
        for (int c = 0; c < 2; ++c) problem.AddParameterBlock(&q[4 * c], 4, new ceres::QuaternionRightPlus());
        int k = 0;
        for (int c = 0; c < 2; ++c)
            for (int l = 0; l < 2; ++l, ++k) {
                const double f[2] = {0.01 * c, 0.02 * l};
                problem.AddResidualBlock(weighted[k] ? ceres::ReprojectionFactor::Create(f, W[k]) : ceres::ReprojectionFactor::Create(f), nullptr,
                                         &q[4 * c], &t[3 * c], &lm[3 * l]);
            }
        problem.SetParameterBlockConstant(&q[0]);
        problem.SetParameterBlockConstant(&t[0]);
    }
};

static int Host() {
    bool ok = true;
    const double W[4][4] = {{2.0, 0.5, -0.25, 3.0}, {1.0, 0.0, 0.0, 1.0}, {0.7, 0.1, 0.2, 1.3}, {4.0, 0.0, 0.0, 4.0}};
    {   // the factory, the accessor, Evaluate
        const double f[2] = {0.03, -0.02};
        ceres::ReprojectionFactor* plain = ceres::ReprojectionFactor::Create(f);
        ceres::ReprojectionFactor* wf = ceres::ReprojectionFactor::Create(f, W[0]);
        if (plain->sqrt_information() != nullptr) { std::printf("a factor made without weights has some\n"); ok = false; }
        if (!wf->sqrt_information() || std::memcmp(wf->sqrt_information(), W[0], sizeof W[0]) != 0) { std::printf("sqrt_information() is not what Create got\n"); ok = false; }
        if (wf->fx() != f[0] || wf->fy() != f[1]) { std::printf("the feature is wrong\n"); ok = false; }
        const double q[4] = {0.05, -0.1, 0.02, 0.99}, t[3] = {0.1, -0.2, 0.3}, L[3] = {0.4, 0.5, 3.0};
        const double* p[3] = {q, t, L};
        double r0[2], r1[2], r2[2], j0[3][8], j1[3][8];
        double* J0[3] = {j0[0], j0[1], j0[2]};
        double* J1[3] = {j1[0], j1[1], j1[2]};
        plain->Evaluate(p, r0, J0);
        wf->Evaluate(p, r1, J1);
        wf->Evaluate(p, r2, nullptr);
        const int sizes[3] = {4, 3, 3};
        double worst = 0.0;
        auto cmp = [&](double got, double a, double b, int row) {
            const double want = W[0][2 * row] * a + W[0][2 * row + 1] * b;
            worst = std::fmax(worst, std::fabs(got - want) / (std::fabs(W[0][2 * row] * a) + std::fabs(W[0][2 * row + 1] * b) + 1e-300));
        };
        for (int row = 0; row < 2; ++row) {
            cmp(r1[row], r0[0], r0[1], row);
            cmp(r2[row], r0[0], r0[1], row);
            for (int b = 0; b < 3; ++b) for (int k = 0; k < sizes[b]; ++k) cmp(J1[b][row * sizes[b] + k], J0[b][k], J0[b][sizes[b] + k], row);
        }
        std::printf("weighted Evaluate against W x the unweighted one: worst relative difference %.3e\n", worst);
        if (!(worst <= 4 * 2.220446049250313e-16)) ok = false;
        if (r1[0] == r0[0]) { std::printf("the weighted residual is the unweighted one\n"); ok = false; }
        delete plain; delete wf;
        // literal zeros still mean the (double, double) constructor, as before the pointer form existed; arrays and pointers the new one
        ceres::ReprojectionFactor zero(0, 0);
        double fa[2] = {0.5, 0.25};
        const double* fp = fa;
        ceres::ReprojectionFactor from_array(fa, W[0]), from_pointer(fp, W[0]);
        if (zero.sqrt_information() || zero.fx() != 0.0 || !from_array.sqrt_information() || from_array.fy() != 0.25 || from_pointer.fx() != 0.5) {
            std::printf("constructor overloads are wrong\n"); ok = false;
        }
    }
    {   // DetectBa gathers W next to the features
        const bool mixed[4] = {true, false, true, true}, none[4] = {false, false, false, false};
        Small s(mixed, W);
        ceres::internal::BaLayout L;
        if (!ceres::internal::DetectBa(s.problem, &L, true, 1)) { std::printf("the problem was not recognised\n"); return 1; }
        const double I2[4] = {1.0, 0.0, 0.0, 1.0};
        if (L.sqrt_info.size() != 16) { std::printf("sqrt_info has %zu entries\n", L.sqrt_info.size()); ok = false; }
        else for (int k = 0; k < 4; ++k)
            if (std::memcmp(&L.sqrt_info[4 * k], mixed[k] ? W[k] : I2, 4 * sizeof(double)) != 0) { std::printf("row %d of sqrt_info is wrong\n", k); ok = false; }
        if (ok) std::printf("mixed problem: sqrt_info of 4 rows\n");
        Small p(none, W);
        ceres::internal::BaLayout L0;
        if (!ceres::internal::DetectBa(p.problem, &L0, true, 1) || !L0.sqrt_info.empty()) { std::printf("weights without a weighted factor\n"); ok = false; }
        else std::printf("no weighted factor: sqrt_info empty\n");
        // inner iterations: refused before any device work
        const Small ref(mixed, W);
        ceres::Solver::Options o;
        o.use_inner_iterations = true;
        ceres::Solver::Summary summary;
        ceres::Solve(o, &s.problem, &summary);
        const bool refused = summary.termination_type == ceres::FAILURE && summary.message.find("inner iterations") != std::string::npos &&
                             summary.message.find("sqrt_information") != std::string::npos && summary.execution_path.empty() &&
                             std::memcmp(s.q, ref.q, sizeof s.q) == 0 && std::memcmp(s.t, ref.t, sizeof s.t) == 0 && std::memcmp(s.lm, ref.lm, sizeof s.lm) == 0;
        std::printf("inner iterations with a weighted factor: %s [%s]\n", refused ? "refused" : "NOT REFUSED AS EXPECTED", summary.message.c_str());
        ok = ok && refused;
    }
    if (ok) std::printf("host ok\n");
    return ok ? 0 : 1;
}

static int Device(const char* file, bool callback) {
    std::ifstream in(file);
    int nc = 0, np = 0, no = 0, ncp = 0, nlp = 0;
    if (!(in >> nc >> np >> no >> ncp >> nlp)) return 2;
    std::vector<double> cams((size_t)nc * 7), pts((size_t)np * 3), feat((size_t)no * 2), la((size_t)no), lb((size_t)no), ls((size_t)no), w((size_t)no * 4);
    std::vector<int> fixed((size_t)nc), oc((size_t)no), op((size_t)no), kind((size_t)no), has_w((size_t)no), pa((size_t)ncp), pb((size_t)ncp), lp((size_t)nlp);
    for (auto& v : cams) in >> v;
    for (auto& v : fixed) in >> v;
    for (auto& v : pts) in >> v;
    for (int k = 0; k < no; ++k) in >> oc[k] >> op[k] >> feat[2 * (size_t)k] >> feat[2 * (size_t)k + 1];
    for (int k = 0; k < no; ++k) in >> kind[k] >> la[k] >> lb[k] >> ls[k];
    for (int k = 0; k < no; ++k) in >> has_w[k] >> w[4 * (size_t)k] >> w[4 * (size_t)k + 1] >> w[4 * (size_t)k + 2] >> w[4 * (size_t)k + 3];
    for (int k = 0; k < ncp; ++k) in >> pa[k] >> pb[k];
    for (auto& v : lp) in >> v;
    if (!in) return 2;
    // (quaternion and position of a camera are separate blocks: [qx qy qz qw] and [tx ty tz])
    std::vector<double> q((size_t)nc * 4), t((size_t)nc * 3);
    for (int c = 0; c < nc; ++c) { std::memcpy(&q[4 * (size_t)c], &cams[7 * (size_t)c], 4 * sizeof(double)); std::memcpy(&t[3 * (size_t)c], &cams[7 * (size_t)c + 4], 3 * sizeof(double)); }
    ceres::Problem problem;
    for (int c = 0; c < nc; ++c) problem.AddParameterBlock(&q[4 * (size_t)c], 4, new ceres::QuaternionRightPlus());
    for (int k = 0; k < no; ++k)
        problem.AddResidualBlock(has_w[k] ? ceres::ReprojectionFactor::Create(&feat[2 * (size_t)k], &w[4 * (size_t)k]) : ceres::ReprojectionFactor::Create(&feat[2 * (size_t)k]),
                                 (kind[k] < 0 && ls[k] == 1.0) ? nullptr : MakeLoss(kind[k], la[k], ls[k]),
                                 &q[4 * (size_t)oc[k]], &t[3 * (size_t)oc[k]], &pts[3 * (size_t)op[k]]);
    for (int c = 0; c < nc; ++c) if (fixed[c]) { problem.SetParameterBlockConstant(&q[4 * (size_t)c]); problem.SetParameterBlockConstant(&t[3 * (size_t)c]); }
    ceres::Solver::Options options;
    options.num_threads = 1;
    options.bundle_adjustment_losses = true;
    options.force_callback_path = callback;
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
    if (mode == "device" && argc > 2) return Device(argv[2], argc > 3 && std::string(argv[3]) == "callback");
    std::fprintf(stderr, "usage: test_ba_information_shim host | device <file> [callback]\n");
    return 2;
}
