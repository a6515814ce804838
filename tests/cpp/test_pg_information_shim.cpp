// RelativePoseFactor with a square-root information matrix through include/stba/ceres.h, for tests/test_pg_information_shim.py (host mode,
// no device) and tests/test_gpu_pg_information_shim.py:
//   test_pg_information_shim host            -- the factor itself: residual = W x (residual without W), the autodiff Jacobian against
//       central differences, sqrt_information() of both constructors, and the stacked W of a mixed problem (identity blocks for
//       factors without one; empty when no factor has one)
//   test_pg_information_shim device <file>   -- the graph of <file>: n m n_pairs | n x 7 poses | n fixed flags | m x (i j) | m x 7
//       measurements | m flags (1: the factor gets a W) | m x 36 W | n_pairs x (a b).  Solves it on "gpu-pg" and, from the same start
//       with force_callback_path, on "gpu-dense-callback"; then ceres::Covariance at the gpu-pg solution.  Prints per route
//       "<route> path <execution_path> term <t> iters <k> initial <c0> final <c>" and "<route>_poses ...", and per pair a "T" line.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "stba/ceres.h"
namespace ceres = stba_ceres;

static int Host() {
    const double z[7] = {0.05, -0.02, 0.03, 0.9979, 0.4, -0.1, 0.2};
    double Ti[7] = {0.1, 0.2, -0.1, 0.0, 1.0, 2.0, 3.0}, Tj[7] = {0.15, 0.1, -0.2, 0.0, 1.5, 1.8, 3.1};
    for (double* T : {Ti, Tj}) {
        T[3] = std::sqrt(1.0 - T[0] * T[0] - T[1] * T[1] - T[2] * T[2]);
    }
    double W[36];
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) W[a * 6 + b] = (a == b ? 3.0 + a : 0.0) + 0.37 * std::sin(1.0 + 2.3 * a + 0.7 * b);      // neither symmetric nor triangular
    ceres::RelativePoseFactor plain(z), weighted(z, W);
    if (plain.sqrt_information() != nullptr) { std::printf("the one-argument constructor has a W\n"); return 1; }
    if (!weighted.sqrt_information() || std::memcmp(weighted.sqrt_information(), W, sizeof W) != 0) { std::printf("sqrt_information() is not the W given\n"); return 1; }
    ceres::RelativePoseFactor* made = ceres::RelativePoseFactor::Create(z, W);
    const bool created = made->sqrt_information() && std::memcmp(made->sqrt_information(), W, sizeof W) == 0 && std::memcmp(made->measurement(), z, sizeof z) == 0;
    delete made;
    if (!created) { std::printf("Create(measurement, sqrt_information) lost its arguments\n"); return 1; }
    const double* blocks[2] = {Ti, Tj};
    double r0[6], r1[6], J0[42], J1[42];
    double* jac[2] = {J0, J1};
    if (!plain.Evaluate(blocks, r0, nullptr) || !weighted.Evaluate(blocks, r1, jac)) return 1;
    double worst = 0.0;
    for (int a = 0; a < 6; ++a) {
        double s = 0.0, mag = 0.0;
        for (int k = 0; k < 6; ++k) { s += W[a * 6 + k] * r0[k]; mag += std::fabs(W[a * 6 + k] * r0[k]); }
        worst = std::fmax(worst, std::fabs(r1[a] - s) / (mag * 2.220446049250313e-16));
    }
    std::printf("residual: max |r_W - W r| / (eps sum |W||r|) = %.2f\n", worst);
    if (!(worst <= 8.0)) return 1;
    double rj[6];
    weighted.Evaluate(blocks, rj, nullptr);          // (the residual-only call and the autodiff call agree)
    for (int a = 0; a < 6; ++a) if (std::fabs(rj[a] - r1[a]) > 1e-15 * std::fmax(1.0, std::fabs(r1[a]))) return 1;
    // the autodiff Jacobian (ambient, 6 x 7 per block) against central differences, relative to the largest entry of its block
    double rel = 0.0;
    for (int blk = 0; blk < 2; ++blk) {
        double scale = 0.0;
        for (int q = 0; q < 42; ++q) scale = std::fmax(scale, std::fabs(jac[blk][q]));
        for (int k = 0; k < 7; ++k) {
            double a7[7], b7[7], rp[6], rm[6];
            std::memcpy(a7, blk ? Tj : Ti, sizeof a7); std::memcpy(b7, a7, sizeof b7);
            const double h = 1e-6;
            a7[k] += h; b7[k] -= h;
            const double* pp[2] = {blk ? Ti : a7, blk ? a7 : Tj};
            const double* pm[2] = {blk ? Ti : b7, blk ? b7 : Tj};
            weighted.Evaluate(pp, rp, nullptr); weighted.Evaluate(pm, rm, nullptr);
            for (int a = 0; a < 6; ++a) rel = std::fmax(rel, std::fabs((rp[a] - rm[a]) / (2 * h) - jac[blk][a * 7 + k]) / scale);
        }
    }
    std::printf("jacobian: max |autodiff - central difference| / max |J| = %.3e\n", rel);
    if (!(rel <= 1e-7)) return 1;
    // a mixed problem: factors 1 and 3 of 4 weighted; and one without any weighted factor
    std::vector<double> poses;
    for (int k = 0; k < 5; ++k) { const double p[7] = {0, 0, 0, 1, 0.5 * k, 0, 0}; poses.insert(poses.end(), p, p + 7); }
    for (int mixed = 0; mixed < 2; ++mixed) {
        ceres::Problem problem;
        for (int k = 0; k < 5; ++k) problem.AddParameterBlock(&poses[7 * k], 7, new ceres::SE3RightPlus());
        for (int e = 0; e < 4; ++e)
            problem.AddResidualBlock((mixed && (e == 1 || e == 3)) ? ceres::RelativePoseFactor::Create(z, W) : ceres::RelativePoseFactor::Create(z),
                                     nullptr, {&poses[7 * e], &poses[7 * (e + 1)]});
        problem.SetParameterBlockConstant(&poses[0]);
        ceres::internal::PoseGraphLayout L;
        if (!ceres::internal::DetectPoseGraph(&problem, &L)) { std::printf("the graph was not recognised\n"); return 1; }
        if (!mixed) { if (!L.sqrt_info.empty()) { std::printf("a stacked W without a weighted factor\n"); return 1; } continue; }
        if (L.sqrt_info.size() != 4 * 36) { std::printf("stacked W has %zu doubles\n", L.sqrt_info.size()); return 1; }
        for (int e = 0; e < 4; ++e)
            for (int q = 0; q < 36; ++q) {
                const double want = (e == 1 || e == 3) ? W[q] : ((q % 7 == 0) ? 1.0 : 0.0);
                if (L.sqrt_info[(size_t)e * 36 + q] != want) { std::printf("stacked W: edge %d entry %d\n", e, q); return 1; }
            }
    }
    std::printf("host ok\n");
    return 0;
}

static void PrintVec(const char* tag, const double* v, size_t count) {
    std::printf("%s", tag);
    for (size_t q = 0; q < count; ++q) std::printf(" %.17g", v[q]);
    std::printf("\n");
}

static int Device(const char* file) {
    std::ifstream in(file);
    int n = 0, m = 0, np = 0;
    if (!(in >> n >> m >> np)) return 2;
    std::vector<double> poses0((size_t)n * 7), meas((size_t)m * 7), W((size_t)m * 36);
    std::vector<int> fixed((size_t)n), ei((size_t)m), ej((size_t)m), flag((size_t)m), pa((size_t)np), pb((size_t)np);
    for (auto& v : poses0) in >> v;
    for (auto& v : fixed) in >> v;
    for (int e = 0; e < m; ++e) in >> ei[e] >> ej[e];
    for (auto& v : meas) in >> v;
    for (auto& v : flag) in >> v;
    for (auto& v : W) in >> v;
    for (int k = 0; k < np; ++k) in >> pa[k] >> pb[k];
    if (!in) return 2;
    for (int route = 0; route < 2; ++route) {
        std::vector<double> poses = poses0;
        ceres::Problem problem;
        for (int k = 0; k < n; ++k) problem.AddParameterBlock(&poses[7 * (size_t)k], 7, new ceres::SE3RightPlus());
        for (int e = 0; e < m; ++e)
            problem.AddResidualBlock(flag[e] ? ceres::RelativePoseFactor::Create(&meas[7 * (size_t)e], &W[36 * (size_t)e]) : ceres::RelativePoseFactor::Create(&meas[7 * (size_t)e]),
                                     nullptr, {&poses[7 * (size_t)ei[e]], &poses[7 * (size_t)ej[e]]});
        for (int k = 0; k < n; ++k) if (fixed[k]) problem.SetParameterBlockConstant(&poses[7 * (size_t)k]);
        ceres::Solver::Options options;
        options.num_threads = 1;
        options.function_tolerance = 1e-12;
        options.parameter_tolerance = 1e-11;
        options.force_callback_path = route == 1;
        ceres::Solver::Summary summary;
        ceres::Solve(options, &problem, &summary);
        const char* name = route ? "dense" : "pg";
        std::printf("%s path %s term %d iters %d initial %.17g final %.17g\n", name, summary.execution_path.c_str(), (int)summary.termination_type,
                    (int)summary.iterations.size() - 1, summary.initial_cost, summary.final_cost);
        if (summary.termination_type != ceres::CONVERGENCE) { std::printf("%s message %s\n", name, summary.message.c_str()); return 1; }
        PrintVec(route ? "dense_poses" : "pg_poses", poses.data(), poses.size());
        if (route == 0) {
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
        }
    }
    std::printf("device ok\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "host") return Host();
    if (mode == "device" && argc > 2) return Device(argv[2]);
    std::fprintf(stderr, "usage: test_pg_information_shim host | device <file>\n");
    return 2;
}
