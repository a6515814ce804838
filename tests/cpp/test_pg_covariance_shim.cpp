// ceres::Covariance on a pose graph ("gpu-pg") through include/stba/ceres.h, for tests/test_pg_covariance_shim.py (the refusals, which
// need no device) and tests/test_gpu_pg_covariance_shim.py:
//   test_pg_covariance_shim refuse          -- a graph without a constant pose (gauge freedom) and a pair with an unknown pointer
//   test_pg_covariance_shim device <file>   -- the graph of <file>: n m n_pairs | n x 7 poses | n fixed flags | m x (i j) | m x 7
//       measurements | n_pairs x (a b).  Prints "path <execution_path>", and per pair a "T" line (the 6x6 tangent block), an "A" line
//       (the 7x7 ambient block) and "Ja" / "Jb" lines (SE3RightPlus::ComputeJacobian of the two poses, 7x6), all with 17 digits.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "stba/ceres.h"
namespace ceres = stba_ceres;

static void Build(ceres::Problem& problem, std::vector<double>& poses, const std::vector<int>& ei, const std::vector<int>& ej,
                  const std::vector<double>& meas, const std::vector<int>& fixed) {
    const int n = (int)poses.size() / 7;
    for (int k = 0; k < n; ++k) problem.AddParameterBlock(&poses[7 * k], 7, new ceres::SE3RightPlus());
    for (size_t e = 0; e < ei.size(); ++e)
        problem.AddResidualBlock(ceres::RelativePoseFactor::Create(&meas[7 * e]), nullptr, {&poses[7 * ei[e]], &poses[7 * ej[e]]});
    for (int k = 0; k < n; ++k) if (fixed[k]) problem.SetParameterBlockConstant(&poses[7 * k]);
}

static int Refuse() {
    std::vector<double> poses;
    for (int k = 0; k < 5; ++k) { const double p[7] = {0, 0, 0, 1, 0.5 * k, 0, 0}; poses.insert(poses.end(), p, p + 7); }
    const double z[7] = {0, 0, 0, 1, 0.5, 0, 0};
    std::vector<double> meas;
    for (int e = 0; e < 3; ++e) meas.insert(meas.end(), z, z + 7);
    // two components: {0, 1} with pose 0 constant, {2, 3, 4} without a constant pose
    ceres::Problem problem;
    Build(problem, poses, {0, 2, 3}, {1, 3, 4}, meas, {1, 0, 0, 0, 0});
    ceres::Covariance cov{ceres::Covariance::Options()};
    double out[49];
    if (cov.Compute({{&poses[7], &poses[7]}}, &problem)) { std::printf("a graph with a free component was accepted\n"); return 1; }
    std::printf("message: %s\n", cov.message().c_str());
    if (cov.execution_path() != "gpu-pg") { std::printf("path %s\n", cov.execution_path().c_str()); return 1; }
    if (cov.message().find("component of 3 nodes") == std::string::npos || cov.message().find("first node 2") == std::string::npos) return 1;
    if (cov.GetCovarianceBlock(&poses[7], &poses[7], out)) { std::printf("a block after a refusal\n"); return 1; }
    double stranger[7] = {0, 0, 0, 1, 0, 0, 0};
    ceres::Covariance cov2{ceres::Covariance::Options()};
    if (cov2.Compute({{&poses[0], stranger}}, &problem)) { std::printf("an unknown pointer was accepted\n"); return 1; }
    if (cov2.message().find("not in the problem") == std::string::npos) { std::printf("message: %s\n", cov2.message().c_str()); return 1; }
    std::printf("refuse ok\n");
    return 0;
}

static void PrintLine(const char* tag, size_t k, const double* v, int count) {
    std::printf("%s %zu", tag, k);
    for (int q = 0; q < count; ++q) std::printf(" %.17g", v[q]);
    std::printf("\n");
}

static int Device(const char* file) {
    std::ifstream in(file);
    int n = 0, m = 0, np = 0;
    if (!(in >> n >> m >> np)) return 2;
    std::vector<double> poses((size_t)n * 7), meas((size_t)m * 7);
    std::vector<int> fixed((size_t)n), ei((size_t)m), ej((size_t)m), pa((size_t)np), pb((size_t)np);
    for (auto& v : poses) in >> v;
    for (auto& v : fixed) in >> v;
    for (int e = 0; e < m; ++e) in >> ei[e] >> ej[e];
    for (auto& v : meas) in >> v;
    for (int k = 0; k < np; ++k) in >> pa[k] >> pb[k];
    if (!in) return 2;
    ceres::Problem problem;
    Build(problem, poses, ei, ej, meas, fixed);
    std::vector<std::pair<const double*, const double*>> pairs;
    for (int k = 0; k < np; ++k) pairs.push_back({&poses[7 * pa[k]], &poses[7 * pb[k]]});
    ceres::Covariance cov{ceres::Covariance::Options()};
    const bool ok = cov.Compute(pairs, &problem);
    std::printf("path %s\n", cov.execution_path().c_str());
    if (!ok) { std::printf("failed: %s\n", cov.message().c_str()); return 1; }
    ceres::SE3RightPlus chart;
    for (int k = 0; k < np; ++k) {
        double t[36], a[49], ja[42], jb[42];
        if (!cov.GetCovarianceBlockInTangentSpace(pairs[k].first, pairs[k].second, t) || !cov.GetCovarianceBlock(pairs[k].first, pairs[k].second, a)) return 1;
        chart.ComputeJacobian(pairs[k].first, ja); chart.ComputeJacobian(pairs[k].second, jb);
        PrintLine("T", k, t, 36); PrintLine("A", k, a, 49); PrintLine("Ja", k, ja, 42); PrintLine("Jb", k, jb, 42);
    }
    std::printf("device ok\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "refuse") return Refuse();
    if (mode == "device" && argc > 2) return Device(argv[2]);
    std::fprintf(stderr, "usage: test_pg_covariance_shim refuse | device <file>\n");
    return 2;
}
