// NodePosePriorFactor through include/stba/ceres.h, for tests/test_pg_prior_shim.py (host mode, no device) and
// tests/test_gpu_pg_prior_shim.py:
//   test_pg_prior_shim host            -- the factor itself: its residual is RelativePoseFactor's with the first pose at the identity,
//       the autodiff Jacobian against central differences, sqrt_information() of both forms of Create; and the recognition: a graph
//       with priors interleaved among its edges is a pose graph whose layout sets the priors aside and keeps the per-edge tables in
//       edge order; a prior with a LossFunction, and a problem of priors only, are not.
//   test_pg_prior_shim device <file>   -- the graph of <file>: n m k n_pairs | n x 7 poses | n fixed flags | m x (i j) | m x 7
//       measurements | k prior nodes | k x 7 prior poses | k flags (1: the prior gets a W) | k x 36 W | n_pairs x (a b).  Prints per
//       prior "P <k> r(6) J(36)": the factor's own Evaluate at the start, its Jacobian composed with SE3RightPlus' (6 x 6, tangent).
//       Solves on "gpu-pg" and, from the same start with force_callback_path, on "gpu-dense-callback"; then ceres::Covariance at the
//       gpu-pg solution.  Prints per route "<route> path <execution_path> term <t> iters <k> initial <c0> final <c>" and
//       "<route>_poses ...", and per pair a "T" line.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "stba/ceres.h"
namespace ceres = stba_ceres;

static void MakeW(double* W) {
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) W[a * 6 + b] = (a == b ? 2.0 + a : 0.0) + 0.31 * std::sin(0.7 + 1.9 * a + 0.6 * b);      // neither symmetric nor triangular
}

static int Host() {
    const double z[7] = {0.05, -0.02, 0.03, 0.9979, 0.4, -0.1, 0.2};
    const double I7[7] = {0, 0, 0, 1, 0, 0, 0};
    double T[7] = {0.1, 0.2, -0.1, 0.0, 1.0, 2.0, 3.0};
    T[3] = std::sqrt(1.0 - T[0] * T[0] - T[1] * T[1] - T[2] * T[2]);
    double W[36];
    MakeW(W);
    ceres::NodePosePriorFactor* plain = ceres::NodePosePriorFactor::Create(z);
    ceres::NodePosePriorFactor* weighted = ceres::NodePosePriorFactor::Create(z, W);
    if (plain->sqrt_information() != nullptr) { std::printf("Create(measurement) has a W\n"); return 1; }
    if (!weighted->sqrt_information() || std::memcmp(weighted->sqrt_information(), W, sizeof W) != 0 || std::memcmp(weighted->measurement(), z, sizeof z) != 0) {
        std::printf("Create(measurement, sqrt_information) lost its arguments\n"); return 1;
    }
    // the residual: the edge's own, first pose at the identity -- the same functor, the same bits
    ceres::RelativePoseFactor edge(z, W);
    const double* one[1] = {T};
    const double* two[2] = {I7, T};
    double rp[6], re[6], J[42];
    double* jac[1] = {J};
    if (!weighted->Evaluate(one, rp, jac) || !edge.Evaluate(two, re, nullptr)) return 1;
    for (int a = 0; a < 6; ++a) if (rp[a] != re[a]) { std::printf("the prior's residual is not the edge's from the identity\n"); return 1; }
    double rr[6];
    weighted->Evaluate(one, rr, nullptr);
    for (int a = 0; a < 6; ++a) if (std::fabs(rr[a] - rp[a]) > 1e-15 * std::fmax(1.0, std::fabs(rp[a]))) return 1;
    double scale = 0.0, rel = 0.0;
    for (int q = 0; q < 42; ++q) scale = std::fmax(scale, std::fabs(J[q]));
    for (int k = 0; k < 7; ++k) {
        double a7[7], b7[7], r1[6], r2[6];
        std::memcpy(a7, T, sizeof a7); std::memcpy(b7, T, sizeof b7);
        const double h = 1e-6;
        a7[k] += h; b7[k] -= h;
        const double* pa[1] = {a7};
        const double* pb[1] = {b7};
        weighted->Evaluate(pa, r1, nullptr); weighted->Evaluate(pb, r2, nullptr);
        for (int a = 0; a < 6; ++a) rel = std::fmax(rel, std::fabs((r1[a] - r2[a]) / (2 * h) - J[a * 7 + k]) / scale);
    }
    std::printf("jacobian: max |autodiff - central difference| / max |J| = %.3e\n", rel);
    if (!(rel <= 1e-7)) return 1;
    delete plain; delete weighted;

    // ---- the recognition.  Five poses in a chain, four edges; which = 0: priors interleaved (in front of, between and behind the
    // edges), edge 2 with a W and edge 1 with a Huber loss; 1: the same with a loss on one prior; 2: priors only; 3: no prior at all
    std::vector<double> poses;
    for (int k = 0; k < 5; ++k) { const double p[7] = {0, 0, 0, 1, 0.5 * k, 0, 0}; poses.insert(poses.end(), p, p + 7); }
    for (int which = 0; which < 4; ++which) {
        ceres::Problem problem;
        for (int k = 0; k < 5; ++k) problem.AddParameterBlock(&poses[7 * k], 7, new ceres::SE3RightPlus());
        auto prior = [&](int node, bool with_w, bool with_loss) {
            problem.AddResidualBlock(ceres::NodePosePriorFactor::Create(z, with_w ? W : nullptr), with_loss ? new ceres::HuberLoss(1.0) : nullptr, {&poses[7 * node]});
        };
        auto edge_block = [&](int e) {
            problem.AddResidualBlock(e == 2 ? ceres::RelativePoseFactor::Create(z, W) : ceres::RelativePoseFactor::Create(z),
                                     e == 1 ? new ceres::HuberLoss(0.5) : nullptr, {&poses[7 * e], &poses[7 * (e + 1)]});
        };
        if (which != 3) prior(4, true, false);
        if (which != 2) { edge_block(0); edge_block(1); }
        if (which != 3) prior(2, false, which == 1);
        if (which != 2) { edge_block(2); edge_block(3); }
        if (which != 3) prior(4, false, false);
        ceres::internal::PoseGraphLayout L;
        const bool is_pg = ceres::internal::DetectPoseGraph(&problem, &L);
        std::printf("recognition %d: %s\n", which, is_pg ? "pose graph" : "not a pose graph");
        if (is_pg != (which == 0 || which == 3)) return 1;
        if (which == 3) { if (!L.prior_node.empty() || !L.edge_res.empty() || L.ei.size() != 4) return 1; continue; }
        if (which != 0) continue;
        // nodes are numbered as the residual blocks first name them: block 4 (the first prior's), then 0, 1, 2, 3
        const int want_node[3] = {0, 3, 0}, want_res[4] = {1, 2, 4, 5}, want_i[4] = {1, 2, 3, 4}, want_j[4] = {2, 3, 4, 0};
        if (L.prior_node.size() != 3 || L.prior_pose.size() != 21 || L.prior_w.size() != 108 || L.ei.size() != 4 || L.edge_res.size() != 4) {
            std::printf("layout sizes: %zu priors, %zu edges\n", L.prior_node.size(), L.ei.size()); return 1;
        }
        for (int k = 0; k < 3; ++k) {
            if (L.prior_node[k] != want_node[k] || std::memcmp(&L.prior_pose[7 * k], z, sizeof z) != 0) { std::printf("prior %d: node or pose\n", k); return 1; }
            for (int q = 0; q < 36; ++q)
                if (L.prior_w[36 * k + q] != (k == 0 ? W[q] : (q % 7 == 0 ? 1.0 : 0.0))) { std::printf("prior %d: W entry %d\n", k, q); return 1; }
        }
        for (int e = 0; e < 4; ++e) {
            if (L.edge_res[e] != want_res[e] || L.ei[e] != want_i[e] || L.ej[e] != want_j[e]) { std::printf("edge %d: residual block or ends\n", e); return 1; }
            for (int q = 0; q < 36; ++q)
                if (L.sqrt_info[36 * e + q] != (e == 2 ? W[q] : (q % 7 == 0 ? 1.0 : 0.0))) { std::printf("edge %d: W entry %d\n", e, q); return 1; }
        }
        if (L.loss_kind.size() != 4 || !L.losses_known) { std::printf("loss table: %zu rows\n", L.loss_kind.size()); return 1; }
        for (int e = 0; e < 4; ++e)
            if (L.loss_kind[e] != (e == 1 ? STBA_LOSS_HUBER : STBA_LOSS_TRIVIAL) || (e == 1 && L.loss_a[e] != 0.5)) { std::printf("loss table: edge %d\n", e); return 1; }
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
    int n = 0, m = 0, k = 0, np = 0;
    if (!(in >> n >> m >> k >> np)) return 2;
    std::vector<double> poses0((size_t)n * 7), meas((size_t)m * 7), ppose((size_t)k * 7), W((size_t)k * 36);
    std::vector<int> fixed((size_t)n), ei((size_t)m), ej((size_t)m), pnode((size_t)k), flag((size_t)k), pa((size_t)np), pb((size_t)np);
    for (auto& v : poses0) in >> v;
    for (auto& v : fixed) in >> v;
    for (int e = 0; e < m; ++e) in >> ei[e] >> ej[e];
    for (auto& v : meas) in >> v;
    for (auto& v : pnode) in >> v;
    for (auto& v : ppose) in >> v;
    for (auto& v : flag) in >> v;
    for (auto& v : W) in >> v;
    for (int q = 0; q < np; ++q) in >> pa[q] >> pb[q];
    if (!in) return 2;
    // the factor's own Evaluate at the start, in the tangent: J (6 x 7) times SE3RightPlus' Jacobian (7 x 6)
    for (int q = 0; q < k; ++q) {
        ceres::NodePosePriorFactor f(&ppose[7 * (size_t)q], flag[q] ? &W[36 * (size_t)q] : nullptr);
        const double* blk[1] = {&poses0[7 * (size_t)pnode[q]]};
        double r[6], J[42], Pj[42], Jt[36];
        double* jac[1] = {J};
        if (!f.Evaluate(blk, r, jac) || !ceres::SE3RightPlus().ComputeJacobian(blk[0], Pj)) return 1;
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) {
                double s = 0.0;
                for (int c = 0; c < 7; ++c) s += J[a * 7 + c] * Pj[c * 6 + b];
                Jt[a * 6 + b] = s;
            }
        std::printf("P %d", q);
        for (int a = 0; a < 6; ++a) std::printf(" %.17g", r[a]);
        for (int a = 0; a < 36; ++a) std::printf(" %.17g", Jt[a]);
        std::printf("\n");
    }
    for (int route = 0; route < 2; ++route) {
        std::vector<double> poses = poses0;
        ceres::Problem problem;
        for (int q = 0; q < n; ++q) problem.AddParameterBlock(&poses[7 * (size_t)q], 7, new ceres::SE3RightPlus());
        // (odd priors in front of the edges, even ones behind: the edges are not the first residual blocks)
        auto add_priors = [&](int parity) {
            for (int q = 0; q < k; ++q)
                if ((q & 1) == parity)
                    problem.AddResidualBlock(ceres::NodePosePriorFactor::Create(&ppose[7 * (size_t)q], flag[q] ? &W[36 * (size_t)q] : nullptr), nullptr,
                                             {&poses[7 * (size_t)pnode[q]]});
        };
        add_priors(1);
        for (int e = 0; e < m; ++e)
            problem.AddResidualBlock(ceres::RelativePoseFactor::Create(&meas[7 * (size_t)e]), nullptr, {&poses[7 * (size_t)ei[e]], &poses[7 * (size_t)ej[e]]});
        add_priors(0);
        for (int q = 0; q < n; ++q) if (fixed[q]) problem.SetParameterBlockConstant(&poses[7 * (size_t)q]);
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
            for (int q = 0; q < np; ++q) pairs.push_back({&poses[7 * (size_t)pa[q]], &poses[7 * (size_t)pb[q]]});
            ceres::Covariance cov{ceres::Covariance::Options()};
            const bool ok = cov.Compute(pairs, &problem);
            std::printf("cov path %s\n", cov.execution_path().c_str());
            if (!ok) { std::printf("covariance failed: %s\n", cov.message().c_str()); return 1; }
            for (int q = 0; q < np; ++q) {
                double t[36];
                if (!cov.GetCovarianceBlockInTangentSpace(pairs[q].first, pairs[q].second, t)) return 1;
                std::printf("T %d", q);
                for (int a = 0; a < 36; ++a) std::printf(" %.17g", t[a]);
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
    std::fprintf(stderr, "usage: test_pg_prior_shim host | device <file>\n");
    return 2;
}
