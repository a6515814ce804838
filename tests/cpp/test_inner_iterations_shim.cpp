// Solver::Options::use_inner_iterations through include/stba/ceres.h, for tests/test_inner_iterations_shim_cpu.py (the refusals, which
// need no device) and tests/test_gpu_inner_iterations_shim.py:
//   test_inner_iterations_shim ba <scene> <kind> <strategy> <ordering> <linear_solver_type>  -- the st20 call site (test_ceres.h:98-152)
//       with the user's ProjectFactor (kind 1: recognised, "gpu-ba") or a factor the probe rejects (kind 2: "gpu-ba-hostjac").
//       ordering: -1 inner iterations off; 0 on with the default ordering; 1 {landmarks}, {rotations}, {positions}; 2 a camera's
//       rotation and position in one group; 3 a pointer that is not a parameter block; 4 every rotation and every landmark in one
//       group; 5 a negative inner_iteration_tolerance.  Prints the Summary's path, termination, iterations, inner-iteration fields
//       and message, whether the parameters moved, and the end point ("P" lines: 7 pose doubles per camera, then 3 per landmark).
//   test_inner_iterations_shim pnp <file>  -- the st17 PnP problem ("gpu-dense-callback") with inner iterations
//   test_inner_iterations_shim pg          -- a three-pose graph of RelativePoseFactors ("gpu-pg") with inner iterations
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "stba/ceres.h"
namespace ceres = stba_ceres;

template <typename T> static void QuatConjRotate(const T* q, const T* v, T* out) {   // conj(q) * v
    const T u0 = -q[0], u1 = -q[1], u2 = -q[2], w = q[3];
    const T a0 = T(2.0) * (u1 * v[2] - u2 * v[1]), a1 = T(2.0) * (u2 * v[0] - u0 * v[2]), a2 = T(2.0) * (u0 * v[1] - u1 * v[0]);
    out[0] = v[0] + w * a0 + (u1 * a2 - u2 * a1);
    out[1] = v[1] + w * a1 + (u2 * a0 - u0 * a2);
    out[2] = v[2] + w * a2 + (u0 * a1 - u1 * a0);
}
// test_ceres.h:47-81, the user's functor: recognised as the reprojection factor
struct ProjectFactor {
    double feature[2];
    explicit ProjectFactor(const double* f) { feature[0] = f[0]; feature[1] = f[1]; }
    template <typename T> bool operator()(T const* const* parameters, T* residuals) const {
        const T* q = parameters[0]; const T* t = parameters[1]; const T* L = parameters[2];
        T d[3] = {L[0] - t[0], L[1] - t[1], L[2] - t[2]}, pc[3];
        QuatConjRotate(q, d, pc);
        residuals[0] = pc[0] / pc[2] - T(feature[0]);
        residuals[1] = pc[1] / pc[2] - T(feature[1]);
        return true;
    }
};
// the factor in front of the camera, doubled behind it: the probe point behind the camera rejects it ("gpu-ba-hostjac")
struct BehindScaledProjectFactor {
    double feature[2];
    explicit BehindScaledProjectFactor(const double* f) { feature[0] = f[0]; feature[1] = f[1]; }
    template <typename T> bool operator()(T const* const* parameters, T* residuals) const {
        const T* q = parameters[0]; const T* t = parameters[1]; const T* L = parameters[2];
        T d[3] = {L[0] - t[0], L[1] - t[1], L[2] - t[2]}, pc[3];
        QuatConjRotate(q, d, pc);
        const T w = (pc[2] < T(0.0)) ? T(2.0) : T(1.0);
        residuals[0] = w * (pc[0] / pc[2] - T(feature[0]));
        residuals[1] = w * (pc[1] / pc[2] - T(feature[1]));
        return true;
    }
};
// solver.hpp:127-155
struct PnPFunctor {
    double point[3], feature[2];
    template <typename T> bool operator()(const T* const q, const T* const t, T* residuals) const {
        T d[3] = {T(point[0]) - t[0], T(point[1]) - t[1], T(point[2]) - t[2]}, pc[3];
        QuatConjRotate(q, d, pc);
        residuals[0] = pc[0] / pc[2] - T(feature[0]);
        residuals[1] = pc[1] / pc[2] - T(feature[1]);
        return true;
    }
};

static void PrintInts(const char* name, const std::vector<int>& v) {
    std::printf("%s", name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}

static void PrintSummary(const ceres::Solver::Summary& s) {
    std::printf("path %s\ntermination %d\niterations %d\n", s.execution_path.c_str(), (int)s.termination_type, (int)s.iterations.size() - 1);
    std::printf("inner_given %d\ninner_used %d\ninner_steps %d\ninner_time %.17g\n", s.inner_iterations_given ? 1 : 0,
                s.inner_iterations_used ? 1 : 0, s.num_inner_iteration_steps, s.inner_iteration_time_in_seconds);
    PrintInts("ordering_given", s.inner_iteration_ordering_given);
    PrintInts("ordering_used", s.inner_iteration_ordering_used);
    std::printf("successful");
    for (const auto& it : s.iterations) std::printf(" %d", it.step_is_successful ? 1 : 0);
    std::printf("\nfinal_cost %.17g\nmessage %s\n", s.final_cost, s.message.c_str());
}

static int RunBa(const char* path, int kind, int strategy, int ordering, int linear_solver_type) {
    std::ifstream f(path, std::ios::binary);
    int h[3];
    if (!f.read((char*)h, sizeof h)) return 2;
    const int nc = h[0], np = h[1], no = h[2];
    std::vector<double> cams((size_t)nc * 7), pts((size_t)np * 3), feat((size_t)no * 2);
    std::vector<int> oc(no), op(no);
    std::vector<unsigned char> fixed(nc);
    f.read((char*)cams.data(), cams.size() * 8); f.read((char*)pts.data(), pts.size() * 8);
    f.read((char*)oc.data(), no * 4); f.read((char*)op.data(), no * 4); f.read((char*)feat.data(), feat.size() * 8);
    f.read((char*)fixed.data(), nc);
    if (!f) return 2;
    std::vector<double> q((size_t)nc * 4), t((size_t)nc * 3);
    for (int c = 0; c < nc; ++c) { std::memcpy(&q[4 * c], &cams[7 * c], 32); std::memcpy(&t[3 * c], &cams[7 * c + 4], 24); }
    const std::vector<double> q0 = q, t0 = t, p0 = pts;
    ceres::Problem problem;
    for (int c = 0; c < nc; ++c) problem.AddParameterBlock(&q[4 * c], 4, new ceres::QuaternionRightPlus());
    for (int i = 0; i < no; ++i) {
        ceres::CostFunction* cf;
        if (kind == 1) {
            auto* c1 = new ceres::DynamicAutoDiffCostFunction<ProjectFactor>(new ProjectFactor(&feat[2 * i]));
            for (int k : {4, 3, 3}) c1->AddParameterBlock(k);
            c1->SetNumResiduals(2);
            cf = c1;
        } else {
            auto* c2 = new ceres::DynamicAutoDiffCostFunction<BehindScaledProjectFactor>(new BehindScaledProjectFactor(&feat[2 * i]));
            for (int k : {4, 3, 3}) c2->AddParameterBlock(k);
            c2->SetNumResiduals(2);
            cf = c2;
        }
        problem.AddResidualBlock(cf, nullptr, &q[4 * oc[i]], &t[3 * oc[i]], &pts[3 * op[i]]);
    }
    for (int c = 0; c < nc; ++c)
        if (fixed[c]) { problem.SetParameterBlockConstant(&q[4 * c]); problem.SetParameterBlockConstant(&t[3 * c]); }   // test_ceres.h:127-130
    ceres::Solver::Options options;
    options.linear_solver_type = static_cast<ceres::LinearSolverType>(linear_solver_type);
    options.trust_region_strategy_type = static_cast<ceres::TrustRegionStrategyType>(strategy);
    options.max_num_iterations = 100;
    options.use_inner_iterations = ordering >= 0;
    double stray[3] = {0, 0, 0};
    if (ordering >= 1 && ordering <= 4) {
        auto ord = std::make_shared<ceres::ParameterBlockOrdering>();
        for (int j = 0; j < np; ++j) ord->AddElementToGroup(&pts[3 * j], ordering == 4 ? 1 : 0);
        for (int c = 0; c < nc; ++c) {
            ord->AddElementToGroup(&q[4 * c], 1);
            ord->AddElementToGroup(&t[3 * c], ordering == 2 ? 1 : 2);
        }
        if (ordering == 3) ord->AddElementToGroup(stray, 3);
        options.inner_iteration_ordering = ord;
    }
    if (ordering == 5) options.inner_iteration_tolerance = -1.0;
    ceres::Solver::Summary summary;
    ceres::Solve(options, &problem, &summary);
    PrintSummary(summary);
    std::printf("moved %d\n", (q != q0 || t != t0 || pts != p0) ? 1 : 0);
    for (int c = 0; c < nc; ++c) {
        std::printf("P");
        for (int k = 0; k < 4; ++k) std::printf(" %.17g", q[4 * c + k]);
        for (int k = 0; k < 3; ++k) std::printf(" %.17g", t[3 * c + k]);
        std::printf("\n");
    }
    for (int j = 0; j < np; ++j) std::printf("P %.17g %.17g %.17g\n", pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]);
    return 0;
}

static int RunPnP(const char* path) {
    std::ifstream f(path, std::ios::binary);
    int n = 0;
    if (!f.read((char*)&n, sizeof n)) return 2;
    std::vector<double> x(7), data((size_t)n * 5);
    f.read((char*)x.data(), x.size() * 8); f.read((char*)data.data(), data.size() * 8);
    if (!f) return 2;
    ceres::Problem problem;
    problem.AddParameterBlock(&x[0], 4, new ceres::QuaternionRightPlus());
    for (int i = 0; i < n; ++i) {
        auto* fn = new PnPFunctor{{data[5 * i], data[5 * i + 1], data[5 * i + 2]}, {data[5 * i + 3], data[5 * i + 4]}};
        problem.AddResidualBlock(new ceres::AutoDiffCostFunction<PnPFunctor, 2, 4, 3>(fn), nullptr, &x[0], &x[4]);
    }
    const std::vector<double> x0 = x;
    ceres::Solver::Options options;
    options.use_inner_iterations = true;
    ceres::Solver::Summary summary;
    ceres::Solve(options, &problem, &summary);
    PrintSummary(summary);
    std::printf("moved %d\n", x != x0 ? 1 : 0);
    return 0;
}

static int RunPoseGraph() {
    // three poses on a line, the middle one off by 0.1; identity rotations, unit steps along x
    std::vector<double> poses = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1.1, 0.1, 0, 0, 0, 0, 1, 2, 0, 0};
    const double meas[7] = {0, 0, 0, 1, 1, 0, 0};
    const std::vector<double> x0 = poses;
    ceres::Problem problem;
    for (int k = 0; k < 3; ++k) problem.AddParameterBlock(&poses[7 * k], 7, new ceres::SE3RightPlus());
    for (int k = 0; k < 2; ++k) problem.AddResidualBlock(ceres::RelativePoseFactor::Create(meas), nullptr, {&poses[7 * k], &poses[7 * k + 7]});
    problem.SetParameterBlockConstant(&poses[0]);
    ceres::Solver::Options options;
    options.use_inner_iterations = true;
    ceres::Solver::Summary summary;
    ceres::Solve(options, &problem, &summary);
    PrintSummary(summary);
    std::printf("moved %d\n", poses != x0 ? 1 : 0);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "ba" && argc > 6) return RunBa(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
    if (mode == "pnp" && argc > 2) return RunPnP(argv[2]);
    if (mode == "pg") return RunPoseGraph();
    std::printf("usage: test_inner_iterations_shim ba <scene> <kind> <strategy> <ordering> <linear_solver_type> | pnp <file> | pg\n");
    return 2;
}
