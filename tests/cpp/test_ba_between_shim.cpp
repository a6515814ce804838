// Driver of tests/test_ba_between_reference_cpu.py (no argument: host only) and tests/test_gpu_ba_between_shim.py ("device <scene> <mode>").
// Host mode: ceres::CameraRelativePoseFactor::Evaluate.
//   stdin:  n, then n times: meas[7] cam_i[7] cam_j[7] has_w W[36]
//   stdout: per case one line: r'[6], then J_i'[36] and J_j'[36], each [Jq (6 x 4) . QuaternionRightPlus::ComputeJacobian(q) (4 x 3) |
//           Jt (6 x 3)] row-major; then the line "detect a b c d e": internal::DetectBa on a three-camera BA problem (a) without such a
//           block, (b) with one between the cameras 1 and 0 (and the residual <-> observation bookkeeping checked), (c) with one whose
//           position blocks are swapped between the two cameras, (d) with one onto a camera no observation names, (e) with one that
//           carries a LossFunction
// Device mode: the reference's BA call site (test_ceres.h:98-152) with PosePriorFactor and CameraRelativePoseFactor blocks, no block constant.
//   scene:  nc np no npr ne ccov / cams[nc][7] / pts[np][3] / no x (cam pt fx fy) / npr x (cam pose[7] W[36]) / ne x (i j meas[7] W[36])
//   mode:   lm | iterative | dogleg | inner | callback
//   stdout: "ba <path> <termination> <iterations> <initial cost> <final cost>", "msg <message>", "cams ...", "pts ...",
//           "cov <path> <ok>", "R <9>", "P <9>": the covariance of camera ccov's rotation and position block at the end point
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "stba/ceres.h"

namespace ceres = stba_ceres;

static int device_mode(const char* path, const std::string& mode) {
    FILE* f = std::fopen(path, "r");
    if (!f) return 2;
    int nc, np, no, npr, ne, ccov;
    if (std::fscanf(f, "%d %d %d %d %d %d", &nc, &np, &no, &npr, &ne, &ccov) != 6) return 2;
    std::vector<double> cams((size_t)nc * 7), pts((size_t)np * 3), feat((size_t)no * 2), pose((size_t)npr * 7), W((size_t)npr * 36);
    std::vector<double> meas((size_t)ne * 7), We((size_t)ne * 36);
    std::vector<int> oc((size_t)no), op((size_t)no), pc((size_t)npr), ei((size_t)ne), ej((size_t)ne);
    for (double& v : cams) if (std::fscanf(f, "%lf", &v) != 1) return 2;
    for (double& v : pts) if (std::fscanf(f, "%lf", &v) != 1) return 2;
    for (int i = 0; i < no; ++i) if (std::fscanf(f, "%d %d %lf %lf", &oc[i], &op[i], &feat[2 * i], &feat[2 * i + 1]) != 4) return 2;
    for (int k = 0; k < npr; ++k) {
        if (std::fscanf(f, "%d", &pc[k]) != 1) return 2;
        for (int j = 0; j < 7; ++j) if (std::fscanf(f, "%lf", &pose[(size_t)k * 7 + j]) != 1) return 2;
        for (int j = 0; j < 36; ++j) if (std::fscanf(f, "%lf", &W[(size_t)k * 36 + j]) != 1) return 2;
    }
    for (int k = 0; k < ne; ++k) {
        if (std::fscanf(f, "%d %d", &ei[k], &ej[k]) != 2) return 2;
        for (int j = 0; j < 7; ++j) if (std::fscanf(f, "%lf", &meas[(size_t)k * 7 + j]) != 1) return 2;
        for (int j = 0; j < 36; ++j) if (std::fscanf(f, "%lf", &We[(size_t)k * 36 + j]) != 1) return 2;
    }
    std::fclose(f);
    const std::vector<double> cams0 = cams, pts0 = pts;
    ceres::Problem problem;
    for (int c = 0; c < nc; ++c) {
        problem.AddParameterBlock(&cams[(size_t)c * 7], 4, new ceres::QuaternionRightPlus);
        problem.AddParameterBlock(&cams[(size_t)c * 7 + 4], 3);
    }
    // the edge and prior blocks sit BETWEEN the observations' blocks (an edge behind every 5th observation from the 2nd on, a prior
    // behind every 7th from the 3rd on, the rest behind them all)
    int kp = 0, ke = 0;
    auto add_prior = [&]() {
        const int c = pc[kp];
        problem.AddResidualBlock(ceres::PosePriorFactor::Create(&pose[(size_t)kp * 7], &pose[(size_t)kp * 7 + 4], &W[(size_t)kp * 36]), nullptr,
                                 &cams[(size_t)c * 7], &cams[(size_t)c * 7 + 4]);
        ++kp;
    };
    auto add_edge = [&]() {
        const int i = ei[ke], j = ej[ke];
        problem.AddResidualBlock(ceres::CameraRelativePoseFactor::Create(&meas[(size_t)ke * 7], &meas[(size_t)ke * 7 + 4], &We[(size_t)ke * 36]), nullptr,
                                 &cams[(size_t)i * 7], &cams[(size_t)i * 7 + 4], &cams[(size_t)j * 7], &cams[(size_t)j * 7 + 4]);
        ++ke;
    };
    for (int i = 0; i < no; ++i) {
        if (i >= 3 && i % 7 == 3 && kp < npr) add_prior();
        if (i >= 2 && i % 5 == 2 && ke < ne) add_edge();
        problem.AddResidualBlock(ceres::ReprojectionFactor::Create(&feat[2 * i]), nullptr, &cams[(size_t)oc[i] * 7], &cams[(size_t)oc[i] * 7 + 4],
                                 &pts[(size_t)op[i] * 3]);
    }
    while (kp < npr) add_prior();
    while (ke < ne) add_edge();
    ceres::Solver::Options o;
    o.num_threads = 1;
    if (mode == "iterative") o.linear_solver_type = ceres::ITERATIVE_SCHUR;
    if (mode == "dogleg") o.trust_region_strategy_type = ceres::DOGLEG;
    if (mode == "inner") o.use_inner_iterations = true;
    if (mode == "callback") o.force_callback_path = true;
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
        const double* q = &cams[(size_t)ccov * 7];
        std::vector<std::pair<const double*, const double*>> blocks = {{q, q}, {q + 4, q + 4}};
        const bool ok = cov.Compute(blocks, &problem);
        std::printf("cov %s %d\n", cov.execution_path().empty() ? "none" : cov.execution_path().c_str(), ok ? 1 : 0);
        double R[9], P[9];
        if (ok && cov.GetCovarianceBlockInTangentSpace(q, q, R) && cov.GetCovarianceBlock(q + 4, q + 4, P)) {
            std::printf("R"); for (double v : R) std::printf(" %.17g", v);
            std::printf("\nP"); for (double v : P) std::printf(" %.17g", v);
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
        double meas[7], cam[2][7], W[36];
        int has_w = 0;
        for (double& v : meas) if (std::scanf("%lf", &v) != 1) return 2;
        for (int s = 0; s < 2; ++s) for (double& v : cam[s]) if (std::scanf("%lf", &v) != 1) return 2;
        if (std::scanf("%d", &has_w) != 1) return 2;
        for (double& v : W) if (std::scanf("%lf", &v) != 1) return 2;
        ceres::CostFunction* f = ceres::CameraRelativePoseFactor::Create(meas, meas + 4, has_w ? W : nullptr);
        const double* prm[4] = {cam[0], cam[0] + 4, cam[1], cam[1] + 4};
        double r[6], r2[6], Jq[2][24], Jt[2][18], P[12];
        double* J[4] = {Jq[0], Jt[0], Jq[1], Jt[1]};
        if (!f->Evaluate(prm, r, J) || !f->Evaluate(prm, r2, nullptr)) return 3;
        for (int i = 0; i < 6; ++i) if (r[i] != r2[i]) return 4;
        for (int i = 0; i < 6; ++i) std::printf("%.17g ", r[i]);
        for (int s = 0; s < 2; ++s) {
            ceres::QuaternionRightPlus().ComputeJacobian(cam[s], P);
            for (int i = 0; i < 6; ++i) {
                for (int a = 0; a < 3; ++a) {
                    double v = 0.0;
                    for (int g = 0; g < 4; ++g) v += Jq[s][i * 4 + g] * P[g * 3 + a];
                    std::printf("%.17g ", v);
                }
                for (int a = 0; a < 3; ++a) std::printf("%.17g ", Jt[s][i * 3 + a]);
            }
        }
        std::printf("\n");
        delete f;
    }
    int detect[5];
    for (int variant = 0; variant < 5; ++variant) {
        double q[3][4] = {{0, 0, 0, 1}, {0, 0.1, 0, 0.99498743710662}, {0, 0, 0, 1}}, t[3][3] = {{0, 0, 0}, {1, 0, 0}, {2, 0, 0}};
        double Lm[2][3] = {{0.1, 0.2, 4}, {-0.3, 0.1, 5}};
        const double feat[4][2] = {{0.01, 0.02}, {0.03, 0.04}, {0.05, 0.06}, {0.07, 0.08}};
        const double zq[4] = {0, 0.1, 0, 0.99498743710662}, zt[3] = {1, 0, 0};
        ceres::Problem problem;
        for (int c = 0; c < 3; ++c) {
            problem.AddParameterBlock(q[c], 4, new ceres::QuaternionRightPlus);
            problem.AddParameterBlock(t[c], 3);
        }
        int nb = 0;
        for (int c = 0; c < 2; ++c)
            for (int j = 0; j < 2; ++j) {
                problem.AddResidualBlock(ceres::ReprojectionFactor::Create(feat[c * 2 + j]), nullptr, q[c], t[c], Lm[j]);
                if (++nb != 3) continue;             // (the edge's block sits behind the third observation's: both cameras are known by then)
                auto* e = ceres::CameraRelativePoseFactor::Create(zq, zt);
                if (variant == 0) delete e;
                if (variant == 1) problem.AddResidualBlock(e, nullptr, q[1], t[1], q[0], t[0]);
                if (variant == 2) problem.AddResidualBlock(e, nullptr, q[0], t[1], q[1], t[0]);
                if (variant == 3) problem.AddResidualBlock(e, nullptr, q[0], t[0], q[2], t[2]);
                if (variant == 4) problem.AddResidualBlock(e, new ceres::HuberLoss(1.0), q[0], t[0], q[1], t[1]);
            }
        ceres::internal::BaLayout L;
        bool ok = ceres::internal::DetectBa(problem, &L);
        if (ok && variant == 0) ok = L.obs_res.empty() && L.rel_i.empty() && L.obs_cam.size() == 4;
        if (ok && variant == 1) {
            // four observations at residual blocks 0, 1, 2, 4 with their features in place, one edge from camera 1 to camera 0
            ok = L.obs_cam.size() == 4 && L.obs_res == std::vector<int>({0, 1, 2, 4}) && L.rel_i == std::vector<int>({1}) &&
                 L.rel_j == std::vector<int>({0}) && L.rel_meas.size() == 7 && L.rel_w.size() == 36 && L.prior_cam.empty() && L.feat.size() == 8 &&
                 L.user.size() == 4;
            for (int i = 0; ok && i < 4; ++i) ok = L.feat[2 * i] == feat[i][0] && L.feat[2 * i + 1] == feat[i][1] && L.obs_cam[i] == i / 2 && L.obs_pt[i] == i % 2;
        }
        detect[variant] = ok ? 1 : 0;
    }
    std::printf("detect %d %d %d %d %d\n", detect[0], detect[1], detect[2], detect[3], detect[4]);
    return 0;
}
