// ceres::Covariance through include/stba/ceres.h: the host-side refusals (no device needed) and, with a device, the covariance of a
// small synthetic bundle adjustment printed for tests/test_covariance_shim.py.
//   test_covariance refuse     -- loss, null_space_rank, landmark pairs: refused before any device work, parameters untouched
//   test_covariance nodevice   -- a valid request on a machine without a device: Compute returns false with a message
//   test_covariance device     -- the same request with a device
// and, for tests/test_gpu_covariance_shim.py (blocks printed as "T <block a> <block b> values..." in the tangent space,
// "A ..." in the ambient space, blocks named q<c> / t<c> / L<j> / x):
//   test_covariance ba <scene> <kind>   -- the st20 call site (test_ceres.h:98-152) with the built-in factor (kind 0), the user's
//                                          ProjectFactor (1: recognised, "gpu-ba") or a factor the probe rejects (2: "gpu-ba-hostjac")
//   test_covariance pnp <file>          -- the st17 PnP problem (solver.hpp:247-290): "gpu-dense"
//   test_covariance curve <file>        -- the C1 parabola fit: "gpu-dense"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "stba/ceres.h"
namespace ceres = stba_ceres;

struct Scene {
    std::vector<double> q, t, L;       // 4 | 3 per camera, 3 per landmark
    std::vector<int> oc, op;
    std::vector<double> f;
};

static Scene MakeScene(int nc, int np) {
    Scene s;
    for (int c = 0; c < nc; ++c) {
        const double a = 0.05 * c;
        s.q.insert(s.q.end(), {0.0, std::sin(a / 2), 0.0, std::cos(a / 2)});
        s.t.insert(s.t.end(), {0.3 * c, 0.01 * c, -5.0});
    }
    for (int j = 0; j < np; ++j) s.L.insert(s.L.end(), {-1.0 + 0.37 * (j % 6), -1.0 + 0.41 * (j % 5), 0.5 * (j % 3)});
    for (int j = 0; j < np; ++j)
        for (int c = 0; c < nc; ++c) {
            s.oc.push_back(c); s.op.push_back(j);
            s.f.push_back(0.01 * (j + c)); s.f.push_back(-0.02 * j);
        }
    return s;
}

static void Build(Scene& s, ceres::Problem& p, bool with_loss) {
    const int nc = (int)s.q.size() / 4;
    for (int c = 0; c < nc; ++c) p.AddParameterBlock(&s.q[4 * c], 4, new ceres::QuaternionRightPlus());
    for (size_t k = 0; k < s.oc.size(); ++k)
        p.AddResidualBlock(new ceres::ReprojectionFactor(s.f[2 * k], s.f[2 * k + 1]), (with_loss && k == 3) ? new ceres::LossFunction() : nullptr,
                           &s.q[4 * s.oc[k]], &s.t[3 * s.oc[k]], &s.L[3 * s.op[k]]);
    p.SetParameterBlockConstant(&s.q[0]); p.SetParameterBlockConstant(&s.t[0]);
    p.SetParameterBlockConstant(&s.q[4 * (nc - 1)]); p.SetParameterBlockConstant(&s.t[3 * (nc - 1)]);
}

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static bool Refused(Scene& s, bool loss, int null_rank, const std::vector<std::pair<const double*, const double*>>& pairs, const char* needle) {
    const Scene before = s;
    ceres::Problem p;
    Build(s, p, loss);
    ceres::Covariance::Options o;
    o.null_space_rank = null_rank;
    ceres::Covariance cov(o);
    const bool ok = cov.Compute(pairs, &p);
    std::printf("message %s\n", cov.message().c_str());
    const bool untouched = before.q == s.q && before.t == s.t && before.L == s.L;
    return !ok && untouched && cov.message().find(needle) != std::string::npos;
}

// ---- device modes: scenes written by tests/test_gpu_covariance_shim.py
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
// the reprojection factor in front of the camera, doubled behind it: equal to the factor at every observation of the scene (all in
// front), but the probe point behind the camera rejects it -- so the covariance is the same, computed through the host lineariser
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
// the parabola fit (C1): y = a x^2 + b x + c
struct ParabolaFunctor {
    double x, y;
    template <typename T> bool operator()(const T* const abc, T* residual) const {
        residual[0] = T(y) - (abc[0] * T(x) * T(x) + abc[1] * T(x) + abc[2]);
        return true;
    }
};

static void PrintBlock(const char* kind, const std::string& a, const std::string& b, const double* v, int n) {
    std::printf("%s %s %s", kind, a.c_str(), b.c_str());
    for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
    std::printf("\n");
}

static int RunBa(const char* path, int kind) {
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
    ceres::Problem problem;
    for (int c = 0; c < nc; ++c) problem.AddParameterBlock(&q[4 * c], 4, new ceres::QuaternionRightPlus());
    for (int i = 0; i < no; ++i) {
        ceres::CostFunction* cf;
        if (kind == 0) cf = new ceres::ReprojectionFactor(feat[2 * i], feat[2 * i + 1]);
        else {
            ceres::DynamicAutoDiffCostFunction<ProjectFactor>* c1 = nullptr;
            ceres::DynamicAutoDiffCostFunction<BehindScaledProjectFactor>* c2 = nullptr;
            if (kind == 1) { c1 = new ceres::DynamicAutoDiffCostFunction<ProjectFactor>(new ProjectFactor(&feat[2 * i])); cf = c1; }
            else { c2 = new ceres::DynamicAutoDiffCostFunction<BehindScaledProjectFactor>(new BehindScaledProjectFactor(&feat[2 * i])); cf = c2; }
            for (int k : {4, 3, 3}) { if (c1) c1->AddParameterBlock(k); else c2->AddParameterBlock(k); }
            if (c1) c1->SetNumResiduals(2); else c2->SetNumResiduals(2);
        }
        problem.AddResidualBlock(cf, nullptr, &q[4 * oc[i]], &t[3 * oc[i]], &pts[3 * op[i]]);
    }
    for (int c = 0; c < nc; ++c)
        if (fixed[c]) { problem.SetParameterBlockConstant(&q[4 * c]); problem.SetParameterBlockConstant(&t[3 * c]); }   // test_ceres.h:127-130
    std::vector<std::pair<const double*, const double*>> pairs;
    std::vector<std::pair<std::string, std::string>> names;
    auto add = [&](const double* a, const std::string& na, const double* b, const std::string& nb) { pairs.push_back({a, b}); names.push_back({na, nb}); };
    for (int c = 0; c < nc; ++c) {
        const std::string qc = "q" + std::to_string(c), tc = "t" + std::to_string(c);
        add(&q[4 * c], qc, &q[4 * c], qc); add(&q[4 * c], qc, &t[3 * c], tc); add(&t[3 * c], tc, &t[3 * c], tc);
    }
    for (int c = 0; c < 10; ++c) {
        const int d = (7 * c + 3) % nc;
        add(&q[4 * c], "q" + std::to_string(c), &t[3 * d], "t" + std::to_string(d));
        add(&t[3 * d], "t" + std::to_string(d), &q[4 * c], "q" + std::to_string(c));
    }
    for (int j = 0; j < np; ++j) add(&pts[3 * j], "L" + std::to_string(j), &pts[3 * j], "L" + std::to_string(j));
    ceres::Covariance cov{ceres::Covariance::Options()};
    const bool ok = cov.Compute(pairs, &problem);
    std::printf("path %s\nok %d\n", cov.execution_path().c_str(), ok ? 1 : 0);
    if (!ok) return 1;
    double v[16];
    for (size_t k = 0; k < pairs.size(); ++k) {
        if (!cov.GetCovarianceBlockInTangentSpace(pairs[k].first, pairs[k].second, v)) return 1;
        PrintBlock("T", names[k].first, names[k].second, v, 9);
        if (names[k].first[0] == 'q' && names[k].first == names[k].second) {
            if (!cov.GetCovarianceBlock(pairs[k].first, pairs[k].second, v)) return 1;
            PrintBlock("A", names[k].first, names[k].second, v, 16);
        }
    }
    return 0;
}

static int RunDense(const char* path, bool pnp) {
    std::ifstream f(path, std::ios::binary);
    int n = 0;
    if (!f.read((char*)&n, sizeof n)) return 2;
    std::vector<double> x(pnp ? 7 : 3), data((size_t)n * (pnp ? 5 : 2));
    f.read((char*)x.data(), x.size() * 8); f.read((char*)data.data(), data.size() * 8);
    if (!f) return 2;
    ceres::Problem problem;
    ceres::Covariance cov{ceres::Covariance::Options()};
    bool ok;
    double v[16];
    if (pnp) {
        problem.AddParameterBlock(&x[0], 4, new ceres::QuaternionRightPlus());
        for (int i = 0; i < n; ++i) {
            auto* fn = new PnPFunctor{{data[5 * i], data[5 * i + 1], data[5 * i + 2]}, {data[5 * i + 3], data[5 * i + 4]}};
            problem.AddResidualBlock(new ceres::AutoDiffCostFunction<PnPFunctor, 2, 4, 3>(fn), nullptr, &x[0], &x[4]);
        }
        const double *q = &x[0], *t = &x[4];
        ok = cov.Compute({{q, q}, {q, t}, {t, t}}, &problem);
        std::printf("path %s\nok %d\n", cov.execution_path().c_str(), ok ? 1 : 0);
        if (!ok) return 1;
        const std::pair<const double*, const char*> b[2] = {{q, "q0"}, {t, "t0"}};
        for (auto& a : b) for (auto& c : b) { if (!cov.GetCovarianceBlockInTangentSpace(a.first, c.first, v)) return 1; PrintBlock("T", a.second, c.second, v, 9); }
        if (!cov.GetCovarianceBlock(q, q, v)) return 1;
        PrintBlock("A", "q0", "q0", v, 16);
    } else {
        for (int i = 0; i < n; ++i)
            problem.AddResidualBlock(new ceres::AutoDiffCostFunction<ParabolaFunctor, 1, 3>(new ParabolaFunctor{data[2 * i], data[2 * i + 1]}), nullptr, &x[0]);
        ok = cov.Compute({{&x[0], &x[0]}}, &problem);
        std::printf("path %s\nok %d\n", cov.execution_path().c_str(), ok ? 1 : 0);
        if (!ok) return 1;
        if (!cov.GetCovarianceBlockInTangentSpace(&x[0], &x[0], v)) return 1;
        PrintBlock("T", "x", "x", v, 9);
    }
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "refuse";
    if (mode == "ba" && argc > 3) return RunBa(argv[2], std::atoi(argv[3]));
    if ((mode == "pnp" || mode == "curve") && argc > 2) return RunDense(argv[2], mode == "pnp");
    Scene s = MakeScene(4, 12);
    const double *q1 = &s.q[4], *t1 = &s.t[3], *t2 = &s.t[6], *L0 = &s.L[0], *L1 = &s.L[3];
    if (mode == "refuse") {
        EXPECT(Refused(s, true, 0, {{q1, q1}}, "LossFunction"));
        EXPECT(Refused(s, false, -1, {{q1, q1}}, "null_space_rank"));
        EXPECT(Refused(s, false, 0, {{q1, t2}, {L0, L1}}, "pair 1"));
        EXPECT(Refused(s, false, 0, {{L0, L0}, {t1, L1}}, "pair 1"));
        if (!g_fail) std::printf("refuse ok\n");
    } else if (mode == "nodevice") {
        EXPECT(Refused(s, false, 0, {{q1, q1}, {q1, t2}, {L0, L0}}, "device"));
        if (!g_fail) std::printf("nodevice ok\n");
    } else if (mode == "device") {          // the same request with a device: computed on the built-in factor's route
        ceres::Problem p;
        Build(s, p, false);
        ceres::Covariance cov{ceres::Covariance::Options()};
        EXPECT(cov.Compute({{q1, q1}, {q1, t2}, {L0, L0}}, &p));
        EXPECT(cov.execution_path() == "gpu-ba");
        double a[9], b[9], amb[16];
        EXPECT(cov.GetCovarianceBlockInTangentSpace(q1, t2, a) && cov.GetCovarianceBlockInTangentSpace(t2, q1, b));
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) EXPECT(a[r * 3 + c] == b[c * 3 + r]);
        EXPECT(cov.GetCovarianceBlockInTangentSpace(L0, L0, a) && a[0] > 0 && a[4] > 0 && a[8] > 0);
        EXPECT(cov.GetCovarianceBlock(q1, q1, amb));
        EXPECT(!cov.GetCovarianceBlock(q1, L0, amb));       // (not requested)
        if (!g_fail) std::printf("device ok\n");
    }
    return g_fail ? 1 : 0;
}
