// ceres::Covariance through include/stba/ceres.h on a bundle adjustment: the pairs that are not two camera blocks or one landmark
// with itself -- (rotation | position, landmark), (landmark, rotation | position) and two different landmarks -- which
// Covariance::Options::bundle_adjustment_cross_blocks = true switches on (without it they stay refused).
//   test_covariance_cross nodevice        -- such a request on a machine without a device: it is NOT refused as a pair (it gets as far
//                                            as the device), Compute returns false with the device named
//   test_covariance_cross device          -- the same request with a device: computed, swapped pairs are transposes
//   test_covariance_cross ba <scene> <kind> -- for tests/test_gpu_covariance_cross_shim.py: the scene it wrote, with the built-in
//                                            factor (kind 0: "gpu-ba") or a factor the probe rejects (kind 2: "gpu-ba-hostjac");
//                                            blocks printed as "T <a> <b> <rows> <cols> values..." in the tangent space and
//                                            "A ..." in the ambient space, blocks named q<c> / t<c> / L<j>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "stba/ceres.h"
namespace ceres = stba_ceres;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

template <typename T> static void QuatConjRotate(const T* q, const T* v, T* out) {   // conj(q) * v
    const T u0 = -q[0], u1 = -q[1], u2 = -q[2], w = q[3];
    const T a0 = T(2.0) * (u1 * v[2] - u2 * v[1]), a1 = T(2.0) * (u2 * v[0] - u0 * v[2]), a2 = T(2.0) * (u0 * v[1] - u1 * v[0]);
    out[0] = v[0] + w * a0 + (u1 * a2 - u2 * a1);
    out[1] = v[1] + w * a1 + (u2 * a0 - u0 * a2);
    out[2] = v[2] + w * a2 + (u0 * a1 - u1 * a0);
}

// the reprojection factor in front of the camera, doubled behind it: equal to the factor at every observation of the scene (all in
// front), but the probe point behind the camera rejects it -- the same covariance, computed through the host lineariser
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

struct Scene {
    std::vector<double> q, t, L;       // 4 | 3 per camera, 3 per landmark
    std::vector<int> oc, op;
    std::vector<double> f;
    std::vector<unsigned char> fixed;  // per camera
};

// every camera sees every landmark; the first and the last camera are constant
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
    s.fixed.assign(nc, 0);
    s.fixed[0] = s.fixed[nc - 1] = 1;
    return s;
}

static bool ReadScene(const char* path, Scene* s) {
    std::ifstream f(path, std::ios::binary);
    int h[3];
    if (!f.read((char*)h, sizeof h)) return false;
    const int nc = h[0], np = h[1], no = h[2];
    std::vector<double> cams((size_t)nc * 7);
    s->L.resize((size_t)np * 3); s->f.resize((size_t)no * 2); s->oc.resize(no); s->op.resize(no); s->fixed.resize(nc);
    f.read((char*)cams.data(), cams.size() * 8); f.read((char*)s->L.data(), s->L.size() * 8);
    f.read((char*)s->oc.data(), no * 4); f.read((char*)s->op.data(), no * 4); f.read((char*)s->f.data(), s->f.size() * 8);
    f.read((char*)s->fixed.data(), nc);
    if (!f) return false;
    s->q.resize((size_t)nc * 4); s->t.resize((size_t)nc * 3);
    for (int c = 0; c < nc; ++c) { std::memcpy(&s->q[4 * c], &cams[7 * c], 32); std::memcpy(&s->t[3 * c], &cams[7 * c + 4], 24); }
    return true;
}

static void Build(Scene& s, ceres::Problem& p, int kind) {
    const int nc = (int)s.q.size() / 4;
    for (int c = 0; c < nc; ++c) p.AddParameterBlock(&s.q[4 * c], 4, new ceres::QuaternionRightPlus());
    for (size_t i = 0; i < s.oc.size(); ++i) {
        ceres::CostFunction* cf;
        if (kind == 0) cf = new ceres::ReprojectionFactor(s.f[2 * i], s.f[2 * i + 1]);
        else {
            auto* c2 = new ceres::DynamicAutoDiffCostFunction<BehindScaledProjectFactor>(new BehindScaledProjectFactor(&s.f[2 * i]));
            for (int k : {4, 3, 3}) c2->AddParameterBlock(k);
            c2->SetNumResiduals(2);
            cf = c2;
        }
        p.AddResidualBlock(cf, nullptr, &s.q[4 * s.oc[i]], &s.t[3 * s.oc[i]], &s.L[3 * s.op[i]]);
    }
    for (int c = 0; c < nc; ++c)
        if (s.fixed[c]) { p.SetParameterBlockConstant(&s.q[4 * c]); p.SetParameterBlockConstant(&s.t[3 * c]); }
}

static void PrintBlock(const char* kind, const std::string& a, const std::string& b, int rows, int cols, const double* v) {
    std::printf("%s %s %s %d %d", kind, a.c_str(), b.c_str(), rows, cols);
    for (int i = 0; i < rows * cols; ++i) std::printf(" %.17g", v[i]);
    std::printf("\n");
}

static int RunBa(const char* path, int kind) {
    Scene s;
    if (!ReadScene(path, &s)) return 2;
    const int nc = (int)s.q.size() / 4, np = (int)s.L.size() / 3;
    ceres::Problem problem;
    Build(s, problem, kind);
    struct Named { const double* p; std::string name; int size; };
    std::vector<std::pair<Named, Named>> req;
    auto Q = [&](int c) { return Named{&s.q[4 * c], "q" + std::to_string(c), 4}; };
    auto T = [&](int c) { return Named{&s.t[3 * c], "t" + std::to_string(c), 3}; };
    auto L = [&](int j) { return Named{&s.L[3 * j], "L" + std::to_string(j), 3}; };
    const int cams[4] = {1, nc / 2, nc - 2, nc - 1};                    // (the last one is constant)
    const int pts[4] = {0, 3, np / 2, np - 1};
    for (int c : cams)
        for (int j : pts) {
            req.push_back({Q(c), L(j)});              // (rotation, landmark)
            req.push_back({T(c), L(j)});              // (position, landmark)
            req.push_back({L(j), Q(c)});              // (landmark, rotation)
        }
    req.push_back({L(pts[3]), T(cams[0])});           // (landmark, position), not asked for the other way round
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b) { req.push_back({L(pts[a]), L(pts[b])}); req.push_back({L(pts[b]), L(pts[a])}); }
    req.push_back({L(pts[1]), L(pts[1])});            // a marginal and a camera block in the same request
    req.push_back({Q(cams[0]), T(cams[1])});
    std::vector<std::pair<const double*, const double*>> pairs;
    for (auto& r : req) pairs.push_back({r.first.p, r.second.p});
    ceres::Covariance::Options opt;
    opt.bundle_adjustment_cross_blocks = true;
    ceres::Covariance cov{opt};
    const bool ok = cov.Compute(pairs, &problem);
    std::printf("path %s\nok %d\n", cov.execution_path().c_str(), ok ? 1 : 0);
    if (!ok) { std::printf("message %s\n", cov.message().c_str()); return 1; }
    double v[16];
    for (auto& r : req) {
        if (!cov.GetCovarianceBlockInTangentSpace(r.first.p, r.second.p, v)) return 1;
        PrintBlock("T", r.first.name, r.second.name, 3, 3, v);
        if (!cov.GetCovarianceBlock(r.first.p, r.second.p, v)) return 1;
        PrintBlock("A", r.first.name, r.second.name, r.first.size, r.second.size, v);
    }
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "ba" && argc > 3) return RunBa(argv[2], std::atoi(argv[3]));
    if (mode != "nodevice" && mode != "device") {
        std::fprintf(stderr, "usage: test_covariance_cross nodevice | device | ba <scene> <kind>\n");
        return 2;
    }
    Scene s = MakeScene(4, 12);
    const Scene before = s;
    const double *q1 = &s.q[4], *t2 = &s.t[6], *L0 = &s.L[0], *L1 = &s.L[3], *L5 = &s.L[15];
    ceres::Problem p;
    Build(s, p, 0);
    const std::vector<std::pair<const double*, const double*>> request = {{q1, L0}, {L0, q1}, {t2, L5}, {L0, L1}, {L1, L0}, {L5, L5}, {q1, t2}};
    {   // the default stays the refusal, before any device work, with the option named
        ceres::Covariance plain{ceres::Covariance::Options()};
        EXPECT(!plain.Compute(request, &p));
        EXPECT(plain.message().find("pair 0") != std::string::npos && plain.message().find("bundle_adjustment_cross_blocks") != std::string::npos);
    }
    ceres::Covariance::Options opt;
    opt.bundle_adjustment_cross_blocks = true;
    ceres::Covariance cov{opt};
    const bool ok = cov.Compute(request, &p);
    std::printf("message %s\n", cov.message().c_str());
    EXPECT(before.q == s.q && before.t == s.t && before.L == s.L);
    if (mode == "nodevice") {
        EXPECT(!ok);
        EXPECT(cov.message().find("device") != std::string::npos);
        EXPECT(cov.message().find("pair") == std::string::npos);        // (not refused as a request)
        double v[16];
        EXPECT(!cov.GetCovarianceBlockInTangentSpace(q1, L0, v));
    } else {
        EXPECT(ok);
        EXPECT(cov.execution_path() == "gpu-ba");
        double a[9], b[9], amb[12];
        EXPECT(cov.GetCovarianceBlockInTangentSpace(q1, L0, a) && cov.GetCovarianceBlockInTangentSpace(L0, q1, b));
        double na = 0.0;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { EXPECT(a[r * 3 + c] == b[c * 3 + r]); na += a[r * 3 + c] * a[r * 3 + c]; }
        EXPECT(na > 0.0);
        EXPECT(cov.GetCovarianceBlockInTangentSpace(L0, L1, a) && cov.GetCovarianceBlockInTangentSpace(L1, L0, b));
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) EXPECT(a[r * 3 + c] == b[c * 3 + r]);
        EXPECT(cov.GetCovarianceBlockInTangentSpace(L5, t2, a));        // (the swapped pair of a requested one)
        EXPECT(cov.GetCovarianceBlock(q1, L0, amb));                    // 4 x 3
        EXPECT(!cov.GetCovarianceBlock(q1, L1, amb));                   // (not requested)
    }
    if (!g_fail) std::printf("%s ok\n", mode.c_str());
    return g_fail ? 1 : 0;
}
