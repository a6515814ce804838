// Edge::setInformation through include/stba/g2o.h, for tests/test_ba_information_shim_cpu.py (compiled with -DSTBA_STAND_IN: the C ABI
// functions g2o.h calls are defined HERE and record what they are given; no library, no device) and
// tests/test_gpu_ba_information_shim.py (linked with the library).  The reference's vertex and edge classes as
// tests/cpp/test_g2o_shim.cpp restates them (included, its main renamed), a scene file in that driver's format, and
//   test_g2o_information_shim <scene> <mode> <delta> <iterations>
// mode: identity   setInformation(1.0) on even edges, an identity Mat2 on odd ones
//       four       setInformation(4.0) on every edge
//       scalars    setInformation(w_k), w_k = 0.5 + 0.25 (k mod 7)
//       matrices   setInformation(Mat2{a, b, b, c}), a = 1 + 0.5 (k mod 5), b = 0.3 ((k mod 4) - 1.5), c = 2 + (k mod 3) -- a type of the
//                  caller's with operator()(i, j), as Eigen spells it
//       notspd     matrices, but edge n / 2 gets {1, 2, 2, 1}
// delta > 0: RobustKernelHuber(delta) on every even edge.  Prints "g2o_iters <n> chi2 <c> msg [<message>]", "g2o_cams ...", "g2o_pts ...",
// "edge_information <k> ..." for three edges (the accessor) and, with the stand-in, "set_information_calls <n>" and "information ...".
#define main g2o_shim_main
#include "test_g2o_shim.cpp"
#undef main

struct Mat2 {
    double m[4];
    double operator()(int i, int j) const { return m[i * 2 + j]; }
};

#ifdef STBA_STAND_IN
// ---- the stand-in: what g2o.h calls, recording the weights; the "solve" leaves the parameters where they are
struct stba_ba { int nc, np, no; std::vector<double> cams, pts; };
static int g_information_calls = 0, g_loss_calls = 0;
static std::vector<double> g_information;
extern "C" {
const char* stba_last_error(void) { return ""; }
void stba_lm_default_options(stba_lm_options* o) { std::memset(o, 0, sizeof *o); }
int stba_ba_create(stba_ba** out, int nc, int np, int no, const double* cams, const double* pts, const int*, const int*, const double*,
                   const unsigned char*, const unsigned char*, void*) {
    *out = new stba_ba{nc, np, no, std::vector<double>(cams, cams + nc * 7), std::vector<double>(pts, pts + np * 3)};
    return STBA_OK;
}
int stba_ba_destroy(stba_ba* b) { delete b; return STBA_OK; }
int stba_ba_set_information(stba_ba* b, const double* information) {
    ++g_information_calls;
    g_information.assign(information, information + (size_t)b->no * 4);
    return STBA_OK;
}
int stba_ba_set_loss(stba_ba*, const int*, const double*, const double*, const double*) { ++g_loss_calls; return STBA_OK; }
int stba_ba_solve(stba_ba*, const stba_lm_options*, stba_lm_summary* s, double*, stba_iteration_callback, void*) {
    std::memset(s, 0, sizeof *s);
    s->num_iterations = 1;
    return STBA_OK;
}
int stba_ba_get_params(stba_ba* b, double* cams, double* pts) {
    std::memcpy(cams, b->cams.data(), b->cams.size() * 8); std::memcpy(pts, b->pts.data(), b->pts.size() * 8);
    return STBA_OK;
}
}
#endif

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: test_g2o_information_shim <scene> identity|four|scalars|matrices|notspd <delta> <iterations>\n"); return 2; }
    const std::string mode = argv[2];
    const double delta = std::strtod(argv[3], nullptr);
    const int iterations = std::atoi(argv[4]);
    std::ifstream f(argv[1], std::ios::binary);
    int h[3]; f.read((char*)h, sizeof h);
    const int nc = h[0], np = h[1], no = h[2];
    std::vector<double> cams(nc * 7), pts(np * 3), feat(no * 2); std::vector<int> oc(no), op(no); std::vector<unsigned char> fixed(nc);
    f.read((char*)cams.data(), cams.size() * 8); f.read((char*)pts.data(), pts.size() * 8);
    f.read((char*)oc.data(), no * 4); f.read((char*)op.data(), no * 4); f.read((char*)feat.data(), feat.size() * 8); f.read((char*)fixed.data(), nc);
    if (!f) return 2;
    {
        using BlockSolverType = g2o::BlockSolver<g2o::BlockSolverTraits<6, 3>>;
        using LinearSolverType = g2o::LinearSolverCSparse<BlockSolverType::PoseMatrixType>;
        g2o::SparseOptimizer optimizer;
        optimizer.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<BlockSolverType>(g2o::make_unique<LinearSolverType>())));
        std::vector<VertexCamera*> cv;
        std::vector<VertexLandmark*> lv;
        std::vector<EdgeProject*> ev;
        for (int i = 0; i < nc; ++i) {
            OptPose camera; std::memcpy(camera.q, &cams[i * 7], 32); std::memcpy(camera.t, &cams[i * 7 + 4], 24);
            auto* v = new VertexCamera();
            v->setId(i); v->setEstimate(camera); v->setFixed(fixed[i] != 0);
            optimizer.addVertex(v); cv.push_back(v);
        }
        for (int i = 0; i < np; ++i) {
            Vec3 lm; std::memcpy(lm.v, &pts[i * 3], 24);
            auto* v = new VertexLandmark();
            v->setId(i + nc); v->setEstimate(lm); v->setMarginalized(true);
            optimizer.addVertex(v); lv.push_back(v);
        }
        for (int k = 0; k < no; ++k) {                       // (edges in the caller's observation order)
            auto* e = new EdgeProject;
            e->setVertex(0, cv.at(oc[k])); e->setVertex(1, lv.at(op[k]));
            Vec2 z; z.v[0] = feat[k * 2]; z.v[1] = feat[k * 2 + 1];
            e->setMeasurement(z);
            const Mat2 M{{1.0 + 0.5 * (k % 5), 0.3 * ((k % 4) - 1.5), 0.3 * ((k % 4) - 1.5), 2.0 + (k % 3)}};
            if (mode == "identity") { if (k % 2 == 0) e->setInformation(1.0); else e->setInformation(Mat2{{1.0, 0.0, 0.0, 1.0}}); }
            else if (mode == "four") e->setInformation(4.0);
            else if (mode == "scalars") e->setInformation(0.5 + 0.25 * (k % 7));
            else if (mode == "notspd" && k == no / 2) e->setInformation(Mat2{{1.0, 2.0, 2.0, 1.0}});
            else e->setInformation(M);
            if (delta > 0.0 && k % 2 == 0) e->setRobustKernel(new g2o::RobustKernelHuber(delta));
            optimizer.addEdge(e); ev.push_back(e);
        }
        optimizer.initializeOptimization();
        const int it = optimizer.optimize(iterations);
        std::printf("g2o_iters %d chi2 %.17g msg [%s]\n", it, optimizer.chi2(), optimizer.message().c_str());
        std::printf("g2o_cams");
        for (auto* v : cv) { double o[7]; g2o::Traits<OptPose>::get(v->estimate(), o); for (double x : o) std::printf(" %.17g", x); }
        std::printf("\ng2o_pts");
        for (auto* v : lv) for (double x : v->estimate().v) std::printf(" %.17g", x);
        std::printf("\nedge_information");
        for (int k : {0, 1, no - 1}) {
            double raw[4];
            static_cast<const g2o::Edge*>(ev[k])->information_raw(raw);
            if (std::memcmp(raw, ev[k]->information(), sizeof raw) != 0) return 3;
            std::printf(" %d %.17g %.17g %.17g %.17g", k, raw[0], raw[1], raw[2], raw[3]);
        }
        std::printf("\n");
    }
#ifdef STBA_STAND_IN
    std::printf("set_information_calls %d\nset_loss_calls %d\ninformation", g_information_calls, g_loss_calls);
    for (double x : g_information) std::printf(" %.17g", x);
    std::printf("\n");
#endif
    return 0;
}
