// Robust kernels through include/stba/g2o.h, for tests/test_g2o_loss_shim.py: the reference's vertex and edge classes as
// tests/cpp/test_g2o_shim.cpp restates them (included, its main renamed), a scene file in that driver's format, and
//   test_g2o_loss_shim <scene> huber|cauchy <delta> <iterations>   setRobustKernel(new RobustKernelHuber | RobustKernelCauchy) followed by
//       setDelta(delta) on every even edge (in the caller's observation order), cameras with a fixed flag constant; optimize(iterations)
//   test_g2o_loss_shim <scene> foreign <delta> <iterations>        one edge in the middle carries a RobustKernel subclass of the caller's
// Prints "g2o_iters <n> chi2 <c> msg [<message>]", "g2o_cams ...", "g2o_pts ..." (every landmark) and "kernels <n> owned_deleted <n>".
#define main g2o_shim_main
#include "test_g2o_shim.cpp"
#undef main

static int g_deleted = 0;
struct ForeignKernel : g2o::RobustKernel { ~ForeignKernel() override { ++g_deleted; } };

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: test_g2o_loss_shim <scene> huber|cauchy|foreign <delta> <iterations>\n"); return 2; }
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
    int kernels = 0;
    {
        using BlockSolverType = g2o::BlockSolver<g2o::BlockSolverTraits<6, 3>>;
        using LinearSolverType = g2o::LinearSolverCSparse<BlockSolverType::PoseMatrixType>;
        g2o::SparseOptimizer optimizer;
        optimizer.setAlgorithm(new g2o::OptimizationAlgorithmLevenberg(g2o::make_unique<BlockSolverType>(g2o::make_unique<LinearSolverType>())));
        std::vector<VertexCamera*> cv;
        std::vector<VertexLandmark*> lv;
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
            e->setMeasurement(z); e->setInformation(1.0);
            if (mode == "foreign") {
                if (k == no / 2) { e->setRobustKernel(new ForeignKernel); e->robustKernel()->setDelta(delta); ++kernels; }
            } else if (k % 2 == 0) {
                g2o::RobustKernel* rk = mode == "huber" ? static_cast<g2o::RobustKernel*>(new g2o::RobustKernelHuber) : new g2o::RobustKernelCauchy;
                e->setRobustKernel(rk);
                rk->setDelta(delta);
                if (e->robustKernel() != rk || rk->delta() != delta) return 3;
                ++kernels;
            }
            optimizer.addEdge(e);
        }
        optimizer.initializeOptimization();
        const int it = optimizer.optimize(iterations);
        std::printf("g2o_iters %d chi2 %.17g msg [%s]\n", it, optimizer.chi2(), optimizer.message().c_str());
        std::printf("g2o_cams");
        for (auto* v : cv) { double o[7]; g2o::Traits<OptPose>::get(v->estimate(), o); for (double x : o) std::printf(" %.17g", x); }
        std::printf("\ng2o_pts");
        for (auto* v : lv) for (double x : v->estimate().v) std::printf(" %.17g", x);
        std::printf("\n");
    }   // (the optimizer deletes its edges, the edges their kernels)
    std::printf("kernels %d owned_deleted %d\n", kernels, g_deleted);
    return 0;
}
