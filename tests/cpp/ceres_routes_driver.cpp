// Records what the front door (include/stba/ceres.h) does with a list of tiny problems: one Solve() or one Covariance::Compute()
// per case.  usage: ceres_routes_driver <case file>; a case is one line "name key=value key=value ..." (tests/ceres_route_cases.py).
// stdout, one line per case, tab-separated:  name, term, path, kept (1: every parameter block kept its bits), evals (calls of the
// counting user cost functions' Evaluate), callbacks, iters, cost (%a), the message.  stderr: "@@ name" in front of each case's own.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "stba/ceres.h"
namespace ceres = stba_ceres;

static long g_evals = 0;

// the reprojection factor behind a user's class, residual times w: kind 0 w = 1 (recognised); 1 w = 2 (rejected by the probe); 2 w = 1.5
// once the landmark has moved by between 1e-7 and 0.5 from where it started (right at the probes and the start, wrong at the end)
template <int kKind>
struct UserCost : ceres::SizedCostFunction<2, 4, 3, 3> {
    ceres::ReprojectionFactor f;
    double L0[3];
    UserCost(const double* feat, const double* l0) : f(feat[0], feat[1]) { std::memcpy(L0, l0, sizeof L0); }
    bool Evaluate(double const* const* p, double* r, double** J) const override {
        ++g_evals;
        if (!f.Evaluate(p, r, J)) return false;
        double w = kKind == 1 ? 2.0 : 1.0;
        if (kKind == 2) {
            double m2 = 0;
            for (int k = 0; k < 3; ++k) m2 += (p[2][k] - L0[k]) * (p[2][k] - L0[k]);
            if (m2 > 1e-14 && m2 < 0.25) w = 1.5;
        }
        for (int i = 0; i < 2; ++i) r[i] *= w;
        const int n[3] = {8, 6, 6};
        if (J) for (int b = 0; b < 3; ++b) if (J[b]) for (int i = 0; i < n[b]; ++i) J[b][i] *= w;
        return true;
    }
};
struct BoundCost : ceres::SizedCostFunction<1, 1> {          // 10 - x
    bool Evaluate(double const* const* p, double* r, double** J) const override {
        ++g_evals;
        r[0] = 10.0 - p[0][0];
        if (J && J[0]) J[0][0] = -1.0;
        return true;
    }
};
struct BigCost : ceres::CostFunction {                       // one block of n doubles, r = x[0] - 1
    explicit BigCost(int n) { set_num_residuals(1); mutable_parameter_block_sizes()->push_back(n); }
    bool Evaluate(double const* const* p, double* r, double** J) const override {
        ++g_evals;
        r[0] = p[0][0] - 1.0;
        if (J && J[0]) { std::fill(J[0], J[0] + parameter_block_sizes()[0], 0.0); J[0][0] = 1.0; }
        return true;
    }
};
struct UnknownLoss : ceres::LossFunction {};
struct UserQuatChart : ceres::LocalParameterization {         // the quaternion right-plus behind a user's class
    ceres::QuaternionRightPlus q;
    bool Plus(const double* x, const double* d, double* o) const override { return q.Plus(x, d, o); }
    bool ComputeJacobian(const double* x, double* J) const override { return q.ComputeJacobian(x, J); }
    int GlobalSize() const override { return 4; }
    int LocalSize() const override { return 3; }
};
struct OtherChart : ceres::LocalParameterization {            // 4 -> 3, but q + (d, 0) normalised: not the right-plus
    bool Plus(const double* x, const double* d, double* o) const override {
        double n = 0;
        for (int i = 0; i < 4; ++i) { o[i] = x[i] + (i < 3 ? d[i] : 0.0); n += o[i] * o[i]; }
        for (int i = 0; i < 4; ++i) o[i] /= std::sqrt(n);
        return true;
    }
    bool ComputeJacobian(const double*, double* J) const override {
        std::fill(J, J + 12, 0.0);
        for (int i = 0; i < 3; ++i) J[i * 3 + i] = 1.0;
        return true;
    }
    int GlobalSize() const override { return 4; }
    int LocalSize() const override { return 3; }
};
struct FailingChart : OtherChart {
    bool ComputeJacobian(const double*, double*) const override { return false; }
};
struct Counter : ceres::IterationCallback {
    int calls = 0;
    std::string mode;
    ceres::CallbackReturnType operator()(const ceres::IterationSummary& s) override {
        ++calls;
        if (s.iteration >= 1 && mode == "abort") return ceres::SOLVER_ABORT;
        if (s.iteration >= 1 && mode == "success") return ceres::SOLVER_TERMINATE_SUCCESSFULLY;
        return ceres::SOLVER_CONTINUE;
    }
};

using Spec = std::map<std::string, std::string>;
static std::string Get(const Spec& s, const char* k, const char* dflt) { auto it = s.find(k); return it == s.end() ? dflt : it->second; }
static double Wiggle(int i) { return std::sin(12.9898 * (i + 1)) * 0.5; }        // deterministic "noise" in [-0.5, 0.5]

static ceres::LossFunction* MakeLoss(const std::string& kind) {
    if (kind == "huber") return new ceres::HuberLoss(0.01);
    if (kind == "badhuber") return new ceres::HuberLoss(-1.0);
    if (kind == "cauchy") return new ceres::CauchyLoss(0.02);
    if (kind == "scaled") return new ceres::ScaledLoss(new ceres::CauchyLoss(0.02), 0.7, ceres::TAKE_OWNERSHIP);
    if (kind == "scalednull") return new ceres::ScaledLoss(nullptr, 0.7, ceres::TAKE_OWNERSHIP);
    if (kind == "scaledscaled")
        return new ceres::ScaledLoss(new ceres::ScaledLoss(new ceres::HuberLoss(0.01), 0.5, ceres::TAKE_OWNERSHIP), 0.7, ceres::TAKE_OWNERSHIP);
    return new UnknownLoss;
}

// everything a case owns; the parameter blocks live in `x` (never reallocated after Build)
struct Case {
    ceres::Problem problem;
    std::vector<double> x;
    std::vector<double*> cam_q, cam_t, pts, poses;
    double* scalar = nullptr;
    double* extra = nullptr;       // a parameter block no residual block uses
    double foreign[3] = {0, 0, 0};   // not a parameter block at all
};

static void BuildBa(const Spec& s, Case* c) {
    const int nc = 3, np = 8;
    c->x.assign((size_t)nc * 7 + np * 3 + 3, 0.0);
    double* at = c->x.data();
    std::vector<double> truth(c->x.size());
    for (int i = 0; i < nc; ++i) {
        const double d[3] = {0.02 * i, 0.05 * i, -0.01 * i}, q0[4] = {0, 0, 0, 1};
        ceres::QuaternionRightPlus().Plus(q0, d, at);
        c->cam_q.push_back(at); at += 4;
        at[0] = 0.5 * i; at[1] = 0.02 * i; at[2] = 0.0;
        c->cam_t.push_back(at); at += 3;
    }
    for (int j = 0; j < np; ++j) {
        at[0] = -1.0 + 0.4 * j; at[1] = 0.3 * ((j % 3) - 1); at[2] = 4.0 + 0.25 * (j % 4);
        c->pts.push_back(at); at += 3;
    }
    c->extra = at;
    truth = c->x;
    // the start: landmarks and the free camera parts moved off the truth
    for (int j = 0; j < np; ++j) for (int k = 0; k < 3; ++k) c->pts[j][k] += 0.06 * Wiggle(j * 3 + k);
    for (int k = 0; k < 3; ++k) c->cam_t[2][k] += 0.04 * Wiggle(100 + k);
    const std::string prob = Get(s, "prob", "builtin"), chart = Get(s, "chart", "quat"), loss = Get(s, "loss", "none");
    const std::string weighted = Get(s, "weighted", "0"), prior = Get(s, "prior", "0"), rel = Get(s, "rel", "0");
    for (int i = 0; i < nc; ++i) {
        ceres::LocalParameterization* lp = chart == "user" ? (ceres::LocalParameterization*)new UserQuatChart
                                           : chart == "other" ? (ceres::LocalParameterization*)new OtherChart
                                           : chart == "failjac" ? (ceres::LocalParameterization*)new FailingChart : new ceres::QuaternionRightPlus;
        c->problem.AddParameterBlock(c->cam_q[i], 4, lp);
        c->problem.AddParameterBlock(c->cam_t[i], 3);
    }
    const double W2[4] = {1.5, 0.1, 0.0, 0.8};
    double W6[36] = {0};
    for (int a = 0; a < 6; ++a) { W6[a * 7] = 2.0 + 0.1 * a; if (a) W6[a * 6 + a - 1] = 0.05; }
    auto add_special = [&](bool first) {
        // (a prior / relative-pose block in front of the observations and another behind them: observation k is no longer block k)
        if (prior != "0" && first)
            c->problem.AddResidualBlock(new ceres::PosePriorFactor(&truth[7], &truth[7 + 4], prior == "w" ? W6 : nullptr),
                                        prior == "loss" ? MakeLoss("huber") : nullptr, c->cam_q[1], c->cam_t[prior == "mismatch" ? 2 : 1]);
        if (rel != "0" && !first) {
            double a[7], b[7], ai[7], z[7];
            std::memcpy(a, &truth[7], sizeof a); std::memcpy(b, &truth[14], sizeof b);
            ceres::se3::Inverse(a, ai); ceres::se3::Compose(ai, b, z);
            if (rel == "same")
                c->problem.AddResidualBlock(new ceres::CameraRelativePoseFactor(z, z + 4), nullptr, c->cam_q[1], c->cam_t[1], c->cam_q[1], c->cam_t[1]);
            else
                c->problem.AddResidualBlock(new ceres::CameraRelativePoseFactor(z, z + 4, rel == "w" ? W6 : nullptr),
                                            rel == "loss" ? MakeLoss("huber") : nullptr, c->cam_q[1], c->cam_t[1], c->cam_q[2], c->cam_t[2]);
        }
    };
    add_special(true);
    int k = 0;
    for (int j = 0; j < np; ++j)
        for (int i = 0; i < nc; ++i, ++k) {
            double feat[2];
            ceres::internal::ReprojectionAt(&truth[(size_t)i * 7], &truth[(size_t)i * 7 + 4], &truth[(size_t)nc * 7 + j * 3], feat);
            feat[0] += 0.004 * Wiggle(200 + 2 * k); feat[1] += 0.004 * Wiggle(201 + 2 * k);
            if (k == 5) feat[0] += 0.02;         // one outlier, so that a loss has something to do
            ceres::CostFunction* cost;
            const bool w = weighted == "all" || ((weighted == "some" || weighted == "nan") && k >= 4 && k % 3 == 1);
            const double Wn[4] = {1.5, std::nan(""), 0.0, 0.8};
            if (prob == "user") cost = new UserCost<0>(feat, c->pts[j]);
            else if (prob == "scaled") cost = new UserCost<1>(feat, c->pts[j]);
            else if (prob == "moved") cost = new UserCost<2>(feat, c->pts[j]);
            else if (prob == "mixed" && k % 2) cost = new UserCost<0>(feat, c->pts[j]);
            else cost = w ? new ceres::ReprojectionFactor(feat, weighted == "nan" && k == 7 ? Wn : W2) : new ceres::ReprojectionFactor(feat[0], feat[1]);
            ceres::LossFunction* l = nullptr;
            if (loss != "none" && (Get(s, "loss_on", "all") == "all" || (k >= 3 && k % 2 == 1))) l = MakeLoss(loss);
            c->problem.AddResidualBlock(cost, l, c->cam_q[i], c->cam_t[i], c->pts[j]);
        }
    add_special(false);
    if (Get(s, "gaugefree", "0") != "1") {
        c->problem.SetParameterBlockConstant(c->cam_q[0]);
        c->problem.SetParameterBlockConstant(c->cam_t[0]);
        c->problem.SetParameterBlockConstant(c->cam_t[1]);
    }
    if (Get(s, "bounded", "0") == "1") { c->problem.SetParameterLowerBound(c->pts[0], 2, 0.5); c->problem.SetParameterUpperBound(c->pts[0], 2, 50.0); }
    if (Get(s, "constpt", "0") == "1") c->problem.SetParameterBlockConstant(c->pts[1]);
    if (Get(s, "extra", "0") == "1") c->problem.AddParameterBlock(c->extra, 3);
}

static void BuildPg(const Spec& s, Case* c) {
    const int n = 5;
    c->x.assign((size_t)n * 7 + 3, 0.0);
    std::vector<double> truth(c->x.size());
    for (int i = 0; i < n; ++i) {
        const double a = 2.0 * 3.141592653589793 * i / n;
        const double d[6] = {2.0 * std::cos(a), 2.0 * std::sin(a), 0.1 * i, 0.02 * i, -0.03 * i, a};
        ceres::se3::Exp(d, &truth[(size_t)i * 7]);
    }
    for (int i = 0; i < n; ++i) {
        double d[6];
        for (int k = 0; k < 6; ++k) d[k] = i ? 0.08 * Wiggle(300 + i * 6 + k) : 0.0;
        ceres::SE3RightPlus().Plus(&truth[(size_t)i * 7], d, &c->x[(size_t)i * 7]);
        c->poses.push_back(&c->x[(size_t)i * 7]);
    }
    c->extra = &c->x[(size_t)n * 7];
    const std::string chart = Get(s, "chart", "se3"), loss = Get(s, "loss", "none"), weighted = Get(s, "weighted", "0");
    for (int i = 0; i < n; ++i) {
        if (chart == "none") c->problem.AddParameterBlock(c->poses[i], 7);
        else c->problem.AddParameterBlock(c->poses[i], 7, new ceres::SE3RightPlus);
    }
    double W6[36] = {0};
    for (int a = 0; a < 6; ++a) { W6[a * 7] = 1.5 + 0.1 * a; if (a) W6[a * 6 + a - 1] = 0.05; }
    for (int e = 0; e < n; ++e) {                  // the ring 0-1-2-3-4-0: one loop
        const int i = e, j = (e + 1) % n;
        double ti[7], z[7], dz[6], zn[7];
        ceres::se3::Inverse(&truth[(size_t)i * 7], ti);
        ceres::se3::Compose(ti, &truth[(size_t)j * 7], z);
        for (int k = 0; k < 6; ++k) dz[k] = 0.01 * Wiggle(400 + e * 6 + k) + (e == 3 && k == 0 ? 0.3 : 0.0);      // (edge 3: an outlier)
        ceres::SE3RightPlus().Plus(z, dz, zn);
        const bool w = weighted == "all" || ((weighted == "some" || weighted == "nan") && e >= 2 && e != 3);
        if (weighted == "nan" && e == 2) W6[1] = std::nan("");
        ceres::LossFunction* l = nullptr;
        if (loss != "none" && (Get(s, "loss_on", "all") == "all" || e == 2 || e == 3)) l = MakeLoss(loss);
        c->problem.AddResidualBlock(w ? new ceres::RelativePoseFactor(zn, W6) : new ceres::RelativePoseFactor(zn), l, c->poses[i], c->poses[j]);
    }
    if (Get(s, "gaugefree", "0") != "1") c->problem.SetParameterBlockConstant(c->poses[0]);
    if (Get(s, "bounded", "0") == "1") c->problem.SetParameterLowerBound(c->poses[1], 4, -100.0);
    if (Get(s, "extra", "0") == "1") c->problem.AddParameterBlock(c->extra, 3);
}

static void Build(const Spec& s, Case* c) {
    const std::string prob = Get(s, "prob", "builtin");
    if (prob == "pg") return BuildPg(s, c);
    if (prob == "bound" || prob == "empty" || prob == "big") {
        c->x.assign(prob == "big" ? 5000 : 4, 0.0);
        c->scalar = c->x.data();
        c->extra = c->x.data() + 1;
        if (prob == "empty") { c->problem.AddParameterBlock(c->scalar, 1); return; }
        if (prob == "big") { c->problem.AddResidualBlock(new BigCost(5000), nullptr, c->scalar); return; }
        const std::string loss = Get(s, "loss", "none");
        c->problem.AddResidualBlock(new BoundCost, loss == "none" ? nullptr : MakeLoss(loss), c->scalar);
        if (Get(s, "bounded", "1") == "1") c->problem.SetParameterUpperBound(c->scalar, 0, 3.0);
        if (Get(s, "extra", "0") == "1") c->problem.AddParameterBlock(c->extra, 1);
        return;
    }
    BuildBa(s, c);
}

static ceres::Solver::Options MakeOptions(const Spec& s, Case* c, Counter* counter) {
    ceres::Solver::Options o;
    o.max_num_iterations = std::atoi(Get(s, "maxit", "20").c_str());
    const std::string ls = Get(s, "ls", "sparse_schur"), pc = Get(s, "pc", "jacobi"), tr = Get(s, "tr", "lm"), inner = Get(s, "inner", "off");
    o.linear_solver_type = ls == "iterative_schur" ? ceres::ITERATIVE_SCHUR : ls == "dense_qr" ? ceres::DENSE_QR : ceres::SPARSE_SCHUR;
    o.preconditioner_type = pc == "identity" ? ceres::IDENTITY : pc == "jacobi" ? ceres::JACOBI : pc == "schur_jacobi" ? ceres::SCHUR_JACOBI
                            : pc == "cluster_jacobi" ? ceres::CLUSTER_JACOBI : pc == "cluster_tridiagonal" ? ceres::CLUSTER_TRIDIAGONAL : ceres::SUBSET;
    if (tr != "lm") { o.trust_region_strategy_type = ceres::DOGLEG; o.dogleg_type = tr == "subspace" ? ceres::SUBSPACE_DOGLEG : ceres::TRADITIONAL_DOGLEG; }
    o.bundle_adjustment_losses = Get(s, "ba_losses", "0") == "1";
    o.force_callback_path = Get(s, "force", "0") == "1";
    o.num_threads = std::atoi(Get(s, "threads", "1").c_str());
    const std::string cb = Get(s, "cb", "0");
    if (cb != "0") { counter->mode = cb; o.callbacks.push_back(counter); o.update_state_every_iteration = cb == "state"; }
    if (inner != "off") {
        o.use_inner_iterations = true;
        if (inner == "negtol") o.inner_iteration_tolerance = -1.0;
        if (inner != "default" && inner != "negtol" && !c->pts.empty()) {
            auto ord = std::make_shared<ceres::ParameterBlockOrdering>();
            for (double* p : c->pts) ord->AddElementToGroup(p, 0);
            for (size_t i = 0; i < c->cam_q.size(); ++i) { ord->AddElementToGroup(c->cam_q[i], 1); ord->AddElementToGroup(c->cam_t[i], 2); }
            if (inner == "dep_cam") ord->AddElementToGroup(c->cam_t[2], 1);          // a camera's rotation and position in one group
            if (inner == "dep_pt") ord->AddElementToGroup(c->pts[3], 1);             // a landmark in the group of the rotations that see it
            if (inner == "foreign") ord->AddElementToGroup(c->foreign, 0);
            if (inner == "partial") ord->Remove(c->cam_q[2]);                        // a block that is not swept
            o.inner_iteration_ordering = ord;
        }
    }
    return o;
}

using Pairs = std::vector<std::pair<const double*, const double*>>;
static Pairs MakePairs(const Spec& s, Case* c) {
    Pairs out;
    std::stringstream kinds(Get(s, "pairs", "self"));
    std::string kind;
    const bool ba = !c->cam_q.empty(), pg = !c->poses.empty();
    while (std::getline(kinds, kind, '+')) {
        if (kind == "none") continue;
        if (kind == "foreign") out.push_back({c->foreign, c->foreign});
        else if (kind == "extra") out.push_back({c->extra, c->extra});
        else if (ba && kind == "self") { out.push_back({c->cam_q[1], c->cam_q[1]}); out.push_back({c->cam_q[1], c->cam_t[2]}); out.push_back({c->cam_t[0], c->cam_q[2]}); out.push_back({c->pts[2], c->pts[2]}); }
        else if (ba && kind == "campt") { out.push_back({c->cam_q[1], c->pts[0]}); out.push_back({c->pts[3], c->cam_t[2]}); }
        else if (ba && kind == "ptpt") out.push_back({c->pts[0], c->pts[1]});
        else if (pg) { out.push_back({c->poses[1], c->poses[1]}); out.push_back({c->poses[1], c->poses[3]}); out.push_back({c->poses[0], c->poses[2]}); }
        else out.push_back({c->scalar, c->scalar});
    }
    return out;
}

static std::string OneLine(std::string m) { for (char& ch : m) if (ch == '\n' || ch == '\t') ch = ' '; return m; }

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::stringstream ss(line);
        std::string name, tok;
        if (!(ss >> name) || name[0] == '#') continue;
        Spec s;
        while (ss >> tok) { const size_t eq = tok.find('='); if (eq != std::string::npos) s[tok.substr(0, eq)] = tok.substr(eq + 1); }
        std::fflush(stdout);
        std::fprintf(stderr, "@@ %s\n", name.c_str());
        Case c;
        Build(s, &c);
        const std::vector<double> before = c.x;
        g_evals = 0;
        if (Get(s, "kind", "solve") == "solve") {
            Counter counter;
            const ceres::Solver::Options o = MakeOptions(s, &c, &counter);
            ceres::Solver::Summary sum;
            ceres::Solve(o, &c.problem, &sum);
            const bool kept = std::memcmp(before.data(), c.x.data(), before.size() * sizeof(double)) == 0;
            std::printf("%s\t%d\t%s\t%d\t%ld\t%d\t%d\t%a\tinner=%d/%d/%zu/%zu tr=%d ls=%d\t%s\n", name.c_str(), (int)sum.termination_type,
                        sum.execution_path.c_str(), kept ? 1 : 0, g_evals, counter.calls, (int)sum.iterations.size(), sum.final_cost,
                        (int)sum.inner_iterations_given, (int)sum.inner_iterations_used, sum.inner_iteration_ordering_given.size(),
                        sum.inner_iteration_ordering_used.size(), (int)sum.trust_region_strategy_type, (int)sum.linear_solver_type_used,
                        OneLine(sum.message).c_str());
        } else {
            ceres::Covariance::Options co;
            co.bundle_adjustment_losses = Get(s, "ba_losses", "0") == "1";
            co.bundle_adjustment_cross_blocks = Get(s, "cross", "0") == "1";
            co.null_space_rank = std::atoi(Get(s, "nsr", "0").c_str());
            co.apply_loss_function = Get(s, "apply", "1") == "1";
            ceres::Covariance cov(co);
            const Pairs pairs = MakePairs(s, &c);
            const bool ok = cov.Compute(pairs, &c.problem);
            const bool kept = std::memcmp(before.data(), c.x.data(), before.size() * sizeof(double)) == 0;
            double sum = 0.0;         // (every requested block in the tangent space, summed: one number that any block would move)
            int got = 0;
            for (auto& pr : pairs) {
                double blk[49] = {0};
                if (ok && cov.GetCovarianceBlockInTangentSpace(pr.first, pr.second, blk)) { ++got; for (double v : blk) sum += v; }
            }
            std::printf("%s\t%d\t%s\t%d\t%ld\t%d\t%d\t%a\t-\t%s\n", name.c_str(), ok ? 1 : 0, cov.execution_path().c_str(), kept ? 1 : 0, g_evals,
                        got, 0, sum, OneLine(cov.message()).c_str());
        }
    }
    std::fflush(stdout);
    return 0;
}
