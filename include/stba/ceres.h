// stba/ceres.h -- the reference's operator API (the slice of the Ceres Solver C++ API that
// Unsigned-Long/slam-tricks uses) as a header-only C++17 layer over the C ABI in stba.h.
//
// A maintainer of the reference switches  #include "ceres/ceres.h"  to
//     #include "stba/ceres.h"
//     namespace ceres = stba_ceres;
// and links libstba.so; call sites keep their shape (INTEGRATION.md shows the diff).
//
// Entry points mirrored (paths relative to /root/reference):
//   CostFunction::Evaluate, SizedCostFunction<2,3,3>        st17-ceres/src/include/solver.hpp:157-212
//   AutoDiffCostFunction<F,2,4,3>, <F,2,3>                  solver.hpp:135, st20-g2o/src/include/sim_data.h:175
//   DynamicAutoDiffCostFunction<F> (+AddParameterBlock/SetNumResiduals)
//                                                           solver.hpp:104,263-265, test_ceres.h:56,112-115,
//                                                           st17-ceres/src/ceres_bound.cpp:14,29-30
//   LocalParameterization {Plus, ComputeJacobian, GlobalSize, LocalSize}
//                                                           solver.hpp:30-94, test_ceres.h:14-45
//   Problem::{AddResidualBlock, AddParameterBlock, SetParameterBlockConstant,
//             SetParameterLowerBound, SetParameterUpperBound}
//                                                           solver.hpp:267-270, test_ceres.h:119-130,
//                                                           ceres_bound.cpp:32,51-53
//   Solver::Options / Summary::BriefReport / Solve / IterationCallback
//                                                           solver.hpp:215-290, test_ceres.h:83-151
//
// Where the work runs.  User CostFunction::Evaluate / autodiff functors are host code and are
// evaluated on the host (as in the reference); everything else -- normal equations, Schur
// complement, Cholesky, LM step -- runs in libstba's HIP kernels:
//   * residual blocks that ARE the reprojection factor of test_ceres.h:47-81 -- either the built-in
//     stba_ceres::ReprojectionFactor or ANY user cost function with blocks {4, 3, 3} -> 2 residuals
//     (the reference's own ns_st20::ProjectFactor behind DynamicAutoDiffCostFunction, test_ceres.h:111-121)
//     that is recognised numerically (internal::ProbeReprojection: its value equals
//     proj(R^T (L - t)) - feature at generic points, its Jet Jacobian equals the closed form)
//     -> fully device-resident BA engine (stba_ba_*): residuals and Jacobians are computed by the
//     HIP kernel too, the user functor is never called during the solve;
//   * a BA-SHAPED problem (every block {4, 3, 3} -> 2, quaternion chart) with any OTHER factor -> the device engine with the
//     user's cost functions evaluated on the host in bulk ("gpu-ba-hostjac", stba_ba_set_host_linearizer);
//   * any other problem -> the callback path of stba_dense_solve (<= 4096 local parameters).
// There is no CPU solver behind this header: without a HIP device Solve() reports FAILURE.
#ifndef STBA_CERES_H
#define STBA_CERES_H

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <thread>
#include <type_traits>
#include <typeindex>
#include <typeinfo>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../stba.h"

namespace stba_ceres {

// ------------------------------------------------------------------------------------------
// forward-mode dual numbers (ceres::Jet)
// ------------------------------------------------------------------------------------------
template <typename T, int N>
struct Jet {
    T a;
    T v[N];
    Jet() : a(T(0)) { for (int i = 0; i < N; ++i) v[i] = T(0); }
    Jet(const T& value) : a(value) { for (int i = 0; i < N; ++i) v[i] = T(0); }   // NOLINT
    Jet(const T& value, int k) : a(value) { for (int i = 0; i < N; ++i) v[i] = T(0); v[k] = T(1); }
    Jet& operator+=(const Jet& y) { *this = *this + y; return *this; }
    Jet& operator-=(const Jet& y) { *this = *this - y; return *this; }
    Jet& operator*=(const Jet& y) { *this = *this * y; return *this; }
    Jet& operator/=(const Jet& y) { *this = *this / y; return *this; }
};
#define STBA_JET_BIN(op, expr_a, expr_v)                                                         \
    template <typename T, int N> inline Jet<T, N> operator op(const Jet<T, N>& f, const Jet<T, N>& g) { \
        Jet<T, N> h; h.a = expr_a; for (int i = 0; i < N; ++i) h.v[i] = expr_v; return h; }
STBA_JET_BIN(+, f.a + g.a, f.v[i] + g.v[i])
STBA_JET_BIN(-, f.a - g.a, f.v[i] - g.v[i])
STBA_JET_BIN(*, f.a * g.a, f.a * g.v[i] + f.v[i] * g.a)
STBA_JET_BIN(/, f.a / g.a, (f.v[i] - (f.a / g.a) * g.v[i]) / g.a)
#undef STBA_JET_BIN
template <typename T, int N> inline Jet<T, N> operator-(const Jet<T, N>& f) { Jet<T, N> h; h.a = -f.a; for (int i = 0; i < N; ++i) h.v[i] = -f.v[i]; return h; }
template <typename T, int N> inline Jet<T, N> operator+(const Jet<T, N>& f, T s) { Jet<T, N> h = f; h.a += s; return h; }
template <typename T, int N> inline Jet<T, N> operator+(T s, const Jet<T, N>& f) { return f + s; }
template <typename T, int N> inline Jet<T, N> operator-(const Jet<T, N>& f, T s) { Jet<T, N> h = f; h.a -= s; return h; }
template <typename T, int N> inline Jet<T, N> operator-(T s, const Jet<T, N>& f) { return (-f) + s; }
template <typename T, int N> inline Jet<T, N> operator*(const Jet<T, N>& f, T s) { Jet<T, N> h; h.a = f.a * s; for (int i = 0; i < N; ++i) h.v[i] = f.v[i] * s; return h; }
template <typename T, int N> inline Jet<T, N> operator*(T s, const Jet<T, N>& f) { return f * s; }
template <typename T, int N> inline Jet<T, N> operator/(const Jet<T, N>& f, T s) { return f * (T(1) / s); }
template <typename T, int N> inline Jet<T, N> operator/(T s, const Jet<T, N>& g) { return Jet<T, N>(s) / g; }
template <typename T, int N> inline bool operator<(const Jet<T, N>& f, const Jet<T, N>& g) { return f.a < g.a; }
template <typename T, int N> inline bool operator>(const Jet<T, N>& f, const Jet<T, N>& g) { return f.a > g.a; }
template <typename T, int N> inline bool operator<(const Jet<T, N>& f, T g) { return f.a < g; }
template <typename T, int N> inline bool operator>(const Jet<T, N>& f, T g) { return f.a > g; }
template <typename T, int N> inline Jet<T, N> sqrt(const Jet<T, N>& f) { Jet<T, N> h; h.a = std::sqrt(f.a); const T d = T(0.5) / h.a; for (int i = 0; i < N; ++i) h.v[i] = f.v[i] * d; return h; }
template <typename T, int N> inline Jet<T, N> sin(const Jet<T, N>& f) { Jet<T, N> h; h.a = std::sin(f.a); const T d = std::cos(f.a); for (int i = 0; i < N; ++i) h.v[i] = f.v[i] * d; return h; }
template <typename T, int N> inline Jet<T, N> cos(const Jet<T, N>& f) { Jet<T, N> h; h.a = std::cos(f.a); const T d = -std::sin(f.a); for (int i = 0; i < N; ++i) h.v[i] = f.v[i] * d; return h; }
template <typename T, int N> inline Jet<T, N> atan2(const Jet<T, N>& y, const Jet<T, N>& x) { Jet<T, N> h; h.a = std::atan2(y.a, x.a); const T d = T(1) / (x.a * x.a + y.a * y.a); for (int i = 0; i < N; ++i) h.v[i] = (x.a * y.v[i] - y.a * x.v[i]) * d; return h; }
template <typename T, int N> inline Jet<T, N> abs(const Jet<T, N>& f) { return f.a < T(0) ? -f : f; }
using std::sqrt; using std::sin; using std::cos; using std::atan2; using std::abs;

// ------------------------------------------------------------------------------------------
// enums / small types
// ------------------------------------------------------------------------------------------
enum LinearSolverType { DENSE_NORMAL_CHOLESKY, DENSE_QR, SPARSE_NORMAL_CHOLESKY, DENSE_SCHUR, SPARSE_SCHUR,
                        ITERATIVE_SCHUR, CGNR };
// ITERATIVE_SCHUR on the "gpu-ba" / "gpu-ba-hostjac" paths: conjugate gradients on the implicitly applied reduced camera system
// (stba_ba_create_ex) with IDENTITY, JACOBI or SCHUR_JACOBI; the other preconditioners are refused (FAILURE, the reason
// in Summary::message and on stderr, parameters untouched).  Every other linear_solver_type, and every problem that is not BA-shaped,
// takes the paths it always took.
enum PreconditionerType { IDENTITY, JACOBI, SCHUR_JACOBI, CLUSTER_JACOBI, CLUSTER_TRIDIAGONAL, SUBSET };
// DOGLEG (TRADITIONAL_DOGLEG) on the "gpu-ba" / "gpu-ba-hostjac" paths with the dense Schur solver: Powell's dogleg, one factorisation
// per linearisation (stba_ba_set_trust_region).  Refused before any device work (FAILURE, the reason in Summary::message
// and on stderr, parameters untouched): SUBSPACE_DOGLEG, DOGLEG with ITERATIVE_SCHUR (Ceres' own rule), and DOGLEG on a problem that
// takes "gpu-pg" or "gpu-dense-callback".
enum TrustRegionStrategyType { LEVENBERG_MARQUARDT, DOGLEG };
enum DoglegType { TRADITIONAL_DOGLEG, SUBSPACE_DOGLEG };
enum CallbackReturnType { SOLVER_CONTINUE, SOLVER_ABORT, SOLVER_TERMINATE_SUCCESSFULLY };
enum TerminationType { CONVERGENCE, NO_CONVERGENCE, FAILURE, USER_SUCCESS, USER_FAILURE };
enum Ownership { DO_NOT_TAKE_OWNERSHIP, TAKE_OWNERSHIP };
constexpr int DYNAMIC = -1;

// The reference only passes nullptr (test_ceres.h:120, solver.hpp:267).  Robust losses are implemented for POSE GRAPHS only: a Problem
// that takes the "gpu-pg" route (every residual block a RelativePoseFactor, or a NodePosePriorFactor without a loss) and whose losses are all the built-in classes below
// (recognised by dynamic_cast) is solved with them -- the per-edge table goes to stba_pg_set_loss (include/stba.h), which applies Ceres'
// corrector inside the device's linearisation kernel; Covariance on such a problem returns (J'^T J')^-1 as Ceres does.  Everything
// else that holds a non-null LossFunction -- a bare LossFunction or a user subclass (this base class has no Evaluate to call), any
// loss on a problem that takes a bundle-adjustment or the dense-callback route -- is REFUSED by Solve() and Covariance::Compute
// (FAILURE, parameters untouched, the reason in Summary::message and on stderr) instead of being solved without the loss.
// OPT-IN for bundle adjustment (an extension of this layer, like force_callback_path; the default stays the refusal):
// Solver::Options::bundle_adjustment_losses / Covariance::Options::bundle_adjustment_losses = true let a problem with losses through
// if, without them, it takes "gpu-ba" (device residuals: not "gpu-ba-hostjac", not the callback path), use_inner_iterations is off and
// every loss is one of the built-in classes (ScaledLoss one level deep included).  The per-observation table (kind 0, scale 1 for a
// block without a loss) then goes to stba_ba_set_loss before the solve (include/stba.h); any linear_solver_type and
// trust-region strategy "gpu-ba" accepts is accepted; Covariance returns (J'^T J')^-1.  Everything else is refused as before.
// Not provided: ComposedLoss, LossFunctionWrapper; ScaledLoss wraps a built-in (or nullptr) one level deep.
class LossFunction { public: virtual ~LossFunction() = default; };

// Ceres' loss functions (loss_function.h): Evaluate(s, rho) gives rho(s), rho'(s), rho''(s) at s = |r|^2, the formulas of the device
// kernel (pg_linearize.hip) on the host.  The classes are final: a dynamic_cast to one of them means exactly that loss.
class TrivialLoss final : public LossFunction {
public:
    void Evaluate(double s, double rho[3]) const { rho[0] = s; rho[1] = 1.0; rho[2] = 0.0; }
};
class HuberLoss final : public LossFunction {
public:
    explicit HuberLoss(double a) : a_(a), b_(a * a) {}
    void Evaluate(double s, double rho[3]) const {
        if (s > b_) {
            const double r = std::sqrt(s);
            rho[0] = 2.0 * a_ * r - b_; rho[1] = std::max(DBL_MIN, a_ / r); rho[2] = -rho[1] / (2.0 * s);
        } else { rho[0] = s; rho[1] = 1.0; rho[2] = 0.0; }
    }
    double a() const { return a_; }
private:
    const double a_, b_;
};
class SoftLOneLoss final : public LossFunction {
public:
    explicit SoftLOneLoss(double a) : a_(a), b_(a * a), c_(1.0 / b_) {}
    void Evaluate(double s, double rho[3]) const {
        const double sum = 1.0 + s * c_, tmp = std::sqrt(sum);
        rho[0] = 2.0 * b_ * (tmp - 1.0); rho[1] = std::max(DBL_MIN, 1.0 / tmp); rho[2] = -(c_ * rho[1]) / (2.0 * sum);
    }
    double a() const { return a_; }
private:
    const double a_, b_, c_;
};
class CauchyLoss final : public LossFunction {
public:
    explicit CauchyLoss(double a) : a_(a), b_(a * a), c_(1.0 / b_) {}
    void Evaluate(double s, double rho[3]) const {
        const double sum = 1.0 + s * c_, inv = 1.0 / sum;
        rho[0] = b_ * std::log(sum); rho[1] = std::max(DBL_MIN, inv); rho[2] = -c_ * (inv * inv);
    }
    double a() const { return a_; }
private:
    const double a_, b_, c_;
};
class ArctanLoss final : public LossFunction {
public:
    explicit ArctanLoss(double a) : a_(a), b_(1.0 / (a * a)) {}
    void Evaluate(double s, double rho[3]) const {
        const double sum = 1.0 + s * s * b_, inv = 1.0 / sum;
        rho[0] = a_ * std::atan2(s, a_); rho[1] = std::max(DBL_MIN, inv); rho[2] = -2.0 * s * b_ * (inv * inv);
    }
    double a() const { return a_; }
private:
    const double a_, b_;
};
class TolerantLoss final : public LossFunction {
public:
    TolerantLoss(double a, double b) : a_(a), b_(b), c_(b * std::log(1.0 + std::exp(-a / b))) {}
    void Evaluate(double s, double rho[3]) const {
        const double x = (s - a_) / b_;
        if (x > 36.7) { rho[0] = s - a_ - c_; rho[1] = 1.0; rho[2] = 0.0; }       // log(2^53): e^x + 1 == e^x from here on
        else {
            const double e_x = std::exp(x);
            rho[0] = b_ * std::log(1.0 + e_x) - c_; rho[1] = std::max(DBL_MIN, e_x / (1.0 + e_x)); rho[2] = 0.5 / (b_ * (1.0 + std::cosh(x)));
        }
    }
    double a() const { return a_; }
    double b() const { return b_; }
private:
    const double a_, b_, c_;
};
class TukeyLoss final : public LossFunction {
public:
    explicit TukeyLoss(double a) : a_(a), a_squared_(a * a) {}
    void Evaluate(double s, double rho[3]) const {
        if (s <= a_squared_) {
            const double value = 1.0 - s / a_squared_, value_sq = value * value;
            rho[0] = a_squared_ / 3.0 * (1.0 - value_sq * value); rho[1] = value_sq; rho[2] = -2.0 / a_squared_ * value;
        } else { rho[0] = a_squared_ / 3.0; rho[1] = 0.0; rho[2] = 0.0; }
    }
    double a() const { return a_; }
private:
    const double a_, a_squared_;
};

namespace internal {
// the STBA_LOSS_* row of a built-in loss; false for anything else (a bare LossFunction, a user subclass, a ScaledLoss)
inline bool BuiltinLossRow(const LossFunction* l, int* kind, double* a, double* b) {
    *a = 1.0; *b = 1.0;
    if (dynamic_cast<const TrivialLoss*>(l)) { *kind = STBA_LOSS_TRIVIAL; return true; }
    if (auto* h = dynamic_cast<const HuberLoss*>(l)) { *kind = STBA_LOSS_HUBER; *a = h->a(); return true; }
    if (auto* h = dynamic_cast<const SoftLOneLoss*>(l)) { *kind = STBA_LOSS_SOFTLONE; *a = h->a(); return true; }
    if (auto* h = dynamic_cast<const CauchyLoss*>(l)) { *kind = STBA_LOSS_CAUCHY; *a = h->a(); return true; }
    if (auto* h = dynamic_cast<const ArctanLoss*>(l)) { *kind = STBA_LOSS_ARCTAN; *a = h->a(); return true; }
    if (auto* h = dynamic_cast<const TolerantLoss*>(l)) { *kind = STBA_LOSS_TOLERANT; *a = h->a(); *b = h->b(); return true; }
    if (auto* h = dynamic_cast<const TukeyLoss*>(l)) { *kind = STBA_LOSS_TUKEY; *a = h->a(); return true; }
    return false;
}
}  // namespace internal

// a * rho(s) (rho', rho'' likewise) of a built-in loss, or a * s for a null one.  ONE level: a ScaledLoss around anything that is not one
// of the classes above (another ScaledLoss, a user's loss) is not a built-in loss and is refused like a user's.
class ScaledLoss final : public LossFunction {
public:
    ScaledLoss(const LossFunction* rho, double a, Ownership ownership) : rho_(rho), a_(a), ownership_(ownership) {}
    ScaledLoss(const ScaledLoss&) = delete;
    ScaledLoss& operator=(const ScaledLoss&) = delete;
    ~ScaledLoss() override { if (ownership_ == TAKE_OWNERSHIP) delete rho_; }
    void Evaluate(double s, double rho[3]) const {
        int kind; double a, b;
        if (!rho_) { rho[0] = a_ * s; rho[1] = a_; rho[2] = 0.0; return; }
        if (!internal::BuiltinLossRow(rho_, &kind, &a, &b)) { rho[0] = rho[1] = rho[2] = std::numeric_limits<double>::quiet_NaN(); return; }
        switch (kind) {
        case STBA_LOSS_TRIVIAL: static_cast<const TrivialLoss*>(rho_)->Evaluate(s, rho); break;
        case STBA_LOSS_HUBER: static_cast<const HuberLoss*>(rho_)->Evaluate(s, rho); break;
        case STBA_LOSS_SOFTLONE: static_cast<const SoftLOneLoss*>(rho_)->Evaluate(s, rho); break;
        case STBA_LOSS_CAUCHY: static_cast<const CauchyLoss*>(rho_)->Evaluate(s, rho); break;
        case STBA_LOSS_ARCTAN: static_cast<const ArctanLoss*>(rho_)->Evaluate(s, rho); break;
        case STBA_LOSS_TOLERANT: static_cast<const TolerantLoss*>(rho_)->Evaluate(s, rho); break;
        default: static_cast<const TukeyLoss*>(rho_)->Evaluate(s, rho); break;
        }
        for (int k = 0; k < 3; ++k) rho[k] *= a_;
    }
    const LossFunction* inner() const { return rho_; }
    double scale() const { return a_; }
private:
    const LossFunction* rho_;
    const double a_;
    const Ownership ownership_;
};

namespace internal {
// kind, a, b, scale of a loss this layer knows: a built-in, or a ScaledLoss around a built-in or nullptr
inline bool KnownLossRow(const LossFunction* l, int* kind, double* a, double* b, double* scale) {
    *scale = 1.0;
    if (auto* sl = dynamic_cast<const ScaledLoss*>(l)) {
        *scale = sl->scale();
        if (!sl->inner()) { *kind = STBA_LOSS_TRIVIAL; *a = 1.0; *b = 1.0; return true; }
        return BuiltinLossRow(sl->inner(), kind, a, b);
    }
    return BuiltinLossRow(l, kind, a, b);
}
}  // namespace internal

struct IterationSummary {
    int iteration = 0;
    int linear_solver_iterations = 0;     // PCG iterations of this iteration's step (ITERATIVE_SCHUR; 0 on every other path)
    bool step_is_valid = false, step_is_successful = false;
    double cost = 0, cost_change = 0, gradient_max_norm = 0, step_norm = 0, relative_decrease = 0,
           trust_region_radius = 0;
};

class IterationCallback {
public:
    virtual ~IterationCallback() = default;
    virtual CallbackReturnType operator()(const IterationSummary& summary) = 0;
};

// ------------------------------------------------------------------------------------------
// CostFunction family
// ------------------------------------------------------------------------------------------
class CostFunction {
public:
    virtual ~CostFunction() = default;
    virtual bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const = 0;
    const std::vector<int>& parameter_block_sizes() const { return parameter_block_sizes_; }
    int num_residuals() const { return num_residuals_; }
protected:
    std::vector<int>* mutable_parameter_block_sizes() { return &parameter_block_sizes_; }
    void set_num_residuals(int n) { num_residuals_ = n; }
private:
    friend class Problem;
    std::vector<int> parameter_block_sizes_;
    int num_residuals_ = 0;
    bool owned_by_problem_ = false;      // set by the Problem that will delete it: a cost function shared by residual blocks is freed once
};

template <int kNumResiduals, int... Ns>
class SizedCostFunction : public CostFunction {
public:
    SizedCostFunction() {
        set_num_residuals(kNumResiduals);
        *mutable_parameter_block_sizes() = std::vector<int>{Ns...};
    }
};

namespace internal {
template <int... Ns> struct Sum;
template <> struct Sum<> { static constexpr int value = 0; };
template <int N, int... Ns> struct Sum<N, Ns...> { static constexpr int value = N + Sum<Ns...>::value; };

// calls functor(p0, p1, ..., residuals) with the parameter pointers unpacked
template <typename F, typename T, size_t... I>
inline bool CallVariadic(const F& f, T const* const* params, T* residuals, std::index_sequence<I...>) {
    return f(params[I]..., residuals);
}
}  // namespace internal

template <typename CostFunctor, int kNumResiduals, int... Ns>
class AutoDiffCostFunction : public SizedCostFunction<kNumResiduals, Ns...> {
public:
    explicit AutoDiffCostFunction(CostFunctor* functor, Ownership own = TAKE_OWNERSHIP) : functor_(functor), own_(own) {}
    ~AutoDiffCostFunction() override { if (own_ == TAKE_OWNERSHIP) delete functor_; }
    bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const override {
        constexpr int kBlocks = sizeof...(Ns);
        constexpr int kParams = internal::Sum<Ns...>::value;
        if (!jacobians) return internal::CallVariadic(*functor_, parameters, residuals, std::make_index_sequence<kBlocks>{});
        using JetT = Jet<double, kParams>;
        const int sizes[kBlocks] = {Ns...};
        JetT x[kParams];
        JetT const* ptrs[kBlocks];
        int off = 0;
        for (int b = 0; b < kBlocks; ++b) {
            ptrs[b] = x + off;
            for (int k = 0; k < sizes[b]; ++k) x[off + k] = JetT(parameters[b][k], off + k);
            off += sizes[b];
        }
        JetT out[kNumResiduals];
        if (!internal::CallVariadic(*functor_, ptrs, out, std::make_index_sequence<kBlocks>{})) return false;
        off = 0;
        for (int b = 0; b < kBlocks; ++b) {
            for (int r = 0; r < kNumResiduals; ++r) {
                if (b == 0) residuals[r] = out[r].a;
                if (jacobians[b])
                    for (int k = 0; k < sizes[b]; ++k) jacobians[b][r * sizes[b] + k] = out[r].v[off + k];
            }
            off += sizes[b];
        }
        return true;
    }
private:
    CostFunctor* functor_;
    Ownership own_;
};

template <typename CostFunctor, int Stride = 4>
class DynamicAutoDiffCostFunction : public CostFunction {
public:
    explicit DynamicAutoDiffCostFunction(CostFunctor* functor, Ownership own = TAKE_OWNERSHIP) : functor_(functor), own_(own) {}
    ~DynamicAutoDiffCostFunction() override { if (own_ == TAKE_OWNERSHIP) delete functor_; }
    void AddParameterBlock(int size) {
        auto* v = mutable_parameter_block_sizes();
        if (v->capacity() == 0) v->reserve(4);       // (one allocation for the usual two to four blocks instead of one per doubling: 10^6 cost functions at C5)
        v->push_back(size);
    }
    void SetNumResiduals(int n) { set_num_residuals(n); }
    bool Evaluate(double const* const* parameters, double* residuals, double** jacobians) const override {
        const auto& sizes = parameter_block_sizes();
        const int nb = (int)sizes.size(), nr = num_residuals();
        if (!jacobians) return (*functor_)(parameters, residuals);
        using JetT = Jet<double, Stride>;
        int total = 0;
        for (int s : sizes) total += s;
        // small problems (the reference's: 7-10 parameters, 2 residuals) work on the stack: no allocation per evaluation
        constexpr int kStackParams = 32, kStackRes = 8, kStackBlocks = 8;
        JetT x_stack[kStackParams], out_stack[kStackRes];
        JetT const* ptrs_stack[kStackBlocks];
        int blk_stack[kStackParams], loc_stack[kStackParams];
        std::vector<JetT> x_heap, out_heap;
        std::vector<JetT const*> ptrs_heap;
        std::vector<int> blk_heap, loc_heap;
        const bool on_stack = total <= kStackParams && nr <= kStackRes && nb <= kStackBlocks;
        if (!on_stack) { x_heap.resize(total); out_heap.resize(nr); ptrs_heap.resize(nb); blk_heap.resize(total); loc_heap.resize(total); }
        JetT* x = on_stack ? x_stack : x_heap.data();
        JetT* out = on_stack ? out_stack : out_heap.data();
        JetT const** ptrs = on_stack ? ptrs_stack : ptrs_heap.data();
        int* blk = on_stack ? blk_stack : blk_heap.data();
        int* loc = on_stack ? loc_stack : loc_heap.data();
        for (int b = 0, o = 0; b < nb; ++b) {
            ptrs[b] = x + o;
            for (int k = 0; k < sizes[b]; ++k, ++o) { blk[o] = b; loc[o] = k; }
        }
        // ceil(total / Stride) passes, Stride partial derivatives per pass (as Ceres does)
        for (int start = 0; start < total || start == 0; start += Stride) {
            for (int b = 0, o = 0; b < nb; ++b)
                for (int k = 0; k < sizes[b]; ++k, ++o) {
                    x[o] = JetT(parameters[b][k]);
                    if (o >= start && o < start + Stride) x[o].v[o - start] = 1.0;
                }
            if (!(*functor_)(ptrs, out)) return false;
            for (int r = 0; r < nr; ++r) {
                residuals[r] = out[r].a;
                for (int o = start; o < std::min(total, start + Stride); ++o)
                    if (jacobians[blk[o]]) jacobians[blk[o]][r * sizes[blk[o]] + loc[o]] = out[r].v[o - start];
            }
            if (total == 0) break;
        }
        return true;
    }
private:
    CostFunctor* functor_;
    Ownership own_;
};

// ------------------------------------------------------------------------------------------
// LocalParameterization (Ceres <= 2.1 API, as the reference uses it)
// ------------------------------------------------------------------------------------------
class LocalParameterization {
public:
    virtual ~LocalParameterization() = default;
    virtual bool Plus(const double* x, const double* delta, double* x_plus_delta) const = 0;
    virtual bool ComputeJacobian(const double* x, double* jacobian) const = 0;   // GlobalSize x LocalSize, row-major
    virtual int GlobalSize() const = 0;
    virtual int LocalSize() const = 0;
};

// ------------------------------------------------------------------------------------------
// built-in factor / manifold kinds the HIP kernels implement natively
// ------------------------------------------------------------------------------------------
// q (x,y,z,w) <- q (x) exp(delta): LieLocalParameterization<Sophus::SO3d> (solver.hpp:30-61)
class QuaternionRightPlus : public LocalParameterization {
public:
    bool Plus(const double* q, const double* d, double* out) const override {
        const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        double im, re;
        if (th2 < 1e-20) { im = 0.5 - th2 / 48.0; re = 1.0 - th2 / 8.0; }
        else { const double th = std::sqrt(th2); im = std::sin(0.5 * th) / th; re = std::cos(0.5 * th); }
        const double bx = im * d[0], by = im * d[1], bz = im * d[2], bw = re;
        const double ax = q[0], ay = q[1], az = q[2], aw = q[3];
        double o[4] = {aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                       aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz};
        const double n = std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
        for (int i = 0; i < 4; ++i) out[i] = o[i] / n;
        return true;
    }
    bool ComputeJacobian(const double* q, double* J) const override {   // notes.tex:131-144
        const double x = 0.5 * q[0], y = 0.5 * q[1], z = 0.5 * q[2], w = 0.5 * q[3];
        const double M[12] = {w, -z, y, z, w, -x, -y, x, w, -x, -y, -z};
        std::memcpy(J, M, sizeof M);
        return true;
    }
    int GlobalSize() const override { return 4; }
    int LocalSize() const override { return 3; }
};

// ns_st20::ProjectFactor (test_ceres.h:47-81) as a built-in: blocks {SO3 quaternion 4, POS 3,
// landmark 3}, residual = proj(R^T (L - t)) - feature.  Evaluate() is provided for completeness
// (ambient 2x4 quaternion Jacobian), but a Problem made only of these runs fully on the GPU.
class ReprojectionFactor : public SizedCostFunction<2, 4, 3, 3> {
public:
    ReprojectionFactor(double fx, double fy) : fx_(fx), fy_(fy) {}
    // sqrt_information: W, 2 x 2 row-major -- the factor becomes r = W (proj(R^T (L - t)) - feature), its cost 1/2 r^T W^T W r.  The
    // factor whitens itself (operator() and, through the Jets, Evaluate's Jacobians), so every host route sees the weighted factor;
    // on "gpu-ba" the W of all blocks go to stba_ba_set_sqrt_information
    // (a template over the pointer type so that ReprojectionFactor(0, 0) stays the (double, double) constructor: literal zeros deduce
    // int, which is no pointer)
    template <class P, class = typename std::enable_if<std::is_pointer<P>::value && std::is_convertible<P, const double*>::value>::type>
    ReprojectionFactor(P feature, const double* sqrt_information) : fx_(feature[0]), fy_(feature[1]), has_w_(true) {
        std::memcpy(w_, sqrt_information, sizeof w_);
    }
    static ReprojectionFactor* Create(const double* feature) { return new ReprojectionFactor(feature[0], feature[1]); }
    static ReprojectionFactor* Create(const double* feature, const double* sqrt_information) { return new ReprojectionFactor(feature, sqrt_information); }
    double fx() const { return fx_; }
    double fy() const { return fy_; }
    const double* sqrt_information() const { return has_w_ ? w_ : nullptr; }      // nullptr: made without one (identity)
    template <typename T>
    bool operator()(const T* q, const T* t, const T* L, T* r) const {
        // conj(q) * (L - t) with Eigen's v + 2w(u x v) + 2 u x (u x v), u = -q.xyz
        const T u0 = -q[0], u1 = -q[1], u2 = -q[2], w = q[3];
        const T v0 = L[0] - t[0], v1 = L[1] - t[1], v2 = L[2] - t[2];
        const T a0 = T(2.0) * (u1 * v2 - u2 * v1), a1 = T(2.0) * (u2 * v0 - u0 * v2), a2 = T(2.0) * (u0 * v1 - u1 * v0);
        const T x = v0 + w * a0 + (u1 * a2 - u2 * a1);
        const T y = v1 + w * a1 + (u2 * a0 - u0 * a2);
        const T z = v2 + w * a2 + (u0 * a1 - u1 * a0);
        r[0] = x / z - T(fx_);
        r[1] = y / z - T(fy_);
        if (has_w_) {
            const T e0 = r[0], e1 = r[1];
            r[0] = T(w_[0]) * e0 + T(w_[1]) * e1;
            r[1] = T(w_[2]) * e0 + T(w_[3]) * e1;
        }
        return true;
    }
    bool Evaluate(double const* const* p, double* residuals, double** jacobians) const override {
        if (!jacobians) return (*this)(p[0], p[1], p[2], residuals);
        using J10 = Jet<double, 10>;
        J10 x[10], out[2];
        for (int k = 0; k < 4; ++k) x[k] = J10(p[0][k], k);
        for (int k = 0; k < 3; ++k) { x[4 + k] = J10(p[1][k], 4 + k); x[7 + k] = J10(p[2][k], 7 + k); }
        (*this)(x, x + 4, x + 7, out);
        for (int r = 0; r < 2; ++r) {
            residuals[r] = out[r].a;
            if (jacobians[0]) for (int k = 0; k < 4; ++k) jacobians[0][r * 4 + k] = out[r].v[k];
            if (jacobians[1]) for (int k = 0; k < 3; ++k) jacobians[1][r * 3 + k] = out[r].v[4 + k];
            if (jacobians[2]) for (int k = 0; k < 3; ++k) jacobians[2][r * 3 + k] = out[r].v[7 + k];
        }
        return true;
    }
private:
    double fx_, fy_;
    bool has_w_ = false;
    double w_[4] = {1.0, 0.0, 0.0, 1.0};
};

// A prior on a camera's pose, the host form of the device engine's pose-prior factor (stba_ba_set_pose_priors): blocks
// {SO3 quaternion 4, POS 3} -> 6 residuals r = W [Log(qh^-1 (x) q); t - th], order [rot(3), pos(3)]; W the 6 x 6 row-major
// square-root information (nullptr: the identity; zero rotation rows: a position-only prior).  The Jacobians are ambient (6 x 4 and
// 6 x 3): the quaternion's is W[:, :3] Jr^-1(r_theta) P^+ with P = QuaternionRightPlus::ComputeJacobian(q) and P^+ = 4 P^T / |q|^2
// its left inverse, so that composed with that chart it is W[:, :3] Jr^-1 -- the device factor's J under q <- q (x) exp(delta).
// Same formulas as the device (slam-tricks_amd/csrc/ba_prior.hpp): the quaternion product with the cancelling products paired (a
// prior AT the camera's pose has the rotation residual exactly 0 in a build without FMA contraction), theta = 2 atan2(|v|, w) behind
// the sign choice w >= 0 (q and -q: the same residual), the hat^2 coefficient (1 - (theta / 2) cot(theta / 2)) / theta^2 with
// cot(theta / 2) = w / |v| (no 0 / 0 at pi), its series below 0.1 rad.
// On a problem that otherwise takes "gpu-ba", the recognition (BaStructure) sets these blocks aside and Solve / Covariance hand them to the device engine
// (stba_ba_set_pose_priors), provided the two blocks are the rotation and the position block of ONE camera that some observation
// names and the block has no LossFunction; otherwise, and on every other route, it is an ordinary host cost function.  With
// ITERATIVE_SCHUR, DOGLEG or use_inner_iterations the solve is refused (FAILURE, parameters untouched, the reason in the message).
class PosePriorFactor : public SizedCostFunction<6, 4, 3> {
public:
    PosePriorFactor(const double q[4], const double t[3], const double* sqrt_information = nullptr) {
        // (normalised as stba_ba_set_pose_priors normalises: a quaternion that is unit to 8 eps keeps its bits)
        const double n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
        const double sc = std::fabs(n2 - 1.0) <= 8 * 2.220446049250313e-16 ? 1.0 : 1.0 / std::sqrt(n2);
        for (int k = 0; k < 4; ++k) pose_[k] = q[k] * sc;
        for (int k = 0; k < 3; ++k) pose_[4 + k] = t[k];
        for (int k = 0; k < 36; ++k) w_[k] = sqrt_information ? sqrt_information[k] : (k % 7 == 0 ? 1.0 : 0.0);
        has_w_ = sqrt_information != nullptr;
    }
    static PosePriorFactor* Create(const double q[4], const double t[3], const double* sqrt_information = nullptr) {
        return new PosePriorFactor(q, t, sqrt_information);
    }
    const double* pose() const { return pose_; }                                  // [qx qy qz qw tx ty tz], the quaternion normalised
    const double* sqrt_information() const { return has_w_ ? w_ : nullptr; }      // nullptr: made without one (identity)
    const double* weights() const { return w_; }                                  // the 36 entries either way
    // the 6 unwhitened residuals at (q, t) and Jr^-1 of the rotation part (3 x 3 row-major; may be null)
    void Residual(const double* q, const double* t, double* r, double* Jri) const {
        const double ax = -pose_[0], ay = -pose_[1], az = -pose_[2], aw = pose_[3];
        const double bx = q[0], by = q[1], bz = q[2], bw = q[3];
        double x = (aw * bx + ax * bw) + (ay * bz - az * by);
        double y = (aw * by + ay * bw) + (az * bx - ax * bz);
        double z = (aw * bz + az * bw) + (ax * by - ay * bx);
        double w = ((aw * bw - ax * bx) - ay * by) - az * bz;
        const double lead = x != 0.0 ? x : (y != 0.0 ? y : z);
        if (w < 0.0 || (w == 0.0 && lead < 0.0)) { x = -x; y = -y; z = -z; w = -w; }
        const double n2 = (x * x + y * y) + z * z, n = std::sqrt(n2);
        double k, cot = 0.0;
        if (n2 < 1e-40) k = 2.0 / w;
        else { k = 2.0 * std::atan2(n, w) / n; cot = w / n; }
        r[0] = k * x; r[1] = k * y; r[2] = k * z;
        for (int i = 0; i < 3; ++i) r[3 + i] = t[i] - pose_[4 + i];
        if (!Jri) return;
        const double th = k * n, t2 = th * th;
        const double c = th < 0.1 ? 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 * (1.0 / 1209600.0 + t2 * (1.0 / 47900160.0))))
                                  : (1.0 - (0.5 * th) * cot) / t2;
        const double pp = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
        const double h[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const double d = a == b ? 1.0 : 0.0;
                Jri[a * 3 + b] = (d + 0.5 * h[a * 3 + b]) + c * (r[a] * r[b] - pp * d);
            }
    }
    bool Evaluate(double const* const* p, double* residuals, double** jacobians) const override {
        const double* q = p[0];
        double r[6], Jri[9];
        Residual(q, p[1], r, Jri);
        for (int i = 0; i < 6; ++i) {
            const double* wi = w_ + i * 6;
            residuals[i] = ((((wi[0] * r[0] + wi[1] * r[1]) + wi[2] * r[2]) + wi[3] * r[3]) + wi[4] * r[4]) + wi[5] * r[5];
        }
        if (!jacobians) return true;
        if (jacobians[0]) {
            double P[12];
            QuaternionRightPlus().ComputeJacobian(q, P);
            const double s = 4.0 / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            for (int i = 0; i < 6; ++i) {
                double wj[3];       // row i of W[:, :3] Jr^-1
                for (int a = 0; a < 3; ++a) wj[a] = (w_[i * 6] * Jri[a] + w_[i * 6 + 1] * Jri[3 + a]) + w_[i * 6 + 2] * Jri[6 + a];
                for (int g = 0; g < 4; ++g) jacobians[0][i * 4 + g] = s * (wj[0] * P[g * 3] + wj[1] * P[g * 3 + 1] + wj[2] * P[g * 3 + 2]);
            }
        }
        if (jacobians[1]) for (int i = 0; i < 6; ++i) for (int a = 0; a < 3; ++a) jacobians[1][i * 3 + a] = w_[i * 6 + 3 + a];
        return true;
    }
private:
    double pose_[7];
    double w_[36];
    bool has_w_ = false;
};

// A prior on a landmark's position (a control point), the host form of the device engine's factor
// (stba_ba_set_landmark_priors): block {landmark 3} -> 3 residuals r = W (p - ph); W the 3 x 3 row-major square-root information
// (nullptr: the identity; one non-zero row: a height-only control point).  The Jacobian is W.  Same operations in the same order as
// the device (slam-tricks_amd/csrc/ba_landmark_prior.hpp): row i of W r as (W_i0 r_0 + W_i1 r_1) + W_i2 r_2, and like there WITHOUT
// contraction into FMAs whatever the build's flags (W r cancels for a tight prior): clang by its pragma, GCC -- which contracts by
// default wherever the target has FMA -- by the optimize attribute on Evaluate.
// On a problem that otherwise takes "gpu-ba", the recognition (BaStructure) sets these blocks aside and Solve / Covariance hand them
// to the device engine, provided the block is a landmark that some observation names, carries no chart and no bounds, and the
// residual block has no LossFunction; otherwise, and on every other route, it is an ordinary host cost function.  ITERATIVE_SCHUR
// and DOGLEG take them; with use_inner_iterations the solve is refused (FAILURE, parameters untouched, the reason in the message).
#ifndef STBA_CERES_NO_CONTRACT       // (the test defines it empty to see that the compiler at hand WOULD contract)
#if defined(__GNUC__) && !defined(__clang__)
#define STBA_CERES_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define STBA_CERES_NO_CONTRACT
#endif
#endif
class LandmarkPriorFactor : public SizedCostFunction<3, 3> {
public:
    LandmarkPriorFactor(const double position[3], const double* sqrt_information = nullptr) {
        for (int k = 0; k < 3; ++k) pos_[k] = position[k];
        for (int k = 0; k < 9; ++k) w_[k] = sqrt_information ? sqrt_information[k] : (k % 4 == 0 ? 1.0 : 0.0);
        has_w_ = sqrt_information != nullptr;
    }
    static LandmarkPriorFactor* Create(const double position[3], const double* sqrt_information = nullptr) {
        return new LandmarkPriorFactor(position, sqrt_information);
    }
    const double* position() const { return pos_; }
    const double* sqrt_information() const { return has_w_ ? w_ : nullptr; }      // nullptr: made without one (identity)
    const double* weights() const { return w_; }                                  // the 9 entries either way
    STBA_CERES_NO_CONTRACT bool Evaluate(double const* const* p, double* residuals, double** jacobians) const override {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double r[3] = {p[0][0] - pos_[0], p[0][1] - pos_[1], p[0][2] - pos_[2]};
        for (int i = 0; i < 3; ++i) residuals[i] = (w_[i * 3] * r[0] + w_[i * 3 + 1] * r[1]) + w_[i * 3 + 2] * r[2];
        if (jacobians && jacobians[0]) for (int k = 0; k < 9; ++k) jacobians[0][k] = w_[k];
        return true;
    }
private:
    double pos_[3];
    double w_[9];
    bool has_w_ = false;
};

// A relative-pose measurement between two cameras, the host form of the device engine's factor
// (stba_ba_set_relative_poses): blocks {q_i 4, t_i 3, q_j 4, t_j 3} -> 6 residuals
//     r = W [ Log(qz^-1 (x) (q_i^-1 (x) q_j)) ; R_i^T (t_j - t_i) - tz ],   order [rot(3), pos(3)],
// poses camera to world as everywhere in the BA engine (NOT the pose graph's RelativePoseFactor below, whose pose is one block of 7
// and whose tangent is [rho, theta]); W the 6 x 6 row-major square-root information (nullptr: the identity).  The Jacobians are
// ambient: the quaternions' are the local ones (6 x 3, the device factor's under q <- q (x) exp(delta)) times P^+ = 4 P^T / |q|^2,
// the left inverse of P = QuaternionRightPlus::ComputeJacobian(q), as PosePriorFactor's.  Same operations in the same order as the
// device (slam-tricks_amd/csrc/ba_between.hpp): negating any of the three quaternions leaves the residual's bits.
// On a problem that otherwise takes "gpu-ba", the recognition (BaStructure) sets these blocks aside and Solve / Covariance hand them to the device engine,
// provided the four blocks are the rotation and position blocks of two DISTINCT cameras that observations name and the block has no
// LossFunction; otherwise, and on every other route, it is an ordinary host cost function.  With ITERATIVE_SCHUR, DOGLEG or
// use_inner_iterations the solve is refused (FAILURE, parameters untouched, the reason in the message).
class CameraRelativePoseFactor : public SizedCostFunction<6, 4, 3, 4, 3> {
public:
    CameraRelativePoseFactor(const double q[4], const double t[3], const double* sqrt_information = nullptr) {
        // (normalised as stba_ba_set_relative_poses normalises: a quaternion that is unit to 8 eps keeps its bits)
        const double n2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
        const double sc = std::fabs(n2 - 1.0) <= 8 * 2.220446049250313e-16 ? 1.0 : 1.0 / std::sqrt(n2);
        for (int k = 0; k < 4; ++k) meas_[k] = q[k] * sc;
        for (int k = 0; k < 3; ++k) meas_[4 + k] = t[k];
        for (int k = 0; k < 36; ++k) w_[k] = sqrt_information ? sqrt_information[k] : (k % 7 == 0 ? 1.0 : 0.0);
    }
    static CameraRelativePoseFactor* Create(const double q_meas[4], const double t_meas[3], const double* sqrt_information = nullptr) {
        return new CameraRelativePoseFactor(q_meas, t_meas, sqrt_information);
    }
    const double* measurement() const { return meas_; }      // [qx qy qz qw tx ty tz], the quaternion normalised
    const double* weights() const { return w_; }              // the 36 entries (the identity if made without)
    static void Rot(const double* q, double* R) {
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        const double s = 2.0 / (((x * x + y * y) + z * z) + w * w);
        R[0] = 1.0 - s * (y * y + z * z); R[1] = s * (x * y - z * w);       R[2] = s * (x * z + y * w);
        R[3] = s * (x * y + z * w);       R[4] = 1.0 - s * (x * x + z * z); R[5] = s * (y * z - x * w);
        R[6] = s * (x * z - y * w);       R[7] = s * (y * z + x * w);       R[8] = 1.0 - s * (x * x + y * y);
    }
    // the 6 unwhitened residuals and, when Ji is given, the two LOCAL 6 x 6 Jacobians (row-major) under q <- q (x) exp(dtheta), t <- t + dt
    void Residual(const double* qi, const double* ti, const double* qj, const double* tj, double* r, double* Ji, double* Jj) const {
        const double ax = -qi[0], ay = -qi[1], az = -qi[2], aw = qi[3];
        const double bx = qj[0], by = qj[1], bz = qj[2], bw = qj[3];
        const double m[4] = {(aw * bx + ax * bw) + (ay * bz - az * by), (aw * by + ay * bw) + (az * bx - ax * bz),
                             (aw * bz + az * bw) + (ax * by - ay * bx), ((aw * bw - ax * bx) - ay * by) - az * bz};
        // Log(qz^-1 (x) m) and Jr^-1: the prior's, with the measurement in the prior pose's place
        double Jri[9];
        PosePriorFactor(meas_, meas_ + 4).Residual(m, meas_ + 4, r, Ji ? Jri : nullptr);
        double Ri[9], v[3];
        Rot(qi, Ri);
        const double d0 = tj[0] - ti[0], d1 = tj[1] - ti[1], d2 = tj[2] - ti[2];
        for (int k = 0; k < 3; ++k) {
            v[k] = (Ri[k] * d0 + Ri[3 + k] * d1) + Ri[6 + k] * d2;
            r[3 + k] = v[k] - meas_[4 + k];
        }
        if (!Ji) return;
        double Rm[9];
        Rot(m, Rm);
        for (int k = 0; k < 36; ++k) Ji[k] = Jj[k] = 0.0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                Ji[a * 6 + b] = -((Jri[a * 3] * Rm[b * 3] + Jri[a * 3 + 1] * Rm[b * 3 + 1]) + Jri[a * 3 + 2] * Rm[b * 3 + 2]);
                Jj[a * 6 + b] = Jri[a * 3 + b];
                Ji[(3 + a) * 6 + 3 + b] = -Ri[b * 3 + a];
                Jj[(3 + a) * 6 + 3 + b] = Ri[b * 3 + a];
            }
        Ji[3 * 6 + 1] = -v[2]; Ji[3 * 6 + 2] = v[1];
        Ji[4 * 6 + 0] = v[2];  Ji[4 * 6 + 2] = -v[0];
        Ji[5 * 6 + 0] = -v[1]; Ji[5 * 6 + 1] = v[0];
    }
    bool Evaluate(double const* const* p, double* residuals, double** jacobians) const override {
        double r[6], Ji[36], Jj[36];
        Residual(p[0], p[1], p[2], p[3], r, jacobians ? Ji : nullptr, Jj);
        auto dot = [](const double* wi, const double* x, int st) {
            return ((((wi[0] * x[0] + wi[1] * x[st]) + wi[2] * x[2 * st]) + wi[3] * x[3 * st]) + wi[4] * x[4 * st]) + wi[5] * x[5 * st];
        };
        for (int i = 0; i < 6; ++i) residuals[i] = dot(w_ + i * 6, r, 1);
        if (!jacobians) return true;
        for (int side = 0; side < 2; ++side) {
            const double* J = side ? Jj : Ji;
            const double* q = p[2 * side];
            if (jacobians[2 * side]) {
                double P[12];
                QuaternionRightPlus().ComputeJacobian(q, P);
                const double s = 4.0 / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
                for (int i = 0; i < 6; ++i) {
                    double wj[3];
                    for (int a = 0; a < 3; ++a) wj[a] = dot(w_ + i * 6, J + a, 6);
                    for (int g = 0; g < 4; ++g) jacobians[2 * side][i * 4 + g] = s * (wj[0] * P[g * 3] + wj[1] * P[g * 3 + 1] + wj[2] * P[g * 3 + 2]);
                }
            }
            if (jacobians[2 * side + 1])
                for (int i = 0; i < 6; ++i) for (int a = 0; a < 3; ++a) jacobians[2 * side + 1][i * 3 + a] = dot(w_ + i * 6, J + 3 + a, 6);
        }
        return true;
    }
private:
    double meas_[7];
    double w_[36];
};

// ------------------------------------------------------------------------------------------
// Pose graph through the same operator API (BASELINE config C4; build-defined: the reference has no pose-graph code, the
// conventions are its Lie-group notes', st23-lie-group-v2/doc.tex:862-996).  A pose is ONE parameter block of 7 doubles
// (qx qy qz qw tx ty tz); SE3RightPlus is its chart T <- T exp(delta), delta = [rho, theta] (Sophus' SE3 tangent order);
// RelativePoseFactor is the edge r = log(Z^-1 T_i^-1 T_j) in R^6.  A Problem made only of these runs on the device pose-graph
// engine (stba_pg_*: "gpu-pg"); Evaluate / Plus / ComputeJacobian below are what the generic host path uses.
// ------------------------------------------------------------------------------------------
namespace se3 {
template <typename T> inline void QuatMul(const T* a, const T* b, T* o) {
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
template <typename T> inline void QuatRotate(const T* q, const T* v, T* o) {     // R(q) v = v + 2w (u x v) + 2 u x (u x v)
    const T u0 = q[0], u1 = q[1], u2 = q[2], w = q[3];
    const T a0 = T(2.0) * (u1 * v[2] - u2 * v[1]), a1 = T(2.0) * (u2 * v[0] - u0 * v[2]), a2 = T(2.0) * (u0 * v[1] - u1 * v[0]);
    o[0] = v[0] + w * a0 + (u1 * a2 - u2 * a1);
    o[1] = v[1] + w * a1 + (u2 * a0 - u0 * a2);
    o[2] = v[2] + w * a2 + (u0 * a1 - u1 * a0);
}
template <typename T> inline void Inverse(const T* a, T* o) {
    const T qc[4] = {-a[0], -a[1], -a[2], a[3]};
    T t[3];
    QuatRotate(qc, a + 4, t);
    for (int i = 0; i < 4; ++i) o[i] = qc[i];
    for (int i = 0; i < 3; ++i) o[4 + i] = -t[i];
}
template <typename T> inline void Compose(const T* a, const T* b, T* o) {
    T q[4], t[3];
    QuatMul(a, b, q);
    QuatRotate(a, b + 4, t);
    for (int i = 0; i < 4; ++i) o[i] = q[i];
    for (int i = 0; i < 3; ++i) o[4 + i] = t[i] + a[4 + i];
}
// Sophus SE3::log of (q, t) -> [rho, theta]
template <typename T> inline void Log(const T* P, T* xi) {
    const T n2 = P[0] * P[0] + P[1] * P[1] + P[2] * P[2], qw = P[3];
    T k;
    if (n2 < T(1e-20)) k = T(2.0) / qw - T(2.0 / 3.0) * n2 / (qw * qw * qw);
    else { const T n = sqrt(n2); k = T(2.0) * ((qw < T(0.0)) ? atan2(-n, -qw) : atan2(n, qw)) / n; }
    const T w[3] = {k * P[0], k * P[1], k * P[2]};
    const T th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    T a, b;
    if (th2 < T(1e-20)) { a = T(0.5) - th2 / T(24.0); b = T(1.0 / 6.0) - th2 / T(120.0); }
    else { const T th = sqrt(th2); a = (T(1.0) - cos(th)) / th2; b = (th - sin(th)) / (th2 * th); }
    const T K[9] = {T(0.0), -w[2], w[1], w[2], T(0.0), -w[0], -w[1], w[0], T(0.0)};
    T V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const T k2 = K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j] + K[i * 3 + 2] * K[6 + j];
            V[i * 3 + j] = (i == j ? T(1.0) : T(0.0)) + a * K[i * 3 + j] + b * k2;
        }
    const T aa = V[0], bb = V[1], cc = V[2], dd = V[3], ee = V[4], ff = V[5], gg = V[6], hh = V[7], ii = V[8];
    const T C0 = ee * ii - ff * hh, C1 = ff * gg - dd * ii, C2 = dd * hh - ee * gg;
    const T inv = T(1.0) / (aa * C0 + bb * C1 + cc * C2);
    const T* t = P + 4;
    xi[0] = inv * (C0 * t[0] + (cc * hh - bb * ii) * t[1] + (bb * ff - cc * ee) * t[2]);
    xi[1] = inv * (C1 * t[0] + (aa * ii - cc * gg) * t[1] + (cc * dd - aa * ff) * t[2]);
    xi[2] = inv * (C2 * t[0] + (bb * gg - aa * hh) * t[1] + (aa * ee - bb * dd) * t[2]);
    xi[3] = w[0]; xi[4] = w[1]; xi[5] = w[2];
}
// Sophus SE3::exp of [rho, theta] -> (q, t)
inline void Exp(const double* d, double* P) {
    const double* th = d + 3;
    const double th2 = th[0] * th[0] + th[1] * th[1] + th[2] * th[2];
    double im, re, a, b;
    if (th2 < 1e-20) { im = 0.5 - th2 / 48.0; re = 1.0 - th2 / 8.0; a = 0.5 - th2 / 24.0; b = 1.0 / 6.0 - th2 / 120.0; }
    else { const double t = std::sqrt(th2); im = std::sin(0.5 * t) / t; re = std::cos(0.5 * t); a = (1.0 - std::cos(t)) / th2; b = (t - std::sin(t)) / (th2 * t); }
    P[0] = im * th[0]; P[1] = im * th[1]; P[2] = im * th[2]; P[3] = re;
    const double K[9] = {0, -th[2], th[1], th[2], 0, -th[0], -th[1], th[0], 0};
    for (int i = 0; i < 3; ++i) {
        double s = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double k2 = K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j] + K[i * 3 + 2] * K[6 + j];
            s += ((i == j ? 1.0 : 0.0) + a * K[i * 3 + j] + b * k2) * d[j];
        }
        P[4 + i] = s;
    }
}
}  // namespace se3

class SE3RightPlus : public LocalParameterization {
public:
    bool Plus(const double* x, const double* d, double* out) const override {
        double e[7], o[7];
        se3::Exp(d, e);
        se3::Compose(x, e, o);
        const double n = std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
        for (int i = 0; i < 4; ++i) out[i] = o[i] / n;
        for (int i = 0; i < 3; ++i) out[4 + i] = o[4 + i];
        return true;
    }
    // d (x (+) delta) / d delta at 0, 7 x 6 row-major: the quaternion moves with theta only (the 4 x 3 block of
    // QuaternionRightPlus), the translation with rho only (R(q))
    bool ComputeJacobian(const double* x, double* J) const override {
        std::fill(J, J + 42, 0.0);
        const double qx = 0.5 * x[0], qy = 0.5 * x[1], qz = 0.5 * x[2], qw = 0.5 * x[3];
        const double M[12] = {qw, -qz, qy, qz, qw, -qx, -qy, qx, qw, -qx, -qy, -qz};
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 3; ++c) J[r * 6 + 3 + c] = M[r * 3 + c];
        for (int c = 0; c < 3; ++c) {
            double e[3] = {0, 0, 0}, col[3];
            e[c] = 1.0;
            se3::QuatRotate(x, e, col);
            for (int r = 0; r < 3; ++r) J[(4 + r) * 6 + c] = col[r];
        }
        return true;
    }
    int GlobalSize() const override { return 7; }
    int LocalSize() const override { return 6; }
};

class RelativePoseFactor : public SizedCostFunction<6, 7, 7> {
public:
    explicit RelativePoseFactor(const double* measurement) { std::memcpy(z_, measurement, sizeof z_); }
    // sqrt_information: W, 6 x 6 row-major in the tangent order [rho, theta] of the residual -- the edge becomes r = W log(...), its
    // cost 1/2 r^T (W^T W) r.  Any finite W; for an information matrix Omega = L L^T the device engine's convention is W = L^T
    // (stba_pg_set_information in include/stba.h)
    RelativePoseFactor(const double* measurement, const double* sqrt_information) : has_w_(true) {
        std::memcpy(z_, measurement, sizeof z_);
        std::memcpy(w_, sqrt_information, sizeof w_);
    }
    static RelativePoseFactor* Create(const double* measurement) { return new RelativePoseFactor(measurement); }
    static RelativePoseFactor* Create(const double* measurement, const double* sqrt_information) { return new RelativePoseFactor(measurement, sqrt_information); }
    const double* measurement() const { return z_; }
    const double* sqrt_information() const { return has_w_ ? w_ : nullptr; }      // nullptr: made without one (identity)
    template <typename T>
    bool operator()(const T* Ti, const T* Tj, T* r) const {
        T Z[7], Zi[7], Tii[7], A[7], E[7];
        for (int k = 0; k < 7; ++k) Z[k] = T(z_[k]);
        se3::Inverse(Z, Zi);
        se3::Inverse(Ti, Tii);
        se3::Compose(Tii, Tj, A);
        se3::Compose(Zi, A, E);
        if (E[3] < T(0.0)) for (int k = 0; k < 4; ++k) E[k] = -E[k];       // shortest rotation
        if (!has_w_) { se3::Log(E, r); return true; }
        T xi[6];
        se3::Log(E, xi);
        for (int a = 0; a < 6; ++a) {
            T s = T(0.0);
            for (int k = 0; k < 6; ++k) s = s + T(w_[a * 6 + k]) * xi[k];
            r[a] = s;
        }
        return true;
    }
    bool Evaluate(double const* const* p, double* residuals, double** jacobians) const override {
        if (!jacobians) return (*this)(p[0], p[1], residuals);
        using J14 = Jet<double, 14>;
        J14 x[14], out[6];
        for (int k = 0; k < 7; ++k) { x[k] = J14(p[0][k], k); x[7 + k] = J14(p[1][k], 7 + k); }
        (*this)(x, x + 7, out);
        for (int r = 0; r < 6; ++r) {
            residuals[r] = out[r].a;
            if (jacobians[0]) for (int k = 0; k < 7; ++k) jacobians[0][r * 7 + k] = out[r].v[k];
            if (jacobians[1]) for (int k = 0; k < 7; ++k) jacobians[1][r * 7 + k] = out[r].v[7 + k];
        }
        return true;
    }
private:
    double z_[7];
    double w_[36] = {0};
    bool has_w_ = false;
};

// A node pose prior of the pose graph (stba_pg_set_priors): r = W log(Z^-1 T) on ONE pose block with the SE3RightPlus chart
// -- RelativePoseFactor with its first pose at the identity, evaluated by that factor's own functor.  measurement: the prior pose Z
// (qx qy qz qw tx ty tz); sqrt_information: W, 6 x 6 row-major in the tangent order [rho, theta] (null: the identity; zero theta
// rows: a position-only prior, GPS).  A Problem of RelativePoseFactor blocks and such priors (added WITHOUT a LossFunction) still runs
// on the device pose-graph engine ("gpu-pg"); Evaluate below is what the generic host path uses.
class NodePosePriorFactor : public SizedCostFunction<6, 7> {
public:
    explicit NodePosePriorFactor(const double* measurement, const double* sqrt_information = nullptr)
        : edge_(sqrt_information ? RelativePoseFactor(measurement, sqrt_information) : RelativePoseFactor(measurement)) {}
    static NodePosePriorFactor* Create(const double* measurement, const double* sqrt_information = nullptr) {
        return new NodePosePriorFactor(measurement, sqrt_information);
    }
    const double* measurement() const { return edge_.measurement(); }
    const double* sqrt_information() const { return edge_.sqrt_information(); }      // nullptr: made without one (identity)
    template <typename T>
    bool operator()(const T* Tn, T* r) const {
        const T I7[7] = {T(0.0), T(0.0), T(0.0), T(1.0), T(0.0), T(0.0), T(0.0)};
        return edge_(I7, Tn, r);
    }
    bool Evaluate(double const* const* p, double* residuals, double** jacobians) const override {
        if (!jacobians || !jacobians[0]) return (*this)(p[0], residuals);
        using J7 = Jet<double, 7>;
        J7 x[7], out[6];
        for (int k = 0; k < 7; ++k) x[k] = J7(p[0][k], k);
        (*this)(x, out);
        for (int r = 0; r < 6; ++r) {
            residuals[r] = out[r].a;
            for (int k = 0; k < 7; ++k) jacobians[0][r * 7 + k] = out[r].v[k];
        }
        return true;
    }
private:
    RelativePoseFactor edge_;
};

// ------------------------------------------------------------------------------------------
// Problem
// ------------------------------------------------------------------------------------------
class Problem {
public:
    struct Options {
        Ownership cost_function_ownership = TAKE_OWNERSHIP, loss_function_ownership = TAKE_OWNERSHIP,
                  local_parameterization_ownership = TAKE_OWNERSHIP;
    };
    Problem() = default;
    explicit Problem(const Options& o) : options_(o) {}
    Problem(const Problem&) = delete;
    Problem& operator=(const Problem&) = delete;
    ~Problem() {
        // the reference never frees what it news (solver.hpp:104,258; test_ceres.h:56,106): the problem
        // owns cost functions and parameterisations, shared pointers are freed once.
        if (options_.cost_function_ownership == TAKE_OWNERSHIP) for (auto* c : owned_costs_) delete c;
        if (options_.local_parameterization_ownership == TAKE_OWNERSHIP) for (auto* l : owned_params_) delete l;
        if (options_.loss_function_ownership == TAKE_OWNERSHIP) for (auto* l : owned_losses_) delete l;
    }

    void AddParameterBlock(double* values, int size, LocalParameterization* local = nullptr) {
        Block& b = block(values, size);
        if (local) { b.local = local; owned_params_.insert(local); }
    }
    template <typename... Ts>
    void AddResidualBlock(CostFunction* cost, LossFunction* loss, double* x0, Ts*... xs) {
        double* const b[] = {x0, xs...};
        AddResidualBlock(cost, loss, b, 1 + sizeof...(xs));
    }
    void AddResidualBlock(CostFunction* cost, LossFunction* loss, std::initializer_list<double*> blocks) {
        AddResidualBlock(cost, loss, blocks.begin(), blocks.size());
    }
    void AddResidualBlock(CostFunction* cost, LossFunction* loss, const std::vector<double*>& blocks) {
        AddResidualBlock(cost, loss, blocks.data(), blocks.size());
    }
    void AddResidualBlock(CostFunction* cost, LossFunction* loss, double* const* blocks, size_t n_blocks) {
        Residual r;
        r.cost = cost;
        r.loss = loss;
        const auto& sizes = cost->parameter_block_sizes();
        if (sizes.size() != n_blocks) { std::fprintf(stderr, "stba_ceres: block count mismatch\n"); std::abort(); }
        r.blocks.pool = &block_pool_; r.blocks.off = (int)block_pool_.size(); r.blocks.n = (int)n_blocks;
        for (size_t i = 0; i < n_blocks; ++i) block_pool_.push_back(block(blocks[i], sizes[i]).index);
        residuals_.push_back(r);
        // (a cost function shared by several residual blocks is listed once: the mark lives in the cost function -- sorting 10^6
        // pointers at destruction was a fifth of the destructor's time)
        if (options_.cost_function_ownership == TAKE_OWNERSHIP && !cost->owned_by_problem_) { cost->owned_by_problem_ = true; owned_costs_.push_back(cost); }
        if (loss) { owned_losses_.insert(loss); ++num_loss_functions_; }
    }
    int NumLossFunctions() const { return num_loss_functions_; }   // residual blocks added with a non-null LossFunction (Solve takes them on gpu-pg, and on gpu-ba with bundle_adjustment_losses)
    void SetParameterBlockConstant(double* values) { find(values).constant = true; }
    void SetParameterBlockVariable(double* values) { find(values).constant = false; }
    void SetParameterLowerBound(double* values, int index, double lower) { Block& b = find(values); b.ensure_bounds(); b.lower[index] = lower; }
    void SetParameterUpperBound(double* values, int index, double upper) { Block& b = find(values); b.ensure_bounds(); b.upper[index] = upper; }
    int NumParameterBlocks() const { return (int)blocks_.size(); }
    int NumResidualBlocks() const { return (int)residuals_.size(); }
    int NumResiduals() const { int n = 0; for (auto& r : residuals_) n += r.cost->num_residuals(); return n; }

    // ---- internals used by Solve ----
    struct Block {
        double* ptr = nullptr; int size = 0, index = 0; bool constant = false;
        LocalParameterization* local = nullptr;
        std::vector<double> lower, upper;
        int local_size() const { return local ? local->LocalSize() : size; }
        void ensure_bounds() { if (lower.empty()) { lower.assign(size, -1e300); upper.assign(size, 1e300); } }
    };
    // the parameter blocks of one residual block: a view into the problem's one index pool (a std::vector per residual block was
    // a heap allocation per observation: 10^6 of them at config C5)
    struct BlockList {
        const std::vector<int>* pool = nullptr; int off = 0, n = 0;
        size_t size() const { return (size_t)n; }
        int operator[](size_t i) const { return (*pool)[(size_t)off + i]; }
        const int* begin() const { return pool->data() + off; }
        const int* end() const { return pool->data() + off + n; }
    };
    struct Residual { CostFunction* cost = nullptr; LossFunction* loss = nullptr; BlockList blocks; };
    std::vector<Block>& blocks() { return blocks_; }
    std::vector<Residual>& residuals() { return residuals_; }

private:
    // parameter block pointer -> index: an open-addressing table (four look-ups per residual block at the reference's BA call site,
    // 4 x 10^6 at C5: std::unordered_map's node per key and its modulo were a third of the construction time)
    struct PtrIndex {
        std::vector<double*> keys; std::vector<int> vals; size_t used = 0; int shift = 64;
        static size_t mix(const double* p) { return (size_t)((reinterpret_cast<std::uintptr_t>(p) >> 3) * 0x9E3779B97F4A7C15ull); }
        void grow() {
            const size_t cap = keys.empty() ? 64 : keys.size() * 2;       // (small first: a PnP problem has two blocks)
            std::vector<double*> k2(cap, nullptr); std::vector<int> v2(cap, 0);
            int sh = 64; for (size_t c = cap; c > 1; c >>= 1) --sh;
            for (size_t q = 0; q < keys.size(); ++q) if (keys[q]) {
                size_t h = mix(keys[q]) >> sh;
                while (k2[h]) h = (h + 1) & (cap - 1);
                k2[h] = keys[q]; v2[h] = vals[q];
            }
            keys.swap(k2); vals.swap(v2); shift = sh;
        }
        int find(const double* p) const {
            if (keys.empty()) return -1;
            const size_t mask = keys.size() - 1;
            for (size_t h = mix(p) >> shift;; h = (h + 1) & mask) { if (keys[h] == p) return vals[h]; if (!keys[h]) return -1; }
        }
        void insert(double* p, int v) {
            if (2 * (used + 1) > keys.size()) grow();
            const size_t mask = keys.size() - 1;
            size_t h = mix(p) >> shift;
            while (keys[h]) h = (h + 1) & mask;
            keys[h] = p; vals[h] = v; ++used;
        }
    };
    Block& block(double* p, int size) {
        const int at = index_.find(p);
        if (at >= 0) {
            if (blocks_[(size_t)at].size != size) { std::fprintf(stderr, "stba_ceres: block re-added with another size\n"); std::abort(); }
            return blocks_[(size_t)at];
        }
        Block b; b.ptr = p; b.size = size; b.index = (int)blocks_.size();
        index_.insert(p, b.index);
        blocks_.push_back(b);
        return blocks_.back();
    }
    Block& find(double* p) {
        const int at = index_.find(p);
        if (at < 0) { std::fprintf(stderr, "stba_ceres: unknown parameter block\n"); std::abort(); }
        return blocks_[(size_t)at];
    }
    Options options_;
    std::vector<Block> blocks_;
    std::vector<Residual> residuals_;
    std::vector<int> block_pool_;
    PtrIndex index_;
    std::vector<CostFunction*> owned_costs_;       // (every cost function once: CostFunction::owned_by_problem_)
    int num_loss_functions_ = 0;
    std::set<LocalParameterization*> owned_params_;
    std::set<LossFunction*> owned_losses_;
};

// ------------------------------------------------------------------------------------------
// ParameterBlockOrdering (Ceres' OrderedGroups<double*>): parameter blocks in groups with integer ids >= 0, the order of the
// inner iterations' sweep (Solver::Options::inner_iteration_ordering)
// ------------------------------------------------------------------------------------------
class ParameterBlockOrdering {
public:
    bool AddElementToGroup(double* element, int group) {
        if (group < 0) return false;
        auto it = element_to_group_.find(element);
        if (it != element_to_group_.end()) {
            if (it->second == group) return true;
            Erase(element, it->second);
        }
        element_to_group_[element] = group;
        group_to_elements_[group].insert(element);
        return true;
    }
    int Remove(double* element) {
        auto it = element_to_group_.find(element);
        if (it == element_to_group_.end()) return 0;
        Erase(element, it->second);
        element_to_group_.erase(element);
        return 1;
    }
    bool IsMember(double* element) const { return element_to_group_.count(element) != 0; }
    int GroupId(double* element) const {
        auto it = element_to_group_.find(element);
        return it == element_to_group_.end() ? -1 : it->second;
    }
    int NumElements() const { return (int)element_to_group_.size(); }
    int NumGroups() const { return (int)group_to_elements_.size(); }
    int GroupSize(int group) const {
        auto it = group_to_elements_.find(group);
        return it == group_to_elements_.end() ? 0 : (int)it->second.size();
    }
    // Ceres' Reverse: the last group keeps its id, the others follow it in reverse order with ids one larger each
    void Reverse() {
        if (group_to_elements_.empty()) return;
        auto it = group_to_elements_.rbegin();
        std::map<int, std::set<double*>> out;
        out[it->first] = it->second;
        int id = it->first + 1;
        for (++it; it != group_to_elements_.rend(); ++it, ++id)
            for (double* e : it->second) { out[id].insert(e); element_to_group_[e] = id; }
        group_to_elements_.swap(out);
    }
    void Clear() { element_to_group_.clear(); group_to_elements_.clear(); }
    const std::map<int, std::set<double*>>& group_to_elements() const { return group_to_elements_; }

private:
    void Erase(double* element, int group) {
        auto g = group_to_elements_.find(group);
        g->second.erase(element);
        if (g->second.empty()) group_to_elements_.erase(g);
    }
    std::map<double*, int> element_to_group_;
    std::map<int, std::set<double*>> group_to_elements_;
};

// ------------------------------------------------------------------------------------------
// Solver
// ------------------------------------------------------------------------------------------
class Solver {
public:
    struct Options {
        int max_num_iterations = 50;
        int num_threads = 1;
        LinearSolverType linear_solver_type = SPARSE_NORMAL_CHOLESKY;
        PreconditionerType preconditioner_type = JACOBI;          // Ceres' defaults for the iterative linear solver
        TrustRegionStrategyType trust_region_strategy_type = LEVENBERG_MARQUARDT;
        DoglegType dogleg_type = TRADITIONAL_DOGLEG;
        double eta = 1e-1;
        int min_linear_solver_iterations = 0, max_linear_solver_iterations = 500;
        bool minimizer_progress_to_stdout = false;
        bool update_state_every_iteration = false;
        std::vector<IterationCallback*> callbacks;
        double initial_trust_region_radius = 1e4, max_trust_region_radius = 1e16, min_trust_region_radius = 1e-32,
               min_relative_decrease = 1e-3, min_lm_diagonal = 1e-6, max_lm_diagonal = 1e32,
               function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
        bool jacobi_scaling = true;
        bool force_callback_path = false;   // (not in Ceres) never replace user cost functions by the built-in device factor: see Solve()
        // (not in Ceres) let built-in LossFunctions through on a problem that takes "gpu-ba": see the comment above class LossFunction.
        // Off by default: without it a loss on a bundle-adjustment problem is refused, as it always was.
        bool bundle_adjustment_losses = false;
        // inner iterations on the "gpu-ba" path: a coordinate-descent sweep behind every valid step.  Default ordering:
        // {every rotation block}, {every position block}, {every landmark} -- Ceres' choice between rotations and positions for the
        // first group depends on hash order; this is its deterministic instance.  Refused before any device work (FAILURE, the reason
        // in Summary::message and on stderr, parameters untouched): with DOGLEG, a negative tolerance, an ordering whose group is not an
        // independent set (a camera's rotation and position, or a camera part and a landmark it observes) or that names a pointer
        // that is not a parameter block, and on problems that take "gpu-ba-hostjac", "gpu-pg" or "gpu-dense-callback".
        bool use_inner_iterations = false;
        double inner_iteration_tolerance = 1e-3;
        std::shared_ptr<ParameterBlockOrdering> inner_iteration_ordering;
    };
    struct Summary {
        TerminationType termination_type = FAILURE;
        std::string message;
        double initial_cost = 0, final_cost = 0;
        // Ceres' own timing fields: everything inside Solve() / in front of the minimiser / the minimiser / behind it
        double total_time_in_seconds = 0, preprocessor_time_in_seconds = 0, minimizer_time_in_seconds = 0, postprocessor_time_in_seconds = 0;
        // (not in Ceres) where the host side of the drop-in spends its time, seconds: recognise = the recognition and the route decision (structure, probes, every
        // user block at its start point); pack = parameters and masks into the engine's arrays; engine_create = stba_*_create (regrouping,
        // Schur plan, uploads); device_solve = stba_*_solve; write_back = parameters back into the user's blocks; verify = every
        // recognised user block at the end point; resolve = a second solve with the user's own code, if the verification failed
        struct Phases { double recognise = 0, pack = 0, engine_create = 0, device_solve = 0, write_back = 0, verify = 0, resolve = 0; } phases;
        int num_successful_steps = 0, num_unsuccessful_steps = 0;
        // ITERATIVE_SCHUR on a BA path; 0 (DENSE_NORMAL_CHOLESKY's value) on every other path, which this field does not describe
        LinearSolverType linear_solver_type_used = static_cast<LinearSolverType>(0);
        // the strategy that ran: DOGLEG / TRADITIONAL_DOGLEG where a BA path ran it, LEVENBERG_MARQUARDT on every other path
        TrustRegionStrategyType trust_region_strategy_type = LEVENBERG_MARQUARDT;
        DoglegType dogleg_type = TRADITIONAL_DOGLEG;
        std::vector<IterationSummary> iterations;
        std::string execution_path;   // "gpu-ba" | "gpu-ba-hostjac" | "gpu-pg" | "gpu-dense-callback"
        // inner iterations: asked for / run; group sizes of the ordering given (empty: none) and of the one used (constant blocks
        // left out); sweeps run; their device time (-1: no sweep ran)
        bool inner_iterations_given = false, inner_iterations_used = false;
        std::vector<int> inner_iteration_ordering_given, inner_iteration_ordering_used;
        int num_inner_iteration_steps = -1;
        double inner_iteration_time_in_seconds = -1.0;
        std::string BriefReport() const {
            char buf[512];
            const char* t = termination_type == CONVERGENCE ? "CONVERGENCE" : termination_type == NO_CONVERGENCE ? "NO_CONVERGENCE"
                            : termination_type == FAILURE ? "FAILURE" : "USER";
            std::snprintf(buf, sizeof buf, "stba Solver Summary: Iterations: %d, Initial cost: %e, Final cost: %e, Termination: %s",
                          (int)iterations.size(), initial_cost, final_cost, t);
            return buf;
        }
        std::string FullReport() const { return BriefReport() + " [" + execution_path + "] " + message; }
    };
};

namespace internal {

inline stba_lm_options ToC(const Solver::Options& o) {
    stba_lm_options c;
    stba_lm_default_options(&c);
    c.max_num_iterations = o.max_num_iterations;
    c.initial_trust_region_radius = o.initial_trust_region_radius;
    c.max_trust_region_radius = o.max_trust_region_radius;
    c.min_trust_region_radius = o.min_trust_region_radius;
    c.min_relative_decrease = o.min_relative_decrease;
    c.min_lm_diagonal = o.min_lm_diagonal;
    c.max_lm_diagonal = o.max_lm_diagonal;
    c.function_tolerance = o.function_tolerance;
    c.gradient_tolerance = o.gradient_tolerance;
    c.parameter_tolerance = o.parameter_tolerance;
    c.jacobi_scaling = o.jacobi_scaling ? 1 : 0;
    c.num_threads = o.num_threads;
    c.minimizer_progress_to_stdout = o.minimizer_progress_to_stdout ? 1 : 0;
    c.update_state_every_iteration = o.update_state_every_iteration ? 1 : 0;
    return c;
}

struct CallbackCtx {
    const Solver::Options* options;
    Solver::Summary* summary;
    void (*sync_state)(void*);   // copies the current iterate into the user's parameter memory
    void* sync_user;
    bool user_abort = false, user_success = false;
};

inline int IterationTrampoline(void* user, int iteration, double cost, double cost_change, double gradient_max_norm,
                               double step_norm, double radius, int ok) {
    auto* ctx = static_cast<CallbackCtx*>(user);
    IterationSummary it;
    it.iteration = iteration; it.cost = cost; it.cost_change = cost_change; it.gradient_max_norm = gradient_max_norm;
    it.step_norm = step_norm; it.trust_region_radius = radius; it.step_is_valid = true; it.step_is_successful = ok != 0;
    if (!ctx->options->callbacks.empty() && ctx->options->update_state_every_iteration && ctx->sync_state)
        ctx->sync_state(ctx->sync_user);   // solver.hpp:233,238: the callback dereferences the live state
    for (auto* cb : ctx->options->callbacks) {
        const CallbackReturnType r = (*cb)(it);
        if (r == SOLVER_ABORT) { ctx->user_abort = true; return 1; }
        if (r == SOLVER_TERMINATE_SUCCESSFULLY) { ctx->user_success = true; return 1; }
    }
    return 0;
}

inline void FillSummary(const stba_lm_summary& s, const std::vector<double>& trace, Solver::Summary* out) {
    out->initial_cost = s.initial_cost; out->final_cost = s.final_cost; out->minimizer_time_in_seconds = s.seconds_total;
    out->num_successful_steps = s.num_successful_steps; out->num_unsuccessful_steps = s.num_unsuccessful_steps;
    out->termination_type = s.termination_type == STBA_CONVERGENCE ? CONVERGENCE
                            : s.termination_type == STBA_NO_CONVERGENCE ? NO_CONVERGENCE : FAILURE;
    if (s.termination_type == STBA_FAILURE && !std::isfinite(s.initial_cost))
        out->message = "Initial residual and Jacobian evaluation failed.";      // (Ceres' wording for a non-finite start point)
    out->iterations.clear();
    for (int i = 0; i <= s.num_iterations; ++i) {
        const double* t = &trace[(size_t)i * STBA_TRACE_COLS];
        IterationSummary it;
        it.iteration = i; it.cost = t[0]; it.cost_change = t[1]; it.gradient_max_norm = t[2]; it.step_norm = t[3];
        it.relative_decrease = t[4]; it.trust_region_radius = t[5]; it.step_is_successful = t[6] != 0; it.step_is_valid = true;
        out->iterations.push_back(it);
    }
}

// ---- recognising the reprojection factor behind an arbitrary CostFunction ---------------------
// The reference's BA call site (st20-g2o/src/include/test_ceres.h:109-121) builds every residual block
// from its OWN functor (ns_st20::ProjectFactor behind DynamicAutoDiffCostFunction, blocks 4/3/3 -> 2).
// Such a block runs on the device if it IS the built-in factor: r = proj(conj(q) (L - t)) - feature.
inline void ReprojectionAt(const double* q, const double* t, const double* L, double* proj, double* pc_out = nullptr) {
    const double u0 = -q[0], u1 = -q[1], u2 = -q[2], w = q[3];
    const double v0 = L[0] - t[0], v1 = L[1] - t[1], v2 = L[2] - t[2];
    const double a0 = 2.0 * (u1 * v2 - u2 * v1), a1 = 2.0 * (u2 * v0 - u0 * v2), a2 = 2.0 * (u0 * v1 - u1 * v0);
    const double x = v0 + w * a0 + (u1 * a2 - u2 * a1), y = v1 + w * a1 + (u2 * a0 - u0 * a2), z = v2 + w * a2 + (u0 * a1 - u1 * a0);
    proj[0] = x / z; proj[1] = y / z;
    if (pc_out) { pc_out[0] = x; pc_out[1] = y; pc_out[2] = z; }
}

// generic probe points (unit quaternions, landmark well in front of the camera)
struct ProbePoint { double q[4], t[3], L[3]; };
inline const ProbePoint* ProbePoints() {
    // (the third point has a different geometry: a rotation of more than 90 degrees and a landmark that projects far off
    // the optical axis, |x/z| ~ 1.9: a cost that clamps or guards large image coordinates differs here)
    // (the fourth point lies BEHIND the camera, z = -1.6 in the camera frame: the built-in factor divides by z whatever its sign,
    // as the reference's functor does (test_ceres.h:72-78); a cost with a cheirality guard differs here and keeps its own code --
    // on the host-linearised device path if the problem is BA-shaped)
    static const ProbePoint pts[4] = {
        {{0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214}, {0.3, -0.2, 0.1}, {1.1, 0.7, 2.9}},
        {{-0.2721655269759087, 0.1360827634879543, 0.4082482904638630, 0.8606629658238704}, {-0.4, 0.25, -0.6}, {0.2, -0.9, 3.3}},
        {{0.0, 0.8, 0.0, 0.6}, {0.5, 0.1, -0.2}, {1.035, -0.775, -2.83}},
        {{0.0, 0.0, 0.0, 1.0}, {0.2, -0.1, 0.4}, {0.9, 0.3, -1.2}}};
    return pts;
}

// The recognition's value checks, per residual block.  `feature` is recovered at the canonical point (identity rotation, camera at
// the origin, landmark on the optical axis: proj = 0, so feature = -residual); the block must then equal proj - feature
//   * at four generic probe points -- the FIRST block of every C++ type (ProbeReprojectionValue; with the Jacobian check below),
//   * AT ITS OWN DATA -- the parameter values it holds when Solve is called and the values it holds when the solve ends -- EVERY
//     block (ReprojectionValueAtData): a block's own data is a generic point of its own (some rotation, some camera position, some
//     landmark), so a per-instance weight, intrinsic or clamp shows there.
// Doubles only, no Jacobians: two evaluations per block before the solve and one after it (round 6; five + one + one until round 5,
// which was 0.22 s of a C5 Solve()).
inline bool IsReprojectionShape(const CostFunction* cost) {
    const auto& sz = cost->parameter_block_sizes();
    return cost->num_residuals() == 2 && sz.size() == 3 && sz[0] == 4 && sz[1] == 3 && sz[2] == 3;
}
inline bool CanonicalFeature(const CostFunction* cost, double* feature) {
    const double q0[4] = {0, 0, 0, 1}, t0[3] = {0, 0, 0}, L0[3] = {0, 0, 1};
    const double* p0[3] = {q0, t0, L0};
    double r[2] = {0, 0};
    if (!cost->Evaluate(p0, r, nullptr) || !std::isfinite(r[0]) || !std::isfinite(r[1])) return false;
    feature[0] = -r[0]; feature[1] = -r[1];
    return true;
}
inline bool ProbeReprojectionValue(const CostFunction* cost, double* feature) {
    if (!IsReprojectionShape(cost) || !CanonicalFeature(cost, feature)) return false;
    const ProbePoint* pp = ProbePoints();
    double r[2];
    for (int k = 0; k < 4; ++k) {
        const double* p[3] = {pp[k].q, pp[k].t, pp[k].L};
        double proj[2];
        ReprojectionAt(pp[k].q, pp[k].t, pp[k].L, proj);
        if (!cost->Evaluate(p, r, nullptr)) return false;
        for (int i = 0; i < 2; ++i)
            if (!(std::fabs(r[i] - (proj[i] - feature[i])) <= 1e-12 * (1.0 + std::fabs(proj[i]) + std::fabs(feature[i])))) return false;
    }
    return true;
}

// value check of one residual block AT ITS OWN DATA.  The tolerance grows with |L - t| / |z|: near z = 0 the projection is
// ill-conditioned and two correct ways of computing it differ by more than 1e-11 (advisor, round 5).
inline bool ReprojectionValueAtData(const CostFunction* cost, const double* q, const double* t, const double* L, const double* feature) {
    const double* p[3] = {q, t, L};
    double r[2] = {0, 0}, proj[2], pc[3];
    if (!cost->Evaluate(p, r, nullptr)) return false;
    ReprojectionAt(q, t, L, proj, pc);
    const double amp = std::max(1.0, (std::fabs(pc[0]) + std::fabs(pc[1]) + std::fabs(pc[2])) / std::fabs(pc[2]));
    for (int i = 0; i < 2; ++i)
        if (!(std::fabs(r[i] - (proj[i] - feature[i])) <= 1e-11 * amp * (1.0 + std::fabs(proj[i]) + std::fabs(feature[i])))) return false;
    return true;
}

// derivative check, once per cost-function TYPE: the ambient Jacobians the user's Evaluate returns, composed
// with the quaternion right-plus chart, must equal the closed form the HIP kernel evaluates
// (A hat(pInC) | -A R^T | A R^T, A = d proj / d pInC; SURVEY.md header fact 2).
inline bool ProbeReprojectionJacobian(const CostFunction* cost) {
    const ProbePoint& P = ProbePoints()[0];
    const double* p[3] = {P.q, P.t, P.L};
    double r[2], Jq[8], Jt[6], JL[6];
    double* J[3] = {Jq, Jt, JL};
    if (!cost->Evaluate(p, r, J)) return false;
    double plus[12];
    QuaternionRightPlus().ComputeJacobian(P.q, plus);
    double proj[2], pc[3];
    ReprojectionAt(P.q, P.t, P.L, proj, pc);
    const double zi = 1.0 / pc[2];
    const double A[6] = {zi, 0, -pc[0] * zi * zi, 0, zi, -pc[1] * zi * zi};
    const double H[9] = {0, -pc[2], pc[1], pc[2], 0, -pc[0], -pc[1], pc[0], 0};
    const double x = P.q[0], y = P.q[1], z = P.q[2], w = P.q[3];
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                         2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j) {
            double rot = 0, exp_rot = 0, exp_L = 0;
            for (int g = 0; g < 4; ++g) rot += Jq[i * 4 + g] * plus[g * 3 + j];
            for (int k = 0; k < 3; ++k) { exp_rot += A[i * 3 + k] * H[k * 3 + j]; exp_L += A[i * 3 + k] * R[j * 3 + k]; }   // (A R^T)_ij
            if (!(std::fabs(rot - exp_rot) <= 1e-9) || !(std::fabs(JL[i * 3 + j] - exp_L) <= 1e-9) ||
                !(std::fabs(Jt[i * 3 + j] + exp_L) <= 1e-9)) return false;
        }
    return true;
}

// joins a helper thread when the scope is left, however it is left
struct JoinOnExit {
    std::thread* t;
    ~JoinOnExit() { if (t && t->joinable()) t->join(); }
};

// [lo, hi) in `threads` contiguous ranges, one std::thread each (threads <= 1: inline).  Used for the per-block evaluations of the
// recognition only when Solver::Options::num_threads > 1 -- the caller's promise, as in Ceres, that Evaluate may run concurrently.
template <class F> inline void ParallelRanges(size_t n, int threads, F fn) {
    if (threads <= 1 || n < 4096) { fn((size_t)0, n); return; }
    const size_t nt = std::min<size_t>((size_t)threads, std::max<size_t>(1, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (size_t k = 0; k < nt; ++k) th.emplace_back(fn, n * k / nt, n * (k + 1) / nt);
    for (auto& t : th) t.join();
}

// ---- Problem -> layout: the tables both engines take, built the same way ----------------------
// [n] each, the residual blocks' losses as stba_ba_set_loss / stba_pg_set_loss take them (TRIVIAL, scale 1 for a block without one), in
// the order of the observations / edges; EMPTY if no block has a loss.  losses_known: every loss is a built-in (KnownLossRow)
struct LossTable {
    std::vector<int> loss_kind;
    std::vector<double> loss_a, loss_b, loss_scale;
    bool losses_known = true;
};
// the table of n blocks; block k is residual block res_of[k] (res_of EMPTY: residual block k)
inline void FillLossTable(Problem& p, const std::vector<int>& res_of, size_t n, LossTable* t) {
    t->loss_kind.clear(); t->loss_a.clear(); t->loss_b.clear(); t->loss_scale.clear();
    t->losses_known = true;
    if (p.NumLossFunctions() == 0) return;
    for (size_t k = 0; k < n; ++k) {
        const auto& r = p.residuals()[res_of.empty() ? k : (size_t)res_of[k]];
        int kind = STBA_LOSS_TRIVIAL;
        double a = 1.0, b = 1.0, scale = 1.0;
        if (r.loss && !KnownLossRow(r.loss, &kind, &a, &b, &scale)) t->losses_known = false;
        t->loss_kind.push_back(kind); t->loss_a.push_back(a); t->loss_b.push_back(b); t->loss_scale.push_back(scale);
    }
}
// row k of a per-block square-root-information table [n][dim x dim] (2 x 2: observations; 6 x 6: edges).  The table is EMPTY until
// the first factor that has one: that makes it, with the identity in every other row
inline void SetSqrtInfoRow(std::vector<double>* t, size_t n, int dim, size_t k, const double* w) {
    const size_t sz = (size_t)dim * dim;
    if (t->empty()) {
        t->assign(n * sz, 0.0);
        for (size_t i = 0; i < n; ++i) for (int a = 0; a < dim; ++a) (*t)[i * sz + (size_t)a * (dim + 1)] = 1.0;
    }
    std::memcpy(&(*t)[k * sz], w, sz * sizeof(double));
}

// ---- path 1: every residual block is the reprojection factor (built-in or recognised) --------
struct BaLayout : LossTable {                // (the losses: per observation, the order of obs_cam / obs_pt / feat)
    std::vector<int> rot_block, pos_block;   // per camera: Problem block indices
    std::vector<int> pt_block;               // per landmark
    std::vector<int> obs_cam, obs_pt;
    std::vector<double> feat;
    // [n_obs][4], the built-in factors' square-root information as stba_ba_set_sqrt_information takes it, gathered next to feat
    // (SetSqrtInfoRow)
    std::vector<double> sqrt_info;
    std::vector<unsigned char> user;         // per residual block: 1 = a user cost function taken over (0: the built-in factor)
    size_t n_user = 0;
    // PosePriorFactor blocks, set aside: camera, pose [7], W [36] as stba_ba_set_pose_priors takes them, in the order of
    // the residual blocks.  obs_res: observation index -> residual block index; EMPTY when the problem has no prior block -- then
    // observation k IS residual block k, as it always was, and nothing below looks at this
    std::vector<int> prior_cam, obs_res;
    std::vector<double> prior_pose, prior_w;
    // CameraRelativePoseFactor blocks, set aside the same way: the two cameras, measurement [7], W [36] as
    // stba_ba_set_relative_poses takes them
    std::vector<int> rel_i, rel_j;
    std::vector<double> rel_meas, rel_w;
    // LandmarkPriorFactor blocks, set aside the same way: the landmark, position [3], W [9] as
    // stba_ba_set_landmark_priors takes them
    std::vector<int> lp_pt;
    std::vector<double> lp_pos, lp_w;
    const Problem::Residual& res_of(Problem& p, size_t k) const { return p.residuals()[obs_res.empty() ? k : (size_t)obs_res[k]]; }
};

// every user block at the parameter values its blocks hold right now, against the factor with the block's feature.  take_features
// (L.feat's own storage): first take each block's feature, its residual at the canonical point; null: L.feat as it stands
inline bool CheckUserBlocks(Problem& p, const BaLayout& L, int threads, double* take_features) {
    if (!L.n_user) return true;
    auto& blk = p.blocks();
    std::atomic<int> bad{0};
    ParallelRanges(L.obs_cam.size(), threads, [&](size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; ++k) {
            if (!L.user[k]) continue;
            const auto& r = L.res_of(p, k);
            if ((take_features && !CanonicalFeature(r.cost, take_features + 2 * k)) ||
                !ReprojectionValueAtData(r.cost, blk[r.blocks[0]].ptr, blk[r.blocks[1]].ptr, blk[r.blocks[2]].ptr, &L.feat[2 * k])) { bad.store(1); return; }
        }
    });
    return bad.load() == 0;
}
// the end-point check of Solve: every recognised USER block once more, where the solve ended
inline bool VerifyRecognisedBlocks(Problem& p, const BaLayout& L, int threads) { return CheckUserBlocks(p, L, threads, nullptr); }
// the PER-BLOCK half of the recognition: every user block's feature and its value at its own data.  10^6 blocks = 2 x 10^6 calls of the
// user's Evaluate, on the calling thread (options.num_threads of them): the one part of the recognition that costs time -- Solve runs
// it while a helper thread creates the device engine (BaRun::Create).
inline bool DetectBaBlocks(Problem& p, BaLayout* L, int threads) { return CheckUserBlocks(p, *L, threads, L->feat.data()); }

// The STRUCTURE of a bundle adjustment, one pass, no Evaluate: every residual block {quaternion 4, position 3, landmark 3} -> 2 on
// blocks that form cameras and landmarks (4 -> 3 chart on the rotation, no other chart, no bounds), PosePriorFactor and
// CameraRelativePoseFactor blocks without a loss set aside.  The built-in factors' features and weights go to L; every other block is
// marked `user`, the first of each C++ type listed in *user_types for the per-type probes.
inline bool BaStructure(Problem& p, BaLayout* L, std::vector<const CostFunction*>* user_types) {
    auto& res = p.residuals();
    auto& blk = p.blocks();
    if (res.empty()) return false;
    const size_t nr = res.size();
    std::vector<int> cam_of_rot(blk.size(), -1), cam_of_pos(blk.size(), -1), pt_of(blk.size(), -1);
    L->obs_cam.resize(nr); L->obs_pt.resize(nr); L->feat.assign(2 * nr, 0.0); L->user.assign(nr, 0);
    const std::type_info* last_type = nullptr;
    bool last_builtin = false;
    std::vector<const std::type_info*> seen_types;
    // PosePriorFactor blocks are set aside (their residual block index and their two parameter blocks, resolved to a camera behind
    // the loop): from the first one on, observation k (the index of every per-observation array) is no longer residual block kr
    std::vector<size_t> prior_res, rel_res, lp_res;  // (rel_res: CameraRelativePoseFactor blocks, lp_res: LandmarkPriorFactor blocks, the same way)
    size_t k = 0;
    for (size_t kr = 0; kr < nr; ++kr) {
        const auto& r = res[kr];
        if (r.blocks.size() != 3 || !IsReprojectionShape(r.cost)) {
            const bool is_prior = r.blocks.size() == 2 && dynamic_cast<const PosePriorFactor*>(r.cost);
            const bool is_rel = r.blocks.size() == 4 && dynamic_cast<const CameraRelativePoseFactor*>(r.cost);
            const bool is_lp = r.blocks.size() == 1 && dynamic_cast<const LandmarkPriorFactor*>(r.cost);
            if (r.loss || !(is_prior || is_rel || is_lp)) return false;
            if (prior_res.empty() && rel_res.empty() && lp_res.empty()) { L->obs_res.resize(k); for (size_t i = 0; i < k; ++i) L->obs_res[i] = (int)i; }
            (is_prior ? prior_res : is_rel ? rel_res : lp_res).push_back(kr);
            continue;
        }
        if (!prior_res.empty() || !rel_res.empty() || !lp_res.empty()) L->obs_res.push_back((int)kr);
        const std::type_info& ti = typeid(*r.cost);
        if (!last_type || !(ti == *last_type)) {
            last_type = &ti;
            last_builtin = dynamic_cast<const ReprojectionFactor*>(r.cost) != nullptr;
            bool seen = false;
            for (auto* st : seen_types) seen = seen || (*st == ti);
            if (!seen) { seen_types.push_back(&ti); if (!last_builtin) user_types->push_back(r.cost); }
        }
        if (last_builtin) {
            auto* f = static_cast<const ReprojectionFactor*>(r.cost); L->feat[2 * k] = f->fx(); L->feat[2 * k + 1] = f->fy();
            // (a table of nr rows, filled at the observation index: cut to the observations below)
            if (const double* w = f->sqrt_information()) SetSqrtInfoRow(&L->sqrt_info, nr, 2, k, w);
        }
        else { L->user[k] = 1; ++L->n_user; }
        const int b0 = r.blocks[0], b1 = r.blocks[1], b2 = r.blocks[2];
        const auto& rb = blk[b0];
        // a user LocalParameterization with the 4 -> 3 signature is accepted only if it IS the quaternion right-plus (checked
        // numerically: UsesQuaternionRightPlus, Recognition::charts)
        if (!rb.local || rb.local->GlobalSize() != 4 || rb.local->LocalSize() != 3) return false;
        if (blk[b1].local || blk[b2].local) return false;
        if (!rb.lower.empty() || !blk[b1].lower.empty() || !blk[b2].lower.empty()) return false;
        int c = cam_of_rot[b0];
        if (c < 0) {
            if (cam_of_pos[b1] >= 0) return false;                 // a position block shared by two rotation blocks
            c = (int)L->rot_block.size(); cam_of_rot[b0] = c; cam_of_pos[b1] = c; L->rot_block.push_back(b0); L->pos_block.push_back(b1);
        } else if (L->pos_block[(size_t)c] != b1) return false;    // a rotation block shared by two cameras with different position blocks
        int j = pt_of[b2];
        if (j < 0) { j = (int)L->pt_block.size(); pt_of[b2] = j; L->pt_block.push_back(b2); }
        L->obs_cam[k] = c; L->obs_pt[k] = j;
        ++k;
    }
    if (!prior_res.empty() || !rel_res.empty() || !lp_res.empty()) {
        const size_t no = k;
        if (no == 0) return false;
        L->obs_cam.resize(no); L->obs_pt.resize(no); L->feat.resize(2 * no); L->user.resize(no);
        if (!L->sqrt_info.empty()) L->sqrt_info.resize(4 * no);
        for (size_t kr : prior_res) {
            // a prior's two blocks must be the rotation and the position block of ONE camera that some observation names
            const auto& r = res[kr];
            const int b0 = r.blocks[0], b1 = r.blocks[1];
            const int c = cam_of_rot[(size_t)b0];
            if (c < 0 || L->pos_block[(size_t)c] != b1) return false;
            auto* f = static_cast<const PosePriorFactor*>(r.cost);
            L->prior_cam.push_back(c);
            L->prior_pose.insert(L->prior_pose.end(), f->pose(), f->pose() + 7);
            L->prior_w.insert(L->prior_w.end(), f->weights(), f->weights() + 36);
        }
        for (size_t kr : rel_res) {
            // an edge's four blocks must be the rotation and position blocks of two DISTINCT cameras that observations name
            const auto& r = res[kr];
            const int ci = cam_of_rot[(size_t)r.blocks[0]], cj = cam_of_rot[(size_t)r.blocks[2]];
            if (ci < 0 || cj < 0 || ci == cj || L->pos_block[(size_t)ci] != r.blocks[1] || L->pos_block[(size_t)cj] != r.blocks[3]) return false;
            auto* f = static_cast<const CameraRelativePoseFactor*>(r.cost);
            L->rel_i.push_back(ci); L->rel_j.push_back(cj);
            L->rel_meas.insert(L->rel_meas.end(), f->measurement(), f->measurement() + 7);
            L->rel_w.insert(L->rel_w.end(), f->weights(), f->weights() + 36);
        }
        for (size_t kr : lp_res) {
            // a landmark prior's block must be a landmark that some observation names (which has neither chart nor bounds)
            const auto& r = res[kr];
            const int j = pt_of[(size_t)r.blocks[0]];
            if (j < 0) return false;
            auto* f = static_cast<const LandmarkPriorFactor*>(r.cost);
            L->lp_pt.push_back(j);
            L->lp_pos.insert(L->lp_pos.end(), f->position(), f->position() + 3);
            L->lp_w.insert(L->lp_w.end(), f->weights(), f->weights() + 9);
        }
    }
    for (size_t c = 0; c < L->rot_block.size(); ++c)                // a block cannot be a rotation AND a landmark / position
        if (pt_of[(size_t)L->rot_block[c]] >= 0 || pt_of[(size_t)L->pos_block[c]] >= 0 || cam_of_pos[(size_t)L->rot_block[c]] >= 0) return false;
    return true;
}

// numerically confirms that a user-supplied 4->3 parameterisation is q (x) exp(delta)
inline bool UsesQuaternionRightPlus(const LocalParameterization* lp) {
    if (dynamic_cast<const QuaternionRightPlus*>(lp)) return true;
    const double q[4] = {0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214};
    const double d[3] = {0.013, -0.021, 0.008};
    double a[4], b[4];
    QuaternionRightPlus ref;
    if (!lp->Plus(q, d, a)) return false;
    ref.Plus(q, d, b);
    for (int i = 0; i < 4; ++i) if (std::fabs(a[i] - b[i]) > 1e-13) return false;
    return true;
}

// ---- path 3's layout: a pose graph ------------------------------------------------------------
// every residual block a RelativePoseFactor on two distinct 7-double blocks, or a NodePosePriorFactor without a LossFunction on one,
// every block with the SE3RightPlus chart and no bounds, and at least one edge.  Nodes are numbered in the order the residual blocks
// first name them.
struct PoseGraphLayout : LossTable {       // (the losses: per edge)
    std::map<int, int> node_of;            // parameter block index -> node
    std::vector<int> node_block, ei, ej;   // node -> parameter block index; the edges
    std::vector<double> meas, poses;       // [m][7], [n][7] (the blocks' current values)
    std::vector<unsigned char> fixed;      // [n]
    std::vector<double> sqrt_info;         // [m][36] the factors' W (SetSqrtInfoRow)
    // NodePosePriorFactor blocks, set aside: node, pose [7], W [36] as stba_pg_set_priors takes them, in the order of the
    // residual blocks.  edge_res: edge -> residual block index; EMPTY when the problem has no prior block -- then edge e IS residual
    // block e, as it always was
    std::vector<int> prior_node, edge_res;
    std::vector<double> prior_pose, prior_w;
};
inline bool DetectPoseGraph(Problem* p, PoseGraphLayout* L) {
    const size_t nr = p->residuals().size();
    if (nr == 0) return false;
    // (a prior with a LossFunction, or a problem of priors only, is no pose graph of this engine)
    size_t m = 0;
    for (size_t k = 0; k < nr; ++k) {
        const auto& r = p->residuals()[k];
        if (r.blocks.size() == 1 && dynamic_cast<NodePosePriorFactor*>(r.cost)) { if (r.loss) return false; }
        else ++m;
    }
    if (m == 0) return false;
    const bool has_priors = m != nr;
    auto node_of_block = [&](int block, int* node) {
        const auto& b = p->blocks()[block];
        if (b.size != 7 || !b.local || !dynamic_cast<SE3RightPlus*>(b.local) || !b.lower.empty()) return false;
        auto it = L->node_of.find(block);
        if (it == L->node_of.end()) { *node = (int)L->node_block.size(); L->node_of[block] = *node; L->node_block.push_back(block); }
        else *node = it->second;
        return true;
    };
    size_t e = 0;
    for (size_t k = 0; k < nr; ++k) {
        const auto& r = p->residuals()[k];
        if (has_priors && r.blocks.size() == 1) {
            if (auto* pf = dynamic_cast<NodePosePriorFactor*>(r.cost)) {
                int node;
                if (!node_of_block(r.blocks[0], &node)) return false;
                L->prior_node.push_back(node);
                L->prior_pose.insert(L->prior_pose.end(), pf->measurement(), pf->measurement() + 7);
                const size_t at = L->prior_w.size();
                L->prior_w.resize(at + 36, 0.0);
                if (pf->sqrt_information()) std::memcpy(&L->prior_w[at], pf->sqrt_information(), 36 * sizeof(double));
                else for (int a = 0; a < 6; ++a) L->prior_w[at + (size_t)a * 7] = 1.0;
                continue;
            }
        }
        auto* f = dynamic_cast<RelativePoseFactor*>(r.cost);
        if (!f || r.blocks.size() != 2 || r.blocks[0] == r.blocks[1]) return false;
        int ends[2];
        for (int q = 0; q < 2; ++q)
            if (!node_of_block(r.blocks[q], &ends[q])) return false;
        L->ei.push_back(ends[0]); L->ej.push_back(ends[1]);
        L->meas.insert(L->meas.end(), f->measurement(), f->measurement() + 7);
        if (f->sqrt_information()) SetSqrtInfoRow(&L->sqrt_info, m, 6, e, f->sqrt_information());
        if (has_priors) L->edge_res.push_back((int)k);
        ++e;
    }
    FillLossTable(*p, L->edge_res, m, L);
    const int n = (int)L->node_block.size();
    L->poses.assign((size_t)n * 7, 0.0);
    L->fixed.assign((size_t)n, 0);
    for (int k = 0; k < n; ++k) {
        std::memcpy(&L->poses[(size_t)k * 7], p->blocks()[L->node_block[k]].ptr, 7 * sizeof(double));
        L->fixed[k] = p->blocks()[L->node_block[k]].constant ? 1 : 0;
    }
    return true;
}

// ---- the recognition: what a Problem is, read ONCE per Solve / Covariance::Compute -------------
// CONTRACT.  A user cost function is replaced by the built-in device factor if
//   * the first block of its C++ type equals proj(conj(q)(L - t)) - feature at four generic probe points, one of them behind the
//     camera (1e-12), and its Jacobian, composed with the chart, equals the closed form at a probe point (1e-9)  [Types()];
//   * EVERY block equals the factor AT ITS OWN DATA -- the parameter values it holds when Solve is called (1e-11) -- with the
//     feature it shows at the canonical point  [Blocks()], and once more at the point the solve ENDED at: a cost that departed from
//     the factor on the way is solved again with its own code (SolveDispatch).
// What remains unchecked is a cost that differs from the factor only at iterates in between; Solver::Options::force_callback_path
// = true (or STBA_CERES_FORCE_CALLBACK=1 in the environment) keeps every block on the generic path, where the user's Evaluate is
// what runs.  The summary's message names the number of blocks taken over.
// NOTE for callers with IterationCallbacks: if the end-point check fails, the callbacks have already fired for the discarded
// device solve and fire again for the second one (the summary's message says that a second solve ran; its iterations are the
// ones reported, the time of both is in total_time_in_seconds, the first one's under phases.resolve's complement).
//
// The two halves that call the user's Evaluate are lazy and cached: Types() (six calls per C++ type) and Blocks() (two calls per
// user block) run when a decision first needs them, at most once each, so no route calls Evaluate for an answer it does not use.
struct Recognition {
    Problem* problem = nullptr;
    int threads = 1;
    bool force_callback = false;     // force_callback_path or STBA_CERES_FORCE_CALLBACK: never take a user cost for the device factor
    bool structure = false;          // BaStructure holds; `ba` is its layout (priors, relative poses, sqrt_info included)
    bool charts = false;             // ... and every rotation block's chart is the quaternion right-plus
    bool ba_losses = false;          // asked for, and: the device-factor reading holds, blocks included, and every loss is a built-in
    bool is_pg = false;              // DetectPoseGraph holds; `pg` is its layout.  Looked at only where the BA structure does not hold
    BaLayout ba;
    PoseGraphLayout pg;
    std::vector<const CostFunction*> user_types;
    int types = -1, blocks = -1;     // the lazy halves: -1 not asked yet, 0 failed, 1 passed
    bool dropped = false;            // the end-point check failed: the device-factor reading is off

    bool Special() const { return !ba.prior_cam.empty() || !ba.rel_i.empty() || !ba.lp_pt.empty(); }
    // the camera-side factors, which DOGLEG and ITERATIVE_SCHUR engines do not take (LandmarkPriorFactor blocks they do)
    bool CameraSpecial() const { return !ba.prior_cam.empty() || !ba.rel_i.empty(); }
    // the shape-only reading (blocks 4 / 3 / 3 -> 2, no prior or relative-pose block): the factor may stay the user's ("gpu-ba-hostjac")
    bool ShapeRaw() const { return structure && !Special(); }
    bool Shape() const { return ShapeRaw() && charts; }
    bool Types() {
        if (types < 0) {
            types = 1;
            double f[2];
            for (auto* c : user_types) if (!ProbeReprojectionValue(c, f) || !ProbeReprojectionJacobian(c)) { types = 0; break; }
        }
        return types == 1;
    }
    bool Blocks() {
        if (blocks < 0) blocks = DetectBaBlocks(*problem, &ba, threads) ? 1 : 0;
        return blocks == 1;
    }
    // the device-factor reading ("gpu-ba"), as far as it has been checked: Blocks() may still be to come.  NOT a plain query: the
    // first call that gets past the cheap conditions runs the per-type probes (Types(): the user's Evaluate)
    bool Factor() { return !force_callback && !dropped && structure && charts && blocks != 0 && Types(); }
    // `ba` as the shape-only reading hands it to the engine: no features, nothing taken over, no weights (the factors whiten themselves)
    void MakeShapeOnly() {
        std::fill(ba.feat.begin(), ba.feat.end(), 0.0); std::fill(ba.user.begin(), ba.user.end(), 0);
        ba.n_user = 0; ba.sqrt_info.clear();
    }
};

// the one parsing of the force-callback switch
inline bool ForceCallbackPath(bool option) {
    const char* fe = std::getenv("STBA_CERES_FORCE_CALLBACK");
    return option || (fe && *fe && *fe != '0');
}

// want_ba_losses: the caller would take built-in losses on "gpu-ba" -- then, on a problem that has losses, the whole device-factor
// reading is checked here, blocks included, because the answer decides a refusal that comes before any device work
inline void Recognise(Problem& p, bool force_callback, bool want_ba_losses, int threads, Recognition* r) {
    r->problem = &p; r->threads = threads; r->force_callback = force_callback;
    r->structure = BaStructure(p, &r->ba, &r->user_types);
    if (!r->structure) { r->is_pg = DetectPoseGraph(&p, &r->pg); return; }
    r->charts = true;
    for (int rb : r->ba.rot_block) r->charts = r->charts && UsesQuaternionRightPlus(p.blocks()[rb].local);
    if (!want_ba_losses || p.NumLossFunctions() == 0 || !r->Factor()) return;
    FillLossTable(p, r->ba.obs_res, r->ba.obs_cam.size(), &r->ba);
    r->ba_losses = r->ba.losses_known && r->Blocks();
    if (!r->ba_losses) {        // (no table on any other route; losses_known keeps what was found)
        r->ba.loss_kind.clear(); r->ba.loss_a.clear(); r->ba.loss_b.clear(); r->ba.loss_scale.clear();
    }
}

// ---- the BA engine behind Solve and Covariance: pack, create, configure -----------------------
// cameras [nc][7], landmarks [np][3] and the fixed masks ([nc][6]: rotation, position; [np]) as stba_ba_create takes them
struct BaPacked { std::vector<double> cams, pts; std::vector<unsigned char> cam_fixed, pt_fixed; };
inline void PackBa(Problem& p, const BaLayout& L, BaPacked* out) {
    const size_t nc = L.rot_block.size(), np = L.pt_block.size();
    out->cams.resize(nc * 7); out->pts.resize(np * 3); out->cam_fixed.assign(nc * 6, 0); out->pt_fixed.assign(np, 0);
    for (size_t c = 0; c < nc; ++c) {
        const auto& rb = p.blocks()[L.rot_block[c]]; const auto& pb = p.blocks()[L.pos_block[c]];
        std::memcpy(&out->cams[c * 7], rb.ptr, 4 * sizeof(double));
        std::memcpy(&out->cams[c * 7 + 4], pb.ptr, 3 * sizeof(double));
        for (int k = 0; k < 3; ++k) { out->cam_fixed[c * 6 + k] = rb.constant ? 1 : 0; out->cam_fixed[c * 6 + 3 + k] = pb.constant ? 1 : 0; }
    }
    for (size_t j = 0; j < np; ++j) {
        std::memcpy(&out->pts[j * 3], p.blocks()[L.pt_block[j]].ptr, 3 * sizeof(double));
        out->pt_fixed[j] = p.blocks()[L.pt_block[j]].constant ? 1 : 0;
    }
}
// the engine's parameters back into the user's blocks (also the IterationCallbacks' sync_state)
struct BaSync { stba_ba* ba; Problem* p; const BaLayout* L; BaPacked* x; };
inline void BaCopyOut(void* user) {
    auto* s = static_cast<BaSync*>(user);
    if (stba_ba_get_params(s->ba, s->x->cams.data(), s->x->pts.data()) != STBA_OK) return;
    for (size_t c = 0; c < s->L->rot_block.size(); ++c) {
        std::memcpy(s->p->blocks()[s->L->rot_block[c]].ptr, &s->x->cams[c * 7], 4 * sizeof(double));
        std::memcpy(s->p->blocks()[s->L->pos_block[c]].ptr, &s->x->cams[c * 7 + 4], 3 * sizeof(double));
    }
    for (size_t j = 0; j < s->L->pt_block.size(); ++j)
        std::memcpy(s->p->blocks()[s->L->pt_block[j]].ptr, &s->x->pts[j * 3], 3 * sizeof(double));
}

// host lineariser of the "gpu-ba-hostjac" path (stba_ba_set_host_linearizer): the user's cost functions, evaluated in bulk at
// the engine's current parameters, in residual-block order; the camera Jacobian is composed with the rotation block's chart
// (2x4 . 4x3) next to the 2x3 position block.  options.num_threads > 1 (and an OpenMP build) evaluates blocks in parallel,
// as Ceres does -- the reference pins num_threads = 1 (test_ceres.h:143).
struct BaHostCtx { Problem* p; const BaLayout* L; int threads; };
inline int BaHostLinearize(void* user, const double* cams, const double* pts, double* r, double* Jc, double* Jp) {
    auto* c = static_cast<BaHostCtx*>(user);
    auto& res = c->p->residuals();
    const int no = (int)res.size();
    int bad = 0;
#if defined(_OPENMP)
#pragma omp parallel for schedule(static) num_threads(c->threads > 1 ? c->threads : 1) reduction(+ : bad)
#endif
    for (int i = 0; i < no; ++i) {
        const double* q = cams + (size_t)c->L->obs_cam[i] * 7;
        const double* prm[3] = {q, q + 4, pts + (size_t)c->L->obs_pt[i] * 3};
        double Jq[8], Jt[6], JL[6];
        double* J[3] = {Jq, Jt, JL};
        if (!res[i].cost->Evaluate(prm, r + (size_t)i * 2, Jc ? J : nullptr)) { ++bad; continue; }
        if (!Jc) continue;
        double plus[12];
        const LocalParameterization* lp = c->p->blocks()[res[i].blocks[0]].local;
        if (!lp->ComputeJacobian(q, plus)) { ++bad; continue; }
        for (int row = 0; row < 2; ++row) {
            for (int l = 0; l < 3; ++l) {
                double sacc = 0.0;
                for (int g = 0; g < 4; ++g) sacc += Jq[row * 4 + g] * plus[g * 3 + l];
                Jc[(size_t)i * 12 + row * 6 + l] = sacc;
                Jc[(size_t)i * 12 + row * 6 + 3 + l] = Jt[row * 3 + l];
                Jp[(size_t)i * 6 + row * 3 + l] = JL[row * 3 + l];
            }
        }
    }
    return bad ? 1 : 0;
}

inline double WallSeconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the inner iterations' ordering in the engine's terms (stba_ba_set_inner_iterations): a group id per camera rotation, camera position
// and landmark (-1: not swept), and the sizes of the groups used (constant blocks left out)
struct InnerGroups {
    std::vector<int> rot, pos, pt;
    std::vector<int> sizes_given, sizes_used;
};

// Solver::Options::inner_iteration_ordering (or the default one) -> *out; false with *why if the ordering is refused
inline bool MakeInnerGroups(const Solver::Options& o, Problem& p, const BaLayout& L, InnerGroups* out, std::string* why) {
    const int nc = (int)L.rot_block.size(), np = (int)L.pt_block.size();
    out->rot.assign((size_t)nc, -1); out->pos.assign((size_t)nc, -1); out->pt.assign((size_t)np, -1);
    out->sizes_given.clear(); out->sizes_used.clear();
    const auto& blk = p.blocks();
    if (!o.inner_iteration_ordering) {
        std::fill(out->rot.begin(), out->rot.end(), 0); std::fill(out->pos.begin(), out->pos.end(), 1); std::fill(out->pt.begin(), out->pt.end(), 2);
    } else {
        std::unordered_map<const double*, std::pair<int, int>> where;    // block pointer -> (0 rotation | 1 position | 2 landmark, index)
        for (int c = 0; c < nc; ++c) { where[blk[L.rot_block[c]].ptr] = {0, c}; where[blk[L.pos_block[c]].ptr] = {1, c}; }
        for (int j = 0; j < np; ++j) where[blk[L.pt_block[j]].ptr] = {2, j};
        for (const auto& g : o.inner_iteration_ordering->group_to_elements()) {
            out->sizes_given.push_back((int)g.second.size());
            for (double* e : g.second) {
                auto it = where.find(e);
                if (it == where.end()) { *why = "the inner iteration ordering names a pointer that is not a parameter block of the problem"; return false; }
                (it->second.first == 0 ? out->rot : it->second.first == 1 ? out->pos : out->pt)[(size_t)it->second.second] = g.first;
            }
        }
    }
    for (int c = 0; c < nc; ++c) {           // (constant blocks are ignored)
        if (blk[L.rot_block[c]].constant) out->rot[(size_t)c] = -1;
        if (blk[L.pos_block[c]].constant) out->pos[(size_t)c] = -1;
        if (out->rot[(size_t)c] >= 0 && out->rot[(size_t)c] == out->pos[(size_t)c]) {
            *why = "inner iteration ordering: group " + std::to_string(out->rot[(size_t)c]) + " is not an independent set (the rotation and the "
                   "position of camera " + std::to_string(c) + " share residuals)";
            return false;
        }
    }
    for (int j = 0; j < np; ++j) if (blk[L.pt_block[j]].constant) out->pt[(size_t)j] = -1;
    for (size_t i = 0; i < L.obs_cam.size(); ++i) {
        const int c = L.obs_cam[i], j = L.obs_pt[i], g = out->pt[(size_t)j];
        if (g >= 0 && (g == out->rot[(size_t)c] || g == out->pos[(size_t)c])) {
            *why = "inner iteration ordering: group " + std::to_string(g) + " is not an independent set (camera " + std::to_string(c) +
                   " and landmark " + std::to_string(j) + " share a residual)";
            return false;
        }
    }
    std::map<int, int> used;
    for (int v : out->rot) if (v >= 0) ++used[v];
    for (int v : out->pos) if (v >= 0) ++used[v];
    for (int v : out->pt) if (v >= 0) ++used[v];
    for (const auto& u : used) out->sizes_used.push_back(u.second);
    return true;
}

// owns an engine handle: the one place that destroys it
struct BaEngine {
    stba_ba* h = nullptr;
    BaEngine() = default;
    BaEngine(const BaEngine&) = delete;
    BaEngine& operator=(const BaEngine&) = delete;
    ~BaEngine() { Reset(); }
    void Reset() { if (h) stba_ba_destroy(h); h = nullptr; }
};

// stba_ba_create, or stba_ba_create_ex + stba_ba_set_pcg for ITERATIVE_SCHUR (solve null: Covariance, the direct solver).  false with
// *error "call: text" -- the text taken here, on the thread that ran the call (stba_last_error is thread-local)
inline bool CreateBa(const BaLayout& L, const BaPacked& x, const Solver::Options* solve, BaEngine* e, std::string* error) {
    const int nc = (int)L.rot_block.size(), np = (int)L.pt_block.size(), no = (int)L.obs_cam.size();
    int rc;
    if (!solve || solve->linear_solver_type != ITERATIVE_SCHUR)
        rc = stba_ba_create(&e->h, nc, np, no, x.cams.data(), x.pts.data(), L.obs_cam.data(), L.obs_pt.data(), L.feat.data(), x.cam_fixed.data(),
                            x.pt_fixed.data(), nullptr);
    else {
        const Solver::Options& o = *solve;
        stba_ba_create_options co;
        co.struct_size = sizeof co;
        co.linear_solver = STBA_LINEAR_ITERATIVE_SCHUR;
        rc = stba_ba_create_ex(&e->h, nc, np, no, x.cams.data(), x.pts.data(), L.obs_cam.data(), L.obs_pt.data(), L.feat.data(),
                               x.cam_fixed.data(), x.pt_fixed.data(), nullptr, &co);
        const int pc = o.preconditioner_type == IDENTITY ? STBA_PRECOND_IDENTITY : o.preconditioner_type == JACOBI ? STBA_PRECOND_JACOBI
                                                                                                                   : STBA_PRECOND_SCHUR_JACOBI;
        if (rc == STBA_OK) rc = stba_ba_set_pcg(e->h, pc, o.eta, o.min_linear_solver_iterations, o.max_linear_solver_iterations, 4);
    }
    if (rc == STBA_OK) return true;
    *error = std::string("stba_ba_create: ") + stba_last_error();
    e->Reset();
    return false;
}

// what ConfigureBa hands to an engine besides the layout's own tables
struct BaSetup {
    bool losses;                       // the layout's loss table (Covariance with apply_loss_function = false: not)
    BaHostCtx* host;                   // "gpu-ba-hostjac": the user's cost functions as the engine's lineariser; null: device factors
    const Solver::Options* solve;      // Solve: the trust-region strategy; null: Covariance
    const InnerGroups* inner;          // Solve with inner iterations; null: none
};
// The layout's sqrt_info, losses, relative poses, pose priors, landmark priors and the host lineariser to the engine, then Solve's
// trust region and inner iterations.  Returns the NAME of the first call that failed (its text: stba_last_error()), or null.  One order for Solve and
// Covariance: relative poses before priors, so that an engine that takes neither (ITERATIVE_SCHUR) names the relative poses.
inline const char* ConfigureBa(stba_ba* ba, const BaLayout& L, const BaSetup& s) {
    // (weighted ReprojectionFactors; with host Jacobians the factors whiten themselves)
    if (!s.host && !L.sqrt_info.empty() && stba_ba_set_sqrt_information(ba, L.sqrt_info.data()) != STBA_OK) return "stba_ba_set_sqrt_information";
    if (s.losses && !L.loss_kind.empty() && stba_ba_set_loss(ba, L.loss_kind.data(), L.loss_a.data(), L.loss_b.data(), L.loss_scale.data()) != STBA_OK)
        return "stba_ba_set_loss";
    // (PosePriorFactor / CameraRelativePoseFactor blocks: the engine refuses them on an ITERATIVE_SCHUR engine here -- before any solve,
    // the parameters untouched, the engine's reason in the message; DOGLEG and inner iterations are refused by DecideSolve)
    if (!L.rel_i.empty() && stba_ba_set_relative_poses(ba, (int)L.rel_i.size(), L.rel_i.data(), L.rel_j.data(), L.rel_meas.data(), nullptr,
                                                       L.rel_w.data()) != STBA_OK) return "stba_ba_set_relative_poses";
    if (!L.prior_cam.empty() && stba_ba_set_pose_priors(ba, (int)L.prior_cam.size(), L.prior_cam.data(), L.prior_pose.data(), nullptr,
                                                        L.prior_w.data()) != STBA_OK) return "stba_ba_set_pose_priors";
    // (LandmarkPriorFactor blocks: every engine that gets here takes them; inner iterations are refused by DecideSolve)
    if (!L.lp_pt.empty() && stba_ba_set_landmark_priors(ba, (int)L.lp_pt.size(), L.lp_pt.data(), L.lp_pos.data(), nullptr, L.lp_w.data()) != STBA_OK)
        return "stba_ba_set_landmark_priors";
    if (s.host && stba_ba_set_host_linearizer(ba, &BaHostLinearize, s.host) != STBA_OK) return "stba_ba_set_host_linearizer";
    if (s.solve && s.solve->trust_region_strategy_type == DOGLEG && stba_ba_set_trust_region(ba, STBA_TR_TRADITIONAL_DOGLEG) != STBA_OK)
        return "stba_ba_set_trust_region";
    if (s.inner && stba_ba_set_inner_iterations(ba, 1, s.solve->inner_iteration_tolerance, s.inner->rot.data(), s.inner->pos.data(),
                                                s.inner->pt.data()) != STBA_OK) return "stba_ba_set_inner_iterations";
    return nullptr;
}

// ---- one "gpu-ba" / "gpu-ba-hostjac" solve: named steps over one state -----------------------
struct BaRun {
    const Solver::Options& o;
    Problem* p;
    Recognition* rec;                  // its `ba` is the layout
    Solver::Summary* sum;
    bool host_jacobians = false;       // "gpu-ba-hostjac"
    const InnerGroups* inner = nullptr;   // null: no inner iterations
    bool blocks_failed = false;        // Create(): the per-block half of the recognition said no -- nothing was solved, the caller goes on
    BaPacked x;
    BaEngine engine;
    BaSync sync{nullptr, nullptr, nullptr, nullptr};
    BaHostCtx host{nullptr, nullptr, 1};
    std::thread destroyer;             // Destroy(): frees the engine next to the caller's end-point check; joined with this object
    double t0 = WallSeconds();

    BaRun(const Solver::Options& options, Problem* problem, Recognition* recognition, Solver::Summary* summary)
        : o(options), p(problem), rec(recognition), sum(summary) {}
    ~BaRun() { if (destroyer.joinable()) destroyer.join(); }
    const BaLayout& L() const { return rec->ba; }
    void Lap(double* acc) { const double t1 = WallSeconds(); *acc += t1 - t0; t0 = t1; }
    bool Fail(const std::string& message) { sum->termination_type = FAILURE; sum->message = message; return false; }

    void Pack() { PackBa(*p, L(), &x); Lap(&sum->phases.pack); }

    // With user blocks whose per-block check is still to come (Recognition::blocks < 0) that check runs HERE, on the calling thread,
    // while a helper thread creates the device engine (regrouping, Schur plan, uploads: ~50 ms at 10^6 observations, next to ~35 ms of
    // user Evaluate calls); the features it finds go to the engine afterwards (stba_ba_set_features).
    bool Create() {
        std::string error;
        bool ok = false;
        const bool check_blocks = L().n_user && rec->blocks < 0;
        int device = 0;
        if (check_blocks && !std::getenv("STBA_CERES_NO_OVERLAP") && stba_get_device(&device) == STBA_OK) {
            // (the helper thread creates the engine from the layout as it stands.  stba_ba_create READS L.feat while Blocks() writes the
            // user blocks' entries: a data race in the letter of the language, harmless in effect -- whatever the upload saw of those
            // entries is replaced by stba_ba_set_features below before anything is linearised.  Removing it needs a second n_obs-sized
            // array or another C ABI.  The thread starts on device 0 whatever this thread has selected, hence stba_set_device)
            std::thread helper([&]() {
                if (stba_set_device(device) != STBA_OK) error = std::string("stba_ba_create: ") + stba_last_error();
                else ok = CreateBa(L(), x, &o, &engine, &error);
            });
            JoinOnExit helper_guard{&helper};                           // (a user Evaluate that throws must not leave the thread running)
            const double tb0 = WallSeconds();
            const bool blocks_ok = rec->Blocks();
            const double t_blocks = WallSeconds() - tb0;
            helper.join();
            sum->phases.recognise += t_blocks;
            t0 += t_blocks;                                             // (what is left of the creation's wall time goes to engine_create)
            if (!blocks_ok) { engine.Reset(); Lap(&sum->phases.engine_create); blocks_failed = true; return false; }
            if (ok && stba_ba_set_features(engine.h, L().feat.data()) != STBA_OK) { ok = false; error = std::string("stba_ba_create: ") + stba_last_error(); }
        } else {
            if (check_blocks) {
                const bool blocks_ok = rec->Blocks();
                Lap(&sum->phases.recognise);
                if (!blocks_ok) { blocks_failed = true; return false; }
            }
            ok = CreateBa(L(), x, &o, &engine, &error);
        }
        Lap(&sum->phases.engine_create);
        return ok || Fail(error);
    }

    bool Configure() {
        host = BaHostCtx{p, &L(), o.num_threads};
        const BaSetup setup{true, host_jacobians ? &host : nullptr, &o, inner};
        const char* failed = ConfigureBa(engine.h, L(), setup);
        if (!failed) return true;
        // (the one message with a gloss of its own, kept as it always read)
        const bool rel = std::strcmp(failed, "stba_ba_set_relative_poses") == 0;
        return Fail(std::string(failed) + (rel ? " (relative pose factors): " : ": ") + stba_last_error());
    }

    bool Solve() {
        stba_lm_options co = ToC(o);
        if (inner) co.phase_timing = 1;          // (the sweeps' device time for Summary::inner_iteration_time_in_seconds)
        stba_lm_summary cs;
        std::vector<double> trace((size_t)(o.max_num_iterations + 1) * STBA_TRACE_COLS, 0.0);
        sync = BaSync{engine.h, p, &L(), &x};
        CallbackCtx ctx{&o, sum, &BaCopyOut, &sync};
        const int rc = stba_ba_solve(engine.h, &co, &cs, trace.data(), o.callbacks.empty() ? nullptr : &IterationTrampoline, &ctx);
        Lap(&sum->phases.device_solve);
        if (rc != STBA_OK) return Fail(std::string("stba_ba_solve: ") + stba_last_error());
        BaCopyOut(&sync);   // parameters are updated in place, like ceres::Solve
        FillSummary(cs, trace, sum);
        if (o.trust_region_strategy_type == DOGLEG) { sum->trust_region_strategy_type = DOGLEG; sum->dogleg_type = TRADITIONAL_DOGLEG; }
        stba_inner_summary is{};
        is.struct_size = sizeof is;
        if (inner && stba_ba_last_inner_summary(engine.h, &is) == STBA_OK) {
            sum->inner_iterations_used = true;
            sum->inner_iteration_ordering_used = inner->sizes_used;
            sum->num_inner_iteration_steps = is.sweeps;
            sum->inner_iteration_time_in_seconds = is.sweep_ms * 1e-3;
        }
        if (o.linear_solver_type == ITERATIVE_SCHUR) {
            sum->linear_solver_type_used = ITERATIVE_SCHUR;
            std::vector<int> its((size_t)cs.num_iterations, 0);
            if (cs.num_iterations > 0 && stba_ba_last_pcg_iterations(engine.h, its.data(), cs.num_iterations) == STBA_OK)
                for (int i = 1; i <= cs.num_iterations && i < (int)sum->iterations.size(); ++i) sum->iterations[(size_t)i].linear_solver_iterations = its[(size_t)i - 1];
        }
        if (ctx.user_abort) sum->termination_type = USER_FAILURE;
        if (ctx.user_success) sum->termination_type = USER_SUCCESS;
        return true;
    }

    // (the engine's ~40 device buffers take a few ms to free: where user blocks were taken over that happens on a helper thread, next
    // to the caller's end-point check of those blocks)
    void Destroy() {
        int dev_now = 0;
        if (L().n_user && !host_jacobians && stba_get_device(&dev_now) == STBA_OK) {
            BaEngine* e = &engine;
            destroyer = std::thread([e, dev_now]() { if (stba_set_device(dev_now) == STBA_OK) e->Reset(); });
        } else engine.Reset();
        Lap(&sum->phases.write_back);
    }

    // false: nothing was solved (the summary says why, or blocks_failed)
    bool Run() {
        Pack();
        if (!Create() || !Configure()) return false;
        const bool ok = Solve();
        Destroy();
        return ok;
    }
};

// ---- path 2: generic residual blocks through the host-callback dense path -------------------
struct DenseCtx {
    Problem* p;
    std::vector<int> var_blocks;         // non-constant block indices
    std::vector<int> amb_off, loc_off;   // per var block
    int n_amb = 0, n_loc = 0, n_res = 0;
    // scratch of DenseResidual, sized once per solve (it runs a dozen times per solve of a 40-residual problem whose published
    // wall time is 0.12 ms: no allocation per call, none per residual block)
    std::vector<const double*> cur, params;
    std::vector<int> var_index;
    std::vector<double*> jacs;
    std::vector<double> jac_store, plusJ;
    void Prepare() {
        auto& blocks = p->blocks();
        cur.resize(blocks.size()); var_index.assign(blocks.size(), -1);
        for (size_t v = 0; v < var_blocks.size(); ++v) var_index[var_blocks[v]] = (int)v;
        size_t max_nb = 0, max_jac = 0, max_plus = 0;
        for (auto& res : p->residuals()) {
            size_t need = 0;
            for (int k : res.blocks) { need += (size_t)res.cost->num_residuals() * blocks[k].size; max_plus = std::max(max_plus, (size_t)blocks[k].size * blocks[k].local_size()); }
            max_nb = std::max(max_nb, res.blocks.size()); max_jac = std::max(max_jac, need);
        }
        params.resize(max_nb); jacs.resize(max_nb); jac_store.resize(max_jac); plusJ.resize(max_plus);
    }
};

inline int DenseResidual(void* user, const double* x, double* r, double* J) {
    auto* c = static_cast<DenseCtx*>(user);
    auto& blocks = c->p->blocks();
    for (size_t k = 0; k < blocks.size(); ++k) c->cur[k] = blocks[k].ptr;
    for (size_t v = 0; v < c->var_blocks.size(); ++v) c->cur[c->var_blocks[v]] = x + c->amb_off[v];
    if (J) std::fill(J, J + (size_t)c->n_res * c->n_loc, 0.0);
    int row = 0;
    for (auto& res : c->p->residuals()) {
        const int nr = res.cost->num_residuals();
        const size_t nb = res.blocks.size();
        const double** params = c->params.data();
        double** jacs = c->jacs.data();
        size_t o = 0;
        for (size_t b = 0; b < nb; ++b) {
            params[b] = c->cur[res.blocks[b]];
            // constant blocks get no Jacobian request, like Ceres (NB solver.hpp:183: the reference's
            // PnPSizedCostFunction then skips ALL its Jacobians -- only hit when a block is constant)
            jacs[b] = (J && c->var_index[res.blocks[b]] >= 0) ? c->jac_store.data() + o : nullptr;
            o += (size_t)nr * blocks[res.blocks[b]].size;
        }
        if (J) std::fill(c->jac_store.begin(), c->jac_store.begin() + (long)o, 0.0);
        if (!res.cost->Evaluate(params, r + row, J ? jacs : nullptr)) return 1;
        if (J) {
            for (size_t b = 0; b < nb; ++b) {
                const int v = c->var_index[res.blocks[b]];
                if (v < 0 || !jacs[b]) continue;
                const auto& blk = blocks[res.blocks[b]];
                const int gs = blk.size, ls = blk.local_size();
                if (blk.local) {
                    double* plusJ = c->plusJ.data();
                    std::fill(plusJ, plusJ + (size_t)gs * ls, 0.0);
                    if (!blk.local->ComputeJacobian(params[b], plusJ)) return 1;
                    for (int rr = 0; rr < nr; ++rr)
                        for (int l = 0; l < ls; ++l) {
                            double s = 0;
                            for (int g = 0; g < gs; ++g) s += jacs[b][rr * gs + g] * plusJ[(size_t)g * ls + l];
                            J[(size_t)(row + rr) * c->n_loc + c->loc_off[v] + l] += s;
                        }
                } else {
                    for (int rr = 0; rr < nr; ++rr)
                        for (int g = 0; g < gs; ++g) J[(size_t)(row + rr) * c->n_loc + c->loc_off[v] + g] += jacs[b][rr * gs + g];
                }
            }
        }
        row += nr;
    }
    return 0;
}

inline void DensePlus(void* user, const double* x, const double* d, double* out) {
    auto* c = static_cast<DenseCtx*>(user);
    for (size_t v = 0; v < c->var_blocks.size(); ++v) {
        const auto& blk = c->p->blocks()[c->var_blocks[v]];
        if (blk.local) blk.local->Plus(x + c->amb_off[v], d + c->loc_off[v], out + c->amb_off[v]);
        else for (int k = 0; k < blk.size; ++k) out[c->amb_off[v] + k] = x[c->amb_off[v] + k] + d[c->loc_off[v] + k];
    }
}

struct DenseSync { DenseCtx* c; const double* x; };

// the variable blocks of the dense path (used by a residual block and not constant), their offsets, and the scratch of DenseResidual
inline void DenseLayout(Problem* p, DenseCtx& c, bool* any_bounds, bool* any_local) {
    c.p = p;
    std::vector<unsigned char> used(p->blocks().size(), 0);
    for (auto& r : p->residuals()) for (int k : r.blocks) used[(size_t)k] = 1;
    for (auto& b : p->blocks()) {
        if (!used[(size_t)b.index] || b.constant) continue;
        c.var_blocks.push_back(b.index); c.amb_off.push_back(c.n_amb); c.loc_off.push_back(c.n_loc);
        c.n_amb += b.size; c.n_loc += b.local_size();
        *any_bounds |= !b.lower.empty(); *any_local |= (b.local != nullptr);
    }
    c.n_res = p->NumResiduals();
    c.Prepare();
}

inline bool SolveDense(const Solver::Options& o, Problem* p, Solver::Summary* sum) {
    DenseCtx c;
    bool any_bounds = false, any_local = false;
    DenseLayout(p, c, &any_bounds, &any_local);
    if (c.n_loc == 0 || c.n_res == 0) { sum->termination_type = CONVERGENCE; sum->message = "nothing to optimise"; return true; }
    if (c.n_loc > 4096 || (double)c.n_loc * c.n_res > 2.7e8) { sum->termination_type = FAILURE; sum->message = "generic (callback) problems are limited to 4096 local parameters and 2.7e8 Jacobian entries; use ReprojectionFactor for large bundle adjustment"; return false; }
    std::vector<double> x(c.n_amb), lo, up;
    for (size_t v = 0; v < c.var_blocks.size(); ++v) std::memcpy(&x[c.amb_off[v]], p->blocks()[c.var_blocks[v]].ptr, sizeof(double) * p->blocks()[c.var_blocks[v]].size);
    if (any_bounds) {
        lo.assign(c.n_amb, -1e300); up.assign(c.n_amb, 1e300);
        for (size_t v = 0; v < c.var_blocks.size(); ++v) {
            const auto& b = p->blocks()[c.var_blocks[v]];
            if (!b.lower.empty()) for (int k = 0; k < b.size; ++k) { lo[c.amb_off[v] + k] = b.lower[k]; up[c.amb_off[v] + k] = b.upper[k]; }
        }
    }
    stba_lm_options co = ToC(o);
    stba_lm_summary cs;
    std::vector<double> trace((size_t)(o.max_num_iterations + 1) * STBA_TRACE_COLS, 0.0);
    struct Sync { DenseCtx* c; double* x; } sync{&c, x.data()};
    auto copy_out = [](void* u) {
        auto* s = static_cast<Sync*>(u);
        for (size_t v = 0; v < s->c->var_blocks.size(); ++v) {
            auto& b = s->c->p->blocks()[s->c->var_blocks[v]];
            std::memcpy(b.ptr, s->x + s->c->amb_off[v], sizeof(double) * b.size);
        }
    };
    CallbackCtx ctx{&o, sum, copy_out, &sync};
    const int rc = stba_dense_solve(&DenseResidual, any_local ? &DensePlus : nullptr, &c, c.n_amb, c.n_loc, c.n_res, x.data(),
                                    any_bounds ? lo.data() : nullptr, any_bounds ? up.data() : nullptr, &co, &cs, trace.data(),
                                    o.callbacks.empty() ? nullptr : &IterationTrampoline, &ctx);
    if (rc != STBA_OK) { sum->termination_type = FAILURE; sum->message = std::string("stba_dense_solve: ") + stba_last_error(); return false; }
    copy_out(&sync);
    FillSummary(cs, trace, sum);
    if (ctx.user_abort) sum->termination_type = USER_FAILURE;
    if (ctx.user_success) sum->termination_type = USER_SUCCESS;
    return true;
}

// ---- path 3: pose graph on the device engine (stba_pg_*) -------------------------------------
// owns an engine handle: the one place that destroys it
struct PgEngine {
    stba_pg* h = nullptr;
    PgEngine() = default;
    PgEngine(const PgEngine&) = delete;
    PgEngine& operator=(const PgEngine&) = delete;
    ~PgEngine() { if (h) stba_pg_destroy(h); }
};
// create, then the layout's sqrt_info and (losses: not for Covariance with apply_loss_function = false) loss table.  Returns the NAME
// of the first call that failed (its text: stba_last_error()), or null
inline const char* CreatePg(const PoseGraphLayout& L, bool losses, PgEngine* e) {
    if (stba_pg_create(&e->h, (int)L.node_block.size(), (int)L.ei.size(), L.poses.data(), L.ei.data(), L.ej.data(), L.meas.data(), L.fixed.data(),
                       nullptr) != STBA_OK) return "stba_pg_create";
    if (!L.sqrt_info.empty() && stba_pg_set_sqrt_information(e->h, L.sqrt_info.data()) != STBA_OK) return "stba_pg_set_sqrt_information";
    if (losses && !L.loss_kind.empty() && stba_pg_set_loss(e->h, L.loss_kind.data(), L.loss_a.data(), L.loss_b.data(), L.loss_scale.data()) != STBA_OK)
        return "stba_pg_set_loss";
    if (!L.prior_node.empty() && stba_pg_set_priors(e->h, (int)L.prior_node.size(), L.prior_node.data(), L.prior_pose.data(), nullptr, L.prior_w.data()) != STBA_OK)
        return "stba_pg_set_priors";
    return nullptr;
}
inline void SolvePoseGraph(const Solver::Options& o, Problem* p, PoseGraphLayout& L, Solver::Summary* sum) {
    const int n = (int)L.node_block.size();
    PgEngine pg;
    if (const char* failed = CreatePg(L, true, &pg)) { sum->termination_type = FAILURE; sum->message = std::string(failed) + ": " + stba_last_error(); return; }
    stba_lm_options co = ToC(o);
    stba_lm_summary cs;
    std::vector<double> trace((size_t)(o.max_num_iterations + 1) * STBA_TRACE_COLS, 0.0);
    int pcg_total = 0;
    int rc = stba_pg_solve(pg.h, &co, nullptr, &cs, trace.data(), &pcg_total);
    if (rc == STBA_OK) rc = stba_pg_get_poses(pg.h, L.poses.data());
    if (rc == STBA_OK) {
        for (int k = 0; k < n; ++k) std::memcpy(p->blocks()[L.node_block[k]].ptr, &L.poses[(size_t)k * 7], 7 * sizeof(double));
        FillSummary(cs, trace, sum);
    } else {
        sum->termination_type = FAILURE;
        sum->message = std::string("stba_pg_solve: ") + stba_last_error();
    }
}

// ---- the route decision ------------------------------------------------------------------------
// Where a recognised problem goes.  Solve: "gpu-ba", "gpu-ba-hostjac", "gpu-pg", "gpu-dense-callback"; Covariance: the same with
// "gpu-dense" for the last.
enum class Route { BA, BA_HOSTJAC, PG, DENSE };
// pg_allowed: Solve takes "gpu-pg" only without a forced callback path and without IterationCallbacks.  blocks_now: the per-block half
// of the device-factor reading is settled here (Covariance; Solve's inner iterations), not next to the engine's creation.
// Picking may RUN the recognition's lazy halves (Factor() -> Types(), and Blocks() with blocks_now): the user's Evaluate is called
// here the first time, and not again.
inline Route PickRoute(Recognition& r, bool pg_allowed, bool blocks_now) {
    if (r.Factor() && (!blocks_now || r.Blocks())) return Route::BA;
    if (pg_allowed && r.is_pg) return Route::PG;
    return r.Shape() ? Route::BA_HOSTJAC : Route::DENSE;
}

// Solve's decision: a route, or the first refusal in the order LossFunction, DOGLEG, inner iterations, preconditioner -- each before
// any device work, the parameters untouched.  `why` is the refusal's text (empty: go); each text stands here and nowhere else.
struct Decision {
    enum Stage { GO, LOSS, DOGLEG_STAGE, INNER, PRECONDITIONER } stage = GO;
    Route route = Route::DENSE;        // set with GO and with PRECONDITIONER (the route that would have run)
    std::string why;
    Decision& Refuse(Stage s, const std::string& text) { stage = s; why = text; return *this; }
};
// inner: with use_inner_iterations and no refusal, the ordering in the engine's terms.
// A function of (options, recognition) in its RESULT, not free of effects: the recognition is mutable because deciding is what first
// asks for Types() and Blocks(), which call the user's Evaluate and cache the answer.  The order of the short-circuits below is
// therefore what fixes how often Evaluate runs -- e.g. `r.Special() && r.Types()` probes only a problem that has prior / relative-pose
// blocks, and the preconditioner is refused without the per-block half -- and tests/test_*ceres_routes*.py hold the counts.
inline Decision DecideSolve(const Solver::Options& o, Recognition& r, InnerGroups* inner) {
    Decision d;
    Problem& p = *r.problem;
    const bool pg_allowed = !r.force_callback && o.callbacks.empty();
    const bool dogleg = o.trust_region_strategy_type == DOGLEG, iterative = o.linear_solver_type == ITERATIVE_SCHUR;
    // (Ceres would apply the loss; this layer has one to apply on "gpu-pg", and on "gpu-ba" where asked to -- a solve without it would
    // be a silently different problem)
    if (p.NumLossFunctions() > 0 && !r.ba_losses && !(pg_allowed && r.is_pg && r.pg.losses_known))
        return d.Refuse(Decision::LOSS, std::to_string(p.NumLossFunctions()) + " residual block(s) carry a LossFunction; robust losses are "
                                        "not implemented by this layer (the reference passes nullptr: test_ceres.h:120)");
    if (dogleg) {
        if (o.dogleg_type != TRADITIONAL_DOGLEG) return d.Refuse(Decision::DOGLEG_STAGE, "SUBSPACE_DOGLEG is not implemented by this layer (TRADITIONAL_DOGLEG is)");
        if (iterative) return d.Refuse(Decision::DOGLEG_STAGE, "DOGLEG only supports exact factorization based linear solvers, not ITERATIVE_SCHUR");
        // (LandmarkPriorFactor blocks go with DOGLEG on "gpu-ba": the engine's three J sums carry their rows)
        if (!r.ShapeRaw() && !(r.structure && !r.CameraSpecial() && r.Factor())) {
            const bool special = r.structure && r.Types();
            return d.Refuse(Decision::DOGLEG_STAGE,
                special && !r.ba.rel_i.empty() ? "DOGLEG with CameraRelativePoseFactor (relative pose) blocks is not implemented (the dogleg's |J g|^2 is summed from the observation records)"
                : special && !r.ba.prior_cam.empty() ? "DOGLEG with PosePriorFactor blocks is not implemented (the dogleg's |J g|^2 is summed from the observation records)"
                : "DOGLEG is implemented for bundle adjustment (gpu-ba, gpu-ba-hostjac) only, not for problems that take gpu-pg or gpu-dense-callback");
        }
    }
    if (o.use_inner_iterations) {
        std::string why;
        if (dogleg) why = "inner iterations are not implemented with DOGLEG";
        else if (!(o.inner_iteration_tolerance >= 0.0)) why = "inner_iteration_tolerance must be >= 0";
        else if (!r.Shape() && r.structure && r.Special() && r.Types())
            why = !r.ba.rel_i.empty() ? "inner iterations with CameraRelativePoseFactor (relative pose) blocks are not implemented"
                  : !r.ba.prior_cam.empty() ? "inner iterations with PosePriorFactor blocks are not implemented"
                                            : "inner iterations with LandmarkPriorFactor blocks are not implemented (the per-landmark sweep solves from the observation records)";
        else if (!r.Shape())
            why = "inner iterations are implemented for bundle adjustment on the gpu-ba path only, not for problems that take gpu-pg or gpu-dense-callback";
        else if (r.force_callback) why = "inner iterations are implemented on the gpu-ba path only, not on gpu-ba-hostjac (force_callback_path)";
        else if (!MakeInnerGroups(o, p, r.ba, inner, &why)) {}
        // (gpu-ba only: every block must be the reprojection factor -- the per-block half of the recognition runs here, before any
        // device work, instead of next to the engine's creation)
        else if (PickRoute(r, false, true) != Route::BA)
            why = "inner iterations are implemented on the gpu-ba path only: this problem's cost functions are not the reprojection factor "
                  "(gpu-ba-hostjac)";
        else if (!r.ba.sqrt_info.empty()) why = "inner iterations with weighted ReprojectionFactors (sqrt_information) are not implemented";
        if (!why.empty()) return d.Refuse(Decision::INNER, why);
    }
    d.route = PickRoute(r, pg_allowed, false);
    const bool ba_engine = d.route == Route::BA || d.route == Route::BA_HOSTJAC;
    if (ba_engine && iterative && o.preconditioner_type != IDENTITY && o.preconditioner_type != JACOBI && o.preconditioner_type != SCHUR_JACOBI)
        return d.Refuse(Decision::PRECONDITIONER, "ITERATIVE_SCHUR with the CLUSTER_JACOBI, CLUSTER_TRIDIAGONAL or SUBSET preconditioner is not implemented by "
                                                  "this layer (IDENTITY, JACOBI and SCHUR_JACOBI are)");
    return d;
}

// refused before any device work: FAILURE, the reason in the message and on stderr
inline void Refuse(Solver::Summary* summary, const std::string& why) {
    summary->termination_type = FAILURE;
    summary->message = "stba_ceres: " + why + " -- nothing was solved.";
    std::fprintf(stderr, "%s\n", summary->message.c_str());
}
inline const char* RouteName(Route route) {
    return route == Route::BA ? "gpu-ba" : route == Route::BA_HOSTJAC ? "gpu-ba-hostjac" : route == Route::PG ? "gpu-pg" : "gpu-dense-callback";
}
inline void NoteRecognisedBlocks(size_t n_user, Solver::Summary* summary) {
    if (n_user) summary->message += (summary->message.empty() ? "" : " ") + std::to_string(n_user) +
                                    " user cost functions recognised as the reprojection factor (probe points, start point, end point) and evaluated by the device kernel.";
}

inline void SolveDispatch(const Solver::Options& options, Problem* problem, Solver::Summary* summary) {
    double t0 = WallSeconds();
    Recognition r;
    Recognise(*problem, ForceCallbackPath(options.force_callback_path), options.bundle_adjustment_losses && !options.use_inner_iterations,
              options.num_threads, &r);
    InnerGroups inner;
    Decision d = DecideSolve(options, r, &inner);
    summary->phases.recognise = WallSeconds() - t0;
    if (d.stage != Decision::LOSS && d.stage != Decision::DOGLEG_STAGE) {
        summary->inner_iterations_given = options.use_inner_iterations;
        if (options.use_inner_iterations && options.inner_iteration_ordering)
            for (const auto& g : options.inner_iteration_ordering->group_to_elements()) summary->inner_iteration_ordering_given.push_back((int)g.second.size());
    }
    // (a preconditioner is refused by the BA route it would have run on: the summary names that route, and the blocks taken over)
    auto refused = [&](const Decision& dd) {
        if (dd.stage == Decision::GO) return false;
        if (dd.stage == Decision::PRECONDITIONER) summary->execution_path = RouteName(dd.route);
        Refuse(summary, dd.why);
        if (dd.stage == Decision::PRECONDITIONER && dd.route == Route::BA) NoteRecognisedBlocks(r.ba.n_user, summary);
        return true;
    };
    if (refused(d)) return;
    std::string carried;
    if (d.route == Route::BA) {
        std::vector<double> saved;
        if (r.ba.n_user) for (auto& b : problem->blocks()) saved.insert(saved.end(), b.ptr, b.ptr + b.size);
        summary->execution_path = RouteName(Route::BA);
        BaRun run(options, problem, &r, summary);
        if (options.use_inner_iterations) run.inner = &inner;
        run.Run();
        if (run.blocks_failed) {
            // a block is not the factor: on to the other routes, nothing was touched
            summary->execution_path.clear();
            d = DecideSolve(options, r, &inner);
        } else {
            t0 = WallSeconds();
            const bool still_factor = summary->termination_type == FAILURE || VerifyRecognisedBlocks(*problem, r.ba, options.num_threads);
            if (run.destroyer.joinable()) run.destroyer.join();
            summary->phases.verify = WallSeconds() - t0;
            if (still_factor) { NoteRecognisedBlocks(r.ba.n_user, summary); return; }
            size_t at = 0;
            for (auto& b : problem->blocks()) { std::copy(saved.begin() + at, saved.begin() + at + b.size, b.ptr); at += (size_t)b.size; }
            if (r.ba_losses) {
                // (the second solve would take gpu-ba-hostjac, which has no losses: refused, the parameters as they were)
                *summary = Solver::Summary();
                Refuse(summary, "a user cost function taken for the reprojection factor differs from it at the solution, and robust losses are "
                                "not implemented on the gpu-ba-hostjac path (LossFunction)");
                return;
            }
            const Solver::Summary::Phases first = summary->phases;
            const std::vector<int> given = summary->inner_iteration_ordering_given;
            *summary = Solver::Summary();
            summary->phases = first;
            carried = "a user cost function taken for the reprojection factor differs from it at the solution: solved again with the user's Evaluate.";
            if (options.use_inner_iterations) {
                // (the second solve takes gpu-ba-hostjac, which has no inner iterations: it runs without them)
                summary->inner_iterations_given = true;
                summary->inner_iteration_ordering_given = given;
                carried += " The second solve ran without inner iterations (gpu-ba-hostjac has none).";
            }
            // the one re-reading: the recognition as it stands, with the device-factor reading struck out
            r.dropped = true;
            Solver::Options again = options;
            again.use_inner_iterations = false;
            d = DecideSolve(again, r, &inner);
        }
        if (refused(d)) return;
    }
    const double t_resolve = WallSeconds();
    summary->execution_path = RouteName(d.route);
    if (d.route == Route::PG) {
        // a pose graph: every residual block a RelativePoseFactor between two 7-double pose blocks with the SE3 right-plus chart, or a
        // NodePosePriorFactor on one
        SolvePoseGraph(options, problem, r.pg, summary);
    } else if (d.route == Route::BA_HOSTJAC) {
        // BA-SHAPED, but not (or not to be taken for) the built-in factor: every residual block is {quaternion 4, position 3,
        // landmark 3} -> 2 with the quaternion right-plus chart.  The user's cost functions are evaluated on the host, in bulk, into
        // the device engine's residual / Jacobian buffers, and the Schur complement, the factorisation, the back-substitution and the
        // LM loop run on the device as for the built-in factor: any size the engine takes, where the dense callback path stops at
        // 4096 local parameters.  (The reference's BA cost IS a generic functor: test_ceres.h:56.)
        r.MakeShapeOnly();
        const Solver::Summary::Phases ph = summary->phases;
        BaRun run(options, problem, &r, summary);
        run.host_jacobians = true;
        run.Run();
        if (!carried.empty()) { summary->phases = ph; summary->phases.resolve = WallSeconds() - t_resolve; }
    } else SolveDense(options, problem, summary);
    if (!carried.empty()) summary->message = carried + (summary->message.empty() ? "" : " ") + summary->message;
}

// ---- the recognition under the names the C++ tests drive it by (tests/cpp/*_shim.cpp); nothing in this header calls these -----
// probe = false: the shape-only reading, L->feat left at zero
inline bool DetectBa(Problem& p, BaLayout* L, bool probe = true, int threads = 1) {
    Recognition r;
    Recognise(p, false, false, threads, &r);
    const bool ok = probe ? r.structure && r.Types() && r.Blocks() : r.ShapeRaw();
    if (!probe) r.MakeShapeOnly();
    *L = std::move(r.ba);
    return ok;
}
inline bool BaWithKnownLosses(Problem* problem, int threads, BaLayout* L) {
    Recognition r;
    Recognise(*problem, false, true, threads, &r);
    const bool ok = problem->NumLossFunctions() > 0 ? r.ba_losses : r.Factor() && r.Blocks();
    *L = std::move(r.ba);
    return ok;
}
inline bool LossesGoToPoseGraph(const Solver::Options& options, Problem* problem) {
    Recognition r;
    Recognise(*problem, ForceCallbackPath(options.force_callback_path), false, options.num_threads, &r);
    return !r.force_callback && options.callbacks.empty() && r.is_pg && r.pg.losses_known;
}
inline bool LossesGoToBa(const Solver::Options& options, Problem* problem) {
    BaLayout L;
    return options.bundle_adjustment_losses && !options.use_inner_iterations && !ForceCallbackPath(options.force_callback_path) &&
           BaWithKnownLosses(problem, options.num_threads, &L);
}
}  // namespace internal

inline void Solve(const Solver::Options& options, Problem* problem, Solver::Summary* summary) {
    *summary = Solver::Summary();
    const double t0 = internal::WallSeconds();
    internal::SolveDispatch(options, problem, summary);
    // Ceres' timing fields: total = everything inside Solve(); minimizer = the engine's own solve time (set by FillSummary)
    summary->total_time_in_seconds = internal::WallSeconds() - t0;
    const auto& ph = summary->phases;
    summary->preprocessor_time_in_seconds = ph.recognise + ph.pack + ph.engine_create;
    summary->postprocessor_time_in_seconds = ph.write_back + ph.verify;
}

// ------------------------------------------------------------------------------------------
// Covariance (the Ceres <= 2.1 surface): C = (J^T J)^-1 of the undamped problem at the parameter values the blocks hold when
// Compute is called, not multiplied by a residual variance.  It is computed on the device and nowhere else:
//   * "gpu-ba": every residual block is the reprojection factor (built-in, or a user cost function recognised as it at the current
//     point, as Solve recognises it) -> stba_ba_covariance_compute with device Jacobians;
//   * "gpu-ba-hostjac": BA-shaped with another factor -> the same with the user's cost functions as the host lineariser;
//   * "gpu-pg": a pose graph as Solve recognises it (every residual block a RelativePoseFactor on two SE3RightPlus blocks, or a
//     NodePosePriorFactor on one: a block with such a prior anchors its connected component like a constant block) ->
//     stba_pg_covariance, a batched conjugate gradient on the device engine's matrix-free J^T J: any size the engine takes.  A
//     requested pair is any two pose blocks of the graph; a connected component without a constant block makes J^T J singular and
//     Compute return false (the message names the component), before any device work;
//   * "gpu-dense": anything else within the dense solve's limits -> stba_dense_covariance.
// On the BA routes a requested pair is two camera blocks (rotation / position, of one camera or of two) or one landmark with
// itself; with Options::bundle_adjustment_cross_blocks = true (an extension of this layer, off by default: tests/cpp/test_covariance.cpp
// pins the refusal) it is any two of the rotation blocks, position blocks and landmarks, as in Ceres: also camera-landmark blocks
// (either way round) and the blocks of two different landmarks (stba_ba_camera_point_covariance, stba_ba_point_pair_covariance).
// Without the option those pairs are refused before any device work.  Constant blocks give zero blocks.  Limits: robust losses on "gpu-pg", and on "gpu-ba"
// with Options::bundle_adjustment_losses set, where the result is (J'^T J')^-1 of the corrected Jacobian as in Ceres (refused elsewhere as Solve refuses them), no pseudo-inverse (null_space_rank must be 0), and the rank test is the pivot ratio of the Cholesky
// factorisations (stba.h, stba_ba_covariance_compute) -- not a condition number estimate.  algorithm_type and num_threads are
// accepted for source compatibility and do not change the computation.
// (not in Ceres) execution_path() and message(): which route ran, and why Compute returned false.
enum CovarianceAlgorithmType { DENSE_SVD, SPARSE_QR, SUITE_SPARSE_QR, EIGEN_SPARSE_QR };

class Covariance {
public:
    struct Options {
        CovarianceAlgorithmType algorithm_type = SPARSE_QR;
        double min_reciprocal_condition_number = 1e-14;
        int null_space_rank = 0;
        int num_threads = 1;
        bool apply_loss_function = true;
        bool bundle_adjustment_losses = false;   // (not in Ceres) as Solver::Options::bundle_adjustment_losses: built-in losses on "gpu-ba"
        bool bundle_adjustment_cross_blocks = false;   // (not in Ceres) camera-landmark pairs and pairs of different landmarks on the BA routes (off: refused, the default this layer has had)
    };
    explicit Covariance(const Options& options) : options_(options) {}

    bool Compute(const std::vector<std::pair<const double*, const double*>>& covariance_blocks, Problem* problem) {
        blocks_.clear(); tangent_.clear(); path_.clear(); message_.clear();
        const bool ok = ComputeImpl(covariance_blocks, problem);
        if (!ok) std::fprintf(stderr, "stba_ceres::Covariance: %s\n", message_.c_str());
        return ok;
    }
    // Ja C Jb^T in the ambient space of the two blocks (J: LocalParameterization::ComputeJacobian at Compute's point; the identity
    // for a block without one), row-major size(a) x size(b)
    bool GetCovarianceBlock(const double* a, const double* b, double* cov) const {
        const auto ia = blocks_.find(a), ib = blocks_.find(b);
        const auto it = tangent_.find({a, b});
        if (ia == blocks_.end() || ib == blocks_.end() || it == tangent_.end()) return false;
        const Info &A = ia->second, &B = ib->second;
        std::vector<double> t((size_t)A.size * B.local, 0.0);            // Ja C
        for (int r = 0; r < A.size; ++r)
            for (int c = 0; c < B.local; ++c) {
                double s = 0.0;
                for (int k = 0; k < A.local; ++k) s += A.jac[(size_t)r * A.local + k] * it->second[(size_t)k * B.local + c];
                t[(size_t)r * B.local + c] = s;
            }
        for (int r = 0; r < A.size; ++r)
            for (int c = 0; c < B.size; ++c) {
                double s = 0.0;
                for (int k = 0; k < B.local; ++k) s += t[(size_t)r * B.local + k] * B.jac[(size_t)c * B.local + k];
                cov[(size_t)r * B.size + c] = s;
            }
        return true;
    }
    // C itself, row-major local(a) x local(b)
    bool GetCovarianceBlockInTangentSpace(const double* a, const double* b, double* cov) const {
        const auto it = tangent_.find({a, b});
        if (it == tangent_.end()) return false;
        std::copy(it->second.begin(), it->second.end(), cov);
        return true;
    }
    const std::string& execution_path() const { return path_; }      // "gpu-ba" | "gpu-ba-hostjac" | "gpu-pg" | "gpu-dense" (empty: none ran)
    const std::string& message() const { return message_; }

private:
    struct Info { int size = 0, local = 0; std::vector<double> jac; };   // jac: size x local
    Options options_;
    std::map<const double*, Info> blocks_;
    std::map<std::pair<const double*, const double*>, std::vector<double>> tangent_;
    std::string path_, message_;

    bool Fail(const std::string& m) { message_ = m; blocks_.clear(); tangent_.clear(); return false; }
    static std::string PairName(size_t k) { return "pair " + std::to_string(k); }
    // both orders of a computed pair; the block of (b, a) is the transpose
    void Store(const double* a, const double* b, int la, int lb, std::vector<double> t) {
        std::vector<double> tt((size_t)la * lb);
        for (int r = 0; r < la; ++r) for (int c = 0; c < lb; ++c) tt[(size_t)c * la + r] = t[(size_t)r * lb + c];
        tangent_[{a, b}] = std::move(t);
        tangent_[{b, a}] = std::move(tt);
    }

    using Pairs = std::vector<std::pair<const double*, const double*>>;
    using BlockIndex = std::unordered_map<const double*, int>;

    // the refusals that do not depend on the request, in their order: LossFunction, null_space_rank.  Empty: go
    std::string Refusal(Problem& p, const internal::Recognition& r) const {
        if (p.NumLossFunctions() > 0 && !r.ba_losses && !(r.is_pg && r.pg.losses_known))
            return std::to_string(p.NumLossFunctions()) + " residual block(s) carry a LossFunction; robust losses are not implemented by this layer -- no covariance computed";
        if (options_.null_space_rank != 0)
            return "null_space_rank = " + std::to_string(options_.null_space_rank) + ": this layer has no pseudo-inverse (only 0 is supported)";
        return std::string();
    }

    bool ComputeImpl(const Pairs& pairs, Problem* p) {
        using namespace internal;
        Recognition r;
        Recognise(*p, false, options_.bundle_adjustment_losses, options_.num_threads, &r);
        const std::string refusal = Refusal(*p, r);
        if (!refusal.empty()) return Fail(refusal);
        BlockIndex index;
        for (auto& b : p->blocks()) index[b.ptr] = b.index;
        for (size_t k = 0; k < pairs.size(); ++k)
            if (!index.count(pairs[k].first) || !index.count(pairs[k].second)) return Fail(PairName(k) + " names a parameter block that is not in the problem");
        for (auto& b : p->blocks()) {
            Info in;
            in.size = b.size; in.local = b.local_size();
            in.jac.assign((size_t)in.size * in.local, 0.0);
            if (b.local) { if (!b.local->ComputeJacobian(b.ptr, in.jac.data())) return Fail("LocalParameterization::ComputeJacobian failed"); }
            else for (int k = 0; k < in.size; ++k) in.jac[(size_t)k * in.local + k] = 1.0;
            blocks_[b.ptr] = std::move(in);
        }
        switch (PickRoute(r, true, true)) {
        case Route::BA: return ComputeBa(pairs, p, r.ba, index, false);
        case Route::BA_HOSTJAC: r.MakeShapeOnly(); return ComputeBa(pairs, p, r.ba, index, true);
        case Route::PG: return ComputePoseGraph(pairs, r.pg, index);
        default: return ComputeDense(pairs, p, index);
        }
    }

    bool ComputePoseGraph(const Pairs& pairs, const internal::PoseGraphLayout& G, const BlockIndex& index) {
        const int n = (int)G.node_block.size(), m = (int)G.ei.size();
        std::vector<int> na, nb;
        for (size_t k = 0; k < pairs.size(); ++k) {
            const auto a = G.node_of.find(index.at(pairs[k].first)), b = G.node_of.find(index.at(pairs[k].second));
            if (a == G.node_of.end() || b == G.node_of.end()) return Fail(PairName(k) + " names a parameter block that no residual block of the pose graph uses");
            na.push_back(a->second); nb.push_back(b->second);
        }
        path_ = "gpu-pg";
        if (pairs.empty()) return true;
        // (the gauge check of stba_pg_covariance, here so that a graph it refuses never needs a device)
        // (with NodePosePriorFactor blocks a node with a prior anchors its component too: the engine's own check knows them)
        if (G.prior_node.empty() && stba_pg_gauge_check(n, m, G.ei.data(), G.ej.data(), G.fixed.data()) != STBA_OK)
            return Fail(std::string("stba_pg_covariance: ") + stba_last_error());
        internal::PgEngine pg;
        // (apply_loss_function = false: (J^T J)^-1 of the uncorrected Jacobian, as in Ceres)
        if (const char* failed = internal::CreatePg(G, options_.apply_loss_function, &pg)) return Fail(std::string(failed) + ": " + stba_last_error());
        std::vector<double> blk(pairs.size() * 36);
        if (stba_pg_covariance(pg.h, (int)pairs.size(), na.data(), nb.data(), nullptr, blk.data(), nullptr) != STBA_OK)
            return Fail(std::string("stba_pg_covariance: ") + stba_last_error());
        for (size_t k = 0; k < pairs.size(); ++k)
            Store(pairs[k].first, pairs[k].second, 6, 6, std::vector<double>(blk.begin() + (ptrdiff_t)k * 36, blk.begin() + (ptrdiff_t)(k + 1) * 36));
        // (the columns of C come from separate conjugate-gradient solves, so C[a, b] and C[b, a]^T differ in their last bits: Store's
        // transpose serves the swapped pair nobody asked for, and every REQUESTED pair -- a diagonal one, or both orders of one --
        // keeps the block that was computed for it)
        for (size_t k = 0; k < pairs.size(); ++k)
            tangent_[{pairs[k].first, pairs[k].second}].assign(blk.begin() + (ptrdiff_t)k * 36, blk.begin() + (ptrdiff_t)(k + 1) * 36);
        return true;
    }

    bool ComputeBa(const Pairs& pairs, Problem* p, const internal::BaLayout& L, const BlockIndex& index, bool host) {
        using namespace internal;
        const int nc = (int)L.rot_block.size(), np = (int)L.pt_block.size();
        auto& blk = p->blocks();
        // block index -> (camera, 0 | 3) or landmark
        std::vector<int> cam_of(blk.size(), -1), off_of(blk.size(), 0), pt_of(blk.size(), -1);
        for (int c = 0; c < nc; ++c) { cam_of[L.rot_block[c]] = c; cam_of[L.pos_block[c]] = c; off_of[L.pos_block[c]] = 3; }
        for (int j = 0; j < np; ++j) pt_of[L.pt_block[j]] = j;
        // four kinds of pair, one C-ABI call each: camera-camera, a landmark's marginal, camera-landmark (a (landmark, camera) pair
        // is asked for as (camera, landmark) and transposed), landmark-landmark
        std::vector<int> ca, cb, pj, xc, xp, la, lb;
        for (size_t k = 0; k < pairs.size(); ++k) {
            const int a = index.at(pairs[k].first), b = index.at(pairs[k].second);
            if (cam_of[a] >= 0 && cam_of[b] >= 0) { ca.push_back(cam_of[a]); cb.push_back(cam_of[b]); }
            else if (pt_of[a] >= 0 && a == b) pj.push_back(pt_of[a]);
            else if (!options_.bundle_adjustment_cross_blocks)
                return Fail(PairName(k) + " is neither two camera blocks nor one landmark with itself: camera-landmark and landmark-landmark "
                            "blocks of the bundle-adjustment route need Covariance::Options::bundle_adjustment_cross_blocks = true");
            else if (cam_of[a] >= 0 && pt_of[b] >= 0) { xc.push_back(cam_of[a]); xp.push_back(pt_of[b]); }
            else if (pt_of[a] >= 0 && cam_of[b] >= 0) { xc.push_back(cam_of[b]); xp.push_back(pt_of[a]); }
            else if (pt_of[a] >= 0 && pt_of[b] >= 0) { la.push_back(pt_of[a]); lb.push_back(pt_of[b]); }
            else return Fail(PairName(k) + " names a parameter block that no residual block of the bundle adjustment uses");
        }
        path_ = host ? "gpu-ba-hostjac" : "gpu-ba";
        BaPacked x;
        PackBa(*p, L, &x);
        BaEngine engine;
        std::string error;
        if (!CreateBa(L, x, nullptr, &engine, &error)) return Fail(error);
        stba_ba* ba = engine.h;
        BaHostCtx hctx{p, &L, options_.num_threads};
        // (apply_loss_function = false: (J^T J)^-1 of the uncorrected Jacobian, as in Ceres)
        const BaSetup setup{options_.apply_loss_function, host ? &hctx : nullptr, nullptr, nullptr};
        if (const char* failed = ConfigureBa(ba, L, setup)) return Fail(std::string(failed) + ": " + stba_last_error());
        double rc = 0.0;
        if (stba_ba_covariance_compute(ba, options_.min_reciprocal_condition_number, &rc) != STBA_OK)
            return Fail(std::string("stba_ba_covariance_compute: ") + stba_last_error());
        std::vector<double> cblk(ca.size() * 36), pblk(pj.size() * 9), xblk(xc.size() * 18), lblk(la.size() * 9);
        if (stba_ba_camera_covariance(ba, (int)ca.size(), ca.data(), cb.data(), cblk.data()) != STBA_OK ||
            stba_ba_point_covariance(ba, (int)pj.size(), pj.data(), pblk.data()) != STBA_OK ||
            stba_ba_camera_point_covariance(ba, (int)xc.size(), xc.data(), xp.data(), xblk.data()) != STBA_OK ||
            stba_ba_point_pair_covariance(ba, (int)la.size(), la.data(), lb.data(), lblk.data()) != STBA_OK)
            return Fail(std::string("covariance blocks: ") + stba_last_error());
        size_t kc = 0, kp = 0, kx = 0, kl = 0;
        for (auto& pr : pairs) {
            const int a = index.at(pr.first), b = index.at(pr.second);
            std::vector<double> t(9);
            if (cam_of[a] >= 0 && cam_of[b] >= 0) {
                const double* s6 = &cblk[kc++ * 36];
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) t[(size_t)r * 3 + c] = s6[(size_t)(off_of[a] + r) * 6 + off_of[b] + c];
            } else if (pt_of[a] >= 0 && a == b) { const double* s3 = &pblk[kp++ * 9]; t.assign(s3, s3 + 9); }
            else if (cam_of[a] >= 0) {              // (rotation | position, landmark): rows off .. off + 3 of the 6 x 3 block
                const double* s = &xblk[kx++ * 18] + (size_t)off_of[a] * 3;
                t.assign(s, s + 9);
            } else if (cam_of[b] >= 0) {            // (landmark, rotation | position): the transpose
                const double* s = &xblk[kx++ * 18] + (size_t)off_of[b] * 3;
                for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) t[(size_t)r * 3 + c] = s[(size_t)c * 3 + r];
            } else { const double* s3 = &lblk[kl++ * 9]; t.assign(s3, s3 + 9); }
            Store(pr.first, pr.second, 3, 3, std::move(t));
        }
        return true;
    }

    bool ComputeDense(const std::vector<std::pair<const double*, const double*>>& pairs, Problem* p,
                      const std::unordered_map<const double*, int>& index) {
        using namespace internal;
        DenseCtx c;
        bool any_bounds = false, any_local = false;
        DenseLayout(p, c, &any_bounds, &any_local);
        if (c.n_loc == 0 || c.n_res == 0) return Fail("nothing to compute: no variable parameter block or no residual");
        if (c.n_loc > 4096 || (double)c.n_loc * c.n_res > 2.7e8)
            return Fail("generic (callback) problems are limited to 4096 local parameters and 2.7e8 Jacobian entries");
        path_ = "gpu-dense";
        std::vector<double> x(c.n_amb), cov((size_t)c.n_loc * c.n_loc);
        for (size_t v = 0; v < c.var_blocks.size(); ++v) std::memcpy(&x[c.amb_off[v]], p->blocks()[c.var_blocks[v]].ptr, sizeof(double) * p->blocks()[c.var_blocks[v]].size);
        double rc = 0.0;
        if (stba_dense_covariance(&DenseResidual, &c, c.n_amb, c.n_loc, c.n_res, x.data(), options_.min_reciprocal_condition_number, cov.data(), &rc) != STBA_OK)
            return Fail(std::string("stba_dense_covariance: ") + stba_last_error());
        std::vector<int> var_of(p->blocks().size(), -1);
        for (size_t v = 0; v < c.var_blocks.size(); ++v) var_of[c.var_blocks[v]] = (int)v;
        for (auto& pr : pairs) {
            const int a = index.at(pr.first), b = index.at(pr.second);
            const int la = p->blocks()[a].local_size(), lb = p->blocks()[b].local_size();
            std::vector<double> t((size_t)la * lb, 0.0);
            if (var_of[a] >= 0 && var_of[b] >= 0)
                for (int r = 0; r < la; ++r)
                    for (int q = 0; q < lb; ++q) t[(size_t)r * lb + q] = cov[(size_t)(c.loc_off[var_of[a]] + r) * c.n_loc + c.loc_off[var_of[b]] + q];
            Store(pr.first, pr.second, la, lb, std::move(t));
        }
        return true;
    }
};

}  // namespace stba_ceres
#endif
