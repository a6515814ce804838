// slam-tricks_amd/csrc/inner_policy.hpp (the LM of one block of an inner-iteration sweep) compiled with a plain C++ compiler, for
// tests/test_inner_iterations_cpu.py, which runs inner_iterations_ref.block_lm on the same cases.  One case per input line:
//   family max_num_iterations function_tolerance gradient_tolerance parameter_tolerance initial_radius min_radius x0 x1
// families: 0 r = x - (1, 2); 1 Rosenbrock r = (10 (x1 - x0^2), 1 - x0); 2 r_i = x1 exp(x0 t_i) - y_i, t_i = i / 4, i < 5;
// 3 a constant, indefinite "H" = [[1, 100], [100, 1]] with g = (1, 0) (no least-squares problem has it: every step fails to factor).
// Output per case: iterations stop x0 x1.
#include <cmath>
#include <cstdio>

#include "../../slam-tricks_amd/csrc/inner_policy.hpp"

static const double kY[5] = {2.0, 2.2663, 2.5681, 2.9099, 3.2974};

// residuals and the 2-column Jacobian of a family at x (m rows); returns m
static int Residuals(int fam, const double* x, double* r, double* J) {
    if (fam == 0) { r[0] = x[0] - 1.0; r[1] = x[1] - 2.0; J[0] = 1; J[1] = 0; J[2] = 0; J[3] = 1; return 2; }
    if (fam == 1) { r[0] = 10.0 * (x[1] - x[0] * x[0]); r[1] = 1.0 - x[0]; J[0] = -20.0 * x[0]; J[1] = 10.0; J[2] = -1.0; J[3] = 0.0; return 2; }
    for (int i = 0; i < 5; ++i) {
        const double t = 0.25 * i, e = std::exp(x[0] * t);
        r[i] = x[1] * e - kY[i];
        J[2 * i] = x[1] * t * e; J[2 * i + 1] = e;
    }
    return 5;
}

int main() {
    int fam, max_it;
    double ftol, gtol, ptol, r0, rmin, x[2];
    while (std::scanf("%d %d %lf %lf %lf %lf %lf %lf %lf", &fam, &max_it, &ftol, &gtol, &ptol, &r0, &rmin, &x[0], &x[1]) == 9) {
        stba::inner::BlockOptions o;
        o.max_num_iterations = max_it; o.function_tolerance = ftol; o.gradient_tolerance = gtol; o.parameter_tolerance = ptol;
        o.initial_trust_region_radius = r0; o.min_trust_region_radius = rmin;
        auto cost_at = [fam](const double* X) {
            if (fam == 3) return 1.0;
            double r[5], J[10];
            const int m = Residuals(fam, X, r, J);
            double c = 0.0;
            for (int i = 0; i < m; ++i) c += r[i] * r[i];
            return 0.5 * c;
        };
        auto lin = [fam, cost_at](const double* X, double* H, double* g) {
            if (fam == 3) { H[0] = 1; H[1] = 100; H[2] = 100; H[3] = 1; g[0] = 1; g[1] = 0; return 1.0; }
            double r[5], J[10];
            const int m = Residuals(fam, X, r, J);
            for (int a = 0; a < 2; ++a) {
                g[a] = 0.0;
                for (int b = 0; b < 2; ++b) H[a * 2 + b] = 0.0;
                for (int i = 0; i < m; ++i) {
                    g[a] += J[2 * i + a] * r[i];
                    for (int b = 0; b < 2; ++b) H[a * 2 + b] += J[2 * i + a] * J[2 * i + b];
                }
            }
            return cost_at(X);
        };
        auto plus = [](const double* X, const double* d, double* Xn) { Xn[0] = X[0] + d[0]; Xn[1] = X[1] + d[1]; };
        auto norm2 = [](const double* X) { return X[0] * X[0] + X[1] * X[1]; };
        auto dist2 = [](const double* X, const double* Xn) { const double a = X[0] - Xn[0], b = X[1] - Xn[1]; return a * a + b * b; };
        const stba::inner::BlockResult res = stba::inner::block_lm<2, 2>(o, 3u, x, lin, cost_at, plus, norm2, dist2);
        std::printf("%d %d %.17g %.17g\n", res.iterations, res.stop, x[0], x[1]);
    }
    return 0;
}
