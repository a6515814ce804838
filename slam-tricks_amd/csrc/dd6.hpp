// dd6.hpp -- the Cholesky factor of ONE symmetric positive definite 6 x 6 in double-double arithmetic, for both sides: the pose
// graph factors its edge weights with it on the device (pg_information_kernel, pg_linearize.hip), the bundle adjustment its priors'
// and relative poses' information matrices on the host (sqrt_information6, ba_factor_input.hpp).  The factor is made once per
// setter call and is a 6 x 6 per factor, so its cost does not matter, while an FP64 factorisation loses about cond(Omega) eps in
// its last pivots -- an error the caller could not tell from one of the solver's.
// Plain C++: a host compiler builds this header too (tests/cpp/ba_factor_input_driver.cpp); STBA_HD is small_linalg.hpp's.
#pragma once
#include <cmath>

#include "small_linalg.hpp"

namespace stba {

// a value as an unevaluated sum hi + lo
struct dd { double hi, lo; };
STBA_HD inline dd dd_make(double a, double b) { const double s = a + b; return {s, b - (s - a)}; }      // |a| >= |b|
STBA_HD inline dd dd_add(dd x, dd y) {
    const double s = x.hi + y.hi, bb = s - x.hi;
    const double e = ((x.hi - (s - bb)) + (y.hi - bb)) + (x.lo + y.lo);
    return dd_make(s, e);
}
STBA_HD inline dd dd_neg(dd x) { return {-x.hi, -x.lo}; }
STBA_HD inline dd dd_mul(dd x, dd y) {
    const double p = x.hi * y.hi;
    const double e = fma(x.hi, y.hi, -p) + (x.hi * y.lo + x.lo * y.hi);
    return dd_make(p, e);
}
STBA_HD inline dd dd_div(dd x, dd y) {
    const double q1 = x.hi / y.hi;
    dd r = dd_add(x, dd_neg(dd_mul(y, dd{q1, 0.0})));
    const double q2 = r.hi / y.hi;
    r = dd_add(r, dd_neg(dd_mul(y, dd{q2, 0.0})));
    const double q3 = r.hi / y.hi;
    return dd_add(dd_make(q1, q2), dd{q3, 0.0});
}
STBA_HD inline dd dd_sqrt(dd x) {           // x.hi > 0
    const double s = sqrt(x.hi);
    const double p = s * s;
    const dd r = dd_add(x, dd{-p, -fma(s, s, -p)});
    return dd_make(s, r.hi / (2.0 * s));
}

// Omega = L L^T, W = L^T of the symmetric positive definite A (row-major; the lower triangle is factored), by an unblocked Cholesky
// in double-double rounded to FP64 at the end.  false: an entry that is not finite, or a pivot that is not a positive finite number;
// W then holds nothing of use.
STBA_HD inline bool information6_factor(const double* A, double* W) {
    using std::isfinite;
    for (int k = 0; k < 36; ++k) { if (!isfinite(A[k])) return false; W[k] = 0.0; }
    dd L[21];                                  // lower triangle, row a at a (a + 1) / 2
    for (int k = 0; k < 21; ++k) L[k] = dd{0.0, 0.0};
    for (int c = 0; c < 6; ++c) {
        dd d = dd{A[c * 7], 0.0};
        for (int k = 0; k < c; ++k) d = dd_add(d, dd_neg(dd_mul(L[c * (c + 1) / 2 + k], L[c * (c + 1) / 2 + k])));
        if (!(d.hi > 0.0) || !isfinite(d.hi)) return false;
        const dd lcc = dd_sqrt(d);
        L[c * (c + 1) / 2 + c] = lcc;
        W[c * 7] = lcc.hi;
        for (int a = c + 1; a < 6; ++a) {
            dd v = dd{A[a * 6 + c], 0.0};
            for (int k = 0; k < c; ++k) v = dd_add(v, dd_neg(dd_mul(L[a * (a + 1) / 2 + k], L[c * (c + 1) / 2 + k])));
            v = dd_div(v, lcc);
            L[a * (a + 1) / 2 + c] = v;
            W[c * 6 + a] = v.hi;              // W = L^T
        }
    }
    for (int k = 0; k < 36; ++k) if (!isfinite(W[k])) return false;
    return true;
}

}  // namespace stba
