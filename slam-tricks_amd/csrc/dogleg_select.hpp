// dogleg_select.hpp -- Powell's dogleg step at radius Delta from the six scalars of one linearisation.  One
// function for the device (the prologue of ba_dogleg_step_kernel, dogleg.hip) and the host's C++ test (tests/cpp/
// test_dogleg_policy.cpp, plain g++): the case selection and the beta formula are written here and nowhere else.
//
// Coordinates are Ceres' dogleg coordinates z = d .* y (y: the Jacobi-scaled step, d: the clamped column norms of the scaled
// Jacobian).  With gamma = g^ ./ d, u = gamma ./ d and the Gauss-Newton step y_gn (z_gn = d .* y_gn), the step is
// y = a u + b y_gn and every quantity of the step follows from
//   gg = |gamma|^2, gz = gamma^T z_gn, zz = |z_gn|^2, uu = |J^ u|^2, nn = |J^ y_gn|^2, un = (J^ u)^T (J^ y_gn).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define STBA_DOGLEG_HD __host__ __device__
#else
#define STBA_DOGLEG_HD
#endif

namespace stba {

enum { DOGLEG_GAUSS_NEWTON = 0, DOGLEG_CAUCHY = 1, DOGLEG_INTERPOLATED = 2, DOGLEG_INVALID_GN = -1 };

struct DoglegScalars {
    double gg, gz, zz, uu, nn, un;
};

struct DoglegStep {
    int kase;            // DOGLEG_GAUSS_NEWTON | DOGLEG_CAUCHY | DOGLEG_INTERPOLATED; DOGLEG_INVALID_GN: the scalars are not finite
    double a, b;         // y = a u + b y_gn
    double beta;         // the interpolation parameter (case 3), 1 in case 1, 0 in case 2
    double z_norm;       // |z|
    double model;        // m = -(g^T y + |J^ y|^2 / 2)
};

STBA_DOGLEG_HD inline DoglegStep dogleg_select(const DoglegScalars& s, double radius) {
    DoglegStep o;
    o.kase = DOGLEG_INVALID_GN; o.a = 0.0; o.b = 0.0; o.beta = 0.0; o.z_norm = 0.0; o.model = 0.0;
    if (!(std::isfinite(s.gg) && std::isfinite(s.gz) && std::isfinite(s.zz) && std::isfinite(s.uu) && std::isfinite(s.nn) &&
          std::isfinite(s.un)))
        return o;
    const double gn_norm = std::sqrt(s.zz), g_norm = std::sqrt(s.gg);
    const double alpha = s.gg / s.uu;                 // Cauchy step length along -gamma
    if (gn_norm <= radius) {
        // case 1: the Gauss-Newton step lies inside the region
        o.kase = DOGLEG_GAUSS_NEWTON; o.b = 1.0; o.beta = 1.0; o.z_norm = gn_norm;
    } else if (alpha * g_norm >= radius) {
        // case 2: the Cauchy point lies outside: the steepest-descent direction cut at the radius
        o.kase = DOGLEG_CAUCHY; o.a = -radius / g_norm; o.z_norm = radius;
    } else {
        // case 3: the point of the segment from the Cauchy point a = -alpha gamma to b = z_gn at distance radius
        const double b_dot_a = -alpha * s.gz;
        const double a_sq = (alpha * g_norm) * (alpha * g_norm);
        const double b_minus_a_sq = a_sq - 2.0 * b_dot_a + s.zz;
        const double c = b_dot_a - a_sq;
        const double d = std::sqrt(c * c + b_minus_a_sq * (radius * radius - a_sq));
        const double beta = (c <= 0.0) ? (d - c) / b_minus_a_sq : (radius * radius - a_sq) / (d + c);
        o.kase = DOGLEG_INTERPOLATED; o.a = -alpha * (1.0 - beta); o.b = beta; o.beta = beta; o.z_norm = radius;
    }
    // g^T u = |gamma|^2, g^T y_gn = gamma^T z_gn
    o.model = -(o.a * s.gg + o.b * s.gz + 0.5 * (o.a * o.a * s.uu + 2.0 * o.a * o.b * s.un + o.b * o.b * s.nn));
    return o;
}

}  // namespace stba
