// robust_loss.hpp -- the robust loss functions, evaluated on the device: ONE definition for the pose graph's linearisation
// (pg_linearize.hip) and bundle adjustment's (ba_kernels.hip)
#pragma once
#include <cfloat>
#include <vector>

#include "common.hpp"      // (with include/stba.h: the STBA_LOSS_* kinds)

namespace stba {

// rho(s), rho'(s), rho''(s) of one residual block's robust loss (s = its squared norm), Ceres' definitions; kind is an STBA_LOSS_* of include/stba.h
// other than TRIVIAL.  rho' is clamped from below by DBL_MIN where Ceres clamps it.
__device__ inline void robust_loss(int kind, double a, double b, double s, double* rho) {
    const double b2 = a * a;
    switch (kind) {
    case STBA_LOSS_HUBER:
        if (s > b2) {
            const double q = sqrt(s);
            rho[0] = 2.0 * a * q - b2; rho[1] = fmax(DBL_MIN, a / q); rho[2] = -rho[1] / (2.0 * s);
        } else { rho[0] = s; rho[1] = 1.0; rho[2] = 0.0; }
        break;
    case STBA_LOSS_SOFTLONE: {
        const double c = 1.0 / b2, sum = 1.0 + s * c, t = sqrt(sum);
        rho[0] = 2.0 * b2 * (t - 1.0); rho[1] = fmax(DBL_MIN, 1.0 / t); rho[2] = -(c * rho[1]) / (2.0 * sum);
        break;
    }
    case STBA_LOSS_CAUCHY: {
        const double c = 1.0 / b2, sum = 1.0 + s * c, inv = 1.0 / sum;
        rho[0] = b2 * log(sum); rho[1] = fmax(DBL_MIN, inv); rho[2] = -c * (inv * inv);
        break;
    }
    case STBA_LOSS_ARCTAN: {
        const double c = 1.0 / b2, sum = 1.0 + s * s * c, inv = 1.0 / sum;
        rho[0] = a * atan2(s, a); rho[1] = fmax(DBL_MIN, inv); rho[2] = -2.0 * s * c * (inv * inv);
        break;
    }
    case STBA_LOSS_TOLERANT: {
        const double c = b * log(1.0 + exp(-a / b)), x = (s - a) / b;
        if (x > 36.7) { rho[0] = s - a - c; rho[1] = 1.0; rho[2] = 0.0; }      // (36.7 = log(2^53): e^x + 1 == e^x from here on)
        else {
            const double ex = exp(x);
            rho[0] = b * log(1.0 + ex) - c; rho[1] = fmax(DBL_MIN, ex / (1.0 + ex)); rho[2] = 0.5 / (b * (1.0 + cosh(x)));
        }
        break;
    }
    case STBA_LOSS_TUKEY:
        if (s <= b2) {
            const double v = 1.0 - s / b2, v2 = v * v;
            rho[0] = b2 / 3.0 * (1.0 - v2 * v); rho[1] = v2; rho[2] = -2.0 / b2 * v;
        } else { rho[0] = b2 / 3.0; rho[1] = 0.0; rho[2] = 0.0; }
        break;
    default:                                    // TRIVIAL with a scale
        rho[0] = s; rho[1] = 1.0; rho[2] = 0.0;
    }
}

// host: a caller's loss table (m entries; a, b, scale may be null) checked before an engine takes it.  The first bad entry is
// refused as "<who>: <noun> <index>: <reason>"; otherwise ha, hb, hs hold a, b, scale with the defaults (1) where an entry's kind does
// not read them.  `noun`: what an entry belongs to ("observation", "edge")
inline int loss_table_check(const char* who, const char* noun, size_t m, const int* kind, const double* a, const double* b,
                            const double* scale, std::vector<double>& ha, std::vector<double>& hb, std::vector<double>& hs) {
    ha.assign(m, 1.0); hb.assign(m, 1.0); hs.assign(m, 1.0);
    for (size_t e = 0; e < m; ++e) {
        const int kd = kind[e];
        std::string why;
        if (kd < STBA_LOSS_TRIVIAL || kd > STBA_LOSS_TUKEY) why = "unknown loss kind " + std::to_string(kd);
        else if (kd != STBA_LOSS_TRIVIAL && (!a || !std::isfinite(a[e]) || !(a[e] > 0.0))) why = "the loss parameter a must be finite and positive";
        else if (kd == STBA_LOSS_TOLERANT && (!b || !std::isfinite(b[e]) || !(b[e] > 0.0))) why = "the loss parameter b must be finite and positive";
        else if (scale && (!std::isfinite(scale[e]) || !(scale[e] >= 0.0))) why = "the loss scale must be finite and not negative";
        if (!why.empty()) return fail(STBA_ERR_INVALID_ARGUMENT, std::string(who) + ": " + noun + " " + std::to_string(e) + ": " + why);
        if (kd != STBA_LOSS_TRIVIAL) ha[e] = a[e];
        if (kd == STBA_LOSS_TOLERANT) hb[e] = b[e];
        if (scale) hs[e] = scale[e];
    }
    return STBA_OK;
}

}  // namespace stba
