// robust_loss.hpp -- the robust loss functions, evaluated on the device: ONE definition for the pose graph's linearisation
// (pg_engine.hip) and bundle adjustment's (ba_kernels.hip)
#pragma once
#include <cfloat>

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

}  // namespace stba
