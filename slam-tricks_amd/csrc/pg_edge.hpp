// pg_edge.hpp -- the pose graph's factor maths on the device, for the units that linearise with it: the residual and the two Jacobians of
// one relative-pose edge (pg_edge) and the whitening by a 6 x 6 square-root information (pg_whiten_cols).  pg_linearize.hip runs them
// per edge; pg_prior.hip runs the same pg_edge with T_i = I for a node pose prior -- there is one log and one Jr^-1 in this engine.
// Everything here is inline; no kernel is declared or defined here.  Internal linkage, like pg_device.hpp.
#pragma once
#include "pg_device.hpp"

namespace stba {
namespace {

// r, Ji, Jj of one edge
__device__ inline void pg_edge(const double* Ti, const double* Tj, const double* Z, double* r, double* Ji, double* Jj) {
    double Zi[7], Tii[7], A[7], E[7];
    se3_inverse(Z, Zi);
    se3_inverse(Ti, Tii);
    se3_compose(Tii, Tj, A);
    se3_compose(Zi, A, E);
    if (E[3] < 0) for (int k = 0; k < 4; ++k) E[k] = -E[k];
    se3_log7(E, r);
    if (!Ji) return;
    // Jr^-1 = I + ad/2 + ad^2/12, ad(xi) = [[hat(th), hat(rho)], [0, hat(th)]]
    double Hr[9], Ht[9], ad[36], Jr[36];
    hat3d(r, Hr); hat3d(r + 3, Ht);
    for (int k = 0; k < 36; ++k) ad[k] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { ad[i * 6 + j] = Ht[i * 3 + j]; ad[i * 6 + 3 + j] = Hr[i * 3 + j]; ad[(3 + i) * 6 + 3 + j] = Ht[i * 3 + j]; }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += ad[i * 6 + k] * ad[k * 6 + j];
            Jr[i * 6 + j] = (i == j ? 1.0 : 0.0) + 0.5 * ad[i * 6 + j] + s / 12.0;
        }
    for (int k = 0; k < 36; ++k) Jj[k] = Jr[k];
    // Ad(T_j^-1 T_i) = [[R, hat(t) R], [0, R]]
    double Ainv[7], R[9], Hh[9], AdM[36];
    se3_inverse(A, Ainv);
    quat_to_rot(Ainv, R);
    hat3d(Ainv + 4, Hh);
    for (int k = 0; k < 36; ++k) AdM[k] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += Hh[i * 3 + k] * R[k * 3 + j];
            AdM[i * 6 + j] = R[i * 3 + j]; AdM[i * 6 + 3 + j] = s; AdM[(3 + i) * 6 + 3 + j] = R[i * 3 + j];
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += Jr[i * 6 + k] * AdM[k * 6 + j];
            Ji[i * 6 + j] = -s;
        }
}

// x <- W x for `cols` columns of a 6-row matrix held row-major with row stride `ld` (a 6-vector: cols = ld = 1): one column at a
// time through a 6-vector of temporaries, so that the product needs W (36) and six doubles on top of what is whitened in place
__device__ inline void pg_whiten_cols(const double* W, double* x, int cols, int ld) {
    for (int c = 0; c < cols; ++c) {
        double t[6];
        for (int a = 0; a < 6; ++a) {
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += W[a * 6 + k] * x[k * ld + c];
            t[a] = s;
        }
        for (int a = 0; a < 6; ++a) x[a * ld + c] = t[a];
    }
}

}  // namespace
}  // namespace stba
