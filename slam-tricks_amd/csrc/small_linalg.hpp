// small_linalg.hpp -- host-side dense helpers for the closed-form initialisers (calib_io.cpp, two_view.hip), and the closed forms
// that run on both sides: the Givens row fold of two_view.hip and the SPD 3 x 3 inverse of the landmark kernels (ba_kernels.hip).
// Plain C++: a host compiler builds this header too (tests/cpp/small_linalg_driver.cpp)
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define STBA_HD __host__ __device__
#define STBA_UNROLL _Pragma("unroll")
#else
#define STBA_HD
#define STBA_UNROLL
#endif

namespace stba {

// fold the row a (9 entries) into the packed upper-triangular R (row k holds R[k][k..8])
STBA_HD inline void givens_fold(double (&R)[45], double (&a)[9]) {
    int idx = 0;
    STBA_UNROLL
    for (int k = 0; k < 9; ++k) {
        const double ak = a[k];
        if (ak != 0.0) {
            const double d = R[idx];
            const double r = sqrt(d * d + ak * ak);
            const double c = d / r, s = ak / r;
            R[idx] = r;
            STBA_UNROLL
            for (int j = k + 1; j < 9; ++j) {
                const double x = R[idx + j - k], y = a[j];
                R[idx + j - k] = c * x + s * y;
                a[j] = c * y - s * x;
            }
        }
        idx += 9 - k;
    }
}

// Inverse of the symmetric positive definite 3 x 3 block A, packed (00, 01, 02, 11, 12, 22), and a square root of that inverse:
//   Ai (packed like A) = A^-1,   R (3 x 3, row-major) with R R^T = A^-1.
// A is scaled by powers of two to a diagonal in [0.5, 2) (exact: it only keeps the products in range) and factored B = L L^T
// with the larger of the two remaining pivots taken second; L is inverted by substitution and A^-1 = S L^-T L^-1 S.  The error
// is eps lambda_1 / lambda_3 of A^-1 -- cofactors over the determinant give eps lambda_1^2 / (lambda_2 lambda_3), and lose
// definiteness on blocks with two small eigenvalues.  Ai is formed from one set of products per entry: packed, so exactly
// symmetric.  R is a row permutation of a triangular matrix (three exact zeros).
// Returns false, Ai and R untouched, where A is not numerically positive definite: a diagonal entry that is not positive and
// finite, or a pivot below SPD3_PIVOT_MIN of its diagonal entry.  pivot / diagonal = 1 - the squared multiple correlation with
// the rows taken before it, which no diagonal scaling changes; it is at least 1 / (3 kappa_2(A)), so blocks up to kappa 1e13 pass
// with a margin of nine.  The last pivot of a rank-2 block -- one observation, no damping -- is rounding noise of either sign,
// a few eps of its diagonal entry BECAUSE the better-determined row went before it (without that choice the noise is eps over
// the second pivot's ratio, and no threshold separates the two kinds of block).
constexpr double SPD3_PIVOT_MIN = 16.0 * 2.220446049250313e-16;
STBA_HD inline bool spd3_inverse(const double A[6], double Ai[6], double R[9]) {
    if (!(A[0] > 0.0) || !(A[3] > 0.0) || !(A[5] > 0.0) || !(A[0] < 1e300) || !(A[3] < 1e300) || !(A[5] < 1e300)) return false;
    int e0, e1, e2;
    frexp(A[0], &e0); frexp(A[3], &e1); frexp(A[5], &e2);
    const double s0 = ldexp(1.0, -(e0 >> 1));
    double s1 = ldexp(1.0, -(e1 >> 1)), s2 = ldexp(1.0, -(e2 >> 1));
    const double b00 = A[0] * s0 * s0, b12 = A[4] * s1 * s2;
    double b01 = A[1] * s0 * s1, b02 = A[2] * s0 * s2, b11 = A[3] * s1 * s1, b22 = A[5] * s2 * s2;
    const double l00 = sqrt(b00), m00 = 1.0 / l00;
    double l10 = b01 * m00, l20 = b02 * m00;
    double d1 = b11 - l10 * l10;
    const double d1alt = b22 - l20 * l20;
    // rows 1 and 2 change places where row 2 is the better determined one (ratios compared without a division)
    const bool swap = d1alt * b11 > d1 * b22;
    if (swap) {
        double t;
        t = s1; s1 = s2; s2 = t;
        t = b11; b11 = b22; b22 = t;
        t = l10; l10 = l20; l20 = t;
        d1 = d1alt;
    }
    if (!(d1 > SPD3_PIVOT_MIN * b11)) return false;
    const double l11 = sqrt(d1), m11 = 1.0 / l11;
    const double l21 = (b12 - l20 * l10) * m11;
    const double d2 = (b22 - l20 * l20) - l21 * l21;
    if (!(d2 > SPD3_PIVOT_MIN * b22)) return false;
    const double l22 = sqrt(d2), m22 = 1.0 / l22;
    // M = L^-1 (lower), then back to A's scale: column k of M times s_k
    const double m10 = -(l10 * m00) * m11;
    const double m21 = -(l21 * m11) * m22;
    const double m20 = -(l20 * m00 + l21 * m10) * m22;
    const double r00 = m00 * s0, r01 = m10 * s0, r02 = m20 * s0, r11 = m11 * s1, r12 = m21 * s1, r22 = m22 * s2;
    const double i00 = r00 * r00 + r01 * r01 + r02 * r02, i01 = r01 * r11 + r02 * r12, i02 = r02 * r22;
    const double i11 = r11 * r11 + r12 * r12, i12 = r12 * r22, i22 = r22 * r22;
    const int p = swap ? 2 : 1, q = swap ? 1 : 2;
    R[0] = r00; R[1] = r01; R[2] = r02;
    R[p * 3] = 0.0; R[p * 3 + 1] = r11; R[p * 3 + 2] = r12;
    R[q * 3] = 0.0; R[q * 3 + 1] = 0.0; R[q * 3 + 2] = r22;
    Ai[0] = i00; Ai[1] = swap ? i02 : i01; Ai[2] = swap ? i01 : i02;
    Ai[3] = swap ? i22 : i11; Ai[4] = i12; Ai[5] = swap ? i11 : i22;
    return true;
}

// One-sided (Hestenes) Jacobi SVD of A (m x n, row-major, m >= n): on return the columns of A are
// U * diag(sigma) (mutually orthogonal), V (n x n, row-major) holds the right singular vectors.
inline void jacobi_svd_onesided(std::vector<double>& A, int m, int n, std::vector<double>& V) {
    V.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                double app = 0, aqq = 0, apq = 0;
                for (int r = 0; r < m; ++r) {
                    const double x = A[(size_t)r * n + p], y = A[(size_t)r * n + q];
                    app += x * x; aqq += y * y; apq += x * y;
                }
                if (apq == 0.0) continue;
                // |cos| of the angle between the two columns.  sqrt(app) * sqrt(aqq), not sqrt(app * aqq): the product of
                // the squares leaves the double range for entries near 1e+-150, and the sweep then stops unconverged
                const double den = std::sqrt(app) * std::sqrt(aqq);
                if (den > 0.0) off = std::max(off, std::fabs(apq) / den);
                const double zeta = (aqq - app) / (2.0 * apq);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < m; ++r) {
                    const double x = A[(size_t)r * n + p], y = A[(size_t)r * n + q];
                    A[(size_t)r * n + p] = c * x - s * y;
                    A[(size_t)r * n + q] = s * x + c * y;
                }
                for (int r = 0; r < n; ++r) {
                    const double x = V[(size_t)r * n + p], y = V[(size_t)r * n + q];
                    V[(size_t)r * n + p] = c * x - s * y;
                    V[(size_t)r * n + q] = s * x + c * y;
                }
            }
        if (off < 1e-15) break;
    }
}

// right singular vector of the smallest singular value (same accuracy class as Eigen::JacobiSVD, which the
// reference uses; forming A^T A instead would square the condition number of the unnormalised DLT systems)
inline void smallest_right_singular_vector(std::vector<double> A, int m, int n, double* v_out) {
    std::vector<double> V;
    jacobi_svd_onesided(A, m, n, V);
    int best = 0;
    double bn = 1e300;
    for (int j = 0; j < n; ++j) {
        double nn = 0;
        for (int r = 0; r < m; ++r) nn += A[(size_t)r * n + j] * A[(size_t)r * n + j];
        if (nn < bn) { bn = nn; best = j; }
    }
    for (int r = 0; r < n; ++r) v_out[r] = V[(size_t)r * n + best];
}

// full SVD of a 3x3 (row-major): M = U diag(s) V^T, s descending, U and V orthogonal at every rank (a singular
// value of zero, or below 1e-12 of the largest, gets the cross product of the other two left vectors)
inline void svd3(const double* M, double* U, double* s, double* V) {
    std::vector<double> A(M, M + 9), Vv;
    jacobi_svd_onesided(A, 3, 3, Vv);
    double nrm[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) nrm[j] = std::sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    std::sort(ord, ord + 3, [&](int a, int b) { return nrm[a] > nrm[b]; });
    for (int k = 0; k < 3; ++k) {
        const int j = ord[k];
        s[k] = nrm[j];
        for (int r = 0; r < 3; ++r) { V[r * 3 + k] = Vv[(size_t)r * 3 + j]; U[r * 3 + k] = (nrm[j] > 0) ? A[(size_t)r * 3 + j] / nrm[j] : 0.0; }
    }
    if (!(s[2] > 1e-12 * s[0])) {            // rank <= 2: u3 from the cross product of the other two left vectors
        if (!(s[0] > 0.0)) {                 // M = 0: any orthonormal basis
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 2; ++c) U[r * 3 + c] = (r == c) ? 1.0 : 0.0;
        } else if (!(s[1] > 0.0)) {          // rank 1 with an exactly zero second column: any unit vector orthogonal to u1
            int k = 0;
            for (int r = 1; r < 3; ++r)
                if (std::fabs(U[r * 3]) < std::fabs(U[k * 3])) k = r;
            const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
            const double w[3] = {U[3] * e[2] - U[6] * e[1], U[6] * e[0] - U[0] * e[2], U[0] * e[1] - U[3] * e[0]};
            const double nw = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            for (int r = 0; r < 3; ++r) U[r * 3 + 1] = w[r] / nw;
        }
        const double c0 = U[3] * U[7] - U[6] * U[4], c1 = U[6] * U[1] - U[0] * U[7], c2 = U[0] * U[4] - U[3] * U[1];
        // the sign of the Jacobi column where it has one, so that U diag(s) V^T stays M for a small non-zero s[2]
        const int j = ord[2];
        const double sg = (c0 * A[j] + c1 * A[3 + j] + c2 * A[6 + j] < 0.0) ? -1.0 : 1.0;
        U[2] = sg * c0; U[5] = sg * c1; U[8] = sg * c2;
    }
}

}  // namespace stba
