// ba_factor_input.hpp -- what the factor setters of the bundle adjustment do to their input before anything reaches the device: the
// check and normalisation of an SE(3) pose row, the 6 x 6 and 2 x 2 square-root informations, and the grouping of factor references
// into a CSR.  A check returns 0, or a status of include/stba.h with the reason in *why (the caller puts "<who>: prior <k>: " in
// front).  Host only: the standard library and include/stba.h, nothing of HIP (tests/cpp/ba_factor_input_driver.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/stba.h"
#include "dd6.hpp"

namespace stba {

// one row [q(x, y, z, w), t] of a prior's pose or an edge's measurement -> out, the quaternion normalised.  `what`: "the pose" or
// "the measurement".  A quaternion that is unit to rounding (|n^2 - 1| <= 8 eps) keeps its bits: a prior AT a camera's pose then has
// the residual exactly 0
inline int pose7_check_normalise(const double* in, double* out, const char* what, std::string* why) {
    for (int j = 0; j < 7; ++j)
        if (!std::isfinite(in[j])) { *why = std::string(what) + " has an entry that is not finite"; return STBA_ERR_INVALID_ARGUMENT; }
    const double n2 = ((in[0] * in[0] + in[1] * in[1]) + in[2] * in[2]) + in[3] * in[3];
    if (!(n2 > 0.0) || !std::isfinite(n2)) { *why = "zero quaternion"; return STBA_ERR_INVALID_ARGUMENT; }
    const double sc = std::fabs(n2 - 1.0) <= 8 * 2.220446049250313e-16 ? 1.0 : 1.0 / std::sqrt(n2);
    for (int j = 0; j < 4; ++j) out[j] = in[j] * sc;
    for (int j = 4; j < 7; ++j) out[j] = in[j];
    return 0;
}

// Omega = L L^T, W = L^T of ONE symmetric positive definite 6 x 6 (row-major; the lower triangle is factored): information6_factor of
// dd6.hpp, the double-double Cholesky the pose graph factors its edge weights with on the device, under the name the factor
// setters know it by.  false: an entry that is not finite, or a pivot that is not a positive finite number.
inline bool prior_information_factor(const double* A, double* W) { return information6_factor(A, W); }

// the 6 x 6 square-root information W [36] of one factor: the caller's square root as it is (any finite matrix, rank-deficient ones
// included), the factor of the caller's information matrix, or -- neither given -- the identity
inline int sqrt_information6(const double* information_k, const double* sqrt_information_k, double* W, std::string* why) {
    if (sqrt_information_k) {
        for (int j = 0; j < 36; ++j) {
            if (!std::isfinite(sqrt_information_k[j])) { *why = "the square-root information has an entry that is not finite"; return STBA_ERR_INVALID_ARGUMENT; }
            W[j] = sqrt_information_k[j];
        }
    } else if (information_k) {
        for (int j = 0; j < 36; ++j)
            if (!std::isfinite(information_k[j])) { *why = "the information matrix has an entry that is not finite"; return STBA_ERR_INVALID_ARGUMENT; }
        if (!prior_information_factor(information_k, W)) { *why = "the information matrix is not positive definite"; return STBA_ERR_NOT_POSITIVE_DEFINITE; }
    } else {
        for (int j = 0; j < 36; ++j) W[j] = (j % 7 == 0) ? 1.0 : 0.0;
    }
    return 0;
}

// Omega = L L^T, W = L^T of ONE symmetric 2 x 2 from its lower triangle (a, b, c) = (in[0], in[2], in[3]): l11 = sqrt(a), l21 = b / l11,
// l22 = sqrt(c - b^2 / a).  The pivot is formed directly from a, b, c with error-free products: t = fl(b / a), t b = p + e and
// b - t a = rem exactly (FMA), c - p = sum + err exactly (two-sum), so pivot = sum + (err - e - rem b / a) carries one rounding where
// c - l21^2 would carry kappa(Omega) of them: every entry of W is within 4 eps of the exact factor of the matrix given.
// false: an entry that is not finite, or a pivot that is not a positive finite number.
inline bool ba_information_factor(const double* in, double* W) {
    const double a = in[0], bb = in[2], c = in[3];
    if (!std::isfinite(a) || !std::isfinite(in[1]) || !std::isfinite(bb) || !std::isfinite(c) || !(a > 0.0)) return false;
    const double l11 = std::sqrt(a);
    const double t = bb / a;
    const double p = t * bb, e = std::fma(t, bb, -p);
    const double rem = std::fma(-t, a, bb);
    const double sum = c - p, z = sum - c;
    const double err = (c - (sum - z)) + (-p - z);
    const double pivot = sum + ((err - e) - rem * bb / a);
    if (!(pivot > 0.0) || !std::isfinite(pivot)) return false;
    W[0] = l11; W[1] = bb / l11; W[2] = 0.0; W[3] = std::sqrt(pivot);
    return std::isfinite(W[0]) && std::isfinite(W[1]) && std::isfinite(W[3]);
}

// refs [n_refs] (the caller's order) -> sorted by key_of(ref), stably: inside a group of equal keys the caller's order stays; the
// groups as a CSR: ptr [groups + 1] into refs, keys [groups].  Key: anything with < and !=, an int camera or a std::pair of them
template <class Key, class KeyOf>
inline void group_csr(size_t n_refs, KeyOf key_of, std::vector<int>& refs, std::vector<int>& ptr, std::vector<Key>& keys) {
    std::stable_sort(refs.begin(), refs.end(), [&](int x, int y) { return key_of(x) < key_of(y); });
    ptr.clear(); keys.clear();
    for (size_t p = 0; p < n_refs; ++p) {
        const Key k = key_of(refs[p]);
        if (p == 0 || k != keys.back()) { ptr.push_back((int)p); keys.push_back(k); }
    }
    ptr.push_back((int)n_refs);
}

}  // namespace stba
