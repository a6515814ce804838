// small_linalg_driver.cpp -- runs the closed forms of slam-tricks_amd/csrc/small_linalg.hpp on matrices read from stdin, for
// tests/test_small_linalg.py.  Every number crosses the pipe as a %a hex double, so nothing is rounded on the way.
// Commands, one after the other until end of input; each answer is one line:
//   srsv m n  <m*n values, row-major>     -> the n entries of smallest_right_singular_vector
//   svd3      <9 values, row-major>       -> U (9), s (3), V (9)
//   fold m    <m*9 values, row-major>     -> the packed triangular factor (45) after folding the rows in order, then the 9
//                                            entries of smallest_right_singular_vector of that factor (what two_view.hip does)
//   inv3 n    <n*6 values: packed SPD 3x3> -> per block 23 values: spd3_inverse's flag (1 = inverted), Ai (6), R (9), then the
//                                            flag and Ai (6) of the cofactor formula the landmark kernels used before it
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../slam-tricks_amd/csrc/small_linalg.hpp"

static bool read_doubles(double* out, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (std::scanf("%la", &out[i]) != 1) return false;
    return true;
}

static void print_doubles(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) std::printf("%a%c", v[i], i + 1 == n ? '\n' : ' ');
}

// the cofactor inverse (inv3_sym6 of common.hpp before spd3_inverse replaced it in the landmark kernels), kept to print its error
static bool inv3_cofactor(const double A[6], double Ai[6]) {
    const double a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5];
    const double C00 = d * f - e * e, C01 = c * e - b * f, C02 = b * e - c * d;
    const double det = a * C00 + b * C01 + c * C02;
    if (!(det > 0.0) || !(std::fabs(det) < 1e300)) return false;
    const double inv = 1.0 / det;
    Ai[0] = C00 * inv; Ai[1] = C01 * inv; Ai[2] = C02 * inv;
    Ai[3] = (a * f - c * c) * inv; Ai[4] = (b * c - a * e) * inv; Ai[5] = (a * d - b * b) * inv;
    return true;
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "srsv")) {
            int m, n;
            if (std::scanf("%d %d", &m, &n) != 2 || m < n || n < 1) return 2;
            std::vector<double> A((size_t)m * n), v(n);
            if (!read_doubles(A.data(), A.size())) return 2;
            stba::smallest_right_singular_vector(A, m, n, v.data());
            print_doubles(v.data(), v.size());
        } else if (!std::strcmp(cmd, "svd3")) {
            double M[9], out[21];
            if (!read_doubles(M, 9)) return 2;
            stba::svd3(M, out, out + 9, out + 12);
            print_doubles(out, 21);
        } else if (!std::strcmp(cmd, "fold")) {
            int m;
            if (std::scanf("%d", &m) != 1 || m < 0) return 2;
            std::vector<double> A((size_t)m * 9);
            if (!read_doubles(A.data(), A.size())) return 2;
            double R[45] = {0}, out[54];
            for (int i = 0; i < m; ++i) {
                double a[9];
                for (int j = 0; j < 9; ++j) a[j] = A[(size_t)i * 9 + j];
                stba::givens_fold(R, a);
            }
            std::vector<double> Rfull(81, 0.0);
            int idx = 0;
            for (int k = 0; k < 9; ++k) { for (int j = k; j < 9; ++j) Rfull[(size_t)k * 9 + j] = R[idx + j - k]; idx += 9 - k; }
            std::memcpy(out, R, sizeof R);
            stba::smallest_right_singular_vector(Rfull, 9, 9, out + 45);
            print_doubles(out, 54);
        } else if (!std::strcmp(cmd, "inv3")) {
            int n;
            if (std::scanf("%d", &n) != 1 || n < 0) return 2;
            std::vector<double> A((size_t)n * 6), out((size_t)n * 23, 0.0);
            if (!read_doubles(A.data(), A.size())) return 2;
            for (int i = 0; i < n; ++i) {
                double* o = &out[(size_t)i * 23];
                o[0] = stba::spd3_inverse(&A[(size_t)i * 6], o + 1, o + 7) ? 1.0 : 0.0;
                o[16] = inv3_cofactor(&A[(size_t)i * 6], o + 17) ? 1.0 : 0.0;
            }
            print_doubles(out.data(), out.size());
        } else {
            return 2;
        }
    }
    return 0;
}
