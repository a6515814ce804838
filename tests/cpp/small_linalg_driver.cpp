// small_linalg_driver.cpp -- runs the closed forms of slam-tricks_amd/csrc/small_linalg.hpp on matrices read from stdin, for
// tests/test_small_linalg.py.  Every number crosses the pipe as a %a hex double, so nothing is rounded on the way.
// Commands, one after the other until end of input; each answer is one line:
//   srsv m n  <m*n values, row-major>     -> the n entries of smallest_right_singular_vector
//   svd3      <9 values, row-major>       -> U (9), s (3), V (9)
//   fold m    <m*9 values, row-major>     -> the packed triangular factor (45) after folding the rows in order, then the 9
//                                            entries of smallest_right_singular_vector of that factor (what two_view.hip does)
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
        } else {
            return 2;
        }
    }
    return 0;
}
