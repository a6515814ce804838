// Stand-alone driver of slam-tricks_amd/csrc/ba_features.hpp and ba_factor_input.hpp for tests/test_ba_factor_input_cpu.py: no
// device, no HIP.
//   ba_factor_input_driver table          every row of BA_REFUSALS, and for every asker and every one of the 2^9 held masks what
//                                         ba_conflict answers to a setting and to a clearing call; one JSON object on stdout
//   ba_factor_input_driver cases <file>   one command per line of <file>, one JSON object per line on stdout.  Doubles travel as C99
//                                         hexadecimal floats in both directions (exact):
//     pose7 <what, '_' for ' '> <7 doubles>
//     sqrt6 <I | S | N> <36 doubles, not for N>      the information, the square root, or neither given
//     info2 <4 doubles>
//     group_cam <n> <n keys>                         priors by camera
//     group_edges <n> <n cam_i> <n cam_j>            edges by camera (2 n references) and by unordered pair, as the setter makes them
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../slam-tricks_amd/csrc/ba_features.hpp"
#include "../../slam-tricks_amd/csrc/ba_factor_input.hpp"

using namespace stba;

static const char* ba_feature_name(unsigned bit) {
    static const char* const names[BA_FEATURE_COUNT] = {"ITERATIVE_SCHUR", "DOGLEG", "INNER_ITERATIONS", "HOST_LINEARIZER", "ALLREDUCE",
                                                        "LOSS", "INFORMATION", "POSE_PRIORS", "RELATIVE_POSES"};
    for (int k = 0; k < BA_FEATURE_COUNT; ++k) if (bit == 1u << k) return names[k];
    return "?";
}

static std::string quoted(const std::string& s) {
    std::string o = "\"";
    for (char c : s) { if (c == '"' || c == '\\') o += '\\'; o += c; }
    return o + "\"";
}
static void put_doubles(const char* name, const double* v, int n) {
    printf(", \"%s\": [", name);
    for (int k = 0; k < n; ++k) printf("%s\"%a\"", k ? ", " : "", v[k]);
    printf("]");
}
static void put_ints(const char* name, const std::vector<int>& v) {
    printf("%s\"%s\": [", name[0] == '!' ? "" : ", ", name + (name[0] == '!'));
    for (size_t k = 0; k < v.size(); ++k) printf("%s%d", k ? ", " : "", v[k]);
    printf("]");
}
static std::vector<double> get_doubles(std::istringstream& in, int n) {
    std::vector<double> v((size_t)n);
    std::string t;
    for (int k = 0; k < n; ++k) { in >> t; v[(size_t)k] = strtod(t.c_str(), nullptr); }
    return v;
}
static std::vector<int> get_ints(std::istringstream& in, int n) {
    std::vector<int> v((size_t)n);
    for (int k = 0; k < n; ++k) in >> v[(size_t)k];
    return v;
}

static void answers(const char* asker, bool sets) {
    printf("[");
    for (unsigned held = 0; held < (1u << BA_FEATURE_COUNT); ++held) {
        std::string why;
        const int code = ba_conflict(asker, held, &why, sets);
        printf("%s[%d, %s]", held ? ", " : "", code, quoted(why).c_str());
    }
    printf("]");
}

static int table() {
    printf("{\"features\": [");
    for (int k = 0; k < BA_FEATURE_COUNT; ++k) printf("%s\"%s\"", k ? ", " : "", ba_feature_name(1u << k));
    printf("],\n \"rows\": [");
    std::vector<std::string> askers;
    bool first = true;
    for (const BaRefusal& r : BA_REFUSALS) {
        printf("%s\n  {\"asker\": \"%s\", \"held\": [", first ? "" : ",", r.asker);
        bool f2 = true;
        for (int k = 0; k < BA_FEATURE_COUNT; ++k)
            if (r.held & (1u << k)) { printf("%s\"%s\"", f2 ? "" : ", ", ba_feature_name(1u << k)); f2 = false; }
        printf("], \"code\": %d, \"text\": %s, \"when_clearing\": %s}", r.code, quoted(r.text).c_str(), r.when_clearing ? "true" : "false");
        first = false;
        if (askers.empty() || askers.back() != r.asker) askers.push_back(r.asker);
    }
    printf("],\n \"setting\": {");
    for (size_t a = 0; a < askers.size(); ++a) { printf("%s\n  \"%s\": ", a ? "," : "", askers[a].c_str()); answers(askers[a].c_str(), true); }
    printf("},\n \"clearing\": {");
    for (size_t a = 0; a < askers.size(); ++a) { printf("%s\n  \"%s\": ", a ? "," : "", askers[a].c_str()); answers(askers[a].c_str(), false); }
    printf("}}\n");
    return 0;
}

static int cases(const char* path) {
    std::ifstream f(path);
    if (!f) { fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        std::string why;
        if (cmd == "pose7") {
            std::string what;
            in >> what;
            for (char& c : what) if (c == '_') c = ' ';
            const std::vector<double> p = get_doubles(in, 7);
            double out[7] = {0};
            const int rc = pose7_check_normalise(p.data(), out, what.c_str(), &why);
            printf("{\"rc\": %d, \"why\": %s", rc, quoted(why).c_str());
            put_doubles("out", out, 7);
        } else if (cmd == "sqrt6") {
            std::string mode;
            in >> mode;
            const std::vector<double> m = mode == "N" ? std::vector<double>() : get_doubles(in, 36);
            double W[36] = {0}, D[36] = {0};
            const int rc = sqrt_information6(mode == "I" ? m.data() : nullptr, mode == "S" ? m.data() : nullptr, W, &why);
            printf("{\"rc\": %d, \"why\": %s", rc, quoted(why).c_str());
            put_doubles("W", W, 36);
            if (mode == "I") {
                printf(", \"direct_ok\": %s", prior_information_factor(m.data(), D) ? "true" : "false");
                put_doubles("direct", D, 36);
            }
        } else if (cmd == "info2") {
            const std::vector<double> m = get_doubles(in, 4);
            double W[4] = {0};
            printf("{\"ok\": %s", ba_information_factor(m.data(), W) ? "true" : "false");
            put_doubles("W", W, 4);
        } else if (cmd == "group_cam") {
            int n = 0;
            in >> n;
            const std::vector<int> cam = get_ints(in, n);
            std::vector<int> refs((size_t)n), ptr, keys;
            for (int k = 0; k < n; ++k) refs[(size_t)k] = k;
            group_csr((size_t)n, [&](int k) { return cam[(size_t)k]; }, refs, ptr, keys);
            printf("{");
            put_ints("!refs", refs); put_ints("ptr", ptr); put_ints("keys", keys);
        } else if (cmd == "group_edges") {
            int n = 0;
            in >> n;
            const std::vector<int> ci = get_ints(in, n), cj = get_ints(in, n);
            std::vector<int> cref(2 * (size_t)n), cgp, cgc, pref((size_t)n), pgp, hi, lo;
            std::vector<std::pair<int, int>> pairs;
            for (int k = 0; k < 2 * n; ++k) cref[(size_t)k] = k;
            group_csr(2 * (size_t)n, [&](int ref) { return (ref & 1) ? cj[(size_t)(ref >> 1)] : ci[(size_t)(ref >> 1)]; }, cref, cgp, cgc);
            for (int k = 0; k < n; ++k) pref[(size_t)k] = 2 * k + (cj[(size_t)k] > ci[(size_t)k] ? 1 : 0);
            group_csr((size_t)n, [&](int ref) { const size_t e = (size_t)(ref >> 1); return std::make_pair(std::max(ci[e], cj[e]), std::min(ci[e], cj[e])); },
                      pref, pgp, pairs);
            for (const auto& p : pairs) { hi.push_back(p.first); lo.push_back(p.second); }
            printf("{");
            put_ints("!cg_ref", cref); put_ints("cg_ptr", cgp); put_ints("cg_cam", cgc);
            put_ints("pg_ref", pref); put_ints("pg_ptr", pgp); put_ints("pg_hi", hi); put_ints("pg_lo", lo);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        printf("}\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "table")) return table();
    if (argc == 3 && !strcmp(argv[1], "cases")) return cases(argv[2]);
    fprintf(stderr, "usage: %s table | cases <file>\n", argv[0]);
    return 2;
}
