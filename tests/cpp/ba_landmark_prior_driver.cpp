// Stand-alone driver of slam-tricks_amd/csrc/ba_landmark_prior.hpp (the host side of the landmark position priors) and of
// the second refusal table of ba_features.hpp for tests/test_ba_landmark_prior_reference_cpu.py: no device, no HIP.
//   ba_landmark_prior_driver table          every row of BA_REFUSALS_MORE, and for every asker of BOTH tables and every one of the
//                                           2^10 held masks what ba_conflict answers to a setting and to a clearing call
//   ba_landmark_prior_driver cases <file>   one command per line of <file>, one JSON object per line on stdout.  Doubles travel as
//                                           C99 hexadecimal floats in both directions (exact):
//     sqrt3 <I | S | N> <9 doubles, not for N>       the information, the square root, or neither given
//     check <pt> <n_pts> <3 doubles>                 landmark_prior_check with the identity weight
//     group <n> <n_pts> <n landmarks>                landmark_prior_group
//     eval <9 W> <3 position> <3 p>                  r', the six entries of W^T W (xx xy xz yy yz zz) and W^T r'
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../slam-tricks_amd/csrc/ba_features.hpp"
#include "../../slam-tricks_amd/csrc/ba_landmark_prior.hpp"

using namespace stba;

static const char* const NAMES[BA_FEATURE_COUNT_ALL] = {"ITERATIVE_SCHUR", "DOGLEG", "INNER_ITERATIONS", "HOST_LINEARIZER", "ALLREDUCE",
                                                        "LOSS", "INFORMATION", "POSE_PRIORS", "RELATIVE_POSES", "LANDMARK_PRIORS"};

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
static void put_ints(const char* name, const std::vector<int>& v, bool first = false) {
    printf("%s\"%s\": [", first ? "" : ", ", name);
    for (size_t k = 0; k < v.size(); ++k) printf("%s%d", k ? ", " : "", v[k]);
    printf("]");
}
static std::vector<double> get_doubles(std::istringstream& in, int n) {
    std::vector<double> v((size_t)n);
    std::string t;
    for (int k = 0; k < n; ++k) { in >> t; v[(size_t)k] = strtod(t.c_str(), nullptr); }
    return v;
}

static void answers(const char* asker, bool sets) {
    printf("[");
    for (unsigned held = 0; held < (1u << BA_FEATURE_COUNT_ALL); ++held) {
        std::string why;
        const int code = ba_conflict(asker, held, &why, sets);
        printf("%s[%d, %s]", held ? ", " : "", code, quoted(why).c_str());
    }
    printf("]");
}

static int table() {
    printf("{\"features\": [");
    for (int k = 0; k < BA_FEATURE_COUNT_ALL; ++k) printf("%s\"%s\"", k ? ", " : "", NAMES[k]);
    printf("],\n \"rows\": [");
    std::vector<std::string> askers;
    const auto know = [&](const char* a) {
        for (const std::string& s : askers) if (s == a) return;
        askers.push_back(a);
    };
    for (const BaRefusal& r : BA_REFUSALS) know(r.asker);
    bool first = true;
    for (const BaRefusal& r : BA_REFUSALS_MORE) {
        printf("%s\n  {\"asker\": \"%s\", \"held\": [", first ? "" : ",", r.asker);
        bool f2 = true;
        for (int k = 0; k < BA_FEATURE_COUNT_ALL; ++k)
            if (r.held & (1u << k)) { printf("%s\"%s\"", f2 ? "" : ", ", NAMES[k]); f2 = false; }
        printf("], \"code\": %d, \"text\": %s, \"when_clearing\": %s}", r.code, quoted(r.text).c_str(), r.when_clearing ? "true" : "false");
        first = false;
        know(r.asker);
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
        if (cmd == "sqrt3") {
            std::string mode;
            in >> mode;
            const std::vector<double> m = mode == "N" ? std::vector<double>() : get_doubles(in, 9);
            double W[9] = {0};
            const int rc = sqrt_information3(mode == "I" ? m.data() : nullptr, mode == "S" ? m.data() : nullptr, W, &why);
            printf("{\"rc\": %d, \"why\": %s", rc, quoted(why).c_str());
            put_doubles("W", W, 9);
        } else if (cmd == "check") {
            int pt = 0, n_pts = 0;
            in >> pt >> n_pts;
            const std::vector<double> p = get_doubles(in, 3);
            double W[9] = {0};
            const int rc = landmark_prior_check(pt, n_pts, p.data(), nullptr, nullptr, W, &why);
            printf("{\"rc\": %d, \"why\": %s", rc, quoted(why).c_str());
        } else if (cmd == "group") {
            int n = 0, n_pts = 0;
            in >> n >> n_pts;
            std::vector<int> pt((size_t)n), order, start;
            for (int k = 0; k < n; ++k) in >> pt[(size_t)k];
            landmark_prior_group((size_t)n, pt.data(), n_pts, order, start);
            printf("{");
            put_ints("order", order, true); put_ints("start", start);
        } else if (cmd == "eval") {
            const std::vector<double> W = get_doubles(in, 9), pos = get_doubles(in, 3), p = get_doubles(in, 3);
            double rw[3], h[6], g[3];
            lp_residual(W.data(), pos.data(), p.data(), rw);
            int e = 0;
            for (int a = 0; a < 3; ++a)
                for (int b = a; b < 3; ++b) h[e++] = lp_wtw(W.data(), a, b);
            for (int a = 0; a < 3; ++a) g[a] = lp_wtr(W.data(), rw, a);
            printf("{\"symmetric\": %s", lp_wtw(W.data(), 0, 2) == lp_wtw(W.data(), 2, 0) && lp_wtw(W.data(), 1, 0) == lp_wtw(W.data(), 0, 1) ? "true" : "false");
            put_doubles("r", rw, 3); put_doubles("h", h, 6); put_doubles("g", g, 3);
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
