// Stand-alone driver of slam-tricks_amd/csrc/pg_plan.hpp for tests/test_pg_plan_cpu.py: no device, no HIP.
//   pg_plan_driver <case file>
// One command per line of the case file, one JSON object per line on stdout.  Doubles travel as C99 hexadecimal floats in both
// directions (exact).  Every array is printed in full, with the 64-bit FNV-1a digest of its little-endian int32 bytes next to it.
//   graph <n> <m> <group_opt> <k> <k x (one_kernel_solve several_ranks cus lds_max_optin)> <m edge_i> <m edge_j>
//         pg_check_edges; then, if no edge is bad, pg_build_ends, pg_plan_coarse, and pg_one_kernel_fits for each of the k settings
//   fits <agg> <na> <nc> <max_group_ends> <one_kernel_solve> <several_ranks> <cus> <lds_max_optin>       a plan given as such
//   gauge <n> <m> <has_fixed> <m edge_i> <m edge_j> [<n fixed>]
//   eta <forcing_eta0> <forcing_eta_min> <forcing_eta_final> <function_tolerance> <eta> <g2> <g2_new> <cost_change> <new_cost>
//   waits <coarse_async> <coarse_async_after> <coarse_async_decrease> <forcing> <jobs> <iter> <last_rel_decrease>
//   constants
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../slam-tricks_amd/csrc/pg_plan.hpp"

using namespace stba;

static unsigned long long fnv1a(const void* p, size_t bytes) {
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* q = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < bytes; ++k) { h ^= q[k]; h *= 1099511628211ull; }
    return h;
}

static void put_array(const char* name, const std::vector<int>& v) {
    static_assert(sizeof(int) == sizeof(int32_t), "the digests are over int32");
    printf(", \"%s\": {\"digest\": \"%016llx\", \"values\": [", name, fnv1a(v.data(), v.size() * sizeof(int)));
    for (size_t k = 0; k < v.size(); ++k) printf("%s%d", k ? ", " : "", v[k]);
    printf("]}");
}
static std::vector<int> get_ints(std::istringstream& in, int n) {
    std::vector<int> v((size_t)n);
    for (int k = 0; k < n; ++k) in >> v[(size_t)k];
    return v;
}
static double get_double(std::istringstream& in) {
    std::string t;
    in >> t;
    return strtod(t.c_str(), nullptr);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <case file>\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "graph") {
            int n = 0, m = 0, group_opt = 0, k = 0;
            in >> n >> m >> group_opt >> k;
            const std::vector<int> lim = get_ints(in, 4 * k), ei = get_ints(in, m), ej = get_ints(in, m);
            if (!in) { fprintf(stderr, "short line: %s\n", line.substr(0, 60).c_str()); return 2; }
            const int bad = pg_check_edges(n, m, ei.data(), ej.data());
            printf("{\"bad_edge\": %d", bad);
            if (bad < 0) {
                PgEnds e;
                pg_build_ends(n, m, ei.data(), ej.data(), &e);
                put_array("node_start", e.node_start); put_array("end_code", e.end_code); put_array("end_node", e.end_node);
                put_array("end_pos", e.end_pos); put_array("end_rem", e.end_rem);
                PgCoarsePlan c;
                std::string why;
                const int rc = pg_plan_coarse(n, e.node_start, group_opt, &c, &why);
                printf(", \"rc\": %d, \"why\": \"%s\"", rc, why.c_str());          // (the messages hold no quote and no backslash)
                if (rc == 0) {
                    printf(", \"plan\": {\"agg\": %d, \"na\": %d, \"nc\": %d, \"np\": %d, \"parts\": %d, \"max_group_ends\": %d, \"build_lds_bytes\": %zu}, \"fits\": [",
                           c.agg, c.na, c.nc, c.np, c.parts, c.max_group_ends, c.build_lds_bytes);
                    for (int q = 0; q < k; ++q)
                        printf("%s%d", q ? ", " : "", (int)pg_one_kernel_fits(c, lim[(size_t)4 * q], lim[(size_t)4 * q + 1] != 0, PgDeviceLimits{lim[(size_t)4 * q + 2], lim[(size_t)4 * q + 3]}));
                    printf("]");
                }
            }
        } else if (cmd == "fits") {
            PgCoarsePlan c;
            int one = 0, ranks = 0, cus = 0, lds = 0;
            in >> c.agg >> c.na >> c.nc >> c.max_group_ends >> one >> ranks >> cus >> lds;
            printf("{\"fits\": %d", (int)pg_one_kernel_fits(c, one, ranks != 0, PgDeviceLimits{cus, lds}));
        } else if (cmd == "gauge") {
            int n = 0, m = 0, has_fixed = 0;
            in >> n >> m >> has_fixed;
            const std::vector<int> ei = get_ints(in, m), ej = get_ints(in, m), fx = get_ints(in, has_fixed ? n : 0);
            const std::vector<unsigned char> fixed(fx.begin(), fx.end());
            int size = -1, first = -1;
            const bool ok = pg_gauge_fixed(n, m, ei.data(), ej.data(), has_fixed ? fixed.data() : nullptr, &size, &first);
            printf("{\"ok\": %d, \"size\": %d, \"first_node\": %d", (int)ok, size, first);
        } else if (cmd == "eta") {
            stba_pcg_options pcg;
            stba_lm_options opt;
            memset(&pcg, 0, sizeof pcg); memset(&opt, 0, sizeof opt);
            pcg.forcing_eta0 = get_double(in); pcg.forcing_eta_min = get_double(in); pcg.forcing_eta_final = get_double(in);
            opt.function_tolerance = get_double(in);
            const double eta = get_double(in), g2 = get_double(in), g2_new = get_double(in), cost_change = get_double(in), new_cost = get_double(in);
            printf("{\"eta\": \"%a\"", pg_next_eta(pcg, opt, eta, g2, g2_new, cost_change, new_cost));
        } else if (cmd == "waits") {
            stba_pcg_options pcg;
            memset(&pcg, 0, sizeof pcg);
            int forcing = 0, jobs = 0, iter = 0;
            in >> pcg.coarse_async >> pcg.coarse_async_after;
            pcg.coarse_async_decrease = get_double(in);
            in >> forcing >> jobs >> iter;
            const double dec = get_double(in);
            printf("{\"waits\": %d", (int)pg_waits_for_own_inverse(pcg, forcing != 0, jobs, iter, dec));
        } else if (cmd == "constants") {
            printf("{\"PG_NT\": %d, \"PG_NPW\": %d, \"PP_T\": %d, \"PP_VCAP\": %d, \"PP_NCMAX\": %d, \"PP_SLOT\": %d, \"PP_STAMP\": %d, \"PP_GROUPS_MAX\": %d, "
                   "\"PP_GROUP_NODES_MAX\": %d, \"PP_LDS_MAX\": %zu, \"PG_COARSE_BUILD_LDS_MAX\": %zu, \"pp_lds_bytes_256_1536\": %zu, \"pg_coarse_build_lds_6_4\": %zu",
                   PG_NT, PG_NPW, PP_T, PP_VCAP, PP_NCMAX, PP_SLOT, PP_STAMP, PP_GROUPS_MAX, PP_GROUP_NODES_MAX, PP_LDS_MAX, PG_COARSE_BUILD_LDS_MAX,
                   pp_lds_bytes(256, 1536), pg_coarse_build_lds(6, 4));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        printf("}\n");
    }
    return 0;
}
