// Stand-alone driver of slam-tricks_amd/csrc/schur_plan.hpp for tests/test_schur_plan_cpu.py: no device, no HIP.
//   schur_plan_driver <case file> <output directory>
// The case file is little-endian binary: eight int64 {n_cams, n_pts, n_obs, free_bytes, have_mem_info, iterative, lda, 0},
// then obs_cam and obs_pt as int32[n_obs].  The features are made here: observation i is at (i + 0.25, -i - 0.5).
// Every array of the plan goes to <output directory>/<name>.bin as raw little-endian binary; one JSON object on stdout has the
// return code, the refusal message, the scalars, and per array its element count and the 64-bit FNV-1a digest of its bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../slam-tricks_amd/csrc/schur_plan.hpp"

static unsigned long long fnv1a(const void* p, size_t bytes) {
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* q = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < bytes; ++k) { h ^= q[k]; h *= 1099511628211ull; }
    return h;
}

static std::string g_dir;
static bool g_first = true;

template <class T>
static void emit(const char* name, const T* data, size_t count) {
    const std::string path = g_dir + "/" + name + ".bin";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || (count > 0 && fwrite(data, sizeof(T), count, f) != count)) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
    printf("%s\"%s\": [%zu, \"%016llx\"]", g_first ? "" : ", ", name, count, fnv1a(data, count * sizeof(T)));
    g_first = false;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <case file> <output directory>\n", argv[0]); return 2; }
    g_dir = argv[2];
    FILE* f = fopen(argv[1], "rb");
    int64_t h[8];
    if (!f || fread(h, sizeof(int64_t), 8, f) != 8) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int n_cams = (int)h[0], n_pts = (int)h[1], n_obs = (int)h[2];
    std::vector<int> obs_cam((size_t)n_obs), obs_pt((size_t)n_obs);
    if (fread(obs_cam.data(), sizeof(int), (size_t)n_obs, f) != (size_t)n_obs || fread(obs_pt.data(), sizeof(int), (size_t)n_obs, f) != (size_t)n_obs) {
        fprintf(stderr, "%s is short\n", argv[1]);
        return 2;
    }
    fclose(f);
    std::vector<double> obs_feat((size_t)n_obs * 2);
    for (int i = 0; i < n_obs; ++i) { obs_feat[2 * (size_t)i] = i + 0.25; obs_feat[2 * (size_t)i + 1] = -i - 0.5; }
    stba::SchurPlanOptions opt;
    opt.free_bytes = (size_t)h[3]; opt.have_mem_info = h[4] != 0; opt.iterative = h[5] != 0; opt.lda = (int)h[6];
    stba::SchurPlan P;
    std::string why;
    const int rc = stba::build_schur_plan(n_cams, n_pts, n_obs, obs_cam.data(), obs_pt.data(), obs_feat.data(), opt, &P, &why);
    printf("{\"rc\": %d, \"why\": \"%s\"", rc, why.c_str());          // (the messages hold no quote and no backslash)
    if (rc == 0) {
        printf(", \"scalars\": {\"n_chunks\": %zu, \"n_dup\": %zu, \"total_pairs\": %zu, \"n_tasks\": %d, \"max_cols\": %d, \"lm_slices\": %d, "
               "\"schur_mode\": %d, \"dup_overflow\": %d, \"have_pair_plan\": %d, \"plan_mode\": %d, \"pairs\": %zu, \"lds_atomics\": %.17g, "
               "\"part_doubles\": %zu}, \"digests\": {",
               P.chunk_begin.size(), P.n_dup, P.total_pairs, P.n_tasks, P.max_cols, (int)P.lm_slices, P.schur_mode, (int)P.dup_overflow,
               (int)P.have_pair_plan, P.plan_mode, P.pairs, P.lds_atomics, P.part_doubles);
#define V_(v) emit(#v, P.v.data(), P.v.size())
        V_(perm); V_(s_cam); V_(s_pt); V_(s_feat); V_(pt_start); V_(cam_start); V_(cam_perm); V_(chunk_begin); V_(chunk_end);
        V_(cam_chunk_start); V_(dup_run); V_(row_col_ptr); V_(row_cols); V_(task_cam); V_(task_col_lo); V_(task_col_hi); V_(task_p_lo);
        V_(task_p_hi); V_(pair_begin); V_(pair_end); V_(task_vs_ptr); V_(vs_first); V_(task_part_off); V_(row_task_ptr); V_(row_tasks);
#undef V_
        emit("pair_rec", P.pair_rec.get(), P.pairs);
        printf("}");
    }
    printf("}\n");
    return 0;
}
