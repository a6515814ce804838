// Stand-alone driver of slam-tricks_amd/csrc/chol_schedule.hpp for tests/test_chol_schedule_cpu.py: no device, no HIP.
//   chol_schedule_driver lists <output prefix> <nblk> <queues> <workers> <nwide> [option=value ...]
//   chol_schedule_driver shard <nblk> <gpus> <xcds per gpu> <workers> <rows per group> <hop us> <tile us>
// lists: the ticket lists of one case go to <prefix>.tasks.bin (int32[ntasks][4]), <prefix>.lstart.bin (int32[queues + 1]) and
// <prefix>.start.bin (float32[ntasks], the simulated start times) as raw little-endian binary; one JSON object on stdout has the
// task count, the makespan's bit pattern and per array the 64-bit FNV-1a digest of its bytes.  The options are the fields of
// MegaScheduleOptions by name; what is not given keeps mega_default_options(nblk).
// shard: the three outputs of the multi-GPU what-if model, as bit patterns.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../slam-tricks_amd/csrc/chol_schedule.hpp"
using namespace stba;

static unsigned long long fnv1a(const void* p, size_t bytes) {
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* q = static_cast<const unsigned char*>(p);
    for (size_t k = 0; k < bytes; ++k) { h ^= q[k]; h *= 1099511628211ull; }
    return h;
}

static unsigned long long bits(double v) {
    unsigned long long u;
    memcpy(&u, &v, sizeof u);
    return u;
}

template <class T>
static void emit(const std::string& prefix, const char* name, const std::vector<T>& v, bool last) {
    const std::string path = prefix + "." + name + ".bin";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size())) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
    printf("\"%s\": \"%016llx\"%s", name, fnv1a(v.data(), v.size() * sizeof(T)), last ? "" : ", ");
}

static bool set_option(MegaScheduleOptions& o, const std::string& name, const char* val) {
#define I_(f) if (name == #f) { o.f = atoi(val); return true; }
#define D_(f) if (name == #f) { o.f = atof(val); return true; }
    I_(thalf_from) I_(tu10_from) I_(q_from) I_(dq_from) I_(qrows) I_(batch) I_(far_batch) I_(batch_lag)
    D_(thalf_dur) D_(tu10_dur) D_(dur_k) D_(blevel)
#undef I_
#undef D_
    if (name == "dur") return sscanf(val, "%lf,%lf,%lf,%lf,%lf,%lf", &o.dur[0], &o.dur[1], &o.dur[2], &o.dur[3], &o.dur[4], &o.dur[5]) == 6;
    return false;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "shard" && argc == 9) {
        MegaShardModel sh;
        MegaMachine m;
        const int nblk = atoi(argv[2]);
        sh.n_gpus = atoi(argv[3]);
        m.nq = sh.n_gpus * atoi(argv[4]); m.wg = atoi(argv[5]);
        sh.rows_per_group = atoi(argv[6]); sh.hop_us = atof(argv[7]); sh.tile_us = atof(argv[8]);
        MegaSchedule s;
        mega_build_tasks(s, nblk, 0, m, mega_default_options(nblk), &sh);
        printf("{\"shard\": [\"%016llx\", \"%016llx\", \"%016llx\"]}\n", bits(s.makespan_us), bits(sh.cross_edges), bits(sh.tiles_in_max));
        return 0;
    }
    if (mode != "lists" || argc < 7) { fprintf(stderr, "usage: %s lists <prefix> <nblk> <queues> <workers> <nwide> [option=value ...] | shard ...\n", argv[0]); return 2; }
    const std::string prefix = argv[2];
    const int nblk = atoi(argv[3]), nwide = atoi(argv[6]);
    MegaMachine m;
    m.nq = atoi(argv[4]); m.wg = atoi(argv[5]);
    MegaScheduleOptions opt = mega_default_options(nblk);
    for (int k = 7; k < argc; ++k) {
        const char* eq = strchr(argv[k], '=');
        if (!eq || !set_option(opt, std::string(argv[k], (size_t)(eq - argv[k])), eq + 1)) { fprintf(stderr, "bad option %s\n", argv[k]); return 2; }
    }
    MegaSchedule s;
    mega_build_tasks(s, nblk, nwide, m, opt);
    static_assert(sizeof(MegaTask) == 4 * sizeof(int32_t), "a task is four 32-bit words");
    printf("{\"ntasks\": %zu, \"makespan\": \"%016llx\", \"digests\": {", s.tasks.size(), bits(s.makespan_us));
    emit(prefix, "tasks", s.tasks, false);
    emit(prefix, "lstart", s.lstart, false);
    emit(prefix, "start", s.sim_start, true);
    printf("}}\n");
    return 0;
}
