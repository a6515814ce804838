// schur_plan.hpp -- the host-side plan of the bundle-adjustment engine's reduced-system build: the landmark-major regrouping of the
// observations, the camera-side permutation and its chunks, the choice between the pair plan and the dense form of the Schur
// complement, the block pattern of S, the cut of its camera rows into tasks, and every task's per-wave pair records.
// Host only: the standard library and nothing of HIP, so that a plain C++ compiler builds it and tests/test_schur_plan_cpu.py
// checks it without a device.  stba_engine.hip (ba_fill) calls build_schur_plan and uploads what it returns; the kernels
// that read the plan are in ba_kernels.hip.
#pragma once
#include <algorithm>
#include <cstddef>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace stba {

constexpr int CAM_CHUNK = 256;                 // observations per camera-side reduction chunk
// SCHUR_SPLIT_COLS: non-zero blocks one task accumulates in LDS (two workgroups per CU);
// SCHUR_TASK_PAIRS: most (i, l) observation pairs per task (unlimited: smaller tasks measured slower).
constexpr int SCHUR_PLAN_DEFAULT = 3;                       // SchurArgs::mode of the product build
constexpr int SCHUR_MAX_SLOTS = 256;                        // LDS accumulator slots of a task: two workgroups of 81.5 KB per CU
constexpr int SCHUR_SPLIT_COLS = SCHUR_MAX_SLOTS - 8;       // blocks per task; a heavy block takes up to one extra slot per wave (parts)
constexpr int SCHUR_TASK_PAIRS = 1 << 30;
constexpr int SCHUR_THREADS = 512;    // 8 waves per task, two tasks per CU: 16 waves hide the L2 gathers

// form of the Schur complement the plan was made for: the values of STBA_SCHUR_PAIRS and STBA_SCHUR_DENSE (include/stba.h)
enum { SCHUR_FORM_PAIRS = 1, SCHUR_FORM_DENSE = 2 };

// host-side plan construction runs on a few threads (the camera rows / Schur tasks are independent)
template <typename F>
static void host_parallel_for(int n, F fn) {
    const int nt = std::max(1, std::min({16, (int)std::thread::hardware_concurrency(), n / 64}));
    if (nt <= 1) { fn(0, n, 0); return; }
    std::vector<std::thread> th;
    for (int k = 0; k < nt; ++k) th.emplace_back([=] { fn((int)((long)n * k / nt), (int)((long)n * (k + 1) / nt), k); });
    for (auto& t : th) t.join();
}

// one pair record of a task, as the Schur kernel reads it (an int4 on the device): observation i of the task's camera, observation
// l of the same landmark with camera(l) <= camera(i), the landmark, and accumulator slot | 0x8000 if diagonal block | rotation << 16
struct PairRec { int i, l, landmark, slot_flags; };

struct SchurPlanOptions {
    bool iterative = false;                      // ITERATIVE_SCHUR: no reduced system, so no block pattern and no plan
    size_t free_bytes = 0;                       // free device memory (hipMemGetInfo) ...
    bool have_mem_info = false;                  // ... if the runtime could tell
    int lda = 0;                                 // padded dimension of S (rows of the dense form's Y)
    // debug knobs (environment variables of a debug build, read by the caller; tools/dbg/schur_modes.py): the defaults are the product's
    int task_pairs = SCHUR_TASK_PAIRS;           // STBA_SCHUR_TASK_PAIRS
    int plan_knob = SCHUR_PLAN_DEFAULT;          // STBA_SCHUR_PLAN
    bool plan_runs = true;                       // STBA_SCHUR_RUNS
    bool rot_by_rank = true;                     // STBA_SCHUR_ROT_RANK
    bool lm_slices_allowed = true;               // STBA_SCHUR_LM_SLICES
    std::function<void(const char*)> phase;      // called with its label behind every phase (STBA_CREATE_TIMING); may be empty
};

struct SchurPlan {
    // the observations regrouped landmark-major: perm[sorted position] = the caller's observation index
    std::vector<int> perm, s_cam, s_pt;
    std::vector<double> s_feat;
    std::vector<int> pt_start, cam_start, cam_perm;              // a landmark's range of the sorted list; a camera's range of cam_perm
    std::vector<int> chunk_begin, chunk_end, cam_chunk_start;    // chunks of <= CAM_CHUNK observations of one camera
    std::vector<unsigned char> dup_run;                          // repeated (camera, landmark) pairs, per position of cam_perm (empty: none)
    size_t n_dup = 0, total_pairs = 0;                           // observations behind the first of their pair; sum over landmarks of k (k + 1) / 2
    // block pattern of S (lower triangle, by camera row) and the tasks
    std::vector<int> row_col_ptr, row_cols, task_cam, task_col_lo, task_col_hi, task_p_lo, task_p_hi;
    std::vector<size_t> task_pairs;
    std::vector<std::vector<int>> cnt_of;       // per camera row: pairs of every non-zero block (without the pairs (i, i))
    // pair records: per (task, wave) a range of pair_rec; per task the first accumulator slot of every block of its slice (+ the slot count)
    std::vector<int> pair_begin, pair_end, task_vs_ptr, vs_first;
    // (not a std::vector: its resize() would write 72 MB of zeros at C5, on one thread, in front of the threads that fill it)
    std::unique_ptr<PairRec[]> pair_rec;
    // landmark-range slices (plan_slice_bookkeeping)
    std::vector<long long> task_part_off;
    std::vector<int> row_task_ptr, row_tasks;
    size_t part_doubles = 0;
    int n_tasks = 0, max_cols = 0;              // max_cols: accumulator slots of the largest task (blocks + extra parts)
    bool lm_slices = false;
    int schur_mode = SCHUR_FORM_PAIRS;
    bool dup_overflow = false;                  // some pair has more than 255 observations: the DENSE form cannot take this problem
    bool have_pair_plan = false;
    int plan_mode = 0;                          // SchurArgs::mode the plan was built for
    size_t pairs = 0;                           // pair records
    double lds_atomics = 0.0;                   // LDS atomics of one launch of the Schur kernel (measurement)
};

// ---- landmark-major regrouping (stable counting sort) and the camera-side permutation
inline void plan_regroup(int n_cams, int n_pts, int n_obs, const int* obs_cam, const int* obs_pt, const double* obs_feat, SchurPlan& P) {
    P.pt_start.assign(n_pts + 1, 0);
    for (int i = 0; i < n_obs; ++i) ++P.pt_start[obs_pt[i] + 1];
    for (int j = 0; j < n_pts; ++j) P.pt_start[j + 1] += P.pt_start[j];
    P.perm.resize(n_obs);
    {
        std::vector<int> fill(P.pt_start.begin(), P.pt_start.end() - 1);
        for (int i = 0; i < n_obs; ++i) P.perm[fill[obs_pt[i]]++] = i;
    }
    P.s_cam.resize(n_obs); P.s_pt.resize(n_obs);
    P.s_feat.resize((size_t)n_obs * 2);
    for (int p = 0; p < n_obs; ++p) {
        const int i = P.perm[p];
        P.s_cam[p] = obs_cam[i]; P.s_pt[p] = obs_pt[i];
        P.s_feat[2 * (size_t)p] = obs_feat[2 * (size_t)i]; P.s_feat[2 * (size_t)p + 1] = obs_feat[2 * (size_t)i + 1];
    }
    P.cam_start.assign(n_cams + 1, 0);
    for (int p = 0; p < n_obs; ++p) ++P.cam_start[P.s_cam[p] + 1];
    for (int c = 0; c < n_cams; ++c) P.cam_start[c + 1] += P.cam_start[c];
    P.cam_perm.resize(n_obs);
    {
        std::vector<int> fill(P.cam_start.begin(), P.cam_start.end() - 1);
        for (int p = 0; p < n_obs; ++p) P.cam_perm[fill[P.s_cam[p]]++] = p;
    }
    P.cam_chunk_start.assign(n_cams + 1, 0);
    for (int c = 0; c < n_cams; ++c) {
        P.cam_chunk_start[c] = (int)P.chunk_begin.size();
        for (int s0 = P.cam_start[c]; s0 < P.cam_start[c + 1]; s0 += CAM_CHUNK) {
            P.chunk_begin.push_back(s0);
            P.chunk_end.push_back(std::min(s0 + CAM_CHUNK, P.cam_start[c + 1]));
        }
    }
    P.cam_chunk_start[n_cams] = (int)P.chunk_begin.size();
    // Several observations of one (camera, landmark) pair -- stereo residuals on one pose block, two factors on one pair through the
    // host-linearised path: in a camera's list (landmarks ascending) they are neighbours.  The pair plan treats them like any other
    // pair of observations; the dense form writes ONE block of Y per (camera, landmark) and must sum them (ba_schur_dense_chunk_kernel).
    for (int c = 0; c < n_cams; ++c)
        for (int q = P.cam_start[c]; q < P.cam_start[c + 1];) {
            int e = q + 1;
            while (e < P.cam_start[c + 1] && P.s_pt[P.cam_perm[e]] == P.s_pt[P.cam_perm[q]]) ++e;
            if (e - q > 1) {
                // (the run table is one byte per observation and only the DENSE form reads it: a longer run is refused where that form
                // is chosen, not here -- the pair plan handles any number of observations of one pair; advisor, round 5)
                if (e - q > 255) P.dup_overflow = true;
                if (P.dup_run.empty()) P.dup_run.assign((size_t)n_obs, 0);
                P.dup_run[(size_t)q] = (unsigned char)std::min(254, e - q - 1);
                for (int k = q + 1; k < e; ++k) P.dup_run[(size_t)k] = 255;
                P.n_dup += (size_t)(e - q - 1);
            }
            q = e;
        }
}

// ---- the form of the Schur complement: the pair plan, or the dense product where the plan cannot be held or the product is faster
inline int plan_choose_form(int n_cams, int n_pts, int n_obs, const SchurPlanOptions& opts, SchurPlan& P, std::string* why) {
    for (int j = 0; j < n_pts; ++j) { const size_t k = (size_t)(P.pt_start[j + 1] - P.pt_start[j]); P.total_pairs += k * (k + 1) / 2; }
    if (!opts.iterative) {   // the plan costs 16 bytes per pair on the host and on the device: refuse what cannot be held instead of running out of memory
        // half-way (a landmark seen by k cameras makes k (k + 1) / 2 pairs: 1000 cameras that ALL see 100 000 landmarks are 5e10)
        const size_t free_b = opts.free_bytes;
        const bool have_info = opts.have_mem_info;
        const size_t cap = std::min<size_t>((size_t)1 << 30, have_info ? free_b / 2 / 16 : ((size_t)1 << 30));
        // dense visibility: the Schur complement as one symmetric product on the matrix cores instead (ba_kernels.hip): no plan
        const double visibility = (n_pts > 0 && n_cams > 0) ? (double)((size_t)n_obs - P.n_dup) / ((double)n_pts * n_cams) : 0.0;   // (distinct pairs)
        const size_t y_bytes = (size_t)opts.lda * (((size_t)3 * n_pts + 31) / 16 * 16) * sizeof(double);
        const bool y_fits = !have_info || y_bytes < free_b / 2;
        if (P.total_pairs > cap && !y_fits) {
            *why = "stba_ba_create: " + std::to_string(P.total_pairs) + " observation pairs (sum over landmarks of k (k + 1) / 2, "
                   "k = cameras that see the landmark) need a Schur plan of " + std::to_string(P.total_pairs * 16 / (1 << 20)) + " MiB; the limit here is " +
                   std::to_string(cap) + " pairs (2^30, or half of the free device memory) -- and the dense form needs " +
                   std::to_string(y_bytes / (1 << 20)) + " MiB, which the device does not have free either";
            return 1;
        }
        // (measured, tools/dense_schur_time.py, 59 % visibility: 29 x 600 -- 94 k pairs -- 0.053 ms either way; 60 x 12 000 -- 7.8 M pairs --
        // 1.30 ms by the plan, 0.30 ms as a product; 100 x 8000 -- 14 M -- 1.53 against 0.37 ms)
        if (P.total_pairs > cap || (P.total_pairs > ((size_t)1 << 20) && visibility >= 0.3 && y_fits)) P.schur_mode = SCHUR_FORM_DENSE;
    }
    if (P.schur_mode == SCHUR_FORM_DENSE && P.dup_overflow) {
        *why = "stba_ba_create: more than 255 observations of one (camera, landmark) pair in a problem that needs the dense form of the Schur complement";
        return 1;
    }
    P.have_pair_plan = !opts.iterative && P.schur_mode != SCHUR_FORM_DENSE;
    return 0;
}

// ---- the block pattern of S and the pairs of every block, row by row
inline void plan_block_pattern(int n_cams, SchurPlan& P, std::vector<std::vector<int>>& cols_of) {
    cols_of.assign((size_t)n_cams, std::vector<int>());
    P.cnt_of.assign((size_t)n_cams, std::vector<int>());
    host_parallel_for(n_cams, [&](int c_lo, int c_hi, int) {
        std::vector<int> stamp(n_cams, -1), slot_of((size_t)n_cams, 0);
        for (int c = c_lo; c < c_hi; ++c) {
            std::vector<int>& tmp = cols_of[(size_t)c];
            for (int p = P.cam_start[c]; p < P.cam_start[c + 1]; ++p) {
                const int j = P.s_pt[P.cam_perm[p]];
                for (int l = P.pt_start[j]; l < P.pt_start[j + 1]; ++l) {
                    const int c2 = P.s_cam[l];
                    if (c2 <= c && stamp[c2] != c) { stamp[c2] = c; tmp.push_back(c2); }
                }
            }
            std::sort(tmp.begin(), tmp.end());
            for (size_t q = 0; q < tmp.size(); ++q) slot_of[(size_t)tmp[q]] = (int)q;
            std::vector<int>& cnt = P.cnt_of[(size_t)c];
            cnt.assign(tmp.size(), 0);
            for (int p = P.cam_start[c]; p < P.cam_start[c + 1]; ++p) {
                const int j = P.s_pt[P.cam_perm[p]];
                for (int l = P.pt_start[j]; l < P.pt_start[j + 1]; ++l)
                    if (P.s_cam[l] <= c && l != P.cam_perm[p]) ++cnt[(size_t)slot_of[(size_t)P.s_cam[l]]];     // (not the pair (i, i): below)
            }
        }
    });
}

// The three ways to cut the camera rows into tasks (chosen in plan_rows, where the reasons and the measurements are).
// By landmark range: a task = (row, a contiguous range of the camera's observation list, all columns)
inline void plan_cut_rows_by_landmark_range(int n_cams, const std::vector<std::vector<int>>& cols_of, SchurPlan& P) {
    const size_t cap = std::max<size_t>(8192, P.total_pairs / 1024 + 1);
    for (int c = 0; c < n_cams; ++c) {
        const std::vector<int>& tmp = cols_of[(size_t)c];
        P.row_cols.insert(P.row_cols.end(), tmp.begin(), tmp.end());
        P.row_col_ptr[c + 1] = (int)P.row_cols.size();
        const int ncols_c = (int)tmp.size();
        P.max_cols = std::max(P.max_cols, ncols_c);
        // pairs behind every observation of the camera's list: partners l of the same landmark with camera(l) <= c, l != i
        const int p0 = P.cam_start[c], p1 = P.cam_start[c + 1];
        size_t row_pairs = 0;
        for (int q : P.cnt_of[(size_t)c]) row_pairs += (size_t)q;
        const int n_sl = (int)std::min<size_t>(64, std::max<size_t>(1, (row_pairs + cap - 1) / cap));
        const size_t per = (row_pairs + (size_t)n_sl - 1) / (size_t)n_sl;
        int lo = p0, made = 0;
        size_t acc = 0;
        auto push = [&](int hi) {
            P.task_cam.push_back(c); P.task_col_lo.push_back(0); P.task_col_hi.push_back(ncols_c);
            P.task_p_lo.push_back(lo); P.task_p_hi.push_back(hi); P.task_pairs.push_back(acc);
            ++made; lo = hi; acc = 0;
        };
        for (int p = p0; p < p1; ++p) {
            const int i = P.cam_perm[p];
            const int j = P.s_pt[i];
            size_t w = 0;
            for (int l = P.pt_start[j]; l < P.pt_start[j + 1]; ++l) if (P.s_cam[l] <= c && l != i) ++w;
            if (acc > 0 && acc + w > per && made < n_sl - 1) push(p);
            acc += w;
        }
        push(p1);          // (the last slice; a camera without observations gets one empty task)
    }
}

// By columns: a task = (row, a slice of the row's column list) of at most SCHUR_SPLIT_COLS blocks and row_cap pairs
inline void plan_cut_rows_by_columns(int n_cams, const std::vector<std::vector<int>>& cols_of, size_t row_cap, SchurPlan& P) {
    for (int c = 0; c < n_cams; ++c) {
        const std::vector<int>& tmp = cols_of[(size_t)c];
        const std::vector<int>& cnt = P.cnt_of[(size_t)c];
        P.row_cols.insert(P.row_cols.end(), tmp.begin(), tmp.end());
        P.row_col_ptr[c + 1] = (int)P.row_cols.size();
        const int ncols_c = (int)tmp.size();
        int lo = 0;
        size_t acc = 0;
        for (int q = 0; q <= ncols_c; ++q) {
            // close the slice in front of column q when it is full, and at the end of the row (a camera without
            // observations still gets one empty task: it zeroes its rows and writes its zero camera block)
            const bool end = q == ncols_c;
            const bool full = !end && q > lo && (acc + (size_t)cnt[(size_t)q] > row_cap || q - lo >= SCHUR_SPLIT_COLS);
            if (full || end) {
                P.task_cam.push_back(c); P.task_col_lo.push_back(lo); P.task_col_hi.push_back(q); P.task_pairs.push_back(acc);
                P.max_cols = std::max(P.max_cols, q - lo);
                lo = q; acc = 0;
            }
            if (!end) acc += (size_t)cnt[(size_t)q];
        }
    }
}

// Two slices: by columns, with a cap on the pairs that cuts most rows in two
inline void plan_cut_rows_in_two_slices(int n_cams, const std::vector<std::vector<int>>& cols_of, SchurPlan& P) {
    // (ONE cap for all rows, 0.58 of the mean pairs per row: most rows fall into two slices, a heavy row into three, and no task is
    // longer than the cap -- the kernel ends with its longest task.  450 k pairs per row: 4.7 ms against 5.5 for equal halves of
    // every row and 6.5 for 58 / 42 of every row; 56 k per row -- one rank's share at eight ranks -- 0.48 ms against 1.30 uncut)
    plan_cut_rows_by_columns(n_cams, cols_of, std::max<size_t>(4096, (size_t)(0.58 * (double)P.total_pairs / (double)n_cams) + 1), P);
}

inline void plan_order_tasks(SchurPlan& P) {
    // Task order: heaviest first (most pairs), for a short tail.  (Measured against it in round 3, C5, Schur kernel
    // 0.324 ms: the cameras in trajectory order 0.39 ms; cut into eight contiguous ranges walked by one XCD each, so that
    // the workgroups side by side on an XCD gather the same records, 0.39-0.40 ms in camera order and 0.323 ms heaviest
    // first inside every range: the L2 hits bring nothing.  Slices cut to 3072 / 4096 / 6144 / 8192 pairs: 0.49 / 0.37 / 0.34 / 0.34 ms: a task's fixed costs --
    // zeroing its accumulator and its rows, the block stores -- outweigh the better balance.)
    std::vector<int> order(P.task_cam.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = (int)k;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return P.task_pairs[(size_t)x] > P.task_pairs[(size_t)y]; });
    auto permute = [&](auto& v) { auto t = v; for (size_t k = 0; k < order.size(); ++k) v[k] = t[(size_t)order[k]]; };
    permute(P.task_cam); permute(P.task_col_lo); permute(P.task_col_hi); permute(P.task_pairs);
    if (P.lm_slices) { permute(P.task_p_lo); permute(P.task_p_hi); }
}

// ---- row plan: the block pattern, the tasks and their order
inline void plan_rows(int n_cams, const SchurPlanOptions& opts, SchurPlan& P) {
    P.row_col_ptr.assign(n_cams + 1, 0);
    const int task_pairs = std::max(256, opts.task_pairs);
    if (opts.iterative) {
        // no reduced system at all: no block pattern either (row_col_ptr stays zero)
    } else if (!P.have_pair_plan) {
        // no plan: the block pattern (only the cross-rank packing reads it) is taken as full -- enumerating it costs as much as the pairs
        for (int c = 0; c < n_cams; ++c) {
            for (int c2 = 0; c2 <= c; ++c2) P.row_cols.push_back(c2);
            P.row_col_ptr[c + 1] = (int)P.row_cols.size();
        }
    } else {
        std::vector<std::vector<int>> cols_of;
        plan_block_pattern(n_cams, P, cols_of);
        // FEW camera rows (round 5; the landmark-heavy scenes, e.g. 100 cameras x 1 000 000 landmarks): a task per row leaves most of the
        // 512 workgroup slots empty, so the rows are cut into slices by pair count, about two per row -- measured on 100 x 1 000 000
        // (45 M pairs): one slice per row 10.8 ms, two 4.7, three 5.8, four 6.9 (every further slice walks the camera's observation
        // list once more and finds fewer of a landmark's pairs side by side); on one eighth of it 1.30 / 0.48 / 0.56 ms
        const bool two_slices = n_cams <= 256 && P.total_pairs > ((size_t)1 << 20) && task_pairs == SCHUR_TASK_PAIRS;
        // ROUND 6: with few camera rows whose blocks all fit ONE task's accumulator (<= SCHUR_SPLIT_COLS columns), a row is cut by
        // LANDMARK RANGE instead: a task = (row, a contiguous range of the camera's observation list, all columns).  Cutting by columns
        // (above) makes every slice gather the camera's own records again and finds fewer of a landmark's pairs side by side, so more
        // than ~two slices per row lost (4.7 / 5.8 / 6.9 ms at two / three / four); by landmark range a slice touches only its own
        // stretch of the list, any number of slices balances, and a thousand tasks fill the 512 workgroup slots twice over.  The
        // slices of a row write PARTIAL blocks (plus their share of the camera block, the gradient and the right-hand side); a
        // second, small kernel adds them in slice order -- no atomics on S, bitwise reproducible.
        bool lm_slices = two_slices && opts.lm_slices_allowed;
        for (int c = 0; c < n_cams && lm_slices; ++c) if ((int)cols_of[(size_t)c].size() > SCHUR_SPLIT_COLS) lm_slices = false;
        P.lm_slices = lm_slices;
        if (lm_slices) plan_cut_rows_by_landmark_range(n_cams, cols_of, P);
        else if (two_slices) plan_cut_rows_in_two_slices(n_cams, cols_of, P);
        else plan_cut_rows_by_columns(n_cams, cols_of, (size_t)task_pairs, P);
        plan_order_tasks(P);
    }
    P.n_tasks = (int)P.task_cam.size();
}

// ---- pair plan
inline void plan_pair_records(int n_cams, const SchurPlanOptions& opts, SchurPlan& P) {
    // Pair records (i, l, landmark, accumulator slot | flags) of every task.  RUN-TO-RUN REPRODUCIBILITY (round 5): every LDS
    // accumulator slot of a task is added to by ONE wave of the task's workgroup, so the ds_add_f64 that meet in an LDS address are
    // all issued by the same wave, in program order, and S comes out bit-identical from launch to launch (with the pairs dealt to
    // all 512 lanes in list order, as until round 4, the eight waves raced for the blocks and the sums differed in their last
    // bits: 34 distinct final costs in 48 long LM runs).
    // How the slots are dealt matters for speed.  A first version gave every 6 x 6 block to one wave (heaviest first): correct, and
    // 0.340 instead of 0.257 ms -- a wave's 64 lanes then hold pairs of 64 different landmarks (a landmark's partners are different
    // cameras, i.e. different blocks, i.e. different waves), so the own record J_i and the inverse landmark block are requested 64
    // times per instruction instead of ~12, and a wave that owns a heavy block adds to the same addresses in most of its lanes.
    // So: the camera's observation list (landmarks ascending) is cut into EIGHT RANGES of equal pair count, one per wave; a heavy
    // block gets up to eight PARTS -- accumulator slots of its own, consecutive, added in order when the block is written -- one per
    // range (or per two / four ranges), and part k goes to a wave of its ranges.  A wave's list is then, for the blocks that hold
    // most of the pairs, exactly the pairs of the landmarks of its range in the old order: the same coalescing and the same mix of
    // blocks per instruction as before.  Light blocks (one part) are dealt to the least loaded wave.
    constexpr int NW = SCHUR_THREADS / 64;
    // (debug builds: STBA_SCHUR_PLAN = 1: one list per task, the waves add in turn (token); 2: one list, arrival order -- the round-4 kernel)
    const int plan_knob = std::min(3, std::max(0, opts.plan_knob));
    const bool plan_stripes = plan_knob == 3;
    const bool plan_runs = opts.plan_runs, rot_by_rank = opts.rot_by_rank;
    const int plan_mode = plan_stripes ? 0 : plan_knob;
    P.plan_mode = plan_mode;
    std::vector<size_t> diag_pairs_thr(64, 0);
    int max_slots = 0;
    if (P.have_pair_plan) {
        const int ntask = (int)P.task_cam.size();
        P.pair_begin.resize((size_t)ntask * NW); P.pair_end.resize((size_t)ntask * NW);
        std::vector<size_t> cnt((size_t)ntask + 1, 0);
        P.task_vs_ptr.assign((size_t)ntask + 1, 0);
        for (int k = 0; k < ntask; ++k) {
            cnt[(size_t)k + 1] = cnt[(size_t)k] + P.task_pairs[(size_t)k];
            P.task_vs_ptr[(size_t)k + 1] = P.task_vs_ptr[(size_t)k] + (P.task_col_hi[(size_t)k] - P.task_col_lo[(size_t)k]) + 1;
        }
        P.pairs = cnt[(size_t)ntask];
        P.pair_rec.reset(new PairRec[std::max<size_t>(P.pairs, 1)]);
        P.vs_first.assign((size_t)P.task_vs_ptr[(size_t)ntask], 0);
        std::vector<int> max_slots_thr(64, 0);
        host_parallel_for(ntask, [&](int k_lo, int k_hi, int tix) {
            std::vector<int> slot_of((size_t)n_cams, 0);
            std::vector<int> nparts, wave_of, order, cntR, bcl, rank_of;
            std::vector<unsigned char> range_of;
            const bool lm = P.lm_slices;
            for (int k = k_lo; k < k_hi; ++k) {
                const int c = P.task_cam[(size_t)k];
                const int* cb = P.row_cols.data() + P.row_col_ptr[c];
                const int nco = P.row_col_ptr[c + 1] - P.row_col_ptr[c];
                for (int q = 0; q < nco; ++q) slot_of[(size_t)cb[q]] = q;
                const int slo = P.task_col_lo[(size_t)k], shi = P.task_col_hi[(size_t)k], ncols = shi - slo;
                const size_t total = P.task_pairs[(size_t)k];
                int* vsf = P.vs_first.data() + P.task_vs_ptr[(size_t)k];
                // ---- pass 1: the range of every observation of the camera (equal shares of THIS task's pairs), pairs per (block, range)
                // (a landmark-range slice walks its own stretch of the camera's list only)
                const int p0 = lm ? P.task_p_lo[(size_t)k] : P.cam_start[c], p1 = lm ? P.task_p_hi[(size_t)k] : P.cam_start[c + 1];
                range_of.assign((size_t)(p1 - p0), 0);
                cntR.assign((size_t)ncols * NW, 0);
                {
                    size_t before = 0;
                    for (int p = p0; p < p1; ++p) {
                        const int i = P.cam_perm[p];
                        const int j = P.s_pt[i];
                        // (plan 3: STRIPES -- the list dealt to the waves in runs of ~64 pairs, round robin, so that at any moment the eight
                        // waves work side by side in one stretch of the list as they did with the shared list)
                        const int w = plan_stripes ? (int)((before / 64) % NW) : total > 0 ? (int)std::min<size_t>(NW - 1, before * NW / total) : 0;
                        range_of[(size_t)(p - p0)] = (unsigned char)w;
                        for (int l = P.pt_start[j]; l < P.pt_start[j + 1]; ++l) {
                            const int c2 = P.s_cam[l];
                            if (c2 > c || l == i) continue;
                            const int sl = slot_of[(size_t)c2];
                            if (sl < slo || sl >= shi) continue;
                            ++cntR[(size_t)(sl - slo) * NW + w];
                            ++before;
                        }
                    }
                }
                // ---- parts per block.  A pair whose block has one part is handled by the block's wave whatever landmark it belongs to: its
                // own record and inverse landmark block are then requested by a lane of their own instead of by the handful of neighbouring
                // lanes that hold the same landmark's other pairs (~25 instead of ~12 cache lines per gather instruction).  With P parts the
                // share of such FOREIGN pairs of a block of m pairs is 1 - P / 8, so every accumulator slot spent on a block makes m / 8 of
                // its pairs local, whatever P: the blocks are upgraded heaviest first, to eight parts each, while slots last.
                // pairs per block of the slice (a landmark-range slice counts its own: the row's table covers the whole list)
                const int* bc = P.cnt_of[(size_t)c].data() + slo;
                if (lm) {
                    bcl.assign((size_t)ncols, 0);
                    for (int q = 0; q < ncols; ++q) for (int w2 = 0; w2 < NW; ++w2) bcl[(size_t)q] += cntR[(size_t)q * NW + w2];
                    bc = bcl.data();
                }
                nparts.assign((size_t)ncols, 1);
                int nvs = ncols;
                if (plan_mode == 0) {
                    order.resize((size_t)ncols);
                    for (int q = 0; q < ncols; ++q) order[(size_t)q] = q;
                    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return bc[x] > bc[y]; });
                    for (int q : order) {
                        if (bc[q] < 16) break;                              // (nothing to gain below a couple of pairs per wave)
                        const int np_ = (SCHUR_MAX_SLOTS - nvs >= 7) ? 8 : (SCHUR_MAX_SLOTS - nvs >= 3) ? 4 : (SCHUR_MAX_SLOTS - nvs >= 1) ? 2 : 1;
                        if (np_ == 1) break;
                        nparts[(size_t)q] = np_;
                        nvs += np_ - 1;
                    }
                }
                nvs = 0;
                for (int q = 0; q < ncols; ++q) { vsf[q] = nvs; nvs += nparts[(size_t)q]; }
                vsf[ncols] = nvs;
                max_slots_thr[(size_t)(tix & 63)] = std::max(max_slots_thr[(size_t)(tix & 63)], nvs);
                // ---- slots -> waves: a part goes to the least loaded wave among the ranges it covers; blocks heaviest first
                order.resize((size_t)ncols);
                for (int q = 0; q < ncols; ++q) order[(size_t)q] = q;
                std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return bc[x] > bc[y]; });
                size_t load[NW] = {0};
                wave_of.assign((size_t)nvs, 0);
                for (int q : order) {
                    const int np_ = nparts[(size_t)q], span = NW / np_;
                    if (np_ == 1 && plan_mode == 0 && plan_runs) continue;        // (light blocks: in column runs, below)
                    for (int part = 0; part < np_; ++part) {
                        size_t pc = 0;
                        for (int w = part * span; w < (part + 1) * span; ++w) pc += (size_t)cntR[(size_t)q * NW + w];
                        int best = part * span;
                        for (int w = part * span + 1; w < (part + 1) * span; ++w) if (load[w] < load[best]) best = w;
                        if (plan_mode != 0) best = 0;       // one list per task (the kernel's modes 1 and 2): everything in wave 0's range of the table
                        wave_of[(size_t)(vsf[q] + part)] = best;
                        load[best] += pc;
                    }
                }
                if (plan_mode == 0 && plan_runs) {
                    // Light blocks (one part) in RUNS of consecutive columns: the cameras next to each other in the column list see the same
                    // landmarks, so a landmark's pairs in light blocks mostly fall to one wave, side by side in its list -- and share the
                    // requests for the landmark's own record and inverse block again.  The runs fill the waves up to an equal share.
                    const size_t target = (total + NW - 1) / NW;
                    int cw = 0;
                    for (int q = 0; q < ncols; ++q) {
                        if (nparts[(size_t)q] != 1) continue;
                        while (cw < NW - 1 && load[cw] >= target) ++cw;
                        wave_of[(size_t)vsf[q]] = cw;
                        load[cw] += (size_t)bc[q];
                    }
                }
                size_t wpos[NW];
                {
                    size_t off = cnt[(size_t)k];
                    for (int w2 = 0; w2 < NW; ++w2) {
                        P.pair_begin[(size_t)k * NW + w2] = (int)off; wpos[w2] = off;
                        off += load[w2];
                        P.pair_end[(size_t)k * NW + w2] = (int)off;
                    }
                }
                // ---- pass 2: the records, every wave's list in landmark-major order
                for (int p = p0; p < p1; ++p) {
                    const int i = P.cam_perm[p];
                    const int j = P.s_pt[i];
                    const int w = range_of[(size_t)(p - p0)];
                    for (int l = P.pt_start[j]; l < P.pt_start[j + 1]; ++l) {
                        const int c2 = P.s_cam[l];
                        // (the pairs (i, i) -- an observation's own term of the diagonal block and of the right-hand side -- are
                        // made by the camera-block pass of the Schur kernel in registers, not here)
                        if (c2 > c || l == i) continue;
                        const int sl = slot_of[(size_t)c2];
                        if (sl < slo || sl >= shi) continue;
                        const int q = sl - slo;
                        const int v = vsf[q] + w / (NW / nparts[(size_t)q]);
                        P.pair_rec[wpos[wave_of[(size_t)v]]++] = PairRec{i, l, j, v | (c2 == c ? 0x8000 : 0)};
                        if (c2 == c) ++diag_pairs_thr[(size_t)(tix & 63)];
                    }
                }
                // ---- the COLUMN ROTATION of every pair (bits 16..18 of its fourth word).  The 64 pairs of one wave instruction that add
                // to the SAME block are served one after the other by ds_add_f64 unless they meet in different addresses: the kernel
                // lets a lane walk the six columns of its block starting at column `rotation`.  Round 6: the rotation is the pair's RANK
                // among the pairs of its trip that share its accumulator slot (mod 6) -- the host knows who meets whom.  Until then
                // it was lane mod 3, which does nothing where a landmark has 9 or 12 partners: the lanes that meet -- the same partner
                // camera, consecutive landmarks -- are then 9 or 12 lanes apart.
                rank_of.assign((size_t)nvs, 0);
                for (int w2 = 0; w2 < NW; ++w2) {
                    const size_t lb = (size_t)P.pair_begin[(size_t)k * NW + w2], le = (size_t)P.pair_end[(size_t)k * NW + w2];
                    for (size_t x0 = lb; x0 < le; x0 += 64) {
                        const size_t x1 = std::min(le, x0 + 64);
                        for (size_t x = x0; x < x1; ++x) {
                            const int v = P.pair_rec[x].slot_flags & 0x3fff;
                            const int rot = rot_by_rank ? rank_of[(size_t)v]++ % 6 : 2 * (int)((x - x0) % 3);
                            P.pair_rec[x].slot_flags |= rot << 16;
                        }
                        if (rot_by_rank) for (size_t x = x0; x < x1; ++x) rank_of[(size_t)(P.pair_rec[x].slot_flags & 0x3fff)] = 0;
                    }
                }
            }
        });
        for (int v : max_slots_thr) max_slots = std::max(max_slots, v);
    }
    P.max_cols = std::max(P.max_cols, max_slots);       // accumulator slots of the largest task (blocks + extra parts)
    // LDS atomics of one launch: 36 per pair (21 in a diagonal block)
    size_t n_diag = 0;
    for (size_t v : diag_pairs_thr) n_diag += v;
    P.lds_atomics = 36.0 * (double)(P.pairs - n_diag) + 21.0 * (double)n_diag;
}

// landmark-range slices: where every task writes its partial blocks, and every row's tasks in list order (the order of the sum)
inline void plan_slice_bookkeeping(int n_cams, SchurPlan& P) {
    if (P.lm_slices) {
        const int ntask = (int)P.task_cam.size();
        P.task_part_off.resize((size_t)ntask);
        for (int k = 0; k < ntask; ++k) {
            P.task_part_off[(size_t)k] = (long long)P.part_doubles;
            P.part_doubles += (size_t)(P.task_col_hi[(size_t)k] - P.task_col_lo[(size_t)k]) * 36 + 64;
        }
        std::vector<std::vector<std::pair<int, int>>> by_row((size_t)n_cams);
        for (int k = 0; k < ntask; ++k) by_row[(size_t)P.task_cam[(size_t)k]].push_back({P.task_p_lo[(size_t)k], k});
        P.row_task_ptr.assign((size_t)n_cams + 1, 0);
        for (int c = 0; c < n_cams; ++c) {
            std::sort(by_row[(size_t)c].begin(), by_row[(size_t)c].end());
            for (auto& pr : by_row[(size_t)c]) P.row_tasks.push_back(pr.second);
            P.row_task_ptr[(size_t)c + 1] = (int)P.row_tasks.size();
        }
    }
}

// The whole plan of one engine.  Returns non-zero, with the reason in *why, for a problem that is refused.
inline int build_schur_plan(int n_cams, int n_pts, int n_obs, const int* obs_cam, const int* obs_pt, const double* obs_feat,
                            const SchurPlanOptions& opts, SchurPlan* out, std::string* why) {
    SchurPlan& P = *out;
    auto phase = [&](const char* what) { if (opts.phase) opts.phase(what); };
    plan_regroup(n_cams, n_pts, n_obs, obs_cam, obs_pt, obs_feat, P);
    phase("regroup observations");
    // ---- Schur plan.  Camera row c of the reduced system has one non-zero 6x6 block per partner camera c2 <= c it shares a
    // landmark with; every (observation i of c, observation l of the same landmark with camera(l) <= c) PAIR contributes to
    // one of them.  A task = (camera row, a slice of the row's sorted column list): it owns its blocks alone (one writer per
    // block of S, no atomics on S, and the task zeroes its own stretch of the six matrix rows).  A slice holds at most
    // SCHUR_SPLIT_COLS blocks (the LDS accumulator: two workgroups per CU) and at most SCHUR_TASK_PAIRS pairs (no limit
    // by default: see the task order below).  The pairs of every task are enumerated here once (the structure is static).
    if (plan_choose_form(n_cams, n_pts, n_obs, opts, P, why) != 0) return 1;
    plan_rows(n_cams, opts, P);
    phase("row plan");
    plan_pair_records(n_cams, opts, P);
    plan_slice_bookkeeping(n_cams, P);
    phase("pair plan");
    return 0;
}

}  // namespace stba
