// chol_schedule.hpp -- the host-built program of the persistent dense Cholesky (chol_mega_kernel, dense_chol.hip): the task
// descriptor, the layout of the device flags, and mega_build_tasks, which turns (block columns, machine) into one in-order
// ticket list per XCD.  Host only: the standard library, nothing of HIP and no environment, so that a plain C++ compiler builds
// it and tests/test_chol_schedule_cpu.py checks the lists without a device (tests/chol_schedule_ref.py replays them against
// the table below).  The descriptor's accessors and the flag layout are also what the kernel uses.
//
// THE PROTOCOL.  b: panel (block column), i / j: tile row / column, nrow = nblk + 4 nwide tile rows, of which the rows >= nblk
// are VIRTUAL: row nblk + p is the identity block under panel p of wide inverse block p / 4 (its tiles live in a buffer of their
// own, and only the panels p .. 4 (p / 4) + 3 touch it; first(i) = 0 for a real row, p for the virtual row nblk + p).
// Flags, all zero at the start, all only ever rising (agent-scope atomics):
//   dflag[b]          1 once diagonal block b is factored
//   tflag[b][i]       4 once rows of tile (i, b) are final: a whole panel solve adds 4, each of its two halves 2; for row b+1
//                     the four TU siblings that write X add 1 each; for the virtual row nblk + b, TI(b) adds 4
//   ver[i][j]         4 x (panels applied to tile (i, j)): a whole-tile update of nb panels adds 4 nb, a quarter update 1;
//                     ver[b+1][b+1] gets its 4 for panel b from the TU siblings (below)
//   tuflag[b]         `loaded`: TU siblings of panel b that hold their copy of block row b+1
//   tudone[b]         TU siblings (ten-block form) that have stored their part of tile (b+1, b+1)
// Per task {type | nb << 16, b, z, w} (nb: panels of a batched update, b its LAST one; 0 elsewhere):
//   type            z, w                 waits for                                              publishes
//   D(b)            0, 0                 ver[b][b] >= 4b                                        dflag[b] += 1
//   TI(b)           0, 0                 dflag[b] >= 1                                          tflag[b][nblk+b] += 4 if b < 4 nwide
//   T(b; i)         i, 0 whole           dflag[b] >= 1, ver[i][b] >= 4 (b - first(i))           tflag[b][i] += 4
//                   i, 1 | 2 half        the same                                               tflag[b][i] += 2
//   U(b; i, j)      i, j                 tflag[b][i] >= 4, tflag[b][j] >= 4,                    ver[i][j] += 4 max(1, nb)
//                                        ver[i][j] >= 4 (b - max(1, nb) + 1 - first(i))
//   Uq(b; i, r, j)  4 i + r, j           as U with nb = 1 (32 rows r of the tile)               ver[i][j] += 1
//   TU(b, q)        q, form              ver[b+1][b] >= 4b, ver[b+1][b+1] >= 4b; then INSIDE the task: dflag[b] >= 1,
//                                        tuflag[b] += 1 (its copy of the block row is loaded), its part of tile (b+1, b+1), then
//     form 2: four siblings q = 0..3     ver[b+1][b+1] += 1; waits for tuflag[b] >= 4, writes 32 rows of X;  tflag[b][b+1] += 1
//     form 1: diagonal block of ten      tudone[b] += 1, the LAST of the ten: ver[b+1][b+1] += 4; waits for tuflag[b] >= 10,
//                                        writes 32 rows of X;                                   tflag[b][b+1] += 1
//     form 0: off-diagonal block of ten  tudone[b] += 1, the last of the ten: ver[b+1][b+1] += 4;              nothing more
// At the end dflag = 1, ver[i][j] = 4 (j - first(i)) for every tile that exists, tflag[b][i] = 4 below the diagonal and on the
// span of every virtual row.  Because the version a whole-tile update waits for is the one its predecessor leaves, the panels
// reach a tile exactly once each and in panel order, whoever runs them: the factor is bit-reproducible.
// A workgroup holds ONE ticket of its XCD's list at a time and parks on it until its inputs are there.  What the lists must
// guarantee (and the test replays): with as many workgroups per list as the model had workers, some workgroup always holds a
// task whose inputs are complete (see mega_simulate); and all tasks that write one tile row sit in the list of the row's XCD,
// whose L2 is the only one that ever holds the tile while it changes.  (TI(p) sits in the list of row p and also writes the head
// tile of the virtual row nblk + p: final data, written once and by nobody else.)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <queue>
#include <utility>
#include <vector>

#ifdef __HIPCC__
#define CHOL_HD __host__ __device__ __forceinline__
#else
#define CHOL_HD inline
#endif

namespace stba {

// ---------------------------------------------------------------- the task descriptor
enum { TASK_D = 0, TASK_T = 1, TASK_TI = 2, TASK_U = 3, TASK_UQ = 4, TASK_TU = 5 };
constexpr int MEGA_NTU = 10;           // TU siblings of a panel in the ten-block form: workgroups a list needs resident at least

struct alignas(16) MegaTask { int x, y, z, w; };       // as int4: one 16-byte load in the kernel
// The fields of .x.  As expressions for the kernel's ticket loop: there a call, even one that is always inlined, is opaque to
// the first optimisation passes, and the persistent kernel's instruction stream shifts with what they see.  Everything else goes
// through the accessors below.
#define MEGA_X_TYPE(x) ((x) & 0xff)
#define MEGA_X_BATCH(x) (((x) >> 16) & 0xff)           // as stored: 0 for everything but a batched update
#define MEGA_X_PANELS(x) max(1, MEGA_X_BATCH(x))       // panels a task applies
CHOL_HD MegaTask mega_make_task(int type, int b, int z, int w, int nb = 0) { MegaTask t; t.x = type | nb << 16; t.y = b; t.z = z; t.w = w; return t; }
CHOL_HD int mega_task_type(const MegaTask& d) { return MEGA_X_TYPE(d.x); }
CHOL_HD int mega_task_panels(const MegaTask& d) { using std::max; return MEGA_X_PANELS(d.x); }
// .y: the panel (of a batch: the last one); .z / .w: per type, see the table above
// every task writes tiles of one tile row only (TU writes (b+1, b) and (b+1, b+1))
inline int mega_task_row(const MegaTask& tk) {
    switch (mega_task_type(tk)) {
        case TASK_D: case TASK_TI: return tk.y;
        case TASK_TU: return tk.y + 1;
        case TASK_T: case TASK_U: return tk.z;
        default: return tk.z >> 2;
    }
}

// ---------------------------------------------------------------- the flag arrays: offsets in ints from the start of the block
constexpr int MEGA_MAX_Q = 16;         // XCDs
constexpr int MEGA_ABORT = MEGA_MAX_Q;             // [0, MEGA_MAX_Q): the ticket counters of the lists; then the abort flag
constexpr int MEGA_SYNC_HDR = MEGA_MAX_Q + 1;
// P: the kernel lays the arrays out over its int* (and gets pointers), the host over the offset 0 (and gets offsets and the size)
template <class P>
struct MegaFlags {
    int nblk, nrow;                    // nrow = nblk + 4 nwide
    P abortf;
    P dflag, tuflag, tudone;           // [nblk] each
    P tflag;                           // [panel b][row i], i < nrow
    P ver;                             // [row i][panel j]
    P end;
};
template <class P>
CHOL_HD MegaFlags<P> mega_flag_layout(P base, int nblk, int nwide) {
    MegaFlags<P> v;
    v.nblk = nblk;
    v.nrow = nblk + 4 * nwide;
    v.abortf = base + MEGA_ABORT;
    v.dflag = base + MEGA_SYNC_HDR;
    v.tuflag = v.dflag + nblk;
    v.tudone = v.tuflag + nblk;
    v.tflag = v.tudone + nblk;
    v.ver = v.tflag + nblk * v.nrow;
    v.end = v.ver + v.nrow * nblk;
    return v;
}
inline size_t mega_flag_ints(int nblk, int nwide) { return mega_flag_layout<size_t>(0, nblk, nwide).end; }

// ---------------------------------------------------------------- who owns what
// A tile belongs to the XCD of its tile ROW.  Row i carries ~ i^2 / 2 trailing updates, so the rows are
// dealt out heaviest first, each to the XCD with the least work so far (LPT): the totals differ by < 1 %
// (a boustrophedon deal leaves 8 % between the heaviest XCD and the mean when nblk is not a multiple
// of 16, and the heaviest XCD sets the pace of the throughput-bound first half).
inline std::vector<int> mega_row_owner(int nblk, int nq, int nvirt = 0) {
    std::vector<int> owner((size_t)(nblk + nvirt), 0);
    for (int v = 0; v < nvirt; ++v) owner[(size_t)(nblk + v)] = v % nq;      // virtual rows (inverse blocks): a few light tasks each
    // (dealt boustrophedon or cyclically instead: measured 8 % worse)
    std::vector<double> load((size_t)nq, 0.0);
    for (int row = nblk - 1; row >= 0; --row) {
        int best = 0;
        for (int q = 1; q < nq; ++q)
            if (load[(size_t)q] < load[(size_t)best]) best = q;
        owner[(size_t)row] = best;
        load[(size_t)best] += 24.0 * row * (row - 1) / 2.0 + 23.0 * row + 110.0;
    }
    return owner;
}
struct MegaMachine {
    int nq = 8;                  // XCD queues
    int wg = 32;                 // model workers per queue: no more than the workgroups every XCD really has resident
};
// tile row -> GPU of the block-cyclic distribution of the sharded model: groups of `rows_per_group` consecutive rows in turn
inline int mega_shard_row_gpu(int row, int n_gpus, int rows_per_group) { return (row / std::max(1, rows_per_group)) % std::max(1, n_gpus); }
// What-if: the queues are spread over several GPUs (design study, DESIGN.md "sharded reduced solve").  A policy handed to the
// builder: it deals the tile rows its own way, and charges every dependency that crosses GPUs in the simulation.
struct MegaShardModel {
    int n_gpus = 1;              // queue q belongs to GPU q / (nq / n_gpus)
    int rows_per_group = 0;      // tile rows are dealt to the GPUs in groups of this many consecutive rows (0: one XCD-round, nq / n_gpus)
    double hop_us = 0.0;         // flag latency of a dependency that crosses GPUs
    double tile_us = 0.0;        // + transfer time of the 128 x 128 tile it carries (128 KiB over one xGMI link)
    double cross_edges = 0.0;    // out: dependencies that crossed GPUs
    double tiles_in_max = 0.0;   // out: distinct remote tiles fetched by the busiest GPU
    int q_per_gpu = 1;
    std::vector<double> tiles_in;

    int gpu_of(int q) const { return n_gpus > 1 ? q / q_per_gpu : 0; }
    // block-cyclic over the GPUs, cyclic over a GPU's XCDs: rows [g R, (g+1) R) of every round of n_gpus R rows go to GPU g
    void deal_rows(std::vector<int>& rowq, int nblk, int nq) {
        q_per_gpu = nq / std::max(1, n_gpus);
        tiles_in.assign((size_t)std::max(1, n_gpus), 0.0);
        if (n_gpus <= 1) return;
        const int R = rows_per_group > 0 ? rows_per_group : q_per_gpu;
        for (int row = 0; row < nblk; ++row) {
            const int local = (row / (R * n_gpus)) * R + row % R;        // index among the rows of its GPU
            rowq[(size_t)row] = mega_shard_row_gpu(row, n_gpus, R) * q_per_gpu + local % q_per_gpu;
        }
    }
    // delay of a dependency from a task of queue q0 to one of queue q1; sent_to: GPUs the producer's tile has been shipped to
    double edge_delay(int q0, int q1, unsigned& sent_to) {
        const int g0 = gpu_of(q0), g1 = gpu_of(q1);
        if (g1 == g0) return 0.0;
        cross_edges += 1.0;
        if (!(sent_to >> g1 & 1u)) { sent_to |= 1u << g1; tiles_in[(size_t)g1] += 1.0; }
        return hop_us + tile_us;
    }
    void finish() { tiles_in_max = *std::max_element(tiles_in.begin(), tiles_in.end()); }
};
// Far trailing updates are applied `batch` panels per pass over a tile (see mega_create_tasks).  The batch trades traffic for
// task length: a tile is read and written once per batch (round 4, PMC passes at n = 24 000 with two-panel batches: 383 GB per
// factorisation = 4 TB/s averaged over the kernel -- HBM-bound, 256 KB of operands + 128 KB of tile per panel and tile, no
// reuse of the operand panels in the L2s), but a batch of B panels is a task of ~6 + 18 B us that nothing can pre-empt.  Small
// systems are chain-bound and want short tasks (n = 6000: 2.294 / 2.295 / 2.344 ms with B = 2 / 3 / 4); large ones are
// throughput-bound (n = 12 000: 13.09 / 12.01 / 11.55 ms with B = 2 / 4 / 8; n = 24 000: 96.9 / 88.6 / 84.7 / 82.6 ms with
// B = 2 / 4 / 8 / 16, 0.61 -> 0.71 of the FP64 matrix-core peak).  Rule: double the batch while a batch round still
// leaves every workgroup a few tasks (nblk^2 / 2 tiles on 256 workgroups).
inline int mega_default_batch(int nblk) {
    const double tiles_per_wg = 0.5 * nblk * nblk / 256.0;
    int b = 2;
    while (b < 16 && tiles_per_wg / b >= 2.2) b *= 2;
    return b;
}

// ---------------------------------------------------------------- every threshold of the schedule
struct MegaScheduleOptions {
    // (The chains pace the last ~30 panels whatever the size: the trailing updates of panel nblk - r are r^2 / 2 tiles of ~24 us
    // on 256 workgroups, < 45 us for r < 31.  The *_from thresholds count from the END: measured at n = 6000 -- nblk = 47,
    // panels 17 / 32 / 30 -- and at n = 12 000, where fractions of nblk cost 2-3 %.)
    int thalf_from;      // first panel whose panel solves are two half tasks
    // the fused panel-solve + diagonal-tile update of a step: ten 2 x 2-tile block tasks from panel tu10_from on, four
    // quarter tasks (each solving the whole block row) before
    // (n = 6000, medians of interleaved runs on one box, tools/chol_ab.py: never 2.388 ms; from panel 18 / 26 / 28 / 32 / 36 / 40:
    // 2.373 / 2.357 / 2.364 / 2.351 / 2.365 / 2.382 -- while workgroups are scarce ten siblings wait for each other)
    int tu10_from;
    // from panel q_from on (the chain-bound part of the factorisation, where workgroups are idle) every row's tile in the next
    // panel column is updated by four quarter tasks: the row sweeps T -> U -> T get shorter
    int q_from;          // (panel 30 of 47; with the short TU tasks behind it: 2.351 -> 2.343 ms)
    int dq_from;         // quarter updates of the diagonal tile after next, see mega_create_tasks
    int qrows;           // before q_from: rows below the TU row whose tile in the next panel column is updated in quarters
    int batch;           // panels per pass of a far trailing update, 1 .. 64 (mega_default_batch)
    int far_batch;       // f > 0: a group of 2 batch panels whose last one is still more than f panels in front of its column goes in ONE pass
    int batch_lag;       // the last so many panels before a column's final one stay single tasks, >= 1 (round 3, with the shorter chain tasks: 3 -> 2: -0.02 ms; 1: the same)
    // measured on MI355X (tools/mega_trace.py), microseconds, plus ~2 us of flag latency per hop; by task type
    double dur[6];       // (D: 21.3 us since round 2)
    double dur_k;        // one more panel (K += 128) inside a batched trailing update (measured: 24 us for one panel, 42 for two)
    double thalf_dur;    // a half panel solve, as a fraction of dur[TASK_T]
    double tu10_dur;     // a TU block of the ten-block form, as a fraction of dur[TASK_TU]
    double blevel;       // weight of the bottom level in a task's priority (1: HLFET; 0: the column key alone)
};
inline MegaScheduleOptions mega_default_options(int nblk) {
    MegaScheduleOptions o;
    o.thalf_from = std::max(0, nblk - 30);
    o.tu10_from = std::max(0, nblk - 15);
    o.q_from = std::max(0, nblk - 17);
    o.dq_from = std::max(0, nblk - 17);
    o.qrows = 2;
    o.batch = mega_default_batch(nblk);
    o.far_batch = 0;
    o.batch_lag = 2;
    const double dur[6] = {23.0, 23.0, 19.0, 25.0, 16.5, 20.0};
    for (int k = 0; k < 6; ++k) o.dur[k] = dur[k];
    o.dur_k = 18.0;
    o.thalf_dur = 0.6;
    o.tu10_dur = 0.65;
    o.blevel = 1.0;
    return o;
}
// Options under which the lists are not a correct program are brought back into range, not obeyed.
inline MegaScheduleOptions mega_valid_options(MegaScheduleOptions o) {
    o.batch = std::min(64, std::max(1, o.batch));          // (the panel count of a batch, doubled by far_batch, has eight bits)
    o.far_batch = std::max(0, o.far_batch);
    // With no lag the last batch of column b+2 would end at panel b, the one whose update of the diagonal tile (b+2, b+2) is
    // cut into quarters: the quarters stand for panel b alone, the earlier panels of that batch would never reach the tile, and
    // TU(b+1) would wait for them for ever.  (Without a batch in front of it panel b is always a single task.)
    o.batch_lag = std::max(1, o.batch_lag);
    return o;
}

// ---------------------------------------------------------------- the builder
// The ticket order is produced by LIST SCHEDULING a model of the machine on the host: `wg` workers per XCD queue, measured
// task durations, and bottom-level priorities (longest path to the end of the graph, HLFET).  Sorting the tasks by the
// time their model worker became free gives (i) one global topological order, which the deadlock argument needs, and
// (ii) per-queue orders in which a workgroup rarely takes a ticket whose inputs are far from ready (an in-order ticket
// list has no other notion of priority).
// ORDER IS BEHAVIOUR: the order in which nodes are created and edges inserted decides the ties of both heaps of the simulation.
struct MegaNode { MegaTask tk; std::vector<int> succ; int indeg = 0; double dur = 0, prio = 0, start = 0, ready = 0, avail = 0; int q = 0; int last_pred = -1; };
struct MegaPick { double key, start; int node; };
struct MegaSchedule {
    // in
    int nblk = 0, nwide = 0;
    MegaMachine mach;
    MegaScheduleOptions opt;
    // the task graph.  Node ids by what they compute, -1: no such task
    std::vector<MegaNode> nodes;
    std::vector<int> rowq;                          // tile row (virtual ones included) -> queue
    std::vector<int> idD, idTI, idTU, idT, idT2;    // [b], [b], [b][sibling], [b][i] whole or upper half, [b][i] lower half
    std::vector<int> idUq;                          // [b][i][quarter]: the update of tile (i, b+1) by panel b (slot 0 alone: a whole-tile task)
    std::vector<int> idU;                           // [b][i][j], j >= b+2: the task that applies panel b to tile (i, j)
    std::vector<int> idUd;                          // [b][quarter]: the quartered update of the diagonal tile (b+2, b+2) by panel b
    std::vector<std::vector<MegaPick>> order;       // per queue: the simulation's picks
    // out
    std::vector<MegaTask> tasks;                    // the ticket lists, concatenated
    std::vector<int> lstart;                        // list q holds tasks [lstart[q], lstart[q+1])
    std::vector<float> sim_start;                   // simulated start time of every task
    double makespan_us = 0.0;

    int ntu(int b) const { return b >= opt.tu10_from ? MEGA_NTU : 4; }
    int add(int type, int b, int i, int j, double prio) {
        MegaNode nd; nd.tk = mega_make_task(type, b, i, j); nd.dur = opt.dur[type]; nd.prio = prio;
        nd.q = rowq[(size_t)mega_task_row(nd.tk)];
        nodes.push_back(nd);
        return (int)nodes.size() - 1;
    }
    void dep(int from, int to) {     // `to` needs `from`
        if (from < 0 || to < 0) return;
        nodes[(size_t)from].succ.push_back(to);
        nodes[(size_t)to].indeg++;
    }
};

// Step 1: the tasks of the real rows, panel by panel.
// priorities: smaller = sooner.  The key is the block column a task works towards (10 per column)
// plus a class offset, so that everything the NEXT panels need goes before trailing updates of far
// columns, whatever step they belong to (an in-step order would bury the update of tile (b+1, b+1)
// by panel b-1 behind the whole backlog of panel b-2).  (Replaced by the bottom level in step 4; kept as the tie-break.)
inline void mega_create_tasks(MegaSchedule& s, MegaShardModel* shard) {
    const int NBK = s.nblk;
    const MegaScheduleOptions& o = s.opt;
    s.rowq = mega_row_owner(NBK, s.mach.nq, 4 * s.nwide);
    if (shard) shard->deal_rows(s.rowq, NBK, s.mach.nq);
    s.idD.assign((size_t)NBK, -1); s.idTI.assign((size_t)NBK, -1); s.idTU.assign((size_t)NBK * MEGA_NTU, -1);
    s.idT.assign((size_t)NBK * NBK, -1); s.idT2.assign((size_t)NBK * NBK, -1);
    s.idUq.assign((size_t)NBK * NBK * 4, -1); s.idU.assign((size_t)NBK * NBK * NBK, -1); s.idUd.assign((size_t)NBK * 4, -1);
    std::vector<MegaNode>& nodes = s.nodes;
    for (int b = 0; b < NBK; ++b) {
        s.idD[(size_t)b] = s.add(TASK_D, b, 0, 0, 10.0 * b);
        s.idTI[(size_t)b] = s.add(TASK_TI, b, 0, 0, 10.0 * NBK + b);
        if (b + 1 < NBK)
            for (int q = 0; q < s.ntu(b); ++q) {        // (tk.w = 1: a diagonal block (I, I), which writes 32 rows of X; 2: the four-workgroup form)
                int I = 0;
                while ((I + 1) * (I + 2) / 2 <= q) ++I;
                const bool dg = (q == I * (I + 1) / 2 + I);
                s.idTU[(size_t)b * MEGA_NTU + q] = s.add(TASK_TU, b, q, s.ntu(b) == 4 ? 2 : dg ? 1 : 0, 10.0 * b + 5 + (s.ntu(b) != 4 && dg ? 1e-4 : 0.0));
                if (s.ntu(b) != 4) nodes[(size_t)s.idTU[(size_t)b * MEGA_NTU + q]].dur = o.tu10_dur * o.dur[TASK_TU];
            }
        for (int i = b + 2; i < NBK; ++i) {
            if (b >= o.thalf_from) {
                // two HALF tasks (64 rows each on four waves, see the kernel's TASK_T) once the chains pace the factorisation:
                // a panel solve is one of the two links of every row sweep T -> U -> T, and as a half it waits for 136 KB
                // instead of 200 and has a SIMD per wave -- 11 us instead of 18.4.  (Measured at n = 6000, same box: whole
                // tasks 2.509 ms; halves from panel 0 / 10 / 14 / 17 / 20 / 24: 2.493 / 2.445 / 2.425 / 2.425 / 2.431 / 2.427;
                // QUARTER tasks from 17 / 24: 2.517 / 2.472 -- the 72 KB of the diagonal factor every part stages do not shrink.)
                s.idT[(size_t)b * NBK + i] = s.add(TASK_T, b, i, 1, 10.0 * b + 6 + 1e-3 * i);
                s.idT2[(size_t)b * NBK + i] = s.add(TASK_T, b, i, 2, 10.0 * b + 6 + 1e-3 * i + 5e-4);
                nodes[(size_t)s.idT[(size_t)b * NBK + i]].dur = nodes[(size_t)s.idT2[(size_t)b * NBK + i]].dur = o.thalf_dur * o.dur[TASK_T];
            } else s.idT[(size_t)b * NBK + i] = s.add(TASK_T, b, i, 0, 10.0 * b + 6 + 1e-3 * i);
            // the next panel's column: 32-row tasks (short latency) only for the rows the second critical chain
            // needs soon; a quarter task costs 14.5 us of a workgroup against 23.4 us for a whole tile, so the
            // rows further down take the whole-tile task (their panel solve comes a diagonal block later)
            if (i <= b + 1 + o.qrows || b >= o.q_from) {
                for (int q = 0; q < 4; ++q)
                    s.idUq[((size_t)b * NBK + i) * 4 + q] = s.add(TASK_UQ, b, i * 4 + q, b + 1, 10.0 * (b + 1) + 2 + 1e-3 * i);
            } else {
                s.idUq[((size_t)b * NBK + i) * 4] = s.add(TASK_U, b, i, b + 1, 10.0 * (b + 1) + 2 + 1e-3 * i);
            }
        }
        // Trailing updates of the tiles beyond the next panel column.  Tile (i, j) needs the panels 0 .. j-2 at some point
        // before its last update (panel j-1, above: the latency-critical one); they are applied `batch` panels at a time in
        // one pass over the tile, K = 128 batch: the tile is read and written once per batch instead of once per panel and
        // the task's fixed costs (waiting for the first operands and the tile, the stores, the hand-over: ~10 of 24 us) are
        // paid once per batch.  The task of a batch carries its LAST panel in .y and the panel count in bits 16..23 of .x;
        // the MFMAs run on the same accumulators in the same order as panel-by-panel, so the result is bit-identical.
        for (int j = b + 2; j < NBK; ++j) {
            // panels 0 .. j-2 of column j in batches [0, batch), [batch, 2 batch), ...: this panel closes a batch if it
            // is the last of its group or the last one of the column
            // (the last batch_lag panels before the final one stay single tasks: a long batch there would sit on the path to
            // the tile's panel solve)
            const int lim = j - 2 - o.batch_lag;
            // (far batches: longer tasks only where the chains are far away)
            int BJ = o.batch;
            if (o.far_batch > 0 && o.batch > 1 && j - ((b / (2 * o.batch)) * 2 * o.batch + 2 * o.batch - 1) > o.far_batch) BJ = 2 * o.batch;
            const int b0 = (BJ <= 1 || b > lim) ? b : (b / BJ) * BJ, last = (BJ <= 1 || b > lim) ? b : std::min(b0 + BJ - 1, lim);
            if (b != last) continue;
            const int nb = b - b0 + 1;
            for (int i = j; i < NBK; ++i) {
                if (i == j && j == b + 2 && b >= o.dq_from) {
                    // The diagonal tile (b+2, b+2): its update by panel b is the last input of TU(b+1) to arrive in the
                    // chain-bound part -- D(b) -> half panel solve of row b+2 (12 us) -> this update (24 us as a whole-tile
                    // task) = 38 us against a step of 36 (trace: the last TU(b) block became ready 6 us AFTER D(b) every
                    // other panel).  Four quarter tasks (32 rows each, operands straight from memory: 14.6 us) instead.
                    // (panel b is a single task here, never the end of a batch: mega_valid_options)
                    for (int q = 0; q < 4; ++q) {
                        const int id = s.add(TASK_UQ, b, i * 4 + q, j, 10.0 * j + 1 + 1e-3 * q);
                        s.idUd[(size_t)b * 4 + q] = id;
                        if (q == 0) s.idU[((size_t)b * NBK + i) * NBK + j] = id;
                    }
                    continue;
                }
                const int id = s.add(TASK_U, b, i, j, 10.0 * j + 3 + 1e-3 * i + 1e-6 * b);
                nodes[(size_t)id].tk.x |= nb << 16;
                nodes[(size_t)id].dur += (nb - 1) * o.dur_k;
                for (int bb = b0; bb <= b; ++bb) s.idU[((size_t)bb * NBK + i) * NBK + j] = id;
            }
        }
    }
}

// Step 2: the dependencies between them, panel by panel.
inline void mega_add_dependencies(MegaSchedule& s) {
    const int NBK = s.nblk;
    const std::vector<MegaNode>& nodes = s.nodes;
    for (int b = 0; b < NBK; ++b) {
        const int d = s.idD[(size_t)b];
        if (b > 0)
            for (int q = 0; q < s.ntu(b - 1); ++q) s.dep(s.idTU[(size_t)(b - 1) * MEGA_NTU + q], d);
        s.dep(d, s.idTI[(size_t)b]);
        if (b + 1 < NBK)
            for (int q = 0; q < s.ntu(b); ++q) {
                const int tu = s.idTU[(size_t)b * MEGA_NTU + q];
                s.dep(d, tu);
                if (b > 0) {
                    for (int q2 = 0; q2 < 4; ++q2) s.dep(s.idUq[((size_t)(b - 1) * NBK + (b + 1)) * 4 + q2], tu);
                    s.dep(s.idU[((size_t)(b - 1) * NBK + (b + 1)) * NBK + (b + 1)], tu);
                    for (int q2 = 1; q2 < 4; ++q2) s.dep(s.idUd[(size_t)(b - 1) * 4 + q2], tu);     // (its quarters, if it was split)
                }
            }
        for (int i = b + 2; i < NBK; ++i) {
            const int t = s.idT[(size_t)b * NBK + i], t2 = s.idT2[(size_t)b * NBK + i];
            s.dep(d, t); s.dep(d, t2);
            if (b > 0)
                for (int q2 = 0; q2 < 4; ++q2) { const int uu = s.idUq[((size_t)(b - 1) * NBK + i) * 4 + q2]; s.dep(uu, t); s.dep(uu, t2); }
            for (int q = 0; q < 4; ++q) {
                const int uq = s.idUq[((size_t)b * NBK + i) * 4 + q];
                if (uq < 0) continue;            // (rows with ONE whole-tile task use slot 0 only)
                s.dep(t, uq); s.dep(t2, uq);
                for (int q2 = 0; q2 < s.ntu(b); ++q2) s.dep(s.idTU[(size_t)b * MEGA_NTU + q2], uq);
                if (b > 0) s.dep(s.idU[((size_t)(b - 1) * NBK + i) * NBK + (b + 1)], uq);
            }
        }
        for (int j = b + 2; j < NBK; ++j)
            for (int i = j; i < NBK; ++i) {
                const int u0 = s.idU[((size_t)b * NBK + i) * NBK + j];
                if (nodes[(size_t)u0].tk.y != b) continue;          // (a batch: its dependencies hang on its last panel)
                const bool split = mega_task_type(nodes[(size_t)u0].tk) == TASK_UQ;       // (the diagonal tile after next, in quarters)
                for (int q2 = 0; q2 < (split ? 4 : 1); ++q2) {
                    const int u = split ? s.idUd[(size_t)b * 4 + q2] : u0;
                    for (auto* v : {&s.idT, &s.idT2}) { s.dep((*v)[(size_t)b * NBK + i], u); if (j != i) s.dep((*v)[(size_t)b * NBK + j], u); }
                    const int nbp = split ? 1 : mega_task_panels(nodes[(size_t)u].tk);
                    if (b - nbp >= 0) s.dep(s.idU[((size_t)(b - nbp) * NBK + i) * NBK + j], u);
                }
            }
    }
}

// Step 3: the virtual rows.  Wide inverse blocks: the identity block under panel p = 4q + v of wide block q (virtual row
// nblk + p) is carried through panels p .. 4q+3: TI(p) makes its diagonal tile, then per later panel bj of the block the updates
// U(k; row, bj), k = p .. bj-1, and the panel solve T(bj; row)
inline void mega_add_virtual_rows(MegaSchedule& s) {
    const int NBK = s.nblk;
    for (int qw = 0; qw < s.nwide; ++qw)
        for (int v = 0; v < 4; ++v) {
            const int pnl = 4 * qw + v, iv = NBK + pnl;
            std::vector<int> xdone(4, -1);            // task that finishes tile (iv, 4qw + j)
            xdone[(size_t)v] = s.idTI[(size_t)pnl];
            for (int j = v + 1; j < 4; ++j) {
                const int bj = 4 * qw + j;
                int prev = -1;
                for (int k = pnl; k < bj; ++k) {
                    const int u = s.add(TASK_U, k, iv, bj, 10.0 * NBK + bj);
                    s.dep(xdone[(size_t)(k - 4 * qw)], u);
                    if (bj == k + 1) { for (int q2 = 0; q2 < s.ntu(k); ++q2) s.dep(s.idTU[(size_t)k * MEGA_NTU + q2], u); }
                    else for (auto* v2 : {&s.idT, &s.idT2}) s.dep((*v2)[(size_t)k * NBK + bj], u);
                    s.dep(prev, u);
                    prev = u;
                }
                const int tv = s.add(TASK_T, bj, iv, 0, 10.0 * NBK + bj);
                s.dep(s.idD[(size_t)bj], tv);
                s.dep(prev, tv);
                xdone[(size_t)j] = tv;
            }
        }
}

// Step 4: bottom level (longest path to the end of the graph) as the priority: HLFET list scheduling
inline void mega_bottom_levels(MegaSchedule& s) {
    const double BLW = s.opt.blevel;
    if (!(BLW > 0.0)) return;
    std::vector<MegaNode>& nodes = s.nodes;
    std::vector<int> indeg2(nodes.size()), topo;
    topo.reserve(nodes.size());
    for (size_t k = 0; k < nodes.size(); ++k) { indeg2[k] = nodes[k].indeg; if (indeg2[k] == 0) topo.push_back((int)k); }
    for (size_t h = 0; h < topo.size(); ++h)
        for (int sidx : nodes[(size_t)topo[h]].succ)
            if (--indeg2[(size_t)sidx] == 0) topo.push_back(sidx);
    std::vector<double> bl(nodes.size(), 0.0);
    for (size_t h = topo.size(); h-- > 0;) {
        const int k = topo[h];
        double m = 0.0;
        for (int sidx : nodes[(size_t)k].succ) m = std::max(m, bl[(size_t)sidx]);
        bl[(size_t)k] = nodes[(size_t)k].dur + m;
    }
    for (size_t k = 0; k < nodes.size(); ++k) nodes[k].prio = nodes[k].prio * (1.0 - BLW) * 5.0 - BLW * bl[k];
}

// Step 5: event-driven list scheduling.  A ticket list replays the model if the tickets are sorted by the time
// their worker became FREE (= the moment a workgroup picks its next ticket), not by the task's start:
// a workgroup that picks a ticket early parks on it until its inputs arrive.
// Liveness: a ticket occupies its model worker from pick to end, so at most W - 1 tickets that come later in the
// topological (start time) order can precede any ticket in its list, W = the list's model workers; with at least W
// real workgroups per list one of them always reaches the earliest unfinished task.  (The key must be the time the worker
// became free and nothing else: tickets moved up in their list by a constant break the bound.)
// The model is faithful (C5, one class: 2.55 ms predicted, 2.53-2.60 ms measured; tools/mega_trace.py prints the
// drift), which makes it the place to try policies -- tools/sim_sweep.py, no GPU.  Tried and rejected there AND on the
// machine in rounds 1-2 (and removed from the code since): workers reserved for the tasks of the critical chains,
// priority boosts for those rows, an urgent list per XCD claimed by whichever workgroup is free (a parked workgroup
// starts a critical task the moment its last flag flips; a claimed task pays 2-5 us per hand-over), the last update of
// a tile fused into the panel solve that consumes it.  DESIGN.md 4 has the numbers.
inline void mega_simulate(MegaSchedule& s, MegaShardModel* shard) {
    std::vector<MegaNode>& nodes = s.nodes;
    const int nl = s.mach.nq;                       // one ticket list per XCD queue
    typedef std::pair<double, int> PI;
    typedef std::priority_queue<PI, std::vector<PI>, std::greater<PI>> Heap;
    std::vector<Heap> ready_h((size_t)nl);
    Heap events;                                // (time, node) a task ends | (time, -(node + 1)) the last delayed input of a task arrives
    std::vector<std::vector<double>> idle_since((size_t)nl, std::vector<double>((size_t)s.mach.wg, 0.0));   // LIFO
    double now = 0.0;
    s.order.assign((size_t)nl, std::vector<MegaPick>());
    auto push_ready = [&](int k) { ready_h[(size_t)nodes[(size_t)k].q].push(PI(nodes[(size_t)k].prio, k)); };
    for (int k = 0; k < (int)nodes.size(); ++k)
        if (nodes[(size_t)k].indeg == 0) push_ready(k);
    double makespan = 0.0;
    for (;;) {
        for (int l = 0; l < nl; ++l) {
            std::vector<double>& idl = idle_since[(size_t)l];
            Heap& hb = ready_h[(size_t)l];
            while (!idl.empty() && !hb.empty()) {
                const int k = hb.top().second;
                hb.pop();
                MegaNode& nd = nodes[(size_t)k];
                s.order[(size_t)l].push_back({idl.back(), now, k});
                idl.pop_back();
                nd.start = now;
                events.push(PI(now + nd.dur, k));
            }
        }
        if (events.empty()) break;
        const PI ev = events.top();
        events.pop();
        now = ev.first;
        if (ev.second < 0) {                    // the last delayed input of a task has arrived (a dependency that crossed GPUs)
            const int k = -(ev.second + 1);
            nodes[(size_t)k].ready = now;
            push_ready(k);
            continue;
        }
        makespan = now;
        const MegaNode& nd = nodes[(size_t)ev.second];
        idle_since[(size_t)nd.q].push_back(now);
        unsigned sent_to = 0;                   // (sharded model) GPUs this task's output tile has been shipped to
        for (int sidx : nd.succ) {
            MegaNode& sn = nodes[(size_t)sidx];
            double at = now;
            if (shard) at += shard->edge_delay(nd.q, sn.q, sent_to);
            if (at > sn.avail) { sn.avail = at; sn.last_pred = ev.second; }
            if (--sn.indeg == 0) {
                if (sn.avail <= now) { sn.ready = now; push_ready(sidx); }
                else events.push(PI(sn.avail, -(sidx + 1)));
            }
        }
    }
    s.makespan_us = makespan;
    if (shard) shard->finish();
}

// Step 6: the lists, each queue's picks in the order its workers became free
inline void mega_emit_lists(MegaSchedule& s) {
    const int nl = s.mach.nq;
    s.tasks.clear();
    s.sim_start.clear();
    s.lstart.assign((size_t)nl + 1, 0);
    for (int l = 0; l < nl; ++l) {
        std::stable_sort(s.order[(size_t)l].begin(), s.order[(size_t)l].end(), [](const MegaPick& x, const MegaPick& y) {
            return x.key != y.key ? x.key < y.key : x.start < y.start;
        });
        s.lstart[(size_t)l] = (int)s.tasks.size();
        for (const MegaPick& pk : s.order[(size_t)l]) {
            s.tasks.push_back(s.nodes[(size_t)pk.node].tk);
            s.sim_start.push_back((float)pk.start);
        }
    }
    s.lstart[(size_t)nl] = (int)s.tasks.size();
}

// the task lists for nblk block columns (static per size): one global dataflow order, split into one queue per XCD by the
// owner of the tile row each task writes
inline void mega_build_tasks(MegaSchedule& s, int nblk, int nwide, const MegaMachine& mach, const MegaScheduleOptions& opt, MegaShardModel* shard = nullptr) {
    s = MegaSchedule();
    s.nblk = nblk; s.nwide = nwide; s.mach = mach; s.opt = mega_valid_options(opt);
    mega_create_tasks(s, shard);
    mega_add_dependencies(s);
    mega_add_virtual_rows(s);
    mega_bottom_levels(s);
    mega_simulate(s, shard);
    mega_emit_lists(s);
}

// debugging aid: per panel, when the last TU sibling and the next diagonal block became ready and started, relative to the end
// of the diagonal block, and the chain of last-arriving inputs behind the TU sibling
inline void mega_print_chains(const MegaSchedule& s, FILE* f) {
    static const char* NM[6] = {"D", "T", "TI", "U", "Uq", "TU"};
    const std::vector<MegaNode>& nodes = s.nodes;
    fprintf(f, "%d queues, %d workers each, makespan %.1f us\n", s.mach.nq, s.mach.wg, s.makespan_us);
    for (int b = 0; b + 1 < s.nblk; ++b) {
        const MegaNode& d0 = nodes[(size_t)s.idD[(size_t)b]];
        const MegaNode& d1 = nodes[(size_t)s.idD[(size_t)b + 1]];
        const MegaNode& tu = nodes[(size_t)s.idTU[(size_t)b * MEGA_NTU + s.ntu(b) - 1]];
        const double e0 = d0.start + d0.dur;
        fprintf(f, "b=%2d step %6.1f | TU ready %+6.1f start %+6.1f | D+1 ready %+6.1f start %+6.1f", b, d1.start - d0.start,
                tu.ready - e0, tu.start - e0, d1.ready - e0, d1.start - e0);
        int k = s.idTU[(size_t)b * MEGA_NTU + s.ntu(b) - 1];
        for (int hop = 0; hop < 4 && k >= 0; ++hop) {       // walk back along the last-arriving inputs
            const MegaNode& nd = nodes[(size_t)k];
            fprintf(f, " <- %s(%d;%d,%d) rdy %+.1f st %+.1f", NM[mega_task_type(nd.tk)], nd.tk.y, nd.tk.z, nd.tk.w, nd.ready - e0, nd.start - e0);
            k = nd.last_pred;
        }
        fprintf(f, "\n");
    }
}

}  // namespace stba
