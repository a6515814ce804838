"""The cases of tests/test_chol_schedule_cpu.py: which ticket lists tests/cpp/chol_schedule_driver.cpp builds, and the arguments it gets.

A case of the lists is (nblk, queues, workers, nwide, options): block columns of the padded system, XCD queues, model workers per
queue, wide inverse blocks, and fields of MegaScheduleOptions (slam-tricks_amd/csrc/chol_schedule.hpp) that differ from the defaults."""

# ---- identity with the lists as dense_chol.hip built them before the schedule moved into the header
# the production shape: eight XCDs, 32 resident workgroups each, wide inverse blocks over all panels but the tail.  Every size up to
# n = 6272, and the first sizes of the far-update batches 4, 8, 16 (mega_default_batch: 2 from nblk = 1, then 48, 68, 95).
PRODUCTION = [(nblk, 8, 32, (nblk - 1) // 4) for nblk in list(range(1, 50)) + [64, 68, 95]]
# fewer queues, the least workers the kernel accepts (MEGA_NTU), no wide blocks (what the schedule model entry point builds)
THIN = [(nblk, nq, 10, 0) for nq in (1, 2, 4) for nblk in (1, 2, 3, 5, 9, 16, 20, 33, 47)]
IDENTITY = PRODUCTION + THIN

# the multi-GPU what-if model: four rows of the table of tools/shard_model.py (eight XCDs of 32 workgroups per GPU, eight tile
# rows per GPU and round, 3 us per hop, a 128 KiB tile over a 48 GB/s link), as (nblk, gpus, xcds, workers, rows, hop us, tile us)
TILE_US = 128.0 * 128.0 * 8.0 / (48.0 * 1e3)
SHARD = [(47, 2, 8, 32, 8, 3.0, TILE_US), (47, 4, 8, 32, 8, 3.0, TILE_US), (94, 2, 8, 32, 8, 3.0, TILE_US), (94, 8, 8, 32, 8, 3.0, TILE_US)]


# ---- option sets for the replay: every threshold at both ends, the batch shapes, the priorities
def option_sets(nblk):
    sets = [dict(batch=1), dict(batch=3), dict(batch=16), dict(batch_lag=5), dict(far_batch=4), dict(qrows=0), dict(qrows=6),
            dict(blevel=0.0), dict(blevel=0.5)]
    for f in ("thalf_from", "tu10_from", "q_from", "dq_from"):
        sets += [{f: 0}, {f: nblk + 1}]
    return sets


OPTION_SHAPES = [(47, 8, 32, 11), (20, 2, 10, 0)]


def name(case, opts=None):
    s = "n%d_q%d_w%d_v%d" % tuple(case)
    for k, v in sorted((opts or {}).items()):
        s += "_%s%s" % (k, v)
    return s


def lists_args(prefix, case, opts=None):
    return ["lists", prefix] + [str(v) for v in case] + ["%s=%r" % kv for kv in sorted((opts or {}).items())]


def shard_name(c):
    return "shard_n%d_g%d" % (c[0], c[1])


def shard_args(c):
    return ["shard"] + [repr(v) for v in c]
