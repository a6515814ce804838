"""The ticket lists of the persistent Cholesky (slam-tricks_amd/csrc/chol_schedule.hpp) without a device: tests/cpp/chol_schedule_driver.cpp,
compiled with g++, builds the lists of the cases of tests/chol_schedule_cases.py and writes them back.

Three kinds of check.  (1) Identity with the lists as dense_chol.hip built them before the builder moved into the header:
tests/golden/chol_schedule_digests.json holds the FNV-1a digests of the task array, the list starts and the simulated start times and the
bit pattern of the makespan, made by that earlier code on the same cases, and the three outputs of the multi-GPU model.  (2) Structure,
enumerated in numpy from the protocol table: every task once, every panel on every tile once, one queue per tile row.  (3) A replay of the
flag protocol (tests/chol_schedule_ref.py) with as many workgroups per queue as the model had workers: every task finishes, the final
counters are right, no update starts out of order -- and the replay does fail when it should: too few workgroups, a ticket out of
place, a missing update.  The driver is also built with the address + undefined-behaviour sanitizers and must run without a report."""
import json
import os
import subprocess

import numpy as np
import pytest

import chol_schedule_cases as CC
import chol_schedule_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chol_schedule_digests.json")
SANITIZERS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def run_driver(tmp_path_factory):
    """run_driver(kind, arguments after the prefix, name) -> (the driver's JSON, the prefix of its files); one build per kind, one run per case"""
    base = tmp_path_factory.mktemp("chol_schedule")
    exes, done = {}, {}

    def run(kind, make_args, name):
        if (kind, name) in done:
            return done[(kind, name)]
        if kind not in exes:
            exes[kind] = str(base / f"driver_{kind}")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *SANITIZERS[kind],
                                   os.path.join(ROOT, "tests", "cpp", "chol_schedule_driver.cpp"), "-o", exes[kind]])
        prefix = str(base / f"{kind}_{name}")
        p = subprocess.run([exes[kind]] + make_args(prefix), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and p.stderr == "", (kind, name, p.returncode, p.stderr[-2000:])
        done[(kind, name)] = (json.loads(p.stdout), prefix)
        return done[(kind, name)]
    return run


class Lists:
    def __init__(self, case, out, prefix):
        self.nblk, self.nq, self.wg, self.nwide = case
        self.out = out
        self.tasks = np.fromfile(prefix + ".tasks.bin", dtype="<i4").reshape(-1, 4)
        self.lstart = np.fromfile(prefix + ".lstart.bin", dtype="<i4")
        self.start = np.fromfile(prefix + ".start.bin", dtype="<f4")
        assert len(self.tasks) == out["ntasks"] == len(self.start) and len(self.lstart) == self.nq + 1


@pytest.fixture(scope="module")
def lists(run_driver):
    def get(case, opts=None, kind="plain"):
        out, prefix = run_driver(kind, lambda prefix: CC.lists_args(prefix, case, opts), CC.name(case, opts))
        return Lists(case, out, prefix)
    return get


def _complete(L, workers=None):
    """the whole check of one set of lists: structure, replay to the end, final counters"""
    ref.structure(L.tasks, L.lstart, L.nblk, L.nwide)
    r = ref.replay(L.tasks, L.lstart, L.nblk, L.nwide, L.wg if workers is None else workers)
    assert r["done"], (r["finished"], r["total"])
    ref.check_final(r, L.nblk, L.nwide)


# ---------------------------------------------------------------- identity with the lists dense_chol.hip built
@pytest.mark.parametrize("case", CC.IDENTITY, ids=CC.name)
def test_lists_equal_the_ones_dense_chol_built(lists, golden, case):
    assert lists(case).out == golden[CC.name(case)]


@pytest.mark.parametrize("case", CC.SHARD, ids=CC.shard_name)
def test_shard_model_equals_the_one_dense_chol_computed(run_driver, golden, case):
    out, _ = run_driver("plain", lambda prefix: CC.shard_args(case), CC.shard_name(case))
    assert out == golden[CC.shard_name(case)]


def test_default_batches_begin_where_the_cases_say():
    """(the sizes of the production set that are there for the batch: a batch appears in the lists as its panel count)"""
    assert [min(n for n in range(1, 200) if _batch(n) == b) for b in (2, 4, 8, 16)] == [1, 48, 68, 95]


def _batch(nblk):
    b = 2
    while b < 16 and 0.5 * nblk * nblk / 256.0 / b >= 2.2:
        b *= 2
    return b


@pytest.mark.parametrize("nblk", [48, 68, 95])
def test_the_batch_sizes_reach_the_lists(lists, nblk):
    _, nb, _, _, _ = ref.fields(lists((nblk, 8, 32, (nblk - 1) // 4)).tasks)
    assert nb.max() == _batch(nblk)


# ---------------------------------------------------------------- structure and replay
@pytest.mark.parametrize("case", CC.IDENTITY, ids=CC.name)
def test_default_lists_are_a_complete_program_that_finishes(lists, case):
    _complete(lists(case))


@pytest.mark.parametrize("shape", CC.OPTION_SHAPES, ids=CC.name)
def test_option_sets_are_complete_programs_that_finish(lists, shape):
    default = lists(shape).out
    changed = 0
    for opts in CC.option_sets(shape[0]):
        L = lists(shape, opts)
        changed += L.out != default
        _complete(L)
    assert changed >= 12, "the options reach the builder"


def test_batch_lag_below_one_is_raised_to_one(lists):
    """lag 0 is not a correct program (the quartered update of the diagonal tile after next would drop the earlier panels of its
    batch): the builder raises it to 1, and lag 1 finishes"""
    for shape in CC.OPTION_SHAPES:
        l0, l1 = lists(shape, dict(batch_lag=0)), lists(shape, dict(batch_lag=1))
        assert l0.out == l1.out and l0.out != lists(shape).out
        _complete(l1)


# ---------------------------------------------------------------- the replay can fail
PROD47 = (47, 8, 32, 11)
ONE_QUEUE = (20, 1, 10, 0)


def test_fewer_workgroups_than_model_workers_stall(lists):
    L = lists(PROD47)
    r = ref.replay(L.tasks, L.lstart, L.nblk, L.nwide, 10)
    assert not r["done"] and 0 < r["finished"] < r["total"]
    assert ref.replay(L.tasks, L.lstart, L.nblk, L.nwide, 32)["done"]


def test_diagonal_block_behind_its_successor_stalls(lists):
    L = lists(ONE_QUEUE)
    ty, _, b, _, _ = ref.fields(L.tasks)
    p = L.nblk // 2
    k0, k1 = int(np.flatnonzero((ty == ref.D) & (b == p))[0]), int(np.flatnonzero((ty == ref.D) & (b == p + 1))[0])
    assert k0 < k1
    order = [k for k in range(len(L.tasks)) if k != k0]
    order.insert(order.index(k1) + 1, k0)
    moved = L.tasks[order]
    ref.structure(moved, L.lstart, L.nblk, L.nwide)                 # still every task once, in its queue
    r = ref.replay(moved, L.lstart, L.nblk, L.nwide, L.wg)
    assert not r["done"]


def test_missing_trailing_update_stalls_or_leaves_a_wrong_counter(lists):
    L = lists(PROD47)
    ty, nb, b, z, w = ref.fields(L.tasks)
    for pick in (np.flatnonzero((ty == ref.U) & (nb > 1))[7], np.flatnonzero((ty == ref.U) & (z >= L.nblk))[3], np.flatnonzero(ty == ref.UQ)[-1]):
        q = int(np.searchsorted(L.lstart, pick, side="right")) - 1
        tasks = np.delete(L.tasks, pick, axis=0)
        lstart = L.lstart.copy()
        lstart[q + 1:] -= 1
        with pytest.raises(AssertionError):
            ref.structure(tasks, lstart, L.nblk, L.nwide)
        r = ref.replay(tasks, lstart, L.nblk, L.nwide, L.wg)
        if r["done"]:
            with pytest.raises(AssertionError):
                ref.check_final(r, L.nblk, L.nwide)


def test_task_in_another_queue_trips_the_owner_check(lists):
    L = lists(PROD47)
    k = int(L.lstart[3]) - 1                    # the last ticket of queue 2 becomes the first of queue 3
    lstart = L.lstart.copy()
    lstart[3] -= 1
    rq = ref.row_queues(L.tasks, lstart, L.nblk + 4 * L.nwide)
    assert sorted(rq[int(ref.task_row(L.tasks)[k])]) == [2, 3]
    with pytest.raises(AssertionError):
        ref.structure(L.tasks, lstart, L.nblk, L.nwide)


def test_update_applied_twice_starts_out_of_order(lists):
    """a second copy of a whole-tile update finds its tile a panel further than the version it waits for"""
    L = lists(ONE_QUEUE)
    ty, nb, b, z, w = ref.fields(L.tasks)
    k = int(np.flatnonzero((ty == ref.U) & (nb == 1) & (b == 3))[0])
    tasks = np.insert(L.tasks, k + 1, L.tasks[k], axis=0)
    lstart = L.lstart.copy()
    lstart[1:] += 1
    with pytest.raises(ref.OutOfOrder):
        ref.replay(tasks, lstart, L.nblk, L.nwide, L.wg)


# ---------------------------------------------------------------- the sanitized driver
@pytest.mark.parametrize("case,opts", [(PROD47, None), ((95, 8, 32, 23), None), ((9, 2, 10, 0), None), (PROD47, dict(far_batch=4)),
                                       (PROD47, dict(batch_lag=0)), ((20, 2, 10, 0), dict(thalf_from=21, tu10_from=0))])
def test_sanitized_driver_runs_clean(lists, case, opts):
    """(run_driver asserts exit code 0 and an empty stderr: a sanitizer report is neither)"""
    assert lists(case, opts, kind="asan_ubsan").out == lists(case, opts).out


def test_sanitized_shard_model_runs_clean(run_driver):
    c = CC.SHARD[1]
    a, _ = run_driver("asan_ubsan", lambda prefix: CC.shard_args(c), CC.shard_name(c))
    b, _ = run_driver("plain", lambda prefix: CC.shard_args(c), CC.shard_name(c))
    assert a == b
