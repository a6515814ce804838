"""The host-side Schur plan (slam-tricks_amd/csrc/schur_plan.hpp) without a device: tests/cpp/schur_plan_driver.cpp, compiled with g++,
builds the plan of every case of tests/schur_plan_cases.py and writes its arrays back.

Three kinds of check.  (1) Each case reaches the branch it is there for, by the plan's own flags.  (2) The plan's guarantees -- every
pair exactly once, one writer per block of S, every accumulator slot added to by ONE wave of its task (what makes S bitwise
reproducible) -- against a brute-force enumeration in numpy, written from the definitions in the header's comments.  (3) Identity
with the plan as it was built inside stba_ba_create before it moved into the header: tests/golden/schur_plan_digests.json holds
the FNV-1a digests and the scalars of that code on the same cases, and the free device memory it saw.  The driver is also built
with the address + undefined-behaviour sanitizers and with the thread sanitizer and must run without a report."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import schur_plan_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "schur_plan_digests.json")
NW = 8                      # SCHUR_THREADS / 64: waves of a task
MAX_SLOTS = 256             # SCHUR_MAX_SLOTS
SPLIT_COLS = MAX_SLOTS - 8  # SCHUR_SPLIT_COLS
CAM_CHUNK = 256
PLANNED = [n for n in SC.NAMES if n not in SC.REFUSED]
SANITIZERS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"], "tsan": ["-fsanitize=thread", "-g"]}
DTYPES = {"s_feat": "<f8", "dup_run": "u1", "task_part_off": "<i8"}        # everything else: int32


def _no_address_randomisation():
    """in the driver's process, before it starts: ThreadSanitizer's fixed shadow layout does not take every placement that a kernel with
    32 bits of mmap randomisation hands out, and then stops with "unexpected memory mapping" before main (ADDR_NO_RANDOMIZE)"""
    ctypes.CDLL(None).personality(0x0040000)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def run_driver(tmp_path_factory, golden):
    """run_driver(kind, case name) -> (the driver's JSON, the directory with the arrays); one build per kind, one run per (kind, case)"""
    base = tmp_path_factory.mktemp("schur_plan")
    exes, done = {}, {}

    def run(kind, name):
        if (kind, name) in done:
            return done[(kind, name)]
        if kind not in exes:
            exes[kind] = str(base / f"driver_{kind}")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-Wall", *SANITIZERS[kind],
                                   os.path.join(ROOT, "tests", "cpp", "schur_plan_driver.cpp"), "-o", exes[kind]])
        d = base / f"{kind}_{name}"
        d.mkdir()
        c = SC.case(name)
        g = golden.get(name)            # the memory figures the stored digests were made with
        if g:
            c = dict(c, free_bytes=g["scalars"]["free_bytes"], have_mem_info=bool(g["scalars"]["have_mem_info"]))
        SC.write_case(str(d / "case.bin"), c)
        p = subprocess.run([exes[kind], str(d / "case.bin"), str(d)], capture_output=True, text=True, timeout=300,
                           preexec_fn=_no_address_randomisation if kind == "tsan" else None)
        assert p.returncode == 0 and p.stderr == "", (kind, name, p.returncode, p.stderr[-2000:])
        done[(kind, name)] = (json.loads(p.stdout), str(d), c)
        return done[(kind, name)]
    return run


class Plan:
    def __init__(self, out, d, case):
        self.case, self.sc = case, out["scalars"]
        self.count = {k: v[0] for k, v in out["digests"].items()}
        for k in out["digests"]:
            a = np.fromfile(os.path.join(d, k + ".bin"), dtype=DTYPES.get(k, "<i4"))
            setattr(self, k, a.reshape(-1, 4) if k == "pair_rec" else a)
        self.nc, self.npts, self.no = case["n_cams"], case["n_pts"], len(case["obs_cam"])
        self.ntask = len(self.task_cam)


@pytest.fixture(scope="module")
def plan(run_driver):
    cache = {}

    def get(name):
        if name not in cache:
            out, d, c = run_driver("plain", name)
            assert out["rc"] == 0, out
            cache[name] = Plan(out, d, c)
        return cache[name]
    return get


# ---------------------------------------------------------------- the reference: brute force from the definitions
def _regroup_ref(c):
    """landmark-major stable counting sort, then the camera-side permutation of the sorted list (stable again)"""
    oc, op = c["obs_cam"].astype(np.int64), c["obs_pt"].astype(np.int64)
    perm = np.argsort(op, kind="stable")
    s_cam, s_pt = oc[perm], op[perm]
    pt_start = np.concatenate([[0], np.cumsum(np.bincount(op, minlength=c["n_pts"]))])
    cam_perm = np.argsort(s_cam, kind="stable")
    cam_start = np.concatenate([[0], np.cumsum(np.bincount(oc, minlength=c["n_cams"]))])
    return perm, s_cam, s_pt, pt_start, cam_perm, cam_start


def _candidates(s_pt, pt_start):
    """every (i, l) of sorted observations of one landmark, i == l included"""
    k = (pt_start[1:] - pt_start[:-1])[s_pt]
    i = np.repeat(np.arange(len(s_pt)), k)
    l = pt_start[s_pt[i]] + (np.arange(len(i)) - np.repeat(np.cumsum(k) - k, k))
    return i, l


def _check_regroup(P):
    c = P.case
    perm, s_cam, s_pt, pt_start, cam_perm, cam_start = _regroup_ref(c)
    assert np.array_equal(P.perm, perm) and np.array_equal(P.s_cam, s_cam) and np.array_equal(P.s_pt, s_pt)
    assert np.array_equal(P.s_feat.reshape(-1, 2), SC.features(P.no)[perm])
    assert np.array_equal(P.pt_start, pt_start) and np.array_equal(P.cam_perm, cam_perm) and np.array_equal(P.cam_start, cam_start)
    # chunks: every camera's range of cam_perm in pieces of at most CAM_CHUNK, in order
    cb, ce, ccs = [], [], [0]
    for cam in range(P.nc):
        for s0 in range(cam_start[cam], cam_start[cam + 1], CAM_CHUNK):
            cb.append(s0); ce.append(min(s0 + CAM_CHUNK, cam_start[cam + 1]))
        ccs.append(len(cb))
    assert np.array_equal(P.chunk_begin, cb) and np.array_equal(P.chunk_end, ce) and np.array_equal(P.cam_chunk_start, ccs)
    assert P.sc["n_chunks"] == len(cb)
    # repeated (camera, landmark) pairs: neighbours in a camera's list; the first of a run holds min(254, run - 1), the others 255
    key = s_cam[cam_perm] * max(P.npts, 1) + s_pt[cam_perm]
    dup = np.zeros(P.no, dtype=np.uint8)
    start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if P.no else np.zeros(0, dtype=np.int64)
    length = np.diff(np.concatenate([start, [P.no]]))
    dup[:] = 255
    dup[start] = np.minimum(254, length - 1)
    n_dup = int((length - 1).sum())
    assert P.sc["n_dup"] == n_dup and P.sc["dup_overflow"] == int((length > 255).any())
    assert np.array_equal(P.dup_run, dup if n_dup else np.zeros(0, dtype=np.uint8))
    assert P.sc["total_pairs"] == int((np.diff(pt_start) * (np.diff(pt_start) + 1) // 2).sum())
    return s_cam, s_pt, pt_start, cam_perm, cam_start


def _check_pair_plan(P):
    s_cam, s_pt, pt_start, cam_perm, cam_start = _check_regroup(P)
    assert P.sc["have_pair_plan"] == 1 and P.sc["schur_mode"] == 1 and P.sc["plan_mode"] == 0 and P.sc["n_tasks"] == P.ntask
    lm = bool(P.sc["lm_slices"])
    ci, cl = _candidates(s_pt, pt_start)
    keep = s_cam[cl] <= s_cam[ci]
    ci, cl = ci[keep], cl[keep]
    # ---- block pattern: row c holds camera c2 <= c iff they share a landmark (the camera itself as soon as it sees anything)
    blocks = np.unique(s_cam[ci] * P.nc + s_cam[cl])
    assert np.array_equal(P.row_cols, blocks % P.nc)
    assert np.array_equal(P.row_col_ptr, np.concatenate([[0], np.cumsum(np.bincount(blocks // P.nc, minlength=P.nc))]))
    ncols_row = np.diff(P.row_col_ptr)
    # ---- every pair (i, l), l != i, of one landmark with camera(l) <= camera(i): exactly once over all tasks
    off = ci != cl
    want = np.sort(ci[off] * P.no + cl[off])
    ri, rl, rj, rf = (P.pair_rec[:, k].astype(np.int64) for k in range(4))
    assert P.sc["pairs"] == len(ri) == len(want)
    assert np.array_equal(np.sort(ri * P.no + rl), want)
    assert np.array_equal(rj, s_pt[ri])
    # ---- the wave lists: contiguous, disjoint, tiling the task's range; the tasks tile the records
    pb, pe = P.pair_begin.reshape(P.ntask, NW).astype(np.int64), P.pair_end.reshape(P.ntask, NW).astype(np.int64)
    assert (pb <= pe).all() and np.array_equal(pe[:, :-1], pb[:, 1:])
    assert pb[0, 0] == 0 and pe[-1, -1] == len(ri) and np.array_equal(pe[:-1, -1], pb[1:, 0])
    task_size = pe[:, -1] - pb[:, 0]
    assert (np.diff(task_size) <= 0).all(), "tasks are ordered heaviest first"
    task_of = np.repeat(np.arange(P.ntask), task_size)
    wave_of = np.repeat(np.tile(np.arange(NW), P.ntask), (pe - pb).ravel())              # wave within its task
    list_of = np.repeat(np.arange(P.ntask * NW), (pe - pb).ravel())                     # (task, wave)
    pos_in_list = np.arange(len(ri)) - np.repeat(pb.ravel(), (pe - pb).ravel())
    # ---- flags
    slot, rot = rf & 0x3fff, (rf >> 16) & 7
    assert ((rf & ~(0x3fff | 0x8000 | 0x70000)) == 0).all()
    assert np.array_equal((rf & 0x8000) != 0, s_cam[rl] == s_cam[ri])
    assert (rot < 6).all()
    # ---- reproducibility: every accumulator slot of a task occurs in ONE wave's list
    ts = task_of * (1 << 14) + slot
    assert len(np.unique(ts * NW + wave_of)) == len(np.unique(ts))
    # ---- a record's slot lies in the slot range of its block's column within the task's slice
    tcam = P.task_cam.astype(np.int64)
    assert np.array_equal(s_cam[ri], tcam[task_of])
    col_index = np.full((P.nc, P.nc), -1, dtype=np.int64)
    for c in range(P.nc):
        col_index[c, P.row_cols[P.row_col_ptr[c]:P.row_col_ptr[c + 1]]] = np.arange(ncols_row[c])
    lo, hi = P.task_col_lo.astype(np.int64), P.task_col_hi.astype(np.int64)
    q = col_index[s_cam[ri], s_cam[rl]] - lo[task_of]
    assert (q >= 0).all() and (q < (hi - lo)[task_of]).all()
    vp = P.task_vs_ptr.astype(np.int64)
    assert np.array_equal(np.diff(vp), hi - lo + 1) and vp[0] == 0 and vp[-1] == len(P.vs_first)
    vs = P.vs_first.astype(np.int64)
    assert (vs[vp[task_of] + q] <= slot).all() and (slot < vs[vp[task_of] + q + 1]).all()
    n_slots = vs[vp[1:] - 1]
    assert (vs[vp[:-1]] == 0).all() and (n_slots <= MAX_SLOTS).all() and P.sc["max_cols"] == int(n_slots.max())
    parts = np.diff(vs)[np.setdiff1d(np.arange(len(vs) - 1), vp[1:] - 1)]           # slots per block, all tasks
    assert np.isin(parts, [1, 2, 4, 8]).all()
    # ---- rotations: in one 64-record trip of a wave, the first six records that share a slot have six different rotations
    group = (list_of * (len(ri) // 64 + 2) + pos_in_list // 64) * (1 << 14) + slot
    order = np.argsort(group, kind="stable")
    g_sorted = group[order]
    first = np.concatenate([[True], g_sorted[1:] != g_sorted[:-1]])
    rank = np.arange(len(order)) - np.maximum.accumulate(np.where(first, np.arange(len(order)), 0))
    six = rank < 6
    assert len(np.unique(g_sorted[six] * 8 + rot[order][six])) == six.sum()
    # ---- one writer per block of S: the column slices of a row partition its column list
    inv_cam_perm = np.empty(P.no, dtype=np.int64); inv_cam_perm[cam_perm] = np.arange(P.no)
    if not lm:
        assert P.count["task_p_lo"] == P.count["task_part_off"] == P.count["row_tasks"] == P.count["row_task_ptr"] == 0 and P.sc["part_doubles"] == 0
        for c in range(P.nc):
            t = np.flatnonzero(tcam == c)
            t = t[np.argsort(lo[t], kind="stable")]
            assert len(t) >= 1 and lo[t[0]] == 0 and hi[t[-1]] == ncols_row[c] and np.array_equal(hi[t[:-1]], lo[t[1:]])
            assert (hi[t] - lo[t] <= SPLIT_COLS).all()
    else:
        # landmark-range slices: all columns; every row's tasks by ascending p_lo partition the camera's list; partial blocks apart
        plo, phi = P.task_p_lo.astype(np.int64), P.task_p_hi.astype(np.int64)
        assert (lo == 0).all() and np.array_equal(hi, ncols_row[tcam]) and (ncols_row <= SPLIT_COLS).all()
        rtp = P.row_task_ptr.astype(np.int64)
        assert rtp[0] == 0 and rtp[-1] == P.ntask and np.array_equal(np.sort(P.row_tasks), np.arange(P.ntask))
        for c in range(P.nc):
            t = P.row_tasks[rtp[c]:rtp[c + 1]]
            assert len(t) >= 1 and (tcam[t] == c).all() and (np.diff(plo[t]) >= 0).all()
            assert plo[t[0]] == cam_start[c] and phi[t[-1]] == cam_start[c + 1] and np.array_equal(phi[t[:-1]], plo[t[1:]])
        p_of = inv_cam_perm[ri]
        assert (plo[task_of] <= p_of).all() and (p_of < phi[task_of]).all()
        ext = (hi - lo) * 36 + 64
        o = np.argsort(P.task_part_off, kind="stable")
        assert P.task_part_off[o[0]] == 0 and np.array_equal(P.task_part_off[o][1:], np.cumsum(ext[o])[:-1])
        assert P.sc["part_doubles"] == int(ext.sum())
    n_diag = int(((rf & 0x8000) != 0).sum())
    assert P.sc["lds_atomics"] == 36.0 * (len(ri) - n_diag) + 21.0 * n_diag
    return dict(ncols_row=ncols_row, parts=parts, task_size=task_size, tcam=tcam, lo=lo, hi=hi, rf=rf)


# ---------------------------------------------------------------- the cases
def test_small_light_blocks_and_an_empty_task(plan):
    P = plan("small")
    r = _check_pair_plan(P)
    assert not P.sc["lm_slices"] and (r["parts"] == 1).all(), "light blocks only"
    assert r["ncols_row"][6] == 0 and (r["task_size"][r["tcam"] == 6] == 0).all() and (r["tcam"] == 6).sum() == 1, "the camera that sees nothing: one empty task"
    assert P.pt_start[39] == P.pt_start[40] and P.pt_start[39] - P.pt_start[38] == 1


def test_two_cams_one_heavy_block_in_eight_parts(plan):
    P = plan("two_cams")
    r = _check_pair_plan(P)
    k = int(np.flatnonzero(r["tcam"] == 1)[0])
    assert P.ntask == 2 and r["hi"][k] - r["lo"][k] == 2, "row 1: the block with camera 0 and the diagonal block"
    v = P.vs_first[P.task_vs_ptr[k]:P.task_vs_ptr[k + 1]]
    assert list(v) == [0, 8, 9] and r["task_size"][k] == 600


def test_wide_row_is_cut_by_columns_on_several_threads(plan):
    P = plan("wide_row")
    r = _check_pair_plan(P)
    assert not P.sc["lm_slices"] and P.nc >= 128 and P.ntask >= 128, "host_parallel_for starts threads from 128 items"
    wide = np.flatnonzero(r["ncols_row"] > SPLIT_COLS)
    assert len(wide) > 0 and all((r["tcam"] == c).sum() >= 2 for c in wide)
    assert (r["hi"] - r["lo"]).max() == SPLIT_COLS


def test_dup_runs_and_the_overflow_that_keeps_the_pair_form(plan):
    P = plan("dup")
    r = _check_pair_plan(P)
    assert P.sc["dup_overflow"] == 1 and P.sc["have_pair_plan"] == 1 and P.sc["n_dup"] == 1 + 2 + 1 + 255
    assert sorted(set(P.dup_run.tolist())) == [0, 1, 2, 254, 255]
    assert ((r["rf"] & 0x8000) != 0).sum() == 2 + 6 + 2 + 256 * 255, "pairs of two observations of one camera: the diagonal blocks"
    assert (r["parts"] == 8).any()


def test_lm_slices_landmark_range_slices(plan):
    P = plan("lm_slices")
    assert P.sc["lm_slices"] == 1 and P.sc["total_pairs"] > 1 << 20 and P.no / (P.nc * P.npts) == 0.25
    r = _check_pair_plan(P)
    assert P.ntask > P.nc and (np.bincount(r["tcam"]) >= 2).sum() > P.nc // 2, "most rows are cut into several slices"


def test_two_slices_row_cap_without_landmark_ranges(plan):
    P = plan("two_slices")
    assert P.sc["lm_slices"] == 0 and P.sc["have_pair_plan"] == 1 and P.sc["total_pairs"] > 1 << 20 and P.nc <= 256
    r = _check_pair_plan(P)
    assert (r["ncols_row"][-4:] > SPLIT_COLS).all(), "what rules the landmark ranges out"
    # a slice closed by the pair cap, not by the column cap: fewer than SCHUR_SPLIT_COLS columns, and not the last of its row
    cap = max(4096, int(0.58 * P.sc["total_pairs"] / P.nc) + 1)
    closed_early = (r["hi"] < r["ncols_row"][r["tcam"]]) & (r["hi"] - r["lo"] < SPLIT_COLS)
    assert closed_early.any() and (r["task_size"][closed_early & (r["hi"] - r["lo"] > 1)] <= cap).all()


def test_dense_form_full_pattern_and_no_records(plan):
    P = plan("dense")
    _check_regroup(P)
    assert P.sc["schur_mode"] == 2 and P.sc["have_pair_plan"] == 0 and P.sc["pairs"] == 0 and P.ntask == 0 and P.sc["max_cols"] == 0
    assert np.array_equal(P.row_col_ptr, np.cumsum(np.arange(P.nc + 1)))
    assert np.array_equal(P.row_cols, np.concatenate([np.arange(c + 1) for c in range(P.nc)]))
    for k in ("pair_begin", "pair_end", "pair_rec", "task_vs_ptr", "vs_first", "task_col_lo", "task_col_hi", "task_p_lo", "row_tasks"):
        assert P.count[k] == 0, k


def test_iterative_has_no_pattern_and_no_plan(plan):
    P = plan("iterative")
    _check_regroup(P)
    assert P.sc["have_pair_plan"] == 0 and P.sc["schur_mode"] == 1 and P.ntask == 0 and P.sc["pairs"] == 0
    assert np.array_equal(P.row_col_ptr, np.zeros(P.nc + 1)) and P.count["row_cols"] == 0 and P.count["pair_rec"] == 0


def test_dense_form_with_a_256_fold_pair_is_refused(run_driver):
    out, _, _ = run_driver("plain", "dense_dup_overflow")
    assert out["rc"] != 0
    assert out["why"] == ("stba_ba_create: more than 255 observations of one (camera, landmark) pair in a problem that needs the dense "
                          "form of the Schur complement")


def test_no_room_for_the_plan_nor_for_y_is_refused(run_driver):
    out, _, c = run_driver("plain", "no_room")
    pairs = 2300 * 30 * 31 // 2
    cap = c["free_bytes"] // 2 // 16
    y_bytes = SC.lda(30) * ((3 * 2300 + 31) // 16 * 16) * 8
    assert pairs > cap and y_bytes >= c["free_bytes"] // 2
    assert out["rc"] != 0
    assert out["why"] == (f"stba_ba_create: {pairs} observation pairs (sum over landmarks of k (k + 1) / 2, k = cameras that see the landmark) "
                          f"need a Schur plan of {pairs * 16 // (1 << 20)} MiB; the limit here is {cap} pairs (2^30, or half of the free device "
                          f"memory) -- and the dense form needs {y_bytes // (1 << 20)} MiB, which the device does not have free either")


# ---------------------------------------------------------------- identity with the plan built inside stba_ba_create
@pytest.mark.parametrize("name", PLANNED)
def test_plan_equals_the_one_stba_ba_create_built(run_driver, golden, name):
    out, _, c = run_driver("plain", name)
    g = golden[name]
    assert out["rc"] == 0 and g["scalars"]["lda"] == SC.lda(c["n_cams"])
    for k, v in out["scalars"].items():
        assert g["scalars"][k] == v, (name, k, g["scalars"][k], v)
    assert sorted(out["digests"]) == sorted(g["digests"])
    for k, v in out["digests"].items():
        assert g["digests"][k] == v, (name, k, g["digests"][k], v)


@pytest.mark.parametrize("name", ["wide_row", "two_slices", "dup"])
@pytest.mark.parametrize("kind", ["asan_ubsan", "tsan"])
def test_sanitized_driver_runs_clean(run_driver, kind, name):
    """(run_driver asserts exit code 0 and an empty stderr: a sanitizer report is neither)"""
    out, _, _ = run_driver(kind, name)
    ref, _, _ = run_driver("plain", name)
    assert out == ref
