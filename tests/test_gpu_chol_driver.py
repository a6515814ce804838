"""The host driver of the dense Cholesky (dense_chol.hip, behind chol_factor_solve_dev / _stages / _split / _profiled and
chol_spd_inverse_dev) through st.cholesky_solve, st.cholesky_inverse and st.cholesky_profile: what it keeps BETWEEN calls.  The
kernels' accuracy is test_gpu_chol_conditioning.py's and test_gpu_chol_inverse.py's subject; here the same well-conditioned systems
are solved again and again and every answer must be the one the first call gave, bit for bit (the factorisation is repeatable: its
tiles receive their panels in panel order whoever runs them, chol_schedule.hpp), while

  - the stream changes from call to call.  The per-thread workspace and the device's persistent program are shared by every stream,
    so a factorisation that arrives on another stream than the last one is ordered behind it through an event recorded on that
    stream (chol_follow_previous).  cholesky_solve and cholesky_profile alone never get there: each builds its own workspace object,
    whose destructor takes its stream out of the device's record (chol_forget_stream) before the call returns, so the next call finds
    no previous stream.  The record-and-wait is reached only while an OWNER of the previous stream lives: the two tests at the end
    keep bundle adjustment engines alive on s1 and s2 (BAEngine.solve_reduced: chol_factor_solve_dev on the engine's stream) and
    factor around and between them.  One of them does so from one host thread: every entry point synchronises its stream before it
    returns, so there the previous factorisation has always finished, and the test shows that the hand-over runs and disturbs
    nothing, not that it is needed.  The other factors from two host threads at once, where it is needed: without it two persistent
    programs share the device and can starve each other into a time-out.  In the STAGE branch the hand-over is reached only in the
    cool-down after a time-out (a profile warms up with a persistent factorisation on its own stream first): not in this file;
  - the size changes from call to call: the cached task plan and its flag array are rebuilt when nblk or nwide differ, the workspace
    arrays only ever grow.  With lda = ceil((n + 1) / 128) 128, nblk = lda / 128 and nwide = (nblk - 1) / 4 wide backward steps:
        n     nblk  nwide
        127   1     0      no panel rows, no trailing update, one backward launch
        130   2     0
        500   4     0      the last size without a wide step
        600   5     1      the tail is block 4 alone; the first wide step applies with chol_bwd_apply_kernel<4>
        1000  8     1      the tail is blocks 4..7
        1100  9     2      the second wide step applies with chol_bwd_apply_kernel<16>
  - the explicit inverse (the stage loop on a workspace of its own) runs in between;
  - the profiled schedule (stage kernels between events, on the shared workspace) runs in between.

No time-out is provoked here, and none must have been provoked earlier in the process: after one the next 64 factorisations take the
stage kernels (the cool-down), and these tests, which pass there too, would no longer run the persistent branch.  In the whole suite
this file runs before test_gpu_chol_conditioning.py and test_gpu_parity.py, which provoke time-outs.
"""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (127, 130, 500, 600, 1000, 1100)
# (n, stream) of the calls, in order; None: no stream given (the call then makes one of its own)
SEQUENCE = ((127, None), (600, "s1"), (130, "s2"), (1100, "s1"), (600, None), (1000, "s2"), (500, "s1"))
N_INVERSE = 129          # two panels


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def spd(n, seed):
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(n, n))
    return G @ G.T + n * np.eye(n), rng.normal(size=n)


@pytest.fixture(scope="module")
def systems():
    """n -> (A, b, numpy's solution)"""
    out = {}
    for n in SIZES:
        A, b = spd(n, 11 + n)
        out[n] = (A, b, np.linalg.solve(A, b))
    return out


@pytest.fixture(scope="module")
def answers(st, systems):
    """n -> the device's solution, each computed once with no stream given, before any test of this file changes streams"""
    return {n: st.cholesky_solve(A, b) for n, (A, b, _) in systems.items()}


@pytest.fixture(scope="module")
def streams(st):
    import torch
    objs = {"s1": torch.cuda.Stream(), "s2": torch.cuda.Stream()}
    yield {None: None, "s1": objs["s1"].cuda_stream, "s2": objs["s2"].cuda_stream}
    for s in objs.values():
        s.synchronize()


def check_solve(st, systems, answers, n, stream):
    A, b, x_ref = systems[n]
    x = st.cholesky_solve(A, b, stream=stream)
    assert np.array_equal(x, answers[n]), f"n = {n}: not the answer of the first call"
    assert np.allclose(x, x_ref, rtol=1e-9, atol=1e-11), f"n = {n}"


def test_the_answer_set_is_right(systems, answers):
    for n, (_, _, x_ref) in systems.items():
        assert np.allclose(answers[n], x_ref, rtol=1e-9, atol=1e-11), f"n = {n}"


def test_alternating_streams_and_sizes_repeat_the_first_answers(st, systems, answers, streams):
    """every call arrives on another stream than the one before it and with another (nblk, nwide): the rebuilt plan and the grown
    workspace change nothing.  (No call finds a previous stream on record: see the head of the file.)"""
    for n, s in SEQUENCE:
        check_solve(st, systems, answers, n, streams[s])


def test_the_inverse_between_two_solves_on_different_streams(st, systems, answers, streams):
    """cholesky_inverse runs the stage loop on its own workspace, between two factorisations that use the shared one: it returns what
    the same call returns alone, and the solves around it return their answers"""
    A, _ = spd(N_INVERSE, 5)
    alone, rc_alone = st.cholesky_inverse(A, stream=streams["s2"])
    for k, (n, s) in enumerate(SEQUENCE):
        check_solve(st, systems, answers, n, streams[s])
        if k == 1:          # behind n = 600 on s1, in front of n = 130 on s2
            X, rc = st.cholesky_inverse(A, stream=streams["s2"])
            assert np.array_equal(X, alone) and rc == rc_alone


@pytest.mark.parametrize("n", [127, 300, 600])
def test_the_profiled_schedule_counts_its_updates_and_leaves_the_driver_usable(st, systems, answers, streams, n):
    """cholesky_profile: the stage kernels between events.  One trailing update per block that has rows below it; the flop counts
    are sums of integers, exact in a double.  The solve behind it (another stream, for n = 127 and 300 another plan) is unaffected"""
    p = st.cholesky_profile(n)
    nblk = (n + 1 + 127) // 128
    rows_below = [max(0, n - 128 * (b + 1)) for b in range(nblk - 1)]
    tiles_below = [nblk - b - 1 for b in range(nblk - 1)]
    assert p["syrk_launches"] == nblk - 1
    assert p["syrk_flops"] == sum(m * (m + 1) * 128 for m in rows_below)
    assert p["syrk_flops_padded"] == sum(mt * (mt + 1) // 2 * 2 * 128**3 for mt in tiles_below)
    for k in ("ms_diag", "ms_trsm", "ms_syrk", "ms_bwd"):
        assert np.isfinite(p[k]) and p[k] >= 0.0, (k, p[k])
    check_solve(st, systems, answers, 600, streams["s1"])


# ------------------------------------------------------------------------------- behind a living owner of another stream
N_CAMS = 100             # the engines' reduced system: n = 600, the plan of (nblk, nwide) = (5, 1)


@pytest.fixture(scope="module")
def engines(st, streams):
    """two engines on the same scene, one on s1 and one on s2, linearised; alive until the module ends"""
    scenes = importlib.import_module("slam-tricks_amd.scenes")
    s = scenes.st20_scene(n_cams=N_CAMS, n_pts=800, seed=9, pos_noise=0.1, ang_noise_deg=1.0, pix_noise=1e-3)
    out = {}
    for name in ("s1", "s2"):
        e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], stream=streams[name])
        e.evaluate()
        e.normal_blocks()
        out[name] = e
    yield out
    for e in out.values():
        e.close()


def reduced_solve(e):
    """the engine's damped reduced system, built again (a solve leaves its factor in place) and solved on the engine's stream"""
    e.reduced_system(np.ones(6 * e.nc), np.ones((e.np_, 3)), fetch=False)
    return e.solve_reduced()


def test_factorisations_follow_a_living_engine_on_another_stream(st, systems, answers, streams, engines):
    """one host thread: each step below finds the stream of a living engine on record and is ordered behind it (persistent branch)"""
    before = st.cholesky_timeout_count()
    ref = reduced_solve(engines["s1"])                              # on record: s1
    check_solve(st, systems, answers, 600, streams["s2"])           # behind s1; its own stream leaves the record with it
    assert np.array_equal(reduced_solve(engines["s1"]), ref)        # on record: s1
    assert np.array_equal(reduced_solve(engines["s2"]), ref)        # behind s1, the same plan; on record: s2
    check_solve(st, systems, answers, 1100, None)                   # behind s2, another plan, a stream of its own
    assert np.array_equal(reduced_solve(engines["s2"]), ref)        # on record: s2
    assert np.array_equal(reduced_solve(engines["s1"]), ref)        # behind s2; on record: s1
    p = st.cholesky_profile(300, stream=streams["s2"])              # its warm-up behind s1, then the stage kernels on s2
    assert p["syrk_launches"] == 2
    assert np.array_equal(reduced_solve(engines["s1"]), ref)        # behind s2
    assert st.cholesky_timeout_count() == before


def test_two_threads_factor_on_two_streams_at_once(st, engines):
    """two host threads, an engine each, factor at the same time: the factorisations alternate between s1 and s2 while the other
    stream's program may still run, which is what the hand-over is for.  Every solution is the one a thread gets alone, and no
    persistent program was starved into a time-out"""
    import threading
    rounds = 8
    before = st.cholesky_timeout_count()
    ref = reduced_solve(engines["s1"])
    bar = threading.Barrier(2)
    out = {"s1": [], "s2": []}

    def run(name):
        bar.wait(timeout=60)
        for _ in range(rounds):
            out[name].append(reduced_solve(engines[name]))

    th = [threading.Thread(target=run, args=(name,)) for name in out]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th)
    for name in out:
        assert len(out[name]) == rounds and all(np.array_equal(x, ref) for x in out[name]), name
    assert st.cholesky_timeout_count() == before
