"""The life of one pose-graph engine around its second-stream job (PgCoarseJob, csrc/pg_engine.hpp).  With default options every
solve of a graph that has a coarse space leaves the inversion of its last coarse operator running on the engine's second stream.
Everything that then frees or overwrites what that job reads or writes -- a setter of weights or losses, a covariance, the kernel
timing, a solve with another group size (new coarse buffers), close() -- has to deal with it first.  The test pins what the caller
sees: after each of these, the engine solves exactly as a FRESH engine does that is given the same poses and settings, no coarse
operator fails to factor, and close() right behind a solve gives every device buffer back.  300 nodes: 38 groups of 8, small enough
for a solve of a few milliseconds, large enough for the coarse space and hence the job."""
import gc
import importlib
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0
    return mod


@pytest.fixture(scope="module")
def scene(scenes):
    return scenes.pose_graph_scene(n_nodes=300, loops_per_node=3, seed=7, sigma_t=0.02, sigma_r=0.005, turns=6)


def pose_diff(a, b):
    dq = np.minimum(np.abs(a[:, :4] - b[:, :4]).max(1), np.abs(a[:, :4] + b[:, :4]).max(1)).max()
    return max(dq, np.abs(a[:, 4:] - b[:, 4:]).max())


def engine(st, s, poses, settings):
    return st.PGEngine(poses, s["edge_i"], s["edge_j"], s["meas"], s["node_fixed"], **settings)


def solved(e, **pcg_kw):
    """(LM iterations, final cost, poses, failed coarse operators, coarse unknowns) of one solve with default options but pcg_kw"""
    summ, _, _ = e.solve(pcg=e.pcg_options(**pcg_kw))
    ps = e.pcg_summary()
    return summ.num_iterations, summ.final_cost, e.get_poses(), ps.coarse_failures, ps.coarse_dim


def same_solve(got, ref, what):
    print(f"  {what}: {got[0]} iterations, cost {got[1]:.17g} (fresh engine: {ref[0]}, {ref[1]:.17g}), "
          f"poses differ by {pose_diff(got[2], ref[2]):.3g}, coarse unknowns {got[4]}")
    assert got[4] > 0, f"{what}: no coarse space, so no second-stream job"
    assert got[0] >= 1, f"{what}: the solve ran no iteration and left no job behind"
    assert got[0] == ref[0], f"{what}: {got[0]} LM iterations, a fresh engine takes {ref[0]}"
    assert abs(got[1] - ref[1]) <= 1e-12 * abs(ref[1]), f"{what}: final cost {got[1]!r}, a fresh engine ends at {ref[1]!r}"
    assert pose_diff(got[2], ref[2]) <= 1e-12, what
    assert got[3] == 0 and ref[3] == 0, f"{what}: coarse operators failed to factor"


@pytest.fixture(scope="module")
def first(st, scene):
    """the solve of a fresh engine from the scene's initial poses, default options: shared by the sequence and the two threads"""
    e = engine(st, scene, scene["poses0"], {})
    out = solved(e)
    e.close()
    return out


def test_engine_solves_like_a_fresh_one_after_every_step_that_meets_the_job(st, scene, first):
    s = scene
    m = len(s["edge_i"])
    rng = np.random.default_rng(3)
    W = np.eye(6)[None] * (1.0 + 0.5 * rng.random((m, 1, 1))) + 0.05 * rng.normal(size=(m, 6, 6))
    gc.collect()          # (engines other tests dropped: their buffers go now, not in the middle of the sequence)
    start = st.live_device_buffers()
    settings = {"loss": ("huber", 0.05)}
    e = engine(st, s, s["poses0"], settings)

    def step(what, **pcg_kw):
        """a solve of the long-lived engine against a fresh engine's from the same poses, with the same settings"""
        ref_e = engine(st, s, e.get_poses(), settings)
        ref = solved(ref_e, **pcg_kw)
        ref_e.close()
        same_solve(solved(e, **pcg_kw), ref, what)

    step("first solve")
    e.set_sqrt_information(W)
    settings["sqrt_information"] = W
    step("after set_sqrt_information")
    e.set_loss(None)
    del settings["loss"]
    assert not e.has_loss and e.has_information
    step("after set_loss(None)")
    pairs = [(0, 0), (7, 7), (7, 150), (299, 299), (299, 3)]
    ref_e = engine(st, s, e.get_poses(), settings)
    blocks_ref, _ = ref_e.covariance(pairs)
    ref_e.close()
    blocks, _ = e.covariance(pairs)
    assert np.isfinite(blocks).all() and np.abs(blocks).max() > 0.0
    # (the same linearisation on both engines; 1e-9 is the covariance PCG's own default tolerance, not a bound on the bits)
    assert np.abs(blocks - blocks_ref).max() <= 1e-9 * np.abs(blocks_ref).max()
    step("after covariance")
    ms = e.time_kernels(2)
    assert all(np.isfinite(v) and v > 0.0 for v in ms)
    step("after time_kernels")
    step("with another coarse_group", coarse_group=16)
    step("back to the automatic coarse_group")
    e.close()             # (the last solve's job may still be running)
    assert st.live_device_buffers() == start

    # the unweighted, loss-free solve from the initial poses is the module's shared one
    e = engine(st, s, s["poses0"], {})
    same_solve(solved(e), first, "a later engine, no weights")
    e.close()
    assert st.live_device_buffers() == start


def test_two_engines_solve_from_two_threads_at_once(st, scene, first):
    """two host threads, an engine each (its own two streams and events), solve at the same time, several times over, with a setter
    in between: every solve is the one a thread gets alone"""
    rounds = 3
    gc.collect()
    start = st.live_device_buffers()
    out = {"a": [], "b": []}
    errors = []
    bar = threading.Barrier(2)

    def run(name):
        try:
            bar.wait(timeout=60)
            for _ in range(rounds):
                e = engine(st, scene, scene["poses0"], {})
                out[name].append(solved(e))
                e.set_loss(None)          # (meets the job the solve left)
                e.close()
        except Exception as ex:           # (reported by the main thread)
            errors.append((name, repr(ex)))

    th = [threading.Thread(target=run, args=(name,)) for name in out]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th)
    assert not errors, errors
    for name in out:
        assert len(out[name]) == rounds
        for k, got in enumerate(out[name]):
            same_solve(got, first, f"thread {name}, solve {k}")
    assert st.live_device_buffers() == start
