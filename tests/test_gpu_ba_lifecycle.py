"""The life of one bundle-adjustment engine around the state that owns itself (csrc/ba_engine.hpp): the phase-timing events, the
event pair around the cross-rank sum, the inner sweep's pair, and the layout of the cost partials (CostSlots).

  events      an engine is solved with phase_timing on (every event pair of its strategy is created and recorded) and again with it
              off, under LM, DOGLEG, LM with inner iterations and ITERATIVE_SCHUR; each solve is bit for bit the solve of a FRESH
              engine that is solved once the same way; after destroy the library's count of live device buffers is what it was
  all-reduce  an engine with an all-reduce hook (world_size 1: the sum over one rank is the identity, and the whole pack / hook /
              unpack sequence with its event pair runs) is solved with timing on and destroyed; a second engine created after it
              solves to the same bits
  cost slots  pose priors, relative-pose factors and landmark priors together -- all three extra slots of the cost partials in use --
              set in two different orders on two engines: stba_ba_cost and a 3-iteration solve give identical bits, so the slot order
              does not depend on the order of the setters

Timed solves are compared with timed solves and untimed with untimed (like with like); whether the two agree with each other is
printed, not asserted.  The scene is test_gpu_buffer_ownership.py's: 4 cameras x 12 landmarks, one constant camera and one constant
landmark.  Nothing here provokes a device error."""
import gc
import importlib

import numpy as np
import pytest

from test_gpu_buffer_ownership import ba_scene

pytestmark = pytest.mark.gpu

ITERATIONS = 4


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


@pytest.fixture(scope="module")
def scene(scenes):
    return ba_scene(scenes)


def baseline(st):
    gc.collect()          # (engines other tests dropped: their buffers go now, not in the middle of a sequence)
    return st.live_device_buffers()


def engine(st, s, mode="lm"):
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], cam_fixed=s["cam_fixed"], pt_fixed=s["pt_fixed"],
                    linear_solver="iterative_schur" if mode == "iterative_schur" else "dense_schur")
    if mode == "dogleg":
        e.set_trust_region("dogleg")
    if mode == "inner":
        e.set_inner_iterations(True)
    return e


def solved(e, s, timing, iterations=ITERATIONS):
    """one solve from the scene's start point: everything the caller sees of it but the times"""
    e.set_params(s["cams0"], s["pts0"])
    summ, trace = e.solve(max_num_iterations=iterations, phase_timing=int(timing))
    cams, pts = e.get_params()
    assert summ.num_iterations >= 1 and np.isfinite(summ.final_cost) and summ.final_cost < summ.initial_cost
    return (summ.num_iterations, summ.termination_type, summ.initial_cost, summ.final_cost, trace.tobytes(), cams.tobytes(), pts.tobytes())


def fresh(st, s, mode, timing):
    e = engine(st, s, mode)
    out = solved(e, s, timing)
    e.close()
    return out


@pytest.mark.parametrize("mode", ["lm", "dogleg", "inner", "iterative_schur"])
def test_timed_and_untimed_solves_of_one_engine_are_a_fresh_engines(st, scene, mode):
    start = baseline(st)
    ref = {timing: fresh(st, scene, mode, timing) for timing in (True, False)}
    assert st.live_device_buffers() == start
    e = engine(st, scene, mode)
    got = {}
    for timing in (True, False, True):          # (the third solve records into events that exist already)
        got[timing] = solved(e, scene, timing)
        print(f"  {mode}, phase_timing {int(timing)}: {got[timing][0]} iterations, cost {got[timing][2]:.17g} -> {got[timing][3]:.17g}")
        assert got[timing] == ref[timing], f"{mode}, phase_timing {int(timing)}: other bits than a fresh engine's ({got[timing][:4]} / {ref[timing][:4]})"
    if mode == "inner":
        assert e.inner_summary().sweeps >= 1
    if mode == "iterative_schur":
        assert e.pcg_summary().solves >= 1
    print(f"  {mode}: timed and untimed solves agree bitwise: {ref[True] == ref[False]}")
    e.close()
    assert st.live_device_buffers() == start


def test_allreduce_event_pair_goes_with_its_engine(st, scene):
    start = baseline(st)
    calls = []

    def hook(_user, _buf, count, _stream):      # (one rank: the sum is what the buffer holds)
        calls.append(int(count))
        return 0

    def one_engine():
        e = engine(st, scene)
        e.set_allreduce(hook, 0, 1)
        del calls[:]
        e.set_params(scene["cams0"], scene["pts0"])
        summ, trace = e.solve(max_num_iterations=ITERATIONS, phase_timing=1)
        cams, pts = e.get_params()
        n, lda = e.reduced_dim()
        # the reduced system travelled (the triangle, or the block list, + the four extras vectors), timed by the event pair
        assert summ.allreduce_calls >= 1 and summ.allreduce_bytes > 0.0 and summ.ms_allreduce > 0.0
        assert any(c > 4 * lda for c in calls) and all(c <= n * (n + 1) // 2 + 4 * lda for c in calls)
        out = (summ.num_iterations, summ.initial_cost, summ.final_cost, summ.allreduce_calls, summ.allreduce_bytes, list(calls),
               trace.tobytes(), cams.tobytes(), pts.tobytes())
        e.close()
        assert st.live_device_buffers() == start
        return out

    first = one_engine()
    second = one_engine()
    print(f"  {first[0]} iterations, cost {first[1]:.17g} -> {first[2]:.17g}, {first[3]} sums of the reduced system")
    assert first == second, f"the second engine gives other bits ({first[:5]} / {second[:5]})"


def test_cost_slot_order_does_not_depend_on_setter_order(st, scene):
    s = scene
    start = baseline(st)
    rng = np.random.default_rng(19)
    prior_poses = np.stack([s["cams0"][1], s["cams0"][2]])
    prior_poses[:, 4:] += rng.normal(0.0, 0.01, (2, 3))
    rel = np.zeros((2, 7))
    rel[:, 3] = 1.0
    rel[:, 4:] = [[0.6, 0.2, 0.0], [0.6, -0.2, 0.0]]
    lm_pos = s["pts0"][[0, 5, 5]] + rng.normal(0.0, 0.01, (3, 3))
    setters = {
        "pose priors": lambda e: e.set_pose_priors([1, 2], prior_poses, information=4.0 * np.eye(6)),
        "relative poses": lambda e: e.set_relative_poses([0, 1], [1, 2], rel, information=2.0 * np.eye(6)),
        "landmark priors": lambda e: e.set_landmark_priors([0, 5, 5], lm_pos, information=9.0 * np.eye(3)),
    }

    def run(order):
        e = engine(st, s)
        plain = e.cost()
        for name in order:
            setters[name](e)
        assert e.pose_prior_count() == 2 and e.relative_pose_count() == 2 and e.landmark_prior_count() == 3
        cost = e.cost()
        assert cost > plain          # (every factor kind adds to the cost)
        out = (cost,) + solved(e, s, False, iterations=3)
        e.close()
        return out

    a = run(["pose priors", "relative poses", "landmark priors"])
    b = run(["landmark priors", "relative poses", "pose priors"])
    print(f"  cost with all three factor kinds {a[0]:.17g}; 3 iterations: {a[3]:.17g} -> {a[4]:.17g}")
    assert a[0] == b[0], f"stba_ba_cost depends on the order of the setters: {a[0]!r} / {b[0]!r}"
    assert a == b, f"the solve depends on the order of the setters ({a[1:5]} / {b[1:5]})"
    assert st.live_device_buffers() == start
