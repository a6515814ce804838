"""Inner iterations on the device (stba_ba_set_inner_iterations / stba_ba_inner_sweep / stba_ba_solve) against the independent
numpy reference of inner_iterations_ref.py: one sweep (iteration counts per block, parameters, costs), whole solves through the
dense Schur and the ITERATIVE_SCHUR path (accept / reject sequence, the iteration that switches sweeps off, trace values), under
the default, user and partial orderings; bitwise reproducibility; and the off path bit for bit as an engine that never enabled
them."""
import importlib

import numpy as np
import pytest

import inner_iterations_ref as I
import lm_step_ref as L

pytestmark = pytest.mark.gpu

# A sweep is a few inner LM steps per block from the same start, with the same iteration counts on both sides (checked exactly), so
# the two agree to rounding amplified by the condition number of the blocks' damped systems.  The worst blocks here are the extras'
# landmarks seen once or at grazing angles (kappa up to ~1e8): kappa * eps ~ 2e-8 relative, hence 1e-8 of max|x| (the largest
# error measured is 5.6e-8 absolute against max|x| ~ 10).  Costs: 1e-10 relative instead of 1e-12, because the device sums the
# ~1e4 float64 terms of st20 in its own order while the reference sums them in long double.
PARAM_TOL = 1e-8
COST_RTOL = 1e-10


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def engine(st, s, solver="dense_schur"):
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s.get("cam_fixed"), pt_fixed=s.get("pt_fixed"),
                    linear_solver=solver)
    if solver == "iterative_schur":
        e.set_pcg("jacobi", eta=1e-14, max_iterations=10000)
    return e


def x_of(e):
    cams, pts = e.get_params()
    return np.concatenate([cams.reshape(-1), pts.reshape(-1)])


def st20():
    sc = importlib.import_module("slam-tricks_amd.scenes").st20_scene()
    sc = dict(sc)
    sc.setdefault("pt_fixed", None)
    return sc


def scene(name):
    if name == "ba":
        return L.ba_scene()
    if name == "ba_extras":
        return L.ba_scene(n_lm=33, extras=True)
    return st20()


ORDERINGS = {
    "default": {},
    "split_camera": dict(rot_group=("rot", 0), pos_group=("pos", 1), pt_group=("pt", 2)),
    "landmarks_first": dict(rot_group=("cam", 1), pos_group=("cam", 1), pt_group=("pt", 0)),
    "landmarks_only": dict(pt_group=("pt", 0)),
}


def ordering_arrays(prob, spec):
    out = {}
    for k, (kind, gid) in spec.items():
        n = prob.np_ if kind == "pt" else prob.nc
        out[k] = np.full(n, gid, np.int32)
    return out


def ref_order(prob, arrs):
    if not arrs:
        return I.ordering(prob)
    return I.ordering(prob, arrs.get("rot_group"), arrs.get("pos_group"), arrs.get("pt_group"))


@pytest.mark.parametrize("name", ["ba", "ba_extras", "st20"])
@pytest.mark.parametrize("order", ["default", "split_camera", "landmarks_first"])
def test_one_sweep_matches_reference(st, name, order):
    s = scene(name)
    prob = L.ba_problem(s) if name != "st20" else L.BAProblem(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"],
                                                              s.get("cam_fixed"))
    arrs = ordering_arrays(prob, ORDERINGS[order])
    e = engine(st, s)
    e.set_inner_iterations(True, 1e-3, **arrs)
    c0, c1, it = e.inner_sweep()
    xs, it_ref = I.sweep(prob, prob.x0, ref_order(prob, arrs))
    for k in ("rot", "pos", "pt"):
        assert np.array_equal(it[k], it_ref[k]), (k, np.nonzero(it[k] != it_ref[k])[0][:10])
    xd = x_of(e)
    err = np.abs(xd - xs).max()
    print(f"INNER sweep {name} {order}: cost {c0:.6e} -> {c1:.6e}, max|dx| {err:.2e}, iterations max {max(it['pt'].max(), it['rot'].max())}")
    assert err <= PARAM_TOL * max(1.0, np.abs(xs).max()), err
    assert abs(c0 - prob.cost(prob.x0)) <= COST_RTOL * prob.cost(prob.x0)
    assert abs(c1 - prob.cost(xs)) <= COST_RTOL * prob.cost(xs)
    assert c1 < c0
    summ = e.inner_summary()
    assert summ.sweeps == 1 and summ.num_groups == len(ref_order(prob, arrs))


def solve_both(st, s, prob, opt_kw, k, arrs, tol, solver):
    e = engine(st, s, solver)
    e.set_inner_iterations(True, tol, **arrs)
    o = L.lm_options(**opt_kw)               # (the reference's options: tolerances 0 unless the case sets them)
    opt = st.default_options(**dict(o, max_num_iterations=k))
    summ, tr = e.solve(opt)
    rows, start = I.outer_reference(prob, dict(o, function_tolerance_takes_step=opt.function_tolerance_takes_step), k,
                                    ref_order(prob, arrs), tol)
    return e, summ, tr, rows, start


def check_solve(e, summ, tr, rows, start, label, cost_rtol=1e-7, values=True):
    ref_tr = I.trace_rows(rows)
    n = len(rows)
    assert summ.num_iterations == n, (label, summ.num_iterations, n)
    assert np.array_equal(tr[1:n + 1, 6], ref_tr[:, 6]), (label, tr[1:n + 1, 6], ref_tr[:, 6])
    off_ref = next((i + 1 for i, r in enumerate(rows) if not r["inner_on"]), -1)
    inner = e.inner_summary()
    assert inner.disabled_at_iteration == off_ref, (label, inner.disabled_at_iteration, off_ref)
    assert inner.sweeps == sum(r["swept"] for r in rows), label
    for i, r in enumerate(rows if values else []):
        # values where the decisions have margin: rho away from min_relative_decrease by 1e-2 and from the switch-off threshold
        if abs(r["rho"] - 1e-3) < 1e-2:
            continue
        d = tr[i + 1]
        assert abs(d[0] - r["trial_cost"]) <= cost_rtol * max(r["trial_cost"], start["cost"] * 1e-6), (label, i + 1, d[0], r["trial_cost"])
        assert abs(d[3] - r["step_norm"]) <= 1e-6 * max(r["step_norm"], 1e-12) + 1e-12, (label, i + 1, d[3], r["step_norm"])
    xd = x_of(e)
    assert np.abs(xd - rows[-1]["x"]).max() <= 1e2 * cost_rtol * max(1.0, np.abs(rows[-1]["x"]).max()), label
    print(f"INNER solve {label}: {n} iterations, accepted {int(ref_tr[:, 6].sum())}, sweeps {inner.sweeps}, off at {off_ref}, "
          f"cost {start['cost']:.6e} -> {summ.final_cost:.6e}")


@pytest.mark.parametrize("solver", ["dense_schur", "iterative_schur"])
@pytest.mark.parametrize("order,tol", [("default", 1e-3), ("default", 0.5), ("landmarks_first", 1e-3), ("landmarks_only", 1e-3),
                                       ("split_camera", 1e-3)])
def test_solve_matches_reference(st, solver, order, tol):
    s = L.ba_scene()
    prob = L.ba_problem(s)
    arrs = ordering_arrays(prob, ORDERINGS[order])
    # (4 iterations: the cost is then within 1e-6 of the scene's floor, where further decisions are made by rounding)
    e, summ, tr, rows, start = solve_both(st, s, prob, {}, 4, arrs, tol, solver)
    check_solve(e, summ, tr, rows, start, f"{solver}/{order}/tol={tol}")
    if tol == 0.5:
        assert any(not r["inner_on"] for r in rows)


def test_solve_with_tolerances_converges_like_reference(st):
    s = L.ba_scene(n_lm=33, extras=True)
    prob = L.ba_problem(s)
    kw = dict(function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8)
    e, summ, tr, rows, start = solve_both(st, s, prob, kw, 30, {}, 1e-3, "dense_schur")
    check_solve(e, summ, tr, rows, start, "tolerances")
    assert summ.termination_type == 0


def test_useful_sweep_rescues_a_step(st):
    """a start point whose first LM step (a huge initial radius: nearly Gauss-Newton) is rejected on rho alone, but the sweep
    brings the candidate below the current cost: the step is taken with rho <= min_relative_decrease"""
    s = L.ba_scene(n_lm=32, ang_noise_deg=6.0, pos_noise=0.5)
    prob = L.ba_problem(s)
    kw = dict(initial_trust_region_radius=1e16)
    e, summ, tr, rows, start = solve_both(st, s, prob, kw, 6, {}, 1e-3, "dense_schur")
    rescued = [i for i, r in enumerate(rows) if r["accepted"] and r["swept"] and r["rho"] <= 1e-3]
    if not rescued:
        pytest.fail("the scene no longer exercises the useful branch: " + str([(r["rho"], r["useful"]) for r in rows]))
    # (a radius of 1e16 makes the outer steps nearly Gauss-Newton and the rejected ones wild: the decisions, the switch-off and the end
    # point are compared, not the trace values of steps that land far from the solution)
    check_solve(e, summ, tr, rows, start, "useful", cost_rtol=1e-5, values=False)


def test_bitwise_reproducible(st):
    s = st20()
    outs = []
    for _ in range(2):
        e = engine(st, s)
        e.set_inner_iterations(True)
        summ, tr = e.solve(st.default_options(max_num_iterations=6))
        outs.append((x_of(e), tr))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_phase_timing_leaves_the_arithmetic_alone(st):
    """phase_timing = 1 with inner iterations: the same trace and parameters bit for bit, and the sweeps' device time reported"""
    s = L.ba_scene()
    outs = []
    for timing in (0, 1):
        e = engine(st, s)
        e.set_inner_iterations(True)
        summ, tr = e.solve(st.default_options(**dict(L.lm_options(), max_num_iterations=4, phase_timing=timing)))
        outs.append((summ, tr, x_of(e), e.inner_summary()))
    (s0, t0, x0, i0), (s1, t1, x1, i1) = outs
    print(f"INNER phase timing: sweep_ms {i1.sweep_ms:.4f}, sweeps {i1.sweeps}, {s1.as_dict()}")
    assert s0.num_iterations == s1.num_iterations == 4 and i0.sweeps == i1.sweeps >= 1
    assert np.array_equal(t0, t1) and np.array_equal(x0, x1)
    assert i0.sweep_ms == 0.0 and i1.sweep_ms > 0.0
    assert all(getattr(s1, f) > 0.0 for f in ("ms_linearize", "ms_schur", "ms_solve", "ms_backsub", "ms_cost")), s1.as_dict()


@pytest.mark.parametrize("solver", ["dense_schur", "iterative_schur"])
def test_off_path_is_bitwise_unchanged(st, solver):
    s = st20()
    e0 = engine(st, s, solver)
    s0, t0 = e0.solve(st.default_options(max_num_iterations=8))
    e1 = engine(st, s, solver)
    e1.set_inner_iterations(True)
    e1.set_inner_iterations(False)
    s1, t1 = e1.solve(st.default_options(max_num_iterations=8))
    assert np.array_equal(t0, t1) and np.array_equal(x_of(e0), x_of(e1))


def test_fixed_iteration_mode_sweeps(st):
    s = L.ba_scene()
    e = engine(st, s)
    e.set_inner_iterations(True, 0.0)
    e.lm_iterations(3)
    assert e.inner_summary().sweeps >= 1


def test_refusals_on_the_device(st):
    s = L.ba_scene()
    prob = L.ba_problem(s)
    e = engine(st, s)
    with pytest.raises(st.StbaError):        # a camera and the landmarks it observes in one group
        e.set_inner_iterations(True, 1e-3, rot_group=np.zeros(prob.nc, np.int32), pt_group=np.zeros(prob.np_, np.int32))
    assert "not an independent set" in st.lib().stba_last_error().decode()
    e.set_inner_iterations(True)
    e.set_trust_region("dogleg")
    x0 = x_of(e)
    with pytest.raises(st.StbaError):
        e.solve()
    assert np.array_equal(x_of(e), x0)
