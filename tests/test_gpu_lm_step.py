"""Every device LM step path against the independent dense reference of lm_step_ref.py (Ceres' documented rules, a Schur-free
float64 solve with refinement in long double): BA through the pair plan (both loop modes), the dense Schur form, two
landmark shards and a host lineariser; the pose graph under every PCG route with exact steps; the dense callback path on
both sides of SMALL_DENSE_MAX_N, with a manifold and with bounds; the calibration's Gauss-Newton.  k = 1 and k = 3 iterations
(calibration: 1 and 2); the end point and every trace row are compared, with bounds C * kappa * eps (lm_step_ref.tolerances).
Each case prints kappa and err / (kappa eps |ref|) per quantity."""
import ctypes
import functools
import importlib
import threading

import numpy as np
import pytest

import lm_step_ref as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def device_options(st, o, k):
    return st.default_options(**dict({f: v for f, v in o.items()}, max_num_iterations=k))


def judge(prob, ref, path, o, x_dev, trace, label, fixed_mode=False, eps_eff=L.EPS, decisions_only=False):
    kap = max(it["kappa"] for it in ref)
    if decisions_only:
        assert not any(it["accepted"] for it in ref) and L.rho_margin_ok(ref, o)
        fails, _ = L.compare(prob, ref, path, o, x_dev, trace, decisions_only=True)
        assert np.array_equal(x_dev, prob.x0), f"{label}: rejected steps moved the parameters"
        assert not fails, f"{label}: " + "; ".join(fails)
        return
    assert L.C_PATH[path] * kap * eps_eff <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = L.compare(prob, ref, path, o, x_dev, trace, fixed_mode=fixed_mode, eps_eff=eps_eff)
    print(f"LMSTEP {path} {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    if not any(it["accepted"] for it in ref):
        assert np.array_equal(x_dev, prob.x0), f"{label}: rejected steps moved the parameters"
    assert not fails, f"{label}: " + "; ".join(fails)


# ------------------------------------------------------------------------------- bundle adjustment
def ba_engine(st, s):
    return st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"])


def ba_x(e):
    cams, pts = e.get_params()
    return np.concatenate([cams.reshape(-1), pts.reshape(-1)])


def run_ba(st, e, o, k, mode):
    opt = device_options(st, o, k)
    if mode == "fixed":
        summ, tr = e.lm_iterations(k, opt)
    elif mode == "watched":              # (an iteration callback: nothing is deferred, nothing speculated)
        summ, tr = e.solve(opt, callback=lambda *a: 0)
    else:
        summ, tr = e.solve(opt)
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    return tr


@pytest.mark.parametrize("mode", ["fixed", "solve", "watched"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", list(L.BA_CASES))
def test_ba_pair_plan(st, case, k, mode):
    sk, ok = L.BA_CASES[case]
    s = L.ba_scene(**sk)
    o = L.lm_options(**ok)
    prob = L.ba_problem(s)
    ref = L.lm_reference(prob, o, k)
    e = ba_engine(st, s)
    tr = run_ba(st, e, o, k, mode)
    judge(prob, ref, "ba", o, ba_x(e), tr, f"{case} k={k} {mode}", fixed_mode=(mode == "fixed"),
          decisions_only=case in L.BA_DECISIONS_ONLY)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", ["lm31_r1e4", "lm33_extras_r1e-3", "lm300_r1e16", "reject_then_accept", "far_off_reject"])
def test_ba_dense_schur(st, case, k):
    sk, ok = L.BA_CASES[case]
    s = L.ba_scene(**sk)
    o = L.lm_options(**ok)
    prob = L.ba_problem(s)
    ref = L.lm_reference(prob, o, k)
    e = ba_engine(st, s)
    e.set_schur_mode(e.SCHUR_DENSE)
    assert e.schur_mode() == e.SCHUR_DENSE
    tr = run_ba(st, e, o, k, "solve")
    judge(prob, ref, "ba", o, ba_x(e), tr, f"dense-schur {case} k={k}", decisions_only=case in L.BA_DECISIONS_ONLY)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", ["lm33_extras_r1e-3", "lm300_r1e16", "reject_then_accept"])
def test_ba_host_linearizer(st, case, k):
    """the host hands over every Jacobian column, constant dofs and constant landmarks included: dropping them is the
    engine's job (include/stba.h asks nothing else of the callback)"""
    sk, ok = L.BA_CASES[case]
    s = L.ba_scene(**sk)
    o = L.lm_options(**ok)
    prob = L.ba_problem(s)
    ref = L.lm_reference(prob, o, k)
    e = ba_engine(st, s)
    assert prob.cam_fixed.any() and prob.pt_fixed.any() or case != "lm33_extras_r1e-3"

    def lin(cams, pts, want_jac):
        return prob.lin_obs(cams.copy(), pts.copy(), want_jac)
    e.set_host_linearizer(lin)
    tr = run_ba(st, e, o, k, "solve")
    judge(prob, ref, "ba", o, ba_x(e), tr, f"host-linearizer {case} k={k}")


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", ["lm300_r1e-3", "lm300_r1e16"])
def test_ba_two_shards_on_one_gpu(st, case, k):
    """two engines = two landmark shards from two threads, the all-reduce summed in-process (test_sharding.py's hook)"""
    import torch
    sharding = importlib.import_module("slam-tricks_amd.sharding")
    sk, ok = L.BA_CASES[case]
    s = L.ba_scene(**sk)
    o = L.lm_options(**ok)
    prob = L.ba_problem(s)
    ref = L.lm_reference(prob, o, k)
    world = 2
    bar = threading.Barrier(world)
    slots, out, errs = [None] * world, [None] * world, []

    def make_hook(rank):
        def hook(_u, buf, count, _stream):
            t = torch.as_tensor(sharding.DeviceVector(buf, count), device="cuda")
            torch.cuda.synchronize()
            slots[rank] = t
            bar.wait()
            total = slots[0] + slots[1]
            torch.cuda.synchronize()
            bar.wait()
            t.copy_(total)
            torch.cuda.synchronize()
            bar.wait()
            return 0
        return hook

    def run(rank):
        try:
            sh = sharding.make_shard(s, rank, world)
            e = st.BAEngine(sh["cams0"], sh["pts0"], sh["obs_cam"], sh["obs_pt"], sh["obs_feat"], sh["cam_fixed"])
            e.set_allreduce(make_hook(rank), rank, world)
            tr = run_ba(st, e, o, k, "solve")
            out[rank] = (tr, e.get_params(), sh)
        except Exception as ex:          # (a thread's failure is the test's)
            errs.append(ex)
            bar.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    (tr0, (c0, p0), sh0), (tr1, (c1, p1), sh1) = out
    assert np.array_equal(c0, c1) and np.array_equal(tr0, tr1)
    pts = np.zeros_like(s["pts0"])
    pts[sh0["lo"]:sh0["hi"]] = p0
    pts[sh1["lo"]:sh1["hi"]] = p1
    judge(prob, ref, "ba", o, np.concatenate([c0.reshape(-1), pts.reshape(-1)]), tr0, f"two-shards {case} k={k}")


# ------------------------------------------------------------------------------- the routes of the BA loop
# What the loop does differently when somebody watches it (a callback, progress text), when its phases are timed, when a late
# gradient test discards a computed step, and when an engine solves twice.  Two fresh engines repeat a solve bit for bit on these
# scenes (the first assertion of every comparison below is that the runs compared ARE comparable: same decisions), so two routes
# that must do the same arithmetic are held to the same bytes.
TERM_GRADIENT, TERM_MAX_ITER, TERM_USER = 1, 4, 8
ROUTE_CASES = ["lm31_r1e4", "reject_then_accept"]


@functools.lru_cache(maxsize=None)
def ba_case(case):
    sk, ok = L.BA_CASES[case]
    s = L.ba_scene(**sk)
    return s, ok, L.ba_problem(s)


@functools.lru_cache(maxsize=None)
def ba_reference(case, k):
    s, ok, prob = ba_case(case)
    return L.lm_reference(prob, L.lm_options(**ok), k)


def same_bits(label, a, b):
    """(trace, parameters) of two runs: prints what differs, then asserts byte equality"""
    (ta, xa), (tb, xb) = a, b
    dt = np.abs(ta - tb).max() if ta.shape == tb.shape else np.inf
    print(f"LMROUTE {label}: trace rows {len(ta)}/{len(tb)} max|d trace|={dt:.3e} max|d x|={np.abs(xa - xb).max():.3e}")
    assert ta.shape == tb.shape and ta.tobytes() == tb.tobytes(), f"{label}: traces differ (max {dt:.3e})"
    assert xa.tobytes() == xb.tobytes(), f"{label}: parameters differ (max {np.abs(xa - xb).max():.3e})"


def decisions(summ):
    return (summ.num_iterations, summ.termination_type, summ.termination_reason, summ.num_successful_steps, summ.num_unsuccessful_steps)


@pytest.mark.parametrize("case", ROUTE_CASES)
def test_ba_a_fresh_engine_repeats_its_bits(st, case):
    """the premise of the byte comparisons below: two fresh engines, one process, the same solve -- unwatched and watched"""
    s, ok, _ = ba_case(case)
    for cb in (None, lambda *a: 0):
        out = []
        for _ in range(2):
            e = ba_engine(st, s)
            summ, tr = e.solve(st.default_options(**ok), callback=cb)
            out.append((decisions(summ), (tr, ba_x(e))))
        assert out[0][0] == out[1][0]
        same_bits(f"repeat {case} {'watched' if cb else 'unwatched'}", out[0][1], out[1][1])


@pytest.mark.parametrize("case", ROUTE_CASES)
def test_ba_watched_equals_unwatched(st, case):
    """to convergence at the library's defaults, once speculating with the deferred read, once with a callback"""
    s, ok, _ = ba_case(case)
    out = []
    for cb in (None, lambda *a: 0):
        e = ba_engine(st, s)
        summ, tr = e.solve(st.default_options(**ok), callback=cb)
        assert summ.termination_type == 0, summ.as_dict()
        out.append((summ, tr, ba_x(e)))
    (su, tu, xu), (sw, tw, xw) = out
    print(f"LMROUTE watched/unwatched {case}: {su.as_dict()}")
    assert decisions(su) == decisions(sw), (su.as_dict(), sw.as_dict())
    assert np.array_equal(tu[:, 6], tw[:, 6])
    same_bits(f"watched/unwatched {case}", (tu, xu), (tw, xw))


def test_ba_callback_stop(st):
    """a callback that returns 1 at iteration 2 ends the solve there, at the point a watched two-iteration solve reaches"""
    s, ok, _ = ba_case("lm31_r1e4")
    o = L.lm_options(**ok)
    seen = []

    def cb(_user, it, *rest):
        seen.append(it)
        return 1 if it == 2 else 0
    e = ba_engine(st, s)
    summ, tr = e.solve(device_options(st, o, 10), callback=cb)
    assert summ.termination_reason == TERM_USER and summ.num_iterations == 2 and seen == [1, 2], (summ.as_dict(), seen)
    f = ba_engine(st, s)
    s2, tr2 = f.solve(device_options(st, o, 2), callback=lambda *a: 0)
    assert s2.num_iterations == 2
    same_bits("callback stop", (tr, ba_x(e)), (tr2, ba_x(f)))


@pytest.mark.parametrize("limit", ["default", "at_convergence"])
@pytest.mark.parametrize("route", ["unwatched", "watched", "dogleg"])
def test_ba_late_gradient_convergence(st, route, limit):
    """gradient_tolerance between the reference's |g|max after iterations 1 and 2 (the trace's second and third rows, their
    geometric mean: a factor sqrt(ratio) > 3 clear of either): the solve converges at iteration 2.  Unwatched, the loop learns that
    with the trial block of iteration 3, whose step it discards; with max_num_iterations = 2 it learns it behind the loop and
    promotes MAX_ITER to GRADIENT."""
    case, k = "lm31_r1e4", 4
    s, ok, _ = ba_case(case)
    ref = ba_reference(case, k)
    g = [ref[0]["start"]["gmax"]] + [it["gmax"] for it in ref]
    assert all(it["accepted"] for it in ref[:2])
    assert g[1] > 10.0 * g[2], f"|g|max rows too close for a tolerance between them: {g}"
    tol = float(np.sqrt(g[1] * g[2]))
    n = next(i for i, v in enumerate(g) if v <= tol)
    assert n == 2 and g[0] > tol
    o = dict(L.lm_options(**ok), gradient_tolerance=tol)
    e = ba_engine(st, s)
    if route == "dogleg":
        e.set_trust_region("dogleg")
    opt = device_options(st, o, 50 if limit == "default" else n)
    summ, tr = e.solve(opt, callback=(lambda *a: 0) if route == "watched" else None)
    print(f"LMROUTE late gradient {route} {limit}: tol {tol:.3e} reference |g|max {g} device {list(tr[:, 2])} {summ.as_dict()}")
    assert summ.termination_type == 0 and summ.termination_reason == TERM_GRADIENT, summ.as_dict()
    assert summ.num_iterations == n and len(tr) == n + 1, summ.as_dict()
    assert tr[n][2] <= tol < tr[n - 1][2]


PHASES = ("ms_linearize", "ms_schur", "ms_solve", "ms_backsub", "ms_cost")


@pytest.mark.parametrize("mode", ["solve", "watched", "fixed"])
@pytest.mark.parametrize("case", ROUTE_CASES)
def test_ba_phase_timing_leaves_the_arithmetic_alone(st, case, mode):
    s, ok, _ = ba_case(case)
    o = L.lm_options(**ok)
    k = 4
    out = []
    for timing in (0, 1):
        e = ba_engine(st, s)
        opt = device_options(st, dict(o, phase_timing=timing), k)
        if mode == "fixed":
            summ, tr = e.lm_iterations(k, opt)
        else:
            summ, tr = e.solve(opt, callback=(lambda *a: 0) if mode == "watched" else None)
        out.append((summ, tr, ba_x(e)))
    (s0, t0, x0), (s1, t1, x1) = out
    ms = {f: getattr(s1, f) for f in PHASES}
    print(f"LMROUTE phase timing {case} {mode}: {ms} total {s1.seconds_total * 1e3:.3f} ms")
    assert s0.num_iterations == s1.num_iterations == k
    same_bits(f"phase timing {case} {mode}", (t0, x0), (t1, x1))
    assert all(getattr(s0, f) == 0.0 for f in PHASES), s0.as_dict()
    assert all(v > 0.0 for v in ms.values()), ms
    assert sum(ms.values()) < s1.seconds_total * 1e3, (ms, s1.seconds_total)


def test_ba_progress_text(st, capfd):
    """minimizer_progress_to_stdout: the header, then one row per trace row, numbered 0 .. num_iterations (a solve that ends on
    its iteration limit: the loop prints no row for an iteration that stops on the function or parameter tolerance)"""
    s, ok, _ = ba_case("reject_then_accept")
    e = ba_engine(st, s)
    libc = ctypes.CDLL(None)
    libc.fflush(None)
    capfd.readouterr()
    summ, tr = e.solve(device_options(st, dict(L.lm_options(**ok), minimizer_progress_to_stdout=1), 3))
    libc.fflush(None)
    lines = capfd.readouterr().out.splitlines()
    assert summ.num_iterations == 3 and len(tr) == 4
    assert lines[0].split()[:2] == ["iter", "cost"], lines
    assert len(lines) == 1 + len(tr), lines
    assert [int(ln.split()[0]) for ln in lines[1:]] == list(range(summ.num_iterations + 1))


@pytest.mark.parametrize("case", ROUTE_CASES)
def test_ba_two_solves_on_one_engine(st, case):
    """the second solve of an engine is the solve of a fresh engine at the same point: what a solve resets (the Jacobi scale, the
    pending read, the PCG summary) it resets per solve"""
    s, ok, _ = ba_case(case)
    e = ba_engine(st, s)
    e.solve(st.default_options(**dict(ok, max_num_iterations=2)))
    cams, pts = e.get_params()
    sa, ta = e.solve(st.default_options(**ok))
    f = st.BAEngine(cams, pts, s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"])
    sb, tb = f.solve(st.default_options(**ok))
    assert decisions(sa) == decisions(sb), (sa.as_dict(), sb.as_dict())
    same_bits(f"two solves {case}", (ta, ba_x(e)), (tb, ba_x(f)))


# ------------------------------------------------------------------------------- pose graph
@pytest.mark.parametrize("pcg", list(L.PG_PCG))
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", list(L.PG_CASES))
def test_pose_graph(st, case, k, pcg):
    sk, ok = L.PG_CASES[case]
    g = L.pg_scene(**sk)
    o = L.lm_options(**ok)
    prob = L.pg_problem(g)
    ref = L.lm_reference(prob, o, k)
    e = st.PGEngine(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"])
    pc = e.pcg_options(forcing_eta0=0.0, relative_tolerance=L.PCG_TOL, **L.PG_PCG[pcg])
    summ, tr, _ = e.solve(device_options(st, o, k), pcg=pc)
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    judge(prob, ref, "pg", o, e.get_poses().reshape(-1), tr, f"{case} k={k} {pcg}", eps_eff=max(L.EPS, L.PCG_TOL))


# ------------------------------------------------------------------------------- dense callback path
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", L.DENSE_CASES)
def test_dense_callback(st, case, k):
    res, x0, m, n, plus, lo, hi, ok = L.dense_case(case)
    o = L.lm_options(**ok)
    prob = L.dense_problem(case)
    ref = L.lm_reference(prob, o, k)
    x, summ, tr = st.dense_solve(res, x0, m, n_local=n, plus=plus, lower=lo, upper=hi, opt=device_options(st, o, k))
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    judge(prob, ref, "dense", o, x, tr, f"{case} k={k}")


# ------------------------------------------------------------------------------- calibration Gauss-Newton
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("case", list(L.CALIB_CASES))
def test_calibration_gauss_newton(st, case, k):
    V, angles = L.CALIB_CASES[case]
    p0, obj, img = L.calib_case(V, angles=angles)
    prob = L.CalibProblem(p0, obj, img)
    ref = L.lm_reference(prob, L.lm_options(), k, gauss_newton=True)
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["calib"] * kap * L.EPS <= 1e-6, kap
    params, it, sse = st.calib_gauss_newton(p0, obj, img, max_iter=k)
    assert it == k
    fails, ratios = L.compare_calib(prob, ref, params, sse)
    print(f"LMSTEP calib {case} k={k} kappa={kap:.2e} " + " ".join(f"{a}={b:.2e}" for a, b in sorted(ratios.items())))
    assert not fails, "; ".join(fails)
