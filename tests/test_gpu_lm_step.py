"""Every device LM step path against the independent dense reference of lm_step_ref.py (Ceres' documented rules, a Schur-free
float64 solve with refinement in long double): BA through the pair plan (both loop modes), the dense Schur form, two
landmark shards and a host lineariser; the pose graph under every PCG route with exact steps; the dense callback path on
both sides of SMALL_DENSE_MAX_N, with a manifold and with bounds; the calibration's Gauss-Newton.  k = 1 and k = 3 iterations
(calibration: 1 and 2); the end point and every trace row are compared, with bounds C * kappa * eps (lm_step_ref.tolerances).
Each case prints kappa and err / (kappa eps |ref|) per quantity."""
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
    else:
        summ, tr = e.solve(opt)
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    return tr


@pytest.mark.parametrize("mode", ["fixed", "solve"])
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
