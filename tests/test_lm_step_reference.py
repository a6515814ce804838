"""CPU tests of the LM step reference (lm_step_ref.py): its float64 numpy factors against the 50-digit model of mp_ref.py, its
whole step against a 50-digit redo on tiny problems, and the teeth of the GPU tests -- every deliberate mistake of
lm_step_ref.MUTATIONS moves a compared quantity by at least 100 x the GPU tests' bound on one of their own scenes."""
import mpmath as mp
import numpy as np
import pytest

import lm_step_ref as L
import mp_ref as M


def rel(a, b, floor=1.0):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), floor))


# ------------------------------------------------------------------------------- numpy factors against mp_ref (>= 200 points)
def test_ba_factors_match_mp_ref():
    rng = np.random.default_rng(0)
    worst = 0.0
    for i in range(80):
        q = M.quat_double(M.axis_angle(rng, [0.0, 1e-9, 0.3, 2.0, np.pi - 1e-7][i % 5]), negate=(i % 2 == 1))
        cam = np.concatenate([q, rng.normal(0, 1, 3)])
        R = L.quat_to_rot(q)
        L3 = cam[4:] + R @ np.array([rng.normal(0, 0.3), rng.normal(0, 0.3), [0.05, 1.0, 10.0, 1e3][i % 4]])
        f = rng.normal(0, 0.1, 2)
        P = L.BAProblem(cam[None], L3[None], [0], [0], f[None])
        r, Jc, Jp = P.lin_obs(cam[None], L3[None])
        rm = M.f64(M.ba_residual(cam, L3, f))
        Jcm, Jpm = (M.f64(x) for x in M.ba_jacobians_analytic(cam, L3))
        worst = max(worst, rel(r[0], rm), rel(Jc[0], Jcm, 0.0), rel(Jp[0], Jpm, 0.0))
        d = rng.normal(0, [0.3, 1e-9, 1.0][i % 3], 6)
        xn = P.plus(np.concatenate([cam, L3]), np.concatenate([d, np.zeros(3)]))
        qm = M.f64(M.rot_to_quat(M.mm(M.quat_to_rot(cam[:4]), M.so3_exp(d[:3]))))
        worst = max(worst, float(L.quat_dist(xn[:4], qm)))
    assert worst <= 1e-13, worst


def mp_rot_as_stored(q):
    """the standard rotation formula applied to q as stored (no normalisation): the BA residual's convention"""
    x, y, z, w = M.vec(q)
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def test_ba_factors_off_the_unit_sphere():
    """quaternions 1e-9 .. 1e-3 off unit length: residual and both Jacobians against 50-digit central differences of the
    as-stored convention (R exp(dtheta), t + dt, L + dL)"""
    rng = np.random.default_rng(3)
    worst = 0.0
    for i in range(24):
        q = M.quat_double(M.axis_angle(rng, [0.3, 2.0, np.pi - 1e-7][i % 3])) * (1.0 + [1e-9, -1e-7, 1e-5, -1e-3][i % 4])
        cam = np.concatenate([q, rng.normal(0, 1, 3)])
        L3 = cam[4:] + L.quat_to_rot(q) @ np.array([rng.normal(0, 0.3), rng.normal(0, 0.3), [0.5, 10.0][i % 2]])
        f = rng.normal(0, 0.1, 2)
        P = L.BAProblem(cam[None], L3[None], [0], [0], f[None])
        r, Jc, Jp = P.lin_obs(cam[None], L3[None])
        R, t, Lm = mp_rot_as_stored(q), M.vec(cam[4:]), M.vec(L3)

        def res(R_, t_, L_):
            pp = M.mv(M.tr(R_), [a - b for a, b in zip(L_, t_)])
            return [pp[0] / pp[2] - mp.mpf(f[0]), pp[1] / pp[2] - mp.mpf(f[1])]
        z6 = [mp.mpf(0)] * 6
        Jcm = M.f64(M.num_jac(lambda d: res(M.mm(R, M.so3_exp(d[:3])), [a + b for a, b in zip(t, d[3:])], Lm), z6, 2))
        Jpm = M.f64(M.num_jac(lambda l: res(R, t, l), Lm, 2))
        worst = max(worst, rel(r[0], M.f64(res(R, t, Lm))), rel(Jc[0], Jcm, 0.0), rel(Jp[0], Jpm, 0.0))
    assert worst <= 1e-13, worst


def test_pose_graph_factors_match_mp_ref():
    from test_lie_reference import LADDER
    rng = np.random.default_rng(1)
    worst = 0.0
    for i in range(70):
        th = LADDER[i % len(LADDER)]
        Ti = np.concatenate([M.quat_double(M.axis_angle(rng, 1.0)), rng.normal(0, 2, 3)])
        rel_q = M.quat_double(M.axis_angle(rng, th))
        Tj = L.rt_pose(*L.se3_compose_rt(L.pose_rt(Ti), (L.quat_to_rot(rel_q), rng.normal(0, 1, 3))))
        Z = L.rt_pose(*L.se3_compose_rt(L.se3_inverse_rt(L.pose_rt(Ti)), L.pose_rt(Tj)))
        Z = L.rt_pose(*L.se3_compose_rt(L.pose_rt(Z), L.se3_exp(rng.normal(0, [1e-3, 0.05][i % 2], 6))))
        P = L.PGProblem(np.stack([Ti, Tj]), [0], [1], Z[None])
        r, J, _ = P.lin(P.x0)
        rm, Jim, Jjm = M.pg_jacobians_build(M.pose(Ti), M.pose(Tj), M.pose(Z))
        worst = max(worst, rel(r[0], M.f64(rm)), rel(J[0], np.concatenate([M.f64(Jim), M.f64(Jjm)], 1), 0.0))
        d = rng.normal(0, [0.5, 1e-8][i % 2], 6)
        xn = P.plus(P.x0, np.concatenate([d, d]))[:7]
        Tm = M.retract(M.pose(Ti), M.vec(d))
        qm, tm = M.f64(M.rot_to_quat(Tm[0])), M.f64(Tm[1])
        worst = max(worst, float(L.quat_dist(xn[:4], qm)), rel(xn[4:], tm))
    assert worst <= 1e-13, worst


def test_calibration_factors_match_mp_ref():
    rng = np.random.default_rng(2)
    intr = np.array([800.0, 790.0, 320.0, 240.0, 0.05, -0.1, 0.02, 1e-4, -2e-4])
    worst = 0.0
    for i in range(60):
        ang = [0.0, 1e-9, 1.0, np.pi - 1e-7][i % 4]
        a = np.array([0.3 * rng.normal(), 0.3 * rng.normal(), 1.0]); a /= np.linalg.norm(a)
        xi = L.se3_log(L.so3_exp(a * ang), np.array([rng.normal(0, 0.02), rng.normal(0, 0.02), 0.5]))
        X, Y = rng.uniform(-0.1, 0.1, 2)
        u, v = rng.uniform(100, 500, 2)
        P = L.CalibProblem(np.concatenate([intr, xi]), np.array([[[X, Y]]]), np.array([[[u, v]]]))
        r, J, _ = P.lin(P.x0)
        rm = M.f64(M.calib_residual(intr, xi, X, Y, u, v))
        Jim, Jxm = (M.f64(x) for x in M.calib_jacobians_analytic(intr, xi, X, Y))
        worst = max(worst, rel(r[0], rm), rel(J[0], np.concatenate([Jim, Jxm], 1), 0.0))
        d = rng.normal(0, [0.2, 1e-9][i % 2], 6)
        xn = P.plus(P.x0, np.concatenate([np.zeros(9), d]))[9:]
        Tm = M.se3_compose(M.se3_exp(M.vec(d)), M.se3_exp(M.vec(xi)))
        A = L.se3_exp(xn)
        worst = max(worst, rel(A[0], M.f64(Tm[0])), rel(A[1], M.f64(Tm[1])))
    assert worst <= 1e-13, worst


# ------------------------------------------------------------------------------- the whole step at 50 digits
def mp_step(prob, opt, gauss_newton=False):
    """the first step of lm_reference redone at 50 digits: residuals and Jacobians from mp_ref, H, g, scaling, damping and
    mp.lu_solve over the free unknowns"""
    n = prob.n_local
    x = prob.x0
    H = mp.zeros(n, n)
    g = [mp.mpf(0)] * n
    for rb, Jb, cols in mp_blocks(prob, x):
        for a in range(len(cols)):
            g[cols[a]] += mp.fsum(Jb[e, a] * rb[e] for e in range(len(rb)))
            for b in range(len(cols)):
                H[cols[a], cols[b]] += mp.fsum(Jb[e, a] * Jb[e, b] for e in range(len(rb)))
    free = [i for i in range(n) if prob.free[i]]
    m = len(free)
    A = mp.zeros(m, m)
    bvec = mp.zeros(m, 1)
    s = [mp.mpf(1)] * n
    if not gauss_newton and opt["jacobi_scaling"]:
        s = [1 / (1 + mp.sqrt(H[i, i])) for i in range(n)]
    for ia, i in enumerate(free):
        bvec[ia] = -s[i] * g[i]
        for ja, j in enumerate(free):
            A[ia, ja] = s[i] * H[i, j] * s[j]
        if not gauss_newton:
            A[ia, ia] += min(max(s[i] ** 2 * H[i, i], mp.mpf(opt["min_lm_diagonal"])), mp.mpf(opt["max_lm_diagonal"])) / \
                mp.mpf(opt["initial_trust_region_radius"])
    y = mp.lu_solve(A, bvec)
    d = np.zeros(n)
    for ia, i in enumerate(free):
        d[i] = float(s[i] * y[ia])
    return d


def mp_blocks(prob, x):
    if isinstance(prob, L.BAProblem):
        cams, pts = prob.split(x)
        for o in range(len(prob.oc)):
            c, j = prob.oc[o], prob.op[o]
            Jc, Jp = M.ba_jacobians_analytic(cams[c], pts[j])
            J = mp.matrix(2, 9)
            for e in range(2):
                for a in range(6): J[e, a] = Jc[e, a]
                for a in range(3): J[e, 6 + a] = Jp[e, a]
            yield M.ba_residual(cams[c], pts[j], prob.f[o]), J, list(prob.cols[o])
    elif isinstance(prob, L.PGProblem):
        P = x.reshape(-1, 7)
        for e in range(len(prob.ei)):
            r, Ji, Jj = M.pg_jacobians_build(M.pose(P[prob.ei[e]]), M.pose(P[prob.ej[e]]), M.pose(prob.meas[e]))
            J = mp.matrix(6, 12)
            for a in range(6):
                for b in range(6): J[a, b] = Ji[a, b]; J[a, 6 + b] = Jj[a, b]
            yield r, J, list(prob.cols[e])
    else:
        intr = x[:9]
        obj, img = prob.obj.reshape(-1, 2), prob.img.reshape(-1, 2)
        for o in range(len(obj)):
            v = o // prob.C
            xi = x[9 + 6 * v: 15 + 6 * v]
            Ji, Jx = M.calib_jacobians_analytic(intr, xi, obj[o, 0], obj[o, 1])
            J = mp.matrix(2, 15)
            for e in range(2):
                for a in range(9): J[e, a] = Ji[e, a]
                for a in range(6): J[e, 9 + a] = Jx[e, a]
            yield M.calib_residual(intr, xi, obj[o, 0], obj[o, 1], img[o, 0], img[o, 1]), J, list(prob.cols[o])


def tiny_problems():
    S = L._st()
    s = S.pnp_scene(seed=17)
    n = len(s["pts"])
    yield "pnp", L.BAProblem(s["pose_init"][None], s["pts"], np.zeros(n, np.int32), np.arange(n, dtype=np.int32), s["feats"],
                             None, np.ones(n, np.uint8)), False
    b = L.ba_scene(n_lm=8, n_cams=2, seed=5)
    b["cam_fixed"] = np.array([[1] * 6, [0] * 6], np.uint8)
    yield "ba_2x8", L.ba_problem(b), False
    g = L.pg_scene(n_nodes=30, seed=4)
    keep = (g["edge_i"] < 4) & (g["edge_j"] < 4)
    p4 = L.rt_pose(*L.se3_compose_rt(L.pose_rt(g["poses0"][:4]), L.se3_exp(np.random.default_rng(3).normal(0, 0.05, (4, 6)))))
    yield "pg_4", L.PGProblem(p4, g["edge_i"][keep], g["edge_j"][keep], g["meas"][keep], g["node_fixed"][:4]), False
    # three views with different tilts (9 + 18 unknowns): one view of a planar board cannot fix the intrinsics
    p0, obj, img = L.calib_case(3, angles=L.CALIB_TILTED)
    yield "calib_3view", L.CalibProblem(p0, obj, img), True


@pytest.mark.parametrize("name", ["pnp", "ba_2x8", "pg_4", "calib_3view"])
def test_step_matches_50_digit_redo(name):
    prob, gn = {n: (p, g) for n, p, g in tiny_problems()}[name]
    assert prob.free.sum() <= 30
    opt = L.lm_options()
    ref = L.lm_reference(prob, opt, 1, gauss_newton=gn)
    d = mp_step(prob, opt, gauss_newton=gn)
    kap = ref[0]["kappa"]
    # a degenerate scene would make the bound below empty: the same gate as the GPU tests'
    assert 64 * kap * L.EPS <= 1e-6, f"{name}: kappa {kap:.2e}"
    err = np.linalg.norm(ref[0]["delta"] - d)
    print(f"{name}: kappa {kap:.2e}, err / (kappa eps |delta|) = {err / (kap * L.EPS * np.linalg.norm(d)):.2e}")
    if gn:          # the equilibrated kappa: the error is measured in the coordinates it bounds
        w = np.sqrt(ref[0]["start"]["hdiag"])
        assert np.linalg.norm(w * (ref[0]["delta"] - d)) <= 4 * kap * L.EPS * np.linalg.norm(w * d)
    else:
        assert err <= 4 * kap * L.EPS * np.linalg.norm(d)


# ------------------------------------------------------------------------------- teeth
def ba(case):
    sk, ok = L.BA_CASES[case]
    return L.ba_problem(L.ba_scene(**sk)), L.lm_options(**ok), "ba"


def pg(case):
    sk, ok = L.PG_CASES[case]
    return L.pg_problem(L.pg_scene(**sk)), L.lm_options(**ok), "pg"


# mutation -> the GPU test scene it is shown on
TEETH = {
    "no_s2_in_d": lambda: ba("lm31_r1e4"),
    "clamp_before_scaling": lambda: ba("lm33_max_diag"),
    "constant_damped_by_one": lambda: ba("lm33_extras_r1e-3"),
    "quat_left_multiply": lambda: ba("lm31_r1e4"),
    "no_quat_renorm": lambda: ba("lm31_q_off_unit"),
    "calib_right_update": None,
    "pg_left_multiply": lambda: pg("n40"),
    "rescale_every_iteration": lambda: ba("lm33_max_diag"),
    "shortcut_model_inexact": lambda: ba("lm300_r1e-3"),
}


def test_every_mutation_has_a_tooth():
    assert set(TEETH) == set(L.MUTATIONS)


@pytest.mark.parametrize("mutation", L.MUTATIONS)
def test_mutation_exceeds_100x_the_gpu_bound(mutation):
    if mutation == "calib_right_update":
        # the mutated run plays the device: compare_calib, the GPU test's own check, must fail, by >= 100 x its bound
        V, angles = L.CALIB_CASES["v20"]
        prob = L.CalibProblem(*L.calib_case(V, angles=angles))
        ref = L.lm_reference(prob, L.lm_options(), 2, gauss_newton=True)
        mut = L.lm_reference(prob, L.lm_options(), 2, mut={mutation}, gauss_newton=True)
        sse = [2 * mut[0]["start"]["cost"], 2 * mut[0]["cost"]]
        fails, ratios = L.compare_calib(prob, ref, mut[-1]["x"], sse)
        assert fails
        factor = ratios["point_over_bound"]
    elif mutation == "shortcut_model_inexact":
        # the control takes the same perturbed first step with Ceres' model change: step and trial point are identical, so
        # only rho can show the model formula (later iterations differ through the radius rho set, so only the first counts)
        prob, opt, path = TEETH[mutation]()
        ref = L.lm_reference(prob, opt, 1, mut={"inexact_step"})
        mut = L.lm_reference(prob, opt, 1, mut={mutation})
        assert np.array_equal(ref[0]["delta"], mut[0]["delta"]) and np.array_equal(ref[0]["x_trial"], mut[0]["x_trial"])
        factor = abs(ref[0]["rho"] - mut[0]["rho"]) / L.tolerances(ref, path, opt)[0]["rho"]
    else:
        prob, opt, path = TEETH[mutation]()
        k = 3
        ref = L.lm_reference(prob, opt, k)
        mut = L.lm_reference(prob, opt, k, mut={mutation})
        tol = L.tolerances(ref, path, opt, max(L.EPS, L.PCG_TOL) if path == "pg" else L.EPS)
        factor = 0.0
        for a, b, t in zip(ref, mut, tol):
            factor = max(factor, np.linalg.norm(a["delta"] - b["delta"]) / t["delta"],
                         L.point_error(prob, b["x"], a["x"]) / t["x"], abs(a["rho"] - b["rho"]) / t["rho"])
            if a["radius"] != b["radius"]:
                factor = max(factor, np.inf if t["radius"] == 0 else abs(a["radius"] - b["radius"]) / t["radius"])
    print(f"{mutation}: {factor:.2e} x the GPU bound")
    assert factor >= 100.0, factor
