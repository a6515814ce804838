"""Camera pose priors of the GPU bundle adjustment (include/stba.h) against tests/ba_prior_ref.py.

  factor      evaluate_pose_priors against the 50-digit values at the angles ba_prior_ref.ANGLES of qh^-1 q (each with q -> -q), a
              full random W and a position-only W.  Per entry the bound is 4 x the error the float64 numpy restatement shows against
              the 50-digit value on the same input, with the floor 4 eps x (row's sum |W_jk| |entry_k|).  MEASURED on an MI355X:
              worst err / bound 0.25 (r') and 0.40 (J'), the worst of the rows at pi - 1e-6 0.25.
  blocks      normal_blocks() Hcc, gc = the prior-less engine's + the reference's sums, each entry within 8 eps x sum |terms| (the
              existing value counts as a term); cameras without priors keep their bits
  cost        evaluate() / cost() relative 1e-12 against the reference's longdouble sum
  solves      lm_step_ref.compare / tolerances on the augmented reference problem, PAIRS and DENSE, the five cases of
              ba_prior_ref.SOLVE_CASES
  geometry    more cameras with priors than two workgroups of the block kernel hold, plus a remainder, plus cameras without
  covariance  against the dense inverse of the reference's J^T J (relative Frobenius <= 50 kappa eps, tests/test_gpu_covariance.py)
  unchanged   never had priors == cleared with n = 0 == before set_pose_priors, bit for bit
  errors      every error and refusal of include/stba.h, in both orders of the two calls"""
import functools
import importlib

import numpy as np
import pytest

import ba_prior_ref as P
import lm_step_ref as L
import mp_ref as M

pytestmark = pytest.mark.gpu

STBA_ERR_INVALID_ARGUMENT, STBA_ERR_NOT_POSITIVE_DEFINITE = -1, -4
EPS = L.EPS


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def engine(st, s, cam_fixed="scene", **kw):
    cf = s["cam_fixed"] if isinstance(cam_fixed, str) else cam_fixed
    return st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], cf, pt_fixed=s.get("pt_fixed"), **kw)


def case_engine(st, name, with_priors=True):
    s, cf, cams, poses, Om, W, Wobs, table = P.case(name)
    kw = {}
    if Wobs is not None:
        kw["sqrt_information"] = Wobs
    if table is not None:
        kw["loss"] = dict(table)
    e = engine(st, s, cam_fixed=cf, **kw)
    if with_priors:
        e.set_pose_priors(cams, poses, information=Om, sqrt_information=W)
    return e


def x_of(e):
    cams, pts = e.get_params()
    return np.concatenate([cams.reshape(-1), pts.reshape(-1)])


def same_bits(x, y):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))


# ------------------------------------------------------------------------------- 1. the factor
ACC_FIXED = np.array([[1] * 6, [0] * 6, [1, 1, 1, 0, 0, 0], [0, 1, 0, 0, 1, 0]], np.uint8)      # cameras 0..3 of the accuracy scene


@functools.lru_cache(maxsize=None)
def accuracy_setup():
    """the default scene with the masks ACC_FIXED on cameras 0..3; on each of them one prior per angle and W kind.
    Returns (scene, cam_fixed, prior cams, poses, W, and per prior and sign of q the 50-digit (r', J'), the numpy restatement's
    errors and the floors)"""
    s = L.ba_scene()
    cf = np.zeros_like(s["cam_fixed"])
    cf[:4] = ACC_FIXED
    rng = np.random.default_rng(11)
    cams, poses, Ws = [], [], []
    for c in range(4):
        for name in P.ANGLES:
            for W in (P.random_W(rng)[0], P.position_only_W()[0]):
                cams.append(c); poses.append(P.pose_at_angle(s["cams0"][c], name, rng)); Ws.append(W)
    cams, poses, Ws = np.array(cams, np.int32), np.array(poses), np.array(Ws)
    ref = {}
    for sign in (1.0, -1.0):
        for k, c in enumerate(cams):
            cam = s["cams0"][c].copy()
            cam[:4] *= sign
            rm, Jm = P.prior_eval_mp(poses[k], cam, Ws[k], cf[c])
            rn, Jn = P.prior_eval_np(poses[k], cam, Ws[k], cf[c])
            ref[(sign, k)] = (rm, Jm, P.err_vs_mp(rn, Jn, rm, Jm), P.floors(Ws[k], poses[k], cam))
    return s, cf, cams, poses, Ws, ref


def test_factor_against_50_digits(st):
    """(the module docstring's `factor`)"""
    s, cf, cams, poses, Ws, ref = accuracy_setup()
    e = engine(st, s, cam_fixed=cf)
    e.set_pose_priors(cams, poses, sqrt_information=Ws)
    assert e.pose_prior_count() == len(cams)
    got = {}
    worst = {"r": 0.0, "J": 0.0, "near_pi": 0.0}
    for sign in (1.0, -1.0):
        c0 = s["cams0"].copy()
        c0[:, :4] *= sign
        e.set_params(c0, s["pts0"])
        cost, r, J = e.evaluate_pose_priors()
        got[sign] = (cost, r, J)
        cref = 0.0
        for k, c in enumerate(cams):
            rm, Jm, (ern, eJn), (fr, fJ) = ref[(sign, k)]
            er, eJ = P.err_vs_mp(r[k], J[k], rm, Jm)
            br, bJ = np.maximum(4 * ern, fr), np.maximum(4 * eJn, fJ)
            fixed = cf[c].astype(bool)
            assert np.all(J[k][:, fixed] == 0.0), f"prior {k}: a constant dof's column is not exactly zero"
            free = ~np.broadcast_to(fixed[None, :], (6, 6))
            qr = float(np.max(np.where(br > 0, er / np.where(br > 0, br, 1.0), np.where(er == 0, 0.0, np.inf))))
            qJ = np.where(bJ > 0, eJ / np.where(bJ > 0, bJ, 1.0), np.where(eJ == 0, 0.0, np.inf))
            qJ = float(np.max(qJ[free])) if free.any() else 0.0
            name = P.ANGLES[(k // 2) % len(P.ANGLES)]
            print(f"  sign {sign:+.0f} camera {c} angle {name:8s} W {'full' if k % 2 == 0 else 'gps '}: r' err/bound {qr:.3f}  J' err/bound {qJ:.3f}")
            worst["r"], worst["J"] = max(worst["r"], qr), max(worst["J"], qJ)
            if name == "pi-1e-6":
                worst["near_pi"] = max(worst["near_pi"], qr, qJ)
            cref += float(sum(v * v for v in rm)) / 2
        print(f"  sign {sign:+.0f}: prior cost {cost:.17g} reference {cref:.17g} relative {abs(cost - cref) / cref:.2e}")
        assert abs(cost - cref) <= 1e-12 * cref
    print(f"PRIOR factor: worst err / bound r' {worst['r']:.3f} J' {worst['J']:.3f} near pi {worst['near_pi']:.3f}")
    assert same_bits(got[1.0], got[-1.0]), "q and -q do not give identical bits"
    # angle exactly 0: the rotation residual is exactly 0 (the position-only W reads nothing else of it; the full W's r' then is W's
    # position columns times the position residual alone, which the bound above has checked)
    k0 = [k for k in range(len(cams)) if P.ANGLES[(k // 2) % len(P.ANGLES)] == "0" and k % 2 == 1]
    for k in k0:
        assert np.array_equal(got[1.0][1][k][:3], np.zeros(3))
    assert worst["r"] <= 1.0 and worst["J"] <= 1.0, worst


def test_a_prior_at_the_cameras_own_pose_is_exact(st):
    """angle exactly 0, identity weights: r' = 0 and J' = I in every bit (constant dofs' columns 0), the cost and the blocks those of
    the observations plus the identity on the free dofs' diagonal"""
    s = L.ba_scene()
    plain, e = engine(st, s), engine(st, s)
    cams = np.arange(len(s["cams0"]), dtype=np.int32)
    e.set_pose_priors(cams, s["cams0"])
    cost, r, J = e.evaluate_pose_priors()
    free = ~s["cam_fixed"].astype(bool)
    assert cost == 0.0 and np.array_equal(r, np.zeros_like(r))
    assert np.array_equal(J, np.eye(6)[None] * free[:, None, :])
    c0, c1 = plain.evaluate(jac=False)[0], e.evaluate(jac=False)[0]
    H0, g0, _, _ = plain.normal_blocks()
    H1, g1, _, _ = e.normal_blocks()
    assert c0 == c1 and np.array_equal(g0, g1)
    assert np.array_equal(H1, H0 + np.eye(6)[None] * free[:, None, :])


# ------------------------------------------------------------------------------- 2. blocks and cost
def check_blocks_and_cost(st, label, plain, e, prob):
    """e: the engine with the priors of prob, plain: the same engine without; both at prob.x0"""
    c0, r0, _, _ = plain.evaluate(jac=False)
    H0, g0, Hp0, gp0 = plain.normal_blocks()
    c1, r1, _, _ = e.evaluate(jac=False)
    H1, g1, Hp1, gp1 = e.normal_blocks()
    assert same_bits((r0, Hp0, gp0), (r1, Hp1, gp1)), f"{label}: the priors changed the observations' residuals or the landmark blocks"
    Hr, gr, Ha, ga = prob.blocks(prob.x0)
    LD = np.longdouble
    eH = np.abs(H1.astype(LD) - (H0.astype(LD) + Hr)).astype(float)
    eg = np.abs(g1.astype(LD) - (g0.astype(LD) + gr)).astype(float)
    bH = 8 * EPS * (np.abs(H0) + Ha.astype(float))
    bg = 8 * EPS * (np.abs(g0) + ga.astype(float))
    qH = float(np.max(np.where(bH > 0, eH / np.where(bH > 0, bH, 1.0), np.where(eH == 0, 0.0, np.inf))))
    qg = float(np.max(np.where(bg > 0, eg / np.where(bg > 0, bg, 1.0), np.where(eg == 0, 0.0, np.inf))))
    print(f"  {label}: Hcc err / bound {qH:.3f}, gc err / bound {qg:.3f}")
    rd, Jd = e.evaluate_pose_priors()[1:]
    rn, Jn = prob.lin_priors(prob.split(prob.x0)[0])
    print(f"  {label}: device r', J' against the numpy restatement: {int((rd != rn).sum())} of {rd.size} and {int((Jd != Jn).sum())} of {Jd.size} entries "
          f"differ, by at most {np.abs(rd - rn).max():.2e} and {np.abs(Jd - Jn).max():.2e}")
    without = np.setdiff1d(np.arange(prob.nc), prob.pr_cam)
    assert same_bits((H0[without], g0[without]), (H1[without], g1[without])), f"{label}: a camera without priors changed"
    const = np.nonzero(prob.cam_fixed.all(1))[0]
    assert same_bits((H0[const], g0[const]), (H1[const], g1[const])), f"{label}: a fully constant camera's blocks changed"
    assert np.array_equal(H1, np.swapaxes(H1, 1, 2)), f"{label}: Hcc is not bitwise symmetric"
    cref = prob.cost(prob.x0)
    c2 = e.cost()
    print(f"  {label}: cost {c1:.17g} / {c2:.17g} reference {cref:.17g} relative {abs(c1 - cref) / cref:.2e} (observations alone {c0:.6g})")
    assert abs(c1 - cref) <= 1e-12 * cref and abs(c2 - cref) <= 1e-12 * cref
    assert qH <= 1.0 and qg <= 1.0
    pc, _, _ = e.evaluate_pose_priors(jac=False)
    assert abs(pc - prob.prior_cost(prob.x0)) <= 1e-12 * max(prob.prior_cost(prob.x0), 1e-300)


@pytest.mark.parametrize("name", ["a_full_all_free", "b_two_on_one", "d_gauge_gps", "e_full_huber_info"])
def test_blocks_and_cost(st, name):
    check_blocks_and_cost(st, name, case_engine(st, name, False), case_engine(st, name), P.problem(name))


def test_constant_camera_contributes_to_the_cost_only(st):
    s = L.ba_scene()
    c = int(np.nonzero(s["cam_fixed"].all(1))[0][0])
    pose = s["cams_true"][c].copy()
    pose[4:] += 0.05
    prob = P.PriorBAProblem(s, [c], pose[None], P.sqrt_of_information(P.random_spd(np.random.default_rng(2), 1)))
    plain, e = engine(st, s), engine(st, s)
    e.set_pose_priors([c], pose[None], sqrt_information=prob.pr_W)
    check_blocks_and_cost(st, "constant camera", plain, e, prob)
    _, r, J = e.evaluate_pose_priors()
    assert np.array_equal(J, np.zeros((1, 6, 6))) and np.abs(r).max() > 0
    assert e.cost() > plain.cost()


def test_more_cameras_with_priors_than_two_workgroups_hold(st):
    """cameras with priors >= 2 x (the block kernel's cameras per workgroup) + a remainder, and cameras without"""
    s = L.ba_scene(n_cams=12)
    plain, e = engine(st, s), engine(st, s)
    per_wg = e.pose_prior_kernel_geometry()
    nc = len(s["cams0"])
    cams = np.arange(1, 2 * per_wg + 2, dtype=np.int32)
    assert len(cams) >= 2 * per_wg + 1 and len(cams) % per_wg != 0 and len(cams) < nc, (per_wg, nc)
    rng = np.random.default_rng(5)
    # (two on the first of them, the caller's order not grouped by camera)
    cams = np.concatenate([cams[::-1], cams[:1]]).astype(np.int32)
    poses = s["cams_true"][cams].copy()
    poses[:, 4:] += rng.normal(0, 0.05, (len(cams), 3))
    poses[:, :4] = L.quat_mul(poses[:, :4], L.quat_exp(rng.normal(0, 0.02, (len(cams), 3))))
    Om = P.random_spd(rng, len(cams))
    e.set_pose_priors(cams, poses, information=Om)
    prob = P.PriorBAProblem(s, cams, poses, P.sqrt_of_information(Om))
    check_blocks_and_cost(st, f"{len(set(cams.tolist()))} cameras with priors, {per_wg} per workgroup", plain, e, prob)
    # the caller's order comes back from the grouped one
    _, r, J = e.evaluate_pose_priors()
    rn, Jn = prob.lin_priors(prob.split(prob.x0)[0])
    assert np.allclose(r, rn, rtol=0, atol=1e-10 * np.abs(rn).max()) and np.allclose(J, Jn, rtol=0, atol=1e-10 * np.abs(Jn).max())


# ------------------------------------------------------------------------------- 3. solves
def judge(prob, ref, o, x_dev, trace, label):
    """tests/test_gpu_lm_step.py's judge"""
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = L.compare(prob, ref, "ba", o, x_dev, trace)
    print(f"LMSTEP ba-prior {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    assert not fails, f"{label}: " + "; ".join(fails)


@pytest.mark.parametrize("form", ["pairs", "dense"])
@pytest.mark.parametrize("name", list(P.SOLVE_CASES))
def test_exact_steps_follow_the_reference_with_priors(st, name, form):
    o = P.options(name)
    prob, ref = P.problem(name), P.reference(name)
    e = case_engine(st, name)
    if form == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
        assert e.schur_mode() == e.SCHUR_DENSE
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=P.K)))
    assert summ.num_iterations == P.K and len(tr) == P.K + 1, summ.as_dict()
    c0 = ref[0]["start"]["cost"]
    print(f"  {name} {form}: start cost {tr[0][0]:.17g} reference {c0:.17g}; |g|max {tr[0][2]:.6e} reference {ref[0]['start']['gmax']:.6e}")
    assert abs(tr[0][0] - c0) <= 1e-12 * c0
    assert abs(summ.initial_cost - c0) <= 1e-12 * c0
    judge(prob, ref, o, x_of(e), tr, f"{name} {form}")


def test_lm_iterations_and_stage_entry_points_with_priors(st):
    """lm_iterations follows the same reference; one step through the stage entry points reproduces the reduced system's step"""
    name = "a_full_all_free"
    o, prob, ref = P.options(name), P.problem(name), P.reference(name)
    e = case_engine(st, name)
    summ, tr = e.lm_iterations(P.K, st.default_options(**o))
    fails, ratios = L.compare(prob, ref, "ba", o, x_of(e), tr, fixed_mode=True)
    print("LMSTEP ba-prior lm_iterations " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    assert not fails, "; ".join(fails)
    # stages: evaluate -> blocks -> reduced system (damping as the reference's first iteration) -> solve -> back-substitute -> apply
    f = case_engine(st, name)
    f.evaluate(jac=False)
    Hcc, gc, Hpp, gp = f.normal_blocks()
    hd = np.concatenate([np.einsum("cii->ci", Hcc).reshape(-1), np.einsum("pii->pi", Hpp).reshape(-1)])
    sc = 1.0 / (1.0 + np.sqrt(hd))
    D = np.clip(sc * sc * hd, o["min_lm_diagonal"], o["max_lm_diagonal"]) / o["initial_trust_region_radius"] / (sc * sc)
    f.reduced_system(D[:6 * f.nc], D[6 * f.nc:].reshape(-1, 3), fetch=False)
    dxc = f.solve_reduced()
    dxp = f.back_substitute()
    new_cost = f.apply_step(True)
    d = np.concatenate([dxc, dxp.reshape(-1)])
    t = L.tolerances(ref, "ba", o)[0]
    err = np.linalg.norm(d - ref[0]["delta"])
    print(f"  stages: |delta - reference| {err:.3e} bound {t['delta']:.3e}; cost {new_cost:.17g} reference {ref[0]['trial_cost']:.17g}")
    assert err <= t["delta"] and abs(new_cost - ref[0]["trial_cost"]) <= t["cost"]


# ------------------------------------------------------------------------------- 4. covariance
def rel_fro(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("name", ["c_gauge_two", "d_gauge_gps"])
def test_covariance_of_a_problem_that_fixes_nothing(st, name):
    prob = P.problem(name)
    assert prob.free.all()
    r, J, cols = prob.lin(prob.x0)
    H, _ = L.normal_equations(prob.n_local, r, J, cols)
    H = H.astype(np.float64)
    ev = np.linalg.eigvalsh(H)
    kappa = ev[-1] / ev[0]
    C = np.linalg.inv(H)
    C = 0.5 * (C + C.T)
    tol = 50 * kappa * EPS
    e = case_engine(st, name)
    nc, np_ = e.nc, e.np_
    pairs = [(a, a) for a in range(nc)] + [(0, nc - 1), (2, 1)]
    cam, pb, rc = e.covariance(cam_pairs=pairs)
    cps, pps = [(0, 0), (nc - 1, 3), (2, np_ - 1)], [(0, 1), (5, 5), (np_ - 1, 2)]
    cp, pp, _ = e.cross_covariance(cps, pps, recompute=False)
    worst = 0.0
    for (a, b), blk in zip(pairs, cam):
        worst = max(worst, rel_fro(blk, C[6 * a:6 * a + 6, 6 * b:6 * b + 6]))
    for j, blk in enumerate(pb):
        o = 6 * nc + 3 * j
        worst = max(worst, rel_fro(blk, C[o:o + 3, o:o + 3]))
    for (a, j), blk in zip(cps, cp):
        worst = max(worst, rel_fro(blk, C[6 * a:6 * a + 6, 6 * nc + 3 * j:6 * nc + 3 * j + 3]))
    for (j, k), blk in zip(pps, pp):
        worst = max(worst, rel_fro(blk, C[6 * nc + 3 * j:6 * nc + 3 * j + 3, 6 * nc + 3 * k:6 * nc + 3 * k + 3]))
    print(f"  {name}: kappa(J^T J) = {kappa:.3e}, rcond {rc:.3e}, tolerance {tol:.3e}, worst relative Frobenius error {worst:.3e}")
    assert worst <= tol, (worst, tol)
    # the same scene without the priors has no gauge: the rank test refuses it, as it always has
    plain = case_engine(st, name, with_priors=False)
    with pytest.raises(st.StbaError):
        plain.covariance(points=[0])
    # and clearing the priors releases the held covariance and brings the refusal back
    e.set_pose_priors(None, None)
    with pytest.raises(st.StbaError):
        e.cross_covariance(cps, pps, recompute=False)
    with pytest.raises(st.StbaError):
        e.covariance(points=[0])


# ------------------------------------------------------------------------------- 5. unchanged without priors, reproducible with
def run_all(st, e, o, form):
    if form == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
    ev = e.evaluate()
    e.normal_blocks()
    n = 6 * e.nc
    S, rhs = e.reduced_system(np.full(n, 1e-3), np.full((e.np_, 3), 1e-3))
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=4)))
    return ev + (S, rhs, tr) + e.get_params()


@pytest.mark.parametrize("form", ["pairs", "dense"])
def test_an_engine_without_priors_is_unchanged(st, form):
    name = "a_full_all_free"
    s, cf, cams, poses, Om, W, Wobs, table = P.case(name)
    o = P.options(name)
    never = run_all(st, engine(st, s), o, form)
    e = engine(st, s)
    assert e.pose_prior_count() == 0 and e.evaluate_pose_priors()[0] == 0.0
    before = run_all(st, e, o, form)
    e.set_params(s["cams0"], s["pts0"])
    e.set_pose_priors(cams, poses, information=Om)
    with_a = run_all(st, e, o, form)
    e.set_params(s["cams0"], s["pts0"])
    e.set_pose_priors([], None)
    assert e.pose_prior_count() == 0
    cleared = run_all(st, e, o, form)
    assert same_bits(never, before) and same_bits(never, cleared)
    assert not np.array_equal(with_a[-2], never[-2])
    f = engine(st, s, pose_priors=dict(cams=cams, poses=poses, information=Om))
    with_b = run_all(st, f, o, form)
    assert same_bits(with_a, with_b), "two runs with priors differ"


# ------------------------------------------------------------------------------- 6. errors and refusals
def refused(st, code, text, fn):
    with pytest.raises(st.StbaError) as ex:
        fn()
    assert ex.value.code == code, str(ex.value)
    assert text in str(ex.value), str(ex.value)


def test_errors_leave_the_priors_as_they_were(st):
    name = "b_two_on_one"
    s, cf, cams, poses, Om, W, Wobs, table = P.case(name)
    e = case_engine(st, name)
    keep = e.evaluate_pose_priors()
    I6 = np.eye(6)
    bad = poses.copy(); bad[1, 5] = np.nan
    zq = poses.copy(); zq[1, :4] = 0.0
    nf = np.stack([I6, I6]); nf[1, 2, 3] = np.inf
    npd = np.stack([I6, I6]); npd[1, 4, 4] = -1.0
    INV = STBA_ERR_INVALID_ARGUMENT
    refused(st, INV, "prior 1: camera index", lambda: e.set_pose_priors([cams[0], e.nc], poses))
    refused(st, INV, "prior 1: camera index", lambda: e.set_pose_priors([cams[0], -1], poses))
    refused(st, INV, "prior 1: the pose has an entry that is not finite", lambda: e.set_pose_priors(cams, bad))
    refused(st, INV, "prior 1: zero quaternion", lambda: e.set_pose_priors(cams, zq))
    refused(st, INV, "prior 1: the square-root information has an entry that is not finite", lambda: e.set_pose_priors(cams, poses, sqrt_information=nf))
    refused(st, INV, "prior 1: the information matrix has an entry that is not finite", lambda: e.set_pose_priors(cams, poses, information=nf))
    refused(st, STBA_ERR_NOT_POSITIVE_DEFINITE, "prior 1: the information matrix is not positive definite", lambda: e.set_pose_priors(cams, poses, information=npd))
    with pytest.raises(ValueError):
        e.set_pose_priors(cams, poses, information=npd, sqrt_information=npd)
    L_ = st.lib()
    import ctypes as C
    c32 = np.ascontiguousarray(cams, np.int32)
    rc = L_.stba_ba_set_pose_priors(e._h, 2, c32.ctypes.data_as(C.c_void_p), poses.ctypes.data_as(C.c_void_p),
                                    npd.ctypes.data_as(C.c_void_p), npd.ctypes.data_as(C.c_void_p))
    assert rc == INV and b"not both" in L_.stba_last_error()
    assert e.pose_prior_count() == 2 and same_bits(keep, e.evaluate_pose_priors())
    summ, _ = e.solve(st.default_options(max_num_iterations=2))
    assert summ.num_iterations == 2
    # quaternions are normalised on the host; a rank-deficient W and the identity are taken
    scaled = poses.copy(); scaled[:, :4] *= 3.0
    e.set_params(s["cams0"], s["pts0"])
    e.set_pose_priors(cams, poses, sqrt_information=P.position_only_W(2))
    a = e.evaluate_pose_priors()
    e.set_pose_priors(cams, scaled, sqrt_information=P.position_only_W(2))
    b = e.evaluate_pose_priors()
    assert np.allclose(a[1], b[1], rtol=0, atol=1e-14) and np.all(a[1][:, :3] == 0.0)
    e.set_pose_priors(cams, poses)
    _, r, J = e.evaluate_pose_priors()
    rn, Jn = P.PriorBAProblem(s, cams, poses, None).lin_priors(s["cams0"])
    assert np.allclose(r, rn, rtol=0, atol=1e-13) and np.allclose(J, Jn, rtol=0, atol=1e-13)


def test_refusals_in_both_orders(st):
    name = "a_full_all_free"
    s, cf, cams, poses, Om, W, Wobs, table = P.case(name)
    INV = STBA_ERR_INVALID_ARGUMENT

    def set_pr(e):
        e.set_pose_priors(cams, poses, information=Om)

    def usable(e, n_priors):
        assert e.pose_prior_count() == n_priors
        summ, _ = e.solve(st.default_options(max_num_iterations=1))
        assert summ.num_iterations == 1

    # ITERATIVE_SCHUR (the solver is fixed at creation: one order)
    e = engine(st, s, linear_solver="iterative_schur")
    refused(st, INV, "ITERATIVE_SCHUR", lambda: set_pr(e))
    usable(e, 0)
    # DOGLEG
    e = engine(st, s); e.set_trust_region("dogleg")
    refused(st, INV, "DOGLEG", lambda: set_pr(e))
    usable(e, 0)
    e = engine(st, s); set_pr(e)
    refused(st, INV, "pose priors", lambda: e.set_trust_region("dogleg"))
    usable(e, len(cams))
    # inner iterations
    e = engine(st, s); e.set_inner_iterations(True)
    refused(st, INV, "inner iterations", lambda: set_pr(e))
    usable(e, 0)
    e = engine(st, s); set_pr(e)
    refused(st, INV, "pose priors", lambda: e.set_inner_iterations(True))
    usable(e, len(cams))
    # a host lineariser
    prob = L.ba_problem(s)

    def lin(c, p, want):
        r, Jc, Jp = prob.lin_obs(c, p, want)
        return r, Jc, Jp
    e = engine(st, s); e.set_host_linearizer(lin)
    refused(st, INV, "host lineariser", lambda: set_pr(e))
    usable(e, 0)
    e = engine(st, s); set_pr(e)
    refused(st, INV, "pose priors", lambda: e.set_host_linearizer(lin))
    usable(e, len(cams))
    # several ranks
    e = engine(st, s); e.set_allreduce(lambda user, buf, count, stream: 0, 0, 1)
    refused(st, INV, "all-reduce", lambda: set_pr(e))
    e = engine(st, s); set_pr(e)
    refused(st, INV, "pose priors", lambda: e.set_allreduce(lambda user, buf, count, stream: 0, 0, 1))
    usable(e, len(cams))
    # clearing is always allowed
    e = engine(st, s, linear_solver="iterative_schur")
    e.set_pose_priors([], None)
    usable(e, 0)
