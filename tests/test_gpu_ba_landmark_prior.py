"""Landmark position priors (control points) of the GPU bundle adjustment (include/stba.h) against
tests/ba_landmark_prior_ref.py.

  factor      evaluate_landmark_priors against the 50-digit values: per entry of r' the bound is 4 x the error the float64 numpy
              restatement shows on the same input, with the floor 4 eps x sum |W_jk| |r_k|; J' is W in every bit, 0 for a constant
              landmark; a prior at the landmark's own position gives r' = 0 exactly
  blocks      normal_blocks() Hpp, gp = the prior-less engine's + the reference's sums, each entry within 8 eps x sum |terms| (the
              existing value counts as a term); landmarks without priors, Hcc and gc keep their bits
  cost        evaluate() / cost() relative 1e-12 against the reference's longdouble sum
  gradient    the gradient max norm of iteration 0 in the trace is the reference's, where a prior's W^T r' is its largest entry
  solves      lm_step_ref.compare / tolerances on the augmented reference problem: LM on PAIRS and DENSE, the five cases;
              ITERATIVE_SCHUR in the exact limit against the direct engine and the reference, and at Ceres' default eta with all
              three preconditioners to the reference's converged cost; DOGLEG at 1, 3 and 10 iterations (dogleg_ref.compare)
  geometry    more landmarks with priors than two workgroups of the block kernel hold, plus a remainder, landmarks without between
  covariance  NO constant camera dof, priors on four landmarks: against the dense inverse of the reference's J^T J (relative
              Frobenius <= 50 kappa eps, tests/test_gpu_covariance.py); the same scene without priors is refused
  unchanged   never had priors == cleared with n = 0, bit for bit, on PAIRS, DENSE, ITERATIVE_SCHUR and DOGLEG engines
  errors      every error and refusal of include/stba.h, in both orders of the two calls
MEASURED on an MI355X (the worst err / bound each test prints): see DESIGN.md 7n."""
import ctypes as C
import functools
import importlib
import json
import os

import numpy as np
import pytest

import ba_landmark_prior_ref as R
import dogleg_ref as D
import lm_step_ref as L

pytestmark = pytest.mark.gpu

INV, NPD = -1, -4
EPS = L.EPS
LD = np.longdouble


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def engine(st, s, cam_fixed="scene", **kw):
    cf = s["cam_fixed"] if isinstance(cam_fixed, str) else cam_fixed
    return st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], cf, pt_fixed=s.get("pt_fixed"), **kw)


def case_engine(st, name, with_priors=True, **kw):
    s, points, pos, Om, W, Wobs, table, cam_priors = R.case(name)
    if Wobs is not None:
        kw["sqrt_information"] = Wobs
    if table is not None:
        kw["loss"] = dict(table)
    if cam_priors is not None:
        kw["pose_priors"] = dict(cams=cam_priors[0], poses=cam_priors[1], information=cam_priors[2])
    e = engine(st, s, **kw)
    if with_priors:
        e.set_landmark_priors(points, pos, information=Om, sqrt_information=W)
    return e


def x_of(e):
    cams, pts = e.get_params()
    return np.concatenate([cams.reshape(-1), pts.reshape(-1)])


def same_bits(x, y):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))


def ratio(err, bound):
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))


# ------------------------------------------------------------------------------- 1. the factor
@functools.lru_cache(maxsize=None)
def accuracy_setup():
    """the default scene with landmarks 0 and 5 constant; per landmark four priors: a full random W, a tight one that cancels
    (rows of +-1e6 on a position 1e-3 away), a height-only row and a W of mixed scales"""
    s = L.ba_scene()
    pf = np.zeros(len(s["pts0"]), np.uint8); pf[[0, 5]] = 1
    s = dict(s, pt_fixed=pf)
    rng = np.random.default_rng(21)
    points, pos, Ws = [], [], []
    tight = np.array([[1e6, -1e6, 0.0], [0.0, 1e6, -1e6], [1e6, 0.0, -1e6]])
    height = np.zeros((3, 3)); height[0, 2] = 50.0
    for j in range(len(s["pts0"])):
        p = s["pts0"][j]
        for W, ph in ((rng.normal(size=(3, 3)), p + rng.normal(0, 0.1, 3)), (tight, p + 1e-3 * (1.0 + 1e-9 * rng.normal(size=3))),
                      (height, p + rng.normal(0, 0.02, 3)), (rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-3, 3, (3, 3)), p + rng.normal(0, 1.0, 3))):
            points.append(j); pos.append(ph); Ws.append(W)
    return s, np.array(points, np.int32), np.array(pos), np.array(Ws)


def test_factor_against_50_digits(st):
    s, points, pos, Ws = accuracy_setup()
    # (the caller's order is not grouped by landmark)
    perm = np.random.default_rng(3).permutation(len(points))
    points, pos, Ws = points[perm], pos[perm], Ws[perm]
    e = engine(st, s)
    e.set_landmark_priors(points, pos, sqrt_information=Ws)
    assert e.landmark_prior_count() == len(points)
    cost, r, J = e.evaluate_landmark_priors()
    worst, cref = 0.0, 0.0
    for k, j in enumerate(points):
        p = s["pts0"][j]
        rm, Jm = R.lp_eval_mp(pos[k], p, Ws[k], bool(s["pt_fixed"][j]))
        rn, Jn = R.lp_eval_np(pos[k], p, Ws[k], bool(s["pt_fixed"][j]))
        ern, _ = R.err_vs_mp(rn, Jn, rm, Jm)
        er, eJ = R.err_vs_mp(r[k], J[k], rm, Jm)
        worst = max(worst, ratio(er, np.maximum(4 * ern, R.floor_r(pos[k], p, Ws[k]))))
        assert np.all(eJ == 0.0), f"prior {k}: J' is not W (or 0 for a constant landmark) in every bit"
        cref += float(sum(v * v for v in rm)) / 2
    print(f"LANDMARK PRIOR factor: worst err / bound r' {worst:.3f}; cost {cost:.17g} reference {cref:.17g} relative {abs(cost - cref) / cref:.2e}")
    fixed = s["pt_fixed"][points].astype(bool)
    assert np.all(J[fixed] == 0.0) and np.array_equal(J[~fixed], Ws[~fixed])
    assert worst <= 1.0 and abs(cost - cref) <= 1e-12 * cref


def test_a_prior_at_the_landmarks_own_position_is_exact(st):
    s = accuracy_setup()[0]
    plain, e = engine(st, s), engine(st, s)
    points = np.arange(len(s["pts0"]), dtype=np.int32)
    W = np.random.default_rng(4).normal(size=(len(points), 3, 3))
    e.set_landmark_priors(points, s["pts0"], sqrt_information=W)
    cost, r, J = e.evaluate_landmark_priors()
    free = ~s["pt_fixed"].astype(bool)
    assert cost == 0.0 and np.array_equal(r, np.zeros_like(r))
    assert np.array_equal(J, W * free[:, None, None])
    assert plain.evaluate(jac=False)[0] == e.evaluate(jac=False)[0]
    _, _, _, g0 = plain.normal_blocks()
    _, _, _, g1 = e.normal_blocks()
    assert np.array_equal(g0, g1)


# ------------------------------------------------------------------------------- 2. blocks and cost
def check_blocks_and_cost(label, plain, e, prob):
    """e: the engine with the priors of prob, plain: the same engine without; both at prob.x0"""
    c0, r0, _, _ = plain.evaluate(jac=False)
    Hc0, gc0, H0, g0 = plain.normal_blocks()
    c1, r1, _, _ = e.evaluate(jac=False)
    Hc1, gc1, H1, g1 = e.normal_blocks()
    assert same_bits((r0, Hc0, gc0), (r1, Hc1, gc1)), f"{label}: the priors changed the observations' residuals or the camera blocks"
    Hr, gr, Ha, ga = prob.landmark_blocks(prob.x0)
    eH = np.abs(H1.astype(LD) - (H0.astype(LD) + Hr)).astype(float)
    eg = np.abs(g1.astype(LD) - (g0.astype(LD) + gr)).astype(float)
    qH = ratio(eH, 8 * EPS * (np.abs(H0) + Ha.astype(float)))
    qg = ratio(eg, 8 * EPS * (np.abs(g0) + ga.astype(float)))
    without = np.setdiff1d(np.arange(prob.np_), prob.lp_pt)
    assert same_bits((H0[without], g0[without]), (H1[without], g1[without])), f"{label}: a landmark without priors changed"
    const = np.nonzero(prob.pt_fixed)[0]
    assert same_bits((H0[const], g0[const]), (H1[const], g1[const])), f"{label}: a constant landmark's blocks changed"
    assert np.array_equal(H1, np.swapaxes(H1, 1, 2)), f"{label}: Hpp is not bitwise symmetric"
    cref = prob.cost(prob.x0)
    c2 = e.cost()
    pc = e.evaluate_landmark_priors(jac=False)[0]
    pref = prob.landmark_prior_cost(prob.x0)
    print(f"LANDMARK PRIOR blocks {label}: Hpp err / bound {qH:.3f}, gp err / bound {qg:.3f}; cost relative {abs(c1 - cref) / cref:.2e} "
          f"(observations alone {c0:.6g}, priors {pc:.6g})")
    assert abs(c1 - cref) <= 1e-12 * cref and abs(c2 - cref) <= 1e-12 * cref and abs(pc - pref) <= 1e-12 * max(pref, 1e-300)
    assert qH <= 1.0 and qg <= 1.0


@pytest.mark.parametrize("name", list(R.SOLVE_CASES))
def test_blocks_and_cost(st, name):
    check_blocks_and_cost(name, case_engine(st, name, False), case_engine(st, name), R.problem(name))


def test_more_landmarks_with_priors_than_two_workgroups_hold(st):
    s = L.ba_scene(n_lm=640, n_cams=10, seed=7)
    plain, e = engine(st, s), engine(st, s)
    per_wg = e.landmark_prior_kernel_geometry()
    npt = len(s["pts0"])
    points = np.array([j for j in range(npt) if j % 8 != 3], np.int32)
    assert len(points) >= 2 * per_wg + 1 and npt % per_wg != 0 and len(points) < npt, (per_wg, npt, len(points))
    rng = np.random.default_rng(6)
    points = np.concatenate([points[::-1], points[:5]]).astype(np.int32)          # (not grouped; two on the first five)
    Om = R.random_spd3(rng, len(points))
    pos = s["pts_true"][points] + rng.normal(0, 0.05, (len(points), 3))
    e.set_landmark_priors(points, pos, information=Om)
    prob = R.LandmarkPriorBAProblem(s, points, pos, R.sqrt_of_information(Om))
    check_blocks_and_cost(f"{len(set(points.tolist()))} of {npt} landmarks with priors, {per_wg} per workgroup", plain, e, prob)
    _, r, J = e.evaluate_landmark_priors()
    rn, Jn = prob.lin_landmark_priors(prob.split(prob.x0)[1])
    assert np.allclose(r, rn, rtol=0, atol=1e-10 * np.abs(rn).max()) and np.allclose(J, Jn, rtol=1e-15, atol=0)
    # the gradient max norm over more than one workgroup's partials
    ref = L.lm_reference(prob, L.lm_options(), 1)
    _, tr = e.solve(st.default_options(max_num_iterations=1))
    g = ref[0]["start"]["gmax"]
    assert abs(tr[0][2] - g) <= L.C_PATH["ba"] * ref[0]["kappa"] * EPS * g, (tr[0][2], g)


@pytest.mark.parametrize("n", [1024, 1025, 2500])
def test_cost_form_on_both_sides_of_one_workgroup(st, n):
    """the cost form takes 1024 priors per workgroup: one workgroup writes the slot itself, more go through partials and a second
    launch.  n priors over the 32 landmarks (about n / 32 on each, the caller's order not grouped): exactly one workgroup full, one
    prior more, and a third workgroup with a remainder"""
    s = L.ba_scene()
    plain, e = engine(st, s), engine(st, s)
    rng = np.random.default_rng(n)
    points = rng.integers(0, len(s["pts0"]), n).astype(np.int32)
    Om = R.random_spd3(rng, n, sigma=0.5)
    pos = s["pts_true"][points] + rng.normal(0, 0.5, (n, 3))
    e.set_landmark_priors(points, pos, information=Om)
    assert e.landmark_prior_count() == n
    check_blocks_and_cost(f"{n} priors on {len(s['pts0'])} landmarks", plain, e, R.LandmarkPriorBAProblem(s, points, pos, R.sqrt_of_information(Om)))


@pytest.mark.parametrize("kind", ["pairs", "dense", "iterative", "dogleg"])
def test_gradient_max_norm_is_that_of_the_sum(st, kind):
    """case a_several_on_one: a prior's W^T r' is the largest entry of the gradient, 3e3 times the observations' largest -- read from
    the landmark-block kernel's own partials the norm would be theirs"""
    name = "a_several_on_one"
    ref = R.reference(name)
    e = case_engine(st, name, **(dict(linear_solver="iterative_schur") if kind == "iterative" else {}))
    if kind == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
    if kind == "dogleg":
        e.set_trust_region("dogleg")
    _, tr = e.solve(st.default_options(max_num_iterations=1))
    g = ref[0]["start"]["gmax"]
    bound = L.C_PATH["ba"] * ref[0]["kappa"] * EPS * g
    print(f"LANDMARK PRIOR gradient {kind}: |g|max of iteration 0 {tr[0][2]:.17g} reference {g:.17g} err / bound {abs(tr[0][2] - g) / bound:.3e}")
    assert abs(tr[0][2] - g) <= bound


# ------------------------------------------------------------------------------- 3. solves
def judge(prob, ref, o, x_dev, trace, label, **kw):
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["ba"] * kap * EPS <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = L.compare(prob, ref, "ba", o, x_dev, trace, **kw)
    print(f"LMSTEP ba-landmark-prior {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    assert not fails, f"{label}: " + "; ".join(fails)


@pytest.mark.parametrize("form", ["pairs", "dense"])
@pytest.mark.parametrize("name", list(R.SOLVE_CASES))
def test_exact_steps_follow_the_reference_with_priors(st, name, form):
    o, prob, ref = R.options(name), R.problem(name), R.reference(name)
    e = case_engine(st, name)
    if form == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=R.K)))
    assert summ.num_iterations == R.K and len(tr) == R.K + 1, summ.as_dict()
    c0 = ref[0]["start"]["cost"]
    assert abs(tr[0][0] - c0) <= 1e-12 * c0 and abs(summ.initial_cost - c0) <= 1e-12 * c0
    judge(prob, ref, o, x_of(e), tr, f"{name} {form}")


def test_stage_entry_points_with_priors(st):
    """evaluate -> blocks -> reduced system (damping as the reference's first iteration) -> solve -> back-substitute -> apply"""
    name = "a_several_on_one"
    o, ref = R.options(name), R.reference(name)
    f = case_engine(st, name)
    f.evaluate(jac=False)
    Hcc, gc, Hpp, gp = f.normal_blocks()
    hd = np.concatenate([np.einsum("cii->ci", Hcc).reshape(-1), np.einsum("pii->pi", Hpp).reshape(-1)])
    sc = 1.0 / (1.0 + np.sqrt(hd))
    Dg = np.clip(sc * sc * hd, o["min_lm_diagonal"], o["max_lm_diagonal"]) / o["initial_trust_region_radius"] / (sc * sc)
    f.reduced_system(Dg[:6 * f.nc], Dg[6 * f.nc:].reshape(-1, 3), fetch=False)
    dxc = f.solve_reduced()
    dxp = f.back_substitute()
    new_cost = f.apply_step(True)
    d = np.concatenate([dxc, dxp.reshape(-1)])
    t = L.tolerances(ref, "ba", o)[0]
    err = np.linalg.norm(d - ref[0]["delta"])
    print(f"LANDMARK PRIOR stages: |delta - reference| / bound {err / t['delta']:.3e}; cost err / bound {abs(new_cost - ref[0]['trial_cost']) / t['cost']:.3e}")
    assert err <= t["delta"] and abs(new_cost - ref[0]["trial_cost"]) <= t["cost"]


def test_iterative_schur_exact_limit_matches_direct_and_reference(st):
    """tests/test_gpu_iterative_schur.py's exact-limit comparison, with priors on both engines"""
    name = R.ITERATIVE_CASE
    o, prob, ref = R.options(name), R.problem(name), R.reference(name)
    opt = st.default_options(**dict(o, max_num_iterations=R.K))
    d = case_engine(st, name)
    sd, trd = d.solve(opt)
    e = case_engine(st, name, linear_solver="iterative_schur")
    e.set_pcg("jacobi", eta=1e-14, max_iterations=max(6 * prob.nc, 10) * 4)
    se, tre = e.solve(opt)
    assert se.num_iterations == sd.num_iterations and se.num_successful_steps == sd.num_successful_steps, (se.as_dict(), sd.as_dict())
    assert np.array_equal(tre[:, 6], trd[:, 6]), "accept/reject decisions differ"
    np.testing.assert_allclose(tre[:, 5], trd[:, 5], rtol=1e-12)           # radii
    np.testing.assert_allclose(tre[:, 0], trd[:, 0], rtol=1e-9)
    np.testing.assert_allclose(tre[:, 3], trd[:, 3], rtol=1e-6, atol=1e-14)
    judge(prob, ref, o, x_of(e), tre, f"{name} iterative exact limit", eps_eff=1e-9)


@pytest.mark.parametrize("pc", ["identity", "jacobi", "schur_jacobi"])
def test_iterative_schur_at_ceres_default_eta(st, pc):
    name = R.ITERATIVE_CASE
    prob = R.problem(name)
    converged = L.lm_reference(prob, R.options(name), 12)[-1]["cost"]
    e = case_engine(st, name, linear_solver="iterative_schur")
    e.set_pcg(pc, eta=0.1, max_iterations=500)
    opt = st.default_options(max_num_iterations=100)
    se, tr = e.solve(opt)
    print(f"LANDMARK PRIOR iterative {pc}: {se.num_iterations} iterations, cost {se.final_cost:.12e}, reference converged {converged:.12e}, "
          f"relative {abs(se.final_cost - converged) / converged:.2e}; pcg {e.pcg_summary().as_dict()}")
    assert se.termination_type == 0, se.as_dict()
    assert abs(se.final_cost - converged) <= opt.function_tolerance * converged


@pytest.mark.parametrize("form", ["pairs", "dense"])
@pytest.mark.parametrize("k", [1, 3, 10])
def test_dogleg_follows_the_reference_with_priors(st, k, form):
    prob, o = R.problem(R.DOGLEG_CASE), R.options(R.DOGLEG_CASE)
    full = R.dogleg_reference(10)
    assert {it["case"] for it in full} == {0, 1, 2} and sum(1 for it in full if not it["accepted"]) >= 1
    ref = full[:k]
    e = case_engine(st, R.DOGLEG_CASE)
    e.set_trust_region("dogleg")
    if form == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=k)))
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["ba"] * kap * EPS <= 1e-6 and L.rho_margin_ok(ref, o)
    fails, ratios = D.compare(prob, ref, o, x_of(e), tr)
    print(f"DOGLEG landmark-prior {form} k={k} kappa={kap:.2e} " + " ".join(f"{n}={v:.2e}" for n, v in sorted(ratios.items())))
    assert not fails, "; ".join(fails)
    assert list(e.dogleg_summary().steps_by_case) == [sum(1 for it in ref if it["case"] == c) for c in range(3)]


# ------------------------------------------------------------------------------- 4. gauge and covariance
def rel_fro(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_covariance_of_a_problem_whose_gauge_is_four_control_points(st):
    s, points, pos, W = R.gauge_case()
    prob = R.gauge_problem()
    assert prob.free.all()
    r, J, cols = prob.lin(prob.x0)
    H, _ = L.normal_equations(prob.n_local, r, J, cols)
    H = H.astype(np.float64)
    ev = np.linalg.eigvalsh(H)
    kappa = ev[-1] / ev[0]
    Cv = np.linalg.inv(H)
    Cv = 0.5 * (Cv + Cv.T)
    tol = 50 * kappa * EPS
    assert tol <= 1e-6
    e = engine(st, s, cam_fixed=None)
    e.set_landmark_priors(points, pos, sqrt_information=W)
    nc, np_ = e.nc, e.np_
    pairs = [(a, a) for a in range(nc)] + [(0, nc - 1), (2, 1)]
    cam, pb, rc = e.covariance(cam_pairs=pairs)
    j0, j1 = int(points[0]), int(points[1])
    cps, pps = [(0, 0), (nc - 1, j0), (2, np_ - 1)], [(0, 1), (j0, j0), (j0, j1), (np_ - 1, 2)]
    cp, pp, _ = e.cross_covariance(cps, pps, recompute=False)
    worst = 0.0
    for (a, b), blk in zip(pairs, cam):
        worst = max(worst, rel_fro(blk, Cv[6 * a:6 * a + 6, 6 * b:6 * b + 6]))
    for j, blk in enumerate(pb):
        o = 6 * nc + 3 * j
        worst = max(worst, rel_fro(blk, Cv[o:o + 3, o:o + 3]))
    for (a, j), blk in zip(cps, cp):
        worst = max(worst, rel_fro(blk, Cv[6 * a:6 * a + 6, 6 * nc + 3 * j:6 * nc + 3 * j + 3]))
    for (j, k), blk in zip(pps, pp):
        worst = max(worst, rel_fro(blk, Cv[6 * nc + 3 * j:6 * nc + 3 * j + 3, 6 * nc + 3 * k:6 * nc + 3 * k + 3]))
    print(f"LANDMARK PRIOR covariance: kappa(J^T J) = {kappa:.3e}, rcond {rc:.3e}, worst relative Frobenius error / (50 kappa eps) {worst / tol:.3e}")
    assert worst <= tol, (worst, tol)
    plain = engine(st, s, cam_fixed=None)
    with pytest.raises(st.StbaError):
        plain.covariance(points=[0])
    e.set_landmark_priors(None, None)
    with pytest.raises(st.StbaError):
        e.cross_covariance(cps, pps, recompute=False)
    with pytest.raises(st.StbaError):
        e.covariance(points=[0])


# ------------------------------------------------------------------------------- 5. unchanged without priors, reproducible with
def make(st, s, kind, **kw):
    e = engine(st, s, **(dict(kw, linear_solver="iterative_schur") if kind == "iterative" else kw))
    if kind == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
    if kind == "dogleg":
        e.set_trust_region("dogleg")
    if kind == "iterative":
        e.set_pcg("schur_jacobi", eta=0.1)
    return e


def run3(st, e, o):
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=3)))
    return (tr,) + e.get_params()


@pytest.mark.parametrize("kind", ["pairs", "dense", "iterative", "dogleg"])
def test_an_engine_without_priors_is_unchanged_and_one_with_is_reproducible(st, kind):
    name = "a_several_on_one"
    s, points, pos, Om, *_ = R.case(name)
    o = R.options(name)
    never = run3(st, make(st, s, kind), o)
    e = make(st, s, kind)
    assert e.landmark_prior_count() == 0 and e.evaluate_landmark_priors()[0] == 0.0
    e.set_landmark_priors(points, pos, information=Om)
    with_a = run3(st, e, o)
    e.set_params(s["cams0"], s["pts0"])
    e.set_landmark_priors([], None)
    assert e.landmark_prior_count() == 0
    cleared = run3(st, e, o)
    assert same_bits(never, cleared), "cleared with n = 0 is not the engine that never had priors"
    assert not np.array_equal(with_a[2], never[2])
    f = make(st, s, kind, landmark_priors=dict(points=points, positions=pos, information=Om))
    assert same_bits(with_a, run3(st, f, o)), "two solves with priors differ"


# ------------------------------------------------------------------------------- 6. errors and refusals
def refused(st, code, text, fn):
    with pytest.raises(st.StbaError) as ex:
        fn()
    assert ex.value.code == code, str(ex.value)
    assert text in str(ex.value), str(ex.value)


def test_errors_leave_the_priors_as_they_were(st):
    name = "b_on_fixed"
    s, points, pos, Om, *_ = R.case(name)
    e = case_engine(st, name)
    n = len(points)
    keep = e.evaluate_landmark_priors()
    before = e.get_params()
    I3 = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    bad = pos.copy(); bad[1, 2] = np.nan
    nf = I3.copy(); nf[1, 0, 2] = np.inf
    npd = I3.copy(); npd[1, 1, 1] = -1.0
    sing = I3.copy(); sing[1] = np.ones((3, 3))
    idx = points.copy(); idx[1] = e.np_
    neg = points.copy(); neg[1] = -1; neg[3] = e.np_
    who = "stba_ba_set_landmark_priors: prior 1: "
    refused(st, INV, who + f"landmark index {e.np_} out of range", lambda: e.set_landmark_priors(idx, pos))
    refused(st, INV, who + "landmark index -1 out of range", lambda: e.set_landmark_priors(neg, pos))
    refused(st, INV, who + "the position has an entry that is not finite", lambda: e.set_landmark_priors(points, bad))
    refused(st, INV, who + "the square-root information has an entry that is not finite", lambda: e.set_landmark_priors(points, pos, sqrt_information=nf))
    refused(st, INV, who + "the information matrix has an entry that is not finite", lambda: e.set_landmark_priors(points, pos, information=nf))
    refused(st, NPD, who + "the information matrix is not positive definite", lambda: e.set_landmark_priors(points, pos, information=npd))
    refused(st, NPD, who + "the information matrix is not positive definite", lambda: e.set_landmark_priors(points, pos, information=sing))
    with pytest.raises(ValueError):
        e.set_landmark_priors(points, pos, information=I3, sqrt_information=I3)
    lib = st.lib()
    p32 = np.ascontiguousarray(points, np.int32)
    rc = lib.stba_ba_set_landmark_priors(e._h, n, p32.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p),
                                         I3.ctypes.data_as(C.c_void_p), I3.ctypes.data_as(C.c_void_p))
    assert rc == INV and b"not both" in lib.stba_last_error()
    assert e.landmark_prior_count() == n
    # (n = 0 clears and is never refused, whatever the pointers: on an engine of its own)
    g = case_engine(st, name)
    assert lib.stba_ba_set_landmark_priors(g._h, 0, None, None, I3.ctypes.data_as(C.c_void_p), I3.ctypes.data_as(C.c_void_p)) == 0
    assert g.landmark_prior_count() == 0
    assert e.landmark_prior_count() == n and same_bits(keep, e.evaluate_landmark_priors()) and same_bits(before, e.get_params())
    summ, _ = e.solve(st.default_options(max_num_iterations=2))
    assert summ.num_iterations == 2
    # a rank-deficient W, the identity, one matrix for all, sigmas
    e.set_params(s["cams0"], s["pts0"])
    h = np.zeros((3, 3)); h[0, 2] = 50.0
    e.set_landmark_priors(points, pos, sqrt_information=h)
    _, r, J = e.evaluate_landmark_priors()
    free = ~s["pt_fixed"][points].astype(bool)
    assert np.all(r[:, 1:] == 0.0) and np.array_equal(J[free], np.broadcast_to(h, (free.sum(), 3, 3)))
    e.set_landmark_priors(points, pos)
    _, r, J = e.evaluate_landmark_priors()
    assert np.array_equal(r, s["pts0"][points] - pos) and np.array_equal(J[free], np.broadcast_to(np.eye(3), (free.sum(), 3, 3)))
    sig = np.linspace(0.5, 2.0, n)
    e.set_landmark_priors(points, pos, sqrt_information=sig)
    a = e.evaluate_landmark_priors()
    e.set_landmark_priors(points, pos, information=sig)
    b = e.evaluate_landmark_priors()
    assert np.array_equal(a[2][free], (np.eye(3)[None] / sig[:, None, None])[free]) and np.allclose(a[1], b[1], rtol=4 * EPS, atol=0)


def test_refusals_in_both_orders(st):
    name = "a_several_on_one"
    s, points, pos, Om, *_ = R.case(name)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_refusals_landmark_priors.json")) as f:
        rows = {(row["asker"], row["held"][0]): row["text"] for row in json.load(f)["rows"]}
    assert len(rows) == 7

    def set_lp(e):
        e.set_landmark_priors(points, pos, information=Om)

    def usable(e, n_priors, before=None):
        assert e.landmark_prior_count() == n_priors
        if before is not None:
            assert same_bits(before, e.get_params())
        summ, _ = e.solve(st.default_options(max_num_iterations=1))
        assert summ.num_iterations == 1

    setter = "stba_ba_set_landmark_priors"
    # inner iterations
    e = engine(st, s); e.set_inner_iterations(True)
    refused(st, INV, f"{setter}: " + rows[(setter, "INNER_ITERATIONS")], lambda: set_lp(e))
    usable(e, 0, (s["cams0"], s["pts0"]))
    e = engine(st, s); set_lp(e)
    refused(st, INV, "stba_ba_set_inner_iterations: " + rows[("stba_ba_set_inner_iterations", "LANDMARK_PRIORS")], lambda: e.set_inner_iterations(True))
    refused(st, INV, "stba_ba_inner_sweep: " + rows[("stba_ba_inner_sweep", "LANDMARK_PRIORS")], lambda: e.inner_sweep())
    usable(e, len(points), (s["cams0"], s["pts0"]))
    # a host lineariser
    prob = L.ba_problem(s)

    def lin(c, p, want):
        return prob.lin_obs(c, p, want)
    e = engine(st, s); e.set_host_linearizer(lin)
    refused(st, INV, f"{setter}: " + rows[(setter, "HOST_LINEARIZER")], lambda: set_lp(e))
    usable(e, 0, (s["cams0"], s["pts0"]))
    e = engine(st, s); set_lp(e)
    refused(st, INV, "stba_ba_set_host_linearizer: " + rows[("stba_ba_set_host_linearizer", "LANDMARK_PRIORS")], lambda: e.set_host_linearizer(lin))
    usable(e, len(points), (s["cams0"], s["pts0"]))
    # an all-reduce hook
    e = engine(st, s); e.set_allreduce(lambda user, buf, count, stream: 0, 0, 1)
    refused(st, INV, f"{setter}: " + rows[(setter, "ALLREDUCE")], lambda: set_lp(e))
    assert e.landmark_prior_count() == 0
    e = engine(st, s); set_lp(e)
    refused(st, INV, "stba_ba_set_allreduce: " + rows[("stba_ba_set_allreduce", "LANDMARK_PRIORS")],
            lambda: e.set_allreduce(lambda user, buf, count, stream: 0, 0, 1))
    usable(e, len(points), (s["cams0"], s["pts0"]))
    # clearing is never refused; ITERATIVE_SCHUR, DOGLEG, pose priors and relative poses take the priors
    e = engine(st, s); e.set_inner_iterations(True)
    e.set_landmark_priors([], None)
    usable(e, 0)
    e = engine(st, s, linear_solver="iterative_schur"); set_lp(e); usable(e, len(points))
    e = engine(st, s); e.set_trust_region("dogleg"); set_lp(e); usable(e, len(points))
    e = engine(st, s); set_lp(e); e.set_trust_region("dogleg"); usable(e, len(points))
