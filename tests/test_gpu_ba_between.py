"""Camera-to-camera relative-pose factors of the GPU bundle adjustment (include/stba.h) against tests/ba_between_ref.py.

  factor      evaluate_relative_poses against the 50-digit values on ba_between_ref.grid() -- every angle of the error rotation, each
              of the three quaternions negated, a full random and a position-only W, every pair of constant-dof mask kinds,
              t_j - t_i small and ~10 units -- under ba_between_ref's bound: per entry 4 x the float64 restatement's own error on that
              input, floor C_FLOOR eps sum |W_jk||entry_k|.  Negating the quaternions again gives identical bits; the cost is within
              1e-15 relative of the longdouble sum of the device's own r'^2.
  blocks      at one point, normal_blocks and reduced_system with dc = dp = 0, with and without edges, PAIRS and DENSE: Hcc, gc within
              8 eps sum |terms| of (edge-less + reference sums); every lower-triangle entry of S against (edge-less S in longdouble)
              + (reference sum J_hi'^T J_lo', on the diagonal sum J_x'^T J_x') within 8 eps sum |terms| + eps |S|, the terms the
              edges' products; rhs against (edge-less rhs - reference sum J_x'^T r') within 8 eps (sum |terms| + |gc|) + eps |rhs|: gc,
              which the edges' sum is added to before rhs takes it, counts as a term as in 7j; pairs without an edge keep their bits
  no accumulation  two builds at one point: the same bits; cleared with n = 0: the edge-less engine's bits
  solves      lm_step_ref.compare / tolerances on the augmented reference problem, PAIRS and DENSE, ba_between_ref.SOLVE_CASES
  covariance  against the dense inverse of the reference's J^T J (relative Frobenius <= 50 kappa eps)
  unchanged   never had edges == cleared with n = 0 == before set_relative_poses, bit for bit
  errors      every error and refusal of include/stba.h, in both orders of the two calls"""
import ctypes as C
import importlib

import numpy as np
import pytest

import ba_between_ref as T
import ba_prior_ref as P
import lm_step_ref as L

pytestmark = pytest.mark.gpu

STBA_ERR_INVALID_ARGUMENT, STBA_ERR_NOT_POSITIVE_DEFINITE = -1, -4
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


def case_engine(st, name, with_edges=True, with_priors=True):
    c = T.case(name)
    kw = {}
    if c["Wobs"] is not None:
        kw["sqrt_information"] = c["Wobs"]
    if c["table"] is not None:
        kw["loss"] = dict(c["table"])
    e = engine(st, c["s"], cam_fixed=c["cam_fixed"], **kw)
    if with_priors and c["priors"] is not None:
        e.set_pose_priors(**c["priors"])
    if with_edges:
        e.set_relative_poses(c["cam_i"], c["cam_j"], c["meas"], information=c["information"], sqrt_information=c["sqrt_information"])
    return e


def x_of(e):
    cams, pts = e.get_params()
    return np.concatenate([cams.reshape(-1), pts.reshape(-1)])


def same_bits(x, y):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))


def ratio(err, bound):
    """max err / bound; an entry whose bound is 0 must be exact"""
    err, bound = np.asarray(err, float), np.asarray(bound, float)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))))


# ------------------------------------------------------------------------------- 1. the factor
def test_factor_against_50_digits_on_the_grid(st):
    g = T.grid()
    n, nc = len(g["meas"]), len(g["cams"])
    # (one landmark per edge that its two cameras "observe": the factor reads the cameras only, nothing is linearised)
    pts = np.random.default_rng(3).normal(size=(n, 3))
    oc = np.arange(nc, dtype=np.int32)
    op = (np.arange(nc) // 2).astype(np.int32)
    e = st.BAEngine(g["cams"], pts, oc, op, np.zeros((nc, 2)), g["cam_fixed"])
    assert np.array_equal(e.get_params()[0], g["cams"])
    e.set_relative_poses(g["cam_i"], g["cam_j"], g["meas"], sqrt_information=g["W"])
    assert e.relative_pose_count() == n
    cost, r, Ji, Jj = e.evaluate_relative_poses()
    worst, at, same = 0.0, None, 0
    for k in range(n):
        i, j = g["cam_i"][k], g["cam_j"][k]
        assert np.all(Ji[k][:, g["cam_fixed"][i].astype(bool)] == 0.0) and np.all(Jj[k][:, g["cam_fixed"][j].astype(bool)] == 0.0), g["names"][k]
        q = T.worst_ratio(k, (r[k], Ji[k], Jj[k]))
        z = g["meas"][k].copy(); z[:4] = P.normalise_like_the_host(z[None, :4])[0]
        same += same_bits((r[k], Ji[k], Jj[k]), T.between_eval_np(z, g["cams"][i], g["cams"][j], g["W"][k], g["cam_fixed"][i], g["cam_fixed"][j]))
        if q > worst:
            worst, at = q, g["names"][k]
    want = float(0.5 * np.sum(r.astype(LD) ** 2))
    print(f"BETWEEN factor: worst err / bound {worst:.3f} at {at}; {same} of {n} edges agree with the float64 restatement in every bit; "
          f"cost {cost:.17g} longdouble sum {want:.17g} relative {abs(cost - want) / want:.2e}")
    assert worst <= 1.0
    assert abs(cost - want) <= 1e-15 * want
    c2, r2, _, _ = e.evaluate_relative_poses(jac=False)
    assert c2 == cost and np.array_equal(r2, r)
    # each of the three quaternions negated (in every edge at once): identical bits
    base = (cost, r, Ji, Jj)
    for which in ("i", "j", "meas"):
        cams, meas = g["cams"].copy(), g["meas"].copy()
        if which == "i":
            cams[g["cam_i"], :4] *= -1.0
        elif which == "j":
            cams[g["cam_j"], :4] *= -1.0
        else:
            meas[:, :4] *= -1.0
        e.set_params(cams, pts)
        e.set_relative_poses(g["cam_i"], g["cam_j"], meas, sqrt_information=g["W"])
        assert same_bits(base, e.evaluate_relative_poses()), f"negating q_{which} changed bits"
    # angle exactly 0: the rotation residual is exactly 0 (seen through an identity W)
    zero = [k for k in range(n) if g["names"][k].startswith("0/")]
    e.set_params(g["cams"], pts)
    e.set_relative_poses(g["cam_i"][zero], g["cam_j"][zero], g["meas"][zero])
    assert np.array_equal(e.evaluate_relative_poses()[1][:, :3], np.zeros((len(zero), 3)))


# ------------------------------------------------------------------------------- 2. blocks
def build(e, form):
    """(Hcc, gc, S, rhs) at the engine's point with dc = dp = 0"""
    if form == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
    e.evaluate(jac=False)
    Hcc, gc, _, _ = e.normal_blocks()
    S, rhs = e.reduced_system(np.zeros(6 * e.nc), np.zeros((e.np_, 3)))
    return Hcc, gc, S, rhs


def check_blocks(st, label, s, cf, ci, cj, meas, W, form, zero_pairs=()):
    plain, e = engine(st, s, cam_fixed=cf), engine(st, s, cam_fixed=cf)
    e.set_relative_poses(ci, cj, meas, sqrt_information=W)
    prob = T.BetweenBAProblem(s, ci, cj, meas, W, cam_fixed=cf)
    H0, g0, S0, r0 = build(plain, form)
    H1, g1, S1, r1 = build(e, form)
    Hr, gr, Ha, ga, Sr = prob.edge_blocks(prob.x0)
    nc = prob.nc
    qH = ratio(np.abs(H1.astype(LD) - (H0.astype(LD) + Hr)), 8 * EPS * (np.abs(H0) + Ha.astype(float)))
    qg = ratio(np.abs(g1.astype(LD) - (g0.astype(LD) + gr)), 8 * EPS * (np.abs(g0) + ga.astype(float)))
    assert np.array_equal(H1, np.swapaxes(H1, 1, 2)), f"{label}: Hcc is not bitwise symmetric"
    qS, untouched = 0.0, 0
    for hi in range(nc):
        for lo in range(hi + 1):
            a, b = slice(6 * hi, 6 * hi + 6), slice(6 * lo, 6 * lo + 6)
            tri = np.tril(np.ones((6, 6), bool)) if hi == lo else np.ones((6, 6), bool)
            if hi == lo:
                add, terms = Hr[hi], Ha[hi].astype(float)
            elif (hi, lo) in Sr:
                add, terms = Sr[(hi, lo)][0], Sr[(hi, lo)][1].astype(float)
            else:
                assert np.array_equal(S1[a, b], S0[a, b]), f"{label}: block ({hi}, {lo}) has no edge and changed"
                untouched += 1
                continue
            if not np.any(terms):
                assert np.array_equal(S1[a, b][tri], S0[a, b][tri])
                continue
            err = np.abs(S1[a, b].astype(LD) - (S0[a, b].astype(LD) + add)).astype(float)
            qS = max(qS, ratio(err[tri], (8 * EPS * terms + EPS * np.abs(S1[a, b]))[tri]))
    qr = ratio(np.abs(r1.astype(LD) - (r0.astype(LD) - gr.reshape(-1))), 8 * EPS * (ga.astype(float) + np.abs(g0)).reshape(-1) + EPS * np.abs(r1))
    for hi, lo in zero_pairs:
        assert (hi, lo) in Sr and np.array_equal(S0[6 * hi:6 * hi + 6, 6 * lo:6 * lo + 6], np.zeros((6, 6))), f"{label}: S without edges is not 0 at ({hi}, {lo})"
        assert np.abs(S1[6 * hi:6 * hi + 6, 6 * lo:6 * lo + 6]).max() > 0
    # constant dofs: their rows and columns of S are exactly 0 off the diagonal
    fixed = np.nonzero(prob.cam_fixed.reshape(-1))[0]
    lower = np.tril(S1)
    for d in fixed:
        assert np.all(lower[d, :d] == 0.0) and np.all(lower[d + 1:, d] == 0.0), f"{label}: constant dof {d} couples to something"
    without = np.setdiff1d(np.arange(nc), np.concatenate([prob.bt_i, prob.bt_j]))
    assert same_bits((H0[without], g0[without]), (H1[without], g1[without])), f"{label}: a camera without edges changed"
    print(f"  {label} {form}: err / bound Hcc {qH:.3f} gc {qg:.3f} S {qS:.3f} rhs {qr:.3f}; {untouched} blocks without an edge keep their bits")
    assert qH <= 1.0 and qg <= 1.0 and qS <= 1.0 and qr <= 1.0
    cref = prob.cost(prob.x0)
    assert abs(e.cost() - cref) <= 1e-12 * cref
    return e, (H1, g1, S1, r1)


def smallest_cases():
    """the disjoint scene with camera 3's mask [0, 1, 0, 0, 1, 0] (camera 0 is constant in the scene): the loop closure (b, a) on the
    pair that shares no landmark, written i > j; (2, 4) and (4, 2) on one pair; (0, 2) onto the constant camera; (3, 5) onto the mixed
    mask; camera 2 has three edges"""
    s, (a, b) = T.disjoint_scene()
    cf = s["cam_fixed"].copy()
    assert cf[0].all() and not cf[1:7].any()
    cf[3] = T.MASKS["mixed"]
    ci, cj = np.array([b, 2, 4, 0, 3], np.int32), np.array([a, 4, 2, 2, 5], np.int32)
    assert a not in (0, 3) and b not in (0, 3)
    rng = np.random.default_rng(41)
    meas = T.odometry(s, ci, cj, rng)
    W = P.sqrt_of_information(P.random_spd(rng, len(ci), rot_sigma=0.01, pos_sigma=0.02))
    return s, cf, ci, cj, meas, W, (b, a)


@pytest.mark.parametrize("form", ["pairs", "dense"])
def test_blocks_of_the_smallest_cases_that_can_go_wrong(st, form):
    s, cf, ci, cj, meas, W, dis = smallest_cases()
    e, _ = check_blocks(st, "disjoint pair, both directions, constant and mixed cameras", s, cf, ci, cj, meas, W, form,
                        zero_pairs=[dis] if form == "pairs" else [])
    if form == "dense":
        # (the dense product computes the block of the pair without a common landmark from zero columns: 0 as well)
        plain = engine(st, s, cam_fixed=cf)
        S0 = build(plain, form)[2]
        assert np.array_equal(S0[6 * dis[0]:6 * dis[0] + 6, 6 * dis[1]:6 * dis[1] + 6], np.zeros((6, 6)))
    _, _, Ji, Jj = e.evaluate_relative_poses()
    assert np.array_equal(Ji[3], np.zeros((6, 6))) and np.abs(Jj[3]).max() > 0          # the edge onto the constant camera


@pytest.mark.parametrize("form", ["pairs", "dense"])
def test_more_groups_than_two_workgroups_hold(st, form):
    """cameras with edges and pairs with edges: each more than 2 x (groups per workgroup), neither a multiple of it, the caller's order
    not grouped"""
    s = L.ba_scene(n_cams=12)
    per_wg = engine(st, s).relative_pose_kernel_geometry()
    nc = len(s["cams0"])
    ci, cj = np.arange(nc - 2, -1, -1, dtype=np.int32), np.arange(nc - 1, 0, -1, dtype=np.int32)      # a chain, listed backwards
    ci, cj = np.append(ci, [5, 1, 10]).astype(np.int32), np.append(cj, [4, 9, 3]).astype(np.int32)   # a repeat (reversed) and two closures
    n_pairs = len({(max(a, b), min(a, b)) for a, b in zip(ci, cj)})
    assert len(set(ci.tolist()) | set(cj.tolist())) == nc
    assert nc > 2 * per_wg and n_pairs > 2 * per_wg and (nc + n_pairs) % per_wg != 0, (nc, n_pairs, per_wg)
    rng = np.random.default_rng(43)
    meas = T.odometry(s, ci, cj, rng)
    W = P.sqrt_of_information(P.random_spd(rng, len(ci), rot_sigma=0.01, pos_sigma=0.02))
    check_blocks(st, f"{nc} cameras and {n_pairs} pairs with edges, {per_wg} groups per workgroup", s, s["cam_fixed"], ci, cj, meas, W, form)


# ------------------------------------------------------------------------------- 3. no accumulation
@pytest.mark.parametrize("form", ["pairs", "dense"])
def test_a_second_build_at_the_same_point_gives_the_same_bits(st, form):
    s, cf, ci, cj, meas, W, _ = smallest_cases()
    e = engine(st, s, cam_fixed=cf)
    e.set_relative_poses(ci, cj, meas, sqrt_information=W)
    first = build(e, form)
    S2, rhs2 = e.reduced_system(np.zeros(6 * e.nc), np.zeros((e.np_, 3)))
    assert same_bits(first[2:], (S2, rhs2)), "a second reduced_system at the same point differs"
    H2, g2, _, _ = e.normal_blocks()
    assert same_bits(first[:2], (H2, g2))
    assert same_bits(first, build(e, form))
    plain = build(engine(st, s, cam_fixed=cf), form)
    assert not np.array_equal(first[2], plain[2])
    e.set_relative_poses([], None, None)
    assert e.relative_pose_count() == 0
    assert same_bits(plain, build(e, form)), "cleared with n = 0: not the edge-less engine's bits"


# ------------------------------------------------------------------------------- 4. solves
def judge(prob, ref, o, x_dev, trace, label):
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = L.compare(prob, ref, "ba", o, x_dev, trace)
    print(f"LMSTEP ba-between {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    assert not fails, f"{label}: " + "; ".join(fails)


@pytest.mark.parametrize("form", ["pairs", "dense"])
@pytest.mark.parametrize("name", list(T.SOLVE_CASES))
def test_exact_steps_follow_the_reference_with_edges(st, name, form):
    o = T.options(name)
    prob, ref = T.problem(name), T.reference(name)
    e = case_engine(st, name)
    if form == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
        assert e.schur_mode() == e.SCHUR_DENSE
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=T.K)))
    assert summ.num_iterations == T.K and len(tr) == T.K + 1, summ.as_dict()
    c0 = ref[0]["start"]["cost"]
    print(f"  {name} {form}: start cost {tr[0][0]:.17g} reference {c0:.17g}; |g|max {tr[0][2]:.6e} reference {ref[0]['start']['gmax']:.6e}")
    assert abs(tr[0][0] - c0) <= 1e-12 * c0
    assert abs(summ.initial_cost - c0) <= 1e-12 * c0
    judge(prob, ref, o, x_of(e), tr, f"{name} {form}")


def test_lm_iterations_and_stage_entry_points_with_edges(st):
    """lm_iterations follows the same reference; one step through the stage entry points reproduces the reduced system's step"""
    name = "b_chain_loop_disjoint"
    o, prob, ref = T.options(name), T.problem(name), T.reference(name)
    e = case_engine(st, name)
    summ, tr = e.lm_iterations(T.K, st.default_options(**o))
    fails, ratios = L.compare(prob, ref, "ba", o, x_of(e), tr, fixed_mode=True)
    print("LMSTEP ba-between lm_iterations " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
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
    print(f"  stages: |delta - reference| {err:.3e} bound {t['delta']:.3e}; cost {new_cost:.17g} reference {ref[0]['trial_cost']:.17g}; the loop's trial cost {tr[1][0]:.17g}")
    assert err <= t["delta"] and abs(new_cost - ref[0]["trial_cost"]) <= t["cost"]
    assert abs(new_cost - tr[1][0]) <= 2 * t["cost"]


# ------------------------------------------------------------------------------- 5. covariance
def rel_fro(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_covariance_with_one_prior_and_a_chain(st):
    """nothing constant: without edges and priors the rank test refuses the scene; one prior (six of the seven gauge freedoms) plus the
    chain of edges (whose measured translations hold the scale) makes the covariance well defined"""
    c = T.case("c_chain_two_priors")
    s = c["s"]
    one = dict(cams=c["priors"]["cams"][:1], poses=c["priors"]["poses"][:1], information=c["priors"]["information"][:1])
    W, Wp = T.case_W("c_chain_two_priors"), P.sqrt_of_information(one["information"])
    prob = T.BetweenPriorBAProblem(s, c["cam_i"], c["cam_j"], c["meas"], W, one["cams"], one["poses"], Wp, cam_fixed=None)
    assert prob.free.all()
    r, J, cols = prob.lin(prob.x0)
    H, _ = L.normal_equations(prob.n_local, r, J, cols)
    H = H.astype(np.float64)
    ev = np.linalg.eigvalsh(H)
    kappa = ev[-1] / ev[0]
    Cv = np.linalg.inv(H)
    Cv = 0.5 * (Cv + Cv.T)
    tol = 50 * kappa * EPS
    e = engine(st, s, cam_fixed=None, pose_priors=one,
               relative_poses=dict(cam_i=c["cam_i"], cam_j=c["cam_j"], measurements=c["meas"], information=c["information"]))
    nc, np_ = e.nc, e.np_
    pairs = [(a, a) for a in range(nc)] + [(0, nc - 1), (2, 1)]
    cam, pb, rc = e.covariance(cam_pairs=pairs)
    cps, pps = [(0, 0), (nc - 1, 3), (2, np_ - 1)], [(0, 1), (5, 5), (np_ - 1, 2)]
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
    print(f"  one prior + chain: kappa(J^T J) = {kappa:.3e}, rcond {rc:.3e}, tolerance {tol:.3e}, worst relative Frobenius error {worst:.3e}")
    assert worst <= tol, (worst, tol)
    # the same scene without edges and priors has no gauge: the rank test refuses it, as it always has
    with pytest.raises(st.StbaError):
        engine(st, s, cam_fixed=None).covariance(points=[0])
    # clearing the edges releases the held covariance
    e.set_relative_poses(None, None, None)
    with pytest.raises(st.StbaError):
        e.cross_covariance(cps, pps, recompute=False)


# ------------------------------------------------------------------------------- 6. unchanged without edges, reproducible with
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
def test_an_engine_without_edges_is_unchanged(st, form):
    name = "a_chain"
    c, o = T.case(name), T.options(name)
    s = c["s"]
    edges = dict(cam_i=c["cam_i"], cam_j=c["cam_j"], measurements=c["meas"], information=c["information"])
    never = run_all(st, engine(st, s), o, form)
    e = engine(st, s)
    assert e.relative_pose_count() == 0 and e.evaluate_relative_poses()[0] == 0.0
    before = run_all(st, e, o, form)
    e.set_params(s["cams0"], s["pts0"])
    e.set_relative_poses(**edges)
    with_a = run_all(st, e, o, form)
    e.set_params(s["cams0"], s["pts0"])
    e.set_relative_poses([], None, None)
    assert e.relative_pose_count() == 0
    cleared = run_all(st, e, o, form)
    assert same_bits(never, before) and same_bits(never, cleared)
    assert not np.array_equal(with_a[-2], never[-2])
    with_b = run_all(st, engine(st, s, relative_poses=edges), o, form)
    assert same_bits(with_a, with_b), "two runs with edges differ"


# ------------------------------------------------------------------------------- 7. errors and refusals
def refused(st, code, text, fn):
    with pytest.raises(st.StbaError) as ex:
        fn()
    assert ex.value.code == code, str(ex.value)
    assert text in str(ex.value), str(ex.value)


def test_errors_leave_the_edges_as_they_were(st):
    name = "a_chain"
    c = T.case(name)
    s, ci, cj, meas = c["s"], c["cam_i"][:2], c["cam_j"][:2], c["meas"][:2]
    e = engine(st, s)
    e.set_relative_poses(ci, cj, meas, information=c["information"][:2])
    keep = e.evaluate_relative_poses()
    I6 = np.eye(6)
    bad = meas.copy(); bad[1, 5] = np.nan
    zq = meas.copy(); zq[1, :4] = 0.0
    nf = np.stack([I6, I6]); nf[1, 2, 3] = np.inf
    npd = np.stack([I6, I6]); npd[1, 4, 4] = -1.0
    INV = STBA_ERR_INVALID_ARGUMENT
    refused(st, INV, "edge 1: camera index", lambda: e.set_relative_poses([ci[0], e.nc], cj, meas))
    refused(st, INV, "edge 1: camera index", lambda: e.set_relative_poses(ci, [cj[0], -1], meas))
    refused(st, INV, "edge 1: cam_i == cam_j", lambda: e.set_relative_poses(ci, [cj[0], ci[1]], meas))
    refused(st, INV, "edge 0: cam_i == cam_j", lambda: e.set_relative_poses(ci, [ci[0], ci[1]], meas))          # (the smallest is named)
    refused(st, INV, "edge 1: the measurement has an entry that is not finite", lambda: e.set_relative_poses(ci, cj, bad))
    refused(st, INV, "edge 1: zero quaternion", lambda: e.set_relative_poses(ci, cj, zq))
    refused(st, INV, "edge 1: the square-root information has an entry that is not finite", lambda: e.set_relative_poses(ci, cj, meas, sqrt_information=nf))
    refused(st, INV, "edge 1: the information matrix has an entry that is not finite", lambda: e.set_relative_poses(ci, cj, meas, information=nf))
    refused(st, STBA_ERR_NOT_POSITIVE_DEFINITE, "edge 1: the information matrix is not positive definite",
            lambda: e.set_relative_poses(ci, cj, meas, information=npd))
    with pytest.raises(ValueError):
        e.set_relative_poses(ci, cj, meas, information=npd, sqrt_information=npd)
    L_ = st.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    i32, j32 = np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(cj, np.int32)
    rc = L_.stba_ba_set_relative_poses(e._h, 2, p(i32), p(j32), p(meas), p(npd), p(npd))
    assert rc == INV and b"not both" in L_.stba_last_error()
    assert e.relative_pose_count() == 2 and same_bits(keep, e.evaluate_relative_poses())
    summ, _ = e.solve(st.default_options(max_num_iterations=2))
    assert summ.num_iterations == 2
    # quaternions are normalised on the host; a rank-deficient W and the identity are taken
    scaled = meas.copy(); scaled[:, :4] *= 3.0
    e.set_params(s["cams0"], s["pts0"])
    e.set_relative_poses(ci, cj, meas, sqrt_information=P.position_only_W(2))
    a = e.evaluate_relative_poses()
    e.set_relative_poses(ci, cj, scaled, sqrt_information=P.position_only_W(2))
    b = e.evaluate_relative_poses()
    assert np.allclose(a[1], b[1], rtol=0, atol=1e-14) and np.all(a[1][:, :3] == 0.0)
    e.set_relative_poses(ci, cj, meas)
    _, r, Ji, Jj = e.evaluate_relative_poses()
    rn, Jin, Jjn = T.BetweenBAProblem(s, ci, cj, meas, None).lin_edges(s["cams0"])
    assert np.allclose(r, rn, rtol=0, atol=1e-13) and np.allclose(Ji, Jin, rtol=0, atol=1e-12) and np.allclose(Jj, Jjn, rtol=0, atol=1e-12)


def test_refusals_in_both_orders(st):
    name = "a_chain"
    c = T.case(name)
    s = c["s"]
    INV = STBA_ERR_INVALID_ARGUMENT
    n_edges = len(c["cam_i"])

    def set_ed(e):
        e.set_relative_poses(c["cam_i"], c["cam_j"], c["meas"], information=c["information"])

    def usable(e, n):
        assert e.relative_pose_count() == n
        summ, _ = e.solve(st.default_options(max_num_iterations=1))
        assert summ.num_iterations == 1

    # ITERATIVE_SCHUR (the solver is fixed at creation: one order)
    e = engine(st, s, linear_solver="iterative_schur")
    refused(st, INV, "ITERATIVE_SCHUR", lambda: set_ed(e))
    usable(e, 0)
    # DOGLEG
    e = engine(st, s); e.set_trust_region("dogleg")
    refused(st, INV, "DOGLEG", lambda: set_ed(e))
    usable(e, 0)
    e = engine(st, s); set_ed(e)
    refused(st, INV, "relative-pose factors", lambda: e.set_trust_region("dogleg"))
    usable(e, n_edges)
    # inner iterations
    e = engine(st, s); e.set_inner_iterations(True)
    refused(st, INV, "inner iterations", lambda: set_ed(e))
    usable(e, 0)
    e = engine(st, s); set_ed(e)
    refused(st, INV, "relative-pose factors", lambda: e.set_inner_iterations(True))
    usable(e, n_edges)
    # a host lineariser
    prob = L.ba_problem(s)

    def lin(cams, pts, want):
        r, Jc, Jp = prob.lin_obs(cams, pts, want)
        return r, Jc, Jp
    e = engine(st, s); e.set_host_linearizer(lin)
    refused(st, INV, "host lineariser", lambda: set_ed(e))
    usable(e, 0)
    e = engine(st, s); set_ed(e)
    refused(st, INV, "relative-pose factors", lambda: e.set_host_linearizer(lin))
    usable(e, n_edges)
    # several ranks
    e = engine(st, s); e.set_allreduce(lambda user, buf, count, stream: 0, 0, 1)
    refused(st, INV, "all-reduce", lambda: set_ed(e))
    e = engine(st, s); set_ed(e)
    refused(st, INV, "relative-pose factors", lambda: e.set_allreduce(lambda user, buf, count, stream: 0, 0, 1))
    usable(e, n_edges)
    # clearing is always allowed
    e = engine(st, s, linear_solver="iterative_schur")
    e.set_relative_poses([], None, None)
    usable(e, 0)
