"""The elimination of the landmarks on the device -- (Hpp_j + D_j)^-1, the reduced system in both forms, back-substitution, the
implicit Schur product, the covariance -- against the 50-digit reference of tests/schur_elim_ref.py on landmarks of a planted
spectrum (tests/schur_elim_cases.py), through the stage API only.  The reference is fed the DEVICE's r, Jc, Jp, so the
linearisation's error is not mixed in.  Every result is judged as err / u in the units of schur_elim_ref.py and held to C u, C
fixed by the LAPACK-Cholesky elimination on the CPU (test_schur_elim_reference_cpu.py); err / u_wide is printed next to it.

What the engine does with a landmark block V_j + D_j (spd3_inverse, small_linalg.hpp): it inverts every block whose Cholesky
pivots are above 16 eps of their diagonal entries -- every positive definite block up to lambda_1 / lambda_3 = 1e13 -- to
eps lambda_1 / lambda_3; a block below that (one observation and no damping: rank 2) gets a zero inverse: the landmark is
constant for the step, absent from S and rhs, dxp_j = 0.  In between (kappa above 1e13 up to the pivot test) a block may go either
way, and an inverse it gets has no correct digit left: such a landmark needs damping, which LM always gives it."""
import functools
import importlib

import numpy as np
import pytest

import lm_step_ref as L
import schur_elim_cases as SC
import schur_elim_ref as SR

pytestmark = pytest.mark.gpu
EPS, C = SR.EPS, SR.C
FORMS = ("pairs", "dense")


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def make_engine(st, c, form="pairs", **kw):
    args, kwargs = SC.engine_args(c)
    e = st.BAEngine(*args, **kwargs, **kw)
    if form != "iterative":
        e.set_schur_mode(e.SCHUR_DENSE if form == "dense" else e.SCHUR_PAIRS)
        assert e.schur_mode() == (e.SCHUR_DENSE if form == "dense" else e.SCHUR_PAIRS)
    return e


_CACHE = {}


def linearised(st, key):
    """(case, the device's r, Jc, Jp, Hpp, gp, the reference built from them), once per case"""
    if key not in _CACHE:
        c = SC.build(*(SC.CASES[key] if isinstance(key, str) else key))
        e = make_engine(st, c)
        _, r, Jc, Jp = e.evaluate()
        _, _, Hpp, gp = e.normal_blocks()
        planted = np.nonzero(c["cls"] != "control")[0]
        ref = SR.Reference(r, Jc, Jp, c["obs_cam"], c["obs_pt"], len(c["cams"]), len(c["pts"]), c["dc"], c["dp"], c["cam_fixed"],
                           c["pt_fixed"], keep_terms=set(planted.tolist()))
        _CACHE[key] = (c, (r, Jc, Jp), (Hpp, gp), ref)
    return _CACHE[key]


def report(label, q, ratios, classes, wide=None):
    """print err / u per class and the class of the worst entry; returns the worst ratio"""
    ratios, classes = np.asarray(ratios).reshape(-1), np.asarray(classes).reshape(-1)
    per = {str(k): float(ratios[classes == k].max()) for k in np.unique(classes)}
    w = int(np.argmax(ratios))
    extra = "" if wide is None else f"  (err/u_wide {float(np.max(wide)):.3g})"
    print(f"SCHURELIM {label} {q}: worst {ratios[w]:.3g} in class {classes[w]};  " + " ".join(f"{k}={v:.3g}" for k, v in sorted(per.items())) + extra)
    return float(ratios[w])


def s_classes(c, worst):
    return np.where(worst >= 0, c["cls"][worst], "none")


def judge_system(label, c, ref, S, rhs):
    nc = len(c["cams"])
    low = np.tril(np.ones((2 * nc, 2 * nc), bool))
    es, er = SR.block_err(np.tril(S), ref.S), SR.block_err(rhs, ref.rhs)
    ws = report(label, "S", SR.ratio(es, ref.u_S)[low], s_classes(c, ref.s_worst)[low], SR.ratio(es, ref.u_S_wide)[low])
    wr = report(label, "rhs", SR.ratio(er, ref.u_rhs), s_classes(c, ref.rhs_worst), SR.ratio(er, ref.u_rhs_wide))
    return ws, wr


def judge_dxp(label, c, ref, dxp, dxc):
    rp, u = ref.dxp(dxc)
    err = np.abs(dxp - rp).max(1)
    return report(label, "dxp", SR.ratio(err, u), c["cls"], SR.ratio(err, ref.u_dxp_wide)), rp


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", list(SC.CASES))
def test_landmark_blocks_are_the_reference_sums(st, name):
    """Hpp_j and gp_j within C times the accumulation unit EPS n_j max|term| (the unit is the size of ONE rounding of the largest
    term per term; a sum of n terms in any order is bounded by its depth times that, and C covers the depth as it does for S)"""
    c, _, (Hpp, gp), ref = linearised(st, name)
    assert np.array_equal(Hpp, np.swapaxes(Hpp, 1, 2))
    wh = report(name, "Hpp", SR.ratio(np.abs(Hpp - ref.Hpp).max((1, 2)), ref.u_Hpp), c["cls"])
    wg = report(name, "gp", SR.ratio(np.abs(gp - ref.gp).max(1), ref.u_gp), c["cls"])
    assert wh <= C and wg <= C


# ------------------------------------------------------------------------------------------ (b), (c)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(SC.CASES))
def test_reduced_system(st, name, form):
    """S (lower block triangle) and rhs of reduced_system(dc, dp), blockwise within C u, in the pair-plan form and in the dense
    form S = -(Y Y^T) -- the 260-observation landmark is a run of 26 repeated (camera, landmark) pairs per camera there.  A
    column of Y that vanished would take the landmark's term out of S: the bound on S sees it (and
    test_no_free_landmark_is_dropped looks for it by name)"""
    c, _, _, ref = linearised(st, name)
    e = make_engine(st, c, form)
    e.evaluate(); e.normal_blocks()
    S, rhs = e.reduced_system(c["dc"], c["dp"])
    ws, wr = judge_system(f"{name} {form}", c, ref, S, rhs)
    if SC.CASES[name][1] != 0:
        c0, _, _, ref0 = linearised(st, name.split("_")[0])
        e0 = make_engine(st, c0, form)
        e0.evaluate(); e0.normal_blocks()
        S0, _ = e0.reduced_system(c0["dc"], c0["dp"])
        sc = 2.0 ** -SC.CASES[name][1]
        D = np.tile(np.r_[np.ones(3), sc * np.ones(3)], len(c["cams"]))
        print(f"SCHURELIM {name} {form}: bits of S agree with the unscaled case: {np.array_equal(np.tril(S), np.tril(S0 * np.outer(D, D)))}")
    assert ws <= C and wr <= C


# ------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(SC.CASES))
def test_reduced_solve_and_back_substitution(st, name, form):
    """solve_reduced(): dxc against the reference's within lm_step_ref's whole-system bound C_PATH kappa EPS |dxc| -- kappa of
    the FULL damped system, which the ill-conditioned landmarks dominate (the bound is wide here; it is the one the LM tests use)
    -- and, the sharper statement about the solve itself, against the solution of the device's own S and rhs within C_PATH
    kappa(S) EPS, S scaled to a unit diagonal (dc is a hundredth of the camera blocks' diagonal: kappa(S) of a few hundred).
    back_substitute(): dxp_j per landmark within C u_j of the reference evaluated at the device's dxc"""
    c, _, _, ref = linearised(st, name)
    e = make_engine(st, c, form)
    e.evaluate(); e.normal_blocks()
    S, rhs = e.reduced_system(c["dc"], c["dp"])
    dxc = e.solve_reduced()
    dxp = e.back_substitute()
    kS = ref.kappa_S()
    Sf = np.tril(S) + np.tril(S, -1).T
    d = 1.0 / np.sqrt(np.diag(Sf))
    own = d * np.asarray(L.refined_solve((Sf * d[:, None] * d[None, :]).astype(L.LD), (rhs * d).astype(L.LD)), float)
    e_own = np.linalg.norm((dxc - own) / d) / np.linalg.norm(own / d)
    kap_full = max(ref.lam[~ref.out, 0].max() / ref.lam[~ref.out, 2].min(), kS)
    e_ref = np.linalg.norm(dxc - ref.dxc) / np.linalg.norm(ref.dxc)
    print(f"SCHURELIM {name} {form} dxc: vs own system {e_own / (kS * EPS):.3g} kappa(S) EPS (kappa(S) = {kS:.3g}); vs reference {e_ref:.3g} "
          f"= {e_ref / (kap_full * EPS):.3g} kappa EPS, kappa >= {kap_full:.3g}")
    assert e_own <= L.C_PATH["ba"] * kS * EPS
    assert e_ref <= L.C_PATH["ba"] * kap_full * EPS
    wp, rp = judge_dxp(f"{name} {form}", c, ref, dxp, dxc)
    assert np.all(dxp[ref.out] == 0)
    assert wp <= C


# ------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("name", ["general", "axis", "general_up40"])
def test_iterative_schur_products(st, name):
    """an iterative_schur engine: the implicit product S x for three seeded x, the Schur-Jacobi preconditioner and the reduced
    right-hand side, over the free camera dofs (the operator has zero rows and columns for the constant ones)"""
    c, (r, Jc, Jp), _, ref = linearised(st, name)
    e = make_engine(st, c, "iterative", linear_solver="iterative_schur")
    _, r2, Jc2, Jp2 = e.evaluate()
    assert np.array_equal(r2, r) and np.array_equal(Jc2, Jc) and np.array_equal(Jp2, Jp)
    e.normal_blocks()
    free = (np.asarray(c["cam_fixed"]).reshape(-1) == 0)
    fh = free.reshape(-1, 3).all(1)
    cls_h = s_classes(c, ref.rhs_worst)
    rhs = e.schur_apply(c["dc"], c["dp"], which=0, x=None)
    er = SR.block_err(rhs * free, ref.rhs * free)
    worst = report(f"{name} iterative", "rhs", SR.ratio(er, ref.u_rhs)[fh], cls_h[fh], SR.ratio(er, ref.u_rhs_wide)[fh])
    sc = 2.0 ** SC.CASES[name][1]
    for seed in range(3):
        x = np.random.default_rng(seed).normal(size=(len(c["cams"]), 6)) * np.r_[np.ones(3), sc * np.ones(3)]
        x = x.reshape(-1) * free
        y = e.schur_apply(c["dc"], c["dp"], which=0, x=x)
        yr, u = ref.apply(x)
        worst = max(worst, report(f"{name} iterative", f"S x (seed {seed})", SR.ratio(SR.block_err(y * free, yr * free), u)[fh], cls_h[fh]))
        z = e.schur_apply(c["dc"], c["dp"], which=2, x=x)
        zr, uz = ref.block_jacobi(x)
        worst = max(worst, report(f"{name} iterative", f"Schur-Jacobi (seed {seed})", SR.ratio(np.abs(z - zr), uz)[free], np.repeat(cls_h, 3)[free]))
    assert worst <= C


# ------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("orientation", ["general", "axis"])
def test_no_free_landmark_is_dropped(st, orientation, form):
    """no free landmark with lambda_1 / lambda_3 <= 1e12 comes back with dxp_j = 0 or without its term in S; the singular one
    (one observation, dp = 0) is zeroed -- the reference leaves it out, and S, rhs and every other dxp_j keep their bounds.  The
    scene holds the "extreme" anisotropic landmarks too (lambda_1 / lambda_3 up to 1e12, lambda_1^2 / (lambda_2 lambda_3) up to
    1e22): a determinant summed from cofactors comes out negative for three of the four in general orientation"""
    key = (orientation, 0, True)
    c, _, _, ref = linearised(st, key)
    e = make_engine(st, c, form)
    e.evaluate(); e.normal_blocks()
    S, rhs = e.reduced_system(c["dc"], c["dp"])
    dxc = e.solve_reduced()
    dxp = e.back_substitute()
    sing = np.nonzero(c["cls"] == "singular")[0]
    assert len(sing) == 1 and ref.out[sing[0]] and np.all(dxp[sing[0]] == 0)
    assert set(c["cls"][ref.out]) == {"fixed", "singular"}
    ws, wr = judge_system(f"{orientation} singular {form}", c, ref, S, rhs)
    wp, rp = judge_dxp(f"{orientation} singular {form}", c, ref, dxp, dxc)
    kap = ref.lam[:, 0] / ref.lam[:, 2]
    live = ~ref.out & (kap <= 1.2e12) & (np.abs(rp).max(1) > 0)
    assert set(c["cls"][live]) >= {"control", "depth", "anisotropic", "single", "big"}
    dropped = [(int(j), str(c["cls"][j]), f"{kap[j]:.1e}") for j in np.nonzero(live)[0] if np.all(dxp[j] == 0)]
    assert not dropped, f"landmarks with dxp = 0: {dropped}"
    # its term in S: at the block where the term is largest the device is nearer to the reference WITH the term than without it,
    # wherever the bound C u of that block is small enough to tell (it is for every planted landmark up to kappa 1e10)
    told, missing = 0, []
    for j, blocks in ref.terms.items():
        (a, b), T = max(blocks.items(), key=lambda kv: np.abs(kv[1]).max())
        D = np.tril(S)[6 * a:6 * a + 6, 6 * b:6 * b + 6] - ref.S[6 * a:6 * a + 6, 6 * b:6 * b + 6]
        if a == b:
            T, D = np.tril(T), np.tril(D)
        if C * ref.u_S[2 * a:2 * a + 2, 2 * b:2 * b + 2].max() < 0.25 * np.abs(T).max():
            told += 1
            if not np.abs(D).max() < 0.5 * np.abs(T).max():
                missing.append((int(j), str(c["cls"][j]), f"{kap[j]:.1e}"))
    print(f"SCHURELIM {orientation} singular {form}: the term of {told} of {len(ref.terms)} planted landmarks is visible in S above C u")
    assert told >= 12 and not missing, f"terms missing from S: {missing}"
    # the neighbours of the zeroed landmark keep their bounds
    assert ws <= C and wr <= C and wp <= C


# ------------------------------------------------------------------------------------------ (g)
@pytest.mark.parametrize("orientation", ["general", "axis"])
def test_point_covariance(st, orientation):
    """covariance(points=...) on the undamped scene (pivot ratios of the V_j from 1e-4 to 1e-10): the landmark blocks of
    (J^T Omega J)^-1 at 50 digits, within C u with the unit of schur_elim_ref.Reference.point_covariance"""
    key = (orientation, 0, False, True)
    c, _, _, ref = linearised(st, key)
    e = make_engine(st, c)
    js = np.concatenate([np.nonzero((c["cls"] != "control") & ~ref.out)[0], np.arange(0, 60, 7)])
    js = js[~ref.out[js]]
    _, blocks, rcond = e.covariance(points=js)
    want, u = ref.point_covariance(js)
    w = report(f"{orientation} covariance", "point blocks", SR.ratio(np.abs(blocks - want).max((1, 2)), u), c["cls"][js])
    print(f"SCHURELIM {orientation} covariance: rcond {rcond:.3g}, kappa(S) {ref.kappa_S():.3g}")
    assert w <= C


# ------------------------------------------------------------------------------------------ (h)
def lm_judge(prob, ref, o, x_dev, trace, label):
    """tests/test_gpu_lm_step.py's judge, as tests/test_gpu_ba_information.py has it"""
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = L.compare(prob, ref, "ba", o, x_dev, trace)
    print(f"SCHURELIM LM {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    assert not fails, f"{label}: " + "; ".join(fails)


@functools.lru_cache(maxsize=None)
def lm_reference(k):
    import ba_information_ref as I
    import ba_loss_ref as B
    s, W = SC.lm_scene()
    prob = I.WeightedBAProblem(s, W)
    return prob, B.lm_reference(prob, L.lm_options(), k)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 3])
def test_full_lm_with_anisotropic_low_parallax_landmarks(st, k, form):
    """solve() for k iterations on the LM scene of schur_elim_cases.lm_scene -- information matrices diag(1, s), s down to 1e-8,
    on landmarks seen through nearly parallel rays -- against the weighted LM reference with the rules of the LM step tests.
    Ceres' default radius 1e4: the reference's kappa is 3.4e7, inside judge's precondition (64 kappa EPS <= 1e-6)"""
    s, W = SC.lm_scene()
    o = L.lm_options()
    prob, ref = lm_reference(k)
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"], sqrt_information=W)
    e.set_schur_mode(e.SCHUR_DENSE if form == "dense" else e.SCHUR_PAIRS)
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=k)))
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    assert abs(tr[0][0] - ref[0]["start"]["cost"]) <= 1e-12 * ref[0]["start"]["cost"]
    cams, pts = e.get_params()
    lm_judge(prob, ref, o, np.concatenate([cams.reshape(-1), pts.reshape(-1)]), tr, f"k={k} {form}")


# ------------------------------------------------------------------------------------------ (i)
def gn_fixed_point(cams, feats, L0):
    """the point where the gradient sum_i Jp_i^T r_i of the reprojection cost vanishes, by Gauss-Newton at 50 digits from L0"""
    import mpmath as mp
    import mp_ref as M
    Lm = [mp.mpf(float(x)) for x in L0]
    for _ in range(60):
        H, g = mp.zeros(3, 3), mp.zeros(3, 1)
        for cam, f in zip(cams, feats):
            r = M.ba_residual(cam, Lm, f)
            _, Jp = M.ba_jacobians_analytic(cam, Lm)
            H += Jp.T * Jp
            g += Jp.T * mp.matrix(r)
        d = mp.lu_solve(H, -g)
        Lm = [Lm[i] + d[i] for i in range(3)]
        if mp.norm(d) < mp.mpf("1e-35") * mp.norm(mp.matrix(Lm)):
            break
    else:
        raise AssertionError("the 50-digit Gauss-Newton did not converge")
    lam = sorted((float(x) for x in mp.eigsy(H, eigvals_only=True)), reverse=True)
    return np.array([float(x) for x in Lm]), lam


@pytest.mark.parametrize("orientation", ["general", "axis"])
def test_triangulation_of_low_parallax_landmarks(st, orientation):
    """triangulate() from a start 2 % off in depth, on the depth-class landmarks (two or three cameras, parallax 2e-2 ... 2e-5,
    noise-free features: the stopping rule of the kernel is relative to the cost, and a cost of rounding size lets it run to the
    end): the converged point against the 50-digit Gauss-Newton fixed point of the same float features, within
    C EPS lambda_1 / lambda_3 |L| (lambda of the undamped 3 x 3 system at the fixed point)"""
    c = SC.build(orientation, 0)
    js = [j for j in np.nonzero(c["cls"] == "depth")[0] if c["claim"][j][2] >= 1e-10]
    cams, pts, feat = np.array(c["cams"]), np.array(c["pts"]), np.array(c["obs_feat"])
    prob = L.BAProblem(cams, pts, c["obs_cam"], c["obs_pt"], feat)
    feat = feat + prob.lin_obs(cams, pts, False)[0]                       # the exact projections of the planted points, rounded
    start = pts.copy()
    for j in js:
        a = c["obs_cam"][np.nonzero(c["obs_pt"] == j)[0][0]]
        start[j] = cams[a, 4:] + 1.02 * (pts[j] - cams[a, 4:])
    fix = np.ones(len(pts), np.uint8); fix[js] = 0                          # only the landmarks under test move
    e = st.BAEngine(cams, start, c["obs_cam"], c["obs_pt"], feat, c["cam_fixed"], pt_fixed=fix)
    e.triangulate(max_iter=200)
    _, got = e.get_params()
    assert np.array_equal(got[fix != 0], start[fix != 0])
    worst = 0.0
    for j in js:
        idx = np.nonzero(c["obs_pt"] == j)[0]
        want, lam = gn_fixed_point(cams[c["obs_cam"][idx]], feat[idx], got[j])
        u = EPS * lam[0] / lam[2] * np.linalg.norm(want)
        err = np.linalg.norm(got[j] - want)
        print(f"SCHURELIM triangulate {orientation} landmark {j}: kappa {lam[0] / lam[2]:.2e}, err {err:.3e} = {err / u:.3g} u, moved {np.linalg.norm(got[j] - start[j]):.3e}")
        worst = max(worst, err / u)
    assert worst <= C
