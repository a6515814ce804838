"""Bundle adjustment's per-observation information matrices on the GPU (BAEngine(information=, sqrt_information=),
stba_ba_set_information / _sqrt_information): the whitening forms of the correcting linearisation kernel and everything behind it --
both Schur forms, ITERATIVE_SCHUR, LM and DOGLEG, covariance -- against tests/ba_information_ref.py.

Bounds:
  factor      every entry of W = L^T within 4 eps relative of the 50-digit factor of the matrix given (include/stba.h);
              stba_ba_set_sqrt_information round-trips ==;
  evaluate    cost to 1e-12 relative.  Whitened r, Jc, Jp against lm_step_ref.BAProblem's whitened in numpy: the unwhitened entry's
              existing bound (tests/test_gpu_parity.py: 1e-14 for r, 1e-12 for Jc and Jp) through the two-term product,
              sum_k |W_jk| base_k + 4 eps |entry| (ba_information_ref.whitened_base); with a loss behind the weights
              ba_loss_ref.corrected_bound with that as its base; constant columns exactly 0;
  solve       lm_step_ref.compare / tolerances on the weighted reference (ITERATIVE_SCHUR: eps_eff = 1e-9 at eta = 1e-14; DOGLEG:
              dogleg_ref.compare on ba_loss_ref.dogleg_reference with the weighted problem);
  covariance  tests/test_gpu_covariance.py's: relative Frobenius error of a block <= 50 kappa eps, on (J^T Omega J)^-1.
Each case prints its figures before it asserts."""
import functools
import importlib

import numpy as np
import pytest

import ba_information_ref as I
import ba_loss_ref as B
import dogleg_ref as D
import lm_step_ref as L
import pg_loss_ref as G

pytestmark = pytest.mark.gpu

STBA_ERR_INVALID_ARGUMENT, STBA_ERR_NOT_POSITIVE_DEFINITE = -1, -4
K = 3
R_BASE, J_BASE = 1e-14, 1e-12
FAMILIES = ("mild", "wide")


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def engine(st, s, **kw):
    return st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s.get("pt_fixed"), **kw)


def x_of(e):
    cams, pts = e.get_params()
    return np.concatenate([cams.reshape(-1), pts.reshape(-1)])


def same_bits(x, y):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))


def masks(prob):
    return prob.cam_fixed[prob.oc], prob.pt_fixed[prob.op]


def loss_kw(table):
    return {} if table is None else dict(loss=dict(table))


def check_eval(label, got, prob, with_loss):
    """got = (cost, r, Jc, Jp) of the device against the numpy problem's r, Jc, Jp whitened by its W (and corrected by its table);
    returns the worst err / bound and the cost's relative error"""
    cost, r, Jc, Jp = got
    cams, pts = prob.split(prob.x0)
    ro, Jco, Jpo = prob.lin_obs(cams, pts)
    rw, Jcw, Jpw = I.whiten(prob.W, ro, Jco, Jpo)
    rc, Jcc, Jpc, terms = G.correct(rw, Jcw, Jpw, prob.table)
    cw = float(0.5 * np.sum(terms.astype(np.longdouble)))
    cm, pm = masks(prob)
    worst = 0.0
    for name, a, b, raw, base in (("r", r, rc, ro, R_BASE), ("Jc", Jc, Jcc, Jco, J_BASE), ("Jp", Jp, Jpc, Jpo, J_BASE)):
        wb = I.whitened_base(prob.W, raw, base)
        err, bound = np.abs(a - b), (B.corrected_bound(rw, prob.table, b, wb) if with_loss else wb)
        if name == "Jc":
            free = ~np.broadcast_to(cm[:, None, :], a.shape)
        elif name == "Jp":
            free = ~np.broadcast_to(pm[:, None, None], a.shape)
        else:
            free = np.ones(a.shape, bool)
        assert np.all(a[~free] == 0.0), f"{label} {name}: a constant column is not exactly zero"
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        ratio = float(np.max(ratio[free]))
        worst = max(worst, ratio)
        print(f"  {label} {name}: max err {err[free].max():.3e}, max err / bound {ratio:.3e}")
    print(f"  {label} cost {cost:.17g} reference {cw:.17g} relative {abs(cost - cw) / cw:.2e}")
    return worst, abs(cost - cw) / cw


# ------------------------------------------------------------------------------- 1. the factor and the order
def test_the_factor_is_the_exact_one_to_four_eps_in_the_callers_order(st):
    """set_information on a scene handed over in a shuffled observation order: the wide family's Omega = W^T W on the first half, matrices
    with kappa up to 1e12 (scales 1e-6 .. 1e6) on the second; what get_sqrt_information returns for observation i is the factor of
    the i-th matrix given"""
    s = B.scene("B")
    n = len(s["obs_cam"])
    p = np.random.default_rng(11).permutation(n)
    su = dict(s, obs_cam=s["obs_cam"][p], obs_pt=s["obs_pt"][p], obs_feat=s["obs_feat"][p])
    Om = I.information_of(I.weights("wide", n, seed=5))
    ill, kap = I.ill_conditioned(n - n // 2)
    Om[n // 2:] = ill
    e = engine(st, su, information=Om)
    assert e.has_information
    Wd = e.sqrt_information()
    worst = I.factor_error(Wd, Om)
    print(f"  factor: worst relative error {worst:.2f} eps over {n} matrices, kappa up to {kap.max():.1e}")
    assert kap.max() == 1e12 and worst <= I.FACTOR_BOUND / L.EPS
    assert np.all(Wd[:, 1, 0] == 0.0) and np.all(Wd[:, 0, 0] > 0) and np.all(Wd[:, 1, 1] > 0)
    # any finite W round-trips ==, not triangular, not symmetric
    W = I.weights("wide", n, seed=6)
    e.set_sqrt_information(W)
    assert np.array_equal(e.sqrt_information(), W)
    e.set_sqrt_information(None)
    assert not e.has_information and np.array_equal(e.sqrt_information(), np.broadcast_to(np.eye(2), (n, 2, 2)))


def test_the_weights_follow_the_callers_observation_order(st):
    """the engine sorts its observations by landmark: a scene handed over in a shuffled order, with its weights shuffled alike, gives
    every observation the bits it has in the sorted scene"""
    s = B.scene("A")
    n = len(s["obs_cam"])
    W = I.weights("wide", n, seed=2)
    p = np.random.default_rng(5).permutation(n)
    su = dict(s, obs_cam=s["obs_cam"][p], obs_pt=s["obs_pt"][p], obs_feat=s["obs_feat"][p])
    a = engine(st, s, sqrt_information=W).evaluate()
    b = engine(st, su, sqrt_information=W[p]).evaluate()
    assert np.array_equal(b[1], a[1][p]) and np.array_equal(b[2], a[2][p]) and np.array_equal(b[3], a[3][p])
    assert not np.array_equal(a[1], engine(st, s).evaluate()[1])


def test_python_shapes(st):
    s = B.scene("A")
    n = len(s["obs_cam"])
    e = engine(st, s, information=4.0)
    assert np.array_equal(e.sqrt_information(), np.broadcast_to(2.0 * np.eye(2), (n, 2, 2)))
    w = np.linspace(1.0, 9.0, n)
    e.set_information(w)
    Wd = e.sqrt_information()
    assert np.array_equal(Wd[:, 0, 0], np.sqrt(w)) and np.array_equal(Wd[:, 1, 1], np.sqrt(w)) and np.all(Wd[:, 0, 1] == 0) and np.all(Wd[:, 1, 0] == 0)
    e.set_information(np.array([[4.0, 0.0], [0.0, 9.0]]))
    assert np.array_equal(e.sqrt_information(), np.broadcast_to(np.diag([2.0, 3.0]), (n, 2, 2)))
    e.set_sqrt_information(np.array([[1.0, 2.0], [3.0, 4.0]]))
    assert np.array_equal(e.sqrt_information(), np.broadcast_to(np.array([[1.0, 2.0], [3.0, 4.0]]), (n, 2, 2)))
    for bad in (np.ones(n + 1), np.ones((n, 3, 2)), np.ones((3, 3))):
        with pytest.raises(ValueError):
            e.set_information(bad)
    with pytest.raises(ValueError):
        engine(st, s, information=1.0, sqrt_information=1.0)


# ------------------------------------------------------------------------------- 2. evaluate
@functools.lru_cache(maxsize=None)
def scene_d(n_total):
    return B.with_idle_cameras(B.scene("A"), n_total)


def eval_scene(st, sname):
    """(scene, engine keywords, the name whose thresholds and weights it uses)"""
    if sname != "D":
        return B.scene(sname), {}, sname
    _, _, max_in_lds = engine(st, B.scene("A"), linear_solver="iterative_schur").loss_kernel_geometry()
    return scene_d(max_in_lds + 1), dict(linear_solver="iterative_schur"), "A"


@pytest.mark.parametrize("name", (None,) + B.LOSS_SETS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("sname", ["A", "B", "C", "D"])
def test_evaluate_is_the_whitened_reference(st, sname, family, name):
    s, kw, tname = eval_scene(st, sname)
    n = len(s["obs_cam"])
    W = I.scene_weights(tname, family)
    table = None if name is None else B.loss_table(tname, name, n)
    prob = I.WeightedBAProblem(s, W, table)
    e = engine(st, s, sqrt_information=W, **loss_kw(table), **kw)
    assert e.has_information and e.has_loss == (name is not None)
    tile, in_lds, max_in_lds = e.loss_kernel_geometry()
    assert in_lds == (sname != "D") and (len(s["cams0"]) <= max_in_lds) == in_lds
    if sname == "C":
        assert -(-n // tile) > 2 and n % tile != 0, (n, tile)
    got = e.evaluate()
    worst, crel = check_eval(f"{sname} {family} {name}", got, prob, name is not None)
    assert worst <= 1.0 and crel <= 1e-12
    assert abs(e.cost() - got[0]) <= 1e-15 * got[0]                     # the residual-only kernel sums the same terms


def test_the_residual_only_kernel_without_cameras_in_lds(st):
    """scene D's trial-point launch (WITH_JAC = false, CAMS_IN_LDS = false), weights only and weights with losses: cost() and two LM
    iterations against the reference's cost at the parameters they end at"""
    s, kw, _ = eval_scene(st, "D")
    n = len(s["obs_cam"])
    W = I.scene_weights("A", "mild")
    for table in (None, B.loss_table("A", "mixed", n)):
        prob = I.WeightedBAProblem(s, W, table)
        e = engine(st, s, sqrt_information=W, **loss_kw(table), **kw)
        assert not e.loss_kernel_geometry()[1]
        want, got = prob.cost(prob.x0), e.cost()
        print(f"  D cost-only {got:.17g} reference {want:.17g}")
        assert abs(got - want) <= 1e-12 * want
        summ, tr = e.solve(max_num_iterations=2)
        assert summ.num_iterations == 2 and abs(e.cost() - summ.final_cost) <= 1e-12 * summ.final_cost
        assert abs(prob.cost(x_of(e)) - summ.final_cost) <= 1e-12 * summ.final_cost


@pytest.mark.parametrize("family", FAMILIES)
def test_information_and_its_square_root_give_the_same_normal_equations(st, family):
    """Omega = W^T W to set_information, W to set_sqrt_information: the factor W' = L^T is not W (Rot(phi) drops out of Omega), so r
    differs, while cost, the J^T J blocks and J^T r agree.  Bound per entry sum_i u_i^T Omega_i v_i (u, v columns of [J | r]; both
    engines whiten the same unwhitened bits): Omega as formed in FP64 is off by 3 eps |W|^T |W| (two products, one sum), W'^T W' from it
    by 8 eps |W'|^T |W'| (every entry of W' within 4 eps), and each whitening product carries 4 eps per factor: 16 eps
    sum_i |u_i|^T (|W_i|^T |W_i| + |W'_i|^T |W'_i|) |v_i| covers the three; the sums are taken in long double"""
    s = B.scene("B")
    n = len(s["obs_cam"])
    W = I.scene_weights("B", family)
    a = engine(st, s, sqrt_information=W)
    b = engine(st, s, information=I.information_of(W))
    Wb = b.sqrt_information()
    assert not np.array_equal(Wb, W) and np.all(Wb[:, 1, 0] == 0.0)
    prob = I.WeightedBAProblem(s, W)
    ga, gb = a.evaluate(), b.evaluate()
    assert not np.array_equal(ga[1], gb[1])
    LD = np.longdouble
    pa = I.normal_parts_of(prob, ga[1].astype(LD), ga[2].astype(LD), ga[3].astype(LD), ga[0])
    pb = I.normal_parts_of(prob, gb[1].astype(LD), gb[2].astype(LD), gb[3].astype(LD), gb[0])
    cams, pts = prob.split(prob.x0)
    ro, Jco, Jpo = prob.lin_obs(cams, pts)
    cm, pm = masks(prob)
    Jco = np.where(cm[:, None, :], 0.0, Jco); Jpo = np.where(pm[:, None, None], 0.0, Jpo)
    M = np.einsum("nki,nkj->nij", np.abs(W), np.abs(W)) + np.einsum("nki,nkj->nij", np.abs(Wb), np.abs(Wb))
    half = np.linalg.cholesky(M).transpose(0, 2, 1)                       # |u|^T M |v| as a product of "whitened" absolute values
    absr, absJc, absJp = (np.einsum("nij,nj...->ni...", half, np.abs(x)) for x in (ro, Jco, Jpo))
    bound = I.normal_parts_of(prob, absr.astype(LD), absJc.astype(LD), absJp.astype(LD), float(0.5 * np.sum(absr.astype(LD) ** 2)))
    worst = 0.0
    for name, x, y, bd in zip(("cost", "Hc", "Hp", "g"), pa, pb, bound):
        err, lim = np.abs(np.asarray(x, LD) - np.asarray(y, LD)), 16 * L.EPS * np.asarray(bd, LD)
        ratio = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), np.where(err == 0, 0.0, np.inf))))
        print(f"  {family} {name}: max difference {float(np.max(err)):.3e}, max difference / bound {ratio:.3e}")
        worst = max(worst, ratio)
    assert worst <= 1.0


# ------------------------------------------------------------------------------- 3. identity
def judge(prob, ref, o, x_dev, trace, label, eps_eff=L.EPS):
    """tests/test_gpu_lm_step.py's judge, as tests/test_gpu_ba_loss.py has it"""
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = L.compare(prob, ref, "ba", o, x_dev, trace, eps_eff=eps_eff)
    print(f"LMSTEP ba-information {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    if not any(it["accepted"] for it in ref):
        assert np.array_equal(x_dev, prob.x0), f"{label}: rejected steps moved the parameters"
    assert not fails, f"{label}: " + "; ".join(fails)


@pytest.mark.parametrize("sname", ["A", "B"])
def test_identity_rows_and_none_are_the_engine_without_weights(st, sname):
    """identity rows inside a mixed array store the bits of the engine that never had weights (the skip rule); set_information(None)
    gives that engine back bit for bit -- evaluate, a 3-iteration trace, the parameters (the lossless kernels)"""
    s = B.scene(sname)
    n = len(s["obs_cam"])
    fresh = engine(st, s)
    plain = fresh.evaluate()
    W = I.scene_weights(sname, "wide").copy()
    ident = np.arange(n) % 3 == 0
    W[ident] = np.eye(2)
    e = engine(st, s, sqrt_information=W)
    got = e.evaluate()
    assert all(np.array_equal(x[ident], y[ident]) for x, y in zip(got[1:], plain[1:]))
    assert not np.array_equal(got[1][~ident], plain[1][~ident])
    # ... and under a table with observations that have no loss: those rows are the lossless engine's
    table = B.loss_table(sname, "mixed", n)
    keep = G.untouched(table) & ident
    assert keep.any()
    got = engine(st, s, sqrt_information=W, loss=dict(table)).evaluate()
    assert all(np.array_equal(x[keep], y[keep]) for x, y in zip(got[1:], plain[1:]))
    for setter in (e.set_information, e.set_sqrt_information):
        e.set_sqrt_information(W)
        assert e.has_information
        setter(None)
        assert not e.has_information and same_bits(e.evaluate(), plain)
    sa, ta = e.solve(max_num_iterations=3)
    sb, tb = fresh.solve(max_num_iterations=3)
    assert sa.num_iterations == sb.num_iterations == 3
    assert np.array_equal(ta, tb) and np.array_equal(x_of(e), x_of(fresh))


@pytest.mark.parametrize("sname", ["A", "B"])
def test_an_all_identity_array_is_the_engine_without_weights(st, sname):
    """an array whose every W is exactly the identity -- through either setter, as a scalar, a (2, 2) or a per-observation array -- is
    not held: the engine is bit for bit the one that never had weights (evaluate with its cost, a 3-iteration trace, the parameters)"""
    s = B.scene(sname)
    n = len(s["obs_cam"])
    fresh = engine(st, s)
    plain = fresh.evaluate()
    eye = np.broadcast_to(np.eye(2), (n, 2, 2)).copy()
    sb, tb = fresh.solve(max_num_iterations=3)
    assert sb.num_iterations == 3
    for kw in (dict(information=1.0), dict(information=eye), dict(sqrt_information=eye), dict(sqrt_information=np.eye(2))):
        e = engine(st, s, **kw)
        assert not e.has_information and same_bits(e.evaluate(), plain)
        sa, ta = e.solve(max_num_iterations=3)
        assert sa.num_iterations == 3 and np.array_equal(ta, tb) and np.array_equal(x_of(e), x_of(fresh))
    # ... and it replaces weights that were held; one row that is not the identity keeps the array
    e = engine(st, s, sqrt_information=I.scene_weights(sname, "mild"))
    assert e.has_information and not same_bits(e.evaluate(), plain)
    e.set_information(eye)
    assert not e.has_information and same_bits(e.evaluate(), plain)
    eye[n // 2, 0, 0] = 1.0 + 2.0 ** -52
    e.set_sqrt_information(eye)
    assert e.has_information and np.array_equal(e.sqrt_information(), eye)
    # under a loss table the identity array leaves the loss-only engine
    table = B.loss_table(sname, "mixed", n)
    only_l = engine(st, s, loss=dict(table)).evaluate()
    f = engine(st, s, information=np.ones(n), loss=dict(table))
    assert not f.has_information and f.has_loss and same_bits(f.evaluate(), only_l)


@pytest.mark.parametrize("sname", ["A", "B"])
def test_weights_and_losses_combine_in_either_order_and_leave_one_by_one(st, sname):
    s = B.scene(sname)
    n = len(s["obs_cam"])
    W = I.scene_weights(sname, "mild")
    table = B.loss_table(sname, "mixed", n)
    both = engine(st, s, sqrt_information=W, loss=dict(table)).evaluate()
    only_w = engine(st, s, sqrt_information=W).evaluate()
    only_l = engine(st, s, loss=dict(table)).evaluate()
    plain = engine(st, s).evaluate()
    assert not same_bits(both, only_w) and not same_bits(both, only_l) and not same_bits(only_w, plain)
    e = engine(st, s)
    e.set_loss(**table); e.set_sqrt_information(W)
    assert same_bits(e.evaluate(), both)
    e.set_loss(None)
    assert e.has_information and not e.has_loss and same_bits(e.evaluate(), only_w)
    e.set_loss(**table)
    assert same_bits(e.evaluate(), both)
    e.set_sqrt_information(None)
    assert e.has_loss and not e.has_information and same_bits(e.evaluate(), only_l)
    e.set_loss(None)
    assert same_bits(e.evaluate(), plain)
    f = engine(st, s)
    f.set_sqrt_information(W); f.set_loss(**table)
    assert same_bits(f.evaluate(), both)
    f.set_sqrt_information(None); f.set_loss(None)
    assert same_bits(f.evaluate(), plain)
    summ, _ = f.solve(max_num_iterations=2)
    assert summ.num_iterations == 2


# ------------------------------------------------------------------------------- 4. the semantics
@pytest.mark.parametrize("name", [None, "huber"])
def test_four_times_the_identity_is_four_times_the_cost(st, name):
    """Omega = 4 I doubles every residual: with Huber's a doubled too, rho_2a(4 s) = 4 rho_a(s), the cost is 4 x the unweighted engine's
    (whose Huber has a); its first LM step follows the weighted reference"""
    s = B.scene("B")
    n = len(s["obs_cam"])
    a0 = B.HUBER_A["B"]
    t1 = None if name is None else B.table_of(1, a0, 1.0, 1.0, n)
    t2 = None if name is None else B.table_of(1, 2 * a0, 1.0, 1.0, n)
    c1 = engine(st, s, **loss_kw(t1)).evaluate()[0]
    e = engine(st, s, information=4.0, **loss_kw(t2))
    c2 = e.evaluate()[0]
    print(f"  4 I {name}: cost {c2:.17g} against 4 x {c1:.17g}, relative {abs(c2 - 4 * c1) / (4 * c1):.2e}")
    assert abs(c2 - 4 * c1) <= 1e-12 * 4 * c1
    o = L.lm_options(initial_trust_region_radius=1e-3)
    prob = I.WeightedBAProblem(s, np.broadcast_to(2.0 * np.eye(2), (n, 2, 2)), t2)
    ref = B.lm_reference(prob, o, 1)
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=1)))
    assert summ.num_iterations == 1
    judge(prob, ref, o, x_of(e), tr, f"4 I {name}")


# ------------------------------------------------------------------------------- 5. exact steps
def make_route(st, s, W, table, route):
    kw = dict(sqrt_information=W, **loss_kw(table))
    if route == "iterative":
        e = engine(st, s, linear_solver="iterative_schur", **kw)
        e.set_pcg("jacobi", eta=1e-14, max_iterations=max(6 * len(s["cams0"]), 10) * 4)
        return e, 1e-9
    e = engine(st, s, **kw)
    if route == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
        assert e.schur_mode() == e.SCHUR_DENSE
    return e, L.EPS


@pytest.mark.parametrize("route", ["pairs", "dense", "iterative"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", list(I.LM_CASES))
def test_exact_steps_follow_the_weighted_reference(st, case, k, route):
    sname, name, ok = I.SOLVE_CASES[case]
    s = B.scene(sname)
    o = L.lm_options(**ok)
    prob, ref = I.problem(sname, name), I.reference(case, k)
    e, eps_eff = make_route(st, s, prob.W, I.table_for(sname, name), route)
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=k)))
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    assert abs(tr[0][0] - ref[0]["start"]["cost"]) <= 1e-12 * ref[0]["start"]["cost"]
    judge(prob, ref, o, x_of(e), tr, f"{case} k={k} {route}", eps_eff=eps_eff)


@pytest.mark.parametrize("form", ["pairs", "dense"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", list(I.DOGLEG_CASES))
def test_dogleg_steps_follow_the_weighted_reference(st, case, k, form):
    sname, name, ok = I.SOLVE_CASES[case]
    s = B.scene(sname)
    o = L.lm_options(**ok)
    prob, ref = I.problem(sname, name), I.reference(case, k, "dogleg")
    e = engine(st, s, sqrt_information=prob.W, **loss_kw(I.table_for(sname, name)))
    e.set_trust_region("dogleg")
    if form == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=k)))
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6 and L.rho_margin_ok(ref, o)
    fails, ratios = D.compare(prob, ref, o, x_of(e), tr)
    print(f"DOGLEG ba-information {case} k={k} {form} kappa={kap:.2e} " + " ".join(f"{q}={v:.2e}" for q, v in sorted(ratios.items())))
    assert not fails, "; ".join(fails)
    assert [bool(v) for v in tr[1:, 6]] == [it["accepted"] for it in ref]
    assert list(e.dogleg_summary().steps_by_case) == [sum(1 for it in ref if it["case"] == c) for c in range(3)]


# ------------------------------------------------------------------------------- 6. covariance
def numpy_covariance(prob, x):
    """(J^T Omega J)^-1 over the free columns at x, embedded with zeros at the constant ones; its kappa"""
    _, J, cols = prob.lin(x)
    N = prob.n_local
    H = np.zeros((N, N))
    np.add.at(H, (cols[:, :, None], cols[:, None, :]), np.einsum("nki,nkj->nij", J, J))
    f = prob.free
    Hf = H[np.ix_(f, f)]
    ev = np.linalg.eigvalsh(Hf)
    Cf = np.linalg.inv(Hf)
    C = np.zeros((N, N))
    C[np.ix_(f, f)] = 0.5 * (Cf + Cf.T)
    return C, ev[-1] / ev[0]


def test_covariance_is_the_inverse_of_the_weighted_normal_matrix(st):
    s = B.scene("B")
    W = I.scene_weights("B", "mild")
    e = engine(st, s, sqrt_information=W)
    e.solve()
    cams, pts = e.get_params()
    nc = len(cams)
    prob = I.WeightedBAProblem(s, W)
    C, kappa = numpy_covariance(prob, x_of(e))
    pairs = [(c, c) for c in range(nc)] + [(1, 2), (2, 1), (3, 8), (0, 4)]
    cam, pb, rc = e.covariance(cam_pairs=pairs)
    tol = 50 * kappa * L.EPS
    worst = 0.0
    for (a, b), blk in zip(pairs, cam):
        ref = C[6 * a:6 * a + 6, 6 * b:6 * b + 6]
        if np.linalg.norm(ref) == 0.0:
            assert np.array_equal(blk, np.zeros((6, 6)))
            continue
        worst = max(worst, np.linalg.norm(blk - ref) / np.linalg.norm(ref))
    for j, blk in enumerate(pb):
        o = 6 * nc + 3 * j
        worst = max(worst, np.linalg.norm(blk - C[o:o + 3, o:o + 3]) / np.linalg.norm(C[o:o + 3, o:o + 3]))
    print(f"  covariance: kappa(J^T Omega J) {kappa:.3e} pivot ratio {rc:.3e} tolerance {tol:.3e} worst relative Frobenius error {worst:.3e}")
    assert worst <= tol
    # the unweighted covariance at the same point is another matrix by far
    f = engine(st, dict(s, cams0=cams, pts0=pts))
    cam0, _, _ = f.covariance(cam_pairs=pairs[:nc])
    far = max(np.linalg.norm(cam0[c] - C[6 * c:6 * c + 6, 6 * c:6 * c + 6]) / np.linalg.norm(C[6 * c:6 * c + 6, 6 * c:6 * c + 6])
              for c in range(nc) if np.linalg.norm(C[6 * c:6 * c + 6, 6 * c:6 * c + 6]) > 0)
    print(f"  unweighted covariance differs by {far:.3e} relative")
    assert far > 1e3 * tol
    # new weights release the held covariance
    e.set_sqrt_information(None)
    with pytest.raises(st.StbaError):
        n_ = np.zeros((1, 6, 6)); a_ = np.zeros(1, np.int32)
        st._chk(st.lib().stba_ba_camera_covariance(e._h, 1, st._p(a_), st._p(a_), st._p(n_)), "stba_ba_camera_covariance")


# ------------------------------------------------------------------------------- 7. refusals
def test_bad_weights_are_refused_with_the_observation_named_and_the_weights_kept(st):
    s = B.scene("B")
    n = len(s["obs_cam"])
    assert n > 600
    W = I.scene_weights("B", "mild")
    Om = I.information_of(W)
    e = engine(st, s, sqrt_information=W)
    before, Wb = e.evaluate(), e.sqrt_information()
    npd = STBA_ERR_NOT_POSITIVE_DEFINITE

    def refused(fn, arr, obs, code, at, val):
        bad = arr.copy()
        for a_, v_ in zip(at, val):
            bad[a_] = v_
        with pytest.raises(st.StbaError) as err:
            fn(bad)
        msg = st.lib().stba_last_error().decode()
        print("  refused:", msg)
        assert err.value.code == code and f"observation {obs}:" in msg, msg
        assert e.has_information and np.array_equal(e.sqrt_information(), Wb) and same_bits(e.evaluate(), before)

    indef, semi = np.array([[1.0, 2.0], [2.0, 1.0]]), np.array([[1.0, 1.0], [1.0, 1.0]])
    nan = np.array([[1.0, 0.0], [0.0, np.nan]])
    refused(e.set_information, Om, 5, npd, [5, 600], [indef, semi])            # both wrong: the smallest observation
    refused(e.set_information, Om, 600, npd, [600], [semi])
    refused(e.set_information, Om, 5, npd, [5, 600], [nan, -np.eye(2)])
    refused(e.set_information, Om, 600, npd, [600], [np.array([[np.inf, 0.0], [0.0, 1.0]])])
    refused(e.set_information, Om, 5, npd, [5], [np.array([[1.0, np.nan], [0.0, 1.0]])])      # the entry the factor does not read
    refused(e.set_sqrt_information, W, 5, STBA_ERR_INVALID_ARGUMENT, [5, 600], [nan, nan])
    refused(e.set_sqrt_information, W, 600, STBA_ERR_INVALID_ARGUMENT, [600], [np.array([[1.0, -np.inf], [0.0, 1.0]])])
    # an engine WITHOUT weights that refuses stays without
    f = engine(st, s)
    bad = Om.copy(); bad[5] = indef
    with pytest.raises(st.StbaError):
        f.set_information(bad)
    assert not f.has_information and same_bits(f.evaluate(), engine(st, s).evaluate())


def test_refusals_in_both_orders(st):
    s = B.scene("A")
    prob = L.ba_problem(s)
    W = I.scene_weights("A", "mild")

    def refused(fn, names):
        """the message names what stands in the way (not merely the function that refused)"""
        with pytest.raises(st.StbaError) as err:
            fn()
        msg = st.lib().stba_last_error().decode()
        print("  refused:", msg)
        assert err.value.code == STBA_ERR_INVALID_ARGUMENT and names in msg.split(":", 1)[1], msg

    def lin(cams, pts, want):
        return prob.lin_obs(cams.copy(), pts.copy(), want)

    def hook(_u, _buf, _count, _stream):
        return 0

    setters = {"host lineariser": lambda e: e.set_host_linearizer(lin), "inner iterations": lambda e: e.set_inner_iterations(True),
               "all-reduce hook": lambda e: e.set_allreduce(hook, 0, 1)}
    plain = engine(st, s).evaluate()
    weighted = engine(st, s, sqrt_information=W).evaluate()
    for what, setter in setters.items():
        e = engine(st, s, sqrt_information=W)                          # the weights first
        refused(lambda: setter(e), "information matrices")
        assert e.has_information and same_bits(e.evaluate(), weighted), what
        summ, _ = e.solve(max_num_iterations=2)
        assert summ.num_iterations == 2
        for put in (lambda f: f.set_sqrt_information(W), lambda f: f.set_information(4.0)):
            f = engine(st, s)                                          # the other setting first
            setter(f)
            refused(lambda: put(f), what)
            assert not f.has_information, what
            if what != "host lineariser":
                assert same_bits(f.evaluate(), plain), what
            f.set_information(None)                                    # removing what is not there is no error
            f.set_information(1.0)                                     # ... and neither is the identity, which is no weight
            assert not f.has_information


# ------------------------------------------------------------------------------- 8. routes of the loop
def decisions(summ):
    return (summ.num_iterations, summ.termination_type, summ.termination_reason, summ.num_successful_steps, summ.num_unsuccessful_steps)


def route_case(which):
    sname, name, ok = I.SOLVE_CASES[which]
    return B.scene(sname), I.scene_weights(sname), I.table_for(sname, name), ok


@pytest.mark.parametrize("which", ["A_none", "A_cauchy"])
def test_watched_equals_unwatched_and_a_fresh_engine_repeats_its_bits(st, which):
    s, W, table, ok = route_case(which)
    out = []
    for cb in (None, None, lambda *a: 0):
        e = engine(st, s, sqrt_information=W, **loss_kw(table))
        summ, tr = e.solve(st.default_options(**ok), callback=cb)
        assert summ.termination_type == 0, summ.as_dict()
        out.append((decisions(summ), tr, x_of(e)))
    print(f"LMROUTE ba-information {which}: {out[0][0]}")
    for other in out[1:]:
        assert other[0] == out[0][0]
        assert other[1].tobytes() == out[0][1].tobytes() and other[2].tobytes() == out[0][2].tobytes()


@pytest.mark.parametrize("which", ["A_none", "A_cauchy"])
def test_two_solves_on_one_engine(st, which):
    s, W, table, ok = route_case(which)
    e = engine(st, s, sqrt_information=W, **loss_kw(table))
    e.solve(st.default_options(**dict(ok, max_num_iterations=2)))
    cams, pts = e.get_params()
    sa, ta = e.solve(st.default_options(**ok))
    f = engine(st, dict(s, cams0=cams, pts0=pts), sqrt_information=W, **loss_kw(table))
    sb, tb = f.solve(st.default_options(**ok))
    assert decisions(sa) == decisions(sb), (sa.as_dict(), sb.as_dict())
    assert ta.tobytes() == tb.tobytes() and x_of(e).tobytes() == x_of(f).tobytes()
