"""Bundle adjustment's robust losses on the GPU (BAEngine(loss=), stba_ba_set_loss): the correcting linearisation kernel and everything
behind it -- both Schur forms, ITERATIVE_SCHUR, LM and DOGLEG, covariance -- against tests/ba_loss_ref.py.

Bounds:
  evaluate    cost to 1e-12 relative.  r', Jc', Jp' against lm_step_ref.BAProblem's r, Jc, Jp corrected in numpy: the uncorrected entry's
              existing bound (tests/test_gpu_parity.py: 1e-14 for r, 1e-12 for Jc and Jp) times the magnitude of the correction factor
              (|rs| for r; |M| = |sqrt(rho') (I - (alpha / s) r r^T)| as a matrix for J) plus c eps |entry|, c = 8 x (the worst error
              of the numpy rho', rho'' against 50 digits on these inputs, in eps) + 16 per kind (ba_loss_ref.RHO_EPS, c_of; measured
              by tests/test_ba_loss_cpu.py); constant columns exactly 0;
  solve       lm_step_ref.compare / tolerances on the robust reference (ITERATIVE_SCHUR: eps_eff = 1e-9 at eta = 1e-14, as
              tests/test_gpu_iterative_schur.py runs its exact limit; DOGLEG: dogleg_ref.compare on ba_loss_ref.dogleg_reference);
  covariance  tests/test_gpu_covariance.py's: relative Frobenius error of a block <= 50 kappa eps, on (J'^T J')^-1.
Each case prints its figures before it asserts."""
import functools
import importlib

import numpy as np
import pytest

import ba_loss_ref as B
import dogleg_ref as D
import lm_step_ref as L
import pg_loss_ref as G

pytestmark = pytest.mark.gpu

STBA_ERR_INVALID_ARGUMENT = -1
K = 3
R_BASE, J_BASE = 1e-14, 1e-12


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
    """per observation: which of the 6 camera columns and whether the landmark is constant"""
    return prob.cam_fixed[prob.oc], prob.pt_fixed[prob.op]


def check_eval(label, got, prob):
    """got = (cost, r, Jc, Jp) of the device against the numpy problem's r, Jc, Jp corrected by its table; returns the worst
    err / bound and the cost's relative error"""
    cost, r, Jc, Jp = got
    cams, pts = prob.split(prob.x0)
    ro, Jco, Jpo = prob.lin_obs(cams, pts)
    rc, Jcc, Jpc, terms = G.correct(ro, Jco, Jpo, prob.table)
    cw = float(0.5 * np.sum(terms.astype(np.longdouble)))
    cm, pm = masks(prob)
    worst = 0.0
    for name, a, b, base in (("r", r, rc, R_BASE), ("Jc", Jc, Jcc, J_BASE), ("Jp", Jp, Jpc, J_BASE)):
        err, bound = np.abs(a - b), B.corrected_bound(ro, prob.table, b, base)
        if name == "Jc":
            free = ~np.broadcast_to(cm[:, None, :], a.shape)
        elif name == "Jp":
            free = ~np.broadcast_to(pm[:, None, None], a.shape)
        else:
            free = np.ones(a.shape, bool)
        assert np.all(a[~free] == 0.0), f"{label} {name}: a constant column is not exactly zero"
        # (a Tukey observation beyond a^2 has r' = 0 and J' = 0 exactly, and a bound of zero: there the device must give zero too)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        ratio = float(np.max(ratio[free]))
        worst = max(worst, ratio)
        print(f"  {label} {name}: max err {err[free].max():.3e}, max err / bound {ratio:.3e}")
    print(f"  {label} cost {cost:.17g} reference {cw:.17g} relative {abs(cost - cw) / cw:.2e}")
    return worst, abs(cost - cw) / cw


# ------------------------------------------------------------------------------- 1. evaluate
@functools.lru_cache(maxsize=None)
def scene_d(n_total):
    return B.with_idle_cameras(B.scene("A"), n_total)


def eval_scene(st, sname):
    """(scene, engine keywords, the name whose thresholds it uses)"""
    if sname != "D":
        return B.scene(sname), {}, sname
    _, _, max_in_lds = engine(st, B.scene("A"), linear_solver="iterative_schur").loss_kernel_geometry()
    return scene_d(max_in_lds + 1), dict(linear_solver="iterative_schur"), "A"


@pytest.mark.parametrize("name", B.LOSS_SETS)
@pytest.mark.parametrize("sname", ["A", "B", "C", "D"])
def test_evaluate_is_the_corrected_reference(st, sname, name):
    s, kw, tname = eval_scene(st, sname)
    n = len(s["obs_cam"])
    table = B.loss_table(tname, name, n)
    prob = B.RobustBAProblem(s, table)
    e = engine(st, s, loss=dict(table), **kw)
    assert e.has_loss
    tile, in_lds, max_in_lds = e.loss_kernel_geometry()
    assert in_lds == (sname != "D") and (len(s["cams0"]) <= max_in_lds) == in_lds
    if sname == "C":
        assert -(-n // tile) > 2 and n % tile != 0, (n, tile)
    got = e.evaluate()
    worst, crel = check_eval(f"{sname} {name}", got, prob)
    assert worst <= 1.0 and crel <= 1e-12
    assert abs(e.cost() - got[0]) <= 1e-15 * got[0]                     # the residual-only kernel sums the same rho
    # observations without a loss (kind 0, scale 1) compare == with the engine that has no table
    keep = G.untouched(table)
    if name == "mixed":
        _, r0, Jc0, Jp0 = engine(st, s, **kw).evaluate()
        _, r, Jc, Jp = got
        assert keep.any() and np.array_equal(r[keep], r0[keep]) and np.array_equal(Jc[keep], Jc0[keep]) and np.array_equal(Jp[keep], Jp0[keep])
        assert not np.array_equal(r[~keep], r0[~keep])


def test_the_residual_only_kernel_without_cameras_in_lds(st):
    """scene D's trial-point launch (WITH_JAC = false, CAMS_IN_LDS = false: the variant is the engine's, decided from the full
    linearisation): cost() and the trial costs of two LM iterations against the reference's"""
    s, kw, _ = eval_scene(st, "D")
    table = B.loss_table("A", "mixed", len(s["obs_cam"]))
    prob = B.RobustBAProblem(s, table)
    e = engine(st, s, loss=dict(table), **kw)
    assert not e.loss_kernel_geometry()[1]
    want = prob.cost(prob.x0)
    got = e.cost()
    print(f"  D cost-only {got:.17g} reference {want:.17g}")
    assert abs(got - want) <= 1e-12 * want
    summ, tr = e.solve(max_num_iterations=2)
    cams, pts = e.get_params()
    assert summ.num_iterations == 2 and abs(e.cost() - summ.final_cost) <= 1e-12 * summ.final_cost
    assert abs(prob.cost(np.concatenate([cams.reshape(-1), pts.reshape(-1)])) - summ.final_cost) <= 1e-12 * summ.final_cost


@pytest.mark.parametrize("sname", ["A", "B"])
def test_a_sharp_tolerant_transition(st, sname):
    """Tolerant with b = a / 60 (the loss sets use a / 4, ba_loss_ref's docstring): r' = rs(s) r and J' = M(s) J depend on s through
    rho' = e^x / (1 + e^x) with a relative sensitivity of up to a / b.  The evaluate bound's first term carries the uncorrected entry's
    bound through the correction factor only; here the term of the factor's DERIVATIVE is added, from the same uncorrected bound:
    |r_device - r_numpy| <= 1e-14 per component moves s by ds <= 2 |r|_1 1e-14, and the corrected entry by |d entry / d s| ds, the
    derivative taken from the reference by a central difference in s"""
    s = B.scene(sname)
    n = len(s["obs_cam"])
    a = B.TOLERANT_A[sname]
    table = B.table_of(5, a, a / 60.0, 1.0, n)
    prob = B.RobustBAProblem(s, table)
    cams, pts = prob.split(prob.x0)
    ro, Jco, Jpo = prob.lin_obs(cams, pts)
    Jo = np.concatenate([Jco, Jpo], 2)
    rc, Jcc, Jpc, terms = G.correct(ro, Jco, Jpo, table)
    Jx = np.concatenate([Jcc, Jpc], 2)

    def at(scale):                                                       # the corrected pair with s scaled (r scaled by sqrt), J as it is
        rr = ro * np.sqrt(scale)
        a_, b_, c_, _ = G.correct(rr, Jco, Jpo, table)
        return a_ / np.sqrt(scale), np.concatenate([b_, c_], 2)
    h = 1e-7
    (rp, Jp_), (rm, Jm_) = at(1 + h), at(1 - h)
    ss = np.sum(ro * ro, 1)
    ds = 2.0 * np.abs(ro).sum(1) * R_BASE
    dr = np.abs(rp - rm) / (2 * h * ss[:, None]) * ds[:, None]
    dJ = np.abs(Jp_ - Jm_) / (2 * h * ss[:, None, None]) * ds[:, None, None]
    cost, r, Jc, Jp = engine(st, s, loss=dict(table)).evaluate()
    J = np.concatenate([Jc, Jp], 2)
    cm, pm = masks(prob)
    free = ~np.concatenate([np.broadcast_to(cm[:, None, :], Jc.shape), np.broadcast_to(pm[:, None, None], Jp.shape)], 2)
    br = B.corrected_bound(ro, table, rc, R_BASE) + dr
    bJ = B.corrected_bound(ro, table, Jx, J_BASE) + dJ
    x = (ss - a) / (a / 60.0)
    wr = float(np.max(np.abs(r - rc) / br))
    wJ = float(np.max((np.abs(J - Jx) / bJ)[free]))
    print(f"  {sname} sharp tolerant: x from {x.min():.1f} to {x.max():.1f}, {np.mean(x > G.TOLERANT_LINEAR):.2f} linear; "
          f"r' err / bound {wr:.3e} (derivative term up to {np.max(dr / br):.2f} of it), J' err / bound {wJ:.3e}")
    assert np.any((x > -5) & (x < 5)) and np.any(x > G.TOLERANT_LINEAR) and np.all(J[~free] == 0.0)
    assert wr <= 1.0 and wJ <= 1.0
    cw = float(0.5 * np.sum(terms.astype(np.longdouble)))
    assert abs(cost - cw) <= 1e-12 * cw


def test_zero_residuals_take_the_first_corrector_branch(st):
    """s == 0 exactly (ba_loss_ref.zero_scene), every kind: r' = 0 and J' = sqrt(rho'(0)) J to c eps"""
    s, table = B.zero_scene()
    n = len(s["obs_cam"])
    cost0, r0, Jc0, Jp0 = engine(st, s).evaluate()
    assert cost0 == 0.0 and np.all(r0 == 0.0)
    cost, r, Jc, Jp = engine(st, s, loss=dict(table)).evaluate()
    rh, sq, _, _ = G.factors(table, np.zeros(n))
    sq = np.where(G.untouched(table), 1.0, sq)
    print(f"  zero scene: cost {cost!r}; sqrt(rho'(0)) from {sq.min():.3g} to {sq.max():.3g}")
    assert np.all(r == 0.0) and abs(cost) <= 1e-15 and set(table["kind"].tolist()) == set(range(7)) and np.any(rh[2] > 0)
    for J, J0 in ((Jc, Jc0), (Jp, Jp0)):
        want = sq[:, None, None] * J0
        assert np.all(np.abs(J - want) <= B.c_of(table["kind"])[:, None, None] * L.EPS * np.abs(want))
    assert np.any(Jp != Jp0) and np.any(Jc != 0.0) and np.all(Jc[s["obs_cam"] == 0] == 0.0)


# ------------------------------------------------------------------------------- 2. setters
@pytest.mark.parametrize("sname", ["A", "B"])
def test_none_restores_the_engine_without_a_loss_bit_for_bit(st, sname):
    s = B.scene(sname)
    n = len(s["obs_cam"])
    fresh = engine(st, s)
    e = engine(st, s, loss=dict(B.loss_table(sname, "huber", n)))
    assert e.has_loss and not fresh.has_loss
    assert not same_bits(e.evaluate(), fresh.evaluate())
    e.set_loss(None)
    assert not e.has_loss and same_bits(e.evaluate(), fresh.evaluate())
    e.set_loss("cauchy", 0.05); e.set_loss(None)
    assert not e.has_loss and same_bits(e.evaluate(), fresh.evaluate())
    sa, ta = e.solve(max_num_iterations=3)
    sb, tb = fresh.solve(max_num_iterations=3)
    assert sa.num_iterations == sb.num_iterations == 3
    assert np.array_equal(ta, tb) and np.array_equal(x_of(e), x_of(fresh))


def judge(prob, ref, o, x_dev, trace, label, eps_eff=L.EPS):
    """tests/test_gpu_lm_step.py's judge, word for word in what it checks (the ITERATIVE_SCHUR route as
    tests/test_gpu_iterative_schur.py::test_exact_limit_matches_direct_and_reference runs it: the case is an accuracy case at eps,
    the comparison's eps_eff is 1e-9)"""
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = L.compare(prob, ref, "ba", o, x_dev, trace, eps_eff=eps_eff)
    print(f"LMSTEP ba-loss {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    if not any(it["accepted"] for it in ref):
        assert np.array_equal(x_dev, prob.x0), f"{label}: rejected steps moved the parameters"
    assert not fails, f"{label}: " + "; ".join(fails)


@pytest.mark.parametrize("case", ["lm33_extras_r1e-3", "lm300_r1e-3"])
def test_an_all_trivial_table_follows_the_lossless_reference(st, case):
    """(not bitwise the lossless engine: the table switches every kernel behind the linearisation to its general form)"""
    sk, ok = L.BA_CASES[case]
    s = L.ba_scene(**sk)
    o = L.lm_options(**ok)
    prob = L.ba_problem(s)
    ref = L.lm_reference(prob, o, K)
    e = engine(st, s, loss="trivial")
    assert e.has_loss
    got, plain = e.evaluate(), engine(st, s).evaluate()
    assert same_bits(got[1:], plain[1:]) and abs(got[0] - plain[0]) <= 4 * L.EPS * plain[0]      # (the cost: other partial sums)
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=K)))
    assert summ.num_iterations == K and len(tr) == K + 1
    judge(prob, ref, o, x_of(e), tr, f"all-trivial {case}")


def test_bad_tables_are_refused_with_the_observation_named_and_the_table_kept(st):
    s = B.scene("B")
    n = len(s["obs_cam"])
    table = B.loss_table("B", "mixed", n)
    e = engine(st, s, loss=dict(table))
    before = e.evaluate()

    def refused(obs, **change):
        bad = {k: v.copy() for k, v in table.items()}
        for key, (at, val) in change.items():
            for a_, v_ in zip(np.atleast_1d(at), np.atleast_1d(val)):
                bad[key][a_] = v_
        with pytest.raises(st.StbaError) as err:
            e.set_loss(**bad)
        msg = st.lib().stba_last_error().decode()
        print("  refused:", msg)
        assert err.value.code == STBA_ERR_INVALID_ARGUMENT and f"observation {obs}:" in msg, msg
        assert e.has_loss and same_bits(e.evaluate(), before)

    refused(5, kind=([5, 600], [7, -1]))                                   # unknown kinds: the smallest observation
    refused(600, kind=(600, 9))
    refused(5, kind=([5, 600], [1, 1]), a=([5, 600], [0.0, np.nan]))       # a not positive / not finite
    refused(600, kind=(600, 3), a=(600, np.inf))
    refused(5, kind=([5, 600], [5, 5]), b=([5, 600], [-1.0, 0.0]))         # b of a Tolerant observation
    refused(600, kind=(600, 5), b=(600, np.nan))
    refused(5, scale=([5, 600], [-0.5, np.nan]))
    refused(600, scale=(600, np.inf))
    # parameters the kind does not use are not read: a NaN b on a Huber observation, a NaN a on one without a loss
    ok = {k: v.copy() for k, v in table.items()}
    ok["kind"][[5, 600]] = [1, 0]; ok["b"][5] = np.nan; ok["a"][600] = np.nan
    e.set_loss(**ok)
    assert e.has_loss and np.isfinite(e.evaluate()[0])
    # an engine WITHOUT a table that refuses stays without
    f = engine(st, s)
    with pytest.raises(st.StbaError):
        f.set_loss(np.full(n, 9), 1.0)
    assert not f.has_loss and same_bits(f.evaluate(), engine(st, s).evaluate())


def test_the_table_follows_the_callers_observation_order(st):
    """the engine sorts its observations by landmark: a scene handed over in a shuffled order, with its table shuffled alike, gives
    every observation the bits it has in the sorted scene"""
    s = B.scene("A")
    n = len(s["obs_cam"])
    table = B.loss_table("A", "mixed", n)
    p = np.random.default_rng(5).permutation(n)
    su = dict(s, obs_cam=s["obs_cam"][p], obs_pt=s["obs_pt"][p], obs_feat=s["obs_feat"][p])
    a = engine(st, s, loss=dict(table)).evaluate()
    b = engine(st, su, loss={k: v[p] for k, v in table.items()}).evaluate()
    assert np.array_equal(b[1], a[1][p]) and np.array_equal(b[2], a[2][p]) and np.array_equal(b[3], a[3][p])


def test_refusals_in_both_orders(st):
    s = B.scene("A")
    n = len(s["obs_cam"])
    prob = L.ba_problem(s)

    def refused(fn):
        with pytest.raises(st.StbaError) as err:
            fn()
        msg = st.lib().stba_last_error().decode()
        print("  refused:", msg)
        assert err.value.code == STBA_ERR_INVALID_ARGUMENT and "loss" in msg, msg

    def lin(cams, pts, want):
        return prob.lin_obs(cams.copy(), pts.copy(), want)

    def hook(_u, _buf, _count, _stream):
        return 0

    setters = {"host lineariser": lambda e: e.set_host_linearizer(lin), "inner iterations": lambda e: e.set_inner_iterations(True),
               "all-reduce hook": lambda e: e.set_allreduce(hook, 0, 1)}
    plain = engine(st, s).evaluate()
    table = B.loss_table("A", "huber", n)
    with_loss = engine(st, s, loss=dict(table)).evaluate()
    for what, setter in setters.items():
        e = engine(st, s, loss=dict(table))                            # the table first
        refused(lambda: setter(e))
        assert e.has_loss and same_bits(e.evaluate(), with_loss), what
        summ, _ = e.solve(max_num_iterations=2)
        assert summ.num_iterations == 2
        f = engine(st, s)                                              # the other setting first
        setter(f)
        refused(lambda: f.set_loss("huber", 0.03))
        assert not f.has_loss, what
        if what != "host lineariser":
            assert same_bits(f.evaluate(), plain), what
        f.set_loss(None)                                               # removing what is not there is no error


# ------------------------------------------------------------------------------- 3. exact steps
def make_route(st, s, table, route):
    if route == "iterative":
        e = engine(st, s, loss=dict(table), linear_solver="iterative_schur")
        e.set_pcg("jacobi", eta=1e-14, max_iterations=max(6 * len(s["cams0"]), 10) * 4)
        return e, 1e-9
    e = engine(st, s, loss=dict(table))
    if route == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
        assert e.schur_mode() == e.SCHUR_DENSE
    return e, L.EPS


@pytest.mark.parametrize("route", ["pairs", "dense", "iterative"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", list(B.LM_CASES))
def test_exact_steps_follow_the_robust_reference(st, case, k, route):
    sname, name, ok = B.SOLVE_CASES[case]
    s = B.scene(sname)
    o = L.lm_options(**ok)
    prob, ref = B.problem(sname, name), B.reference(case, k)
    e, eps_eff = make_route(st, s, prob.table, route)
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=k)))
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    assert abs(tr[0][0] - ref[0]["start"]["cost"]) <= 1e-12 * ref[0]["start"]["cost"]          # the start cost is 1/2 sum rho
    judge(prob, ref, o, x_of(e), tr, f"{case} k={k} {route}", eps_eff=eps_eff)


@pytest.mark.parametrize("form", ["pairs", "dense"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("case", list(B.DOGLEG_CASES + B.DOGLEG_LOOSE_CASES))
def test_dogleg_steps_follow_the_robust_reference(st, case, k, form):
    """scene M has A's constant dofs, constant landmarks and idle camera: the dogleg kernels' general form with masks runs a robust
    problem here.  The Tukey cases are no accuracy cases (ba_loss_ref.DOGLEG_LOOSE_CASES): the same comparison at their own kappa"""
    sname, name, ok = B.SOLVE_CASES[case]
    s = B.scene(sname)
    o = L.lm_options(**ok)
    prob, ref = B.problem(sname, name), B.reference(case, k, "dogleg")
    e = engine(st, s, loss=dict(prob.table))
    e.set_trust_region("dogleg")
    if form == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=k)))
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    kap = max(it["kappa"] for it in ref)
    assert (L.C_PATH["ba"] * kap * L.EPS <= 1e-6) == (case in B.DOGLEG_CASES) and L.rho_margin_ok(ref, o)
    fails, ratios = D.compare(prob, ref, o, x_of(e), tr)
    print(f"DOGLEG ba-loss {case} k={k} {form} kappa={kap:.2e} " + " ".join(f"{q}={v:.2e}" for q, v in sorted(ratios.items())))
    assert not fails, "; ".join(fails)
    assert [bool(v) for v in tr[1:, 6]] == [it["accepted"] for it in ref]
    assert list(e.dogleg_summary().steps_by_case) == [sum(1 for it in ref if it["case"] == c) for c in range(3)]


@pytest.mark.parametrize("route", ["pairs", "watched"])
def test_a_rejected_step_inside_three_iterations(st, route):
    s, table, o = B.reject_case()
    ref = B.reject_reference(K)
    assert [it["accepted"] for it in ref] == [False, False, True]
    prob = B.RobustBAProblem(s, table)
    e = engine(st, s, loss=dict(table))
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=K)), callback=(lambda *a: 0) if route == "watched" else None)
    assert summ.num_iterations == K
    assert [bool(v) for v in tr[1:, 6]] == [it["accepted"] for it in ref]
    judge(prob, ref, o, x_of(e), tr, f"reject {route}")


# ------------------------------------------------------------------------------- 4. routes of the loop
def decisions(summ):
    return (summ.num_iterations, summ.termination_type, summ.termination_reason, summ.num_successful_steps, summ.num_unsuccessful_steps)


def route_case(which):
    if which == "reject":
        s, table, o = B.reject_case()
        return s, table, dict(initial_trust_region_radius=o["initial_trust_region_radius"])
    sname, name, ok = B.SOLVE_CASES[which]
    s = B.scene(sname)
    return s, B.loss_table(sname, name, len(s["obs_cam"])), ok


@pytest.mark.parametrize("which", ["A_tolerant", "reject"])
def test_watched_equals_unwatched_and_a_fresh_engine_repeats_its_bits(st, which):
    s, table, ok = route_case(which)
    out = []
    for cb in (None, None, lambda *a: 0):
        e = engine(st, s, loss=dict(table))
        summ, tr = e.solve(st.default_options(**ok), callback=cb)
        assert summ.termination_type == 0, summ.as_dict()
        out.append((decisions(summ), tr, x_of(e)))
    print(f"LMROUTE ba-loss {which}: {out[0][0]}")
    for other in out[1:]:
        assert other[0] == out[0][0]
        assert other[1].tobytes() == out[0][1].tobytes() and other[2].tobytes() == out[0][2].tobytes()


@pytest.mark.parametrize("which", ["A_tolerant", "reject"])
def test_two_solves_on_one_engine(st, which):
    s, table, ok = route_case(which)
    e = engine(st, s, loss=dict(table))
    e.solve(st.default_options(**dict(ok, max_num_iterations=2)))
    cams, pts = e.get_params()
    sa, ta = e.solve(st.default_options(**ok))
    f = engine(st, dict(s, cams0=cams, pts0=pts), loss=dict(table))
    sb, tb = f.solve(st.default_options(**ok))
    assert decisions(sa) == decisions(sb), (sa.as_dict(), sb.as_dict())
    assert ta.tobytes() == tb.tobytes() and x_of(e).tobytes() == x_of(f).tobytes()


# ------------------------------------------------------------------------------- 5. outliers
def test_cauchy_solve_ends_at_the_robust_reference_not_the_l2_one(st):
    s, bad = B.outlier_scene()
    x_l2, x_rob, cost_rob, table = B.outlier_references()
    e = engine(st, s, loss=dict(table))
    summ, _ = e.solve(function_tolerance=1e-12, parameter_tolerance=1e-11)
    x = x_of(e)
    prob = L.ba_problem(s)
    d_dev, d_l2 = B.distance_to_truth(prob, s, x), B.distance_to_truth(prob, s, x_l2)
    gap = abs(summ.final_cost - cost_rob) / cost_rob
    print(f"  outliers: device cost {summ.final_cost:.12e} ({summ.num_iterations} iterations) reference {cost_rob:.12e} gap {gap:.2e}; "
          f"|x - truth| device {d_dev:.4f}, L2 reference {d_l2:.4f}, robust reference {B.distance_to_truth(prob, s, x_rob):.4f}")
    assert summ.termination_type == 0
    assert gap <= 1e-6 and d_dev < d_l2


# ------------------------------------------------------------------------------- 6. covariance
def numpy_covariance(prob, x):
    """(J'^T J')^-1 over the free columns at x, embedded with zeros at the constant ones; kappa of J'^T J'"""
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


def test_covariance_is_the_inverse_of_the_corrected_normal_matrix(st):
    s = B.scene("B")
    n = len(s["obs_cam"])
    table = B.loss_table("B", "cauchy", n)
    e = engine(st, s, loss=dict(table))
    e.solve()
    cams, pts = e.get_params()
    nc, np_ = len(cams), len(pts)
    x = x_of(e)
    prob = B.RobustBAProblem(s, table)
    C, kappa = numpy_covariance(prob, x)
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
    print(f"  covariance: kappa(J'^T J') {kappa:.3e} pivot ratio {rc:.3e} tolerance {tol:.3e} worst relative Frobenius error {worst:.3e}")
    assert worst <= tol
    # the lossless covariance at the same point is another matrix by far
    f = engine(st, dict(s, cams0=cams, pts0=pts))
    cam0, pb0, _ = f.covariance(cam_pairs=pairs[:nc])
    far = max(np.linalg.norm(cam0[c] - C[6 * c:6 * c + 6, 6 * c:6 * c + 6]) / np.linalg.norm(C[6 * c:6 * c + 6, 6 * c:6 * c + 6])
              for c in range(nc) if np.linalg.norm(C[6 * c:6 * c + 6, 6 * c:6 * c + 6]) > 0)
    print(f"  lossless covariance differs by {far:.3e} relative")
    assert far > 1e3 * tol
    # a new table releases the held covariance
    e.set_loss(None)
    with pytest.raises(st.StbaError):
        n_ = np.zeros((1, 6, 6)); a_ = np.zeros(1, np.int32)
        st._chk(st.lib().stba_ba_camera_covariance(e._h, 1, st._p(a_), st._p(a_), st._p(n_)), "stba_ba_camera_covariance")


# ------------------------------------------------------------------------------- 7. a landmark without weight
def test_tukey_that_switches_a_landmark_off(st):
    """Tukey with a tiny a on every observation of one landmark of A: every one of them has weight zero, the landmark's blocks are zero.
    An input-handling test: the solve returns finite parameters and leaves that landmark where it was; a covariance request returns
    finite numbers or is refused with a status code"""
    s = B.scene("A")
    n = len(s["obs_cam"])
    j = int(np.flatnonzero((np.bincount(s["obs_pt"]) >= 3) & (s["pt_fixed"] == 0))[0])
    on = s["obs_pt"] == j
    table = B.table_of(np.where(on, 6, 0), np.where(on, 1e-9, 1.0), 1.0, 1.0, n)
    e = engine(st, s, loss=dict(table))
    _, r, Jc, Jp = e.evaluate()
    assert np.all(r[on] == 0.0) and np.all(Jc[on] == 0.0) and np.all(Jp[on] == 0.0) and np.any(r[~on] != 0.0)
    summ, tr = e.solve(max_num_iterations=5)
    cams, pts = e.get_params()
    print(f"  landmark {j} ({int(on.sum())} observations) switched off: {summ.as_dict()}")
    assert np.isfinite(cams).all() and np.isfinite(pts).all() and np.isfinite(tr).all()
    assert np.array_equal(pts[j], s["pts0"][j]) and not np.array_equal(pts, s["pts0"])
    try:
        cam, pb, rc = e.covariance()
        assert np.isfinite(cam).all() and np.isfinite(pb).all()
    except st.StbaError as err:
        print("  covariance refused:", err.code, st.lib().stba_last_error().decode())
        assert err.code != 0
