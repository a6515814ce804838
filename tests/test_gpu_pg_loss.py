"""The pose graph's robust losses on the GPU (PGEngine(loss=), stba_pg_set_loss): the correcting linearisation kernel and everything
behind it against tests/pg_loss_ref.py -- two graphs (179 edges: one workgroup; 304 edges: a second, partly filled one) x five loss
sets (Huber, Cauchy on the dense weights, Tolerant, Tukey on the loop closures; every kind spread over all edges).

Bounds:
  evaluate    cost to 1e-12 relative (the existing bound).  r', Ji', Jj' against the oracle's r, Ji, Jj whitened and corrected in numpy:
              the uncorrected entry's existing bound (1e-12 for r, 1e-11 for J, or pg_information_ref.whiten_bound on the weighted set)
              times the magnitude of the correction factor (|rs| for r; |M| = |sqrt(rho') (I - (alpha / s) r r^T)| as a matrix for J)
              plus c eps |entry|, c = 8 x (the worst error of the numpy rho', rho'' against 50 digits, in eps) + 16 per kind.  Measured
              on the CPU (tests/test_pg_loss_cpu.py): huber 1.01, softlone 1.37, cauchy 2.06, arctan 1.98, tolerant 25.0, tukey 428
              eps, so c = 24.8, 27.2, 32.8, 32, 224 and 3456 (pg_loss_ref.RHO_EPS, c_of);
  solve       lm_step_ref.compare / tolerances on the robust reference with eps_eff = max(eps, PCG_TOL), as tests/test_gpu_pg_information.py;
  production  final cost within 1e-6 relative of the exact-step run, hit_cap == 0;
  covariance  pg_covariance_ref.block_bound on (J'^T J')^-1.
Each case prints its figures before it asserts."""
import importlib

import numpy as np
import pytest

import lm_step_ref as L
import pg_covariance_ref as C
import pg_information_ref as P
import pg_loss_ref as R

pytestmark = pytest.mark.gpu

STBA_ERR_INVALID_ARGUMENT = -1
K = 3
SOLVE_CASES = [(g, s) for g in P.GRAPHS for s in R.SOLVE_SETS]
EVAL_CASES = [(g, s) for g in P.GRAPHS for s in R.LOSS_SETS]


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def engine(st, g, **kw):
    return st.PGEngine(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"], **kw)


def oracle_eval(O, g):
    return O.PG(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"]).evaluate()


def same_bits(x, y):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))


def check_eval(label, got, W, table, oracle, weighted):
    """got = (cost, r, Ji, Jj) of the device against the oracle's (r, Ji, Jj) whitened by W and corrected; returns the worst
    err / bound and the cost's relative error"""
    cost, r, Ji, Jj = got
    ro, Jio, Jjo = oracle
    rw, Jiw, Jjw = P.whiten(W, ro, Jio, Jjo)
    rc, Jic, Jjc, terms = R.correct(rw, Jiw, Jjw, table)
    cw = float(0.5 * np.sum(terms.astype(np.longdouble)))
    worst = 0.0
    for name, a, b, x, base in (("r", r, rc, ro, 1e-12), ("Ji", Ji, Jic, Jio, 1e-11), ("Jj", Jj, Jjc, Jjo, 1e-11)):
        before = P.whiten_bound(W, x, base) if weighted else np.full(x.shape, base)
        err, bound = np.abs(a - b), R.corrected_bound(rw, table, b, before)
        # (a Tukey edge beyond a^2 has r' = 0 and J' = 0 exactly, and a bound of zero: there the device must give zero too)
        ratio = np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)))
        worst = max(worst, ratio)
        print(f"  {label} {name}: max err {err.max():.3e}, max err / bound {ratio:.3e}")
    print(f"  {label} cost {cost:.17g} reference {cw:.17g} relative {abs(cost - cw) / cw:.2e}")
    return worst, abs(cost - cw) / cw


# ------------------------------------------------------------------------------- 1. evaluate
@pytest.mark.parametrize("gname,name", EVAL_CASES)
def test_evaluate_is_the_corrected_oracle(st, O, gname, name):
    g = P.graph(gname)
    table, wname = R.loss_set(gname, name)
    W = R.sqrt_information(gname, name)
    _, ro, Jio, Jjo = oracle_eval(O, g)
    e = engine(st, g, **R.engine_kwargs(gname, name))
    assert e.has_loss and e.has_information == (wname is not None)
    got = e.evaluate()
    worst, crel = check_eval(f"{gname} {name}", got, W, table, (ro, Jio, Jjo), wname is not None)
    assert worst <= 1.0 and crel <= 1e-12
    _, r, Ji, Jj = got
    fx = np.flatnonzero(g["node_fixed"])
    assert np.all(Ji[np.isin(g["edge_i"], fx)] == 0) and np.all(Jj[np.isin(g["edge_j"], fx)] == 0)      # constant nodes: columns dropped
    assert np.any(Ji[~np.isin(g["edge_i"], fx)] != 0)
    # edges without a loss (kind 0, scale 1) compare == with the engine that has no table
    kw = P.engine_kwargs(gname, wname) if wname else {}
    _, r0, Ji0, Jj0 = engine(st, g, **kw).evaluate()
    keep = R.untouched(table)
    assert keep.any() and np.array_equal(r[keep], r0[keep]) and np.array_equal(Ji[keep], Ji0[keep]) and np.array_equal(Jj[keep], Jj0[keep])
    assert not np.array_equal(r[~keep], r0[~keep])


def test_zero_residuals_take_the_first_corrector_branch(st):
    """s == 0 exactly (identity poses, identity measurements), every kind: r' = 0, J' = sqrt(rho'(0)) J to the last bit but one"""
    g, table = R.zero_graph()
    m = len(g["edge_i"])
    cost0, r0, Ji0, Jj0 = engine(st, g).evaluate()
    cost, r, Ji, Jj = engine(st, g, loss=dict(table)).evaluate()
    _, sq, _, _ = R.factors(table, np.zeros(m))
    assert cost0 == 0.0 and np.all(r0 == 0.0) and np.all(r == 0.0) and np.isfinite(Ji).all() and np.isfinite(Jj).all()
    print(f"  zero graph: cost {cost!r}; sqrt(rho'(0)) from {sq.min():.3g} to {sq.max():.3g}")
    assert abs(cost) <= 1e-15                      # (SoftLOne, Cauchy, Tolerant, Tukey give rho(0) = 0 up to their own rounding)
    for J, J0 in ((Ji, Ji0), (Jj, Jj0)):
        want = sq[:, None, None] * J0
        assert np.all(np.abs(J - want) <= R.c_of(table["kind"])[:, None, None] * L.EPS * np.abs(want))
    assert np.any(Jj != Jj0)


# ------------------------------------------------------------------------------- 2. setters
@pytest.mark.parametrize("gname", P.GRAPHS)
def test_none_restores_the_engine_without_a_loss_bit_for_bit(st, gname):
    g = P.graph(gname)
    fresh = engine(st, g)
    e = engine(st, g, **R.engine_kwargs(gname, "huber"))
    assert e.has_loss and not fresh.has_loss
    assert not same_bits(e.evaluate(), fresh.evaluate())
    e.set_loss(None)
    assert not e.has_loss and same_bits(e.evaluate(), fresh.evaluate())
    e.set_loss("cauchy", 0.5); e.set_loss(None)
    assert not e.has_loss and same_bits(e.evaluate(), fresh.evaluate())
    sa, ta, na = e.solve(max_num_iterations=6)
    sb, tb, nb = fresh.solve(max_num_iterations=6)
    assert np.array_equal(ta, tb) and np.array_equal(e.get_poses(), fresh.get_poses()) and na == nb


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("gname", P.GRAPHS)
def test_an_all_trivial_table_is_the_engine_without_a_table(st, gname, weighted):
    g = P.graph(gname)
    kw = P.engine_kwargs(gname, "dense") if weighted else {}
    a, b = engine(st, g, loss="trivial", **kw), engine(st, g, **kw)
    assert a.has_loss and not b.has_loss
    assert same_bits(a.evaluate(), b.evaluate())
    sa, ta, _ = a.solve(max_num_iterations=6)
    sb, tb, _ = b.solve(max_num_iterations=6)
    assert sa.num_iterations == sb.num_iterations > 0 and np.array_equal(ta, tb) and np.array_equal(a.get_poses(), b.get_poses())


def test_bad_tables_are_refused_with_the_edge_named_and_the_table_kept(st):
    g = P.graph("n40_pad")
    table, _ = R.loss_set("n40_pad", "mixed")
    e = engine(st, g, loss=dict(table))
    before = e.evaluate()

    def refused(edge, **change):
        bad = {k: v.copy() for k, v in table.items()}
        for key, (at, val) in change.items():
            for a_, v_ in zip(np.atleast_1d(at), np.atleast_1d(val)):
                bad[key][a_] = v_
        with pytest.raises(st.StbaError) as err:
            e.set_loss(**bad)
        msg = st.lib().stba_last_error().decode()
        print("  refused:", msg)
        assert err.value.code == STBA_ERR_INVALID_ARGUMENT and f"edge {edge}:" in msg, msg
        assert e.has_loss and same_bits(e.evaluate(), before)

    refused(5, kind=([5, 300], [7, -1]))                                   # unknown kinds: the smallest edge
    refused(300, kind=(300, 9))
    refused(5, kind=([5, 300], [1, 1]), a=([5, 300], [0.0, np.nan]))       # a not positive / not finite
    refused(300, kind=(300, 3), a=(300, np.inf))
    refused(5, kind=([5, 300], [5, 5]), b=([5, 300], [-1.0, 0.0]))         # b of a Tolerant edge
    refused(300, kind=(300, 5), b=(300, np.nan))
    refused(5, scale=([5, 300], [-0.5, np.nan]))
    refused(300, scale=(300, np.inf))
    # parameters the kind does not use are not read: a NaN b on a Huber edge, a NaN a on an edge without a loss
    ok = {k: v.copy() for k, v in table.items()}
    ok["kind"][[5, 300]] = [1, 0]; ok["b"][5] = np.nan; ok["a"][300] = np.nan
    e.set_loss(**ok)
    assert e.has_loss and np.isfinite(e.evaluate()[0])
    # an engine WITHOUT a table that refuses stays without
    f = engine(st, g)
    with pytest.raises(st.StbaError):
        f.set_loss(np.full(len(g["edge_i"]), 9), 1.0)
    assert not f.has_loss and same_bits(f.evaluate(), engine(st, g).evaluate())


# ------------------------------------------------------------------------------- 3. exact steps
def judge(prob, ref, o, x_dev, trace, label):
    """tests/test_gpu_pg_information.py's judge, word for word in what it checks"""
    eps_eff = max(L.EPS, L.PCG_TOL)
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["pg"] * kap * eps_eff <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = L.compare(prob, ref, "pg", o, x_dev, trace, eps_eff=eps_eff)
    print(f"LMSTEP pg-loss {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    assert not fails, f"{label}: " + "; ".join(fails)


ROUTES = {"launches": dict(one_kernel_solve=0, coarse_group=0), "one_kernel": dict(one_kernel_solve=1, coarse_group=0),
          "no_coarse": dict(one_kernel_solve=1, coarse_group=-1)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("gname,name", SOLVE_CASES)
def test_exact_steps_follow_the_robust_reference(st, gname, name, route):
    g = P.graph(gname)
    o = L.lm_options(**P.LM_OPTIONS)
    prob, ref = R.problem(gname, name), R.reference(gname, name, K)
    e = engine(st, g, **R.engine_kwargs(gname, name))
    pc = e.pcg_options(forcing_eta0=0.0, relative_tolerance=L.PCG_TOL, **ROUTES[route])
    summ, tr, _ = e.solve(st.default_options(**dict(o, max_num_iterations=K)), pcg=pc)
    assert summ.num_iterations == K and len(tr) == K + 1, summ.as_dict()
    ps = e.pcg_summary()
    # (hit_cap is printed, not judged, as in tests/test_gpu_pg_information.py: at 1e-14 the one-kernel PCG can end by its breakdown guard)
    print(f"  {gname} {name} {route}: PCG iterations {ps.iterations_total}, most in a solve {ps.max_iterations_in_a_solve}, hit_cap {ps.hit_cap}")
    assert ps.max_iterations_in_a_solve < pc.max_iterations and (ps.coarse_dim > 0) == (route != "no_coarse")
    assert (ps.one_kernel_solves == K) == (route == "one_kernel"), (route, ps.one_kernel_solves)
    assert abs(tr[0][0] - ref[0]["start"]["cost"]) <= 1e-12 * ref[0]["start"]["cost"]          # the start cost is 1/2 sum rho
    judge(prob, ref, o, e.get_poses().reshape(-1), tr, f"{gname} {name} {route}")


# ------------------------------------------------------------------------------- 4. production
@pytest.mark.parametrize("gname,name", SOLVE_CASES)
def test_production_forcing_reaches_the_exact_step_cost(st, gname, name):
    g = P.graph(gname)
    tight = dict(function_tolerance=1e-12, parameter_tolerance=1e-11)
    a, b = engine(st, g, **R.engine_kwargs(gname, name)), engine(st, g, **R.engine_kwargs(gname, name))
    sa, _, _ = a.solve(**tight)
    sb, _, _ = b.solve(pcg=b.pcg_options(forcing_eta0=0.0), **tight)
    gap = abs(sa.final_cost - sb.final_cost) / sb.final_cost
    print(f"  {gname} {name}: production {sa.final_cost:.12e} ({sa.num_iterations} iterations) exact steps {sb.final_cost:.12e} "
          f"({sb.num_iterations}) relative gap {gap:.2e}")
    assert sa.termination_type == 0 and sb.termination_type == 0 and a.pcg_summary().hit_cap == 0
    assert sa.final_cost < 0.5 * sa.initial_cost
    assert gap <= 1e-6


# ------------------------------------------------------------------------------- 5. outliers
def test_cauchy_solve_ends_at_the_robust_reference_not_the_l2_one(st):
    g, bad = R.outlier_graph()
    x_l2, x_rob, cost_rob, table = R.outlier_references()
    e = engine(st, g, loss=dict(table))
    summ, _, _ = e.solve(function_tolerance=1e-12, parameter_tolerance=1e-11)
    x = e.get_poses().reshape(-1)
    prob = L.pg_problem(g)
    d_rob, d_l2 = L.point_error(prob, x, x_rob), L.point_error(prob, x, x_l2)
    gap = abs(summ.final_cost - cost_rob) / cost_rob
    print(f"  outliers {bad.tolist()}: device cost {summ.final_cost:.12e} reference {cost_rob:.12e} gap {gap:.2e}; "
          f"|x - robust reference| {d_rob:.3e}, |x - L2 reference| {d_l2:.3e}")
    assert summ.termination_type == 0 and e.pcg_summary().hit_cap == 0
    assert gap <= 1e-6 and d_rob < d_l2


# ------------------------------------------------------------------------------- 6. covariance
@pytest.mark.parametrize("gname", P.GRAPHS)
def test_covariance_is_the_inverse_of_the_corrected_normal_matrix(st, O, gname):
    import scipy.sparse as sp
    g = P.graph(gname)
    n, m = len(g["poses0"]), len(g["edge_i"])
    table, wname = R.loss_set(gname, "cauchy_w")
    W = R.sqrt_information(gname, "cauchy_w")
    _, ro, _, _ = oracle_eval(O, g)
    Mc, _ = R.correction_matrix(P.whiten(W, ro), table)
    J = sp.block_diag([Mc[e] for e in range(m)], format="csr") @ P.whitened_jacobian(O, g, W)
    Cs, lam_min, kappa = C.dense_covariance((J.T @ J).tocsc(), g["node_fixed"])
    pairs = [(1, 1), (n // 2 - 1, n // 2 - 1), (n // 2 - 1, n // 2 + 1), (n // 2 + 1, n // 2 - 1), (n - 1, n - 1), (n - 1, 3), (0, 5), (7, n // 2)]
    e = engine(st, g, **R.engine_kwargs(gname, "cauchy_w"))
    Cd, summ = e.covariance(pairs, relative_tolerance=1e-12)
    rho = summ["max_relative_residual"]
    bound = C.block_bound(rho, kappa, lam_min)
    print(f"  {gname}: lambda_min {lam_min:.3e} kappa {kappa:.3e} rho {rho:.3e} bound {bound:.3e}")
    assert rho <= 1e-12
    lossless, _ = engine(st, g, **P.engine_kwargs(gname, wname)).covariance(pairs[:1], relative_tolerance=1e-12)
    for k, (a, b) in enumerate(pairs):
        ref = C.block(Cs, a, b)
        err = np.linalg.norm(Cd[k] - ref)
        print(f"    C[{a},{b}] |err|_F {err:.3e} |C*|_F {np.linalg.norm(ref):.3e} err / bound {err / bound:.3e}")
        assert err <= bound, (a, b, err, bound)
    assert np.all(Cd[6] == 0) and np.all(Cd[7] == 0)                   # pairs that name a constant node
    assert np.linalg.norm(lossless[0] - C.block(Cs, 1, 1)) > 1e3 * bound      # the lossless covariance is another matrix by far
