"""Pose-graph edge information matrices on the GPU (PGEngine(information= / sqrt_information=), stba_pg_set_information): the whitening
linearisation kernel and everything behind it against the whitened references of tests/pg_information_ref.py -- two graphs (179 edges:
one workgroup; 304 edges: a second, partly filled one) x three weight sets (diagonal, dense SPD, a general W through the sqrt entry
point).

Bounds (none of them is new):
  evaluate    |got - want| <= 32 eps sum_k |W_ak| |x_k| + the unweighted evaluate test's bound for x (1e-12 for r, 1e-11 for J), the
              cost to 1e-12 relative -- against the oracle's r, Ji, Jj whitened in numpy;
  solve       lm_step_ref.compare / tolerances on the whitened problem with eps_eff = max(eps, PCG_TOL), exactly as the unweighted case
              of tests/test_gpu_lm_step.py (on the reference's side no weighted case asks for more: its first step is 0.026 kappa eps
              from a 50-digit redo, tests/test_pg_information_cpu.py);
  production  final cost within 1e-6 relative of the exact-step run (tests/test_gpu_pose_graph.py's gap for the unweighted graph);
  covariance  pg_covariance_ref.block_bound on (J~^T J~)^-1.
Each case prints its figures before it asserts."""
import importlib

import numpy as np
import pytest

import lm_step_ref as L
import pg_covariance_ref as R
import pg_information_ref as P

pytestmark = pytest.mark.gpu

STBA_ERR_INVALID_ARGUMENT = -1
STBA_ERR_NOT_POSITIVE_DEFINITE = -4
CASES = [(g, w) for g in P.GRAPHS for w in P.WEIGHTS]
K = 3


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def engine(st, g, **kw):
    return st.PGEngine(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"], **kw)


def oracle_eval(O, g):
    return O.PG(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"]).evaluate()


def check_eval(label, got, W, unweighted):
    """got = (cost, r, Ji, Jj) of the device against the whitened `unweighted` = (r, Ji, Jj); returns the worst err / bound"""
    cost, r, Ji, Jj = got
    ro, Jio, Jjo = unweighted
    rw, Jiw, Jjw = P.whiten(W, ro, Jio, Jjo)
    cw = float(0.5 * np.sum(rw.astype(np.longdouble) ** 2))
    worst = 0.0
    for name, a, b, x, base in (("r", r, rw, ro, 1e-12), ("Ji", Ji, Jiw, Jio, 1e-11), ("Jj", Jj, Jjw, Jjo, 1e-11)):
        err, bound = np.abs(a - b), P.whiten_bound(W, x, base)
        worst = max(worst, (err / bound).max())
        print(f"  {label} {name}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3e}")
    print(f"  {label} cost {cost:.17g} reference {cw:.17g} relative {abs(cost - cw) / cw:.2e}")
    return worst, abs(cost - cw) / cw


# ------------------------------------------------------------------------------- 1. evaluate
@pytest.mark.parametrize("gname,kind", CASES)
def test_evaluate_is_the_whitened_oracle(st, O, gname, kind):
    g = P.graph(gname)
    _, W = P.weights(gname, kind)
    _, ro, Jio, Jjo = oracle_eval(O, g)
    e = engine(st, g, **P.engine_kwargs(gname, kind))
    assert e.has_information
    worst, crel = check_eval(f"{gname} {kind}", e.evaluate(), W, (ro, Jio, Jjo))
    assert worst <= 1.0 and crel <= 1e-12
    _, _, Ji, Jj = e.evaluate()
    fx = np.flatnonzero(g["node_fixed"])
    assert np.all(Ji[np.isin(g["edge_i"], fx)] == 0) and np.all(Jj[np.isin(g["edge_j"], fx)] == 0)      # constant nodes: columns dropped
    assert np.any(Ji[~np.isin(g["edge_i"], fx)] != 0)


# ------------------------------------------------------------------------------- 2. setters
@pytest.mark.parametrize("gname", P.GRAPHS)
def test_information_and_its_factor_give_the_same_engine(st, O, gname):
    """set_information(Omega) against set_sqrt_information(chol(Omega)^T), the factor made at 50 digits and rounded (pg_information_ref.chol_T:
    the device factors in double-double, so both are the correctly rounded W; LAPACK's FP64 factor is itself cond(Omega) eps away --
    its figure is printed, not judged)"""
    g = P.graph(gname)
    om, W = P.weights(gname, "dense")
    _, ro, Jio, Jjo = oracle_eval(O, g)
    a, b = engine(st, g, information=om), engine(st, g, sqrt_information=W)
    ea, eb = a.evaluate(), b.evaluate()
    worst = 0.0
    for name, x, y, base_x, base in (("r", ea[1], eb[1], ro, 1e-12), ("Ji", ea[2], eb[2], Jio, 1e-11), ("Jj", ea[3], eb[3], Jjo, 1e-11)):
        ratio = (np.abs(x - y) / P.whiten_bound(W, base_x, base)).max()
        print(f"  {gname} {name}: information against its 50-digit factor, max |difference| {np.abs(x - y).max():.3e}, / bound {ratio:.3e}")
        worst = max(worst, ratio)
    c = engine(st, g, sqrt_information=np.linalg.cholesky(om).transpose(0, 2, 1)).evaluate()
    print(f"  {gname}: against LAPACK's factor (not judged) max |r difference| {np.abs(ea[1] - c[1]).max():.3e}, "
          f"/ bound {(np.abs(ea[1] - c[1]) / P.whiten_bound(W, ro, 1e-12)).max():.3e}")
    assert worst <= 1.0 and abs(ea[0] - eb[0]) <= 1e-12 * eb[0]


def same_bits(x, y):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))


@pytest.mark.parametrize("gname", P.GRAPHS)
def test_null_restores_the_engine_without_weights_bit_for_bit(st, gname):
    g = P.graph(gname)
    om, W = P.weights(gname, "dense")
    fresh = engine(st, g)
    e = engine(st, g, information=om)
    assert e.has_information and not fresh.has_information
    assert not same_bits(e.evaluate(), fresh.evaluate())
    e.set_information(None)
    assert not e.has_information and same_bits(e.evaluate(), fresh.evaluate())
    e.set_sqrt_information(W); e.set_sqrt_information(None)
    assert not e.has_information and same_bits(e.evaluate(), fresh.evaluate())
    # and the solve behind it: trace and poses, every double
    sa, ta, na = e.solve(max_num_iterations=6)
    sb, tb, nb = fresh.solve(max_num_iterations=6)
    assert np.array_equal(ta, tb) and np.array_equal(e.get_poses(), fresh.get_poses()) and na == nb


@pytest.mark.parametrize("how", ["information", "sqrt_information"])
@pytest.mark.parametrize("gname", P.GRAPHS)
def test_identity_weights_are_the_unweighted_engine(st, gname, how):
    """products with exact 1 and 0 add nothing: cost trace and final poses compare == to the unweighted engine's"""
    g = P.graph(gname)
    eye = np.tile(np.eye(6), (len(g["edge_i"]), 1, 1))
    a, b = engine(st, g, **{how: eye}), engine(st, g)
    assert a.has_information
    ea, eb = a.evaluate(), b.evaluate()
    assert ea[0] == eb[0] and all(np.all(x == y) for x, y in zip(ea[1:], eb[1:]))
    sa, ta, _ = a.solve()
    sb, tb, _ = b.solve()
    assert sa.num_iterations == sb.num_iterations > 0 and np.all(ta == tb) and np.all(a.get_poses() == b.get_poses())


def test_bad_matrices_are_refused_with_the_edge_named_and_the_weights_kept(st):
    g = P.graph("n40_pad")
    om, W = P.weights("n40_pad", "dense")
    e = engine(st, g, information=om)
    before = e.evaluate()

    def refused(call, arr, code, edge):
        with pytest.raises(st.StbaError) as err:
            call(arr)
        msg = st.lib().stba_last_error().decode()
        print("  refused:", msg)
        assert err.value.code == code and f"edge {edge}:" in msg, msg
        assert e.has_information and same_bits(e.evaluate(), before)

    indef = np.diag([1.0, 1.0, -1.0, 1.0, 1.0, 1.0])
    both = om.copy(); both[5] = indef; both[300, 0, 5] = np.nan           # (the NaN sits in the upper triangle, which is not factored)
    refused(e.set_information, both, STBA_ERR_NOT_POSITIVE_DEFINITE, 5)          # the smallest failing edge
    nan = om.copy(); nan[300, 0, 5] = np.nan
    refused(e.set_information, nan, STBA_ERR_NOT_POSITIVE_DEFINITE, 300)
    late = om.copy(); late[299] = indef; late[303] = 0.0
    refused(e.set_information, late, STBA_ERR_NOT_POSITIVE_DEFINITE, 299)
    semi = om.copy(); semi[256] = np.ones((6, 6))                           # rank one: the second pivot is zero
    refused(e.set_information, semi, STBA_ERR_NOT_POSITIVE_DEFINITE, 256)
    winf = W.copy(); winf[300, 4, 1] = np.inf; winf[302, 0, 0] = np.nan
    refused(e.set_sqrt_information, winf, STBA_ERR_INVALID_ARGUMENT, 300)
    # an engine WITHOUT weights that refuses stays without
    f = engine(st, g)
    with pytest.raises(st.StbaError):
        f.set_information(nan)
    assert not f.has_information and same_bits(f.evaluate(), engine(st, g).evaluate())


# ------------------------------------------------------------------------------- 3. solve
def judge(prob, ref, o, x_dev, trace, label):
    """tests/test_gpu_lm_step.py's judge for its pose-graph case, word for word in what it checks"""
    eps_eff = max(L.EPS, L.PCG_TOL)
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["pg"] * kap * eps_eff <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = L.compare(prob, ref, "pg", o, x_dev, trace, eps_eff=eps_eff)
    print(f"LMSTEP pg-information {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    assert not fails, f"{label}: " + "; ".join(fails)


ROUTES = {"launches": dict(one_kernel_solve=0, coarse_group=0), "one_kernel": dict(one_kernel_solve=1, coarse_group=0),
          "no_coarse": dict(one_kernel_solve=1, coarse_group=-1)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("gname,kind", CASES)
def test_exact_steps_follow_the_whitened_reference(st, gname, kind, route):
    g = P.graph(gname)
    o = L.lm_options(**P.LM_OPTIONS)
    prob, ref = P.problem(gname, kind), P.reference(gname, kind, K)
    e = engine(st, g, **P.engine_kwargs(gname, kind))
    pc = e.pcg_options(forcing_eta0=0.0, relative_tolerance=L.PCG_TOL, **ROUTES[route])
    summ, tr, _ = e.solve(st.default_options(**dict(o, max_num_iterations=K)), pcg=pc)
    assert summ.num_iterations == K and len(tr) == K + 1, summ.as_dict()
    ps = e.pcg_summary()
    # (hit_cap is printed, not judged: at a relative tolerance of 1e-14 the one-kernel PCG's recurrence can lose den > 0 in the last
    # iterations and end by its breakdown guard, which it reports as a capped solve -- n60 sqrt one_kernel, 286 iterations of a cap
    # of 1000; what the step is worth is judged below.  The production solves assert hit_cap == 0.)
    print(f"  {gname} {kind} {route}: PCG iterations {ps.iterations_total}, most in a solve {ps.max_iterations_in_a_solve}, hit_cap {ps.hit_cap}")
    assert ps.max_iterations_in_a_solve < pc.max_iterations and (ps.coarse_dim > 0) == (route != "no_coarse")
    assert (ps.one_kernel_solves == K) == (route == "one_kernel"), (route, ps.one_kernel_solves)
    judge(prob, ref, o, e.get_poses().reshape(-1), tr, f"{gname} {kind} {route}")


@pytest.mark.parametrize("gname,kind", CASES)
def test_production_forcing_reaches_the_exact_step_cost(st, gname, kind):
    g = P.graph(gname)
    tight = dict(function_tolerance=1e-12, parameter_tolerance=1e-11)
    a, b = engine(st, g, **P.engine_kwargs(gname, kind)), engine(st, g, **P.engine_kwargs(gname, kind))
    sa, _, _ = a.solve(**tight)
    sb, _, _ = b.solve(pcg=b.pcg_options(forcing_eta0=0.0), **tight)
    gap = abs(sa.final_cost - sb.final_cost) / sb.final_cost
    print(f"  {gname} {kind}: production {sa.final_cost:.12e} ({sa.num_iterations} iterations) exact steps {sb.final_cost:.12e} "
          f"({sb.num_iterations}) relative gap {gap:.2e}")
    assert sa.termination_type == 0 and sb.termination_type == 0 and a.pcg_summary().hit_cap == 0
    assert sa.final_cost < 0.5 * sa.initial_cost
    assert gap <= 1e-6


# ------------------------------------------------------------------------------- 4. covariance
def covariance_reference(O, gname, kind="dense"):
    g = P.graph(gname)
    J = P.whitened_jacobian(O, g, P.weights(gname, kind)[1])
    return R.dense_covariance((J.T @ J).tocsc(), g["node_fixed"])


def covariance_pairs(g):
    n = len(g["poses0"])
    return [(1, 1), (n // 2 - 1, n // 2 - 1), (n // 2 - 1, n // 2 + 1), (n // 2 + 1, n // 2 - 1), (n - 1, n - 1), (n - 1, 3), (0, 5), (7, n // 2)]


@pytest.mark.parametrize("gname", P.GRAPHS)
def test_covariance_is_the_inverse_of_the_weighted_normal_matrix(st, O, gname):
    g = P.graph(gname)
    Cs, lam_min, kappa = covariance_reference(O, gname)
    pairs = covariance_pairs(g)
    e = engine(st, g, **P.engine_kwargs(gname, "dense"))
    C, summ = e.covariance(pairs, relative_tolerance=1e-12)
    rho = summ["max_relative_residual"]
    bound = R.block_bound(rho, kappa, lam_min)
    print(f"  {gname}: lambda_min {lam_min:.3e} kappa {kappa:.3e} rho {rho:.3e} bound {bound:.3e}")
    assert rho <= 1e-12
    plain, _ = engine(st, g).covariance(pairs[:1], relative_tolerance=1e-12)
    for k, (a, b) in enumerate(pairs):
        ref = R.block(Cs, a, b)
        err = np.linalg.norm(C[k] - ref)
        print(f"    C[{a},{b}] |err|_F {err:.3e} |C*|_F {np.linalg.norm(ref):.3e} err / bound {err / bound:.3e}")
        assert err <= bound, (a, b, err, bound)
    assert np.all(C[6] == 0) and np.all(C[7] == 0)                     # pairs that name a constant node
    assert np.linalg.norm(plain[0] - R.block(Cs, 1, 1)) > 1e3 * bound      # (J^T J)^-1 is another matrix by far
