"""Node pose priors of the pose graph on the GPU (PGEngine(priors=), stba_pg_set_priors) against the references the suite already has,
run on the AUGMENTED graph of tests/pg_prior_ref.py: one more node at the identity, constant, and one weighted edge per prior.

Bounds (none of them is new):
  evaluate    |got - want| <= 32 eps sum_k |W_ak| |x_k| + 1e-12 (r) / 1e-11 (J): pg_information_ref.whiten_bound on the oracle's rows
              of the augmented edges; the cost of the sum to 1e-12 relative;
  LM steps    lm_step_ref.compare / tolerances with eps_eff = max(eps, PCG_TOL), exactly as tests/test_gpu_pg_information.py, on each
              of the four solver paths of lm_step_ref.PG_PCG -- a launch product without Hp, a p.q without p^T Hp p, a trial |J x|^2
              without the priors or a coarse inverse made from a stale Hd all move the step by far more;
  production  final cost within 1e-6 relative of the exact-step run (tests/test_gpu_pose_graph.py's gap);
  covariance  pg_covariance_ref.block_bound against (J^T J)^-1 of the augmented graph.
Each case prints its figures before it asserts."""
import importlib

import numpy as np
import pytest

import lm_step_ref as L
import pg_covariance_ref as R
import pg_information_ref as P
import pg_loss_ref as PL
import pg_prior_ref as Q

pytestmark = pytest.mark.gpu

STBA_ERR_INVALID_ARGUMENT = -1
STBA_ERR_NOT_POSITIVE_DEFINITE = -4
K = 3
CASES = [("n60", "few"), ("n60", "dense"), ("n40_pad", "many"), ("n40_pad", "gps"), ("n150", "few"), ("n60_free", "few")]


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def engine(st, g, pr=None, **kw):
    if pr is not None:
        kw["priors"] = Q.engine_kwargs(pr)
    return st.PGEngine(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"], **kw)


def same_bits(x, y):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))


def last_error(st):
    return st.lib().stba_last_error().decode()


# ------------------------------------------------------------------------------- 1. evaluate
@pytest.mark.parametrize("gname,kind", CASES)
def test_evaluate_is_the_whitened_oracle_on_the_augmented_edges(st, O, gname, kind):
    g, pr = Q.graph(gname), Q.priors(gname, kind)
    a = Q.augment(g, pr)
    m, W = len(g["edge_i"]), pr["W"]
    _, ro, _, Jjo = O.PG(a["poses0"], a["edge_i"], a["edge_j"], a["meas"], a["node_fixed"]).evaluate()
    e = engine(st, g, pr)
    assert e.prior_count() == len(pr["nodes"]) and e.prior_kernel_geometry() == (Q.PRIORS_PER_WORKGROUP, Q.NODES_PER_WORKGROUP)
    cp, r, J = e.evaluate_priors()
    rw = P.whiten(W, ro[m:])
    Jw = W @ Jjo[m:]
    worst = 0.0
    for name, got, want, x, base in (("r", r, rw, ro[m:], 1e-12), ("J", J, Jw, Jjo[m:], 1e-11)):
        err, bound = np.abs(got - want), P.whiten_bound(W, x, base)
        worst = max(worst, (err / bound).max())
        print(f"  {gname} {kind} {name}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3e}")
    assert worst <= 1.0
    cpw = float(0.5 * np.sum(rw.astype(np.longdouble) ** 2))
    cew = float(0.5 * np.sum(ro[:m].astype(np.longdouble) ** 2))
    cost, re, Ji, Jj = e.evaluate()
    print(f"  {gname} {kind}: priors' cost {cp:.17g} reference {cpw:.17g}; sum {cost:.17g} reference {cew + cpw:.17g}")
    assert abs(cp - cpw) <= 1e-12 * cpw and abs(cost - (cew + cpw)) <= 1e-12 * (cew + cpw)
    # r, Ji, Jj of evaluate() stay per edge: the engine without priors, bit for bit
    plain = engine(st, g).evaluate()
    assert re.shape == (m, 6) and same_bits((re, Ji, Jj), plain[1:]) and cost > plain[0]
    # a constant node's prior: J' == 0, and its cost is counted
    fx = g["node_fixed"][pr["nodes"]] != 0
    if gname in ("n60", "n150"):
        assert fx.any()
    assert np.all(J[fx] == 0.0) and np.all(np.abs(J[~fx]).max(axis=(1, 2)) > 0.0)
    assert np.all(np.abs(r[fx]).max(axis=1) > 0.0) if fx.any() else True
    assert same_bits(e.evaluate_priors(), (cp, r, J))                # a second run: the same bits
    e.close()


# ------------------------------------------------------------------------------- 2. LM steps, every solver path
def judge(prob, ref, o, x_dev, trace, label):
    """tests/test_gpu_pg_information.py's judge"""
    eps_eff = max(L.EPS, L.PCG_TOL)
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["pg"] * kap * eps_eff <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = L.compare(prob, ref, "pg", o, x_dev, trace, eps_eff=eps_eff)
    print(f"LMSTEP pg-prior {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    assert not fails, f"{label}: " + "; ".join(fails)


def run_steps(st, e, o, route):
    pc = e.pcg_options(forcing_eta0=0.0, relative_tolerance=L.PCG_TOL, **L.PG_PCG[route])
    summ, tr, _ = e.solve(st.default_options(**dict(o, max_num_iterations=K)), pcg=pc)
    assert summ.num_iterations == K and len(tr) == K + 1, summ.as_dict()
    ps = e.pcg_summary()
    print(f"  {route}: PCG iterations {ps.iterations_total}, most in a solve {ps.max_iterations_in_a_solve}, hit_cap {ps.hit_cap}, "
          f"one-kernel solves {ps.one_kernel_solves}, coarse dim {ps.coarse_dim}")
    assert ps.max_iterations_in_a_solve < pc.max_iterations and (ps.coarse_dim > 0) == route.endswith("cg0")
    assert (ps.one_kernel_solves == K) == (route == "k1_cg0"), (route, ps.one_kernel_solves)
    return tr


@pytest.mark.parametrize("route", list(L.PG_PCG))
@pytest.mark.parametrize("gname,kind", CASES)
def test_exact_steps_follow_the_augmented_reference(st, gname, kind, route):
    g, pr = Q.graph(gname), Q.priors(gname, kind)
    o = L.lm_options(**Q.LM_OPTIONS)
    ref = Q.drop_virtual(Q.reference(gname, kind, K))
    e = engine(st, g, pr)
    tr = run_steps(st, e, o, route)
    judge(L.pg_problem(g), ref, o, e.get_poses().reshape(-1), tr, f"{gname} {kind} {route}")
    e.close()


# ------------------------------------------------------------------------------- 3. production solve
@pytest.mark.parametrize("gname,kind", [("n60", "few"), ("n40_pad", "many"), ("n150", "few"), ("n60_free", "few")])
def test_production_solves_reach_the_exact_step_cost(st, gname, kind):
    g, pr = Q.graph(gname), Q.priors(gname, kind)
    tight = dict(function_tolerance=1e-12, parameter_tolerance=1e-11)
    runs = {"default": {}, "exact": dict(forcing_eta0=0.0), "sync": dict(coarse_async=0), "launches": dict(one_kernel_solve=0),
            "launches sync": dict(one_kernel_solve=0, coarse_async=0)}
    cost = {}
    for name, kw in runs.items():
        e = engine(st, g, pr)
        s, _, _ = e.solve(pcg=e.pcg_options(**kw), **tight)
        ps = e.pcg_summary()
        cost[name] = s.final_cost
        print(f"  {gname} {kind} {name}: {s.initial_cost:.6e} -> {s.final_cost:.12e} in {s.num_iterations} iterations, one-kernel solves "
              f"{ps.one_kernel_solves}, hit_cap {ps.hit_cap}")
        assert s.termination_type == 0 and ps.hit_cap == 0 and s.final_cost < 0.5 * s.initial_cost
        assert ps.one_kernel_solves == 0 or not name.startswith("launches")
        e.close()
    for name in runs:
        gap = abs(cost[name] - cost["exact"]) / cost["exact"]
        print(f"  {gname} {kind} {name}: relative gap to the exact-step run {gap:.2e}")
        assert gap <= 1e-6


# ------------------------------------------------------------------------------- 4. a graph without a constant node
def covariance_reference(O, g, pr):
    a = Q.augment(g, pr)
    J = P.whitened_jacobian(O, a, Q.augmented_weights(g, pr))
    C, lam_min, kappa = R.dense_covariance((J.T @ J).tocsc(), a["node_fixed"])
    return Q.drop_virtual_covariance(C), lam_min, kappa


def test_gauge_free_graph_converges_to_the_augmented_reference(st):
    g, pr = Q.graph("n60_free"), Q.priors("n60_free", "few")
    o = L.lm_options(**Q.LM_OPTIONS)
    ref = L.lm_reference(Q.problem(g, pr), o, o["max_num_iterations"])
    assert abs(ref[-1]["cost_change"]) <= 1e-12 * ref[-1]["cost"]
    e = engine(st, g, pr)
    s, _, _ = e.solve(st.default_options(**dict(o, function_tolerance=1e-12, parameter_tolerance=1e-11)))
    gap = abs(s.final_cost - ref[-1]["cost"]) / ref[-1]["cost"]
    err = L.point_error(L.pg_problem(g), e.get_poses().reshape(-1), ref[-1]["x"][:-7])
    # a point whose cost is within gap * cost of the minimum's lies within sqrt(2 gap cost / lambda_min(J^T J)) of it (the quadratic
    # model at the minimum; twice that for the model's own error at this distance)
    lam_min = np.linalg.svd(Q.jacobian(g, pr, x=ref[-1]["x"]), compute_uv=False)[-1] ** 2
    bound = 2.0 * np.sqrt(2.0 * 1e-6 * ref[-1]["cost"] / lam_min)
    print(f"  n60_free few: device {s.final_cost:.12e} reference {ref[-1]['cost']:.12e} gap {gap:.2e}, |x - x_ref| {err:.2e} bound {bound:.2e}")
    assert s.termination_type == 0 and gap <= 1e-6 and err <= bound
    e.close()


@pytest.mark.parametrize("kind", ["few", "three_pos"])
def test_priors_make_the_covariance_of_a_gauge_free_graph(st, O, kind):
    g, pr = Q.graph("n60_free"), Q.priors("n60_free", kind)
    e = engine(st, g)
    pairs = [(3, 3), (17, 17), (3, 17), (17, 3), (30, 30), (59, 59), (0, 40), (21, 21)]
    with pytest.raises(st.StbaError) as err:
        e.covariance(pairs)
    assert err.value.code == STBA_ERR_NOT_POSITIVE_DEFINITE and "contains no constant node" in last_error(st)
    e.set_priors(**Q.engine_kwargs(pr))
    Cs, lam_min, kappa = covariance_reference(O, g, pr)
    C, summ = e.covariance(pairs, relative_tolerance=1e-12)
    rho = summ["max_relative_residual"]
    bound = R.block_bound(rho, kappa, lam_min)
    print(f"  n60_free {kind}: lambda_min {lam_min:.3e} kappa {kappa:.3e} rho {rho:.3e} bound {bound:.3e} iterations {summ['iterations_total']}")
    assert rho <= 1e-12
    for k, (a, b) in enumerate(pairs):
        ref = R.block(Cs, a, b)
        d = np.linalg.norm(C[k] - ref)
        print(f"    C[{a},{b}] |err|_F {d:.3e} |C*|_F {np.linalg.norm(ref):.3e} err / bound {d / bound:.3e}")
        assert d <= bound, (a, b, d, bound)
    cols, _ = e.covariance_columns(17, relative_tolerance=1e-12)
    assert np.linalg.norm(cols[6 * 3:6 * 3 + 6] - R.block(Cs, 3, 17)) <= bound
    e.set_priors(None)
    with pytest.raises(st.StbaError):
        e.covariance(pairs)
    e.close()


def test_a_single_position_prior_is_refused_by_the_solve_not_the_gauge_check(st):
    g, pr = Q.graph("chain12"), Q.priors("chain12", "single_pos")
    e = engine(st, g, pr)
    with pytest.raises(st.StbaError) as err:
        e.covariance([(5, 5), (0, 0)], max_iterations=300)
    print("  refused:", last_error(st))
    assert err.value.code == STBA_ERR_NOT_POSITIVE_DEFINITE and "contains no constant node" not in last_error(st)
    e.close()


# ------------------------------------------------------------------------------- 5. with edge weights and edge losses
def test_priors_with_dense_edge_information(st):
    gname = "n40_pad"
    g, pr = Q.graph(gname), Q.priors(gname, "gps")
    om, We = P.weights(gname, "dense")
    o = L.lm_options(**Q.LM_OPTIONS)
    prob = Q.problem(g, pr, We)
    ref = Q.drop_virtual(L.lm_reference(prob, o, K))
    for route in ("k1_cg0", "k0_cg0"):
        e = engine(st, g, pr, information=om)
        tr = run_steps(st, e, o, route)
        judge(L.pg_problem(g), ref, o, e.get_poses().reshape(-1), tr, f"{gname} gps + dense information {route}")
        e.close()


def test_priors_with_a_huber_loss_on_the_edges(st):
    """the prior edges of the reference carry the trivial loss: priors are not robustified"""
    gname = "n60"
    g, pr = Q.graph(gname), Q.priors(gname, "few")
    table, _ = PL.loss_set(gname, "huber")
    k = len(pr["nodes"])
    aug = dict(kind=np.concatenate([table["kind"], np.zeros(k, np.int32)]), a=np.concatenate([table["a"], np.ones(k)]),
               b=np.concatenate([table["b"], np.ones(k)]), scale=np.concatenate([table["scale"], np.ones(k)]))
    o = L.lm_options(**Q.LM_OPTIONS)
    prob = PL.RobustPGProblem(Q.augment(g, pr), Q.augmented_weights(g, pr), aug)
    ref = Q.drop_virtual(PL.lm_reference(prob, o, K))
    for route in ("k1_cg0", "k0_cg0"):
        e = engine(st, g, pr, loss=dict(table))
        c0 = e.evaluate()[0]
        assert abs(c0 - ref[0]["start"]["cost"]) <= 1e-12 * c0
        tr = run_steps(st, e, o, route)
        judge(L.pg_problem(g), ref, o, e.get_poses().reshape(-1), tr, f"{gname} few + huber {route}")
        e.close()


# ------------------------------------------------------------------------------- 6. identity and clearing
@pytest.mark.parametrize("pcg", [dict(), dict(one_kernel_solve=0)])
def test_cleared_priors_leave_the_engine_that_never_had_any(st, pcg):
    g, pr = Q.graph("n40_pad"), Q.priors("n40_pad", "many")
    fresh, e = engine(st, g), engine(st, g, pr)
    assert e.prior_count() == len(pr["nodes"]) and not same_bits(e.evaluate()[:1], fresh.evaluate()[:1])
    e.solve(max_num_iterations=2)
    e.close()
    e = engine(st, g, pr)
    e.set_priors(None)
    assert e.prior_count() == 0 and same_bits(e.evaluate(), fresh.evaluate())
    e.set_priors(**Q.engine_kwargs(pr)); e.set_priors([], None)
    sa, ta, na = e.solve(max_num_iterations=6, pcg=e.pcg_options(**pcg))
    sb, tb, nb = fresh.solve(max_num_iterations=6, pcg=fresh.pcg_options(**pcg))
    assert np.array_equal(ta, tb) and np.array_equal(e.get_poses(), fresh.get_poses()) and na == nb
    pa, pb = e.pcg_summary(), fresh.pcg_summary()
    assert (pa.iterations_total, pa.solves, pa.one_kernel_solves, pa.coarse_refreshes) == (pb.iterations_total, pb.solves, pb.one_kernel_solves, pb.coarse_refreshes)
    assert e.evaluate_priors()[0] == 0.0
    e.close(); fresh.close()


@pytest.mark.parametrize("pcg", [dict(), dict(one_kernel_solve=0), dict(coarse_async=0)])
def test_two_solves_with_priors_give_the_same_bits(st, pcg):
    g, pr = Q.graph("n40_pad"), Q.priors("n40_pad", "many")
    out = []
    for _ in range(2):
        e = engine(st, g, pr)
        s, tr, n = e.solve(max_num_iterations=6, pcg=e.pcg_options(**pcg))
        out.append((tr, e.get_poses(), n))
        e.close()
    assert same_bits(out[0], out[1])


def test_caller_order_of_priors_does_not_move_a_bit(st):
    """priors are held sorted by node, then by the caller's index: two nodes' priors in swapped order give the same sums"""
    g, pr = Q.graph("n60"), Q.priors("n60", "few")
    idx = np.array([2, 0, 1, 4, 3, 5])              # nodes (17, 3, 3, 59, 30, 0): the two priors of node 3 keep their order
    sw = {k: (v[idx] if v is not None else None) for k, v in pr.items()}
    a, b = engine(st, g, pr), engine(st, g, sw)
    ca, ra, Ja = a.evaluate_priors()
    cb, rb, Jb = b.evaluate_priors()
    assert ca == cb and np.array_equal(ra[idx], rb) and np.array_equal(Ja[idx], Jb)
    for pcg in (dict(), dict(one_kernel_solve=0)):
        sa, ta, _ = a.solve(max_num_iterations=4, pcg=a.pcg_options(**pcg))
        sb, tb, _ = b.solve(max_num_iterations=4, pcg=b.pcg_options(**pcg))
        assert np.array_equal(ta, tb) and np.array_equal(a.get_poses(), b.get_poses())
    a.close(); b.close()


# ------------------------------------------------------------------------------- 7. refusals and lifecycle
def test_bad_priors_are_refused_with_the_prior_named_and_the_priors_kept(st):
    g, pr = Q.graph("n60"), Q.priors("n60", "few")
    e = engine(st, g, pr)
    before = e.evaluate_priors()
    n = len(pr["nodes"])
    eye = np.tile(np.eye(6), (n, 1, 1))

    def refused(code, k, **kw):
        args = dict(Q.engine_kwargs(pr), **kw)
        with pytest.raises(st.StbaError) as err:
            e.set_priors(**args)
        msg = last_error(st)
        print("  refused:", msg)
        assert err.value.code == code and f"prior {k}:" in msg, msg
        assert e.prior_count() == n and same_bits(e.evaluate_priors(), before)

    nodes = pr["nodes"].copy(); nodes[2] = 60; nodes[4] = -1
    refused(STBA_ERR_INVALID_ARGUMENT, 2, nodes=nodes)
    poses = pr["poses"].copy(); poses[3, 5] = np.nan; poses[5, 0] = np.inf
    refused(STBA_ERR_INVALID_ARGUMENT, 3, poses=poses)
    poses = pr["poses"].copy(); poses[1, :4] = 0.0
    refused(STBA_ERR_INVALID_ARGUMENT, 1, poses=poses)
    w = pr["W"].copy(); w[4, 2, 2] = np.nan
    refused(STBA_ERR_INVALID_ARGUMENT, 4, sqrt_information=w)
    om = eye.copy(); om[2] = np.diag([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]); om[5] = 0.0
    refused(STBA_ERR_NOT_POSITIVE_DEFINITE, 2, sqrt_information=None, information=om)
    # both weight arrays: the Python layer refuses first, the C ABI by itself too
    with pytest.raises(ValueError, match="not both"):
        e.set_priors(pr["nodes"], pr["poses"], information=eye, sqrt_information=eye)
    C = importlib.import_module("ctypes")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nd, ps = np.ascontiguousarray(pr["nodes"], np.int32), np.ascontiguousarray(pr["poses"])
    assert st.lib().stba_pg_set_priors(e._h, n, p(nd), p(ps), p(eye), p(eye)) == STBA_ERR_INVALID_ARGUMENT
    assert "not both" in last_error(st) and same_bits(e.evaluate_priors(), before)
    e.close()


def test_a_hook_and_priors_are_refused_in_both_orders(st):
    g, pr = Q.graph("n60"), Q.priors("n60", "few")
    hook = lambda user, buf, count, stream: 0
    e = engine(st, g, pr)
    before = e.evaluate_priors()
    with pytest.raises(st.StbaError) as err:
        e.set_allreduce(hook, 0, 1)
    assert err.value.code == STBA_ERR_INVALID_ARGUMENT and "priors" in last_error(st)
    assert same_bits(e.evaluate_priors(), before)
    s, _, _ = e.solve(max_num_iterations=2)             # still a one-rank engine with its priors
    assert s.num_iterations == 2
    e.set_priors(None)
    e.set_allreduce(hook, 0, 1)
    with pytest.raises(st.StbaError) as err:
        e.set_priors(**Q.engine_kwargs(pr))
    assert err.value.code == STBA_ERR_INVALID_ARGUMENT and "one rank" in last_error(st) and e.prior_count() == 0
    e.set_priors(None)                                    # a call that clears is never refused
    e.close()


def test_priors_are_released_with_the_engine(st):
    start = st.live_device_buffers()
    g, pr = Q.graph("n40_pad"), Q.priors("n40_pad", "many")
    e = engine(st, g, pr)
    assert st.live_device_buffers() > start
    e.solve(max_num_iterations=2)
    e.set_priors(**Q.engine_kwargs(Q.priors("n40_pad", "gps")))
    e.covariance([(1, 1)])
    e.close()
    assert st.live_device_buffers() == start
