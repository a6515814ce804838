"""CPU leg of the pose graph's robust losses: the inputs of the GPU tests (tests/pg_loss_ref.py) have the properties those tests lean
on, the numpy reference agrees with a 50-digit one and with the loss classes of include/stba/ceres.h, and the Python layer builds and
slices the per-edge table without a device."""
import importlib
import subprocess

import numpy as np
import pytest

import lm_step_ref as L
import pg_information_ref as P
import pg_loss_ref as R
from test_pg_loss_shim import build_exe

SOLVE_CASES = [(g, s) for g in P.GRAPHS for s in R.SOLVE_SETS]
K = 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory)


# ------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("gname", P.GRAPHS)
def test_loss_sets_cover_every_branch_at_the_start(gname):
    g = P.graph(gname)
    n0 = R.n_odometry(g)
    s = R.s_at_start(gname, "huber")
    print(f"{gname}: odometry s max {s[:n0].max():.1e}; loops s min {s[n0:].min():.3g} median {np.median(s[n0:]):.3g} max {s[n0:].max():.3g}")
    # (poses0 is the odometry chained up: the odometry residuals are rounding, s < 1e-28 and exactly 0 for some on some
    # implementations; the s == 0 branch proper is tests/pg_loss_ref.zero_graph's)
    assert s[:n0].max() < 1e-28 and np.all(s[n0:] > 1e-3)
    for name, a in (("huber", R.HUBER_A), ("tukey", R.TUKEY_A)):
        table, _ = R.loss_set(gname, name)
        assert np.all(table["kind"][:n0] == 0) and np.all(table["kind"][n0:] == R.KINDS.index(name)) and np.all(table["a"][n0:] == a)
        above = float(np.mean(s[n0:] > a * a))
        print(f"  {name}({a}): {above:.2f} of the loops beyond a^2")
        assert 0.2 <= above <= 0.8
    table, _ = R.loss_set(gname, "tolerant")
    x = (s[n0:] - table["a"][n0:]) / table["b"][n0:]
    print(f"  tolerant{R.TOLERANT_AB}: {np.mean(x > R.TOLERANT_LINEAR):.2f} of the loops on the linear branch")
    assert np.sum(x > R.TOLERANT_LINEAR) >= 5 and np.sum(x <= R.TOLERANT_LINEAR) >= 5
    rh, _, _, k = R.factors(table, s)
    assert np.sum(k[n0:] != 0) >= 5 and np.all(rh[2] >= 0)              # the second corrector branch runs (rho'' > 0)
    table, wname = R.loss_set(gname, "cauchy_w")
    assert wname == "dense" and np.all(table["kind"][n0:] == 3)
    sw = R.s_at_start(gname, "cauchy_w")[n0:]
    rw = R.rho(3, R.CAUCHY_W_A, 1.0, 1.0, sw)[1]
    print(f"  cauchy_w: whitened s median {np.median(sw):.3g}, rho' from {rw.min():.3g} to {rw.max():.3g}")
    assert rw.min() < 0.5 < rw.max()
    table, _ = R.loss_set(gname, "mixed")
    assert set(table["kind"].tolist()) == set(range(7)) and np.any(table["scale"] != 1.0)
    assert np.any(R.untouched(table)) and np.any((table["kind"] == 0) & (table["scale"] != 1.0))
    assert set(table["kind"][256:].tolist()) == set(range(7)) or gname == "n60"            # the second workgroup sees every kind too


@pytest.mark.parametrize("gname", P.GRAPHS)
def test_corrected_jacobian_is_the_gradient_of_the_robust_cost(gname):
    """the gradient of 1/2 rho(|r~|^2) is rho' J~^T r~: the corrected pair gives J'^T r' = rho' J~^T r~ (both corrector branches), and
    rho', rho'' are the derivatives of rho, rho' -- central differences in s, away from the kinks of Huber, Tukey and Tolerant.
    (Not differences in the poses: the build's Jacobian truncates Jr^-1 after ad^2, lm_step_ref.PGProblem, and is no exact derivative.)"""
    for name in R.LOSS_SETS:
        prob = R.problem(gname, name)
        t = prob.table
        rw, Jw, cols = P.WeightedPGProblem.lin(prob, prob.x0)
        rc, Jc, _ = prob.lin(prob.x0)
        s = np.sum(rw * rw, 1)
        rh = R.rho(t["kind"], t["a"], t["b"], t["scale"], s)
        want = rh[1][:, None] * np.einsum("eab,ea->eb", Jw, rw)
        got = np.einsum("eab,ea->eb", Jc, rc)
        err = np.abs(got - want).max() / np.abs(want).max()
        h = 1e-6 * np.maximum(s, 1e-3)
        up, dn = (R.rho(t["kind"], t["a"], t["b"], t["scale"], s + sg * h) for sg in (1, -1))
        kink = np.where(t["kind"] == 5, t["a"] + R.TOLERANT_LINEAR * t["b"], t["a"] ** 2)
        smooth = (np.abs(s - kink) > 2 * h) & (s > 2 * h)
        d1 = np.abs((up[0] - dn[0]) / (2 * h) - rh[1])[smooth].max()
        d2 = (np.abs((up[1] - dn[1]) / (2 * h) - rh[2]) / np.maximum(1.0, np.abs(rh[2])))[smooth].max()
        print(f"{gname} {name}: |J'^T r' - rho' J^T r| / max = {err:.2e}; central differences: rho' {d1:.2e}, rho'' {d2:.2e} ({int(smooth.sum())} edges)")
        assert err <= 64 * L.EPS and d1 <= 1e-6 and d2 <= 1e-6 and smooth.sum() >= 0.5 * np.sum(s > 1e-3)


def test_numpy_losses_match_the_50_digit_ones():
    """the measured figure behind pg_loss_ref.RHO_EPS (and so behind the c of the GPU evaluate bound): over the s of every loss set at
    poses0 on both graphs, the worst relative error of rho' and rho'' -- what the corrector's factors are made of -- per kind in units
    of eps.  rho itself only enters the cost; SoftLOne, Cauchy, Tolerant and Tukey lose it to cancellation where s is rounding noise
    (an odometry edge of the mixed set, s = 1e-30: the formula gives 0), so it is measured where it matters: the summed cost."""
    worst = {k: 0.0 for k in R.KINDS}
    worst_cost = 0.0
    for gname in P.GRAPHS:
        for name in R.LOSS_SETS:
            table, _ = R.loss_set(gname, name)
            s = R.s_at_start(gname, name)
            got = R.rho(table["kind"], table["a"], table["b"], table["scale"], s)
            total = 0
            for e in range(len(s)):
                want = R.rho_mp(int(table["kind"][e]), table["a"][e], table["b"][e], table["scale"][e], s[e])
                total = total + want[0]
                for q in (1, 2):
                    if float(want[q]) == 0.0:
                        assert got[q][e] == 0.0
                        continue
                    rel = abs(float((got[q][e] - want[q]) / want[q])) / L.EPS
                    kn = R.KINDS[int(table["kind"][e])]
                    worst[kn] = max(worst[kn], rel)
            worst_cost = max(worst_cost, abs(float((float(np.sum(got[0].astype(L.LD))) - total) / total)))
    print("worst |numpy - 50 digits| / (eps |value|) of rho', rho'' per kind: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    print(f"worst relative error of sum rho: {worst_cost:.2e}")
    assert worst_cost <= 1e-14
    for k, v in worst.items():
        assert v <= R.RHO_EPS[k], (k, v)


@pytest.mark.parametrize("gname,name", SOLVE_CASES)
def test_solve_cases_are_accuracy_cases(gname, name):
    o = L.lm_options(**P.LM_OPTIONS)
    ref = R.reference(gname, name, K)
    kap = max(it["kappa"] for it in ref)
    print(f"{gname} {name}: kappa {kap:.2e}, cost {ref[0]['start']['cost']:.6e} -> {ref[-1]['cost']:.6e}, "
          f"rho {[round(it['rho'], 3) for it in ref]}, accepted {[it['accepted'] for it in ref]}")
    assert L.C_PATH["pg"] * kap * max(L.EPS, L.PCG_TOL) <= 1e-6
    assert L.rho_margin_ok(ref, o)
    assert ref[0]["accepted"] and ref[-1]["cost"] < ref[0]["start"]["cost"]
    # the start cost is 1/2 sum rho, not 1/2 |r'|^2
    prob = R.problem(gname, name)
    rc = prob.lin(prob.x0, False)[0]
    assert abs(0.5 * np.sum(rc * rc) - ref[0]["start"]["cost"]) > 1e-3 * ref[0]["start"]["cost"]


def test_zero_graph_has_s_exactly_zero_and_takes_the_first_branch():
    g, table = R.zero_graph()
    m = len(g["edge_i"])
    prob = R.RobustPGProblem(g, np.tile(np.eye(6), (m, 1, 1)), table)
    rw, Jw, _ = P.WeightedPGProblem.lin(prob, prob.x0)
    assert np.all(rw == 0.0) and set(table["kind"].tolist()) == set(range(7))
    rh, sq, rs, k = R.factors(table, np.zeros(m))
    assert np.all(k == 0.0) and np.array_equal(rs, sq) and np.any(rh[2] > 0) and np.any(sq != 1.0)
    rc, Jc, _ = prob.lin(prob.x0)
    assert np.all(rc == 0.0) and np.array_equal(Jc, np.where(R.untouched(table)[:, None, None], Jw, sq[:, None, None] * Jw))


def test_trivial_table_is_the_lossless_reference():
    g = P.graph("n60")
    m = len(g["edge_i"])
    table = dict(kind=np.zeros(m, np.int32), a=np.ones(m), b=np.ones(m), scale=np.ones(m))
    prob, base = R.RobustPGProblem(g, np.tile(np.eye(6), (m, 1, 1)), table), L.pg_problem(g)
    a, b = prob.lin(prob.x0), base.lin(base.x0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and prob.cost(prob.x0) == base.cost(base.x0)
    o = L.lm_options(**P.LM_OPTIONS)
    ra, rb = R.lm_reference(prob, o, 2), L.lm_reference(base, o, 2)
    for x, y in zip(ra, rb):
        assert np.array_equal(x["x"], y["x"]) and x["cost"] == y["cost"] and x["rho"] == y["rho"] and x["radius"] == y["radius"]


def test_cauchy_resists_outliers_where_l2_does_not():
    """six loop closures replaced by random poses: the L2 solve is dragged away, the Cauchy solve ends next to the solution of the
    graph WITHOUT the outliers and nearer poses_true than the L2 solve.  (Distances are lm_step_ref.point_error over all 60 poses; the
    clean solution is itself 6.07 from poses_true, the noise of the graph's own measurements.)"""
    g, bad = R.outlier_graph()
    x_l2, x_rob, cost_rob, table = R.outlier_references()
    assert len(bad) == 6 and np.all(bad >= R.n_odometry(g)) and np.all(table["kind"][bad] == 3)
    prob = L.pg_problem(g)
    o = L.lm_options(**P.LM_OPTIONS)
    x_clean = L.lm_reference(L.pg_problem(P.graph("n60")), o, o["max_num_iterations"])[-1]["x"]
    truth = np.asarray(g["poses_true"], float).reshape(-1)
    d_l2, d_rob, apart = L.point_error(prob, x_l2, truth), L.point_error(prob, x_rob, truth), L.point_error(prob, x_l2, x_rob)
    c_l2, c_rob = L.point_error(prob, x_l2, x_clean), L.point_error(prob, x_rob, x_clean)
    print(f"outliers on edges {bad.tolist()}: |L2 - truth| {d_l2:.3f}, |Cauchy - truth| {d_rob:.3f}, |L2 - Cauchy| {apart:.3f}; "
          f"|L2 - clean| {c_l2:.3f}, |Cauchy - clean| {c_rob:.3f}; robust cost {cost_rob:.6f}")
    assert apart > 1.0 and d_rob < d_l2 - 1.0 and c_rob < 0.25 * c_l2


# ------------------------------------------------------------------------------- ceres.h's classes
POINTS = {  # kind: (a, b, [s on both sides of every branch])
    0: (1.0, 1.0, [0.0, 0.3, 7.0]),
    1: (0.5, 1.0, [0.0, 0.1, 0.25, 0.2500001, 0.9, 40.0]),
    2: (0.7, 1.0, [0.0, 0.2, 3.0, 500.0]),
    3: (0.7, 1.0, [0.0, 0.2, 3.0, 500.0]),
    4: (0.7, 1.0, [0.0, 0.2, 3.0, 500.0]),
    5: (0.3, 0.02, [0.0, 0.1, 0.3, 0.9, 1.0339, 1.0341, 2.0, 30.0]),
    6: (0.8, 1.0, [0.0, 0.3, 0.64, 0.6400001, 2.0]),
}


@pytest.mark.parametrize("scale", [1.0, 2.5])
@pytest.mark.parametrize("kind", list(POINTS) + [-1])
def test_ceres_loss_classes_evaluate_the_reference_formulas(exe, kind, scale):
    """Evaluate of every class (scale 2.5: through ScaledLoss; kind -1: ScaledLoss around nullptr) against the numpy reference: the
    same formulas in the same order, so 4 eps relative covers the two libms"""
    a, b, pts = POINTS[max(kind, 0)]
    p = subprocess.run([exe, "eval", str(kind), repr(a), repr(b), repr(scale)] + [repr(s) for s in pts], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    rows = np.array([[float(v) for v in ln.split()[1:]] for ln in p.stdout.splitlines() if ln.startswith("E ")])
    assert len(rows) == len(pts) and np.array_equal(rows[:, 0], pts)
    want = R.rho(np.full(len(pts), max(kind, 0)), a, b, scale, np.array(pts)).T
    err = np.abs(rows[:, 1:] - want)
    print(f"kind {kind} scale {scale}: max |difference| / |value| = {np.max(err / np.maximum(np.abs(want), 1e-300)):.2e}")
    assert np.all(err <= 4 * L.EPS * np.abs(want))
    if kind == 5:
        assert want[3, 2] > 0 and want[4, 2] > 0 and np.all(want[5:, 2] == 0) and np.all(want[5:, 1] == scale)      # both sides of 36.7
    if kind in (1, 6):
        assert want[2, 1] != want[3, 1]                                                                               # both sides of a^2


# ------------------------------------------------------------------------------- the Python layer, no device
def test_loss_table_from_one_spec_or_per_edge_arrays():
    st = importlib.import_module("slam-tricks_amd")
    k, a, b, s = st.pg_loss_table(5, "huber", 0.5)
    assert k.dtype == np.int32 and k.tolist() == [1] * 5 and a.tolist() == [0.5] * 5 and b.tolist() == [1.0] * 5 and s.tolist() == [1.0] * 5
    k, a, b, s = st.pg_loss_table(3, ["Tolerant", None, "tukey"], [0.3, 1.0, 2.0], 0.02, [1.0, 1.0, 3.0])
    assert k.tolist() == [5, 0, 6] and a.tolist() == [0.3, 1.0, 2.0] and b.tolist() == [0.02] * 3 and s.tolist() == [1.0, 1.0, 3.0]
    assert st.pg_loss_table(2, np.array([3, 4]), 1.0)[0].tolist() == [3, 4]
    assert [st.LOSS_KINDS[n] for n in R.KINDS] == list(range(7)) and st.LOSS_KINDS[None] == 0
    with pytest.raises(ValueError, match="unknown loss kind"):
        st.pg_loss_table(3, "hubert", 1.0)
    with pytest.raises(ValueError, match="length 3"):
        st.pg_loss_table(3, ["huber", "huber"], 1.0)
    with pytest.raises(ValueError, match="length 3"):
        st.pg_loss_table(3, "huber", [1.0, 2.0])
    # the engine checks its loss= before it needs a device
    g = P.graph("n60")
    with pytest.raises(ValueError, match="unknown loss kind"):
        st.PGEngine(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"], loss=("l2", 1.0))
    for name in ("stba_pg_set_loss", "stba_pg_has_loss"):
        assert name in st.EXPORTS and hasattr(st.lib(), name)
    assert st.lib().stba_pg_set_loss(None, None, None, None, None) == -1 and st.lib().stba_pg_has_loss(None, None) == -1


def test_make_pg_shard_slices_the_loss_table_with_its_edges():
    sharding = importlib.import_module("slam-tricks_amd.sharding")
    g = P.graph("n40_pad")
    table, _ = R.loss_set("n40_pad", "mixed")
    seen = 0
    for rank in range(3):
        sh = sharding.make_pg_shard(dict(g, loss=dict(table)), rank, 3)
        lo, hi = sh["lo"], sh["hi"]
        for key in ("kind", "a", "b", "scale"):
            assert np.array_equal(sh["loss"][key], table[key][lo:hi]) and len(sh["loss"][key]) == len(sh["edge_i"])
        one = sharding.make_pg_shard(dict(g, loss=dict(kind="cauchy", a=0.5)), rank, 3)
        assert one["loss"] == dict(kind="cauchy", a=0.5)
        seen += hi - lo
    assert seen == len(g["edge_i"]) and "loss" not in sharding.make_pg_shard(g, 0, 2)
