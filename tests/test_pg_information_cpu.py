"""CPU leg of the pose-graph information matrices: the inputs of the GPU tests (tests/pg_information_ref.py) have the properties the
GPU tests lean on, the whitened FP64 reference step agrees with a 50-digit redo, and the Python layer checks its arguments before it
needs a device."""
import importlib

import mpmath as mp
import numpy as np
import pytest

import lm_step_ref as L
import mp_ref as M
import pg_information_ref as P

CASES = [(g, w) for g in P.GRAPHS for w in P.WEIGHTS]


def test_graphs_have_the_shapes_the_gpu_tests_need():
    g60, g40 = P.graph("n60"), P.graph("n40_pad")
    assert len(g60["poses0"]) == 60 and len(g60["edge_i"]) <= 256
    assert len(g40["poses0"]) == 40 and 256 < len(g40["edge_i"]) == P.N_PAD_EDGES and P.N_PAD_EDGES > 300     # (edge 300 exists)
    for g in (g60, g40):
        fx = np.flatnonzero(g["node_fixed"])
        assert len(fx) == 2
        assert (g["edge_i"] == fx[0]).any() and (g["edge_j"] == fx[1]).any()      # one constant node on the i side, one on the j side
        assert np.all(g["edge_i"] != g["edge_j"])


@pytest.mark.parametrize("gname", P.GRAPHS)
def test_weight_sets_are_what_the_docstring_says(gname):
    om, W = P.weights(gname, "diag")
    d = np.diagonal(om, axis1=1, axis2=2)
    assert np.all(om == om * np.eye(6)) and np.allclose(d[:, 3] / d[:, 0], 100.0) and np.array_equal(W @ W, om)
    om, W = P.weights(gname, "dense")
    lam = np.linalg.eigvalsh(om)
    assert np.all(lam[:, 0] >= 1.0 * (1 - 1e-9)) and np.all(lam[:, -1] <= 1e4 * (1 + 1e-9))
    assert max(np.linalg.cond(w) for w in W) <= 100.0 * (1 + 1e-9)
    assert np.all(np.tril(W, -1) == 0) and np.all(np.abs(np.triu(om, 1)).max(axis=(1, 2)) > 1.0)          # W = L^T upper; Omega dense
    assert np.abs(W.transpose(0, 2, 1) @ W - om).max() <= 16 * L.EPS * 1e4
    # the 50-digit factor against LAPACK's: the same matrix to LAPACK's own error, far from bitwise
    Wn = np.linalg.cholesky(om).transpose(0, 2, 1)
    print(f"{gname}: |W_50 - W_lapack| / |W| max {np.abs(W - Wn).max() / np.abs(W).max():.2e}")
    assert np.abs(W - Wn).max() <= 1e4 * L.EPS * np.abs(W).max()
    om, W = P.weights(gname, "sqrt")
    assert om is None and max(np.linalg.cond(w) for w in W) <= 100.0 * (1 + 1e-9)
    assert np.all(np.abs(np.tril(W, -1)).max(axis=(1, 2)) > 1e-3) and np.all(np.abs(W - W.transpose(0, 2, 1)).max(axis=(1, 2)) > 1e-3)


@pytest.mark.parametrize("gname,kind", CASES)
def test_reference_lm_converges_within_the_iteration_cap(gname, kind):
    """numpy alone: the reference LM on the whitened problem, Ceres' cap of 50 iterations"""
    o = L.lm_options(**P.LM_OPTIONS)
    ref = L.lm_reference(P.problem(gname, kind), o, o["max_num_iterations"])
    start, last = ref[0]["start"], ref[-1]
    print(f"{gname} {kind}: cost {start['cost']:.6e} -> {last['cost']:.6e}, |g|max {start['gmax']:.2e} -> {last['gmax']:.2e}, "
          f"{sum(it['accepted'] for it in ref)} accepted")
    assert last["cost"] < 0.5 * start["cost"]
    assert last["gmax"] <= 1e-7 * start["gmax"]
    assert abs(last["cost_change"]) <= 1e-12 * last["cost"]
    # the first three iterations are what the GPU step test compares: an accuracy case, decisions far from the threshold
    ref3 = P.reference(gname, kind, 3)
    kap = max(it["kappa"] for it in ref3)
    assert L.C_PATH["pg"] * kap * max(L.EPS, L.PCG_TOL) <= 1e-6 and L.rho_margin_ok(ref3, o)


def test_whitening_is_the_weighted_cost():
    g = P.graph("n60")
    om, W = P.weights("n60", "dense")
    prob, base = P.problem("n60", "dense"), L.pg_problem(g)
    r = base.lin(base.x0, False)[0]
    want = 0.5 * np.einsum("ea,eab,eb->", r, om, r)
    assert abs(prob.cost(prob.x0) - want) <= 1e-12 * want
    rw, Jw, _ = prob.lin(prob.x0)
    _, J, _ = base.lin(base.x0)
    assert np.array_equal(rw, P.whiten(W, r)) and np.array_equal(Jw[:, :, :6], W @ J[:, :, :6])
    # a transposed W is another problem: the sqrt set tells them apart by far more than any bound of the GPU tests
    _, Ws = P.weights("n60", "sqrt")
    a = P.whiten(Ws, r); b = P.whiten(Ws.transpose(0, 2, 1), r)
    assert np.abs(a - b).max() > 1e-3 * np.abs(a).max()


def mp_whitened_step(prob, opt):
    """the first LM step of the whitened problem at 50 digits: residuals and Jacobians from mp_ref, whitened, H and g summed and the
    scaling and damping formed in mpmath; the damped system is solved by iterative refinement whose residual b - A x is formed at
    50 digits (float64 LU as the corrector: every round gains log10(1 / (kappa eps)) digits), until the correction is below 1e-40"""
    n = prob.n_local
    P7 = prob.x0.reshape(-1, 7)
    H = mp.zeros(n, n)
    g = [mp.mpf(0)] * n
    for e in range(len(prob.ei)):
        r, Ji, Jj = M.pg_jacobians_build(M.pose(P7[prob.ei[e]]), M.pose(P7[prob.ej[e]]), M.pose(prob.meas[e]))
        Wm = mp.matrix(prob.W[e].tolist())
        J = mp.matrix(6, 12)
        for a in range(6):
            for b in range(6): J[a, b] = Ji[a, b]; J[a, 6 + b] = Jj[a, b]
        J = Wm * J
        rw = Wm * mp.matrix([r[a] for a in range(6)])
        cols = list(prob.cols[e])
        Hb, gb = J.T * J, J.T * rw
        for a in range(12):
            g[cols[a]] += gb[a]
            for b in range(12):
                H[cols[a], cols[b]] += Hb[a, b]
    free = [i for i in range(n) if prob.free[i]]
    s = [1 / (1 + mp.sqrt(H[i, i])) for i in range(n)]
    A = mp.matrix(len(free), len(free))
    bvec = mp.matrix(len(free), 1)
    for ia, i in enumerate(free):
        bvec[ia] = -s[i] * g[i]
        for ja, j in enumerate(free):
            A[ia, ja] = s[i] * H[i, j] * s[j]
        A[ia, ia] += min(max(s[i] ** 2 * H[i, i], mp.mpf(opt["min_lm_diagonal"])), mp.mpf(opt["max_lm_diagonal"])) / \
            mp.mpf(opt["initial_trust_region_radius"])
    A64 = np.array(A.tolist(), dtype=float)
    y = mp.matrix(len(free), 1)
    for _ in range(12):
        res = bvec - A * y
        c = np.linalg.solve(A64, np.array([float(v) for v in res]))
        y += mp.matrix(c.tolist())
        if np.abs(c).max() <= 1e-40 * max(abs(float(v)) for v in y):
            break
    else:
        raise AssertionError("the 50-digit refinement did not converge")
    d = np.zeros(n)
    for ia, i in enumerate(free):
        d[i] = float(s[i] * y[ia])
    return d


def test_whitened_reference_step_matches_a_50_digit_redo():
    """the 60-node graph, weight set "dense": the FP64 reference's first step against the 50-digit one.  The measured number --
    err / (kappa eps |delta|) -- is what the GPU step test may lean on if it ever needs a larger eps_eff (ten times this figure;
    tests/test_gpu_pg_information.py uses the unweighted case's eps_eff)."""
    prob = P.problem("n60", "dense")
    opt = L.lm_options(**P.LM_OPTIONS)
    ref = P.reference("n60", "dense", 3)
    d = mp_whitened_step(prob, opt)
    kap = ref[0]["kappa"]
    err = np.linalg.norm(ref[0]["delta"] - d)
    print(f"n60 dense: kappa {kap:.2e}, |delta| {np.linalg.norm(d):.3e}, err {err:.3e}, err / (kappa eps |delta|) = {err / (kap * L.EPS * np.linalg.norm(d)):.2e}")
    assert err <= 4 * kap * L.EPS * np.linalg.norm(d)          # the bound test_lm_step_reference.py holds the unweighted step to


# ------------------------------------------------------------------------------- the Python layer, no device
def test_engine_refuses_both_keywords_and_wrong_shapes_before_any_device_work():
    st = importlib.import_module("slam-tricks_amd")
    g = P.graph("n60")
    m = len(g["edge_i"])
    args = (g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"])
    om = np.tile(np.eye(6), (m, 1, 1))
    with pytest.raises(ValueError, match="not both"):
        st.PGEngine(*args, information=om, sqrt_information=om)
    for bad in (om[:-1], np.eye(6), np.ones((m, 6)), np.ones((m + 1, 36))):
        with pytest.raises(ValueError, match="shape"):
            st.PGEngine(*args, information=bad)
        with pytest.raises(ValueError, match="shape"):
            st.PGEngine(*args, sqrt_information=bad)
    for name in ("stba_pg_set_information", "stba_pg_set_sqrt_information", "stba_pg_has_information"):
        assert name in st.EXPORTS and hasattr(st.lib(), name)
    assert st.lib().stba_pg_set_information(None, None) == -1          # STBA_ERR_INVALID_ARGUMENT: a null engine, no device needed
    has = importlib.import_module("ctypes").c_int(7)
    assert st.lib().stba_pg_has_information(None, None) == -1 and has.value == 7


def test_make_pg_shard_slices_the_weights_with_their_edges():
    sharding = importlib.import_module("slam-tricks_amd.sharding")
    g = P.graph("n40_pad")
    om, W = P.weights("n40_pad", "dense")
    m = len(g["edge_i"])
    seen = 0
    for rank in range(3):
        sh = sharding.make_pg_shard(dict(g, information=om), rank, 3)
        assert np.array_equal(sh["information"], om[sh["lo"]:sh["hi"]]) and len(sh["information"]) == len(sh["edge_i"])
        assert "sqrt_information" not in sh
        sh2 = sharding.make_pg_shard(dict(g, sqrt_information=W), rank, 3)
        assert np.array_equal(sh2["sqrt_information"], W[sh2["lo"]:sh2["hi"]]) and np.array_equal(sh2["edge_i"], g["edge_i"][sh2["lo"]:sh2["hi"]])
        seen += len(sh["edge_i"])
    assert seen == m
    plain = sharding.make_pg_shard(g, 0, 2)
    assert "information" not in plain and "sqrt_information" not in plain
