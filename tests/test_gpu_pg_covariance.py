"""Pose-graph covariance on the GPU (PGEngine.covariance / covariance_columns, pg_covariance.hip) against an independent reference:
numpy / scipy on the ORACLE's Jacobians (tests/pg_covariance_ref.py).

Small graphs (pg_covariance_ref.small_cases; lambda_min and kappa of H_free by eigvalsh, checked on the CPU by
tests/test_pg_covariance_reference.py):
    one fixed node, 24 nodes                                       kappa 6.8e4
    several fixed nodes, 120 nodes                                 kappa 2.1e4
    a fixed node in the middle, 36 nodes                           kappa 6.0e4
    several fixed nodes and a node with a single edge, 501 nodes   kappa 4.6e3
Every requested block must satisfy |C_ab - C*_ab|_F <= sqrt(6) (rho + 50 kappa eps) / lambda_min with rho the largest true relative
residual the call itself reports: a column's error is at most |H^-1| |residual|, and 50 kappa eps is the fp64 term of
tests/test_gpu_covariance.py.  The scenes are chosen so that this bound is at most 1e-6 of |C*_ab|_F for every tested block.

At scale (C4, 10 000 nodes, kappa 4.5e7, lambda_min 1.9e-6 by eigsh): the requested tolerance is 1e-9, not the default 1e-12 --
fp64 evaluates e - H x only to about eps |H| |x| ~ 2.2e-16 x 84 x 1e3 x a few, and the sparse LU's own solution of the far-end
node has a residual of 6e-11."""
import importlib

import numpy as np
import pytest

import pg_covariance_ref as R

pytestmark = pytest.mark.gpu

STBA_ERR_INVALID_ARGUMENT = -1
STBA_ERR_NOT_POSITIVE_DEFINITE = -4
STBA_ERR_STATE = -6
TOL = 1e-12


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0
    return mod


def engine(st, s):
    return st.PGEngine(s["poses0"], s["edge_i"], s["edge_j"], s["meas"], s["node_fixed"])


@pytest.mark.parametrize("case", range(4))
def test_small_graphs_against_the_dense_inverse(st, O, scenes, case):
    name, s, pairs = R.small_cases(scenes)[case]
    H = R.hessian(O, s["poses0"], s["edge_i"], s["edge_j"], s["meas"], s["node_fixed"])
    Cs, lam_min, kappa = R.dense_covariance(H, s["node_fixed"])
    fixed = np.flatnonzero(s["node_fixed"])
    free = np.flatnonzero(s["node_fixed"] == 0)
    zero_pairs = [(int(fixed[0]), int(fixed[0])), (int(fixed[0]), int(free[0])), (int(free[0]), int(fixed[-1]))]
    e = engine(st, s)
    C, summ = e.covariance(pairs + zero_pairs, relative_tolerance=TOL)
    rho = summ["max_relative_residual"]
    bound = R.block_bound(rho, kappa, lam_min)
    print(f"{name}: lambda_min {lam_min:.3e} kappa {kappa:.3e} rho {rho:.3e} bound {bound:.3e} summary {summ}")
    assert rho <= TOL
    got = {}
    worst = 0.0
    for k, (a, b) in enumerate(pairs):
        ref = R.block(Cs, a, b)
        err = np.linalg.norm(C[k] - ref)
        worst = max(worst, err / bound)
        print(f"  C[{a},{b}] |err|_F {err:.3e} |C*|_F {np.linalg.norm(ref):.3e}")
        assert bound <= 1e-6 * np.linalg.norm(ref), (a, b)          # the condition on the inputs: the bound means something
        assert err <= bound, (a, b, err, bound)
        got[(a, b)] = C[k]
    print(f"  worst error / bound {worst:.3e}")
    for (a, b), blk in got.items():
        if a == b:
            assert np.linalg.norm(blk - blk.T) <= bound
        elif (b, a) in got:
            assert np.linalg.norm(blk - got[(b, a)].T) <= bound
    assert np.all(C[len(pairs):] == 0.0)                             # pairs that name a fixed node: exact zeros
    C2, _ = e.covariance(pairs + zero_pairs, relative_tolerance=TOL)
    assert np.array_equal(C, C2)                                     # two calls, the same bits
    assert summ["columns"] == 6 * len({b for _, b in pairs}) and summ["batches"] == -(-summ["columns"] // 64)


def test_columns_of_a_small_graph(st, O, scenes):
    name, s, pairs = R.small_cases(scenes)[1]
    H = R.hessian(O, s["poses0"], s["edge_i"], s["edge_j"], s["meas"], s["node_fixed"])
    Cs, lam_min, kappa = R.dense_covariance(H, s["node_fixed"])
    e = engine(st, s)
    X, summ = e.covariance_columns(80, relative_tolerance=TOL)
    bound = R.block_bound(summ["max_relative_residual"], kappa, lam_min)
    assert summ["max_relative_residual"] <= TOL and summ["columns"] == 6
    for a in range(len(s["poses0"])):
        assert np.linalg.norm(X[6 * a:6 * a + 6] - R.block(Cs, a, 80)) <= bound
    assert np.all(X[6 * 50:6 * 51] == 0)
    Z, zs = e.covariance_columns(50)                                 # a fixed node: zeros, nothing solved
    assert np.all(Z == 0) and zs["columns"] == 0
    blk, _ = e.covariance([(3, 80), (80, 80)], relative_tolerance=TOL)
    assert np.array_equal(blk[0], X[18:24]) and np.array_equal(blk[1], X[480:486])


def test_solve_after_a_covariance_call_is_bit_identical(st, scenes):
    _, s, pairs = R.small_cases(scenes)[1]
    a, b = engine(st, s), engine(st, s)
    a.covariance(pairs)
    sa, ta, na = a.solve(max_num_iterations=8)
    sb, tb, nb = b.solve(max_num_iterations=8)
    assert np.array_equal(a.get_poses(), b.get_poses()) and np.array_equal(ta, tb) and na == nb
    # and between two solves, at poses the first one moved
    a.covariance_columns(7)
    a.solve(max_num_iterations=4); b.solve(max_num_iterations=4)
    assert np.array_equal(a.get_poses(), b.get_poses())


def test_bad_inputs_are_refused(st, scenes):
    _, s, _ = R.small_cases(scenes)[0]
    e = engine(st, s)
    n = len(s["poses0"])
    for bad in ([(0, n)], [(-1, 2)], [(1, 1), (n + 5, 1)]):
        with pytest.raises(st.StbaError) as err:
            e.covariance(bad)
        assert err.value.code == STBA_ERR_INVALID_ARGUMENT
    for bad in (-1, n):
        with pytest.raises(st.StbaError) as err:
            e.covariance_columns(bad)
        assert err.value.code == STBA_ERR_INVALID_ARGUMENT
    e.set_allreduce(lambda user, buf, count, stream: 0, 0, 1)
    with pytest.raises(st.StbaError) as err:
        e.covariance([(1, 1)])
    assert err.value.code == STBA_ERR_STATE


def test_gauge_free_graph_is_refused_with_out_untouched(st, scenes):
    import ctypes as C
    _, s, _ = R.small_cases(scenes)[0]
    s = dict(s); s["node_fixed"] = np.zeros(len(s["poses0"]), np.uint8)
    e = engine(st, s)
    out = np.full(36, 7.0)
    a = np.ones(1, np.int32)
    rc = st.lib().stba_pg_covariance(e._h, 1, st._p(a), st._p(a), None, st._p(out), None)
    assert rc == STBA_ERR_NOT_POSITIVE_DEFINITE and np.all(out == 7.0)
    assert b"component of 24 nodes" in st.lib().stba_last_error()
    cols = np.full(6 * 24 * 6, 7.0)
    rc = st.lib().stba_pg_covariance_columns(e._h, 3, None, st._p(cols), None)
    assert rc == STBA_ERR_NOT_POSITIVE_DEFINITE and np.all(cols == 7.0)


def test_c4_columns_against_sparse_lu(st, O, scenes):
    import scipy.sparse.linalg as spla
    tol = 1e-9                                                       # (the module docstring: why not 1e-12)
    s = scenes.pose_graph_scene(n_nodes=10000, loops_per_node=3, seed=4)
    n = 10000
    H = R.hessian(O, s["poses0"], s["edge_i"], s["edge_j"], s["meas"], s["node_fixed"])
    f = R.free_dofs(n, s["node_fixed"])
    Hf = H[f][:, f].tocsc()
    lu = spla.splu(Hf)
    # lambda_max by Lanczos on H_free, lambda_min by Lanczos on its inverse (the LU): scipy.sparse.linalg.eigsh, both converge
    lam_max = spla.eigsh(Hf, k=1, which="LA", return_eigenvectors=False)[0]
    lam_min = 1.0 / spla.eigsh(spla.LinearOperator(Hf.shape, matvec=lu.solve, dtype=float), k=1, which="LA", return_eigenvectors=False)[0]
    kappa = lam_max / lam_min
    print(f"C4: lambda_min {lam_min:.3e} lambda_max {lam_max:.3e} kappa {kappa:.3e} (eigsh)")
    e = engine(st, s)
    cols = {}
    for node in (1, 5000, 9999):                                     # next to the fixed node, mid-trajectory, the far end
        X, summ = e.covariance_columns(node, relative_tolerance=tol)
        cols[node] = X
        rho = summ["max_relative_residual"]
        E = np.zeros((6 * n, 6)); E[6 * node + np.arange(6), np.arange(6)] = 1.0
        res = np.linalg.norm(H @ X - E, axis=0)                      # |E_k| = 1
        Xlu = np.zeros_like(X); Xlu[f] = lu.solve(E[f])
        bound = R.block_bound(rho, kappa, lam_min)
        err = np.linalg.norm((X - Xlu).reshape(n, 36), axis=1).max()
        print(f"  node {node}: {summ} scipy residual {res.max():.3e} worst block error against LU {err:.3e} bound {bound:.3e} |C_bb| {np.linalg.norm(X[6 * node:6 * node + 6]):.3e}")
        assert rho <= tol
        assert res.max() <= 10 * tol
        assert err <= bound
        assert np.all(X[:6] == 0)
    # more distinct nodes than one batch of 64 columns holds: every block equals the single-node answer bit for bit
    others = [2, 700, 1500, 2600, 3100, 4999, 5001, 6400, 7777, 8800]
    pairs = [(b, b) for b in (1, 5000, 9999)] + [(b, b) for b in others] + [(9999, 5000), (1, 9999), (5000, 1), (3, 5000)]
    C, summ = e.covariance(pairs, relative_tolerance=tol)
    print(f"  batch of {len(pairs)} pairs: {summ}")
    assert summ["batches"] == 2 and summ["columns"] == 78 and summ["max_relative_residual"] <= tol
    for k, (a, b) in enumerate(pairs):
        if b in cols:
            assert np.array_equal(C[k], cols[b][6 * a:6 * a + 6]), (a, b)
