"""The reference of the pose-graph covariance tests (tests/pg_covariance_ref.py) checks itself, on the CPU: its H, assembled from the
oracle's Jacobians, against a central-difference J^T J; its dense inverse against its sparse-LU columns; and the condition the GPU
test puts on its inputs -- for every tested block of every small graph the error bound is at most 1e-6 of the block's norm."""
import numpy as np

import pg_covariance_ref as R


def six_node_graph(scenes):
    s = scenes.pose_graph_scene(n_nodes=6, loops_per_node=1, seed=3, sigma_t=0.02, sigma_r=0.01, turns=1)
    return s


def test_hessian_from_oracle_jacobians_equals_central_differences(O, scenes):
    s = six_node_graph(scenes)
    H = R.hessian(O, s["poses0"], s["edge_i"], s["edge_j"], s["meas"], s["node_fixed"]).toarray()
    Hn = R.numeric_hessian(O, s["poses0"], s["edge_i"], s["edge_j"], s["meas"], s["node_fixed"])
    assert H.shape == (36, 36)
    assert np.all(H[:6] == 0) and np.all(H[:, :6] == 0)          # node 0 is constant
    # central differences with h = 1e-6: truncation h^2 |r'''| and rounding eps / h, both ~1e-10 per Jacobian entry
    assert np.abs(H - Hn).max() <= 1e-7 * np.abs(H).max()


def test_dense_inverse_and_sparse_lu_columns_agree(O, scenes):
    s = scenes.pose_graph_scene(n_nodes=60, loops_per_node=2, seed=9, turns=3)
    s["node_fixed"][37] = 1
    H = R.hessian(O, s["poses0"], s["edge_i"], s["edge_j"], s["meas"], s["node_fixed"])
    Cd, lam_min, kappa = R.dense_covariance(H, s["node_fixed"])
    assert lam_min > 0
    for node in (1, 30, 59):
        X = R.lu_columns(H, node, s["node_fixed"])
        ref = Cd[:, 6 * node:6 * node + 6]
        assert np.abs(X - ref).max() <= 100 * kappa * R.EPS * np.abs(ref).max()
        assert np.all(X[:6] == 0) and np.all(X[6 * 37:6 * 38] == 0)
    assert np.all(R.lu_columns(H, 37, s["node_fixed"]) == 0)
    assert np.abs(Cd - Cd.T).max() <= 100 * kappa * R.EPS * np.abs(Cd).max()


def test_small_cases_make_the_bound_tight(O, scenes):
    for name, s, pairs in R.small_cases(scenes):
        H = R.hessian(O, s["poses0"], s["edge_i"], s["edge_j"], s["meas"], s["node_fixed"])
        C, lam_min, kappa = R.dense_covariance(H, s["node_fixed"])
        bound = R.block_bound(1e-12, kappa, lam_min)
        worst = max(bound / np.linalg.norm(R.block(C, a, b)) for a, b in pairs)
        print(f"{name}: lambda_min {lam_min:.3e} kappa {kappa:.3e} bound {bound:.3e} worst bound / |C_ab| {worst:.3e}")
        assert worst <= 1e-6, name
    deg = np.bincount(np.r_[s["edge_i"], s["edge_j"]])
    assert deg[500] == 1                                         # the last case has a node with a single edge
