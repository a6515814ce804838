"""Independent reference for the pose-graph covariance: numpy / scipy on the ORACLE's residual Jacobians (oracle/oracle_py.py, PG.evaluate),
never the engine's own evaluate.

    H = J^T J   (6 n x 6 n, rows and columns of constant nodes zero), tangent [rho, theta] per node, T <- T exp(delta)
    C = H_free^-1 put back into 6 n x 6 n with zeros for constant nodes

dense_covariance inverts H_free with numpy; lu_columns solves for the six columns of one node with a sparse LU (any size)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

EPS = 2.2e-16


def jacobian(O, poses, edge_i, edge_j, meas, node_fixed=None):
    """the residual Jacobian (6 m x 6 n, scipy CSR) from the oracle's 6x6 blocks; columns of constant nodes are zero"""
    n, m = len(poses), len(edge_i)
    pg = O.PG(poses, edge_i, edge_j, meas, node_fixed)
    _, _, Ji, Jj = pg.evaluate(jac=True)
    ei = np.asarray(edge_i, np.int64); ej = np.asarray(edge_j, np.int64)
    rows = (6 * np.arange(m)[:, None, None] + np.arange(6)[None, :, None] + np.zeros((1, 1, 6), np.int64))
    ci = (6 * ei[:, None, None] + np.zeros((1, 6, 1), np.int64) + np.arange(6)[None, None, :])
    cj = (6 * ej[:, None, None] + np.zeros((1, 6, 1), np.int64) + np.arange(6)[None, None, :])
    J = sp.coo_matrix((np.concatenate([Ji.ravel(), Jj.ravel()]),
                       (np.concatenate([rows.ravel(), rows.ravel()]), np.concatenate([ci.ravel(), cj.ravel()]))),
                      shape=(6 * m, 6 * n)).tocsr()
    if node_fixed is not None:
        keep = np.repeat(np.asarray(node_fixed) == 0, 6).astype(float)
        J = J @ sp.diags(keep)
    return J


def hessian(O, poses, edge_i, edge_j, meas, node_fixed=None):
    J = jacobian(O, poses, edge_i, edge_j, meas, node_fixed)
    return (J.T @ J).tocsc()


def free_dofs(n, node_fixed=None):
    if node_fixed is None:
        return np.arange(6 * n)
    return np.flatnonzero(np.repeat(np.asarray(node_fixed) == 0, 6))


def dense_covariance(H, node_fixed=None):
    """(C, lambda_min, kappa): C 6 n x 6 n dense with zeros for constant nodes; the extreme eigenvalues of H_free (eigvalsh)"""
    N = H.shape[0]
    f = free_dofs(N // 6, node_fixed)
    Hf = H[f][:, f].toarray()
    w = np.linalg.eigvalsh(Hf)
    C = np.zeros((N, N))
    C[np.ix_(f, f)] = np.linalg.inv(Hf)
    return C, w[0], w[-1] / w[0]


def lu_columns(H, node, node_fixed=None):
    """(6 n, 6): the six columns of C that belong to `node`, by a sparse LU of H_free"""
    N = H.shape[0]
    f = free_dofs(N // 6, node_fixed)
    pos = -np.ones(N, np.int64); pos[f] = np.arange(len(f))
    out = np.zeros((N, 6))
    if node_fixed is not None and node_fixed[node]:
        return out
    E = np.zeros((len(f), 6))
    E[pos[6 * node:6 * node + 6], np.arange(6)] = 1.0
    lu = spla.splu(H[f][:, f].tocsc())
    out[f] = lu.solve(E)
    return out


def block(C, a, b):
    return C[6 * a:6 * a + 6, 6 * b:6 * b + 6]


def block_bound(rho, kappa, lam_min):
    """|C_ab - C*_ab|_F <= sqrt(6) (rho + 50 kappa eps) / lambda_min: a column's error is at most |H^-1| |residual|, six columns per
    block; 50 kappa eps is the fp64 term tests/test_gpu_covariance.py uses"""
    return np.sqrt(6.0) * (rho + 50.0 * kappa * EPS) / lam_min


def numeric_hessian(O, poses, edge_i, edge_j, meas, node_fixed=None, h=1e-6):
    """J^T J with J by central differences of the oracle's RESIDUALS over T <- T exp(delta) (small graphs)"""
    poses = np.asarray(poses, float).reshape(-1, 7)
    n, m = len(poses), len(edge_i)
    J = np.zeros((6 * m, 6 * n))
    for v in range(n):
        if node_fixed is not None and node_fixed[v]:
            continue
        for k in range(6):
            d = np.zeros(6); d[k] = h
            rs = []
            for sgn in (1.0, -1.0):
                p = poses.copy()
                p[v] = O.se3_retract(poses[v], sgn * d)
                rs.append(O.PG(p, edge_i, edge_j, meas, node_fixed).evaluate(jac=False)[1].ravel())
            J[:, 6 * v + k] = (rs[0] - rs[1]) / (2 * h)
    return J.T @ J


def add_leaf(scene, parent, rel):
    """the scene with one more node that hangs on `parent` by a single edge with measurement `rel` (7 doubles)"""
    import oracle_py as O
    s = {k: np.array(v) for k, v in scene.items()}
    new = O.se3_compose(s["poses0"][parent], rel)
    n = len(s["poses0"])
    s["poses0"] = np.vstack([s["poses0"], new]); s["poses_true"] = np.vstack([s["poses_true"], new])
    s["edge_i"] = np.append(s["edge_i"], parent).astype(np.int32); s["edge_j"] = np.append(s["edge_j"], n).astype(np.int32)
    s["meas"] = np.vstack([s["meas"], rel]); s["node_fixed"] = np.append(s["node_fixed"], 0).astype(np.uint8)
    return s


def small_cases(scenes):
    """the small graphs of the GPU test: (name, scene, tested pairs).  Chosen on the CPU (tests/test_pg_covariance_reference.py checks
    it) so that block_bound(1e-12, kappa, lambda_min) <= 1e-6 |C*_ab|_F for every tested pair."""
    cases = []
    s = scenes.pose_graph_scene(n_nodes=24, loops_per_node=3, seed=11, turns=2)
    cases.append(("one fixed node, 24 nodes", s, _pairs(s, [1, 5, 12, 17, 23])))
    s = scenes.pose_graph_scene(n_nodes=120, loops_per_node=3, seed=12, turns=4)
    s["node_fixed"][[0, 50, 119]] = 1
    cases.append(("several fixed nodes, 120 nodes", s, _pairs(s, [1, 20, 49, 51, 80, 100, 118])))
    s = scenes.pose_graph_scene(n_nodes=36, loops_per_node=3, seed=13, turns=3)
    s["node_fixed"][:] = 0; s["node_fixed"][18] = 1
    cases.append(("a fixed node in the middle, 36 nodes", s, _pairs(s, [0, 10, 17, 19, 28, 35])))
    s = scenes.pose_graph_scene(n_nodes=500, loops_per_node=3, seed=5, turns=8)
    s["node_fixed"][::50] = 1; s["node_fixed"][499] = 1
    s = add_leaf(s, 275, np.array([0.0, 0.0, np.sin(0.05), np.cos(0.05), 0.3, -0.2, 0.1]))
    cases.append(("several fixed nodes and a node with a single edge, 501 nodes", s, _pairs(s, [1, 25, 75, 274, 275, 276, 333, 498]) + [(500, 500), (500, 275), (275, 500)]))
    return cases


def _pairs(s, nodes):
    """diagonal blocks, neighbour blocks both ways (C[a, b] and C[b, a])"""
    n = len(s["poses0"])
    out = []
    for a in nodes:
        out.append((a, a))
        b = a + 1 if a + 1 < n else a - 1
        if not s["node_fixed"][b]:
            out += [(a, b), (b, a)]
    return out
