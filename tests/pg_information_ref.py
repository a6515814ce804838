"""Reference for pose-graph edge information matrices: the oracle and lm_step_ref.py know no weights, so this module WHITENS what they
give.  Per edge e a 6 x 6 square-root information W_e, tangent order [rho, theta] of the residual:

    r~ = W r,   J~ = blockdiag(W) J,   cost = 1/2 sum |W_e r_e|^2,   Omega_e = W_e^T W_e

and for an information matrix given as such, Omega = L L^T (Cholesky) and W = L^T (include/stba.h).  CPU only, numpy (+ mpmath for
the 50-digit Cholesky factor).

The inputs of the tests (tests/test_pg_information_cpu.py checks their properties on the CPU):
  graphs   "n60": lm_step_ref.pg_scene's 60-node default with its loop closures (179 edges, one workgroup of the edge kernels);
           "n40_pad": the 40-node scene padded with extra loop edges to 304 edges, so that a second, partly filled workgroup exists
           (an SoA stride or tail bug is invisible below 257 edges).  Nodes 0 and n/2 are constant: node 0 is the i side of edge
           (0, 1), node n/2 the j side of edge (n/2 - 1, n/2).
  weights  "diag":  Omega diagonal, translation and rotation weights two decades apart, loop closures a quarter of the odometry's;
           "dense": Omega = Q diag(lambda) Q^T, Q a seeded random orthogonal basis, lambda log-uniform in [1, 1e4]: cond(W) <= 100;
           "sqrt":  a general W = Q1 diag(s) Q2^T, s log-uniform in [1, 100], neither triangular nor symmetric -- through the sqrt entry
                    point; the only set that catches a transposed W."""
import functools

import numpy as np

import lm_step_ref as L

EPS = L.EPS
GRAPHS = ("n60", "n40_pad")
WEIGHTS = ("diag", "dense", "sqrt")
LM_OPTIONS = dict(initial_trust_region_radius=1e2)          # lm_step_ref.PG_CASES' own
N_PAD_EDGES = 304


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "n60":
        return L.pg_scene(n_nodes=60)
    assert name == "n40_pad"
    g = L.pg_scene(n_nodes=40)
    rng = np.random.default_rng(41)
    n, m0 = 40, len(g["edge_i"])
    add = []
    while m0 + len(add) < N_PAD_EDGES:
        i, j = (int(v) for v in rng.integers(0, n, 2))
        if i != j and abs(i - j) > 1:
            add.append((i, j))                      # (parallel edges are fine: every one carries its own measurement and weight)
    ai, aj = np.array(add).T
    T = g["poses_true"]
    rel = L.se3_compose_rt(L.se3_inverse_rt(L.pose_rt(T[ai])), L.pose_rt(T[aj]))
    noise = np.concatenate([rng.normal(0, 0.05, (len(ai), 3)), rng.normal(0, 0.02, (len(ai), 3))], 1)
    meas = L.rt_pose(*L.se3_compose_rt(rel, L.se3_exp(noise)))
    return dict(g, edge_i=np.concatenate([g["edge_i"], ai]).astype(np.int32), edge_j=np.concatenate([g["edge_j"], aj]).astype(np.int32),
                meas=np.vstack([g["meas"], meas]))


def _orthogonal(rng, m):
    Q, R = np.linalg.qr(rng.normal(size=(m, 6, 6)))
    return Q * np.sign(np.diagonal(R, axis1=1, axis2=2))[:, None, :]


@functools.lru_cache(maxsize=None)
def weights(gname, kind):
    """(information | None, sqrt_information): what the engine is given ("diag", "dense": the information; "sqrt": W) and the W the
    reference whitens with"""
    g = graph(gname)
    m, n = len(g["edge_i"]), len(g["poses0"])
    rng = np.random.default_rng({"diag": 1, "dense": 2, "sqrt": 3}[kind] + 10 * GRAPHS.index(gname))
    if kind == "diag":
        scale = np.where(np.arange(m) < n - 1, 1.0, 0.25)              # odometry | loop closures
        om = np.zeros((m, 6, 6))
        om[:, np.arange(6), np.arange(6)] = scale[:, None] * np.array([4.0] * 3 + [400.0] * 3)
        return om, np.sqrt(om)
    if kind == "dense":
        Q = _orthogonal(rng, m)
        lam = 10.0 ** rng.uniform(0, 4, (m, 6))
        om = np.einsum("eab,eb,ecb->eac", Q, lam, Q)
        om = 0.5 * (om + om.transpose(0, 2, 1))
        return om, chol_T(om)
    Q1, Q2 = _orthogonal(rng, m), _orthogonal(rng, m)
    s = 10.0 ** rng.uniform(0, 2, (m, 6))
    return None, np.einsum("eab,eb,ecb->eac", Q1, s, Q2)


def chol_T(om):
    """W = L^T of Omega = L L^T per edge, the factor computed at 50 digits and rounded: the correctly rounded W of the Omega given
    (np.linalg.cholesky's own error is about cond(Omega) eps in the last pivots, which the 32 eps bound of the tests has no room for)"""
    import mpmath as mp
    out = np.zeros_like(om)
    with mp.workdps(50):
        for e in range(len(om)):
            Lm = mp.cholesky(mp.matrix(om[e].tolist()))
            out[e] = np.array([[float(Lm[b, a]) for b in range(6)] for a in range(6)])
    return out


def whiten(W, r, Ji=None, Jj=None):
    rw = np.einsum("eab,eb->ea", W, r)
    if Ji is None:
        return rw
    return rw, W @ Ji, W @ Jj


def whiten_bound(W, x, base):
    """the evaluate bound: every whitened entry is a 6-term sum on top of the unweighted entry's own error --
    32 eps sum_k |W_ak| |x_k| + the bound the unweighted evaluate test uses for x (tests/test_gpu_pose_graph.py: 1e-12 for r, 1e-11 for J)"""
    if x.ndim == 2:
        return 32 * EPS * np.einsum("eab,eb->ea", np.abs(W), np.abs(x)) + base
    return 32 * EPS * (np.abs(W) @ np.abs(x)) + base


class WeightedPGProblem(L.PGProblem):
    """lm_step_ref.PGProblem with the residual and the Jacobian whitened: lm_reference and compare work on it as they are"""

    def __init__(self, g, W):
        super().__init__(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"])
        self.W = np.asarray(W, float).reshape(-1, 6, 6)

    def lin(self, x, jac=True):
        r, J, cols = super().lin(x, jac)
        rw = np.einsum("eab,eb->ea", self.W, r)
        return rw, (None if J is None else self.W @ J), cols


def problem(gname, kind):
    return WeightedPGProblem(graph(gname), weights(gname, kind)[1])


@functools.lru_cache(maxsize=None)
def reference(gname, kind, k):
    """lm_reference on the whitened problem, computed once per case and shared (read-only) by the tests"""
    return L.lm_reference(problem(gname, kind), L.lm_options(**LM_OPTIONS), k)


def engine_kwargs(gname, kind):
    om, W = weights(gname, kind)
    return dict(information=om) if om is not None else dict(sqrt_information=W)


def whitened_jacobian(O, g, W):
    """blockdiag(W) J (scipy CSR, 6 m x 6 n) on the oracle's Jacobian (pg_covariance_ref.jacobian)"""
    import scipy.sparse as sp
    import pg_covariance_ref as R
    J = R.jacobian(O, g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"])
    return sp.block_diag([W[e] for e in range(len(W))], format="csr") @ J
