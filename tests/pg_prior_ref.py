"""Reference for node pose priors of the pose graph.  No reference of the suite knows a prior, and none has to: a prior

    r_k = log(Z_k^-1 T_n),   J_k = Jr^-1(r_k),   cost += 1/2 |W_k r_k|^2

is the relative-pose edge whose other end is a CONSTANT node at the identity (T_i = I in log(Z^-1 T_i^-1 T_j)).  augment() appends that
virtual node and one edge per prior to a graph; the oracle's PG, lm_step_ref, pg_covariance_ref and pg_information_ref.whiten then judge
the feature on the augmented graph as they are, and drop_virtual() takes the virtual node out of a reference's answer.  CPU only.

The prior sets (tests/test_pg_prior_reference_cpu.py checks their properties, cond(J) among them):
  "few"        6 priors with a general full-rank W (cond <= 10): a node that carries two (3, 3), and nodes n/2 and 0 -- the constant
               nodes of the graphs that have any -- so that a constant node's prior is in every run;
  "dense"      the same nodes, given as information matrices Omega = Q diag(lambda) Q^T (the reference whitens with the 50-digit factor);
  "gps"        position-only W = [I / sigma, 0; 0, 0] on every third node, through the sqrt entry point;
  "three_pos"  position-only priors on nodes 3, 17, n - 1: the smallest set that fixes the gauge without a rotation row;
  "single_pos" one position-only prior: the rotation about that point stays free (three singular values of J at rounding level);
  "many"       seven priors on EVERY node (n40_pad: 280 priors, a second workgroup of the per-prior kernel; node 36's seven priors are
               252..258 and straddle the workgroup boundary at 256; 40 prior-bearing nodes are a second workgroup of the per-node kernel)."""
import functools

import numpy as np

import lm_step_ref as L
import pg_information_ref as P

EPS = L.EPS
LM_OPTIONS = P.LM_OPTIONS
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
PRIORS_PER_WORKGROUP = 256          # PGEngine.prior_kernel_geometry(), asserted by the GPU test
NODES_PER_WORKGROUP = 32
SETS = ("few", "dense", "gps", "three_pos", "single_pos", "many")


@functools.lru_cache(maxsize=None)
def graph(name):
    """pg_information_ref's graphs, lm_step_ref's n150, and `<name>_free`: the same graph with no constant node; "chain12": 12 nodes
    joined by odometry edges alone, no constant node"""
    if name.endswith("_free"):
        g = graph(name[:-5])
        return dict(g, node_fixed=np.zeros_like(g["node_fixed"]))
    if name == "n150":
        return L.pg_scene(**L.PG_CASES["n150"][0])
    if name == "chain12":
        g = L.pg_scene(n_nodes=40)
        keep = (g["edge_j"] == g["edge_i"] + 1) & (g["edge_j"] < 12)
        return dict(poses0=g["poses0"][:12], poses_true=g["poses_true"][:12], edge_i=g["edge_i"][keep], edge_j=g["edge_j"][keep],
                    meas=g["meas"][keep], node_fixed=np.zeros(12, np.uint8))
    return P.graph(name)


def _noisy(g, nodes, rng, sigma_t=0.03, sigma_r=0.01):
    """the true poses of `nodes` times a small noise: what a fix would measure"""
    T = g["poses_true"][nodes]
    noise = np.concatenate([rng.normal(0, sigma_t, (len(nodes), 3)), rng.normal(0, sigma_r, (len(nodes), 3))], 1)
    return L.rt_pose(*L.se3_compose_rt(L.pose_rt(T), L.se3_exp(noise)))


@functools.lru_cache(maxsize=None)
def priors(gname, kind):
    """dict(nodes, poses, W, information | None): W is what the reference whitens with; the engine gets `information` where it is not
    None, else W through the sqrt entry point (engine_kwargs)"""
    g = graph(gname)
    n = len(g["poses0"])
    rng = np.random.default_rng(100 + SETS.index(kind) + 10 * (sum(map(ord, gname)) % 7))
    om = None
    if kind in ("few", "dense"):
        nodes = np.array([3, 3, 17 % n, n // 2, n - 1, 0], np.int32)
        Q1, Q2 = P._orthogonal(rng, len(nodes)), P._orthogonal(rng, len(nodes))
        if kind == "few":
            W = np.einsum("eab,eb,ecb->eac", Q1, 10.0 ** rng.uniform(0, 1, (len(nodes), 6)), Q2)
        else:
            om = np.einsum("eab,eb,ecb->eac", Q1, 10.0 ** rng.uniform(0, 3, (len(nodes), 6)), Q1)
            om = 0.5 * (om + om.transpose(0, 2, 1))
            W = P.chol_T(om)
    elif kind in ("gps", "three_pos", "single_pos"):
        nodes = {"gps": np.arange(1, n, 3), "three_pos": np.array([3, 17 % n, n - 1]), "single_pos": np.array([5])}[kind].astype(np.int32)
        W = np.zeros((len(nodes), 6, 6))
        W[:, np.arange(3), np.arange(3)] = 1.0 / np.array([0.5, 0.25, 1.0, 2.0])[np.arange(len(nodes)) % 4][:, None]
    else:
        assert kind == "many"
        nodes = np.repeat(np.arange(n), 7).astype(np.int32)
        Q1, Q2 = P._orthogonal(rng, len(nodes)), P._orthogonal(rng, len(nodes))
        W = np.einsum("eab,eb,ecb->eac", Q1, 10.0 ** rng.uniform(-1, 0, (len(nodes), 6)), Q2)
    return dict(nodes=nodes, poses=_noisy(g, nodes, rng), W=np.ascontiguousarray(W), information=om)


def engine_kwargs(pr):
    kw = dict(nodes=pr["nodes"], poses=pr["poses"])
    if pr["information"] is not None:
        return dict(kw, information=pr["information"])
    return dict(kw, sqrt_information=pr["W"])


def augment(g, pr):
    """the graph with one more node -- at the identity, constant -- and one edge (virtual node -> prior's node) per prior, behind the
    graph's own edges; the prior's pose is the edge's measurement"""
    n = len(g["poses0"])
    k = len(pr["nodes"])
    out = dict(g)
    out["poses0"] = np.vstack([g["poses0"], IDENTITY])
    if "poses_true" in g:
        out["poses_true"] = np.vstack([g["poses_true"], IDENTITY])
    out["edge_i"] = np.concatenate([g["edge_i"], np.full(k, n)]).astype(np.int32)
    out["edge_j"] = np.concatenate([g["edge_j"], pr["nodes"]]).astype(np.int32)
    out["meas"] = np.vstack([g["meas"], pr["poses"]])
    out["node_fixed"] = np.append(g["node_fixed"], 1).astype(np.uint8)
    return out


def augmented_weights(g, pr, W_edges=None):
    """[m + k][6][6]: the edges' W (the identity where none is given), then the priors'"""
    m = len(g["edge_i"])
    We = np.tile(np.eye(6), (m, 1, 1)) if W_edges is None else np.asarray(W_edges, float)
    return np.concatenate([We, pr["W"]], 0)


def problem(g, pr, W_edges=None):
    """the whitened lm_step_ref problem of the augmented graph"""
    return P.WeightedPGProblem(augment(g, pr), augmented_weights(g, pr, W_edges))


def drop_virtual(ref):
    """a reference's per-iteration dicts (lm_step_ref.lm_reference on an augmented problem) without the virtual node: its pose (the
    last 7 of x, x_trial) and its step (the last 6 of delta, zero: it is constant) go, everything else -- costs, norms, which leave
    constant nodes out anyway -- stays"""
    out = []
    for it in ref:
        it = dict(it)
        it["x"], it["x_trial"], it["delta"] = it["x"][:-7], it["x_trial"][:-7], it["delta"][:-6]
        out.append(it)
    return out


def drop_virtual_covariance(C):
    """(6 (n + 1)) x (6 (n + 1)) of an augmented graph -> 6 n x 6 n (the virtual node's rows and columns are zero: it is constant)"""
    return C[:-6, :-6]


@functools.lru_cache(maxsize=None)
def reference(gname, kind, k):
    g, pr = graph(gname), priors(gname, kind)
    return L.lm_reference(problem(g, pr), L.lm_options(**LM_OPTIONS), k)


def jacobian(g, pr, W_edges=None, x=None):
    """the whitened Jacobian of the augmented problem at poses0 (or at x, the virtual node's pose included), dense
    (6 (m + k)) x (6 n): the virtual node's and the constant nodes' columns dropped"""
    prob = problem(g, pr, W_edges)
    r, J, cols = prob.lin(prob.x0 if x is None else x)
    n = prob.n_local
    D = np.zeros((6 * len(r), n))
    for e in range(len(r)):
        D[6 * e:6 * e + 6, cols[e]] += J[e]
    return D[:, prob.free]
