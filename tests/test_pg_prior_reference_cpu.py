"""CPU leg of the node pose priors: the reference of tests/pg_prior_ref.py -- a prior as an edge from a constant node at the identity --
is what it claims to be, at 50 digits too, and the prior sets the GPU tests use have the conditioning those tests lean on."""
import importlib

import mpmath as mp
import numpy as np
import pytest

import lm_step_ref as L
import mp_ref as M
import pg_information_ref as P
import pg_prior_ref as Q


def direct_residual(g, pr):
    """se3_log(Z^-1 T) by lm_step_ref's own functions, no virtual node"""
    Zinv = L.se3_inverse_rt(L.pose_rt(pr["poses"]))
    return L.se3_log(*L.se3_compose_rt(Zinv, L.pose_rt(g["poses0"][pr["nodes"]])))


@pytest.mark.parametrize("gname", ["n60", "n40_pad"])
def test_augmented_edges_are_the_prior(O, gname):
    g, pr = Q.graph(gname), Q.priors(gname, "few")
    a = Q.augment(g, pr)
    n, m, k = len(g["poses0"]), len(g["edge_i"]), len(pr["nodes"])
    assert len(a["poses0"]) == n + 1 and len(a["edge_i"]) == m + k and a["node_fixed"][n] == 1
    assert np.array_equal(a["edge_i"][m:], np.full(k, n)) and np.array_equal(a["edge_j"][m:], pr["nodes"])
    _, r, Ji, Jj = O.PG(a["poses0"], a["edge_i"], a["edge_j"], a["meas"], a["node_fixed"]).evaluate()
    want = direct_residual(g, pr)
    print(f"{gname}: oracle's r on the augmented edges against se3_log(Z^-1 T): max |difference| {np.abs(r[m:] - want).max():.2e}")
    assert np.abs(r[m:] - want).max() <= 1e-13
    assert np.all(Ji[m:] == 0.0)                                    # the virtual end: exactly 0
    fx = g["node_fixed"][pr["nodes"]] != 0
    assert fx.any() and np.all(Jj[m:][fx] == 0.0) and np.all(np.abs(Jj[m:][~fx]).max(axis=(1, 2)) > 0.5)
    # the graph's own edges are untouched by the augmentation
    _, r0, Ji0, Jj0 = O.PG(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"]).evaluate()
    assert np.array_equal(r[:m], r0) and np.array_equal(Ji[:m], Ji0) and np.array_equal(Jj[:m], Jj0)
    # and lm_step_ref's problem on the augmented graph gives the same rows
    prob = Q.problem(g, pr)
    rw, Jw, _ = prob.lin(prob.x0)
    assert np.abs(rw[m:] - P.whiten(pr["W"], want)).max() <= 1e-12


def test_whitened_prior_matches_50_digits():
    """a handful of priors: W r and W Jr^-1 (the series truncated after ad^2, as the engine builds it) against mp_ref with T_i = I, to the
    1e-13 relative that tests/test_lm_step_reference.py holds the edges to"""
    g, pr = Q.graph("n60"), Q.priors("n60", "few")
    prob = Q.problem(g, pr)
    m = len(g["edge_i"])
    rw, Jw, _ = prob.lin(prob.x0)
    worst = 0.0
    for k in range(len(pr["nodes"])):
        rm, Jim, Jjm = M.pg_jacobians_build(M.pose(Q.IDENTITY), M.pose(g["poses0"][pr["nodes"][k]]), M.pose(pr["poses"][k]))
        Wm = mp.matrix(pr["W"][k].tolist())
        r50 = np.array([float(v) for v in Wm * mp.matrix([rm[a] for a in range(6)])])
        J50 = np.array((Wm * Jjm).tolist(), dtype=float)
        er = np.linalg.norm(rw[m + k] - r50) / max(np.linalg.norm(r50), 1.0)
        eJ = np.linalg.norm(Jw[m + k][:, 6:] - J50) / np.linalg.norm(J50)
        worst = max(worst, er, eJ)
    print(f"whitened priors against 50 digits: worst relative error {worst:.2e}")
    assert worst <= 1e-13 * 10.0          # (cond(W) <= 10 of the "few" set multiplies the edges' 1e-13)


def singular_values(gname, kind):
    g, pr = Q.graph(gname), Q.priors(gname, kind)
    return np.linalg.svd(Q.jacobian(g, pr), compute_uv=False)


@pytest.mark.parametrize("gname,kind", [("n60_free", "few"), ("n60_free", "dense"), ("n60_free", "three_pos"), ("n60_free", "gps"),
                                        ("n60", "few"), ("n40_pad", "many"), ("n40_pad", "gps"), ("n150", "few")])
def test_prior_sets_condition_the_problem(gname, kind):
    s = singular_values(gname, kind)
    print(f"{gname} {kind}: cond(J) = {s[0] / s[-1]:.1f} ({len(s)} columns)")
    assert s[0] / s[-1] <= 1e3


def test_a_single_position_prior_leaves_the_rotation_free():
    for gname in ("n60_free", "chain12"):
        s = singular_values(gname, "single_pos")
        small = int(np.sum(s < 1e-10 * s[0]))
        print(f"{gname} single_pos: singular values {s[-4:]} of sigma_max {s[0]:.2f}: {small} below 1e-10 sigma_max")
        assert small == 3


def test_many_has_the_shape_the_kernels_need():
    pr = Q.priors("n40_pad", "many")
    nodes = pr["nodes"]
    assert len(nodes) > Q.PRIORS_PER_WORKGROUP and len(np.unique(nodes)) == 40 > Q.NODES_PER_WORKGROUP
    assert nodes[Q.PRIORS_PER_WORKGROUP - 1] == nodes[Q.PRIORS_PER_WORKGROUP]          # a node's priors straddle the workgroup boundary
    pr = Q.priors("n150", "few")
    assert pr["nodes"].min() < 128 < pr["nodes"].max()                                 # both workgroups of the 128-node kernels
    pr = Q.priors("n60", "few")
    assert np.sum(pr["nodes"] == 3) == 2 and 30 in pr["nodes"] and 0 in pr["nodes"]


@pytest.mark.parametrize("gname,kind", [("n60", "few"), ("n60_free", "few"), ("n40_pad", "many"), ("n150", "few"), ("n40_pad", "gps"), ("n60", "dense")])
def test_reference_steps_are_an_accuracy_case(gname, kind):
    """the three iterations the GPU step test compares: conditioning and decisions far from the threshold, as for the edges' cases"""
    o = L.lm_options(**Q.LM_OPTIONS)
    ref = Q.reference(gname, kind, 3)
    kap = max(it["kappa"] for it in ref)
    print(f"{gname} {kind}: kappa {kap:.2e}, cost {ref[0]['start']['cost']:.4e} -> {ref[-1]['cost']:.4e}")
    assert L.C_PATH["pg"] * kap * max(L.EPS, L.PCG_TOL) <= 1e-6 and L.rho_margin_ok(ref, o)
    d = Q.drop_virtual(ref)
    assert len(d[-1]["x"]) == len(ref[-1]["x"]) - 7 and np.all(ref[-1]["delta"][-6:] == 0) and np.array_equal(ref[-1]["x"][-7:], Q.IDENTITY)


# ------------------------------------------------------------------------------- the Python layer, no device
def test_engine_checks_prior_arguments_before_any_device_work():
    st = importlib.import_module("slam-tricks_amd")
    for name in ("stba_pg_set_priors", "stba_pg_prior_count", "stba_pg_evaluate_priors", "stba_pg_prior_kernel_geometry"):
        assert name in st.EXPORTS and hasattr(st.lib(), name)
    assert st.lib().stba_pg_set_priors(None, 0, None, None, None, None) == -1          # STBA_ERR_INVALID_ARGUMENT: a null engine
    assert st.lib().stba_pg_prior_count(None, None) == -1 and st.lib().stba_pg_evaluate_priors(None, None, None, None) == -1
    assert st.lib().stba_pg_prior_kernel_geometry(None, None, None) == -1
