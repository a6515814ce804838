"""A weighted pose graph through include/stba/ceres.h on the device (tests/cpp/test_pg_information_shim.cpp), the 60-node graph of
tests/pg_information_ref.py:
  * ceres::Solve on "gpu-pg" and, with force_callback_path, on "gpu-dense-callback" (the factor's own operator() and autodiff) end at
    the same cost and poses -- to the tolerance tests/test_cpp_shim.py holds this pair of routes to on the unweighted graph (each
    against the oracle: final cost 1e-6 relative, poses 1e-5).  Twice: every factor with the W of weight set "dense", and a mixed
    problem -- the general W of set "sqrt" on two edges out of three, no W on the rest;
  * ceres::Covariance on the "dense" problem takes "gpu-pg" and returns (J^T Omega J)^-1: the bits of PGEngine.covariance at the same
    poses, and within pg_covariance_ref.block_bound of the dense inverse of the whitened oracle Jacobian's normal matrix (the check
    of tests/test_gpu_pg_information.py's covariance test, at the solution).
(The mixed problem asks for no covariance: its normal matrix mixes edges of weight 1 with edges of weight up to 1e4, and the block-Jacobi
conjugate gradient of stba_pg_covariance stops at its cap of 348 iterations with a true residual of 6e-3 -- refused with that message,
DESIGN.md 7f.)"""
import importlib
import subprocess

import numpy as np
import pytest

import pg_covariance_ref as R
import pg_information_ref as P
from test_pg_information_shim import build_exe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory)


def run_device(exe, O, tmp_path, g, W, flag, pairs):
    """writes the graph, runs the driver; returns (poses of gpu-pg, poses of the dense route, tangent blocks) after the checks both
    problems share"""
    n, m = len(g["poses0"]), len(g["edge_i"])
    Wmix = np.where(flag[:, None, None] == 1, W, np.eye(6))
    path = tmp_path / f"graph_{int(flag.sum())}.txt"
    with open(path, "w") as f:
        f.write(f"{n} {m} {len(pairs)}\n")
        np.savetxt(f, g["poses0"], fmt="%.17g")
        np.savetxt(f, g["node_fixed"][None], fmt="%d")
        np.savetxt(f, np.stack([g["edge_i"], g["edge_j"]], 1), fmt="%d")
        np.savetxt(f, g["meas"], fmt="%.17g")
        np.savetxt(f, flag[None], fmt="%d")
        np.savetxt(f, W.reshape(m, 36), fmt="%.17g")
        if pairs:
            np.savetxt(f, np.array(pairs), fmt="%d")
    p = subprocess.run([exe, "device", str(path)], capture_output=True, text=True, timeout=600)
    lines = p.stdout.splitlines()
    short = "\n".join(ln[:300] for ln in lines if not ln.startswith("T "))
    assert p.returncode == 0 and "device ok" in p.stdout, short + p.stderr[-2000:]
    out, T = {}, {}
    for line in lines:
        w = line.split()
        if w and w[0] == "T":
            T[int(w[1])] = np.array([float(x) for x in w[2:]]).reshape(6, 6)
        elif w and w[0] in ("pg_poses", "dense_poses"):
            out[w[0]] = np.array([float(x) for x in w[1:]]).reshape(-1, 7)
        elif w:
            out[w[0]] = w[1:]
    assert out["pg"][1] == "gpu-pg" and out["dense"][1] == "gpu-dense-callback" and out["cov"][1] == "gpu-pg"
    ipg, fpg, ide, fde = float(out["pg"][7]), float(out["pg"][9]), float(out["dense"][7]), float(out["dense"][9])
    a, b = out["pg_poses"], out["dense_poses"]
    dq = np.minimum(np.abs(a[:, :4] - b[:, :4]).max(1), np.abs(a[:, :4] + b[:, :4]).max(1)).max()
    dt = np.abs(a[:, 4:] - b[:, 4:]).max()
    print(f"{int(flag.sum())} of {m} factors weighted: gpu-pg {ipg:.12e} -> {fpg:.12e} ({out['pg'][5]} iterations), gpu-dense-callback "
          f"{ide:.12e} -> {fde:.12e} ({out['dense'][5]}); final cost gap {abs(fpg - fde) / fde:.2e}, poses dq {dq:.2e} dt {dt:.2e}")
    # the weighted cost, not the unweighted one: the initial cost of both routes is the whitened oracle's
    ro = O.PG(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"]).evaluate(jac=False)[1]
    c0 = float(0.5 * np.sum(P.whiten(Wmix, ro).astype(np.longdouble) ** 2))
    assert abs(ipg - c0) <= 1e-12 * c0 and abs(ide - c0) <= 1e-12 * c0
    assert fpg < 0.5 * c0
    assert abs(fpg - fde) <= 1e-6 * fde and dq < 1e-5 and dt < 1e-5
    assert np.all(a[0] == g["poses0"][0]) and np.all(b[30] == g["poses0"][30])
    return a, b, T


def test_mixed_factors_on_both_routes(exe, O, tmp_path):
    g = P.graph("n60")
    m = len(g["edge_i"])
    run_device(exe, O, tmp_path, g, P.weights("n60", "sqrt")[1], (np.arange(m) % 3 != 2).astype(int), [])


def test_weighted_graph_on_both_routes_and_its_covariance(exe, O, tmp_path):
    st = importlib.import_module("slam-tricks_amd")
    g = P.graph("n60")
    m = len(g["edge_i"])
    _, W = P.weights("n60", "dense")
    pairs = [(1, 1), (29, 29), (29, 31), (31, 29), (59, 59), (59, 3), (0, 5), (7, 30)]
    a, _, T = run_device(exe, O, tmp_path, g, W, np.ones(m, int), pairs)
    # covariance at the gpu-pg solution
    e = st.PGEngine(a, g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"], sqrt_information=W)
    C, summ = e.covariance(pairs)
    J = P.whitened_jacobian(O, dict(g, poses0=a), W)
    Cs, lam_min, kappa = R.dense_covariance((J.T @ J).tocsc(), g["node_fixed"])
    bound = R.block_bound(summ["max_relative_residual"], kappa, lam_min)
    print(f"covariance: lambda_min {lam_min:.3e} kappa {kappa:.3e} rho {summ['max_relative_residual']:.3e} bound {bound:.3e}")
    for k, (x, y) in enumerate(pairs):
        assert np.array_equal(T[k], C[k]), (x, y)                       # the same computation: the same bits
        err = np.linalg.norm(T[k] - R.block(Cs, x, y))
        print(f"  C[{x},{y}] |err|_F {err:.3e} err / bound {err / bound:.3e}")
        assert err <= bound, (x, y, err, bound)
