"""A pose graph with robust losses through include/stba/ceres.h on the device (tests/cpp/test_pg_loss_shim.cpp), the 60-node graph of
tests/pg_information_ref.py:
  * ceres::Solve with HuberLoss on the loop closures takes "gpu-pg" and ends at the C ABI's result for the same table (PGEngine with
    loss=, the same options: the same computation, so the same bits); its initial cost is the robust reference's 1/2 sum rho;
  * the same with ScaledLoss(CauchyLoss(0.5), 2) on the loops and ScaledLoss(nullptr, 0.5) on every fourth odometry edge;
  * ceres::Covariance at the solution takes "gpu-pg" and returns (J'^T J')^-1: the bits of PGEngine.covariance at the same poses."""
import importlib
import subprocess

import numpy as np
import pytest

import pg_information_ref as P
import pg_loss_ref as R
from test_pg_loss_shim import build_exe

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (29, 29), (29, 31), (31, 29), (59, 59), (59, 3), (0, 5), (7, 30)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory)


def run_device(exe, tmp_path, g, rows):
    """rows: m x (kind | -1, a, b, scale) as the driver reads them.  Returns (summary words, poses, tangent blocks)"""
    n, m = len(g["poses0"]), len(g["edge_i"])
    path = tmp_path / "graph.txt"
    with open(path, "w") as f:
        f.write(f"{n} {m} {len(PAIRS)}\n")
        np.savetxt(f, g["poses0"], fmt="%.17g")
        np.savetxt(f, g["node_fixed"][None], fmt="%d")
        np.savetxt(f, np.stack([g["edge_i"], g["edge_j"]], 1), fmt="%d")
        np.savetxt(f, g["meas"], fmt="%.17g")
        for k, a, b, s in rows:
            f.write(f"{int(k)} {float(a)!r} {float(b)!r} {float(s)!r}\n")
        np.savetxt(f, np.array(PAIRS), fmt="%d")
    p = subprocess.run([exe, "device", str(path)], capture_output=True, text=True, timeout=600)
    lines = p.stdout.splitlines()
    short = "\n".join(ln[:300] for ln in lines if not ln.startswith("T "))
    assert p.returncode == 0 and "device ok" in p.stdout, short + p.stderr[-2000:]
    out, T = {}, {}
    for line in lines:
        w = line.split()
        if w and w[0] == "T":
            T[int(w[1])] = np.array([float(x) for x in w[2:]]).reshape(6, 6)
        elif w and w[0] == "pg_poses":
            out["poses"] = np.array([float(x) for x in w[1:]]).reshape(-1, 7)
        elif w:
            out[w[0]] = w[1:]
    assert out["pg"][1] == "gpu-pg" and out["cov"][1] == "gpu-pg"
    return out, out["poses"], T


def check_against_the_c_abi(st, g, table, out, poses, T, label, covariance_differs):
    m = len(g["edge_i"])
    init, final, iters = float(out["pg"][7]), float(out["pg"][9]), int(out["pg"][5])
    prob = R.RobustPGProblem(g, np.tile(np.eye(6), (m, 1, 1)), table)
    c0 = prob.cost(prob.x0)
    e = st.PGEngine(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"], loss=dict(table))
    summ, _, _ = e.solve(function_tolerance=1e-12, parameter_tolerance=1e-11)
    print(f"{label}: ceres.h {init:.12e} -> {final:.12e} ({iters} iterations); C ABI {summ.initial_cost:.12e} -> {summ.final_cost:.12e} "
          f"({summ.num_iterations}); reference initial cost {c0:.12e}")
    assert abs(init - c0) <= 1e-12 * c0 and final < 0.5 * init
    assert summ.termination_type == 0 and summ.num_iterations == iters and summ.final_cost == final
    assert np.array_equal(e.get_poses().reshape(-1, 7), poses)
    assert np.all(poses[0] == g["poses0"][0]) and np.all(poses[30] == g["poses0"][30])
    f = st.PGEngine(poses, g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"], loss=dict(table))
    C, _ = f.covariance(PAIRS)
    lossless, _ = st.PGEngine(poses, g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"]).covariance(PAIRS[:1])
    for k in range(len(PAIRS)):
        assert np.array_equal(T[k], C[k]), PAIRS[k]
    far = np.linalg.norm(T[0] - lossless[0]) / np.linalg.norm(lossless[0])
    print(f"  covariance of node 1 against the lossless one at the same poses: relative difference {far:.2e}")
    if covariance_differs:
        assert far > 1e-3


def test_huber_on_the_loops_through_ceres_h(exe, tmp_path):
    st = importlib.import_module("slam-tricks_amd")
    g = P.graph("n60")
    table, _ = R.loss_set("n60", "huber")
    rows = [(k if k else -1, a, b, s) for k, a, b, s in zip(table["kind"], table["a"], table["b"], table["scale"])]      # odometry: no loss object
    out, poses, T = run_device(exe, tmp_path, g, rows)
    # (at the Huber solution every loop closure is an inlier, s <= a^2, so rho' = 1 and the covariance is the lossless one: printed only)
    check_against_the_c_abi(st, g, table, out, poses, T, "huber(0.5) on the loops", covariance_differs=False)


def test_scaled_cauchy_through_ceres_h(exe, tmp_path):
    st = importlib.import_module("slam-tricks_amd")
    g = P.graph("n60")
    m, n0 = len(g["edge_i"]), R.n_odometry(g)
    loop = np.arange(m) >= n0
    scaled_null = ~loop & (np.arange(m) % 4 == 0)
    table = dict(kind=np.where(loop, 3, 0).astype(np.int32), a=np.where(loop, 0.5, 1.0), b=np.ones(m),
                 scale=np.where(loop, 2.0, np.where(scaled_null, 0.5, 1.0)))
    # the driver makes ScaledLoss(CauchyLoss(0.5), 2) on the loops, ScaledLoss(nullptr, 0.5) for kind -1 with a scale, no loss otherwise
    rows = [((3 if loop[e] else -1), table["a"][e], 1.0, table["scale"][e]) for e in range(m)]
    out, poses, T = run_device(exe, tmp_path, g, rows)
    check_against_the_c_abi(st, g, table, out, poses, T, "ScaledLoss(CauchyLoss(0.5), 2) on the loops", covariance_differs=True)
