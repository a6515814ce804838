"""ceres::Covariance on a 1000-pose graph (6000 local parameters) through include/stba/ceres.h: the "gpu-pg" route, where the dense
route stops at 4096 local parameters.  The tangent blocks must be the C ABI's, the ambient blocks J_a C J_b^T with J the chart's
Jacobian -- multiplied here, and the chart's Jacobian itself held against central differences of the oracle's retraction."""
import importlib
import subprocess

import numpy as np
import pytest

from test_pg_covariance_shim import build_exe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory)


def test_thousand_pose_graph_takes_the_pose_graph_route(exe, O, scenes, tmp_path):
    st = importlib.import_module("slam-tricks_amd")
    s = scenes.pose_graph_scene(n_nodes=1000, loops_per_node=3, seed=21, turns=8)
    s["node_fixed"][[0, 400, 800]] = 1
    pairs = [(1, 1), (250, 250), (250, 251), (251, 250), (999, 999), (999, 5), (400, 3), (7, 800)]
    n, m = len(s["poses0"]), len(s["edge_i"])
    path = tmp_path / "graph.txt"
    with open(path, "w") as f:
        f.write(f"{n} {m} {len(pairs)}\n")
        np.savetxt(f, s["poses0"], fmt="%.17g")
        np.savetxt(f, s["node_fixed"][None], fmt="%d")
        np.savetxt(f, np.stack([s["edge_i"], s["edge_j"]], 1), fmt="%d")
        np.savetxt(f, s["meas"], fmt="%.17g")
        np.savetxt(f, np.array(pairs), fmt="%d")
    p = subprocess.run([exe, "device", str(path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "device ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "path gpu-pg" in p.stdout
    rows = {"T": {}, "A": {}, "Ja": {}, "Jb": {}}
    for line in p.stdout.splitlines():
        w = line.split()
        if w and w[0] in rows:
            rows[w[0]][int(w[1])] = np.array([float(x) for x in w[2:]])
    e = st.PGEngine(s["poses0"], s["edge_i"], s["edge_j"], s["meas"], s["node_fixed"])
    C, summ = e.covariance(pairs)
    print(summ)
    for k, (a, b) in enumerate(pairs):
        T = rows["T"][k].reshape(6, 6)
        assert np.array_equal(T, C[k]), (a, b)                       # the same computation: the same bits
        Ja, Jb = rows["Ja"][k].reshape(7, 6), rows["Jb"][k].reshape(7, 6)
        for J, node in ((Ja, a), (Jb, b)):                           # d (T exp(delta)) / d delta at 0, central differences, h = 1e-6
            Jn = np.zeros((7, 6))
            for q in range(6):
                d = np.zeros(6); d[q] = 1e-6
                Jn[:, q] = (O.se3_retract(s["poses0"][node], d) - O.se3_retract(s["poses0"][node], -d)) / 2e-6
            assert np.abs(J - Jn).max() <= 1e-8 * max(1.0, np.abs(Jn).max())
        A = rows["A"][k].reshape(7, 7)
        ref = Ja @ C[k] @ Jb.T
        assert np.abs(A - ref).max() <= 1e-14 * max(1.0, np.abs(Ja).max() * np.abs(Jb).max()) * max(np.abs(C[k]).max(), 1e-300) * 36
    assert np.all(C[6] == 0) and np.all(C[7] == 0)                   # constant blocks give zero blocks
