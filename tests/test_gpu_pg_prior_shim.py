"""A pose graph with node pose priors through include/stba/ceres.h on the device (tests/cpp/test_pg_prior_shim.cpp), the 60-node graph
of tests/pg_prior_ref.py with NO constant node and the prior set "few" (two of the six priors made without a W):
  * ceres::Solve takes "gpu-pg" and, with force_callback_path, "gpu-dense-callback" (the factor's own operator() and autodiff); both
    start at the whitened oracle's cost of the augmented graph and end at the same cost and poses -- to the tolerance
    tests/test_gpu_pg_information_shim.py holds this pair of routes to (final cost 1e-6 relative, poses 1e-5) -- and gpu-pg ends at
    the C ABI's own answer (PGEngine with the same priors, to the same tolerance; whether the bits agree is printed);
  * ceres::Covariance on this graph, which no constant node anchors, takes "gpu-pg"; its blocks and PGEngine.covariance's at the same
    poses are both within pg_covariance_ref.block_bound of the augmented graph's dense inverse (the front door numbers the nodes in
    the order the residual blocks name them, so the two engines do not sum in the same order: their difference is printed);
  * NodePosePriorFactor::Evaluate on the host, composed with SE3RightPlus, against PGEngine.evaluate_priors: r to the evaluate bound
    (pg_information_ref.whiten_bound, base 1e-12); J to that bound (base 1e-11) plus sum_k |W_ak| T(r), T the remainder of Jr^-1 behind
    the ad^2 term (mp_ref.jr_inv_remainder_bound): the host differentiates the logarithm, the engine builds the truncated series."""
import importlib
import subprocess

import numpy as np
import pytest

import mp_ref as M
import pg_covariance_ref as R
import pg_information_ref as P
import pg_prior_ref as Q
from test_pg_prior_shim import build_exe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory)


def test_priors_through_the_front_door(exe, O, tmp_path):
    st = importlib.import_module("slam-tricks_amd")
    g, pr0 = Q.graph("n60_free"), Q.priors("n60_free", "few")
    n, m, k = len(g["poses0"]), len(g["edge_i"]), len(pr0["nodes"])
    flag = np.array([1, 1, 0, 1, 0, 1])
    pr = dict(pr0, W=np.where(flag[:, None, None] == 1, pr0["W"], np.eye(6)))
    pairs = [(3, 3), (17, 17), (3, 17), (17, 3), (59, 59), (0, 40)]
    path = tmp_path / "graph.txt"
    with open(path, "w") as f:
        f.write(f"{n} {m} {k} {len(pairs)}\n")
        np.savetxt(f, g["poses0"], fmt="%.17g")
        np.savetxt(f, g["node_fixed"][None], fmt="%d")
        np.savetxt(f, np.stack([g["edge_i"], g["edge_j"]], 1), fmt="%d")
        np.savetxt(f, g["meas"], fmt="%.17g")
        np.savetxt(f, pr["nodes"][None], fmt="%d")
        np.savetxt(f, pr["poses"], fmt="%.17g")
        np.savetxt(f, flag[None], fmt="%d")
        np.savetxt(f, pr["W"].reshape(k, 36), fmt="%.17g")
        np.savetxt(f, np.array(pairs), fmt="%d")
    p = subprocess.run([exe, "device", str(path)], capture_output=True, text=True, timeout=600)
    lines = p.stdout.splitlines()
    short = "\n".join(ln[:300] for ln in lines if not ln.startswith(("T ", "P ")))
    assert p.returncode == 0 and "device ok" in p.stdout, short + p.stderr[-2000:]
    out, T, Pr = {}, {}, {}
    for line in lines:
        w = line.split()
        if w and w[0] == "T":
            T[int(w[1])] = np.array([float(x) for x in w[2:]]).reshape(6, 6)
        elif w and w[0] == "P":
            v = np.array([float(x) for x in w[2:]])
            Pr[int(w[1])] = (v[:6], v[6:].reshape(6, 6))
        elif w and w[0] in ("pg_poses", "dense_poses"):
            out[w[0]] = np.array([float(x) for x in w[1:]]).reshape(-1, 7)
        elif w:
            out[w[0]] = w[1:]
    assert out["pg"][1] == "gpu-pg" and out["dense"][1] == "gpu-dense-callback" and out["cov"][1] == "gpu-pg"
    ipg, fpg, ide, fde = float(out["pg"][7]), float(out["pg"][9]), float(out["dense"][7]), float(out["dense"][9])
    a, b = out["pg_poses"], out["dense_poses"]
    dq = np.minimum(np.abs(a[:, :4] - b[:, :4]).max(1), np.abs(a[:, :4] + b[:, :4]).max(1)).max()
    dt = np.abs(a[:, 4:] - b[:, 4:]).max()
    print(f"gpu-pg {ipg:.12e} -> {fpg:.12e} ({out['pg'][5]} iterations), gpu-dense-callback {ide:.12e} -> {fde:.12e} ({out['dense'][5]}); "
          f"final cost gap {abs(fpg - fde) / fde:.2e}, poses dq {dq:.2e} dt {dt:.2e}")
    # the cost of the sum: both routes start at the whitened oracle's cost of the augmented graph
    aug = Q.augment(g, pr)
    _, ro, _, Jjo = O.PG(aug["poses0"], aug["edge_i"], aug["edge_j"], aug["meas"], aug["node_fixed"]).evaluate()
    c0 = float(0.5 * np.sum(P.whiten(Q.augmented_weights(g, pr), ro).astype(np.longdouble) ** 2))
    assert abs(ipg - c0) <= 1e-12 * c0 and abs(ide - c0) <= 1e-12 * c0
    assert fpg < 0.5 * c0 and abs(fpg - fde) <= 1e-6 * fde and dq < 1e-5 and dt < 1e-5
    # ---- the front door reaches the C ABI's answer (the priors in the order the driver adds them: odd ones first)
    order = np.array([1, 3, 5, 0, 2, 4])
    kw = {name: v[order] for name, v in Q.engine_kwargs(pr).items()}
    e = st.PGEngine(g["poses0"], g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"], priors=kw)
    cp, r_dev, J_dev = e.evaluate_priors()
    r_dev, J_dev = r_dev[np.argsort(order)], J_dev[np.argsort(order)]
    s, _, _ = e.solve(function_tolerance=1e-12, parameter_tolerance=1e-11)
    x = e.get_poses()
    print(f"  C ABI {s.final_cost:.17g} front door {fpg:.17g}; the same bits: cost {s.final_cost == fpg}, poses {np.array_equal(x, a)}")
    assert abs(s.final_cost - fpg) <= 1e-6 * fpg and np.abs(x - a).max() < 1e-5          # (the bound of the pair of routes above)
    e.close()
    # ---- the factor's own Evaluate against the device's
    worst = 0.0
    for q in range(k):
        r_host, J_host = Pr[q]
        W = pr["W"][q]
        tail = float(M.jr_inv_remainder_bound(ro[m + q]))
        br = P.whiten_bound(W[None], ro[m + q][None], 1e-12)[0]
        bJ = P.whiten_bound(W[None], Jjo[m + q][None], 1e-11)[0] + np.abs(W).sum(1)[:, None] * tail
        worst = max(worst, (np.abs(r_host - r_dev[q]) / br).max(), (np.abs(J_host - J_dev[q]) / bJ).max())
        print(f"  prior {q}: |r_host - r_dev| {np.abs(r_host - r_dev[q]).max():.2e}, |J_host - J_dev| {np.abs(J_host - J_dev[q]).max():.2e} "
              f"(series remainder {tail:.2e})")
    assert worst <= 1.0
    # ---- covariance at the gpu-pg solution: the engine's bits, and the augmented graph's dense inverse
    e = st.PGEngine(a, g["edge_i"], g["edge_j"], g["meas"], g["node_fixed"], priors=kw)
    C, summ = e.covariance(pairs)
    e.close()
    J = P.whitened_jacobian(O, dict(aug, poses0=np.vstack([a, Q.IDENTITY])), Q.augmented_weights(g, pr))
    Cs, lam_min, kappa = R.dense_covariance((J.T @ J).tocsc(), aug["node_fixed"])
    bound = R.block_bound(summ["max_relative_residual"], kappa, lam_min)
    print(f"covariance: lambda_min {lam_min:.3e} kappa {kappa:.3e} rho {summ['max_relative_residual']:.3e} bound {bound:.3e}")
    # (the front door numbers the nodes in the order the residual blocks first name them -- here the odd priors' nodes first --, so
    # its engine sums in another order than the one made above: both are held to the dense inverse, the difference is printed)
    for q, (x, y) in enumerate(pairs):
        err, err_abi = np.linalg.norm(T[q] - R.block(Cs, x, y)), np.linalg.norm(C[q] - R.block(Cs, x, y))
        print(f"  C[{x},{y}] front door |err|_F {err:.3e} err / bound {err / bound:.3e}; C ABI {err_abi / bound:.3e}; "
              f"|front door - C ABI|_F {np.linalg.norm(T[q] - C[q]):.3e}")
        assert err <= bound and err_abi <= bound, (x, y, err, err_abi, bound)
