"""Information matrices through both front doors on the device.
include/stba/g2o.h (tests/cpp/test_g2o_information_shim.cpp): scene B with setInformation(w_k) per edge -- scalars, and a 2 x 2 type
of the caller's -- and RobustKernelHuber on the even edges ends at BAEngine's bits for the same information and table: iterations,
chi2() == 2 x the final cost, every estimate; setInformation(1.0) and identity matrices give the bits of the engine without weights;
a non-SPD Omega makes optimize() return 0 with the edge named and the estimates untouched.
include/stba/ceres.h (tests/cpp/test_ba_information_shim.cpp): scene B with ReprojectionFactor::Create(f, W) on every third block, with
and without HuberLoss (Solver::Options::bundle_adjustment_losses), takes "gpu-ba" and ends at BAEngine.solve's final cost and
parameters for the same weights in every bit (the cameras listed in the order the shim numbers them), ceres::Covariance at the solution
returns BAEngine.covariance's bits; the same problem forced onto the callback path (the factor's own Evaluate, which whitens itself)
agrees to that path's existing tolerance (tests/test_cpp_shim.py: cost 1e-6 relative, parameters 1e-8)."""
import importlib
import subprocess

import numpy as np
import pytest

import ba_information_ref as I
import ba_loss_ref as B
from test_ba_information_shim_cpu import build_ceres_exe, build_g2o_exe, g2o_information
from test_cpp_shim import run, vec, write_scene
from test_gpu_ba_loss_shim import CAM_PAIRS, LANDMARKS, as_the_shim_numbers_it

pytestmark = pytest.mark.gpu

ITERATIONS = 40
DELTA = 0.03


@pytest.fixture(scope="module")
def st():
    return importlib.import_module("slam-tricks_amd")


@pytest.fixture(scope="module")
def g2o_exe(tmp_path_factory):
    return build_g2o_exe(tmp_path_factory, stand_in=False)


@pytest.fixture(scope="module")
def ceres_exe(tmp_path_factory):
    return build_ceres_exe(tmp_path_factory)


# ------------------------------------------------------------------------------- g2o.h
def g2o_run(g2o_exe, tmp_path, s, mode, delta):
    f = str(tmp_path / "s.bin")
    write_scene(f, s)
    out = run(g2o_exe, f, mode, repr(delta), str(ITERATIONS))
    toks = out["g2o_iters"].split()
    return out, int(toks[0]), float(toks[2])


@pytest.mark.parametrize("mode", ["scalars", "matrices"])
def test_set_information_reaches_the_c_abis_bits(st, g2o_exe, tmp_path, mode):
    s = B.scene("B")
    n = len(s["obs_cam"])
    assert np.array_equal(s["cam_fixed"].any(1), s["cam_fixed"].all(1))
    out, iters, chi2 = g2o_run(g2o_exe, tmp_path, s, mode, DELTA)
    assert iters >= 1, out["g2o_iters"]
    Om = g2o_information(n, mode).reshape(n, 2, 2)
    on = np.arange(n) % 2 == 0
    table = dict(kind=np.where(on, st.LOSS_KINDS["huber"], 0).astype(np.int32), a=np.where(on, DELTA, 1.0))
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], information=Om, loss=table)
    summ, _ = e.solve(max_num_iterations=ITERATIONS)
    cams, pts = e.get_params()
    print(f"g2o {mode} + huber({DELTA}) on every even edge: {iters} iterations chi2 {chi2:.12e}; C ABI {summ.num_iterations} iterations "
          f"2 x cost {2 * summ.final_cost:.12e}")
    assert iters == summ.num_iterations and chi2 == 2.0 * summ.final_cost
    assert np.array_equal(vec(out, "g2o_cams").reshape(-1, 7), cams) and np.array_equal(vec(out, "g2o_pts").reshape(-1, 3), pts)
    # chi2 is sum rho(e^T Omega e) at the end point
    W = np.array([[float(x) for x in row] for row in I.chol2_mp(Om)]).reshape(n, 2, 2)
    prob = I.WeightedBAProblem(dict(s, pt_fixed=None), W, B.table_of(table["kind"], table["a"], 1.0, 1.0, n))
    ref_cost = prob.cost(np.concatenate([cams.reshape(-1), pts.reshape(-1)]))
    assert abs(2 * ref_cost - chi2) <= 1e-12 * chi2
    # (not the unweighted problem's)
    plain = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], loss=table)
    plain.solve(max_num_iterations=ITERATIONS)
    assert not np.array_equal(plain.get_params()[0], cams)


def test_identity_information_stays_the_engine_without_weights(st, g2o_exe, tmp_path):
    s = B.scene("B")
    out, iters, chi2 = g2o_run(g2o_exe, tmp_path, s, "identity", 0.0)
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
    summ, _ = e.solve(max_num_iterations=ITERATIONS)
    cams, pts = e.get_params()
    assert iters == summ.num_iterations and chi2 == 2.0 * summ.final_cost
    assert np.array_equal(vec(out, "g2o_cams").reshape(-1, 7), cams) and np.array_equal(vec(out, "g2o_pts").reshape(-1, 3), pts)


def test_an_information_matrix_that_is_not_positive_definite_is_refused(g2o_exe, tmp_path):
    s = B.scene("B")
    n = len(s["obs_cam"])
    out, iters, _ = g2o_run(g2o_exe, tmp_path, s, "notspd", DELTA)
    print(out["g2o_iters"])
    assert iters == 0 and f"edge {n // 2}:" in out["g2o_iters"] and "not positive definite" in out["g2o_iters"]
    assert np.array_equal(vec(out, "g2o_cams").reshape(-1, 7), s["cams0"]) and np.array_equal(vec(out, "g2o_pts").reshape(-1, 3), s["pts0"])


# ------------------------------------------------------------------------------- ceres.h
def ceres_run(exe, tmp_path, s, rows, W, weighted, callback=False):
    nc, np_, no = len(s["cams0"]), len(s["pts0"]), len(s["obs_cam"])
    fixed = s["cam_fixed"].all(1).astype(int)
    assert np.array_equal(s["cam_fixed"].any(1), s["cam_fixed"].all(1)) and not s["pt_fixed"].any()      # whole cameras only
    path = tmp_path / "scene.txt"
    with open(path, "w") as f:
        f.write(f"{nc} {np_} {no} {len(CAM_PAIRS)} {len(LANDMARKS)}\n")
        np.savetxt(f, s["cams0"], fmt="%.17g")
        np.savetxt(f, fixed[None], fmt="%d")
        np.savetxt(f, s["pts0"], fmt="%.17g")
        for c, j, (fx, fy) in zip(s["obs_cam"], s["obs_pt"], s["obs_feat"]):
            f.write(f"{int(c)} {int(j)} {float(fx)!r} {float(fy)!r}\n")
        for k, a, b, sc in rows:
            f.write(f"{int(k)} {float(a)!r} {float(b)!r} {float(sc)!r}\n")
        for on, w in zip(weighted, W.reshape(-1, 4)):
            f.write(f"{int(on)} " + " ".join(repr(float(x)) for x in w) + "\n")
        np.savetxt(f, np.array(CAM_PAIRS), fmt="%d")
        np.savetxt(f, np.array(LANDMARKS)[None], fmt="%d")
    p = subprocess.run([exe, "device", str(path)] + (["callback"] if callback else []), capture_output=True, text=True, timeout=600)
    lines = p.stdout.splitlines()
    short = "\n".join(ln[:300] for ln in lines if ln[:2] not in ("R ", "P ", "L "))
    assert p.returncode == 0 and "device ok" in p.stdout, short + p.stderr[-2000:]
    out, T = {}, {}
    for line in lines:
        w = line.split()
        if w and w[0] in ("R", "P", "L"):
            T[(w[0], int(w[1]))] = np.array([float(x) for x in w[2:]]).reshape(3, 3)
        elif w and w[0] in ("ba_cams", "ba_pts"):
            out[w[0]] = np.array([float(x) for x in w[1:]])
        elif w:
            out[w[0]] = w[1:]
    return out, out["ba_cams"].reshape(-1, 7), out["ba_pts"].reshape(-1, 3), T


@pytest.mark.parametrize("huber", [False, True])
def test_weighted_factors_through_ceres_h(st, ceres_exe, tmp_path, huber):
    s_caller = B.scene("B")
    n = len(s_caller["obs_cam"])
    weighted = np.arange(n) % 3 == 0
    W = np.where(weighted[:, None, None], I.scene_weights("B", "mild"), np.eye(2))
    table = B.loss_table("B", "huber", n) if huber else None
    rows = list(zip(table["kind"], table["a"], table["b"], table["scale"])) if huber else [(-1, 1.0, 1.0, 1.0)] * n
    out, cams_caller, pts, T = ceres_run(ceres_exe, tmp_path, s_caller, rows, W, weighted)
    assert out["ba"][1] == "gpu-ba" and out["cov"][1] == "gpu-ba", (out["ba"], out["cov"])
    init, final, iters = float(out["ba"][7]), float(out["ba"][9]), int(out["ba"][5])
    prob = I.WeightedBAProblem(s_caller, W, table)
    c0 = prob.cost(prob.x0)
    s, order, rank = as_the_shim_numbers_it(s_caller)
    cams = cams_caller[order]
    pairs = [(int(rank[a]), int(rank[b])) for a, b in CAM_PAIRS]
    kw = dict(sqrt_information=W, **({"loss": dict(table)} if huber else {}))
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"], **kw)
    summ, _ = e.solve()
    print(f"weighted every third block, huber={huber}: ceres.h {init:.12e} -> {final:.12e} ({iters} iterations); C ABI {summ.initial_cost:.12e} -> "
          f"{summ.final_cost:.12e} ({summ.num_iterations}); reference initial cost {c0:.12e}")
    assert abs(init - c0) <= 1e-12 * c0 and final < init
    assert summ.termination_type == 0 and summ.num_iterations == iters and summ.final_cost == final
    ec, ep = e.get_params()
    assert np.array_equal(ec, cams) and np.array_equal(ep, pts)
    f = st.BAEngine(cams, pts, s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"], **kw)
    C, P, _ = f.covariance(cam_pairs=pairs, points=LANDMARKS)
    for k in range(len(CAM_PAIRS)):
        assert np.array_equal(T[("R", k)], C[k][:3, :3]) and np.array_equal(T[("P", k)], C[k][3:, 3:]), CAM_PAIRS[k]
    for k in range(len(LANDMARKS)):
        assert np.array_equal(T[("L", k)], P[k]), LANDMARKS[k]
    # the unweighted engine ends elsewhere
    plain = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"],
                        **({"loss": dict(table)} if huber else {}))
    plain.solve()
    assert not np.array_equal(plain.get_params()[0], cams)
    if not huber:
        # the same problem on the callback path: the factor's own Evaluate whitens
        out2, cams2, pts2, _ = ceres_run(ceres_exe, tmp_path, s_caller, rows, W, weighted, callback=True)
        assert out2["ba"][1] != "gpu-ba", out2["ba"]
        final2 = float(out2["ba"][9])
        dq = np.minimum(np.abs(cams2[:, :4] - cams_caller[:, :4]).max(1), np.abs(cams2[:, :4] + cams_caller[:, :4]).max(1)).max()
        dt, dp = np.abs(cams2[:, 4:] - cams_caller[:, 4:]).max(), np.abs(pts2 - pts).max()
        print(f"  callback path {out2['ba'][1]}: final {final2:.12e} ({out2['ba'][5]} iterations), relative {abs(final2 - final) / final:.2e}; "
              f"quaternions {dq:.2e} positions {dt:.2e} landmarks {dp:.2e} away")
        assert abs(final2 - final) <= 1e-6 * final and dq < 1e-8 and dt < 1e-8 and dp < 1e-8
