"""Camera-to-camera relative-pose factors through include/stba/ceres.h on the device (tests/cpp/test_ba_between_shim.cpp, its device
mode): the reference's BA call site (test_ceres.h:98-152 shape) with ceres::CameraRelativePoseFactor blocks on a chain of cameras and
ceres::PosePriorFactor on two of them instead of SetParameterBlockConstant -- no block is constant.  Solve takes "gpu-ba" and ends at
BAEngine.solve's final cost and parameters for the same edges and priors in every bit (the comparison of the other *_shim GPU tests:
the scene listed the way the shim numbers its cameras); ceres::Covariance on "gpu-ba" returns BAEngine.covariance's bits; the same
problem forced onto the callback path -- the factor's own Evaluate -- agrees to that path's existing tolerance (cost 1e-6 relative,
parameters 1e-8); ITERATIVE_SCHUR, DOGLEG and use_inner_iterations come back as FAILURE with the reason in the message and the
parameters untouched."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ba_between_ref as T
import ba_prior_ref as P
from test_gpu_ba_loss_shim import as_the_shim_numbers_it

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAILURE = 2
CASE = "c_chain_two_priors"


@pytest.fixture(scope="module")
def st():
    return importlib.import_module("slam-tricks_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    pkg = os.path.join(ROOT, "slam-tricks_amd")
    out = str(tmp_path_factory.mktemp("cpp") / "test_ba_between_shim")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_ba_between_shim.cpp"),
                           "-L", pkg, "-lstba", f"-Wl,-rpath,{pkg}", "-lpthread", "-o", out])
    return out


@pytest.fixture(scope="module")
def scene():
    """the case with nothing constant in the listing the shim numbers it by: (scene, priors dict, edges dict, camera of the covariance
    check), the weights as square roots"""
    c = T.case(CASE)
    assert c["cam_fixed"] is None and c["Wobs"] is None and c["table"] is None
    s, order, rank = as_the_shim_numbers_it(dict(c["s"], cam_fixed=np.zeros_like(c["s"]["cam_fixed"])))
    pr = c["priors"]
    priors = dict(cams=rank[pr["cams"]].astype(np.int32), poses=pr["poses"], sqrt_information=P.sqrt_of_information(pr["information"]))
    edges = dict(cam_i=rank[c["cam_i"]].astype(np.int32), cam_j=rank[c["cam_j"]].astype(np.int32), measurements=c["meas"],
                 sqrt_information=T.case_W(CASE))
    return s, priors, edges, int(rank[c["cam_i"][2]])


def run(exe, tmp_path, scene, mode):
    s, priors, edges, ccov = scene
    path = tmp_path / "scene.txt"
    row = lambda a: " ".join(repr(float(x)) for x in np.asarray(a).reshape(-1))
    with open(path, "w") as f:
        f.write(f"{len(s['cams0'])} {len(s['pts0'])} {len(s['obs_cam'])} {len(priors['cams'])} {len(edges['cam_i'])} {ccov}\n")
        np.savetxt(f, s["cams0"], fmt="%.17g")
        np.savetxt(f, s["pts0"], fmt="%.17g")
        for c, j, (fx, fy) in zip(s["obs_cam"], s["obs_pt"], s["obs_feat"]):
            f.write(f"{int(c)} {int(j)} {float(fx)!r} {float(fy)!r}\n")
        for c, pose, w in zip(priors["cams"], priors["poses"], priors["sqrt_information"]):
            f.write(f"{int(c)} {row(pose)} {row(w)}\n")
        for i, j, z, w in zip(edges["cam_i"], edges["cam_j"], edges["measurements"], edges["sqrt_information"]):
            f.write(f"{int(i)} {int(j)} {row(z)} {row(w)}\n")
    p = subprocess.run([exe, "device", str(path), mode], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "device ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    out = {}
    for line in p.stdout.splitlines():
        w = line.split()
        if w:
            out[w[0]] = w[1:]
    vec = lambda k: np.array([float(x) for x in out[k]])
    return out, vec


def test_edges_between_cameras_reach_the_c_abis_bits(st, exe, tmp_path, scene):
    s, priors, edges, ccov = scene
    out, vec = run(exe, tmp_path, scene, "lm")
    path, term, iters, init, final = out["ba"][0], int(out["ba"][1]), int(out["ba"][2]), float(out["ba"][3]), float(out["ba"][4])
    assert path == "gpu-ba" and term != FAILURE, (out["ba"], out.get("msg"))
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], None, pose_priors=priors, relative_poses=edges)
    summ, _ = e.solve()
    c0 = T.problem(CASE).cost(T.problem(CASE).x0)
    print(f"ceres.h {init:.12e} -> {final:.12e} ({iters} iterations); C ABI {summ.initial_cost:.12e} -> {summ.final_cost:.12e} "
          f"({summ.num_iterations}); reference initial cost {c0:.12e}")
    assert abs(init - c0) <= 1e-12 * c0 and final < 1e-2 * init
    assert summ.num_iterations == iters and summ.final_cost == final and summ.initial_cost == init
    ec, ep = e.get_params()
    assert np.array_equal(ec, vec("cams").reshape(-1, 7)) and np.array_equal(ep, vec("pts").reshape(-1, 3))
    # ceres::Covariance hands the edges and the priors to its engine too
    assert out["cov"] == ["gpu-ba", "1"], out["cov"]
    f = st.BAEngine(ec, ep, s["obs_cam"], s["obs_pt"], s["obs_feat"], None, pose_priors=priors, relative_poses=edges)
    Cv, _, _ = f.covariance(cam_pairs=[(ccov, ccov)], points=[0])
    assert np.array_equal(vec("R").reshape(3, 3), Cv[0][:3, :3]) and np.array_equal(vec("P").reshape(3, 3), Cv[0][3:, 3:])
    g = st.BAEngine(ec, ep, s["obs_cam"], s["obs_pt"], s["obs_feat"], None, pose_priors=priors)
    C0, _, _ = g.covariance(cam_pairs=[(ccov, ccov)], points=[0])
    assert not np.array_equal(C0[0], Cv[0])              # (the edges do count in it)
    # the callback path runs the factor's own Evaluate
    out2, vec2 = run(exe, tmp_path, scene, "callback")
    assert out2["ba"][0] not in ("gpu-ba", "none") and int(out2["ba"][1]) != FAILURE, (out2["ba"], out2.get("msg"))
    final2 = float(out2["ba"][4])
    c2, p2 = vec2("cams").reshape(-1, 7), vec2("pts").reshape(-1, 3)
    dq = np.minimum(np.abs(c2[:, :4] - ec[:, :4]).max(1), np.abs(c2[:, :4] + ec[:, :4]).max(1)).max()
    dt, dp = np.abs(c2[:, 4:] - ec[:, 4:]).max(), np.abs(p2 - ep).max()
    print(f"  callback path {out2['ba'][0]}: final {final2:.12e} ({out2['ba'][2]} iterations), relative {abs(final2 - final) / final:.2e}; "
          f"quaternions {dq:.2e} positions {dt:.2e} landmarks {dp:.2e} away")
    assert abs(final2 - final) <= 1e-6 * final and dq < 1e-8 and dt < 1e-8 and dp < 1e-8


@pytest.mark.parametrize("mode, word", [("iterative", "ITERATIVE_SCHUR"), ("dogleg", "DOGLEG"), ("inner", "inner iterations")])
def test_what_the_engine_refuses_with_edges_is_a_failure_here(exe, tmp_path, scene, mode, word):
    out, _ = run(exe, tmp_path, scene, mode)
    msg = " ".join(out.get("msg", []))
    print(out["ba"], msg)
    assert int(out["ba"][1]) == FAILURE and out["untouched"] == ["1"]
    assert word in msg and "relative pose" in msg
