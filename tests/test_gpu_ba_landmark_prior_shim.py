"""Landmark position priors through include/stba/ceres.h on the device (tests/cpp/test_ba_landmark_prior_shim.cpp, its device mode):
the reference's BA call site (test_ceres.h:98-152 shape) with ceres::LandmarkPriorFactor on four landmarks instead of
SetParameterBlockConstant -- no block is constant, the four control points hold the gauge (ba_landmark_prior_ref.gauge_case).
Solve takes "gpu-ba" and ends at BAEngine.solve's final cost and parameters for the same priors in every bit (the scene listed the
way the shim numbers its cameras); ceres::Covariance on "gpu-ba" returns BAEngine.covariance's bits; use_inner_iterations comes back
as FAILURE with the reason in the message and the parameters untouched.
The strategies -- default options, ITERATIVE_SCHUR, DOGLEG -- each report "gpu-ba" on that scene too.  Where they END is compared
on ba_landmark_prior_ref.pinned_case -- no constant dof, a tight prior on every landmark -- whose minimiser is sharp: costs that
agree to 1e-15 relative are at most 1.6e-9 apart there (tests/test_ba_landmark_prior_reference_cpu.py checks it; on the four-point
gauge scene, kappa 2e7, the same agreement in cost left ITERATIVE_SCHUR and DOGLEG 6e-8 and 4e-8 from the callback route, a
distance no stopping rule can see).  Each strategy is run to the minimiser (tolerances 1e-15) next to the dense callback route,
where the factor's own Evaluate runs, and ends within the existing prior shim test's distance of it: cost 1e-6 relative,
parameters 1e-8."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ba_landmark_prior_ref as R
from test_gpu_ba_loss_shim import as_the_shim_numbers_it

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAILURE = 2


@pytest.fixture(scope="module")
def st():
    return importlib.import_module("slam-tricks_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    pkg = os.path.join(ROOT, "slam-tricks_amd")
    out = str(tmp_path_factory.mktemp("cpp") / "test_ba_landmark_prior_shim")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_ba_landmark_prior_shim.cpp"), "-L", pkg, "-lstba", f"-Wl,-rpath,{pkg}", "-lpthread", "-o", out])
    return out


@pytest.fixture(scope="module")
def scene():
    """(scene in the listing the shim numbers it by, prior landmarks, positions, W, camera and landmark of the covariance check)"""
    s_caller, points, pos, W = R.gauge_case()
    s, order, rank = as_the_shim_numbers_it(dict(s_caller, cam_fixed=np.zeros_like(s_caller["cam_fixed"])))
    # (one more prior on the first control point: several on one landmark, not adjacent in the caller's order)
    points = np.concatenate([points, points[:1]]).astype(np.int32)
    pos = np.vstack([pos, pos[:1] + 0.01])
    W = np.concatenate([W, W[:1] * 0.5])
    return s, points, pos, W, 2, int(points[1])


@pytest.fixture(scope="module")
def pinned_scene():
    s_caller, points, pos, W = R.pinned_case()
    s, order, rank = as_the_shim_numbers_it(dict(s_caller, cam_fixed=np.zeros_like(s_caller["cam_fixed"])))
    return s, points, pos, W, 2, int(points[1])


def make_runs(exe, tmp_path_factory, scene):
    s, points, pos, W, ccov, pcov = scene
    path = tmp_path_factory.mktemp("lp_scene") / "scene.txt"
    with open(path, "w") as f:
        f.write(f"{len(s['cams0'])} {len(s['pts0'])} {len(s['obs_cam'])} {len(points)} {ccov} {pcov}\n")
        np.savetxt(f, s["cams0"], fmt="%.17g")
        np.savetxt(f, s["pts0"], fmt="%.17g")
        for c, j, (fx, fy) in zip(s["obs_cam"], s["obs_pt"], s["obs_feat"]):
            f.write(f"{int(c)} {int(j)} {float(fx)!r} {float(fy)!r}\n")
        for j, ph, w in zip(points, pos, W):
            f.write(f"{int(j)} " + " ".join(repr(float(x)) for x in ph) + " " + " ".join(repr(float(x)) for x in w.reshape(-1)) + "\n")
    cache = {}

    def run(mode):
        if mode not in cache:
            p = subprocess.run([exe, "device", str(path), mode], capture_output=True, text=True, timeout=300)
            assert p.returncode == 0 and "device ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
            out = {}
            for line in p.stdout.splitlines():
                w = line.split()
                if w:
                    out[w[0]] = w[1:]
            cache[mode] = (out, lambda k, out=out: np.array([float(x) for x in out[k]]))
        return cache[mode]
    return run


@pytest.fixture(scope="module")
def runs(exe, tmp_path_factory, scene):
    return make_runs(exe, tmp_path_factory, scene)


@pytest.fixture(scope="module")
def pinned_runs(exe, tmp_path_factory, pinned_scene):
    return make_runs(exe, tmp_path_factory, pinned_scene)


def test_default_options_reach_the_c_abis_bits(st, runs, scene):
    s, points, pos, W, ccov, pcov = scene
    out, vec = runs("lm")
    path, term, iters, init, final = out["ba"][0], int(out["ba"][1]), int(out["ba"][2]), float(out["ba"][3]), float(out["ba"][4])
    assert path == "gpu-ba" and term != FAILURE, (out["ba"], out.get("msg"))
    lp = dict(points=points, positions=pos, sqrt_information=W)
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], None, landmark_priors=lp)
    summ, _ = e.solve()
    prob = R.LandmarkPriorBAProblem(s, points, pos, W, cam_fixed=None)
    c0 = prob.cost(prob.x0)
    print(f"ceres.h {init:.12e} -> {final:.12e} ({iters} iterations); C ABI {summ.initial_cost:.12e} -> {summ.final_cost:.12e} "
          f"({summ.num_iterations}); reference initial cost {c0:.12e}")
    assert abs(init - c0) <= 1e-12 * c0 and final < 1e-3 * init
    assert summ.num_iterations == iters and summ.final_cost == final and summ.initial_cost == init
    ec, ep = e.get_params()
    assert np.array_equal(ec, vec("cams").reshape(-1, 7)) and np.array_equal(ep, vec("pts").reshape(-1, 3))
    # ceres::Covariance hands the priors to its engine too: without them this problem has no gauge
    assert out["cov"] == ["gpu-ba", "1"], out["cov"]
    f = st.BAEngine(ec, ep, s["obs_cam"], s["obs_pt"], s["obs_feat"], None, landmark_priors=lp)
    Cc, Cp, _ = f.covariance(cam_pairs=[(ccov, ccov)], points=[pcov])
    assert np.array_equal(vec("P").reshape(3, 3), Cc[0][3:, 3:]) and np.array_equal(vec("Q").reshape(3, 3), Cp[0])


@pytest.mark.parametrize("mode", ["lm", "iterative", "dogleg"])
def test_every_strategy_takes_gpu_ba_and_ends_where_the_callback_route_ends(runs, pinned_runs, mode):
    for r in (runs, pinned_runs):
        out0, _ = r(mode)
        assert out0["ba"][0] == "gpu-ba" and int(out0["ba"][1]) != FAILURE, (out0["ba"], out0.get("msg"))
    out, vec = pinned_runs(mode + "_tight")
    ref, rvec = pinned_runs("callback_tight")
    assert out["ba"][0] == "gpu-ba" and int(out["ba"][1]) != FAILURE, (out["ba"], out.get("msg"))
    assert ref["ba"][0] == "gpu-dense-callback" and int(ref["ba"][1]) != FAILURE, (ref["ba"], ref.get("msg"))
    final, final2 = float(out["ba"][4]), float(ref["ba"][4])
    c1, p1 = vec("cams").reshape(-1, 7), vec("pts").reshape(-1, 3)
    c2, p2 = rvec("cams").reshape(-1, 7), rvec("pts").reshape(-1, 3)
    dq = np.minimum(np.abs(c2[:, :4] - c1[:, :4]).max(1), np.abs(c2[:, :4] + c1[:, :4]).max(1)).max()
    dt, dp = np.abs(c2[:, 4:] - c1[:, 4:]).max(), np.abs(p2 - p1).max()
    print(f"LANDMARK PRIOR shim {mode}: {out0['ba'][2]} iterations at the default tolerances; to the minimiser {out['ba'][2]} iterations, "
          f"final {final:.12e}; callback route {ref['ba'][2]} iterations, final {final2:.12e}, relative {abs(final2 - final) / final:.2e}; "
          f"quaternions {dq:.2e} positions {dt:.2e} landmarks {dp:.2e} away; worst / 1e-8 {max(dq, dt, dp) / 1e-8:.3e}")
    assert abs(final2 - final) <= 1e-6 * final and dq < 1e-8 and dt < 1e-8 and dp < 1e-8


def test_inner_iterations_are_a_failure_here(runs):
    out, _ = runs("inner")
    msg = " ".join(out.get("msg", []))
    print(out["ba"], msg)
    assert int(out["ba"][1]) == FAILURE and out["untouched"] == ["1"]
    assert "inner iterations with LandmarkPriorFactor blocks are not implemented" in msg
