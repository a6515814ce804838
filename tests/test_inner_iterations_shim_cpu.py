"""Solver::Options::use_inner_iterations through include/stba/ceres.h, driven by tests/cpp/test_inner_iterations_shim.cpp: every
refusal comes before any device work -- FAILURE, the parameters untouched, the reason in Summary::message and on stderr -- so none
needs a device: DOGLEG, a non-independent ordering (a camera's rotation and position; a camera and the landmarks it observes), a
pointer that is not a parameter block, a negative tolerance, and the problems that take gpu-ba-hostjac, gpu-pg or gpu-dense-callback."""
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE_SCHUR, ITERATIVE_SCHUR = 3, 5                # LinearSolverType (include/stba/ceres.h)
LEVENBERG_MARQUARDT, DOGLEG = 0, 1                 # TrustRegionStrategyType


@pytest.fixture(scope="module")
def inner_shim(tmp_path_factory):
    st = importlib.import_module("slam-tricks_amd")
    st.lib()
    scenes = importlib.import_module("slam-tricks_amd.scenes")
    d = tmp_path_factory.mktemp("inner_shim")
    exe = str(d / "test_inner_iterations_shim")
    pkg = os.path.join(ROOT, "slam-tricks_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_inner_iterations_shim.cpp"), "-L", pkg, "-lstba", f"-Wl,-rpath,{pkg}",
                           "-o", exe])
    s = scenes.st20_scene(pix_noise=1e-3)
    ba = str(d / "st20.bin")
    with open(ba, "wb") as f:
        f.write(struct.pack("iii", len(s["cams0"]), len(s["pts0"]), len(s["obs_cam"])))
        for a, t in ((s["cams0"], np.float64), (s["pts0"], np.float64), (s["obs_cam"], np.int32), (s["obs_pt"], np.int32),
                     (s["obs_feat"], np.float64), (s["cam_fixed"][:, 0], np.uint8)):
            f.write(np.ascontiguousarray(a, t).tobytes())
    p = scenes.pnp_scene()
    pnp = str(d / "pnp.bin")
    with open(pnp, "wb") as f:
        f.write(struct.pack("i", len(p["pts"])))
        f.write(np.asarray(p["pose_init"], np.float64).tobytes())
        f.write(np.ascontiguousarray(np.hstack([p["pts"], p["feats"]]), np.float64).tobytes())
    return exe, ba, pnp


def inner_shim_run(exe, *args):
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = {"stderr": p.stderr}
    for line in p.stdout.splitlines():
        w = line.split(" ", 1)
        if w[0] != "P":
            out[w[0]] = w[1] if len(w) > 1 else ""
    return out


def refused(out, what):
    assert out["termination"] == "2" and out["moved"] == "0" and out["iterations"] == "-1", out      # FAILURE, parameters untouched
    assert what in out["message"] and what in out["stderr"] and "nothing was solved" in out["message"], out
    assert out["inner_given"] == "1" and out["inner_used"] == "0"


@pytest.mark.parametrize("kind,strategy,ordering,solver,what", [
    (1, DOGLEG, 0, DENSE_SCHUR, "DOGLEG"),
    (1, LEVENBERG_MARQUARDT, 2, DENSE_SCHUR, "not an independent set (the rotation and the position of camera"),
    (1, LEVENBERG_MARQUARDT, 4, DENSE_SCHUR, "not an independent set (camera"),
    (1, LEVENBERG_MARQUARDT, 3, DENSE_SCHUR, "not a parameter block"),
    (1, LEVENBERG_MARQUARDT, 5, DENSE_SCHUR, "inner_iteration_tolerance"),
    (2, LEVENBERG_MARQUARDT, 0, DENSE_SCHUR, "gpu-ba-hostjac"),
    (2, LEVENBERG_MARQUARDT, 0, ITERATIVE_SCHUR, "gpu-ba-hostjac"),
])
def test_ceres_shim_refusals_on_ba(inner_shim, kind, strategy, ordering, solver, what):
    exe, ba, _ = inner_shim
    refused(inner_shim_run(exe, "ba", ba, kind, strategy, ordering, solver), what)


def test_ceres_shim_refuses_the_dense_callback_path(inner_shim):
    exe, _, pnp = inner_shim
    refused(inner_shim_run(exe, "pnp", pnp), "gpu-dense-callback")


def test_ceres_shim_refuses_a_pose_graph(inner_shim):
    exe, _, _ = inner_shim
    refused(inner_shim_run(exe, "pg"), "gpu-pg")
