"""Solver::Options::linear_solver_type = ITERATIVE_SCHUR through include/stba/ceres.h, driven by tests/cpp/test_iterative_schur.cpp:
the st20 call site on "gpu-ba" and "gpu-ba-hostjac" for every preconditioner against the Python engine run with the same options;
linear_solver_type_used and every iteration's linear_solver_iterations filled; CLUSTER_JACOBI refused with the parameters untouched;
PnP ("gpu-dense-callback") bit-identical under ITERATIVE_SCHUR and DENSE_SCHUR."""
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

import lm_step_ref as L
from conftest import ROOT

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "cpp", "test_iterative_schur.cpp")
PKG = os.path.join(ROOT, "slam-tricks_amd")
DENSE_SCHUR, ITERATIVE_SCHUR = 3, 5                    # ceres.h LinearSolverType
PRECONDITIONERS = {"identity": 0, "jacobi": 1, "schur_jacobi": 2, "cluster_jacobi": 3}


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


@pytest.fixture(scope="module")
def exe(st, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "test_iterative_schur")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC,
                           "-L", PKG, "-lstba", f"-Wl,-rpath,{PKG}", "-o", out])
    return out


def run(exe, *args):
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = {"P": [], "stderr": p.stderr}
    for line in p.stdout.splitlines():
        w = line.split(" ", 1)
        if w[0] == "P":
            out["P"].append(line)
        else:
            out[w[0]] = w[1] if len(w) > 1 else ""
    return out


@pytest.fixture(scope="module")
def st20(tmp_path_factory):
    scenes = importlib.import_module("slam-tricks_amd.scenes")
    s = scenes.st20_scene(pix_noise=1e-3)
    path = str(tmp_path_factory.mktemp("scene") / "st20.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("iii", len(s["cams0"]), len(s["pts0"]), len(s["obs_cam"])))
        f.write(np.ascontiguousarray(s["cams0"], np.float64).tobytes())
        f.write(np.ascontiguousarray(s["pts0"], np.float64).tobytes())
        f.write(np.ascontiguousarray(s["obs_cam"], np.int32).tobytes())
        f.write(np.ascontiguousarray(s["obs_pt"], np.int32).tobytes())
        f.write(np.ascontiguousarray(s["obs_feat"], np.float64).tobytes())
        f.write(np.ascontiguousarray(s["cam_fixed"][:, 0], np.uint8).tobytes())
    return s, path


def end_point(out, nc):
    v = [np.array([float(x) for x in line.split()[1:]]) for line in out["P"]]
    return np.array(v[:nc]), np.array(v[nc:])


@pytest.mark.parametrize("pc", ["identity", "jacobi", "schur_jacobi"])
@pytest.mark.parametrize("kind,expect", [(1, "gpu-ba"), (2, "gpu-ba-hostjac")])
def test_st20_call_site_matches_the_engine(st, exe, st20, kind, expect, pc):
    s, path = st20
    out = run(exe, "ba", path, kind, PRECONDITIONERS[pc])
    assert out["path"] == expect and out["termination"] == "0", out
    assert int(out["used"]) == ITERATIVE_SCHUR
    n_it = int(out["iterations"])
    lin = [int(x) for x in out["linear"].split()]
    assert len(lin) == n_it + 1 and lin[0] == 0 and all(k >= 1 for k in lin[1:]), lin
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], linear_solver="iterative_schur")
    prob = L.ba_problem(dict(s, pt_fixed=None))
    if kind == 2:
        e.set_host_linearizer(lambda cams, pts, want: prob.lin_obs(cams.copy(), pts.copy(), want))
    e.set_pcg(pc, eta=0.1, min_iterations=0, max_iterations=500)
    summ, _ = e.solve(st.default_options(max_num_iterations=100))
    cams, pts = e.get_params()
    c_cpp, p_cpp = end_point(out, len(cams))
    dq = np.minimum(np.abs(c_cpp[:, :4] - cams[:, :4]).max(1), np.abs(c_cpp[:, :4] + cams[:, :4]).max(1)).max()
    dt, dl = np.abs(c_cpp[:, 4:] - cams[:, 4:]).max(), np.abs(p_cpp - pts).max()
    print(f"{expect} {pc}: {n_it} LM iterations (engine {summ.num_iterations}), PCG {lin[1:]} (engine {list(e.pcg_iterations(summ.num_iterations))}), "
          f"end point against the engine: dq {dq:.2e} dt {dt:.2e} dL {dl:.2e}")
    # (measured: the same LM and PCG iteration counts on both paths, end points within 1e-14 of the engine's)
    assert n_it == summ.num_iterations and lin[1:] == list(e.pcg_iterations(summ.num_iterations))
    assert max(dq, dt, dl) <= 1e-11


@pytest.mark.parametrize("kind", [1, 2])
def test_cluster_jacobi_is_refused(exe, st20, kind):
    _, path = st20
    out = run(exe, "ba", path, kind, PRECONDITIONERS["cluster_jacobi"])
    assert out["termination"] == "2" and out["moved"] == "0", out          # FAILURE, parameters untouched
    assert "CLUSTER_JACOBI" in out["message"] and "CLUSTER_JACOBI" in out["stderr"]
    assert int(out["used"]) == 0


def test_pnp_ignores_the_option(exe, tmp_path):
    scenes = importlib.import_module("slam-tricks_amd.scenes")
    s = scenes.pnp_scene()
    f = str(tmp_path / "pnp.bin")
    with open(f, "wb") as fh:
        fh.write(struct.pack("i", len(s["pts"])))
        fh.write(np.asarray(s["pose_init"], np.float64).tobytes())
        fh.write(np.ascontiguousarray(np.hstack([s["pts"], s["feats"]]), np.float64).tobytes())
    a = run(exe, "pnp", f, ITERATIVE_SCHUR)
    b = run(exe, "pnp", f, DENSE_SCHUR)
    assert a["path"] == b["path"] == "gpu-dense-callback"
    assert a["P"] == b["P"] and a["iterations"] == b["iterations"] and a["termination"] == b["termination"] == "0"
    assert int(a["used"]) == 0 and set(a["linear"].split()) == {"0"}
