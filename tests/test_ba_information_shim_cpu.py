"""Information matrices through the two front doors on the host.
include/stba/g2o.h (tests/cpp/test_g2o_information_shim.cpp compiled with g++ and -DSTBA_STAND_IN: the driver itself defines the C ABI
functions the header calls and records what they are given -- no library, no device): setInformation(1.0) and an identity matrix
produce no table (stba_ba_set_information is not called), a scalar 4.0 and a 2 x 2 type of the caller's with operator()(i, j) produce
the expected n_obs x 4 array, before stba_ba_set_loss.
include/stba/ceres.h (tests/cpp/test_ba_information_shim.cpp against the header and the library, host mode): the factory and
sqrt_information(), the self-whitening Evaluate, the W gathered next to the features, inner iterations refused before any device work."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ba_loss_ref as B
from conftest import ROOT
from test_cpp_shim import run, vec, write_scene

PKG = os.path.join(ROOT, "slam-tricks_amd")
CPP = os.path.join(ROOT, "tests", "cpp")


def build_g2o_exe(tmp_path_factory, stand_in):
    out = str(tmp_path_factory.mktemp("cpp") / "test_g2o_information_shim")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CPP, os.path.join(CPP, "test_g2o_information_shim.cpp")]
    if stand_in:
        cmd += ["-DSTBA_STAND_IN"]
    else:
        st = importlib.import_module("slam-tricks_amd")
        if not os.path.exists(st.LIB_PATH):
            importlib.import_module("slam-tricks_amd.build").build()
        cmd += ["-L", PKG, "-lstba", f"-Wl,-rpath,{PKG}"]
    subprocess.check_call(cmd + ["-o", out])
    return out


def build_ceres_exe(tmp_path_factory):
    st = importlib.import_module("slam-tricks_amd")
    if not os.path.exists(st.LIB_PATH):
        importlib.import_module("slam-tricks_amd.build").build()
    out = str(tmp_path_factory.mktemp("cpp") / "test_ba_information_shim")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "test_ba_information_shim.cpp"),
                           "-L", PKG, "-lstba", f"-Wl,-rpath,{PKG}", "-o", out])
    return out


def g2o_information(n, mode):
    """the n x 4 array the driver's edges carry in `mode` (tests/cpp/test_g2o_information_shim.cpp)"""
    k = np.arange(n)
    if mode == "scalars":
        w = 0.5 + 0.25 * (k % 7)
        return np.stack([w, 0 * w, 0 * w, w], 1)
    b = 0.3 * ((k % 4) - 1.5)
    return np.stack([1.0 + 0.5 * (k % 5), b, b, 2.0 + (k % 3)], 1)


@pytest.fixture(scope="module")
def g2o_exe(tmp_path_factory):
    return build_g2o_exe(tmp_path_factory, stand_in=True)


@pytest.fixture(scope="module")
def scene_file(tmp_path_factory):
    f = str(tmp_path_factory.mktemp("scene") / "s.bin")
    write_scene(f, B.scene("B"))
    return f


def test_identity_information_produces_no_table(g2o_exe, scene_file):
    out = run(g2o_exe, scene_file, "identity", "0.015", "3")
    assert out["g2o_iters"].startswith("1 "), out["g2o_iters"]
    assert out["set_information_calls"] == "0" and out["set_loss_calls"] == "1" and out["information"] == ""
    n = len(B.scene("B")["obs_cam"])
    assert out["edge_information"] == f"0 1 0 0 1 1 1 0 0 1 {n - 1} 1 0 0 1"


@pytest.mark.parametrize("mode", ["four", "scalars", "matrices"])
def test_information_reaches_the_c_abi_as_the_expected_array(g2o_exe, scene_file, mode):
    n = len(B.scene("B")["obs_cam"])
    out = run(g2o_exe, scene_file, mode, "0", "3")
    assert out["g2o_iters"].startswith("1 "), out["g2o_iters"]
    assert out["set_information_calls"] == "1" and out["set_loss_calls"] == "0"
    want = np.tile([4.0, 0.0, 0.0, 4.0], (n, 1)) if mode == "four" else g2o_information(n, mode)
    assert np.array_equal(vec(out, "information").reshape(n, 4), want)
    acc = vec(out, "edge_information").reshape(3, 5)
    assert np.array_equal(acc[:, 0], [0, 1, n - 1]) and np.array_equal(acc[:, 1:], want[[0, 1, n - 1]])


def test_ceres_h_weighted_factor_on_the_host(tmp_path_factory):
    exe = build_ceres_exe(tmp_path_factory)
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "host ok" in p.stdout, p.stdout + p.stderr
    assert "mixed problem: sqrt_info of 4 rows" in p.stdout and "no weighted factor: sqrt_info empty" in p.stdout
    assert "inner iterations with a weighted factor: refused" in p.stdout and "NOT REFUSED" not in p.stdout
