"""NodePosePriorFactor through include/stba/ceres.h: tests/cpp/test_pg_prior_shim.cpp compiled with g++ against the header and
libstba.so.  On the host: the factor's residual is RelativePoseFactor's with the first pose at the identity (the same bits), its
autodiff Jacobian matches central differences to 1e-7 relative, and the recognition -- a graph of edges and priors is a pose graph
whose layout sets the priors aside (node, pose, W; the identity where none was given) and keeps the edges' weights and losses in edge
order; a prior with a LossFunction and a problem of priors only are not pose graphs; a graph without priors is laid out as before."""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_pg_prior_shim.cpp")
PKG = os.path.join(ROOT, "slam-tricks_amd")


def build_exe(tmp_path_factory):
    st = importlib.import_module("slam-tricks_amd")
    if not os.path.exists(st.LIB_PATH):
        importlib.import_module("slam-tricks_amd.build").build()
    out = str(tmp_path_factory.mktemp("cpp") / "test_pg_prior_shim")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC,
                           "-L", PKG, "-lstba", f"-Wl,-rpath,{PKG}", "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory)


def test_prior_factor_and_its_recognition_on_the_host(exe):
    p = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0 and "host ok" in p.stdout, p.stdout + p.stderr
    for which, what in enumerate(["pose graph", "not a pose graph", "not a pose graph", "pose graph"]):
        assert f"recognition {which}: {what}\n" in p.stdout
