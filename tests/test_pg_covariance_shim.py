"""ceres::Covariance on a pose graph through include/stba/ceres.h: tests/cpp/test_pg_covariance_shim.cpp compiled with g++ against the
header and libstba.so.  On the host: a graph with a component that has no constant pose is refused with the component named, before
any device is needed, and a pair with an unknown pointer is refused as on every route."""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_pg_covariance_shim.cpp")
PKG = os.path.join(ROOT, "slam-tricks_amd")


def build_exe(tmp_path_factory):
    st = importlib.import_module("slam-tricks_amd")
    if not os.path.exists(st.LIB_PATH):
        importlib.import_module("slam-tricks_amd.build").build()
    out = str(tmp_path_factory.mktemp("cpp") / "test_pg_covariance_shim")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC,
                           "-L", PKG, "-lstba", f"-Wl,-rpath,{PKG}", "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory)


def test_gauge_free_graph_and_unknown_pointer_are_refused_on_the_host(exe):
    p = subprocess.run([exe, "refuse"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "refuse ok" in p.stdout, p.stdout + p.stderr
    assert "component of 3 nodes" in p.stdout
    assert "stba_ceres::Covariance:" in p.stderr
