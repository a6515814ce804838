"""ceres::Covariance in include/stba/ceres.h: tests/cpp/test_covariance.cpp compiled with g++ against the header and libstba.so.
On the host: the requests the layer refuses before any device work, and the failure without a device."""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_covariance.cpp")
PKG = os.path.join(ROOT, "slam-tricks_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    st = importlib.import_module("slam-tricks_amd")
    if not os.path.exists(st.LIB_PATH):
        importlib.import_module("slam-tricks_amd.build").build()
    out = str(tmp_path_factory.mktemp("cpp") / "test_covariance")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC,
                           "-L", PKG, "-lstba", f"-Wl,-rpath,{PKG}", "-o", out])
    return out


def run(exe, mode):
    p = subprocess.run([exe, mode], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_refusals_on_the_host(exe):
    rc, out, err = run(exe, "refuse")
    assert rc == 0 and "refuse ok" in out, out + err
    assert "stba_ceres::Covariance:" in err            # the reason also goes to stderr, as Solve's does


def test_valid_request_fails_without_a_device_and_runs_with_one(exe):
    st = importlib.import_module("slam-tricks_amd")
    mode = "device" if st.device_count() > 0 else "nodevice"
    rc, out, err = run(exe, mode)
    assert rc == 0 and f"{mode} ok" in out, out + err
