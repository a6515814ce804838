"""Robust kernels through include/stba/g2o.h (tests/cpp/test_g2o_loss_shim.cpp): setRobustKernel(new RobustKernelHuber) with setDelta
reaches the same bits as the C ABI with Huber(delta) on the same observations (g2o's Huber and Cauchy are Ceres' rho with a = delta;
chi2 is sum rho = 2 x the engine's cost); a RobustKernel subclass of the caller's is refused the way a foreign edge type is, before
any device work, and the edge owns (and deletes) its kernel."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import ba_loss_ref as B
from conftest import ROOT
from test_cpp_shim import run, vec, write_scene

PKG = os.path.join(ROOT, "slam-tricks_amd")
ITERATIONS = 40


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    st = importlib.import_module("slam-tricks_amd")
    if not os.path.exists(st.LIB_PATH):
        importlib.import_module("slam-tricks_amd.build").build()
    out = str(tmp_path_factory.mktemp("cpp") / "test_g2o_loss_shim")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "test_g2o_loss_shim.cpp"), "-L", PKG, "-lstba", f"-Wl,-rpath,{PKG}", "-o", out])
    return out


def test_a_foreign_kernel_class_is_refused_and_the_edge_owns_its_kernel(exe, tmp_path):
    s = B.scene("B")
    f = str(tmp_path / "s.bin")
    write_scene(f, s)
    out = run(exe, f, "foreign", "0.015", str(ITERATIONS))
    assert out["g2o_iters"].startswith("0 ")
    assert f"edge {len(s['obs_cam']) // 2}: unsupported robust kernel" in out["g2o_iters"]
    assert out["kernels"] == "1 owned_deleted 1"
    assert np.array_equal(vec(out, "g2o_cams").reshape(-1, 7), s["cams0"]) and np.array_equal(vec(out, "g2o_pts").reshape(-1, 3), s["pts0"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,delta", [("huber", 0.015), ("cauchy", 0.015)])
def test_robust_kernels_reach_the_c_abis_bits(exe, tmp_path, kind, delta):
    st = importlib.import_module("slam-tricks_amd")
    s = B.scene("B")
    n = len(s["obs_cam"])
    assert np.array_equal(s["cam_fixed"].any(1), s["cam_fixed"].all(1))
    f = str(tmp_path / "s.bin")
    write_scene(f, s)
    out = run(exe, f, kind, repr(delta), str(ITERATIONS))
    toks = out["g2o_iters"].split()
    iters, chi2 = int(toks[0]), float(toks[2])
    assert iters >= 1, out["g2o_iters"]
    on = np.arange(n) % 2 == 0
    table = dict(kind=np.where(on, st.LOSS_KINDS[kind], 0).astype(np.int32), a=np.where(on, delta, 1.0))
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], loss=table)
    summ, _ = e.solve(max_num_iterations=ITERATIONS)
    cams, pts = e.get_params()
    print(f"g2o {kind}({delta}) on every even edge: {iters} iterations chi2 {chi2:.12e}; C ABI {summ.num_iterations} iterations 2 x cost {2 * summ.final_cost:.12e}")
    assert iters == summ.num_iterations and chi2 == 2.0 * summ.final_cost
    assert np.array_equal(vec(out, "g2o_cams").reshape(-1, 7), cams) and np.array_equal(vec(out, "g2o_pts").reshape(-1, 3), pts)
    prob = B.RobustBAProblem(dict(s, pt_fixed=None), B.table_of(table["kind"], table["a"], 1.0, 1.0, n))
    ref_cost = prob.cost(np.concatenate([cams.reshape(-1), pts.reshape(-1)]))
    assert abs(2 * ref_cost - chi2) <= 1e-12 * chi2                      # chi2 is sum rho at the end point
    # (not the lossless problem's: at this end point 1/2 sum r^2 is another number, and the lossless solve ends elsewhere)
    plain = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
    summ0, _ = plain.solve(max_num_iterations=ITERATIONS)
    c0, _ = plain.get_params()
    print(f"  lossless solve: 2 x cost {2 * summ0.final_cost:.12e}, cameras {np.abs(c0 - cams).max():.2e} away")
    assert not np.array_equal(c0, cams)
    assert out["kernels"] == f"{int(on.sum())} owned_deleted 0"
