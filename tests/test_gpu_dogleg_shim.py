"""Solver::Options::trust_region_strategy_type = DOGLEG through include/stba/ceres.h, driven by tests/cpp/test_dogleg_shim.cpp: the
st20 call site on "gpu-ba" and "gpu-ba-hostjac" gives the C-ABI engine's DOGLEG solve -- the same iterations, accept / reject
sequence, radii (IterationSummary::trust_region_radius is the dogleg radius) and end point -- and the Summary reports DOGLEG."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import lm_step_ref as L
from test_dogleg_cpu import DENSE_SCHUR, DOGLEG, TRADITIONAL_DOGLEG, shim, shim_run  # noqa: F401  (the fixture builds the driver)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def end_point(exe, *args):
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    return [np.array([float(x) for x in line.split()[1:]]) for line in p.stdout.splitlines() if line.startswith("P ")]


@pytest.mark.parametrize("kind,expect", [(1, "gpu-ba"), (2, "gpu-ba-hostjac")])
def test_st20_call_site_matches_the_engine(st, shim, kind, expect):
    exe, ba, _ = shim
    args = ("ba", ba, kind, DOGLEG, TRADITIONAL_DOGLEG, DENSE_SCHUR)
    out = shim_run(exe, *args)
    assert out["path"] == expect and out["termination"] == "0", out
    assert out["strategy"] == str(DOGLEG) and out["dogleg"] == str(TRADITIONAL_DOGLEG)
    scenes = importlib.import_module("slam-tricks_amd.scenes")
    s = scenes.st20_scene(pix_noise=1e-3)
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
    if kind == 2:
        prob = L.ba_problem(dict(s, pt_fixed=None))
        e.set_host_linearizer(lambda cams, pts, want: prob.lin_obs(cams.copy(), pts.copy(), want))
    e.set_trust_region("dogleg")
    summ, tr = e.solve(st.default_options(max_num_iterations=100))
    n_it = int(out["iterations"])
    radius = [float(x) for x in out["radius"].split()]
    ok = [int(x) for x in out["successful"].split()]
    assert n_it == summ.num_iterations and e.dogleg_summary().factorizations >= 1
    assert ok[1:] == [int(v) for v in tr[1:, 6]]
    assert np.allclose(radius, tr[:, 5], rtol=1e-12, atol=0), (radius, tr[:, 5])
    cams, pts = e.get_params()
    v = end_point(exe, *args)
    c_cpp, p_cpp = np.array(v[:len(cams)]), np.array(v[len(cams):])
    dq = np.minimum(np.abs(c_cpp[:, :4] - cams[:, :4]).max(1), np.abs(c_cpp[:, :4] + cams[:, :4]).max(1)).max()
    dt, dl = np.abs(c_cpp[:, 4:] - cams[:, 4:]).max(), np.abs(p_cpp - pts).max()
    print(f"{expect} DOGLEG: {n_it} iterations, end point against the engine: dq {dq:.2e} dt {dt:.2e} dL {dl:.2e}")
    assert max(dq, dt, dl) <= 1e-11
