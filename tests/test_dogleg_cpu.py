"""The DOGLEG policy on the host: DoglegRegion and the shared case selection (slam-tricks_amd/csrc/dogleg_select.hpp), compiled
with g++, against dogleg_ref.traditional_dogleg on a table of cases; the new C-ABI symbols; the Python wrapper's argument checks."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import dogleg_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table():
    """(gamma, z_gn, alpha) triples that land in every case, with the six scalars the engine would hand the selection"""
    rng = np.random.default_rng(3)
    rows = []
    for k in range(60):
        n = 5
        d = rng.uniform(0.5, 2.0, n)
        gamma = rng.normal(size=n)
        zgn = -rng.uniform(0.5, 3.0) * gamma / d + 0.3 * rng.normal(size=n)
        Jh = rng.normal(size=(8, n))
        u, ygn = gamma / d, zgn / d
        ju, jn = Jh @ u, Jh @ ygn
        sc = (gamma @ gamma, gamma @ zgn, zgn @ zgn, ju @ ju, jn @ jn, ju @ jn)
        alpha = sc[0] / sc[3]
        radius = [1e-3, 0.5 * alpha * np.linalg.norm(gamma), 0.5 * (alpha * np.linalg.norm(gamma) + np.linalg.norm(zgn)),
                  2 * np.linalg.norm(zgn)][k % 4]
        rows.append((gamma, zgn, d, Jh, sc, radius))
    return rows


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dl") / "test_dogleg_policy")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_dogleg_policy.cpp"), "-o", out])
    return out


def test_selection_matches_reference(exe):
    rows = table()
    inp = "".join(" ".join(f"{v:.17g}" for v in (*sc, radius)) + "\n" for *_, sc, radius in rows)
    p = subprocess.run([exe], input=inp, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "dogleg_policy ok" in p.stdout, p.stdout[-2000:]
    lines = p.stdout.splitlines()[: len(rows)]
    seen = set()
    for (gamma, zgn, d, Jh, sc, radius), line in zip(rows, lines):
        kase, a, b, beta, znorm, model = line.split()
        kase, a, b, beta, znorm, model = int(kase), float(a), float(b), float(beta), float(znorm), float(model)
        alpha = sc[0] / sc[3]
        z, rk, rbeta = D.traditional_dogleg(-alpha * gamma, zgn, radius)
        seen.add(rk)
        assert kase == rk
        zc = a * gamma + b * zgn                     # y = a u + b y_gn  <=>  z = a gamma + b z_gn
        assert np.allclose(zc, z, rtol=1e-12, atol=1e-14 * np.linalg.norm(z))
        assert abs(znorm - np.linalg.norm(z)) <= 1e-13 * np.linalg.norm(z)
        y = z / d
        gh = gamma * d
        m_ref = -(gh @ y + 0.5 * (Jh @ y) @ (Jh @ y))
        assert abs(model - m_ref) <= 1e-11 * max(abs(m_ref), 1e-300)
        if kase == 2:
            assert abs(beta - rbeta) <= 1e-12
    assert seen == {0, 1, 2}


def test_non_finite_scalars_make_no_step(exe):
    p = subprocess.run([exe], input="nan 1 1 1 1 1 1\n1 1 inf 1 1 1 1\n", capture_output=True, text=True, timeout=60)
    assert p.stdout.splitlines()[:2] == ["-1 0 0 0 0 0", "-1 0 0 0 0 0"]


def test_new_symbols_are_exported():
    st = importlib.import_module("slam-tricks_amd")
    L = st.lib()
    for name in ("stba_ba_set_trust_region", "stba_ba_last_dogleg_summary"):
        assert name in st.EXPORTS
        getattr(L, name)
    assert st.TRUST_REGIONS == {"lm": 0, "dogleg": 1}


# ---- include/stba/ceres.h: what DOGLEG refuses, before any device work (tests/cpp/test_dogleg_shim.cpp; no device needed)
DENSE_SCHUR, ITERATIVE_SCHUR = 3, 5                   # ceres.h LinearSolverType
LEVENBERG_MARQUARDT, DOGLEG = 0, 1                    # TrustRegionStrategyType
TRADITIONAL_DOGLEG, SUBSPACE_DOGLEG = 0, 1            # DoglegType


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    import struct
    st = importlib.import_module("slam-tricks_amd")
    st.lib()
    scenes = importlib.import_module("slam-tricks_amd.scenes")
    d = tmp_path_factory.mktemp("shim")
    exe = str(d / "test_dogleg_shim")
    pkg = os.path.join(ROOT, "slam-tricks_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_dogleg_shim.cpp"), "-L", pkg, "-lstba", f"-Wl,-rpath,{pkg}", "-o", exe])
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


def shim_run(exe, *args):
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = {"stderr": p.stderr}
    for line in p.stdout.splitlines():
        w = line.split(" ", 1)
        if w[0] != "P":
            out[w[0]] = w[1] if len(w) > 1 else ""
    return out


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("what,dogleg_type,solver", [("SUBSPACE_DOGLEG", SUBSPACE_DOGLEG, DENSE_SCHUR),
                                                     ("ITERATIVE_SCHUR", TRADITIONAL_DOGLEG, ITERATIVE_SCHUR)])
def test_ceres_shim_refusals_on_ba(shim, kind, what, dogleg_type, solver):
    exe, ba, _ = shim
    out = shim_run(exe, "ba", ba, kind, DOGLEG, dogleg_type, solver)
    assert out["termination"] == "2" and out["moved"] == "0" and out["iterations"] == "-1", out      # FAILURE, parameters untouched
    assert what in out["message"] and what in out["stderr"] and "nothing was solved" in out["message"]
    assert out["strategy"] == str(LEVENBERG_MARQUARDT)


def test_ceres_shim_refuses_dogleg_off_the_ba_paths(shim):
    exe, _, pnp = shim
    out = shim_run(exe, "pnp", pnp, DOGLEG)
    assert out["termination"] == "2" and out["moved"] == "0", out
    assert "gpu-dense-callback" in out["message"] and "gpu-dense-callback" in out["stderr"]
