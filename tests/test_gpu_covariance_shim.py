"""ceres::Covariance (include/stba/ceres.h) on the device, driven by tests/cpp/test_covariance.cpp:
  * the st20 call site with the built-in factor, the user's recognised ProjectFactor ("gpu-ba") and a factor the probe rejects
    ("gpu-ba-hostjac"): every tangent block against BAEngine.covariance at the same point; the ambient SO3 block equals J C J^T;
  * the st17 PnP problem and the C1 parabola fit ("gpu-dense", stba_dense_covariance) against numpy's (J^T J)^-1."""
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "cpp", "test_covariance.cpp")
PKG = os.path.join(ROOT, "slam-tricks_amd")
EPS = 2.2e-16


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


@pytest.fixture(scope="module")
def exe(st, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "test_covariance")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC,
                           "-L", PKG, "-lstba", f"-Wl,-rpath,{PKG}", "-o", out])
    return out


def run(exe, *args):
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    path, T, A = None, {}, {}
    for line in p.stdout.splitlines():
        w = line.split()
        if w[0] == "path":
            path = w[1] if len(w) > 1 else ""
        elif w[0] in ("T", "A"):
            v = np.array([float(x) for x in w[3:]])
            n = int(round(np.sqrt(len(v))))
            (T if w[0] == "T" else A)[(w[1], w[2])] = v.reshape(n, n)
    return path, T, A


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def plus_jacobian(q, h=1e-6):
    """d (q (x) exp(delta)) / d delta at 0, by central differences (4 x 3)"""
    def plus(d):
        th = np.linalg.norm(d)
        e = np.array([*(np.sin(th / 2) / th * d), np.cos(th / 2)]) if th > 0 else np.array([0, 0, 0, 1.0])
        return quat_mul(q, e)
    J = np.zeros((4, 3))
    for k in range(3):
        d = np.zeros(3); d[k] = h
        J[:, k] = (plus(d) - plus(-d)) / (2 * h)
    return J


def write_scene(path, s, cams, pts):
    with open(path, "wb") as f:
        f.write(struct.pack("iii", len(cams), len(pts), len(s["obs_cam"])))
        f.write(np.ascontiguousarray(cams, np.float64).tobytes())
        f.write(np.ascontiguousarray(pts, np.float64).tobytes())
        f.write(np.ascontiguousarray(s["obs_cam"], np.int32).tobytes())
        f.write(np.ascontiguousarray(s["obs_pt"], np.int32).tobytes())
        f.write(np.ascontiguousarray(s["obs_feat"], np.float64).tobytes())
        f.write(np.ascontiguousarray(s["cam_fixed"][:, 0], np.uint8).tobytes())


@pytest.fixture(scope="module")
def st20_solved(st, tmp_path_factory):
    scenes = importlib.import_module("slam-tricks_amd.scenes")
    s = scenes.st20_scene()
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
    e.solve()
    cams, pts = e.get_params()
    path = str(tmp_path_factory.mktemp("scene") / "st20.bin")
    write_scene(path, s, cams, pts)
    nc = len(cams)
    pairs = [(c, c) for c in range(nc)] + [(c, (7 * c + 3) % nc) for c in range(10)]
    cam, pb, _ = e.covariance(cam_pairs=pairs)
    return dict(path=path, cams=cams, pts=pts, pairs=pairs, cam=cam, pb=pb)


@pytest.mark.parametrize("kind,expect", [(0, "gpu-ba"), (1, "gpu-ba"), (2, "gpu-ba-hostjac")])
def test_st20_call_site_matches_the_engine(exe, st20_solved, kind, expect):
    path, T, A = run(exe, "ba", st20_solved["path"], kind)
    assert path == expect
    ref = {}
    for (a, b), blk in zip(st20_solved["pairs"], st20_solved["cam"]):
        ref[(f"q{a}", f"t{b}")] = blk[:3, 3:]
        if a == b:
            ref[(f"q{a}", f"q{a}")] = blk[:3, :3]
            ref[(f"t{a}", f"t{a}")] = blk[3:, 3:]
    for j, blk in enumerate(st20_solved["pb"]):
        ref[(f"L{j}", f"L{j}")] = blk
    worst, n = 0.0, 0
    for key, r in ref.items():
        got = T[key]
        if np.linalg.norm(r) == 0.0:               # a constant camera
            assert np.array_equal(got, np.zeros((3, 3)))
            continue
        worst = max(worst, rel(got, r)); n += 1
        if (key[1], key[0]) in T:                  # (asked for both ways round: the swapped pair is the transpose)
            assert np.array_equal(T[(key[1], key[0])], got.T)
    print(f"{expect} (kind {kind}): {n} blocks, worst relative difference from BAEngine.covariance {worst:.3e}")
    assert worst <= 1e-10
    # ambient SO3 block = J C J^T, J the chart's Jacobian at the camera's quaternion
    wa = 0.0
    for c, cam in enumerate(st20_solved["cams"]):
        C = T[(f"q{c}", f"q{c}")]
        if not C.any():
            assert not A[(f"q{c}", f"q{c}")].any()
            continue
        J = plus_jacobian(cam[:4])
        wa = max(wa, rel(A[(f"q{c}", f"q{c}")], J @ C @ J.T))
    print(f"ambient SO3 blocks against J C J^T: worst {wa:.3e}")
    assert wa <= 1e-8


def test_pnp_takes_the_dense_route_and_matches_numpy(exe, O, tmp_path):
    scenes = importlib.import_module("slam-tricks_amd.scenes")
    s = scenes.pnp_scene()
    pose = np.asarray(s["pose_init"], np.float64)
    f = str(tmp_path / "pnp.bin")
    with open(f, "wb") as fh:
        fh.write(struct.pack("i", len(s["pts"])))
        fh.write(pose.tobytes())
        fh.write(np.ascontiguousarray(np.hstack([s["pts"], s["feats"]]), np.float64).tobytes())
    path, T, A = run(exe, "pnp", f)
    assert path == "gpu-dense"
    J = np.concatenate([O.reproj_jacobian(pose[:4], pose[4:], L)[0] for L in s["pts"]])     # (2n, 6): [dtheta, dt]
    H = J.T @ J
    ev = np.linalg.eigvalsh(H)
    kappa = ev[-1] / ev[0]
    C = np.linalg.inv(H)
    got = np.block([[T[("q0", "q0")], T[("q0", "t0")]], [T[("t0", "q0")], T[("t0", "t0")]]])
    err = rel(got, C)
    print(f"PnP: kappa {kappa:.3e}, relative error {err:.3e}, tolerance {50 * kappa * EPS:.3e}")
    assert err <= 50 * kappa * EPS
    Jq = plus_jacobian(pose[:4])
    assert rel(A[("q0", "q0")], Jq @ C[:3, :3] @ Jq.T) <= 1e-8


def test_curve_fit_takes_the_dense_route_and_matches_numpy(exe, tmp_path):
    scenes = importlib.import_module("slam-tricks_amd.scenes")
    xy = scenes.curve_fit_data()
    abc = np.array([0.5, 1.0, 1.5])
    f = str(tmp_path / "curve.bin")
    with open(f, "wb") as fh:
        fh.write(struct.pack("i", len(xy)))
        fh.write(abc.tobytes())
        fh.write(np.ascontiguousarray(xy, np.float64).tobytes())
    path, T, _ = run(exe, "curve", f)
    assert path == "gpu-dense"
    x = xy[:, 0]
    J = -np.stack([x * x, x, np.ones_like(x)], 1)
    H = J.T @ J
    ev = np.linalg.eigvalsh(H)
    kappa = ev[-1] / ev[0]
    err = rel(T[("x", "x")], np.linalg.inv(H))
    print(f"curve fit: kappa {kappa:.3e}, relative error {err:.3e}, tolerance {50 * kappa * EPS:.3e}")
    assert err <= 50 * kappa * EPS
