"""ceres::Covariance (include/stba/ceres.h) on a bundle adjustment, for the pairs that are not two camera blocks or one landmark
with itself (Covariance::Options::bundle_adjustment_cross_blocks), driven by tests/cpp/test_covariance_cross.cpp: the st20 problem on "gpu-ba" and "gpu-ba-hostjac" with
(rotation, landmark), (position, landmark), (landmark, rotation) and two different landmarks both ways round.  Every tangent
block against BAEngine.cross_covariance at the same point, swapped blocks are transposes, the ambient block of an SO3 block
against a landmark is J C for the parameterisation's Jacobian."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_covariance_shim import plus_jacobian, rel, write_scene

pytestmark = pytest.mark.gpu

SRC = os.path.join(ROOT, "tests", "cpp", "test_covariance_cross.cpp")
PKG = os.path.join(ROOT, "slam-tricks_amd")


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


@pytest.fixture(scope="module")
def exe(st, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "test_covariance_cross")
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
            rows, cols = int(w[3]), int(w[4])
            (T if w[0] == "T" else A)[(w[1], w[2])] = np.array([float(x) for x in w[5:]]).reshape(rows, cols)
    return path, T, A


@pytest.fixture(scope="module")
def st20_solved(st, tmp_path_factory):
    scenes = importlib.import_module("slam-tricks_amd.scenes")
    s = scenes.st20_scene()
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
    e.solve()
    cams, pts = e.get_params()
    path = str(tmp_path_factory.mktemp("scene") / "st20.bin")
    write_scene(path, s, cams, pts)
    return dict(path=path, cams=cams, e=e)


def block_of(name):
    kind, idx = re.fullmatch(r"([qtL])(\d+)", name).groups()
    return kind, int(idx)


@pytest.mark.parametrize("kind,expect", [(0, "gpu-ba"), (2, "gpu-ba-hostjac")])
def test_st20_cross_blocks_match_the_engine(exe, st20_solved, kind, expect):
    path, T, A = run(exe, "ba", st20_solved["path"], kind)
    assert path == expect
    e, cams = st20_solved["e"], st20_solved["cams"]
    # what the driver asked for, from the engine at the same point
    cam_points = sorted({(block_of(a)[1], block_of(b)[1]) for a, b in T if block_of(a)[0] in "qt" and block_of(b)[0] == "L"} |
                        {(block_of(b)[1], block_of(a)[1]) for a, b in T if block_of(a)[0] == "L" and block_of(b)[0] in "qt"})
    point_pairs = sorted((block_of(a)[1], block_of(b)[1]) for a, b in T if block_of(a)[0] == "L" and block_of(b)[0] == "L")
    assert len(cam_points) == 16 and len(point_pairs) == 13
    cp, pp, _ = e.cross_covariance(cam_points=cam_points, point_pairs=point_pairs)
    cp = dict(zip(cam_points, cp))
    pp = dict(zip(point_pairs, pp))
    worst, n, zeros = 0.0, 0, 0
    kinds = set()
    for (na, nb), got in T.items():
        (ka, ia), (kb, ib) = block_of(na), block_of(nb)
        if ka in "qt" and kb in "qt":
            continue                                         # (a camera block: tests/test_gpu_covariance_shim.py)
        if ka in "qt":
            ref = cp[(ia, ib)][:3] if ka == "q" else cp[(ia, ib)][3:]
        elif kb in "qt":
            ref = (cp[(ib, ia)][:3] if kb == "q" else cp[(ib, ia)][3:]).T
        else:
            ref = pp[(ia, ib)]
        kinds.add((ka, kb))
        if np.linalg.norm(ref) == 0.0:                       # the constant camera
            assert np.array_equal(got, np.zeros((3, 3)))
            zeros += 1
        else:
            worst = max(worst, rel(got, ref)); n += 1
        if (nb, na) in T:                                    # asked for both ways round: the swapped pair is the transpose
            assert np.array_equal(T[(nb, na)], got.T), (na, nb)
    assert {("q", "L"), ("t", "L"), ("L", "q"), ("L", "t"), ("L", "L")} <= kinds and zeros > 0
    print(f"{expect} (kind {kind}): {n} cross blocks, worst relative difference from BAEngine.cross_covariance {worst:.3e}, {zeros} exactly zero")
    assert worst <= 1e-10
    # ambient blocks: J C for an SO3 block against a landmark (4 x 3), C J^T the other way round (3 x 4), C itself elsewhere
    wa, na_ = 0.0, 0
    for (na, nb), amb in A.items():
        (ka, ia), (kb, ib) = block_of(na), block_of(nb)
        Ja = plus_jacobian(cams[ia][:4]) if ka == "q" else np.eye(3)
        Jb = plus_jacobian(cams[ib][:4]) if kb == "q" else np.eye(3)
        ref = Ja @ T[(na, nb)] @ Jb.T
        assert amb.shape == ref.shape == (4 if ka == "q" else 3, 4 if kb == "q" else 3)
        if not ref.any():
            assert not amb.any()
            continue
        if ka != "q" and kb != "q":
            assert np.array_equal(amb, T[(na, nb)])
            continue
        wa = max(wa, rel(amb, ref)); na_ += 1
    print(f"{na_} ambient SO3 blocks against J C: worst {wa:.3e}")
    assert na_ >= 18 and wa <= 1e-8
