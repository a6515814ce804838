"""Observation patterns for tests/test_schur_plan_cpu.py: the smallest shapes at which every branch of the Schur plan
(slam-tricks_amd/csrc/schur_plan.hpp) is live.  Plain index arithmetic, no random generator: the same everywhere.

A case is a dict: n_cams, n_pts, obs_cam, obs_pt (int32), free_bytes, have_mem_info, iterative.  The features are not part of it:
observation i is at (i + 0.25, -i - 0.5), here (features) and in tests/cpp/schur_plan_driver.cpp."""
import math

import numpy as np

GIB = 1 << 30
PLENTY = 200 * GIB              # free device memory where the case is not about it
NAMES = ["small", "two_cams", "wide_row", "dup", "lm_slices", "two_slices", "dense", "dense_dup_overflow", "no_room", "iterative"]
REFUSED = ["dense_dup_overflow", "no_room"]


def lda(n_cams):
    """chol_padded_dim(6 n_cams) of csrc/common.hpp: the padded dimension of S"""
    return (6 * n_cams + 1 + 127) // 128 * 128


def features(n_obs):
    i = np.arange(n_obs, dtype=np.float64)
    return np.stack([i + 0.25, -i - 0.5], axis=1)


def _shuffled(cam, pt):
    """the observations in a scattered order (position k holds observation k * stride mod n, stride coprime to n near 0.618 n), so
    that the regrouping has something to do"""
    cam, pt = np.asarray(cam, dtype=np.int64), np.asarray(pt, dtype=np.int64)
    n = len(cam)
    if n < 3:
        return cam.astype(np.int32), pt.astype(np.int32)
    stride = int(0.618 * n) | 1
    while math.gcd(stride, n) != 1:
        stride += 2
    idx = (np.arange(n, dtype=np.int64) * stride) % n
    return cam[idx].astype(np.int32), pt[idx].astype(np.int32)


def _window(n_pts, n_cams, k, first=None):
    """landmark j seen by the k cameras first(j), first(j) + 1, ... (mod n_cams)"""
    j = np.repeat(np.arange(n_pts, dtype=np.int64), k)
    off = np.tile(np.arange(k, dtype=np.int64), n_pts)
    f = (j if first is None else first(j))
    return (f + off) % n_cams, j


def _small_lists():
    # cameras 0..5 in a ring, camera 6 sees nothing; landmarks 0..37 by three neighbours, 38 by camera 0 alone, 39 by nobody
    cam, pt = _window(38, 6, 3)
    return np.append(cam, 0), np.append(pt, 38)


def _dense_lists():
    return _window(2300, 30, 30, first=lambda j: 0 * j)


def _case(n_cams, n_pts, cam, pt, free_bytes=PLENTY, iterative=False, shuffle=True):
    oc, op = _shuffled(cam, pt) if shuffle else (np.asarray(cam, np.int32), np.asarray(pt, np.int32))
    return dict(n_cams=n_cams, n_pts=n_pts, obs_cam=oc, obs_pt=op, free_bytes=free_bytes, have_mem_info=True, iterative=iterative)


def case(name):
    if name == "small":
        return _case(7, 40, *_small_lists())
    if name == "iterative":
        return _case(7, 40, *_small_lists(), iterative=True)
    if name == "two_cams":
        return _case(2, 600, *_window(600, 2, 2, first=lambda j: 0 * j))
    if name == "wide_row":
        # landmark 0 by all 300 cameras; landmarks 1..600 by three neighbours (two landmarks per first camera)
        c0, p0 = _window(1, 300, 300)
        c1, p1 = _window(600, 300, 3, first=lambda j: j // 2)
        return _case(300, 601, np.concatenate([c0, c1]), np.concatenate([p0, p1 + 1]))
    if name == "dup":
        cam, pt = _small_lists()
        extra_c, extra_p = [], []
        for (c, j, times) in [(1, 0, 2), (3, 2, 3), (4, 3, 2), (5, 4, 256)]:        # (camera c sees landmark j: `times` observations of it)
            assert ((cam == c) & (pt == j)).sum() == 1
            extra_c += [c] * (times - 1); extra_p += [j] * (times - 1)
        return _case(7, 40, np.concatenate([cam, extra_c]), np.concatenate([pt, extra_p]))
    if name == "lm_slices":
        return _case(40, 20000, *_window(20000, 40, 10))
    if name == "two_slices":
        # landmark j = base + 256 t by the 20 cameras base + k stride(t) mod 256.  The multiples k stride, |k| < 20, of these fifteen
        # strides are all the 255 differences of two camera numbers, so the last rows share a landmark with every camera in front
        # of them (odd strides alone cannot make a difference that 32 divides)
        strides = np.array([1, 10, 23, 13, 21, 9, 37, 33, 4, 53, 55, 47, 17, 15, 8], dtype=np.int64)
        j = np.repeat(np.arange(5200, dtype=np.int64), 20)
        k = np.tile(np.arange(20, dtype=np.int64), 5200)
        return _case(256, 5200, (j % 256 + k * strides[(j // 256) % 15]) % 256, j)
    if name == "dense":
        return _case(30, 2300, *_dense_lists())
    if name == "dense_dup_overflow":
        cam, pt = _dense_lists()
        return _case(30, 2300, np.concatenate([cam, np.full(255, 7)]), np.concatenate([pt, np.full(255, 11)]))
    if name == "no_room":
        return _case(30, 2300, *_dense_lists(), free_bytes=1 << 20)
    raise KeyError(name)


def write_case(path, c, free_bytes=None):
    head = np.array([c["n_cams"], c["n_pts"], len(c["obs_cam"]), c["free_bytes"] if free_bytes is None else free_bytes,
                     int(c["have_mem_info"]), int(c["iterative"]), lda(c["n_cams"]), 0], dtype="<i8")
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(np.asarray(c["obs_cam"], dtype="<i4").tobytes())
        f.write(np.asarray(c["obs_pt"], dtype="<i4").tobytes())
