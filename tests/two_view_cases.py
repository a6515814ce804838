"""The inputs that tests/test_gpu_two_view_reference.py and tests/test_small_linalg.py share: the noise-free st22 scene at the sizes
where the reduction of the n x 9 epipolar system changes path, and the same rows in other orders and through a second camera.

tv_qr_kernel runs min(64, ceil(n / 512)) blocks of 128 lanes; a lane folds rows i, i + blocks * 128, ... into its own
triangular factor, a tree over LDS merges the 128 factors of a block, the host merges the blocks:
    8, 9            fewer rows than columns + 1; 120 lanes of the tree hold no row at all
    127, 128, 129   the lane boundary (129: one lane has two rows)
    512, 513        one block -> two blocks
    32768, 32769    64 blocks, four rows per lane -> the fifth trip of the grid-stride loop
    40000           the 64-block cap well behind
"""
import importlib

import numpy as np

scenes = importlib.import_module("slam-tricks_amd.scenes")

SIZES = [8, 9, 127, 128, 129, 512, 513, 32768, 32769, 40000]
VARIANT_SIZES = [129, 513, 32769]
VARIANTS = ["shuffled", "ascending", "descending", "K2"]
K2 = np.array([[4000.0, 0, 3000.0], [0, 4000.0, 2000.0], [0, 0, 1.0]])      # ten times the pixel magnitudes of the st22 camera

_cache = {}


def project(K, R, t, pts):
    """pixels of the frame-1 points in the camera with pose (R, t) in frame 1"""
    pc = (pts - t) @ R
    return np.stack([K[0, 0] * pc[:, 0] / pc[:, 2] + K[0, 2], K[1, 1] * pc[:, 1] / pc[:, 2] + K[1, 2]], 1)


def base():
    """the st22 correspondences, 40000 of them (a shorter scene is a prefix of this one), and the same landmarks through K2"""
    if "base" not in _cache:
        s = scenes.two_view_pairs(n_pts=max(SIZES), seed=22)
        s["g1"] = project(K2, np.eye(3), np.zeros(3), s["pts_f1"])
        s["g2"] = project(K2, s["R_true"], s["t_true"], s["pts_f1"])
        _cache["base"] = s
    return _cache["base"]


def f_case_ids():
    return [f"n{n}" for n in SIZES] + [f"n{n}-{v}" for n in VARIANT_SIZES for v in VARIANTS]


def f_case(cid):
    """-> dict(f1, f2, K, cam, n): cam ('K1' | 'K2') and n name the Gram matrix of the case.  A permutation of the rows leaves
    A^T A, and so the exact null vector and singular values, unchanged: the three reordered variants share the reference of
    the plain case and differ only in which lane and which level of the tree each row meets"""
    s = base()
    name, _, variant = cid.partition("-")
    n = int(name[1:])
    cam = "K2" if variant == "K2" else "K1"
    f1, f2 = (s["g1"][:n], s["g2"][:n]) if cam == "K2" else (s["f1"][:n], s["f2"][:n])
    if variant == "shuffled":
        p = np.random.default_rng(n).permutation(n)
    elif variant in ("ascending", "descending"):
        p = np.argsort(np.abs(f1[:, 0] * f2[:, 0]), kind="stable")
        p = p[::-1] if variant == "descending" else p
    else:
        p = np.arange(n)
    return dict(f1=np.ascontiguousarray(f1[p]), f2=np.ascontiguousarray(f2[p]), K=K2 if cam == "K2" else s["K"], cam=cam, n=n)


def system(f1, f2):
    """the n x 9 matrix as two_view.hip builds it (two_view_geometry.cpp:24-32), in doubles"""
    u1, v1, u2, v2 = f1[:, 0], f1[:, 1], f2[:, 0], f2[:, 1]
    return np.stack([u1 * u2, u1 * v2, u1, v1 * u2, v1 * v2, v1, u2, v2, np.ones(len(u1))], 1)
