"""Wall time of the covariance block getters on C5 (1000 cameras, 100 000 landmarks), after one stba_ba_covariance_compute: the 10^5
landmark marginals, 10^5 camera-landmark blocks (every landmark with the camera of its first observation) and 10^5 landmark pairs
(j, j + 1), in one run.  Each call uploads its indices, makes one launch, copies the blocks home and returns behind a stream
synchronisation; the best of --reps calls, one JSON line.  Landmarks whose V_j has a pivot ratio below 1e-10 are held
constant, as tests/test_gpu_covariance.py::test_c5_full_size holds them.
usage: python tools/cov_cross_time.py [--reps R]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
st = importlib.import_module("slam-tricks_amd")
S = importlib.import_module("slam-tricks_amd.scenes")


def pivot_ratio3(H):
    d0 = H[:, 0, 0]
    d1 = H[:, 1, 1] - H[:, 0, 1] ** 2 / d0
    e12 = H[:, 1, 2] - H[:, 0, 1] * H[:, 0, 2] / d0
    d2 = H[:, 2, 2] - H[:, 0, 2] ** 2 / d0 - e12 ** 2 / d1
    d = np.stack([d0, d1, d2], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rc = d.min(1) / d.max(1)
    return np.where((d > 0).all(1), rc, 0.0)


def best_of(reps, fn):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        assert fn() == 0, st.lib().stba_last_error().decode()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    s = S.st20_scene(n_cams=1000, n_pts=100000, max_obs_per_pt=10, seed=20, pix_noise=1e-3)
    e0 = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
    e0.evaluate()
    weak = pivot_ratio3(e0.normal_blocks()[2]) < 1e-10
    e0.close()
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], weak.astype(np.uint8))
    L = st.lib()
    rc = C.c_double()
    t0 = time.perf_counter()
    assert L.stba_ba_covariance_compute(e._h, C.c_double(1e-14), C.byref(rc)) == 0, L.stba_last_error().decode()
    t_compute = (time.perf_counter() - t0) * 1e3
    np_ = e.np_
    op, oc = np.asarray(s["obs_pt"]), np.asarray(s["obs_cam"])
    seen, first = np.unique(op, return_index=True)                   # a landmark's first observation in the caller's order
    assert len(seen) == np_
    pts = np.arange(np_, dtype=np.int32)
    cam = np.ascontiguousarray(oc[first], np.int32)
    nxt = np.ascontiguousarray((pts + 1) % np_, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    marg, cp, pp = np.zeros((np_, 3, 3)), np.zeros((np_, 6, 3)), np.zeros((np_, 3, 3))
    L.stba_ba_point_covariance(e._h, 1, p(pts), p(marg))             # (the first launch of anything pays for loading the code)
    out = dict(scene="c5", n_cams=e.nc, n_pts=np_, n_obs=e.no, constant_landmarks=int(weak.sum()), reps=a.reps, compute_ms=t_compute,
               pivot_ratio=rc.value)
    out["marginals_ms"] = best_of(a.reps, lambda: L.stba_ba_point_covariance(e._h, np_, p(pts), p(marg)))
    out["camera_landmark_ms"] = best_of(a.reps, lambda: L.stba_ba_camera_point_covariance(e._h, np_, p(cam), p(pts), p(cp)))
    out["landmark_pairs_ms"] = best_of(a.reps, lambda: L.stba_ba_point_pair_covariance(e._h, np_, p(pts), p(nxt), p(pp)))
    for k in ("marginals_ms", "camera_landmark_ms", "landmark_pairs_ms"):
        out[k.replace("_ms", "_us_per_block")] = out[k] * 1e3 / np_
    # what came back: finite, and Sigma[j + 1, j] is bitwise Sigma[j, j + 1]^T
    back = np.zeros((1000, 3, 3))
    assert L.stba_ba_point_pair_covariance(e._h, 1000, p(nxt), p(pts), p(back)) == 0
    out["finite"] = bool(np.isfinite(marg).all() and np.isfinite(cp).all() and np.isfinite(pp).all())
    out["swapped_is_transpose"] = bool(np.array_equal(back, pp[:1000].transpose(0, 2, 1)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
