"""ITERATIVE_SCHUR against the dense path on C5 (1000 cameras x 100 000 landmarks x 10 observations, bench.py's scene) and on
the 50 000-camera scene of tests/test_gpu_iterative_schur.py; prints ONE JSON line.

  c5_lm_it_per_s            {dense, identity, jacobi, schur_jacobi}: LM iterations per second of stba_ba_lm_iterations (K each)
  c5_pcg_per_lm             PCG iterations per LM iteration, per preconditioner (Ceres' defaults: eta 0.1, at most 500)
  c5_matvec_ms              one implicit product S x (landmark pass + camera pass) on the device: hipEvents around R back-to-back
                            products (stba_ba_time_schur_apply); matvec_ms_50k the same on the 50 000-camera scene
  bytes_per_matvec          algorithmic: 2 x (64 B record + 4 B index) per observation + 24 B of z per landmark written and read
  share_of_hbm_peak         bytes / time / 8 TB/s (C5's 64 MB of records fit the 256 MiB Infinity Cache: this can exceed 1)
  s_per_lm_it_50k           the 50 000-camera scene, seconds per LM iteration of a solve with Schur-Jacobi
Run on the GPU:  python tools/iterative_schur_time.py [--steps K]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
st = importlib.import_module("slam-tricks_amd")
scenes = importlib.import_module("slam-tricks_amd.scenes")
HBM_PEAK = 8.0e12


def engine(s, solver):
    return st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], linear_solver=solver)


def lm_rate(s, solver, pc, k):
    e = engine(s, solver)
    if pc:
        e.set_pcg(pc)
    e.lm_iterations(2)                                   # warm-up
    e.set_params(s["cams0"], s["pts0"])
    t = time.perf_counter()
    summ, _ = e.lm_iterations(k)
    dt = time.perf_counter() - t
    pcg = e.pcg_summary().iterations_total / max(1, e.pcg_summary().solves) if pc else None
    return k / dt, pcg


def matvec_ms(s, reps=50):
    """device time of one implicit product (stba_ba_time_schur_apply)"""
    e = engine(s, "iterative_schur")
    e.evaluate(jac=False)
    e.normal_blocks()
    n = 6 * e.nc
    dc, dp = np.full(n, 1e-3), np.full((e.np_, 3), 1e-3)
    x = np.random.default_rng(0).normal(size=n)
    e.schur_apply(dc, dp, 0, x)
    return e.time_schur_apply(reps)


def matvec_bytes(s):
    # per observation: the 64 B record and a 4 B index in each pass; per landmark: z written and read; per camera: x read, y written
    return 2 * (64 + 4) * len(s["obs_cam"]) + 2 * 24 * len(s["pts0"]) + 2 * 48 * len(s["cams0"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    s = scenes.st20_scene(n_cams=1000, n_pts=100000, max_obs_per_pt=10, seed=20, pix_noise=1e-3, retriangulate=False)
    out = {"c5_lm_it_per_s": {}, "c5_pcg_per_lm": {}}
    out["c5_lm_it_per_s"]["dense"] = lm_rate(s, "dense_schur", None, args.steps)[0]
    for pc in ("identity", "jacobi", "schur_jacobi"):
        r, p = lm_rate(s, "iterative_schur", pc, args.steps)
        out["c5_lm_it_per_s"][pc] = r
        out["c5_pcg_per_lm"][pc] = p
    ms = matvec_ms(s)
    out["c5_matvec_ms"] = ms
    out["bytes_per_matvec"] = matvec_bytes(s)
    out["share_of_hbm_peak"] = matvec_bytes(s) / (ms * 1e-3) / HBM_PEAK
    big = scenes.large_ba_scene(n_cams=50000, n_pts=500000, views_per_pt=10, seed=1)
    ms_big = matvec_ms(big)
    out["matvec_ms_50k"] = ms_big
    out["bytes_per_matvec_50k"] = matvec_bytes(big)
    out["share_of_hbm_peak_50k"] = matvec_bytes(big) / (ms_big * 1e-3) / HBM_PEAK
    e = engine(big, "iterative_schur")
    e.set_pcg("schur_jacobi")
    t = time.perf_counter()
    summ, _ = e.solve(st.default_options(max_num_iterations=50))
    out["s_per_lm_it_50k"] = (time.perf_counter() - t) / max(1, summ.num_iterations)
    out["lm_iterations_50k"] = summ.num_iterations
    out["pcg_iterations_50k"] = e.pcg_summary().iterations_total
    print(json.dumps(out))


if __name__ == "__main__":
    main()
