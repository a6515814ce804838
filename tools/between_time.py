"""time per LM iteration of the C5 bundle adjustment (1000 cameras, 100k landmarks, 1M observations) with and without camera-to-camera
relative-pose factors: tools/prior_time.py's method -- lm_iterations the way bench.py runs it, the median of --reps x
--steps iterations, one JSON line.
  --edges      an odometry chain over all cameras (999 edges) plus --closures loop closures between random distant cameras, each with a
               full random-SPD information, the measurements the true relative poses disturbed by the sensor's sigma
  --root DIR   import the package from another checkout (the parent commit's tree, built there) to compare builds in one session"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--edges", action="store_true")
ap.add_argument("--closures", type=int, default=100)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
st = importlib.import_module("slam-tricks_amd")
scenes = importlib.import_module("slam-tricks_amd.scenes")
cache = os.path.join(os.environ.get("TMPDIR", "/tmp"), "stba_scene_c1000_p100000_m10_s20.npz")
if os.path.exists(cache):
    z = np.load(cache); s = {k: z[k] for k in z.files}
else:
    s = scenes.st20_scene(n_cams=1000, n_pts=100000, max_obs_per_pt=10, seed=20, pix_noise=1e-3)
    np.savez(cache, **s)
e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
n_edges = 0
if args.edges:
    rng = np.random.default_rng(1)
    nc = len(s["cams0"])
    ci, cj = np.arange(nc - 1), np.arange(1, nc)
    a = rng.integers(0, nc, args.closures)
    b = (a + rng.integers(nc // 4, 3 * nc // 4, args.closures)) % nc
    ci, cj = np.concatenate([ci, a]), np.concatenate([cj, b])
    T = s["cams_true"]

    def quat_mul(p, q):
        return np.stack([p[:, 3] * q[:, 0] + p[:, 0] * q[:, 3] + p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1],
                         p[:, 3] * q[:, 1] - p[:, 0] * q[:, 2] + p[:, 1] * q[:, 3] + p[:, 2] * q[:, 0],
                         p[:, 3] * q[:, 2] + p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0] + p[:, 2] * q[:, 3],
                         p[:, 3] * q[:, 3] - p[:, 0] * q[:, 0] - p[:, 1] * q[:, 1] - p[:, 2] * q[:, 2]], 1)
    qi = T[ci, :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    x, y, zz, w = T[ci, 0], T[ci, 1], T[ci, 2], T[ci, 3]
    R = np.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - zz * w), 2 * (x * zz + y * w),
                  2 * (x * y + zz * w), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - x * w),
                  2 * (x * zz - y * w), 2 * (y * zz + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    d = rng.normal(size=(len(ci), 6)) * np.array([0.01] * 3 + [0.02] * 3)
    half = 0.5 * d[:, :3]
    dq = np.concatenate([half, np.sqrt(1.0 - np.sum(half * half, 1, keepdims=True))], 1)
    meas = np.concatenate([quat_mul(quat_mul(qi, T[cj, :4]), dq), np.einsum("nji,nj->ni", R, T[cj, 4:] - T[ci, 4:]) + d[:, 3:]], 1)
    A = rng.normal(size=(len(ci), 6, 6))
    Om = A @ np.swapaxes(A, 1, 2) + 6 * np.eye(6)
    Om[:, :3, :3] *= 2500.0; Om[:, 3:, 3:] *= 400.0; Om[:, :3, 3:] *= 1000.0; Om[:, 3:, :3] *= 1000.0
    e.set_relative_poses(ci, cj, meas, information=Om)
    n_edges = e.relative_pose_count()
e.lm_iterations(args.warmup)
ms = []
for _ in range(args.reps):
    e.set_params(s["cams0"], s["pts0"])
    t0 = time.perf_counter()
    summ, _ = e.lm_iterations(args.steps)
    ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
print(json.dumps(dict(label=args.label, root=os.path.relpath(args.root), edges=n_edges, steps=args.steps, reps=args.reps,
                      ms_per_iteration_median=float(np.median(ms)), ms_per_iteration=[round(v, 5) for v in ms],
                      final_cost=summ.final_cost, successful_steps=summ.num_successful_steps)))
