"""time per LM iteration of the C5 bundle adjustment (1000 cameras, 100k landmarks, 1M observations) with and without landmark
position priors: lm_iterations the way bench.py runs it, the median of --reps x --steps iterations, one JSON line.
  --priors     a full random-SPD prior on every landmark (the true position disturbed by the prior's sigma, 5 cm)
  --root DIR   import the package from another checkout (the parent commit's tree, built there) to compare builds in one session
  --no-cache   generate the scene again.  Without it the scene (a minute to generate) is kept in $TMPDIR under a name made of the
               generator's arguments and read back by the next run -- also by the run of another build, which must time the same
               scene; a file whose sizes are not the ones asked for is not used"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--priors", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--label", default="")
ap.add_argument("--no-cache", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
st = importlib.import_module("slam-tricks_amd")
scenes = importlib.import_module("slam-tricks_amd.scenes")
GEN = dict(n_cams=1000, n_pts=100000, max_obs_per_pt=10, seed=20, pix_noise=1e-3)
cache = os.path.join(os.environ.get("TMPDIR", "/tmp"), "stba_scene_" + "_".join(f"{k}{v}" for k, v in sorted(GEN.items())) + ".npz")
s = None
if not args.no_cache and os.path.exists(cache):
    z = np.load(cache)
    s = {k: z[k] for k in z.files}
    if len(s.get("cams0", ())) != GEN["n_cams"] or len(s.get("pts0", ())) != GEN["n_pts"] or "pts_true" not in s:
        s = None                # (not this tool's file)
if s is None:
    s = scenes.st20_scene(**GEN)
    np.savez(cache, **s)
e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
n_priors = 0
if args.priors:
    rng = np.random.default_rng(1)
    npt = len(s["pts0"])
    pos = s["pts_true"] + rng.normal(0, 0.05, (npt, 3))
    A = rng.normal(size=(npt, 3, 3))
    Om = (A @ np.swapaxes(A, 1, 2) + 3 * np.eye(3)) * 100.0
    e.set_landmark_priors(np.arange(npt), pos, information=Om)
    n_priors = e.landmark_prior_count()
e.lm_iterations(args.warmup)
ms = []
for _ in range(args.reps):
    e.set_params(s["cams0"], s["pts0"])
    t0 = time.perf_counter()
    summ, _ = e.lm_iterations(args.steps)
    ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
print(json.dumps(dict(label=args.label, root=os.path.relpath(args.root), priors=n_priors, steps=args.steps, reps=args.reps,
                      ms_per_iteration_median=float(np.median(ms)), ms_per_iteration=[round(v, 5) for v in ms],
                      final_cost=summ.final_cost, successful_steps=summ.num_successful_steps)))
