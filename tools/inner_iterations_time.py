"""LM with and without inner iterations on C5 and on the st20 scene at its default noise: outer iterations,
factorisations (one per iteration that builds the reduced system), the wall time of the solve to convergence (stba_ba_solve returns
behind a stream synchronisation; best of --reps, the two variants alternating), the sweeps' device time per outer iteration
(phase_timing, a run of its own; per sweep and spread over all outer iterations), the inner LM iterations per block of one sweep at the start point (median, max) and the final
cost, one JSON line per scene and variant.  Per-kernel device times come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/inner_iterations_time.py --only c5 --reps 1`.
usage: python tools/inner_iterations_time.py [--only c5|st20] [--reps R]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
st = importlib.import_module("slam-tricks_amd")
S = importlib.import_module("slam-tricks_amd.scenes")

SCENES = {
    "c5": dict(n_cams=1000, n_pts=100000, max_obs_per_pt=10, seed=20, pix_noise=1e-3),
    "st20": dict(pix_noise=1e-3),
}


def engine(s, inner):
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
    if inner:
        e.set_inner_iterations(True)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(SCENES))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for name, kw in SCENES.items():
        if a.only and name != a.only:
            continue
        s = S.st20_scene(**kw)
        best = {False: None, True: None}
        for _ in range(a.reps):
            for inner in (False, True):          # alternating, so that drift of the device hits both
                e = engine(s, inner)
                t0 = time.perf_counter()
                summ, _ = e.solve()
                dt = time.perf_counter() - t0
                if best[inner] is None or dt < best[inner][0]:
                    best[inner] = (dt, summ, e.inner_summary() if inner else None)
        for inner in (False, True):
            dt, summ, isum = best[inner]
            out = dict(scene=name, inner_iterations=inner, outer_iterations=summ.num_iterations,
                       successful=summ.num_successful_steps, unsuccessful=summ.num_unsuccessful_steps,
                       factorizations=summ.num_iterations, seconds=round(dt, 5), final_cost=summ.final_cost,
                       termination=summ.termination_reason)
            if inner:
                e = engine(s, True)
                summ_t, _ = e.solve(st.default_options(phase_timing=1))
                it = e.inner_summary()
                out.update(sweeps=isum.sweeps, disabled_at_iteration=isum.disabled_at_iteration,
                           sweep_ms_per_sweep=round(it.sweep_ms / max(it.sweeps, 1), 4),
                           sweep_ms_per_outer_iteration=round(it.sweep_ms / max(summ_t.num_iterations, 1), 4),
                           group_sizes=list(it.group_size)[: it.num_groups])
                e = engine(s, True)
                c0, c1, per = e.inner_sweep()
                cams = np.maximum(per["rot"], per["pos"])
                out.update(first_sweep_cost=[c0, c1],
                           inner_iterations_camera_median_max=[float(np.median(cams)), int(cams.max())],
                           inner_iterations_landmark_median_max=[float(np.median(per["pt"])), int(per["pt"].max())])
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
