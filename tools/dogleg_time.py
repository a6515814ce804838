"""LM against DOGLEG on C5 and on the st20 scene at its default noise and from a harder start: iterations, successful
and unsuccessful steps, factorisations, the best wall time of the solve over --reps runs (stba_ba_solve returns behind a stream
synchronisation) and the final cost, one JSON line per run.  The device time of the two DOGLEG kernels comes from a run of its own
under `rocprofv3 --kernel-trace --stats -- python tools/dogleg_time.py --only c5 --reps 1`.
usage: python tools/dogleg_time.py [--only c5|st20|st20_hard] [--reps R]"""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
st = importlib.import_module("slam-tricks_amd")
S = importlib.import_module("slam-tricks_amd.scenes")

SCENES = {
    "c5": dict(n_cams=1000, n_pts=100000, max_obs_per_pt=10, seed=20, pix_noise=1e-3),
    "st20": dict(pix_noise=1e-3),
    "st20_hard": dict(pix_noise=1e-3, pos_noise=0.6, ang_noise_deg=6.0),      # twice the default start noise
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(SCENES))
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for name, kw in SCENES.items():
        if a.only and name != a.only:
            continue
        s = S.st20_scene(**kw)
        for strat in ("lm", "dogleg"):
            best = None
            for _ in range(a.reps):
                e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
                e.set_trust_region(strat)
                t0 = time.perf_counter()
                summ, _ = e.solve()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
                ds = e.dogleg_summary()
                e.close()
            print(json.dumps(dict(scene=name, strategy=strat, iterations=summ.num_iterations, successful=summ.num_successful_steps,
                                  unsuccessful=summ.num_unsuccessful_steps, termination=summ.termination_type,
                                  factorizations=ds.factorizations if strat == "dogleg" else summ.num_iterations,
                                  reused_steps=ds.reused_steps, steps_by_case=list(ds.steps_by_case), final_cost=summ.final_cost,
                                  wall_s_best=best)), flush=True)


if __name__ == "__main__":
    main()
