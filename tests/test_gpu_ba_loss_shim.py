"""A bundle adjustment with robust losses through include/stba/ceres.h on the device (tests/cpp/test_ba_loss_shim.cpp), scene B of
tests/ba_loss_ref.py fed through the driver with Solver::Options::bundle_adjustment_losses set:
  * ceres::Solve with HuberLoss(0.015) on every block takes "gpu-ba" and ends at BAEngine.solve's final cost and parameters for the same
    table in every bit (the same options and the cameras listed in the order the shim numbers them: the same computation); its
    initial cost is the robust reference's 1/2 sum rho;
  * the same with ScaledLoss(CauchyLoss(0.015), 2) on every third block and no loss object elsewhere;
  * ceres::Covariance at the solution takes "gpu-ba" and returns (J'^T J')^-1: the bits of BAEngine.covariance at the same point."""
import importlib
import subprocess

import numpy as np
import pytest

import ba_loss_ref as B
from test_ba_loss_shim import build_exe

pytestmark = pytest.mark.gpu

CAM_PAIRS = [(1, 1), (4, 4), (1, 2), (2, 1), (8, 3), (0, 5)]
LANDMARKS = [0, 7, 150, 299]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory)


def run_device(exe, tmp_path, s, rows):
    """rows: n_obs x (kind | -1, a, b, scale) as the driver reads them.  Returns (summary words, cams, pts, blocks)"""
    nc, np_, no = len(s["cams0"]), len(s["pts0"]), len(s["obs_cam"])
    fixed = s["cam_fixed"].all(1).astype(int)
    assert np.array_equal(s["cam_fixed"].any(1), s["cam_fixed"].all(1)) and not s["pt_fixed"].any()      # whole cameras only
    path = tmp_path / "scene.txt"
    with open(path, "w") as f:
        f.write(f"{nc} {np_} {no} {len(CAM_PAIRS)} {len(LANDMARKS)}\n")
        np.savetxt(f, s["cams0"], fmt="%.17g")
        np.savetxt(f, fixed[None], fmt="%d")
        np.savetxt(f, s["pts0"], fmt="%.17g")
        for c, j, (fx, fy) in zip(s["obs_cam"], s["obs_pt"], s["obs_feat"]):
            f.write(f"{int(c)} {int(j)} {float(fx)!r} {float(fy)!r}\n")
        for k, a, b, sc in rows:
            f.write(f"{int(k)} {float(a)!r} {float(b)!r} {float(sc)!r}\n")
        np.savetxt(f, np.array(CAM_PAIRS), fmt="%d")
        np.savetxt(f, np.array(LANDMARKS)[None], fmt="%d")
    p = subprocess.run([exe, "device", str(path)], capture_output=True, text=True, timeout=600)
    lines = p.stdout.splitlines()
    short = "\n".join(ln[:300] for ln in lines if ln[:2] not in ("R ", "P ", "L "))
    assert p.returncode == 0 and "device ok" in p.stdout, short + p.stderr[-2000:]
    out, T = {}, {}
    for line in lines:
        w = line.split()
        if w and w[0] in ("R", "P", "L"):
            T[(w[0], int(w[1]))] = np.array([float(x) for x in w[2:]]).reshape(3, 3)
        elif w and w[0] in ("ba_cams", "ba_pts"):
            out[w[0]] = np.array([float(x) for x in w[1:]])
        elif w:
            out[w[0]] = w[1:]
    assert out["ba"][1] == "gpu-ba" and out["cov"][1] == "gpu-ba", (out["ba"], out["cov"])
    return out, out["ba_cams"].reshape(-1, 7), out["ba_pts"].reshape(-1, 3), T


def as_the_shim_numbers_it(s):
    """ceres.h numbers cameras and landmarks in the order the residual blocks first name them (DetectBa); sums over cameras run in
    that order, so the engine the shim creates is the engine of THIS listing of the scene.  Returns (scene, order): camera k of the
    listing is camera order[k] of s (B is landmark-major and every landmark is observed: the landmarks keep their numbers)"""
    _, first = np.unique(s["obs_cam"], return_index=True)
    order = s["obs_cam"][np.sort(first)]
    assert len(order) == len(s["cams0"]) and np.array_equal(np.unique(s["obs_pt"]), np.arange(len(s["pts0"])))
    assert np.all(np.diff(s["obs_pt"]) >= 0)
    rank = np.empty(len(order), np.int32); rank[order] = np.arange(len(order), dtype=np.int32)
    return dict(s, cams0=s["cams0"][order], cam_fixed=s["cam_fixed"][order], obs_cam=rank[s["obs_cam"]]), order, rank


def check_against_the_c_abi(st, s_caller, table, out, cams_caller, pts, T, label, covariance_differs):
    init, final, iters = float(out["ba"][7]), float(out["ba"][9]), int(out["ba"][5])
    prob = B.RobustBAProblem(s_caller, table)
    c0 = prob.cost(prob.x0)
    s, order, rank = as_the_shim_numbers_it(s_caller)
    assert not np.array_equal(order, np.arange(len(order)))              # (the listing is another one: the comparison below needs it)
    cams = cams_caller[order]
    pairs = [(int(rank[a]), int(rank[b])) for a, b in CAM_PAIRS]
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"], loss=dict(table))
    summ, _ = e.solve()
    print(f"{label}: ceres.h {init:.12e} -> {final:.12e} ({iters} iterations); C ABI {summ.initial_cost:.12e} -> {summ.final_cost:.12e} "
          f"({summ.num_iterations}); reference initial cost {c0:.12e}")
    assert abs(init - c0) <= 1e-12 * c0 and final < init
    assert summ.termination_type == 0 and summ.num_iterations == iters and summ.final_cost == final
    ec, ep = e.get_params()
    assert np.array_equal(ec, cams) and np.array_equal(ep, pts)
    assert np.array_equal(cams_caller[0], s_caller["cams0"][0]) and not np.array_equal(cams_caller[1], s_caller["cams0"][1])
    f = st.BAEngine(cams, pts, s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"], loss=dict(table))
    C, P, _ = f.covariance(cam_pairs=pairs, points=LANDMARKS)
    for k in range(len(CAM_PAIRS)):
        assert np.array_equal(T[("R", k)], C[k][:3, :3]) and np.array_equal(T[("P", k)], C[k][3:, 3:]), CAM_PAIRS[k]
    for k in range(len(LANDMARKS)):
        assert np.array_equal(T[("L", k)], P[k]), LANDMARKS[k]
    C0, _, _ = st.BAEngine(cams, pts, s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"]).covariance(cam_pairs=pairs[:1])
    far = np.linalg.norm(C[0] - C0[0]) / np.linalg.norm(C0[0])
    print(f"  covariance of camera 1 against the lossless one at the same point: relative difference {far:.2e}")
    if covariance_differs:
        assert far > 1e-3


def test_huber_on_every_block_through_ceres_h(exe, tmp_path):
    st = importlib.import_module("slam-tricks_amd")
    s = B.scene("B")
    table = B.loss_table("B", "huber", len(s["obs_cam"]))
    rows = list(zip(table["kind"], table["a"], table["b"], table["scale"]))
    out, cams, pts, T = run_device(exe, tmp_path, s, rows)
    # (at the Huber solution every observation is an inlier, s <= a^2: rho' = 1 and the covariance is the lossless one -- printed only)
    check_against_the_c_abi(st, s, table, out, cams, pts, T, "huber(0.015) on every block", covariance_differs=False)


def test_scaled_cauchy_on_a_subset_through_ceres_h(exe, tmp_path):
    st = importlib.import_module("slam-tricks_amd")
    s = B.scene("B")
    n = len(s["obs_cam"])
    on = np.arange(n) % 3 == 0
    table = dict(kind=np.where(on, 3, 0).astype(np.int32), a=np.where(on, 0.015, 1.0), b=np.ones(n), scale=np.where(on, 2.0, 1.0))
    # the driver makes ScaledLoss(CauchyLoss(0.015), 2) on the subset and no loss object elsewhere
    rows = [((3 if on[k] else -1), table["a"][k], 1.0, table["scale"][k]) for k in range(n)]
    out, cams, pts, T = run_device(exe, tmp_path, s, rows)
    check_against_the_c_abi(st, s, table, out, cams, pts, T, "ScaledLoss(CauchyLoss(0.015), 2) on every third block", covariance_differs=True)
