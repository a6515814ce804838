"""Every device buffer is freed by the object that holds it (DevBuf, csrc/common.hpp): the library's count of live buffers
(stba_live_device_buffers) around everything that allocates.

  engines      a DENSE_SCHUR and an ITERATIVE_SCHUR bundle-adjustment engine and a pose-graph engine go through every call of the
               Python wrapper that allocates (creation, the setters, the strategies, the covariances, the dense Schur form); after
               destroy the count is what it was before creation
  refusals     in the middle of the sequences: an argument check that returns a status leaves the count as it was (the pose graph's
               information check runs after its device buffers exist)
  stand-alone  cholesky_solve, calib_evaluate and the two-view initialiser hold nothing once they have returned
  results      every solve of a sequence is bitwise what the same calls give on a second, freshly created engine that sees none of
               the refusals: no buffer was freed or replaced while something still read it, and a refused call changed nothing

The shapes are the smallest that reach every allocating path: 4 cameras x 12 landmarks, every landmark seen by every camera, one
constant camera and one constant landmark (cam_fixed, pt_fixed and omask exist); a ring of 8 nodes with 2 chords, node 0 constant.
Nothing here provokes a device error: every refusal is an argument check."""
import gc
import importlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def baseline(st):
    gc.collect()          # (engines other tests dropped: their buffers go now, not in the middle of a sequence)
    return st.live_device_buffers()


class Refusals:
    """with on: the refused calls are made, and the count must not move across any of them"""

    def __init__(self, st, on):
        self.st, self.on, self.made = st, on, 0

    def refused(self, code, call, *a, **kw):
        if not self.on:
            return
        before = self.st.live_device_buffers()
        with pytest.raises(self.st.StbaError) as e:
            call(*a, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))
        assert self.st.live_device_buffers() == before, (str(e.value), before, self.st.live_device_buffers())
        self.made += 1


# ---------------------------------------------------------------- bundle adjustment
def ba_scene(scenes):
    rng = np.random.default_rng(7)
    nc, npt = 4, 12
    cams = np.zeros((nc, 7))
    for c in range(nc):
        R = scenes.axis_angle([0, 1, 0], 0.08 * (c - 1.5)) @ scenes.axis_angle([1, 0, 0], 0.05 * (c % 2))
        cams[c, :4] = scenes.quat_from_rot(R)
        cams[c, 4:] = [0.6 * (c - 1.5), 0.2 * (c % 2), 0.0]
    pts = np.stack([rng.uniform(-1.0, 1.0, npt), rng.uniform(-0.8, 0.8, npt), rng.uniform(4.0, 6.0, npt)], 1)
    obs_pt = np.repeat(np.arange(npt, dtype=np.int32), nc)          # landmark-major
    obs_cam = np.tile(np.arange(nc, dtype=np.int32), npt)
    feat, depth = scenes.project(cams, pts, obs_cam, obs_pt)
    assert (depth > 0).all()
    feat = feat + rng.normal(0.0, 2e-3, feat.shape)
    cams0 = cams.copy()
    cams0[1:, 4:] += rng.normal(0.0, 0.05, (nc - 1, 3))
    pts0 = pts + rng.normal(0.0, 0.05, pts.shape)
    cam_fixed = np.zeros((nc, 6), np.uint8)
    cam_fixed[0] = 1
    pt_fixed = np.zeros(npt, np.uint8)
    pt_fixed[3] = 1
    pts0[3] = pts[3]
    return dict(cams0=cams0, pts0=pts0, obs_cam=obs_cam, obs_pt=obs_pt, obs_feat=feat, cam_fixed=cam_fixed, pt_fixed=pt_fixed)


def ba_sequence(st, s, solver, with_refusals):
    """the whole life of one engine; returns (what every solve gave, the refusals made)"""
    INVALID, NOT_PD = -1, -4
    iterative = solver == "iterative_schur"
    rf = Refusals(st, with_refusals)
    got = []
    no = len(s["obs_cam"])

    def solved(e, label, summ):
        cams, pts = e.get_params()
        got.append((label, summ.initial_cost, summ.final_cost, summ.num_iterations, cams.tobytes(), pts.tobytes()))

    start = st.live_device_buffers()
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], cam_fixed=s["cam_fixed"], pt_fixed=s["pt_fixed"],
                    linear_solver=solver)
    assert st.live_device_buffers() > start
    solved(e, "two LM iterations", e.lm_iterations(2)[0])
    # a loss
    bad_kind = (np.full(no, 99, np.int32), np.ones(no), np.ones(no), np.ones(no))
    rf.refused(INVALID, e._set_loss_table, bad_kind)
    e.set_loss("huber", 0.01)
    rf.refused(INVALID, e._set_loss_table, bad_kind)            # (with a table held: it stays)
    assert e.has_loss
    solved(e, "loss", e.solve(max_num_iterations=4)[0])
    # information
    not_pd = np.tile(np.array([[1.0, 2.0], [2.0, 1.0]]), (no, 1, 1))
    rf.refused(NOT_PD, e.set_information, not_pd)
    e.set_information(np.array([[2.0, 0.3], [0.3, 1.5]]))
    rf.refused(NOT_PD, e.set_information, not_pd)
    assert e.has_information
    solved(e, "loss + information", e.solve(max_num_iterations=4)[0])
    e.set_loss(None)
    e.set_information(None)
    assert not e.has_loss and not e.has_information
    # pose priors: two on one camera
    prior_poses = np.stack([s["cams0"][1], s["cams0"][1]])
    prior_poses[1, 4:] += 0.01
    rf.refused(INVALID, e.set_pose_priors, [1, 4], prior_poses)
    if iterative:
        rf.refused(INVALID, e.set_pose_priors, [1, 1], prior_poses, information=4.0 * np.eye(6))
    else:
        e.set_pose_priors([1, 1], prior_poses, information=4.0 * np.eye(6))
        rf.refused(INVALID, e.set_pose_priors, [1, 4], prior_poses)
        cost, r, J = e.evaluate_pose_priors()
        assert e.pose_prior_count() == 2 and cost > 0.0 and np.abs(J).max() > 0.0
        solved(e, "pose priors", e.solve(max_num_iterations=4)[0])
        e.set_pose_priors(None, None)
        assert e.pose_prior_count() == 0
    # DOGLEG
    if iterative:
        rf.refused(INVALID, e.set_trust_region, "dogleg")
    else:
        e.set_trust_region("dogleg")
        solved(e, "dogleg", e.solve(max_num_iterations=4)[0])
    # inner iterations (DOGLEG refuses a solve with them)
    e.set_inner_iterations(True)
    if not iterative:
        rf.refused(INVALID, e.solve, max_num_iterations=4)
        e.set_trust_region("lm")
    solved(e, "inner iterations", e.solve(max_num_iterations=4)[0])
    e.set_inner_iterations(True, tolerance=1e-2)                 # (a second ordering replaces the first)
    e.set_inner_iterations(False)
    # covariance: one block of each of the four kinds
    if iterative:
        rf.refused(INVALID, e.covariance, cam_pairs=[(1, 2)], points=[0])
        rf.refused(INVALID, e.set_schur_mode, e.SCHUR_DENSE)
    else:
        cam, pb, rcond = e.covariance(cam_pairs=[(1, 2)], points=[0])
        cp, pp, _ = e.cross_covariance(cam_points=[(1, 0)], point_pairs=[(0, 1)], recompute=False)
        assert rcond > 0.0 and all(np.isfinite(x).all() and np.abs(x).max() > 0.0 for x in (cam, pb, cp, pp))
        held = st.live_device_buffers()
        e.covariance_release()
        assert st.live_device_buffers() < held
        # the dense form of the Schur complement
        e.set_schur_mode(e.SCHUR_DENSE)
        solved(e, "dense Schur form", e.solve(max_num_iterations=4)[0])
    assert st.live_device_buffers() > start
    e.close()
    assert st.live_device_buffers() == start
    return got, rf.made


@pytest.mark.parametrize("solver", ["dense_schur", "iterative_schur"])
def test_ba_engine_frees_what_it_holds(st, scenes, solver):
    s = ba_scene(scenes)
    start = baseline(st)
    got, made = ba_sequence(st, s, solver, True)
    assert st.live_device_buffers() == start
    again, _ = ba_sequence(st, s, solver, False)
    assert st.live_device_buffers() == start
    assert made >= 6 and [g[0] for g in got] == [g[0] for g in again]
    for a, b in zip(got, again):
        print(f"  {solver}: {a[0]}: cost {a[1]:.17g} -> {a[2]:.17g} in {a[3]} iterations")
        assert np.isfinite(a[2]) and a[2] <= a[1]
        assert a == b, f"{solver}: {a[0]}: a second engine gives other bits ({a[1:4]} / {b[1:4]})"


# ---------------------------------------------------------------- pose graph
def pg_scene(scenes):
    rng = np.random.default_rng(11)
    n = 8
    poses = np.zeros((n, 7))
    for i in range(n):
        a = 2 * np.pi * i / n
        poses[i, :4] = scenes.quat_from_rot(scenes.axis_angle([0, 0, 1], a + np.pi / 2))
        poses[i, 4:] = [2.0 * np.cos(a), 2.0 * np.sin(a), 0.1 * i]
    ei = np.array(list(range(n)) + [0, 2], np.int32)
    ej = np.array([(i + 1) % n for i in range(n)] + [4, 6], np.int32)
    rel = scenes._se3_mul(scenes._se3_inv(poses[ei]), poses[ej])
    noise = np.concatenate([rng.normal(0, 0.01, (len(ei), 3)), rng.normal(0, 0.002, (len(ei), 3))], 1)
    meas = np.stack([scenes._se3_mul(rel[k][None], scenes._se3_exp7(noise[k])[None])[0] for k in range(len(ei))])
    init = poses.copy()
    init[1:, 4:] += rng.normal(0, 0.05, (n - 1, 3))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return dict(poses0=init, edge_i=ei, edge_j=ej, meas=meas, node_fixed=fixed)


def pg_sequence(st, s, with_refusals):
    INVALID, NOT_PD = -1, -4
    rf = Refusals(st, with_refusals)
    got = []
    m = len(s["edge_i"])

    def solved(g, label, summ):
        got.append((label, summ.initial_cost, summ.final_cost, summ.num_iterations, g.get_poses().tobytes()))

    start = st.live_device_buffers()
    g = st.PGEngine(s["poses0"], s["edge_i"], s["edge_j"], s["meas"], node_fixed=s["node_fixed"])
    assert st.live_device_buffers() > start
    solved(g, "plain", g.solve(max_num_iterations=5)[0])
    omega = np.tile(np.diag([4.0, 4.0, 4.0, 9.0, 9.0, 9.0]), (m, 1, 1))
    omega[:, 0, 1] = omega[:, 1, 0] = 0.5
    not_pd = omega.copy()
    not_pd[7] = -np.eye(6)                  # (found by the conversion kernel: the new array and its staging exist by then)
    rf.refused(NOT_PD, g.set_information, not_pd)
    g.set_information(omega)
    rf.refused(NOT_PD, g.set_information, not_pd)
    g.set_sqrt_information(np.tile(np.diag([2.0, 2.0, 2.0, 3.0, 3.0, 3.0]), (m, 1, 1)))
    rf.refused(INVALID, g.set_loss, 99, 1.0)
    g.set_loss("cauchy", 0.5)
    rf.refused(INVALID, g.set_loss, 99, 1.0)
    assert g.has_information and g.has_loss
    solved(g, "sqrt information + loss", g.solve(max_num_iterations=5)[0])
    g.set_loss(None)
    g.set_sqrt_information(None)
    g.set_information(None)
    assert not g.has_information and not g.has_loss
    held = st.live_device_buffers()
    blocks, _ = g.covariance([(1, 2)])
    cols, _ = g.covariance_columns(3)
    assert np.isfinite(blocks).all() and np.isfinite(cols).all() and np.abs(blocks).max() > 0.0
    assert st.live_device_buffers() == held
    solved(g, "plain again", g.solve(max_num_iterations=5)[0])
    g.close()
    assert st.live_device_buffers() == start
    return got, rf.made


def test_pg_engine_frees_what_it_holds(st, scenes):
    s = pg_scene(scenes)
    start = baseline(st)
    got, made = pg_sequence(st, s, True)
    assert st.live_device_buffers() == start
    again, _ = pg_sequence(st, s, False)
    assert st.live_device_buffers() == start
    assert made == 4 and [g[0] for g in got] == [g[0] for g in again]
    for a, b in zip(got, again):
        print(f"  pose graph: {a[0]}: cost {a[1]:.17g} -> {a[2]:.17g} in {a[3]} iterations")
        assert np.isfinite(a[2]) and a[2] <= a[1]
        assert a == b, f"pose graph: {a[0]}: a second engine gives other bits ({a[1:4]} / {b[1:4]})"


# ---------------------------------------------------------------- stand-alone entry points
def test_stand_alone_calls_hold_nothing_afterwards(st, scenes, known):
    from conftest import GOLDEN
    start = baseline(st)
    # a 5 x 5 SPD system
    rng = np.random.default_rng(5)
    M = rng.normal(size=(5, 5))
    A = M @ M.T + 5.0 * np.eye(5)
    rhs = rng.normal(size=5)
    x = st.cholesky_solve(A, rhs)
    assert np.abs(A @ x - rhs).max() <= 1e-12 * np.abs(rhs).max() * np.linalg.cond(A)
    assert st.live_device_buffers() == start
    # the calibration kernel on the recorded corner files
    d = os.path.join(GOLDEN, "st3_calib")
    img = []
    for f in sorted(n for n in os.listdir(d) if n.endswith(".txt")):
        rows, cols, xy = st.corners_read(os.path.join(d, f))
        img.append(xy.reshape(-1, 2))
    img = np.array(img)
    jj, ii = np.meshgrid(np.arange(cols), np.arange(rows))
    board = np.stack([jj.reshape(-1), ii.reshape(-1)], 1) * known["st3_calibration"]["board_square_m"]
    obj = np.repeat(board[None], len(img), 0)
    p0, _ = st.zhang_init(obj, img)
    assert st.live_device_buffers() == start
    sse, e, Ji, Jx = st.calib_evaluate(p0, obj, img)
    assert np.isfinite(sse) and abs(sse - float((e ** 2).sum())) <= 1e-9 * sse and np.abs(Ji).max() > 0.0 and np.abs(Jx).max() > 0.0
    assert st.live_device_buffers() == start
    # the two-view initialiser on 8 correspondences
    c = scenes.two_view_pairs(n_pts=8)
    g = st.two_view_init(c["f1"], c["f2"], c["K"])
    assert list(g["fails"]).count(0) == 1 and abs(np.linalg.det(g["R"]) - 1.0) <= 1e-12 and g["pts"].shape == (8, 3)
    assert st.live_device_buffers() == start
