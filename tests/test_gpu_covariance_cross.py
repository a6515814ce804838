"""The off-diagonal blocks of a bundle adjustment's covariance on the device (stba_ba_camera_point_covariance,
stba_ba_point_pair_covariance, BAEngine.cross_covariance): camera-landmark 6 x 3 blocks and the 3 x 3 blocks of two different
landmarks, against the dense inverse tests/test_gpu_covariance.py builds in numpy (numpy_covariance).  Tolerance per block, as
there: relative Frobenius error <= 50 kappa eps, kappa = cond(J^T J) (printed); the worst error is printed per kind of block."""
import ctypes as C
import importlib

import numpy as np
import pytest

from test_gpu_covariance import EPS, engine, free_mask, numpy_covariance, rel_fro, solved_st20

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def covariance_of(s, nc, np_, Jc, Jp):
    """numpy_covariance on given per-observation Jacobians (the caller's observation order)"""
    oc, op = np.asarray(s["obs_cam"]), np.asarray(s["obs_pt"])
    idx = np.concatenate([6 * oc[:, None] + np.arange(6), 6 * nc + 3 * op[:, None] + np.arange(3)], 1)
    Jo = np.concatenate([Jc, Jp], 2)
    N = 6 * nc + 3 * np_
    H = np.zeros((N, N))
    np.add.at(H, (idx[:, :, None], idx[:, None, :]), np.einsum("nki,nkj->nij", Jo, Jo))
    f = free_mask(s, nc, np_)
    Hf = H[np.ix_(f, f)]
    ev = np.linalg.eigvalsh(Hf)
    Cf = np.linalg.inv(Hf)
    Cm = np.zeros((N, N))
    Cm[np.ix_(f, f)] = 0.5 * (Cf + Cf.T)
    return Cm, ev[-1] / ev[0]


def ref_cp(Cm, nc, a, j):
    return Cm[6 * a:6 * a + 6, 6 * nc + 3 * j:6 * nc + 3 * j + 3]


def ref_pp(Cm, nc, j, k):
    return Cm[6 * nc + 3 * j:6 * nc + 3 * j + 3, 6 * nc + 3 * k:6 * nc + 3 * k + 3]


def check_cross(label, Cm, nc, kappa, cam_points, cp, point_pairs, pp):
    """every block against numpy's; a block that is zero in numpy (a constant camera or landmark) must be exactly zero"""
    tol = 50 * kappa * EPS
    worst = {"camera-landmark": 0.0, "landmark-landmark": 0.0}
    zeros = 0
    for kind, req, got, ref_of in (("camera-landmark", cam_points, cp, ref_cp), ("landmark-landmark", point_pairs, pp, ref_pp)):
        assert len(got) == len(req)
        for (a, b), blk in zip(req, got):
            ref = ref_of(Cm, nc, a, b)
            if np.linalg.norm(ref) == 0.0:
                assert np.array_equal(blk, np.zeros_like(ref)), (kind, a, b)
                zeros += 1
                continue
            worst[kind] = max(worst[kind], rel_fro(blk, ref))
    print(f"{label}: kappa(J^T J) = {kappa:.3e}, tolerance {tol:.3e}, worst relative Frobenius error camera-landmark "
          f"{worst['camera-landmark']:.3e} ({len(cam_points)} blocks), landmark-landmark {worst['landmark-landmark']:.3e} "
          f"({len(point_pairs)} blocks), {zeros} exactly zero")
    assert max(worst.values()) <= tol, (worst, tol)


def distinct_pairs(rng, n, count):
    a = rng.integers(0, n, count)
    b = (a + rng.integers(1, n, count)) % n
    return [(int(x), int(y)) for x, y in zip(a, b)]


@pytest.fixture(scope="module")
def st20(st, O, scenes):
    """the solved st20 scene, its engine and numpy's covariance at the solution (shared, left unchanged)"""
    s, e = solved_st20(st, scenes)
    cams, pts = e.get_params()
    Cm, kappa = numpy_covariance(O, s, cams, pts)
    return dict(s=s, e=e, cams=cams, pts=pts, C=Cm, kappa=kappa)


def test_st20_after_solve_matches_numpy(st20):
    s, e, Cm, kappa = st20["s"], st20["e"], st20["C"], st20["kappa"]
    nc, np_ = e.nc, e.np_
    assert np.all(s["cam_fixed"][0]) and np.all(s["cam_fixed"][nc - 1])
    cam_list = [0, nc - 1, 3, 7, 12]
    assert not np.any(s["cam_fixed"][[3, 7, 12]])
    cam_points = [(a, j) for a in cam_list for j in range(np_)]
    point_pairs = distinct_pairs(np.random.default_rng(2), np_, 300)
    cp, pp, rc = e.cross_covariance(cam_points=cam_points, point_pairs=point_pairs)
    assert cp.shape == (len(cam_points), 6, 3) and pp.shape == (300, 3, 3) and rc > 0
    check_cross("st20", Cm, nc, kappa, cam_points, cp, point_pairs, pp)
    for (a, _), blk in zip(cam_points, cp):
        if a in (0, nc - 1):
            assert np.array_equal(blk, np.zeros((6, 3)))


def test_swapped_pairs_are_transposes_and_the_diagonal_is_the_marginal(st20):
    e, Cm, kappa = st20["e"], st20["C"], st20["kappa"]
    nc, np_ = e.nc, e.np_
    fwd = distinct_pairs(np.random.default_rng(4), np_, 50)
    swp = [(b, a) for a, b in fwd]
    _, pp, _ = e.cross_covariance(point_pairs=fwd + swp)
    for k in range(len(fwd)):
        assert np.array_equal(pp[k], pp[len(fwd) + k].T), fwd[k]
    # a landmark with itself, alone and among others: the marginal, bit for bit
    js = [0, 17, np_ - 1]
    _, pb, _ = e.covariance(cam_pairs=[(0, 0)], points=js)
    _, pd, _ = e.cross_covariance(point_pairs=[(j, j) for j in js])
    assert np.array_equal(pd, pb)
    mixed = [fwd[0], (17, 17), fwd[1], (0, 0), (np_ - 1, np_ - 1), swp[0]]
    _, pm, _ = e.cross_covariance(point_pairs=mixed)
    assert np.array_equal(pm[1], pb[1]) and np.array_equal(pm[3], pb[0]) and np.array_equal(pm[4], pb[2])
    assert np.array_equal(pm[0], pp[0]) and np.array_equal(pm[2], pp[1]) and np.array_equal(pm[5], pp[len(fwd)])
    # camera-landmark blocks against the transposed block of numpy's symmetric C
    tol = 50 * kappa * EPS
    cam_points = [(5, 11), (9, 300), (14, np_ - 1)]
    cp, _, _ = e.cross_covariance(cam_points=cam_points, recompute=False)
    worst = 0.0
    for (a, j), blk in zip(cam_points, cp):
        lower = Cm[6 * nc + 3 * j:6 * nc + 3 * j + 3, 6 * a:6 * a + 6]          # C[landmark, camera]
        worst = max(worst, rel_fro(blk.T, lower))
    print(f"camera-landmark blocks against C[landmark, camera]^T: worst {worst:.3e}, tolerance {tol:.3e}")
    assert worst <= tol


def heavy_scene(scenes):
    """the scene of test_gpu_covariance.test_landmarks_with_more_than_one_chunk_of_views: landmarks with 40 and 70 views"""
    s = scenes.st20_scene()
    rng = np.random.default_rng(3)
    cnt = np.bincount(s["obs_pt"])
    a, b = np.argsort(-cnt, kind="stable")[:2]
    extra = []
    for j, target in ((a, 40), (b, 70)):
        own = np.flatnonzero(s["obs_pt"] == j)
        extra.append(rng.choice(own, target - len(own), replace=True))
    extra = np.concatenate(extra)
    s["obs_cam"] = np.concatenate([s["obs_cam"], s["obs_cam"][extra]])
    s["obs_pt"] = np.concatenate([s["obs_pt"], s["obs_pt"][extra]])
    s["obs_feat"] = np.concatenate([s["obs_feat"], s["obs_feat"][extra] + rng.normal(0, 1e-3, (len(extra), 2))])
    order = np.argsort(s["obs_pt"], kind="stable")
    for k in ("obs_cam", "obs_pt", "obs_feat"):
        s[k] = s[k][order]
    n = np.bincount(s["obs_pt"])
    assert n[a] == 40 and n[b] == 70
    return s, int(a), int(b), n


def test_more_than_one_trip_and_more_than_one_chunk(st, O, scenes):
    """70 views: two trips of 64 lanes in cov_cam_point_kernel; 40 and 70 views: two and three chunks of 32 in cov_point_pair_kernel"""
    s, a, b, n = heavy_scene(scenes)
    # an ordinary landmark to pair the heavy ones with: the most viewed of the others (8 views; the scene has none with 10)
    others = n.copy()
    others[[a, b]] = 0
    light = int(np.argmax(others))
    assert 8 <= n[light] <= 10
    e = engine(st, s)
    point_pairs = [(a, b), (b, a), (a, light), (light, a), (b, light), (light, b)]
    cam_points = [(c, j) for c in range(e.nc) for j in (a, b)]
    cp, pp, _ = e.cross_covariance(cam_points=cam_points, point_pairs=point_pairs)
    Cm, kappa = numpy_covariance(O, s, s["cams0"], s["pts0"])
    check_cross(f"landmarks with {n[a]} and {n[b]} views (and one with {n[light]})", Cm, e.nc, kappa, cam_points, cp, point_pairs, pp)
    assert np.array_equal(pp[0], pp[1].T) and np.array_equal(pp[2], pp[3].T) and np.array_equal(pp[4], pp[5].T)


def test_repeated_observations_in_both_schur_modes(st, O, scenes):
    """the scene of test_gpu_covariance.test_repeated_camera_landmark_pairs_match_numpy: a camera that sees a landmark twice (or
    three times) contributes once per observation"""
    s = scenes.st20_scene(n_cams=12, n_pts=300, seed=11, pos_noise=0.1, ang_noise_deg=1.5, pix_noise=1e-3, half_w=3.0, half_h=3.0)
    rng = np.random.default_rng(5)
    no = len(s["obs_cam"])
    twice = rng.choice(no, 200, replace=False)
    extra = np.concatenate([twice, twice[:40]])
    repeated = sorted(set(int(j) for j in s["obs_pt"][extra]))
    s["obs_cam"] = np.concatenate([s["obs_cam"], s["obs_cam"][extra]])
    s["obs_pt"] = np.concatenate([s["obs_pt"], s["obs_pt"][extra]])
    s["obs_feat"] = np.concatenate([s["obs_feat"], s["obs_feat"][extra] + rng.normal(0, 2e-3, (len(extra), 2))])
    order = np.argsort(s["obs_pt"], kind="stable")
    for k in ("obs_cam", "obs_pt", "obs_feat"):
        s[k] = s[k][order]
    Cm, kappa = numpy_covariance(O, s, s["cams0"], s["pts0"])
    prs = np.random.default_rng(6)
    point_pairs = distinct_pairs(prs, 300, 200) + [(repeated[k], repeated[k + 1]) for k in range(0, 40, 2)]
    cam_points = [(c, j) for c in range(12) for j in repeated[:40]]
    for mode in ("pairs", "dense"):
        e = engine(st, s)
        if mode == "dense":
            e.set_schur_mode(e.SCHUR_DENSE)
        cp, pp, _ = e.cross_covariance(cam_points=cam_points, point_pairs=point_pairs)
        check_cross(f"repeated observations, Schur mode {mode}", Cm, 12, kappa, cam_points, cp, point_pairs, pp)


def test_partly_constant_camera_dofs_and_a_constant_landmark(st, O, scenes):
    s = scenes.st20_scene()
    s["cam_fixed"] = np.array(s["cam_fixed"], dtype=np.uint8).reshape(-1, 6).copy()
    s["cam_fixed"][3, 3] = 1
    s["cam_fixed"][4, :3] = 1
    np_ = len(s["pts0"])
    s["pt_fixed"] = np.zeros(np_, dtype=np.uint8)
    s["pt_fixed"][7] = 1
    e = engine(st, s)
    nc = e.nc
    cam_points = [(a, j) for a in (2, 3, 4) for j in range(0, np_, 5)] + [(a, 7) for a in range(nc)]
    point_pairs = [(7, k) for k in (0, 8, 100)] + [(k, 7) for k in (0, 8, 100)] + distinct_pairs(np.random.default_rng(8), np_, 100)
    cp, pp, _ = e.cross_covariance(cam_points=cam_points, point_pairs=point_pairs)
    Cm, kappa = numpy_covariance(O, s, s["cams0"], s["pts0"])
    check_cross("partly constant dofs, landmark 7 constant", Cm, nc, kappa, cam_points, cp, point_pairs, pp)
    for (a, j), blk in zip(cam_points, cp):
        if a == 3:
            assert np.array_equal(blk[3], np.zeros(3))
        if a == 4:
            assert np.array_equal(blk[:3], np.zeros((3, 3)))
        if j == 7:
            assert np.array_equal(blk, np.zeros((6, 3)))
    for (j, k), blk in zip(point_pairs, pp):
        if j == 7 or k == 7:
            assert np.array_equal(blk, np.zeros((3, 3)))


def test_losses_and_information_matrices(st, scenes):
    """the cross blocks are made from the engine's own corrected and whitened Jacobians: against numpy on evaluate()'s, and
    against an engine that gets those Jacobians from a host lineariser"""
    s, e0 = solved_st20(st, scenes)
    cams, pts = e0.get_params()
    s = dict(s, cams0=cams, pts0=pts)
    no = len(s["obs_cam"])
    rng = np.random.default_rng(12)
    A = rng.normal(0, 0.4, (no, 2, 2))
    information = np.einsum("nij,nkj->nik", A, A) + np.eye(2) * rng.uniform(0.5, 2.0, no)[:, None, None]
    e = engine(st, s, loss=("huber", 0.03), information=information)
    assert e.has_loss and e.has_information
    _, r, Jc, Jp = e.evaluate()
    nc, np_ = e.nc, e.np_
    Cm, kappa = covariance_of(s, nc, np_, Jc, Jp)
    cam_points = [(a, j) for a in (0, 2, 9, 15) for j in range(0, np_, 3)]
    point_pairs = distinct_pairs(np.random.default_rng(13), np_, 200)
    cp, pp, _ = e.cross_covariance(cam_points=cam_points, point_pairs=point_pairs)
    check_cross("huber(0.03) and per-observation information", Cm, nc, kappa, cam_points, cp, point_pairs, pp)
    # the plain engine at the same point has another covariance by far
    cp0, pp0, _ = e0.cross_covariance(cam_points=cam_points, point_pairs=point_pairs)
    far = max(rel_fro(a, b) for a, b in zip(pp0, pp))
    print(f"the unweighted, lossless blocks differ by up to {far:.3e} relative")
    assert far > 1e3 * 50 * kappa * EPS
    # a host-lineariser engine fed with the same Jacobians
    h = engine(st, s)
    h.set_host_linearizer(lambda c, p, want_jac: (r, Jc, Jp))
    cph, pph, _ = h.cross_covariance(cam_points=cam_points, point_pairs=point_pairs)
    dc = max(rel_fro(a, b) for a, b in zip(cph, cp) if np.linalg.norm(b) > 0)
    dp = max(rel_fro(a, b) for a, b in zip(pph, pp))
    print(f"host lineariser against the device engine: camera-landmark {dc:.3e}, landmark-landmark {dp:.3e}")
    assert dc <= 1e-12 and dp <= 1e-12
    for a, b in zip(cph, cp):
        if np.linalg.norm(b) == 0:
            assert np.array_equal(a, b)


def test_bitwise_reproducible_and_the_solve_is_left_alone(st, scenes):
    s = scenes.st20_scene()
    e1, e2 = engine(st, s), engine(st, s)
    cam_points, point_pairs = [(3, 5), (0, 9), (11, 599)], [(1, 2), (2, 1), (5, 5), (400, 17)]
    a = e2.cross_covariance(cam_points=cam_points, point_pairs=point_pairs)
    b = e2.cross_covariance(cam_points=cam_points, point_pairs=point_pairs)
    c = e2.cross_covariance(cam_points=cam_points, point_pairs=point_pairs, recompute=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and c[2] is None
    s1, t1 = e1.solve()
    s2, t2 = e2.solve()
    c1, p1 = e1.get_params()
    c2, p2 = e2.get_params()
    assert np.array_equal(c1, c2) and np.array_equal(p1, p2) and np.array_equal(t1, t2)
    assert s1.num_iterations == s2.num_iterations and s1.final_cost == s2.final_cost


SENTINEL = 7.25


def raw_calls(st, e, cam, pt, pa, pb):
    """both getters through ctypes on sentinel-filled buffers -> (status, buffer) each"""
    L = st.lib()
    out = []
    for fn, x, y, width in ((L.stba_ba_camera_point_covariance, cam, pt, 18), (L.stba_ba_point_pair_covariance, pa, pb, 9)):
        x, y = np.ascontiguousarray(x, np.int32), np.ascontiguousarray(y, np.int32)
        buf = np.full(len(x) * width, SENTINEL)
        out.append((fn(e._h, len(x), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)), buf))
    return out


def test_refusals(st, scenes):
    s = scenes.st20_scene()
    e = engine(st, s)
    nc, np_ = e.nc, e.np_
    # no compute
    with pytest.raises(st.StbaError) as ei:
        e.cross_covariance(cam_points=[(1, 1)], recompute=False)
    assert ei.value.code == -6
    with pytest.raises(st.StbaError) as ei:
        e.cross_covariance(point_pairs=[(1, 2)], recompute=False)
    assert ei.value.code == -6
    for status, buf in raw_calls(st, e, [1], [1], [1], [2]):
        assert status == -6 and np.all(buf == SENTINEL)
    # index out of range, the position named, nothing written
    e.covariance(cam_pairs=[(0, 0)], points=[0])
    for bad in ([(1, 1), (2, 2), (nc, 3)], [(1, 1), (2, 2), (3, np_)], [(1, 1), (2, 2), (-1, 3)], [(1, 1), (2, 2), (3, -1)]):
        with pytest.raises(st.StbaError) as ei:
            e.cross_covariance(cam_points=bad, recompute=False)
        print(ei.value)
        assert ei.value.code == -1 and "pair 2" in str(ei.value)
    for bad in ([(1, 2), (np_, 3)], [(1, 2), (3, np_)], [(1, 2), (-1, 3)], [(1, 2), (3, -1)]):
        with pytest.raises(st.StbaError) as ei:
            e.cross_covariance(point_pairs=bad, recompute=False)
        print(ei.value)
        assert ei.value.code == -1 and "pair 1" in str(ei.value)
    (s1, b1), (s2, b2) = raw_calls(st, e, [1, nc], [1, 1], [1, 2], [2, np_])
    assert s1 == -1 and s2 == -1 and np.all(b1 == SENTINEL) and np.all(b2 == SENTINEL)
    L = st.lib()
    one = np.zeros(1, np.int32)
    buf = np.full(18, SENTINEL)
    assert L.stba_ba_camera_point_covariance(e._h, 1, None, one.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)) == -1
    assert L.stba_ba_point_pair_covariance(e._h, 1, one.ctypes.data_as(C.c_void_p), None, buf.ctypes.data_as(C.c_void_p)) == -1
    assert np.all(buf == SENTINEL)
    assert L.stba_ba_camera_point_covariance(e._h, 0, None, None, None) == 0 and L.stba_ba_point_pair_covariance(e._h, 0, None, None, None) == 0
    # the compute's own refusals, as before: an ITERATIVE_SCHUR engine and an engine with an all-reduce hook
    it = engine(st, s, linear_solver="iterative_schur")
    with pytest.raises(st.StbaError) as ei:
        it.cross_covariance(cam_points=[(1, 1)])
    assert ei.value.code == -1
    for status, buf in raw_calls(st, it, [1], [1], [1], [2]):
        assert status == -6 and np.all(buf == SENTINEL)
    sh = engine(st, s)
    sh.set_allreduce(lambda user, buf, count, stream: 0, 0, 1)
    with pytest.raises(st.StbaError) as ei:
        sh.cross_covariance(point_pairs=[(1, 2)])
    assert ei.value.code == -6
    for status, buf in raw_calls(st, sh, [1], [1], [1], [2]):
        assert status == -6 and np.all(buf == SENTINEL)
