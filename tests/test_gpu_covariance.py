"""Covariance of a bundle adjustment on the device (stba_ba_covariance_compute / _camera_covariance / _point_covariance,
BAEngine.covariance) against numpy: J^T J assembled from the oracle's per-observation Jacobians, constant columns dropped,
inverted densely.  Tolerance per block: relative Frobenius error <= 50 kappa eps, kappa = cond(J^T J) (printed)."""
import importlib
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def engine(st, s, **kw):
    return st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], s.get("pt_fixed"), **kw)


def oracle_at(O, s, cams, pts):
    return O.BA(cams, pts, s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], s.get("pt_fixed"))


def free_mask(s, nc, np_):
    cf = np.asarray(s["cam_fixed"], dtype=bool).reshape(nc, 6).reshape(-1)
    pf = np.zeros(np_, dtype=bool) if s.get("pt_fixed") is None else np.asarray(s["pt_fixed"], dtype=bool)
    return np.concatenate([~cf, np.repeat(~pf, 3)])


def numpy_covariance(O, s, cams, pts):
    """(J^T J)^-1 over the free columns, embedded with zeros at the constant ones; kappa of J^T J"""
    nc, np_ = len(cams), len(pts)
    _, _, Jc, Jp = oracle_at(O, s, cams, pts).evaluate()
    oc, op = np.asarray(s["obs_cam"]), np.asarray(s["obs_pt"])
    idx = np.concatenate([6 * oc[:, None] + np.arange(6), 6 * nc + 3 * op[:, None] + np.arange(3)], 1)     # (no, 9)
    Jo = np.concatenate([Jc, Jp], 2)                                                                    # (no, 2, 9)
    blocks = np.einsum("nki,nkj->nij", Jo, Jo)
    N = 6 * nc + 3 * np_
    H = np.zeros((N, N))
    np.add.at(H, (idx[:, :, None], idx[:, None, :]), blocks)
    f = free_mask(s, nc, np_)
    Hf = H[np.ix_(f, f)]
    ev = np.linalg.eigvalsh(Hf)
    kappa = ev[-1] / ev[0]
    Cf = np.linalg.inv(Hf)
    Cf = 0.5 * (Cf + Cf.T)
    C = np.zeros((N, N))
    C[np.ix_(f, f)] = Cf
    return C, kappa


def pivot_ratio3(H):
    """smallest / largest pivot of the LDL^T factorisation of every 3 x 3 block (0 if one is not positive)"""
    d0 = H[:, 0, 0]
    d1 = H[:, 1, 1] - H[:, 0, 1] ** 2 / d0
    e12 = H[:, 1, 2] - H[:, 0, 1] * H[:, 0, 2] / d0
    d2 = H[:, 2, 2] - H[:, 0, 2] ** 2 / d0 - e12 ** 2 / d1
    d = np.stack([d0, d1, d2], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rc = d.min(1) / d.max(1)
    return np.where((d > 0).all(1), rc, 0.0)


def rel_fro(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def check_blocks(C, nc, cam, pairs, pb, pts, kappa):
    tol = 50 * kappa * EPS
    worst = 0.0
    for (a, b), blk in zip(pairs, cam):
        ref = C[6 * a:6 * a + 6, 6 * b:6 * b + 6]
        if np.linalg.norm(ref) == 0.0:
            assert np.array_equal(blk, np.zeros((6, 6)))
            continue
        worst = max(worst, rel_fro(blk, ref))
    for j, blk in zip(pts, pb):
        o = 6 * nc + 3 * j
        ref = C[o:o + 3, o:o + 3]
        worst = max(worst, rel_fro(blk, ref))
    print(f"kappa(J^T J) = {kappa:.3e}, tolerance {tol:.3e}, worst relative Frobenius error {worst:.3e}")
    assert worst <= tol, (worst, tol)


def solved_st20(st, scenes):
    s = scenes.st20_scene()
    e = engine(st, s)
    e.solve()
    return s, e


def test_st20_after_solve_matches_numpy(st, O, scenes):
    s, e = solved_st20(st, scenes)
    cams, pts = e.get_params()
    nc, np_ = len(cams), len(pts)
    rng = np.random.default_rng(1)
    cross = [(int(a), int(b)) for a, b in rng.integers(0, nc, (10, 2))]
    pairs = [(c, c) for c in range(nc)] + cross
    cam, pb, rc = e.covariance(cam_pairs=pairs)
    C, kappa = numpy_covariance(O, s, cams, pts)
    print(f"st20 pivot ratio (first and last camera constant): {rc:.3e}")
    check_blocks(C, nc, cam, pairs, pb, range(np_), kappa)
    # constant dofs: exactly zero rows and columns
    for k, (a, b) in enumerate(pairs):
        for r in range(6):
            if s["cam_fixed"][a][r]:
                assert np.all(cam[k][r, :] == 0.0)
            if s["cam_fixed"][b][r]:
                assert np.all(cam[k][:, r] == 0.0)
    # a swapped pair is the transpose
    c2, _, _ = e.covariance(cam_pairs=[(3, 7), (7, 3)], points=[0])
    assert np.array_equal(c2[0], c2[1].T)


def test_pairs_and_dense_schur_forms_agree(st, O, scenes):
    s, e = solved_st20(st, scenes)
    cams, pts = e.get_params()
    cam1, pb1, _ = e.covariance()
    e.set_schur_mode(e.SCHUR_DENSE)
    cam2, pb2, _ = e.covariance()
    assert max(rel_fro(a, b) for a, b in zip(cam2, cam1) if np.linalg.norm(b) > 0) <= 1e-12
    assert max(rel_fro(a, b) for a, b in zip(pb2, pb1)) <= 1e-12
    C, kappa = numpy_covariance(O, s, cams, pts)
    check_blocks(C, len(cams), cam2, [(c, c) for c in range(len(cams))], pb2, range(len(pts)), kappa)


def test_repeated_camera_landmark_pairs_match_numpy(st, O, scenes):
    s = scenes.st20_scene(n_cams=12, n_pts=300, seed=11, pos_noise=0.1, ang_noise_deg=1.5, pix_noise=1e-3, half_w=3.0, half_h=3.0)
    rng = np.random.default_rng(5)
    no = len(s["obs_cam"])
    twice = rng.choice(no, 200, replace=False)
    extra = np.concatenate([twice, twice[:40]])
    s["obs_cam"] = np.concatenate([s["obs_cam"], s["obs_cam"][extra]])
    s["obs_pt"] = np.concatenate([s["obs_pt"], s["obs_pt"][extra]])
    s["obs_feat"] = np.concatenate([s["obs_feat"], s["obs_feat"][extra] + rng.normal(0, 2e-3, (len(extra), 2))])
    order = np.argsort(s["obs_pt"], kind="stable")
    for k in ("obs_cam", "obs_pt", "obs_feat"):
        s[k] = s[k][order]
    for mode in ("pairs", "dense"):
        e = engine(st, s)
        if mode == "dense":
            e.set_schur_mode(e.SCHUR_DENSE)
        cam, pb, _ = e.covariance()
        C, kappa = numpy_covariance(O, s, s["cams0"], s["pts0"])
        check_blocks(C, e.nc, cam, [(c, c) for c in range(e.nc)], pb, range(e.np_), kappa)


def test_host_lineariser_matches_device(st, O, scenes):
    s, e = solved_st20(st, scenes)
    cams, pts = e.get_params()
    cam1, pb1, _ = e.covariance()
    h = engine(st, s)
    h.set_params(cams, pts)

    def lin(c, p, want_jac):
        _, r, Jc, Jp = oracle_at(O, s, c.copy(), p.copy()).evaluate(jac=want_jac)
        return r, Jc, Jp
    h.set_host_linearizer(lin)
    cam2, pb2, _ = h.covariance()
    assert max(rel_fro(a, b) for a, b in zip(cam2, cam1) if np.linalg.norm(b) > 0) <= 1e-12
    assert max(rel_fro(a, b) for a, b in zip(pb2, pb1)) <= 1e-12


def test_compute_is_bitwise_reproducible(st, scenes):
    s, e = solved_st20(st, scenes)
    a = e.covariance(cam_pairs=[(0, 5), (5, 5), (20, 3)])
    b = e.covariance(cam_pairs=[(0, 5), (5, 5), (20, 3)])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_covariance_leaves_the_solve_unchanged(st, scenes):
    s = scenes.st20_scene()
    e1, e2 = engine(st, s), engine(st, s)
    s1, t1 = e1.solve()
    e2.covariance()
    s2, t2 = e2.solve()
    c1, p1 = e1.get_params()
    c2, p2 = e2.get_params()
    assert np.array_equal(c1, c2) and np.array_equal(p1, p2) and np.array_equal(t1, t2)
    assert s1.num_iterations == s2.num_iterations and s1.final_cost == s2.final_cost
    # and after a solve: a second solve from the same state, with and without a compute in between
    e2.covariance()
    s3, t3 = e2.solve()
    s4, t4 = e1.solve()
    assert np.array_equal(t3, t4) and np.array_equal(e1.get_params()[0], e2.get_params()[0])


def test_landmark_seen_once_is_refused(st, scenes):
    s = scenes.st20_scene()
    nc, np_ = len(s["cams0"]), len(s["pts0"])
    c = 5
    p_new = s["pts0"][0] + np.array([0.05, -0.03, 0.02])
    s["pts0"] = np.concatenate([s["pts0"], p_new[None]])
    s["obs_cam"] = np.concatenate([s["obs_cam"], [c]]).astype(np.int32)
    s["obs_pt"] = np.concatenate([s["obs_pt"], [np_]]).astype(np.int32)
    s["obs_feat"] = np.concatenate([s["obs_feat"], [[0.01, 0.02]]])
    e = engine(st, s)
    before = e.get_params()
    with pytest.raises(st.StbaError) as ei:
        e.covariance()
    print(ei.value)
    assert ei.value.code == -4 and f"landmark {np_}" in str(ei.value)
    after = e.get_params()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_sharded_engine_is_refused(st, scenes):
    s = scenes.st20_scene()
    e = engine(st, s)
    e.set_allreduce(lambda user, buf, count, stream: 0, 0, 1)
    with pytest.raises(st.StbaError) as ei:
        e.covariance()
    assert ei.value.code == -6


def test_gauge_free_scene_pivot_ratio(st, scenes):
    """report, not a promise: what the pivot test sees on the st20 scene with NO constant camera (a 7-dof gauge freedom)"""
    s, e = solved_st20(st, scenes)
    cams, pts = e.get_params()
    g = dict(s)
    g["cam_fixed"] = np.zeros_like(s["cam_fixed"])
    eg = engine(st, g)
    eg.set_params(cams, pts)
    _, _, rc_fixed = e.covariance(points=[0])
    try:
        _, _, rc_free = eg.covariance(points=[0], min_rcond=0.0)
        print(f"gauge-free st20: pivot ratio {rc_free:.3e} (fixed gauge: {rc_fixed:.3e})")
    except st.StbaError as ex:
        print(f"gauge-free st20: {ex} (fixed gauge: {rc_fixed:.3e})")
    try:
        eg.covariance(points=[0])
        print("gauge-free st20 with the default threshold 1e-14: accepted")
    except st.StbaError as ex:
        print(f"gauge-free st20 with the default threshold 1e-14: refused: {ex}")


def test_c5_full_size(st, O, scenes):
    s = scenes.st20_scene(n_cams=1000, n_pts=100000, max_obs_per_pt=10, seed=20, pix_noise=1e-3)
    # the scene has landmarks whose few views are (nearly) parallel: V_j is singular in floating point.  The engine must name them;
    # numpy's pivot ratio of the oracle's V_j agrees; then they are held constant and the rest is computed
    o = oracle_at(O, s, s["cams0"], s["pts0"])
    _, r, Jc, Jp = o.evaluate()
    Hcc, gc, Hpp, gp = o.normal_blocks(r, Jc, Jp)
    ratio = pivot_ratio3(Hpp)
    e0 = engine(st, s)
    with pytest.raises(st.StbaError) as ei:
        e0.covariance(cam_pairs=[(0, 0)], points=[0])
    e0.close()
    msg = str(ei.value)
    first = int(msg.rsplit("landmark ", 1)[1])
    print(f"C5 as generated: {msg}; numpy: {(ratio < 1e-14).sum()} below 1e-14, ratio of landmark {first}: {ratio[first]:.3e}")
    assert ei.value.code == -4 and ratio[first] < 1e-12
    weak = ratio < 1e-10
    s["pt_fixed"] = weak.astype(np.uint8)
    print(f"C5: {weak.sum()} landmarks with a pivot ratio below 1e-10 held constant")
    e = engine(st, s)
    nc, np_ = e.nc, e.np_
    t0 = time.perf_counter()
    rc_dummy = e.covariance(cam_pairs=[(0, 0)], points=[0])[2]
    t_compute_and_small = time.perf_counter() - t0
    import ctypes as C
    L = st.lib()
    rc = C.c_double()
    t0 = time.perf_counter()
    assert L.stba_ba_covariance_compute(e._h, C.c_double(1e-14), C.byref(rc)) == 0
    t_compute = time.perf_counter() - t0
    ca = np.arange(nc, dtype=np.int32)
    cam = np.zeros((nc, 6, 6))
    t0 = time.perf_counter()
    assert L.stba_ba_camera_covariance(e._h, nc, ca.ctypes.data_as(C.c_void_p), ca.ctypes.data_as(C.c_void_p), cam.ctypes.data_as(C.c_void_p)) == 0
    t_cam = time.perf_counter() - t0
    pb = np.zeros((np_, 3, 3))
    t0 = time.perf_counter()
    assert L.stba_ba_point_covariance(e._h, np_, None, pb.ctypes.data_as(C.c_void_p)) == 0
    t_pts = time.perf_counter() - t0
    print(f"C5 covariance: compute {t_compute * 1e3:.1f} ms, {nc} camera blocks {t_cam * 1e3:.1f} ms, {np_} landmark marginals "
          f"{t_pts * 1e3:.1f} ms (first call with a warm-up: {t_compute_and_small * 1e3:.1f} ms); pivot ratio {rc.value:.3e} / {rc_dummy:.3e}")
    # camera blocks: numpy's inverse of the oracle's zero-damped reduced system
    o = oracle_at(O, s, s["cams0"], s["pts0"])
    _, r, Jc, Jp = o.evaluate()
    S, _ = o.reduced_system(r, Jc, Jp, np.zeros((nc, 6)), np.zeros((np_, 3)))
    S = np.tril(S) + np.tril(S, -1).T
    f = ~np.asarray(s["cam_fixed"], dtype=bool).reshape(-1)
    Sf = S[np.ix_(f, f)]
    ev = np.linalg.eigvalsh(Sf)
    kappa = ev[-1] / ev[0]
    Sig = np.zeros_like(S)
    Sig[np.ix_(f, f)] = np.linalg.inv(Sf)
    tol = 50 * kappa * EPS
    worst = max(rel_fro(cam[c], Sig[6 * c:6 * c + 6, 6 * c:6 * c + 6]) for c in range(nc) if f[6 * c:6 * c + 6].any())
    print(f"C5 camera blocks: kappa(S) = {kappa:.3e}, worst {worst:.3e}, tolerance {tol:.3e}")
    assert worst <= tol
    # 200 landmarks through the Schur formula
    Hcc, gc, Hpp, gp = o.normal_blocks(r, Jc, Jp)
    cf = np.asarray(s["cam_fixed"], dtype=bool)
    oc, op = np.asarray(s["obs_cam"]), np.asarray(s["obs_pt"])
    start = np.searchsorted(op, np.arange(np_ + 1))
    rng = np.random.default_rng(9)
    worst = 0.0
    for j in rng.choice(np.flatnonzero(~weak), 200, replace=False):
        V = np.linalg.inv(Hpp[j])
        ks = range(start[j], start[j + 1])
        F = [np.where(cf[oc[k]][:, None], 0.0, Jc[k].T @ Jp[k]) @ V for k in ks]
        cs = [oc[k] for k in ks]
        ref = V.copy()
        for Fa, a in zip(F, cs):
            for Fb, b in zip(F, cs):
                ref += Fa.T @ Sig[6 * a:6 * a + 6, 6 * b:6 * b + 6] @ Fb
        worst = max(worst, rel_fro(pb[j], ref))
    print(f"C5 landmark marginals (200 sampled): worst {worst:.3e}, tolerance {tol:.3e}")
    assert worst <= tol


def test_landmarks_with_more_than_one_chunk_of_views(st, O, scenes):
    """cov_point_kernel stages views in chunks of 32: a landmark seen 40 times (two chunks) and one seen 70 times (three) take the
    cross-chunk pairs; the extra views are repeated observations with a little noise on the feature"""
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
    e = engine(st, s)
    cam, pb, _ = e.covariance()
    C, kappa = numpy_covariance(O, s, s["cams0"], s["pts0"])
    check_blocks(C, e.nc, cam, [(c, c) for c in range(e.nc)], pb, range(e.np_), kappa)
    for j in (a, b):
        o = 6 * e.nc + 3 * j
        print(f"landmark {j} with {n[j]} views: relative error {rel_fro(pb[j], C[o:o + 3, o:o + 3]):.3e}")


def test_pivot_ratio_against_numpy(st, O, scenes):
    """the returned rcond is min(pivot ratio of S over its free dofs, pivot ratios of the V_j); S's against numpy's Cholesky of the
    free part of the oracle's zero-damped S, and the threshold trips exactly there"""
    s, e = solved_st20(st, scenes)
    cams, pts = e.get_params()
    o = oracle_at(O, s, cams, pts)
    _, r, Jc, Jp = o.evaluate()
    nc, np_ = len(cams), len(pts)
    S, _ = o.reduced_system(r, Jc, Jp, np.zeros((nc, 6)), np.zeros((np_, 3)))
    S = np.tril(S) + np.tril(S, -1).T
    f = ~np.asarray(s["cam_fixed"], dtype=bool).reshape(-1)
    piv = np.diag(np.linalg.cholesky(S[np.ix_(f, f)])) ** 2
    r_s = piv.min() / piv.max()
    _, _, Hpp, _ = o.normal_blocks(r, Jc, Jp)
    r_l = pivot_ratio3(Hpp).min()
    _, _, rc = e.covariance(points=[0])
    print(f"st20 pivot ratios: S {r_s:.6e}, smallest V_j {r_l:.6e}, returned {rc:.6e}")
    assert abs(rc - min(r_s, r_l)) <= 1e-6 * min(r_s, r_l)
    assert r_l > 1.01 * r_s                      # (so the threshold below is S's)
    e.covariance(points=[0], min_rcond=0.999 * r_s)
    with pytest.raises(st.StbaError) as ei:
        e.covariance(points=[0], min_rcond=1.001 * r_s)
    assert ei.value.code == -4 and "reduced camera system S" in str(ei.value)
