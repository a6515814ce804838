"""The device kernels that carry the SE(3) maths against the 50-digit reference tests/mp_ref.py, not against oracle/oracle.c:
the oracle restates the same formulas, so a mistake the two share (the literal (1 - cos theta) / theta^2 of the SO(3) left
Jacobian, 0 instead of 1/2 where cos theta rounds to 1) passes every HIP-vs-oracle comparison.  Angles walk the ladder of
tests/test_lie_reference.py through each factor:
  (a) the pose-graph edge kernel (pg_linearize_kernel, through PGEngine.evaluate): r = log(Z^-1 Ti^-1 Tj), the cost, Ji and Jj
      against the build-defined formula and against the exact derivative within the series remainder;
  (b) the calibration kernel (calib_linearize_kernel, through calib_evaluate): e, Ji and Jx;
  (c) the BA linearisation (through BAEngine.evaluate): r, Jc and Jp -- a guard, its helpers do not involve V(theta).

Tolerances are EPS times the scale of the quantity times a small factor.  The factors were set from the CPU oracle, which
runs the same double arithmetic as the kernels: it lands within a few units of each scale, and the factors below leave 2x-4x
room for FMA contraction and a different libm on the device."""
import importlib

import mpmath as mp
import numpy as np
import pytest

import mp_ref as M
from test_lie_reference import LADDER, tangent

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
TRANS = [1e3, 1.0, 1e-6, 0.0]        # residual translations; the first edge has the largest, so a lost block partial shows
N_BASE = 256                          # unique edges: ladder (16) x residual translation (4) x what walks (2) x placement (2)


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0
    return mod


# ---------------------------------------------------------------- (a) pose-graph edges
def pg_base_edges():
    """N_BASE edges, edge k between nodes 2k and 2k + 1, with
    th = LADDER[k % 16], residual translation TRANS[(k // 16) % 4],
    what walks the ladder: (k // 64) % 2 == 0 the residual rotation, 1 the relative rotation Ti^-1 Tj (near pi included,
    where pg_edge flips the sign of the residual quaternion),
    placement: (k // 128) % 2 == 0 nodes near the origin, 1 nodes around 1e4 m.
    Returns poses (2 N_BASE, 7), meas (N_BASE, 7), fixed (2 N_BASE,) uint8"""
    rng = np.random.default_rng(2024)
    poses = np.zeros((2 * N_BASE, 7))
    meas = np.zeros((N_BASE, 7))
    for k in range(N_BASE):
        th, tr = LADDER[k % 16], TRANS[(k // 16) % 4]
        walk_rel, far = (k // 64) % 2 == 1, (k // 128) % 2 == 1
        centre = rng.normal(size=3) * (1e4 if far else 1.0)
        Ti = M.se3_exp(M.vec(np.concatenate([np.zeros(3), M.f64(M.axis_angle(rng, 0.9))])))
        Ti = (Ti[0], M.vec(centre))
        if walk_rel:
            A = M.se3_exp(M.vec(tangent(k, th, 2.0)))
            res = tangent(k + 1000, mp.mpf("1e-3"), tr)
        else:
            A = M.se3_exp(M.vec(np.concatenate([rng.normal(size=3), M.f64(M.axis_angle(rng, 1.1))])))
            res = tangent(k + 1000, th, tr)
        Z = M.se3_compose(A, M.se3_exp(M.vec(-res)))     # Z^-1 Ti^-1 Tj = exp(res), up to the rounding of the inputs
        pi, pj, z = M.pose7(Ti), M.pose7(M.se3_compose(Ti, A)), M.pose7(Z)
        # quaternions with qw < 0 on some of the inputs: the same rotations
        if k % 3 == 1:
            pi[:4] = -pi[:4]
        if k % 3 == 2:
            z[:4] = -z[:4]
        poses[2 * k], poses[2 * k + 1], meas[k] = pi, pj, z
    fixed = np.zeros(2 * N_BASE, np.uint8)
    fixed[0::10] = 1          # node i of every fifth edge
    fixed[7::14] = 1          # node j of every seventh edge, from edge 3
    return poses, meas, fixed


@pytest.fixture(scope="module")
def pg_ref():
    """per base edge: r, Ji, Jj by the build's formula, Ji, Jj exact (None where the series bound is not small), the bound"""
    poses, meas, fixed = pg_base_edges()
    out = []
    for k in range(N_BASE):
        Ti, Tj, Z = M.pose(poses[2 * k]), M.pose(poses[2 * k + 1]), M.pose(meas[k])
        r, Ji, Jj = M.pg_jacobians_build(Ti, Tj, Z)
        bound = M.jr_inv_remainder_bound(r)
        Jie = Jje = None
        if bound < mp.mpf("1e-4"):
            Jie, Jje = M.pg_jacobians_exact(Ti, Tj, Z)
            Jie, Jje = M.f64(Jie), M.f64(Jje)
        Ad = M.f64(M.Ad(M.se3_compose(M.se3_inverse(Tj), Ti)))
        out.append(dict(r=M.f64(r), Ji=M.f64(Ji), Jj=M.f64(Jj), Jie=Jie, Jje=Jje, bound=float(bound), Ad=Ad))
    return poses, meas, fixed, out


def pg_graph(poses, meas, fixed, m):
    """m edges over the base edges, edge e = base edge e % N_BASE (edge N_BASE repeats edge 0 on the same two nodes)"""
    nb = min(m, N_BASE)
    e = np.arange(m) % N_BASE
    return poses[: 2 * nb], (2 * e).astype(np.int32), (2 * e + 1).astype(np.int32), meas[e], fixed[: 2 * nb]


def check_pg(poses, meas, fixed, ref, m, cost, r, Ji, Jj):
    base = np.arange(m) % N_BASE
    n_exact = 0
    cost_ref = 0.0
    for e in range(m):
        k = base[e]
        R = ref[k]
        ti, tj, tz = poses[2 * k, 4:], poses[2 * k + 1, 4:], meas[k, 4:]
        # the translations enter through compositions of poses of size |t|: rounding of order EPS |t| each
        scale_t = 1.0 + np.abs(ti).sum() + np.abs(tj).sum() + np.abs(tz).sum()
        rn = np.linalg.norm(R["r"])
        # r: rotation part to 16 EPS absolute (the residual quaternion is a product of unit quaternions, each exact to EPS);
        # translation part to 16 EPS scale_t
        d = np.abs(r[e] - R["r"])
        assert d[3:].max() <= 16 * EPS * (1 + rn), (e, k, r[e], R["r"])
        assert d[:3].max() <= 16 * EPS * (scale_t + rn), (e, k, d, scale_t, r[e], R["r"])
        cost_ref += 0.5 * float(np.dot(R["r"], R["r"]))
        # Jacobians: ad(r) is linear in r, so an error dr moves Jr^-1 by ~|dr| (1 + |r|); Ad(Tj^-1 Ti) adds its own
        # rounding times |Jr^-1|.  Their scale: (1 + |r|)^2 (1 + |Ad|)
        scale_j = (1 + rn) ** 2 * (1 + np.abs(R["Ad"]).max()) * (scale_t + rn)
        tol_j = 16 * EPS * scale_j
        fi, fj = fixed[2 * k], fixed[2 * k + 1]
        if fi:
            assert not Ji[e].any(), e
        else:
            assert np.abs(Ji[e] - R["Ji"]).max() <= tol_j, (e, k, np.abs(Ji[e] - R["Ji"]).max(), tol_j)
        if fj:
            assert not Jj[e].any(), e
        else:
            assert np.abs(Jj[e] - R["Jj"]).max() <= tol_j, (e, k, np.abs(Jj[e] - R["Jj"]).max(), tol_j)
        # against the exact derivative: the build truncates Jr^-1 after ad^2, within the Bernoulli tail bound
        # (mp_ref.jr_inv_remainder_bound, checked against the exact derivative in test_lie_reference.py)
        if R["Jie"] is not None:
            n_exact += 1
            if not fj:
                assert np.linalg.norm(Jj[e] - R["Jje"]) <= R["bound"] + 6 * tol_j, (e, k)
            if not fi:
                assert np.linalg.norm(Ji[e] - R["Jie"]) <= R["bound"] * np.linalg.norm(R["Ad"]) + 6 * tol_j, (e, k)
    # the cost: per-block partials summed on the device; 1e-13 relative covers the double sum of m terms of 1e6 at most
    assert abs(cost - cost_ref) <= 1e-13 * cost_ref, (cost, cost_ref)
    assert abs(cost - 0.5 * float((r[:m] ** 2).sum())) <= 1e-13 * cost_ref
    return n_exact


@pytest.mark.parametrize("m", [1, 255, 256, 257])
def test_pg_edges_against_reference(st, pg_ref, m):
    poses, meas, fixed, ref = pg_ref
    P, ei, ej, Z, fx = pg_graph(poses, meas, fixed, m)
    eng = st.PGEngine(P, ei, ej, Z, fx)
    cost, r, Ji, Jj = eng.evaluate()
    eng.close()
    n_exact = check_pg(poses, meas, fixed, ref, m, cost, r, Ji, Jj)
    if m >= N_BASE:
        assert n_exact >= 64        # every edge of the relative-rotation walk with a small residual


# ---------------------------------------------------------------- (b) calibration corners
INTR = np.array([500.0, 480.0, 320.0, 240.0, -0.2, 0.05, -0.01, 1e-3, -2e-3])


def calib_problem():
    """one view per rung and depth: the view rotation walks the ladder, the board (4 x 5 corners over 0.2 x 0.25 m, Z = 0)
    sits 0.3, 1 or 3 m in front of the camera; img = the 50-digit projection plus 0.5 px of noise"""
    rng = np.random.default_rng(77)
    xis, depths = [], [0.3, 1.0, 3.0]
    for k, th in enumerate(LADDER):
        for depth in depths:
            w = M.axis_angle(rng, th)
            R = M.so3_exp(w)
            # the board's centre (0.1, 0.125, 0) lands at (dx, dy, depth)
            want = M.vec([rng.uniform(-0.05, 0.05) * depth, rng.uniform(-0.05, 0.05) * depth, depth])
            t = [a - b for a, b in zip(want, M.mv(R, M.vec([0.1, 0.125, 0.0])))]
            rho = M.solve3(M.left_jacobian(w), t)
            xis.append(M.f64(rho + w))
    xis = np.array(xis)
    jj, ii = np.meshgrid(np.arange(5) * 0.05, np.arange(4) * (0.25 / 3))
    board = np.stack([jj.reshape(-1), ii.reshape(-1)], 1)
    V = len(xis)
    obj = np.repeat(board[None], V, 0)
    img = np.zeros_like(obj)
    for v in range(V):
        T = M.se3_exp(M.vec(xis[v]))
        for c in range(len(board)):
            img[v, c] = M.f64(M.calib_project(M.vec(INTR), T, *board[c])) + rng.normal(0, 0.5, 2)
    return np.concatenate([INTR, xis.reshape(-1)]), obj, img


@pytest.fixture(scope="module")
def calib_ref():
    params, obj, img = calib_problem()
    V, Cn = obj.shape[:2]
    e = np.zeros((V, Cn, 2)); Ji = np.zeros((V, Cn, 2, 9)); Jx = np.zeros((V, Cn, 2, 6))
    for v in range(V):
        xi = params[9 + 6 * v: 15 + 6 * v]
        for c in range(Cn):
            e[v, c] = M.f64(M.calib_residual(INTR, xi, *obj[v, c], *img[v, c]))
            a, b = M.calib_jacobians_numeric(INTR, xi, *obj[v, c])
            Ji[v, c], Jx[v, c] = M.f64(a), M.f64(b)
    return params, obj, img, e, Ji, Jx


def check_calib(calib_ref, sse, e, Ji, Jx):
    params, obj, img, e_ref, Ji_ref, Jx_ref = calib_ref
    # e: pixels of magnitude ~1e3 (alpha xd + u0); 64 EPS of that is 1.4e-11 px.  The literal form is off by up to ~5e-7 px
    assert np.abs(e - e_ref).max() <= 64 * EPS * 1e3, np.abs(e - e_ref).max()
    assert abs(sse - float((e_ref ** 2).sum())) <= 1e-12 * float((e_ref ** 2).sum())
    # Jacobians row by row, relative to the row's largest entry
    for J, Jr in ((Ji, Ji_ref), (Jx, Jx_ref)):
        row = np.abs(Jr).max(-1, keepdims=True)
        assert (np.abs(J - Jr) <= 64 * EPS * row).all(), (np.abs(J - Jr) / row).max()


def test_calib_against_reference(st, calib_ref):
    params, obj, img = calib_ref[:3]
    sse, e, Ji, Jx = st.calib_evaluate(params, obj, img)
    check_calib(calib_ref, sse, e, Ji, Jx)


# ---------------------------------------------------------------- (c) BA reprojection (guard)
def ba_problem():
    """one camera per rung (qw < 0 on every other), 8 landmarks each: depths 1e-3 .. 1e5 along directions up to 3 off the
    axis, the camera centres up to 1e3 from the origin; each landmark seen once, by its camera"""
    rng = np.random.default_rng(55)
    cams, pts, oc, op, feat = [], [], [], [], []
    depths = [1e-3, 1e-2, 1.0, 10.0, 1e3, 1e5, 3.0, 0.5]
    for k, th in enumerate(LADDER):
        q = M.quat_double(M.axis_angle(rng, th), negate=(k % 2 == 1))
        cam = np.concatenate([q, rng.normal(size=3) * (1e3 if k % 3 == 0 else 1.0)])
        R, t = M.pose(cam)
        for z in depths:
            u, v = rng.uniform(-3, 3, 2)
            L = M.f64([a + b for a, b in zip(M.mv(R, M.vec([u * z, v * z, z])), t)])
            oc.append(len(cams)); op.append(len(pts))
            pts.append(L)
            feat.append(np.array([u, v]) + rng.normal(0, 1e-3, 2))
        cams.append(cam)
    return np.array(cams), np.array(pts), np.array(oc, np.int32), np.array(op, np.int32), np.array(feat)


@pytest.fixture(scope="module")
def ba_ref():
    cams, pts, oc, op, feat = ba_problem()
    n = len(oc)
    r = np.zeros((n, 2)); Jc = np.zeros((n, 2, 6)); Jp = np.zeros((n, 2, 3)); kappa = np.zeros(n)
    for o in range(n):
        r[o] = M.f64(M.ba_residual(cams[oc[o]], pts[op[o]], feat[o]))
        a, b = M.ba_jacobians_numeric(cams[oc[o]], pts[op[o]])
        Jc[o], Jp[o] = M.f64(a), M.f64(b)
        R, t = M.pose(cams[oc[o]])
        p = M.f64(M.mv(M.tr(R), [mp.mpf(x) - y for x, y in zip(pts[op[o]], t)]))
        kappa[o] = np.linalg.norm(p) / abs(p[2])
    return cams, pts, oc, op, feat, r, Jc, Jp, kappa


def check_ba(ba_ref, cost, r, Jc, Jp):
    cams, pts, oc, op, feat, r_ref, Jc_ref, Jp_ref, kappa = ba_ref
    # p = R^T (L - t) carries EPS |L - t| per coordinate; x/z then EPS kappa (kappa = |p| / z, up to ~4.4 here), and so do
    # the Jacobians relative to their rows (A = d(x/z)/dp has rows of size kappa / z)
    k = kappa[:, None]
    assert (np.abs(r - r_ref) <= 32 * EPS * k * k).all(), (np.abs(r - r_ref) / (k * k)).max() / EPS
    for J, Jr in ((Jc, Jc_ref), (Jp, Jp_ref)):
        row = np.abs(Jr).max(-1)
        assert (np.abs(J - Jr).max(-1) <= 32 * EPS * kappa[:, None] ** 2 * row).all(), \
            (np.abs(J - Jr).max(-1) / (kappa[:, None] ** 2 * row)).max() / EPS
    c_ref = 0.5 * float((r_ref ** 2).sum())
    assert abs(cost - c_ref) <= 1e-12 * c_ref


def test_ba_linearize_against_reference(st, ba_ref):
    cams, pts, oc, op, feat = ba_ref[:5]
    eng = st.BAEngine(cams, pts, oc, op, feat)
    cost, r, Jc, Jp = eng.evaluate()
    eng.close()
    check_ba(ba_ref, cost, r, Jc, Jp)
