"""SO(3) / SE(3) of the CPU oracle (oracle/oracle.c) and of slam-tricks_amd/scenes.py against the 50-digit reference
tests/mp_ref.py, on an angle ladder that walks every branch and every cancellation of the closed forms: 0, the 1e-10
switch of the small-angle series, the band 1e-10 .. 2e-8 where cos(theta) rounds to 1, the band up to 1e-5 where
(1 - cos theta) / theta^2 loses its leading digits, and the two approaches to pi.  A round trip exp -> log cannot see a
mistake that exp and log share; a comparison with the reference can.  The first tests check the reference itself.

Tolerances are in units of the double epsilon times the scale of the quantity: |theta| for a rotation vector, 1 for a unit
quaternion, |rho| or |t| for a translation.  A correct double implementation lands within a few epsilon of the reference
(measured: at most 3.5 eps on these cases, scenes.se3_log near pi); 8 eps leaves room for a libm that rounds differently,
and is still 1/300 of what the literal (1 - cos theta) / theta^2 got wrong at theta = 1e-5 (5e-13 |rho|)."""
import mpmath as mp
import numpy as np
import pytest

import mp_ref as M

EPS = np.finfo(float).eps
ULPS = 8
TOL = ULPS * EPS
LADDER = [mp.mpf(0), mp.mpf("1e-14"), mp.mpf("9.9e-11"), mp.mpf("1.01e-10"), mp.mpf("1e-9"), mp.mpf("1e-8"),
          mp.mpf("3e-8"), mp.mpf("1e-7"), mp.mpf("1e-6"), mp.mpf("1e-5"), mp.mpf("1e-3"), mp.mpf("0.1"), mp.mpf(1),
          mp.mpf(3), mp.pi - mp.mpf("1e-6"), mp.pi - mp.mpf("1e-9")]
RHO = [0.0, 1e-6, 1.0, 1e3]
LADDER_IDS = [mp.nstr(t, 4) for t in LADDER]


def tangent(seed, th, rho):
    """a double tangent [rho, theta]: random axis, angle th, |rho| = rho"""
    rng = np.random.default_rng(seed)
    w = M.f64(M.axis_angle(rng, th))
    r = rng.normal(size=3)
    return np.concatenate([r / np.linalg.norm(r) * rho, w])


def qdist(a, b):
    """distance of two unit quaternions as rotations (q and -q are one rotation)"""
    return min(np.abs(a - b).max(), np.abs(a + b).max())


def quat_of(T):
    return M.f64(M.rot_to_quat(T[0]))


def err_ratio(got, want, scale):
    """max |got - want| in units of EPS * scale (scale 0: the exact answer is wanted)"""
    d = np.abs(np.asarray(got, float) - np.asarray(want, float)).max()
    return d / (EPS * scale) if scale > 0 else (0.0 if d == 0 else np.inf)


# ---------------------------------------------------------------- the reference checks itself
@pytest.mark.parametrize("th", LADDER, ids=LADDER_IDS)
def test_mp_ref_roundtrips(th):
    for k, rho in enumerate(RHO):
        xi = M.vec(tangent(k, th, rho))
        back = M.se3_log(M.se3_exp(xi))
        assert max(abs(a - b) for a, b in zip(back, xi)) <= mp.mpf("1e-40") * max(1, rho)
        R = M.so3_exp(xi[3:])
        assert max(abs(a - b) for a, b in zip(M.so3_log(M.quat_to_rot(M.rot_to_quat(R))), xi[3:])) <= mp.mpf("1e-40")
        # R is orthogonal to the working precision
        RtR = M.mm(M.tr(R), R)
        assert max(abs(RtR[i][j] - (1 if i == j else 0)) for i in range(3) for j in range(3)) <= mp.mpf("1e-45")
    # the series and the closed forms agree where they meet
    for th0 in (mp.mpf("0.1"), mp.mpf("0.0999999")):
        for s, c in zip(M.coeffs(th0), (mp.sin(th0) / th0, (1 - mp.cos(th0)) / th0 ** 2, (th0 - mp.sin(th0)) / th0 ** 3)):
            assert abs(s - c) <= mp.mpf("1e-44")


def test_mp_ref_jacobians_analytic_vs_numeric():
    """the reference's chain-rule Jacobians of the calibration corner and the BA reprojection against its own 50-digit
    central differences (exact to ~1e-30)"""
    rng = np.random.default_rng(3)
    intr = [500.0, 480.0, 320.0, 240.0, -0.2, 0.05, -0.01, 1e-3, -2e-3]
    for th in LADDER:
        xi = tangent(int(rng.integers(1 << 30)), th, 1.0)
        xi[:3] = xi[:3] * 0.1 + np.array([0.0, 0.0, 1.0])
        X, Y = rng.uniform(-0.2, 0.2, 2)
        Ji_n, Jx_n = M.calib_jacobians_numeric(intr, xi, X, Y)
        Ji_a, Jx_a = M.calib_jacobians_analytic(intr, xi, X, Y)
        assert mp.mnorm(Ji_n - Ji_a, 1) <= mp.mpf("1e-25") * mp.mnorm(Ji_a, 1)
        assert mp.mnorm(Jx_n - Jx_a, 1) <= mp.mpf("1e-25") * mp.mnorm(Jx_a, 1)
        cam = np.concatenate([M.quat_double(M.axis_angle(rng, th), negate=bool(rng.integers(2))), rng.normal(size=3)])
        R, t = M.pose(cam)
        L = M.f64([a + b for a, b in zip(M.mv(R, M.vec([0.3, -0.2, 2.0])), t)])
        Jc_n, Jp_n = M.ba_jacobians_numeric(cam, L)
        Jc_a, Jp_a = M.ba_jacobians_analytic(cam, L)
        assert mp.mnorm(Jc_n - Jc_a, 1) <= mp.mpf("1e-25") * mp.mnorm(Jc_a, 1)
        assert mp.mnorm(Jp_n - Jp_a, 1) <= mp.mpf("1e-25") * mp.mnorm(Jp_a, 1)


@pytest.mark.parametrize("th", LADDER, ids=LADDER_IDS)
def test_mp_ref_edge_jacobian_within_remainder(th):
    """the build's truncated Jr^-1 = I + ad/2 + ad^2/12 against the exact derivative of the exact residual:
    ||Jj - Jj_exact||_F <= T(||ad(r)||_F) and ||Ji - Ji_exact||_F <= T(||ad(r)||_F) ||Ad(Tj^-1 Ti)||_F, with T the tail of the
    Bernoulli series (mp_ref.jr_inv_remainder_bound), plus 1e-28 for the central differences.  The relative rotation walks the
    ladder; the residual is a small, fixed twist, so that the bound is finite and tight"""
    rng = np.random.default_rng(11)
    Ti = M.se3_exp(M.vec(np.concatenate([rng.normal(size=3), M.f64(M.axis_angle(rng, 0.7))])))
    A = M.se3_exp(M.vec(tangent(5, th, 2.0)))
    Tj = M.se3_compose(Ti, A)
    for resid in (np.zeros(6), np.array([1e-6, -2e-6, 3e-6, 1e-7, 2e-7, -1e-7]), np.array([0.02, -0.01, 0.03, 0.01, -0.02, 0.015])):
        Z = M.se3_compose(A, M.se3_exp(M.vec(-resid)))
        r, Ji, Jj = M.pg_jacobians_build(Ti, Tj, Z)
        Jie, Jje = M.pg_jacobians_exact(Ti, Tj, Z)
        bound = M.jr_inv_remainder_bound(r)
        assert bound < mp.mpf("1e-6")
        assert mp.mnorm(Jj - Jje, "f") <= bound + mp.mpf("1e-28")
        assert mp.mnorm(Ji - Jie, "f") <= bound * mp.mnorm(M.Ad(M.se3_compose(M.se3_inverse(Tj), Ti)), "f") + mp.mpf("1e-28")
        # and the bound is not vacuous: the largest residual moves the Jacobian by about its x^4/720 term, far above the
        # 1e-28 of the differences
        if resid[0] > 0.01:
            assert mp.mnorm(Jj - Jje, "f") >= bound / 1e3


# ---------------------------------------------------------------- the oracle and scenes.py against the reference
@pytest.mark.parametrize("th", LADDER, ids=LADDER_IDS)
def test_oracle_so3_against_reference(O, th):
    for seed in range(3):
        w = tangent(seed, th, 0.0)[3:]
        q_ref = M.f64(M.quat_from_axis_angle(M.vec(w)))
        q = O.so3_exp(w)
        assert err_ratio(q, q_ref, 1.0) <= ULPS, (q, q_ref)
        # log of the double quaternion, given with qw >= 0 and with qw < 0 (the same rotation)
        w_ref = M.f64(M.so3_log(M.quat_to_rot(q)))
        th_d = float(np.linalg.norm(w_ref))
        for sgn in (1.0, -1.0):
            assert err_ratio(O.so3_log(sgn * q), w_ref, th_d) <= ULPS, (sgn, O.so3_log(sgn * q), w_ref)


@pytest.mark.parametrize("th", LADDER, ids=LADDER_IDS)
def test_oracle_se3_exp_log_against_reference(O, th):
    for k, rho in enumerate(RHO):
        xi = tangent(k, th, rho)
        T = M.se3_exp(M.vec(xi))
        q, t = O.se3_exp(xi)
        assert qdist(q, quat_of(T)) <= TOL
        assert err_ratio(t, M.f64(T[1]), rho) <= ULPS, (float(th), rho, t, M.f64(T[1]))
        # log of a double pose, with qw >= 0 and qw < 0
        qd, td = quat_of(T), M.f64(T[1])
        ref = M.f64(M.se3_log(M.pose(np.concatenate([qd, td]))))
        for sgn in (1.0, -1.0):
            got = O.se3_log(sgn * qd, td)
            assert err_ratio(got[3:], ref[3:], float(np.linalg.norm(ref[3:]))) <= ULPS, (sgn, got, ref)
            assert err_ratio(got[:3], ref[:3], rho) <= ULPS, (float(th), rho, sgn, got[:3], ref[:3])


@pytest.mark.parametrize("th", LADDER, ids=LADDER_IDS)
def test_oracle_se3_group_ops_against_reference(O, th):
    """compose, inverse and the right retraction T exp(d) of 7-double poses; a with a rotation on the ladder, b with qw < 0,
    translations up to 1e3"""
    rng = np.random.default_rng(7)
    for k, rho in enumerate(RHO):
        a = np.concatenate([M.quat_double(M.axis_angle(rng, th), negate=(k % 2 == 1)), rng.normal(size=3) * rho])
        b = np.concatenate([M.quat_double(M.axis_angle(rng, 1.3), negate=True), rng.normal(size=3) * (rho + 1)])
        Ta, Tb = M.pose(a), M.pose(b)
        scale = np.abs(a[4:]).sum() + np.abs(b[4:]).sum()
        c = O.se3_compose(a, b)
        ref = M.se3_compose(Ta, Tb)
        assert qdist(c[:4], quat_of(ref)) <= TOL and err_ratio(c[4:], M.f64(ref[1]), scale) <= ULPS
        ai = O.se3_inverse(a)
        ref = M.se3_inverse(Ta)
        assert qdist(ai[:4], quat_of(ref)) <= TOL and err_ratio(ai[4:], M.f64(ref[1]), scale) <= ULPS
        # retract by a step whose rotation walks the ladder: T exp(d)
        d = tangent(k + 10, th, rho)
        e = O.se3_retract(b, d)
        ref = M.retract(Tb, M.vec(d))
        scale = np.abs(b[4:]).sum() + rho
        assert qdist(e[:4], quat_of(ref)) <= TOL
        assert err_ratio(e[4:], M.f64(ref[1]), scale) <= ULPS, (float(th), rho, e[4:], M.f64(ref[1]))


@pytest.mark.parametrize("th", LADDER, ids=LADDER_IDS)
def test_scenes_se3_against_reference(scenes, th):
    for k, rho in enumerate(RHO):
        xi = tangent(k, th, rho)
        T = M.se3_exp(M.vec(xi))
        R, t = scenes.se3_exp(xi)
        assert err_ratio(R, M.f64(T[0]), 1.0) <= ULPS
        assert err_ratio(t, M.f64(T[1]), rho) <= ULPS, (float(th), rho, t, M.f64(T[1]))
        # log of the double (R, t): the reference takes R as given (orthogonal to ~1e-16)
        Rd, td = M.f64(T[0]), M.f64(T[1])
        ref = M.f64(M.se3_log((M.tr(M.tr([M.vec(row) for row in Rd])), M.vec(td))))
        got = scenes.se3_log(Rd, td)
        th_d = float(np.linalg.norm(ref[3:]))
        assert err_ratio(got[3:], ref[3:], max(th_d, 1e-300)) <= ULPS or np.abs(got[3:] - ref[3:]).max() <= 4 * EPS, (got, ref)
        assert err_ratio(got[:3], ref[:3], rho) <= ULPS, (float(th), rho, got[:3], ref[:3])
