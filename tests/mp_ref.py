"""A 50-digit reference for the project's Lie-group maths and the factors built on it (mpmath, mp.dps = 50).

Independent of oracle/oracle.c and of the device code: SO(3) is axis-angle / Rodrigues with the three coefficient functions
summed as power series below 0.1 rad (no cancellation at any angle), the logarithm is read from the rotation matrix (the
antisymmetric part below pi/2, the symmetric part above, so that it keeps its digits at 0 and at pi), and every derivative
the tests need is a central difference at h = 1e-20, exact to about 1e-30 at this precision.  Quaternions appear only at
the boundary, in the project's layout:
    pose  (qx, qy, qz, qw, tx, ty, tz)          tangent  [rho(3), theta(3)]
Matrices are 3x3 lists of mpf (6x6 and the Jacobians: mp.matrix), vectors lists of mpf; f64() rounds any of them to numpy."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
H = mp.mpf("1e-20")          # central-difference step: truncation h^2 ~ 1e-40, rounding 1e-50 / h = 1e-30
ZERO, ONE = mp.mpf(0), mp.mpf(1)


# ---------------------------------------------------------------- small linear algebra
def vec(v):
    return [mp.mpf(x) for x in v]


def eye():
    return [[ONE if i == j else ZERO for j in range(3)] for i in range(3)]


def mm(A, B):
    return [[mp.fsum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def mv(A, v):
    return [mp.fsum(A[i][k] * v[k] for k in range(3)) for i in range(3)]


def tr(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def madd(*terms):
    """sum of (coefficient, matrix) pairs"""
    return [[mp.fsum(c * M[i][j] for c, M in terms) for j in range(3)] for i in range(3)]


def chol6_T(A):
    """W = L^T (mp.matrix, upper triangular) of the symmetric positive definite A = L L^T, from A's FP64 entries as they are"""
    return mp.cholesky(mp.matrix(np.asarray(A, float).tolist())).T


def hat(v):
    return [[ZERO, -v[2], v[1]], [v[2], ZERO, -v[0]], [-v[1], v[0], ZERO]]


def norm(v):
    return mp.sqrt(mp.fsum(x * x for x in v))


def solve3(A, b):
    x = mp.lu_solve(mp.matrix(A), mp.matrix(b))
    return [x[0], x[1], x[2]]


# ---------------------------------------------------------------- SO(3)
def _series(th2, first):
    """sum_k (-1)^k th^2k / (2k + first)!  -- sin(th)/th (first=1), (1-cos th)/th^2 (2), (th-sin th)/th^3 (3)"""
    s, term, k = ZERO, ONE / mp.factorial(first), 0
    while abs(term) > mp.mpf(10) ** (-mp.mp.dps - 5):
        s += term
        k += 1
        term = -term * th2 / ((2 * k + first - 1) * (2 * k + first))
    return s


def coeffs(th):
    """(sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3) to full precision at every angle"""
    if th < mp.mpf("0.1"):
        t2 = th * th
        return _series(t2, 1), _series(t2, 2), _series(t2, 3)
    return mp.sin(th) / th, (1 - mp.cos(th)) / th ** 2, (th - mp.sin(th)) / th ** 3


def so3_exp(w):
    """Rodrigues: R = I + (sin th / th) K + ((1 - cos th) / th^2) K^2"""
    w = vec(w)
    s, a, _ = coeffs(norm(w))
    K = hat(w)
    return madd((ONE, eye()), (s, K), (a, mm(K, K)))


def left_jacobian(w):
    """V(theta) = I + ((1 - cos th) / th^2) K + ((th - sin th) / th^3) K^2: the left Jacobian of SO(3)"""
    w = vec(w)
    _, a, b = coeffs(norm(w))
    K = hat(w)
    return madd((ONE, eye()), (a, K), (b, mm(K, K)))


def so3_log(R):
    """theta in [0, pi]: atan2 of |vee(R - R^T)| / 2 = sin th and (tr R - 1) / 2 = cos th; the axis from the antisymmetric part
    below pi/2 and from the symmetric part R + R^T - 2 cos th I = 2 (1 - cos th) n n^T above it (sign from the antisymmetric part)"""
    v = [(R[2][1] - R[1][2]) / 2, (R[0][2] - R[2][0]) / 2, (R[1][0] - R[0][1]) / 2]
    c = (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    s = norm(v)
    th = mp.atan2(s, c)
    if c > 0:
        if s == 0:
            return [ZERO, ZERO, ZERO]
        return [x * th / s for x in v]
    S = [[(R[i][j] + R[j][i]) / 2 - (c if i == j else 0) for j in range(3)] for i in range(3)]
    k = max(range(3), key=lambda i: S[i][i])
    d = mp.sqrt(S[k][k] * (1 - c))
    n = [S[i][k] / d for i in range(3)]
    if mp.fsum(n[i] * v[i] for i in range(3)) < 0:
        n = [-x for x in n]
    return [x * th for x in n]


def quat_to_rot(q):
    """(x, y, z, w), normalised here: the double inputs are taken as exact, up to scale"""
    q = vec(q)
    nq = norm(q)
    x, y, z, w = (c / nq for c in q)
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def rot_to_quat(R):
    """the quaternion with qw >= 0, from the axis-angle of R"""
    w = so3_log(R)
    th = norm(w)
    if th == 0:
        return [ZERO, ZERO, ZERO, ONE]
    s = mp.sin(th / 2) / th
    return [w[0] * s, w[1] * s, w[2] * s, mp.cos(th / 2)]


def quat_from_axis_angle(w):
    th = norm(vec(w))
    if th == 0:
        return [ZERO, ZERO, ZERO, ONE]
    s = mp.sin(th / 2) / th
    return [mp.mpf(w[0]) * s, mp.mpf(w[1]) * s, mp.mpf(w[2]) * s, mp.cos(th / 2)]


# ---------------------------------------------------------------- SE(3) as (R, t)
def se3_exp(xi):
    xi = vec(xi)
    return so3_exp(xi[3:]), mv(left_jacobian(xi[3:]), xi[:3])


def se3_log(T):
    R, t = T
    w = so3_log(R)
    return solve3(left_jacobian(w), t) + w


def se3_compose(A, B):
    return mm(A[0], B[0]), [x + y for x, y in zip(mv(A[0], B[1]), A[1])]


def se3_inverse(A):
    Rt = tr(A[0])
    return Rt, [-x for x in mv(Rt, A[1])]


def pose(p):
    """(qx, qy, qz, qw, tx, ty, tz) -> (R, t)"""
    return quat_to_rot(p[:4]), vec(p[4:])


def pose7(T):
    """(R, t) -> 7 floats, qw >= 0"""
    return np.array([float(x) for x in rot_to_quat(T[0]) + T[1]])


def retract(T, d):
    """T exp(d): the right-multiplicative update of the pose graph"""
    return se3_compose(T, se3_exp(d))


# ---------------------------------------------------------------- Jacobians of SE(3)
def ad(xi):
    """ad(xi) = [[hat(theta), hat(rho)], [0, hat(theta)]]  (6x6, mp.matrix)"""
    M = mp.zeros(6, 6)
    Hr, Ht = hat(xi[:3]), hat(xi[3:])
    for i in range(3):
        for j in range(3):
            M[i, j] = Ht[i][j]; M[i, 3 + j] = Hr[i][j]; M[3 + i, 3 + j] = Ht[i][j]
    return M


def Ad(T):
    """Ad(T) = [[R, hat(t) R], [0, R]]"""
    R, t = T
    HR = mm(hat(t), R)
    M = mp.zeros(6, 6)
    for i in range(3):
        for j in range(3):
            M[i, j] = R[i][j]; M[i, 3 + j] = HR[i][j]; M[3 + i, 3 + j] = R[i][j]
    return M


def jr_inv_build(r):
    """the build-defined truncation Jr^-1(r) ~ I + ad/2 + ad^2/12"""
    A = ad(vec(r))
    return mp.eye(6) + A / 2 + A * A / 12


def jr_inv_remainder_bound(r):
    """|| Jr^-1(r) - (I + ad/2 + ad^2/12) ||_F <= T(x) with x = ||ad(r)||_F < 2 pi:  Jr^-1 = f(ad) for f(x) = x / (1 - e^-x)
    = 1 + x/2 + sum_k>=1 B_2k x^2k / (2k)!, and sum_k>=1 |B_2k| x^2k / (2k)! = 1 - (x/2) cot(x/2); the Frobenius norm is
    sub-multiplicative, so the tail from k = 2 is bounded by that series without its x^2/12 term"""
    x = mp.mnorm(ad(vec(r)), "f")
    if x >= 2 * mp.pi:
        return mp.inf
    if x == 0:
        return ZERO
    if x < mp.mpf("0.1"):
        # the same tail, summed: |B_4|/4! x^4 + |B_6|/6! x^6 + ... (no cancellation)
        s, k = ZERO, 2
        while True:
            term = abs(mp.bernoulli(2 * k)) * x ** (2 * k) / mp.factorial(2 * k)
            s += term
            if term < mp.mpf(10) ** (-mp.mp.dps - 5):
                return s
            k += 1
    return 1 - (x / 2) * mp.cot(x / 2) - x * x / 12


# ---------------------------------------------------------------- pose-graph edge
def pg_residual(Ti, Tj, Z):
    """log(Z^-1 Ti^-1 Tj) of (R, t) poses"""
    return se3_log(se3_compose(se3_inverse(Z), se3_compose(se3_inverse(Ti), Tj)))


def pg_jacobians_build(Ti, Tj, Z):
    """(r, Ji, Jj) with the build's formulas: Jj = Jr^-1(r), Ji = -Jr^-1(r) Ad(Tj^-1 Ti), Jr^-1 truncated after ad^2"""
    r = pg_residual(Ti, Tj, Z)
    Jr = jr_inv_build(r)
    return r, -(Jr * Ad(se3_compose(se3_inverse(Tj), Ti))), Jr


def num_jac(f, x0, n_out, h=H):
    """d f / d x at x0 by central differences at 50 digits (mp.matrix n_out x len(x0))"""
    J = mp.zeros(n_out, len(x0))
    for k in range(len(x0)):
        xp = list(x0); xm = list(x0)
        xp[k] += h; xm[k] -= h
        fp, fm = f(xp), f(xm)
        for i in range(n_out):
            J[i, k] = (fp[i] - fm[i]) / (2 * h)
    return J


def pg_jacobians_exact(Ti, Tj, Z):
    """d r / d delta_i and d r / d delta_j of the exact residual under T <- T exp(delta)"""
    z6 = [ZERO] * 6
    Ji = num_jac(lambda d: pg_residual(retract(Ti, d), Tj, Z), z6, 6)
    Jj = num_jac(lambda d: pg_residual(Ti, retract(Tj, d), Z), z6, 6)
    return Ji, Jj


# ---------------------------------------------------------------- st3 calibration corner
def calib_project(intr, T, X, Y):
    """pixel of the board point (X, Y, 0) seen from the view pose T = (R, t): P' = R P + t, pinhole, radial k1 k2 k3 and
    tangential p1 p2 distortion, then (alpha, beta, u0, v0)"""
    alpha, beta, u0, v0, k1, k2, k3, p1, p2 = intr
    P = [x + y for x, y in zip(mv(T[0], [mp.mpf(X), mp.mpf(Y), ZERO]), T[1])]
    xn, yn = P[0] / P[2], P[1] / P[2]
    r2 = xn * xn + yn * yn
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
    yd = yn * rad + 2 * p2 * xn * yn + p1 * (r2 + 2 * yn * yn)
    return [alpha * xd + u0, beta * yd + v0]


def calib_residual(intr, xi, X, Y, u, v):
    """e = predicted - measured, the view pose given by its tangent xi = [rho, theta]"""
    p = calib_project(vec(intr), se3_exp(xi), X, Y)
    return [p[0] - mp.mpf(u), p[1] - mp.mpf(v)]


def calib_jacobians_numeric(intr, xi, X, Y):
    """(Ji 2x9 w.r.t. the intrinsics, Jx 2x6 w.r.t. the LEFT perturbation exp(delta) T of the view pose)"""
    intr, T = vec(intr), se3_exp(xi)
    Ji = num_jac(lambda p: calib_project(p, T, X, Y), intr, 2)
    Jx = num_jac(lambda d: calib_project(intr, se3_compose(se3_exp(d), T), X, Y), [ZERO] * 6, 2)
    return Ji, Jx


def calib_jacobians_analytic(intr, xi, X, Y):
    """the same two blocks by the chain rule: d pixel / d intrinsics directly; d pixel / d P' (distortion, then pinhole)
    times d P' / d delta = [I | -hat(P')]"""
    alpha, beta, u0, v0, k1, k2, k3, p1, p2 = intr = vec(intr)
    R, t = se3_exp(xi)
    P = [x + y for x, y in zip(mv(R, [mp.mpf(X), mp.mpf(Y), ZERO]), t)]
    xn, yn = P[0] / P[2], P[1] / P[2]
    r2 = xn * xn + yn * yn
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = xn * rad + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
    yd = yn * rad + 2 * p2 * xn * yn + p1 * (r2 + 2 * yn * yn)
    Ji = mp.matrix([[xd, 0, 1, 0, alpha * xn * r2, alpha * xn * r2 ** 2, alpha * xn * r2 ** 3, 2 * alpha * xn * yn,
                     alpha * (r2 + 2 * xn * xn)],
                    [0, yd, 0, 1, beta * yn * r2, beta * yn * r2 ** 2, beta * yn * r2 ** 3, beta * (r2 + 2 * yn * yn),
                     2 * beta * xn * yn]])
    drad = 2 * k1 + 4 * k2 * r2 + 6 * k3 * r2 ** 2          # d rad / d r2 times 2
    D = mp.matrix([[rad + xn * xn * drad + 2 * p1 * yn + 6 * p2 * xn, xn * yn * drad + 2 * p1 * xn + 2 * p2 * yn],
                   [xn * yn * drad + 2 * p1 * xn + 2 * p2 * yn, rad + yn * yn * drad + 2 * p2 * xn + 6 * p1 * yn]])
    N = mp.matrix([[1 / P[2], 0, -P[0] / P[2] ** 2], [0, 1 / P[2], -P[1] / P[2] ** 2]])
    dP = mp.zeros(3, 6)
    nH = hat(P)
    for i in range(3):
        dP[i, i] = ONE
        for j in range(3):
            dP[i, 3 + j] = -nH[i][j]
    return Ji, mp.diag([alpha, beta]) * D * N * dP


# ---------------------------------------------------------------- BA reprojection (include/stba.h local order)
def ba_residual(cam, L, f):
    """x/z - f of p = R^T (L - t), cam = (qx, qy, qz, qw, tx, ty, tz) with t the camera position"""
    R, t = pose(cam)
    p = mv(tr(R), [mp.mpf(a) - b for a, b in zip(L, t)])
    return [p[0] / p[2] - mp.mpf(f[0]), p[1] / p[2] - mp.mpf(f[1])]


def _ba_rt(R, t, L):
    p = mv(tr(R), [a - b for a, b in zip(L, t)])
    return [p[0] / p[2], p[1] / p[2]]


def ba_jacobians_numeric(cam, L):
    """(Jc 2x6 w.r.t. [dtheta of q <- q (x) exp(dtheta), dt], Jp 2x3 w.r.t. L)"""
    R, t = pose(cam)
    L = vec(L)
    z6 = [ZERO] * 6
    Jc = num_jac(lambda d: _ba_rt(mm(R, so3_exp(d[:3])), [a + b for a, b in zip(t, d[3:])], L), z6, 2)
    Jp = num_jac(lambda l: _ba_rt(R, t, l), L, 2)
    return Jc, Jp


def ba_jacobians_analytic(cam, L):
    """A = d(x/z, y/z)/dp; rotation block A hat(p) (R exp(d) turns p into exp(-d) p), translation -A R^T, landmark A R^T"""
    R, t = pose(cam)
    p = mv(tr(R), [mp.mpf(a) - b for a, b in zip(L, t)])
    A = mp.matrix([[1 / p[2], 0, -p[0] / p[2] ** 2], [0, 1 / p[2], -p[1] / p[2] ** 2]])
    Jrot = A * mp.matrix(hat(p))
    Jp = A * mp.matrix(tr(R))
    Jc = mp.zeros(2, 6)
    for i in range(2):
        for j in range(3):
            Jc[i, j] = Jrot[i, j]; Jc[i, 3 + j] = -Jp[i, j]
    return Jc, Jp


# ---------------------------------------------------------------- to numpy
def f64(x):
    """mpf / list / mp.matrix -> float64 numpy array"""
    if isinstance(x, mp.matrix):
        return np.array([[float(x[i, j]) for j in range(x.cols)] for i in range(x.rows)])
    if isinstance(x, (list, tuple)):
        return np.array([f64(y) for y in x], dtype=float)
    return float(x)


def axis_angle(rng, th):
    """rotation vector of angle th about a random axis (mpf components, the angle exact to 50 digits)"""
    a = rng.normal(size=3)
    a = vec(a / np.linalg.norm(a))
    na = norm(a)
    return [x / na * mp.mpf(th) for x in a]


def quat_double(w, negate=False):
    """the quaternion of the rotation vector w, rounded to doubles (qw < 0 when negate: the same rotation)"""
    q = f64(quat_from_axis_angle(w))
    return -q if negate else q
