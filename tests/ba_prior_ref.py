"""Reference for the camera pose priors of the bundle adjustment (include/stba.h).  CPU only.

A prior k on camera c: r = [Log(qh^-1 (x) q_c); t_c - th] in the order [rot(3), pos(3)], J = blockdiag(Jr^-1(r_theta), I) under the
chart q <- q (x) exp(dtheta), t <- t + dt; whitened r' = W r, J' = W J; the cost gains 1/2 |r'|^2.

Two evaluations of one prior:
  prior_eval_mp   50 digits, on tests/mp_ref.py: the quaternions are taken as exact up to scale, Log is read from the rotation
                  matrix R(qh)^T R(q) (mp_ref.so3_log), and Jr^-1 is the INVERSE (an LU solve at 50 digits) of the right Jacobian
                  Jr(phi) = V(-phi), mp_ref.left_jacobian: no closed form of the inverse enters.
  prior_eval_np   float64, scalar: a restatement of the factor as the library documents it -- the quaternion product in a fixed
                  order, theta = 2 atan2(|v|, w) behind the sign choice w >= 0, the coefficient of hat(phi)^2 as
                  (1 - (theta / 2) cot(theta / 2)) / theta^2 with cot(theta / 2) = w / |v| (its series below 0.1 rad).
The error of prior_eval_np against prior_eval_mp on an input is the yardstick of the device's on the same input (the GPU test).

The problems: PriorBAProblem (lm_step_ref.BAProblem) and PriorWeightedBAProblem (ba_information_ref.WeightedBAProblem: whitened
and corrected observations) append the whitened prior rows to r and J -- three residual blocks of two rows per prior, on the
camera's six columns (and, to keep the blocks' shape, landmark 0's three with zeros) -- so that lm_step_ref.lm_reference /
ba_loss_ref.lm_reference, tolerances and compare apply unchanged."""
import functools
import math

import mpmath as mp
import numpy as np

import ba_information_ref as I
import ba_loss_ref as B
import lm_step_ref as L
import mp_ref as M

EPS = L.EPS
LD = np.longdouble
SERIES_THETA = 0.1
# the angle of qh^-1 q the accuracy tests run at (each also with q -> -q)
ANGLES = ("0", "1e-12", "1e-8", "1e-4", "0.3", "1.5", "3.0", "pi-1e-6")


def angle_value(name):
    return mp.pi - mp.mpf("1e-6") if name == "pi-1e-6" else mp.mpf(name)


# ------------------------------------------------------------------------------------------ one prior, float64
def prior_eval_np(pose, cam, W, fixed=None):
    """(r'[6], J'[6, 6]) of one prior in float64; fixed[6]: the camera's constant dofs (their columns are exactly 0)"""
    qh, q = [float(v) for v in pose[:4]], [float(v) for v in cam[:4]]
    ax, ay, az, aw = -qh[0], -qh[1], -qh[2], qh[3]
    bx, by, bz, bw = q
    x = (aw * bx + ax * bw) + (ay * bz - az * by)
    y = (aw * by + ay * bw) + (az * bx - ax * bz)
    z = (aw * bz + az * bw) + (ax * by - ay * bx)
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    lead = x if x != 0.0 else (y if y != 0.0 else z)
    if w < 0.0 or (w == 0.0 and lead < 0.0):
        x, y, z, w = -x, -y, -z, -w
    n2 = (x * x + y * y) + z * z
    n = math.sqrt(n2)
    if n2 < 1e-40:
        k, cot = 2.0 / w, 0.0
    else:
        k, cot = 2.0 * math.atan2(n, w) / n, w / n
    p = np.array([k * x, k * y, k * z])
    th = k * n
    t2 = th * th
    if th < SERIES_THETA:
        c = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 * (1.0 / 1209600.0 + t2 * (1.0 / 47900160.0))))
    else:
        c = (1.0 - (0.5 * th) * cot) / t2
    pp = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    h = np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])
    J = np.eye(6)
    for a in range(3):
        for b in range(3):
            d = 1.0 if a == b else 0.0
            J[a, b] = (d + 0.5 * h[a, b]) + c * (p[a] * p[b] - pp * d)
    r = np.concatenate([p, np.asarray(cam[4:], float) - np.asarray(pose[4:], float)])
    W = np.asarray(W, float).reshape(6, 6)
    rw = np.array([((((W[i, 0] * r[0] + W[i, 1] * r[1]) + W[i, 2] * r[2]) + W[i, 3] * r[3]) + W[i, 4] * r[4]) + W[i, 5] * r[5]
                   for i in range(6)])
    Jw = np.zeros((6, 6))
    for i in range(6):
        for a in range(6):
            Jw[i, a] = (W[i, 0] * J[0, a] + W[i, 1] * J[1, a]) + W[i, 2] * J[2, a] if a < 3 else W[i, a]
    if fixed is not None:
        Jw[:, np.asarray(fixed, bool)] = 0.0
    return rw, Jw


# ------------------------------------------------------------------------------------------ one prior, 50 digits
def prior_eval_mp(pose, cam, W, fixed=None):
    """(r'[6], J'[6, 6]) as lists of mpf / mp.matrix, the double inputs taken as exact (the quaternions up to scale)"""
    Rh, R = M.quat_to_rot(pose[:4]), M.quat_to_rot(cam[:4])
    phi = M.so3_log(M.mm(M.tr(Rh), R))
    Jr = M.left_jacobian([-v for v in phi])
    Jri = mp.inverse(mp.matrix(Jr))
    r = list(phi) + [mp.mpf(float(cam[4 + k])) - mp.mpf(float(pose[4 + k])) for k in range(3)]
    J = mp.eye(6)
    for a in range(3):
        for b in range(3):
            J[a, b] = Jri[a, b]
    Wm = mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(W, float).reshape(6, 6)])
    rw = Wm * mp.matrix(r)
    Jw = Wm * J
    if fixed is not None:
        for a in range(6):
            if fixed[a]:
                for i in range(6):
                    Jw[i, a] = M.ZERO
    return [rw[i] for i in range(6)], Jw


def floors(W, pose, cam):
    """4 eps x (row's sum |W_jk| |entry_k|) for r'[6] and J'[6, 6], the entries those of the 50-digit evaluation at W = I"""
    r, J = prior_eval_mp(pose, cam, np.eye(6))
    aW = np.abs(np.asarray(W, float).reshape(6, 6))
    return 4 * EPS * aW @ np.abs(M.f64(r)), 4 * EPS * aW @ np.abs(M.f64(J))


def err_vs_mp(got_r, got_J, ref_r, ref_J):
    """|double - 50-digit| per entry, formed at 50 digits"""
    er = np.array([float(abs(mp.mpf(float(got_r[i])) - ref_r[i])) for i in range(6)])
    eJ = np.array([[float(abs(mp.mpf(float(got_J[i, a])) - ref_J[i, a])) for a in range(6)] for i in range(6)])
    return er, eJ


def pose_at_angle(cam, name, rng):
    """a prior pose[7] in doubles whose qh^-1 q has the angle `name` (up to the rounding of qh) for the camera pose cam[7]:
    qh = q (x) exp(-phi) formed at 50 digits and rounded, phi of that angle about a random axis; angle 0: qh is q's bits"""
    th = angle_value(name)
    q = np.asarray(cam[:4], float)
    if th == 0:
        qh = q.copy()
    else:
        e = M.quat_from_axis_angle([-v for v in M.axis_angle(rng, th)])
        a = M.vec(q)
        qh = M.f64([a[3] * e[0] + a[0] * e[3] + a[1] * e[2] - a[2] * e[1], a[3] * e[1] - a[0] * e[2] + a[1] * e[3] + a[2] * e[0],
                    a[3] * e[2] + a[0] * e[1] - a[1] * e[0] + a[2] * e[3], a[3] * e[3] - a[0] * e[0] - a[1] * e[1] - a[2] * e[2]])
    return np.concatenate([qh, np.asarray(cam[4:], float) - 0.1 * rng.normal(size=3)])


def angle_pair(name, seed, negate=False):
    """(pose[7], cam[7]): a random camera pose (unit quaternion to rounding; -q when negate) and a prior at that angle from it"""
    rng = np.random.default_rng(seed)
    cam = np.concatenate([M.quat_double(M.axis_angle(rng, rng.uniform(0.2, 2.5))), rng.normal(size=3)])
    pose = pose_at_angle(cam, name, rng)
    if negate:
        cam[:4] = -cam[:4]
    return pose, cam


def random_W(rng, n=1):
    """full random square-root informations (entries of order 1, no structure)"""
    return rng.normal(size=(n, 6, 6))


def position_only_W(n=1, sigma=0.05):
    """a GPS prior: zero rotation rows, the position rows I / sigma"""
    W = np.zeros((n, 6, 6))
    W[:, 3:, 3:] = np.eye(3) / sigma
    return W


def random_spd(rng, n, rot_sigma=0.02, pos_sigma=0.05):
    """random symmetric positive definite 6 x 6 information matrices: a random rotation of diag(1 / sigma^2), sigmas spread 3x"""
    out = np.zeros((n, 6, 6))
    for k in range(n):
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        sig = np.concatenate([rot_sigma * 3.0 ** rng.uniform(-1, 1, 3), pos_sigma * 3.0 ** rng.uniform(-1, 1, 3)])
        # (mixing only inside the rotation and the position triple keeps the two units apart)
        Q[:3, 3:] = Q[3:, :3] = 0.0
        Q[:3, :3], _ = np.linalg.qr(Q[:3, :3]); Q[3:, 3:], _ = np.linalg.qr(Q[3:, 3:])
        A = Q @ np.diag(1.0 / sig ** 2) @ Q.T
        out[k] = 0.5 * (A + A.T)
    return out


def sqrt_of_information(Om):
    """W = L^T of Omega = L L^T (float64 Cholesky: the reference's own factor; the engine's is within 4 eps of the exact one)"""
    return np.stack([np.linalg.cholesky(o).T for o in np.asarray(Om, float).reshape(-1, 6, 6)])


# ------------------------------------------------------------------------------------------ the problems
def normalise_like_the_host(q):
    """include/stba.h: quaternions are normalised on the host, one that is unit to 8 eps keeps its bits.  The same operations, so
    that the reference holds the bits the engine holds (a quaternion moved by eps moves Log by eps ABSOLUTE, whatever its size)"""
    q = np.asarray(q, float)
    n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    sc = np.where(np.abs(n2 - 1.0) <= 8 * EPS, 1.0, 1.0 / np.sqrt(n2))
    return q * sc[:, None]


class PriorMixin:
    """adds priors (cams[n], poses[n, 7], W[n, 6, 6]) to a BA problem: lin appends their whitened rows, cost their 1/2 |r'|^2"""

    def set_priors(self, cams, poses, W):
        self.pr_cam = np.asarray(cams, np.int64).reshape(-1)
        self.pr_pose = np.asarray(poses, float).reshape(-1, 7).copy()
        self.pr_pose[:, :4] = normalise_like_the_host(self.pr_pose[:, :4])
        n = len(self.pr_cam)
        self.pr_W = np.broadcast_to(np.eye(6), (n, 6, 6)).copy() if W is None else np.broadcast_to(np.asarray(W, float), (n, 6, 6)).copy()
        k9 = np.concatenate([np.arange(6), 6 * self.nc + np.arange(3)])
        self.pr_cols = np.repeat((6 * self.pr_cam[:, None] * (np.arange(9) < 6) + k9[None, :]), 3, axis=0)
        return self

    def lin_priors(self, cams, jac=True):
        """(r'[n, 6], J'[n, 6, 6]) at the cameras `cams`, columns of constant dofs zero"""
        n = len(self.pr_cam)
        r, J = np.zeros((n, 6)), np.zeros((n, 6, 6))
        for k in range(n):
            c = self.pr_cam[k]
            r[k], J[k] = prior_eval_np(self.pr_pose[k], cams[c], self.pr_W[k], self.cam_fixed[c])
        return r, (J if jac else None)

    def lin(self, x, jac=True):
        r, J, cols = super().lin(x, jac)
        cams, _ = self.split(x)
        rp, Jp = self.lin_priors(cams, jac)
        r = np.concatenate([r, rp.reshape(-1, 2)])
        if jac:
            J9 = np.zeros((len(rp), 6, 9))
            J9[:, :, :6] = Jp
            J = np.concatenate([J, J9.reshape(-1, 2, 9)])
        return r, J, np.concatenate([cols, self.pr_cols])

    def prior_cost(self, x):
        cams, _ = self.split(x)
        return float(0.5 * np.sum(self.lin_priors(cams, False)[0].astype(LD) ** 2))

    def blocks(self, x):
        """(sum J'^T J' [nc, 6, 6], sum J'^T r' [nc, 6], and the sums of |terms| of both) of the priors per camera, in longdouble"""
        cams, _ = self.split(x)
        rp, Jp = self.lin_priors(cams)
        H, g = np.zeros((self.nc, 6, 6), LD), np.zeros((self.nc, 6), LD)
        Ha, ga = np.zeros((self.nc, 6, 6), LD), np.zeros((self.nc, 6), LD)
        JL, rL = Jp.astype(LD), rp.astype(LD)
        for k, c in enumerate(self.pr_cam):
            H[c] += JL[k].T @ JL[k]; g[c] += JL[k].T @ rL[k]
            Ha[c] += np.abs(JL[k]).T @ np.abs(JL[k]); ga[c] += np.abs(JL[k]).T @ np.abs(rL[k])
        return H, g, Ha, ga


class PriorBAProblem(PriorMixin, L.BAProblem):
    def __init__(self, s, cams, poses, W, cam_fixed="scene"):
        cf = s["cam_fixed"] if isinstance(cam_fixed, str) else cam_fixed
        L.BAProblem.__init__(self, s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], cf, s.get("pt_fixed"))
        self.set_priors(cams, poses, W)


class PriorWeightedBAProblem(PriorMixin, I.WeightedBAProblem):
    """whitened and corrected observations (ba_information_ref) plus priors: cost = 1/2 sum rho + 1/2 sum |r'|^2"""

    def __init__(self, s, Wobs, table, cams, poses, W):
        I.WeightedBAProblem.__init__(self, s, Wobs, table)
        self.set_priors(cams, poses, W)

    def lin_obs_corrected(self, cams, pts, jac=True):
        return I.WeightedBAProblem.lin_obs_corrected(self, cams, pts, jac)

    def cost(self, x):
        return I.WeightedBAProblem.cost(self, x) + self.prior_cost(x)


# ------------------------------------------------------------------------------------------ the solve cases
K = 3
SOLVE_CASES = ("a_full_all_free", "b_two_on_one", "c_gauge_two", "d_gauge_gps", "e_full_huber_info")
# scene keywords and option overrides of every case (chosen so that the reference converges with every rho at least 1e-2 from
# min_relative_decrease: test_ba_prior_reference_cpu.py checks it)
CASE_SCENE = dict.fromkeys(SOLVE_CASES, dict())
CASE_OPT = dict.fromkeys(SOLVE_CASES, dict())


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene dict, cam_fixed or None, prior cams, prior poses, information or None, sqrt_information or None, obs W or None,
    loss table or None) of a solve case.  Prior poses: the true poses disturbed by the prior's own sigma (a GPS / INS reading)"""
    s = L.ba_scene(**CASE_SCENE[name])
    nc = len(s["cams0"])
    rng = np.random.default_rng(100 + SOLVE_CASES.index(name))
    true = s["cams_true"]

    def noisy(cams, rot=0.02, pos=0.05):
        out = true[cams].copy()
        d = rng.normal(size=(len(cams), 6)) * np.array([rot] * 3 + [pos] * 3)
        out[:, :4] = L.quat_mul(out[:, :4], L.quat_exp(d[:, :3]))
        out[:, 4:] += d[:, 3:]
        return out
    free = np.nonzero(~s["cam_fixed"].astype(bool).all(1))[0]
    cf, Om, W, Wobs, table = s["cam_fixed"], None, None, None, None
    if name in ("a_full_all_free", "e_full_huber_info"):
        cams = free
        Om = random_spd(rng, len(cams))
        if name == "e_full_huber_info":
            n = len(s["obs_cam"])
            Wobs = I.weights("mild", n, seed=3)
            table = B.table_of(B.KINDS.index("huber"), 2e-3, 1.0, 1.0, n)
    elif name == "b_two_on_one":
        cams = np.array([free[1], free[1]])
        Om = random_spd(rng, 2)
    elif name == "c_gauge_two":
        cf = None
        cams = np.array([0, nc - 1])
        Om = random_spd(rng, 2)
    else:
        cf = None
        cams = np.arange(nc)
        W = position_only_W(nc)
    return s, cf, np.asarray(cams, np.int32), noisy(cams), Om, W, Wobs, table


def case_W(name):
    s, cf, cams, poses, Om, W, Wobs, table = case(name)
    return sqrt_of_information(Om) if Om is not None else W


def problem(name):
    s, cf, cams, poses, Om, W, Wobs, table = case(name)
    if Wobs is not None or table is not None:
        return PriorWeightedBAProblem(s, Wobs, table, cams, poses, case_W(name))
    return PriorBAProblem(s, cams, poses, case_W(name), cam_fixed=cf)


def options(name):
    return L.lm_options(**CASE_OPT[name])


@functools.lru_cache(maxsize=None)
def reference(name, k=K):
    prob = problem(name)
    lm = B.lm_reference if isinstance(prob, PriorWeightedBAProblem) else L.lm_reference
    return lm(prob, options(name), k)
