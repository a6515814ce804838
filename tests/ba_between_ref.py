"""Reference for the camera-to-camera relative-pose factors of the bundle adjustment (include/stba.h).  CPU only.

An edge k between the cameras i and j with the measurement (qz, tz) and the square-root information W, poses camera to world, chart
q <- q (x) exp(dtheta), t <- t + dt, order [rot(3), pos(3)]:
    r   = [ Log(qz^-1 (x) (q_i^-1 (x) q_j)) ; R_i^T (t_j - t_i) - tz ]
    J_j = [ Jr^-1(r_theta)  0 ; 0  R_i^T ]        J_i = [ -Jr^-1(r_theta) R_j^T R_i  0 ; hat(R_i^T (t_j - t_i))  -R_i^T ]
    r' = W r,  J_i' = W J_i,  J_j' = W J_j;  the cost gains 1/2 |r'|^2;  columns of constant dofs exactly 0.

Two evaluations of one edge:
  between_eval_mp   50 digits, on tests/mp_ref.py: the quaternions are taken as exact up to scale, Log is read from the rotation matrix
                    R(qz)^T R(q_i)^T R(q_j) (mp_ref.so3_log), and Jr^-1 is the INVERSE (an LU solve at 50 digits) of the right Jacobian
                    Jr(phi) = V(-phi), mp_ref.left_jacobian: no closed form of an inverse enters.
  between_eval_np   float64, scalar: a restatement of the operation order slam-tricks_amd/csrc/ba_between.hpp documents -- m = conj(q_i)
                    (x) q_j in the paired order, Log and Jr^-1 as the priors' (ba_prior_ref.prior_eval_np), R(q) = I + (2 / |q|^2)(...),
                    R_j^T R_i = R(m)^T, three-term products (a0 b0 + a1 b1) + a2 b2, whitening dots of six terms from the left.

The bound of anything that evaluates an edge in doubles (the header on the host, the kernels), per entry of r', J_i', J_j':
    err <= max(4 x the restatement's own error on that input,  C_FLOOR eps sum_k |W_jk| |entry_k|)
the entries those of the 50-digit evaluation at W = I.  C_FLOOR is the restatement's own worst err / (eps sum_k |W_jk| |entry_k|) over
the edge grid below, rounded up to a power of two: MEASURED 152.8 (tests/test_ba_between_reference_cpu.py prints and pins it; at a
position-only edge whose position residual is 0.05 to 0.15 a component while t_j - t_i is 10 units long: R_i^T (t_j - t_i) carries
roundings of 10 eps, the sum's terms are 200 times smaller) -> C_FLOOR = 256.  It comes from the reference side only and is never fitted to the header or the device.

The problems: every residual block gets k = 12 columns -- an edge is three blocks of two rows on the twelve columns of its two
cameras, and what the base problem makes (observations: 9 columns, with priors 9 too) is padded with zero columns -- so that
lm_step_ref.normal_equations / lm_reference / tolerances / compare apply unchanged."""
import functools
import math

import mpmath as mp
import numpy as np

import ba_information_ref as I
import ba_loss_ref as B
import ba_prior_ref as P
import lm_step_ref as L
import mp_ref as M

EPS = L.EPS
LD = np.longdouble
ANGLES = P.ANGLES
C_FLOOR = 256.0
NEGATE = ("none", "meas", "i", "j")
# the kinds of constant-dof masks of a camera: [rot(3), pos(3)]
MASKS = {"none": (0, 0, 0, 0, 0, 0), "all": (1, 1, 1, 1, 1, 1), "mixed": (0, 1, 0, 0, 1, 0), "rot": (1, 1, 1, 0, 0, 0), "pos": (0, 0, 0, 1, 1, 1)}
MASK_PAIRS = [(a, b) for a in MASKS for b in MASKS]


# ------------------------------------------------------------------------------------------ one edge, float64
def _qmul_conj_a(a, b):
    """conj(a) (x) b in the paired order of ba_prior.hpp / ba_between.hpp, python floats"""
    ax, ay, az, aw = -a[0], -a[1], -a[2], a[3]
    bx, by, bz, bw = b
    return [(aw * bx + ax * bw) + (ay * bz - az * by), (aw * by + ay * bw) + (az * bx - ax * bz),
            (aw * bz + az * bw) + (ax * by - ay * bx), ((aw * bw - ax * bx) - ay * by) - az * bz]


def _rot(q):
    x, y, z, w = q
    s = 2.0 / (((x * x + y * y) + z * z) + w * w)
    return [[1.0 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
            [s * (x * y + z * w), 1.0 - s * (x * x + z * z), s * (y * z - x * w)],
            [s * (x * z - y * w), s * (y * z + x * w), 1.0 - s * (x * x + y * y)]]


def _dot6(w, x):
    return ((((w[0] * x[0] + w[1] * x[1]) + w[2] * x[2]) + w[3] * x[3]) + w[4] * x[4]) + w[5] * x[5]


def between_eval_np(meas, ci, cj, W, fixed_i=None, fixed_j=None):
    """(r'[6], J_i'[6, 6], J_j'[6, 6]) of one edge in float64; fixed_i / fixed_j[6]: the cameras' constant dofs"""
    meas, ci, cj = ([float(v) for v in a] for a in (meas, ci, cj))
    m = _qmul_conj_a(ci[:4], cj[:4])
    x, y, z, w = _qmul_conj_a(meas[:4], m)
    lead = x if x != 0.0 else (y if y != 0.0 else z)
    if w < 0.0 or (w == 0.0 and lead < 0.0):
        x, y, z, w = -x, -y, -z, -w
    n2 = (x * x + y * y) + z * z
    n = math.sqrt(n2)
    if n2 < 1e-40:
        k, cot = 2.0 / w, 0.0
    else:
        k, cot = 2.0 * math.atan2(n, w) / n, w / n
    p = [k * x, k * y, k * z]
    th = k * n
    t2 = th * th
    if th < P.SERIES_THETA:
        c = 1.0 / 12.0 + t2 * (1.0 / 720.0 + t2 * (1.0 / 30240.0 + t2 * (1.0 / 1209600.0 + t2 * (1.0 / 47900160.0))))
    else:
        c = (1.0 - (0.5 * th) * cot) / t2
    pp = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    h = [[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]]
    Jri = [[((1.0 if a == b else 0.0) + 0.5 * h[a][b]) + c * (p[a] * p[b] - pp * (1.0 if a == b else 0.0)) for b in range(3)] for a in range(3)]
    Ri, Rm = _rot(ci[:4]), _rot(m)
    d = [cj[4] - ci[4], cj[5] - ci[5], cj[6] - ci[6]]
    v = [(Ri[0][a] * d[0] + Ri[1][a] * d[1]) + Ri[2][a] * d[2] for a in range(3)]
    r = p + [v[a] - meas[4 + a] for a in range(3)]
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    for a in range(3):
        for b in range(3):
            Ji[a, b] = -((Jri[a][0] * Rm[b][0] + Jri[a][1] * Rm[b][1]) + Jri[a][2] * Rm[b][2])
            Jj[a, b] = Jri[a][b]
            Ji[3 + a, 3 + b] = -Ri[b][a]
            Jj[3 + a, 3 + b] = Ri[b][a]
    Ji[3, 1], Ji[3, 2], Ji[4, 0], Ji[4, 2], Ji[5, 0], Ji[5, 1] = -v[2], v[1], v[2], -v[0], -v[1], v[0]
    W = np.asarray(W, float).reshape(6, 6)
    Wl, Jil, Jjl = W.tolist(), Ji.T.tolist(), Jj.T.tolist()
    rw = np.array([_dot6(Wl[i], r) for i in range(6)])
    Jiw = np.array([[_dot6(Wl[i], Jil[a]) for a in range(6)] for i in range(6)])
    Jjw = np.array([[_dot6(Wl[i], Jjl[a]) for a in range(6)] for i in range(6)])
    if fixed_i is not None:
        Jiw[:, np.asarray(fixed_i, bool)] = 0.0
    if fixed_j is not None:
        Jjw[:, np.asarray(fixed_j, bool)] = 0.0
    return rw, Jiw, Jjw


# ------------------------------------------------------------------------------------------ one edge, 50 digits
def between_residual_mp(Rz, tz, Ri, ti, Rj, tj):
    phi = M.so3_log(M.mm(M.tr(Rz), M.mm(M.tr(Ri), Rj)))
    v = M.mv(M.tr(Ri), [tj[k] - ti[k] for k in range(3)])
    return list(phi) + [v[k] - tz[k] for k in range(3)], v


def between_eval_mp(meas, ci, cj, W, fixed_i=None, fixed_j=None):
    """(r'[6], J_i', J_j') as a list of mpf and two mp.matrix, the double inputs taken as exact (the quaternions up to scale)"""
    Rz, Ri, Rj = M.quat_to_rot(meas[:4]), M.quat_to_rot(ci[:4]), M.quat_to_rot(cj[:4])
    tz, ti, tj = ([mp.mpf(float(v)) for v in a[4:]] for a in (meas, ci, cj))
    r, v = between_residual_mp(Rz, tz, Ri, ti, Rj, tj)
    Jri = mp.inverse(mp.matrix(M.left_jacobian([-x for x in r[:3]])))
    A = Jri * mp.matrix(M.mm(M.tr(Rj), Ri))
    hv, RiT = M.hat(v), M.tr(Ri)
    Ji, Jj = mp.zeros(6, 6), mp.zeros(6, 6)
    for a in range(3):
        for b in range(3):
            Ji[a, b] = -A[a, b]
            Jj[a, b] = Jri[a, b]
            Ji[3 + a, b] = hv[a][b]
            Ji[3 + a, 3 + b] = -RiT[a][b]
            Jj[3 + a, 3 + b] = RiT[a][b]
    Wm = mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.asarray(W, float).reshape(6, 6)])
    rw, Jiw, Jjw = Wm * mp.matrix(r), Wm * Ji, Wm * Jj
    for J, fx in ((Jiw, fixed_i), (Jjw, fixed_j)):
        if fx is not None:
            for a in range(6):
                if fx[a]:
                    for i in range(6):
                        J[i, a] = M.ZERO
    return [rw[i] for i in range(6)], Jiw, Jjw


def between_jacobians_numeric_mp(meas, ci, cj):
    """d r / d[dtheta_i, dt_i] and d r / d[dtheta_j, dt_j] (not whitened) by central differences at 50 digits, under the engine's chart
    R <- R Exp(dtheta), t <- t + dt"""
    Rz, Ri, Rj = M.quat_to_rot(meas[:4]), M.quat_to_rot(ci[:4]), M.quat_to_rot(cj[:4])
    tz, ti, tj = ([mp.mpf(float(v)) for v in a[4:]] for a in (meas, ci, cj))

    def at(di, dj):
        return between_residual_mp(Rz, tz, M.mm(Ri, M.so3_exp(di[:3])), [ti[k] + di[3 + k] for k in range(3)],
                                   M.mm(Rj, M.so3_exp(dj[:3])), [tj[k] + dj[3 + k] for k in range(3)])[0]
    z6 = [M.ZERO] * 6
    return M.num_jac(lambda d: at(d, z6), z6, 6), M.num_jac(lambda d: at(z6, d), z6, 6)


def scales(W, meas, ci, cj, fixed_i=None, fixed_j=None):
    """eps sum_k |W_jk| |entry_k| for r'[6], J_i'[6, 6], J_j'[6, 6], the entries those of the 50-digit evaluation at W = I"""
    r, Ji, Jj = between_eval_mp(meas, ci, cj, np.eye(6), fixed_i, fixed_j)
    aW = np.abs(np.asarray(W, float).reshape(6, 6))
    return EPS * aW @ np.abs(M.f64(r)), EPS * aW @ np.abs(M.f64(Ji)), EPS * aW @ np.abs(M.f64(Jj))


def err_vs_mp(got, ref):
    """|double - 50-digit| per entry of (r', J_i', J_j'), formed at 50 digits"""
    er = np.array([float(abs(mp.mpf(float(got[0][i])) - ref[0][i])) for i in range(6)])
    eJ = [np.array([[float(abs(mp.mpf(float(g[i, a])) - m[i, a])) for a in range(6)] for i in range(6)]) for g, m in zip(got[1:], ref[1:])]
    return er, eJ[0], eJ[1]


# ------------------------------------------------------------------------------------------ the edge grid
def grid_edge(angle, negate, baseline, seed):
    """(meas[7], ci[7], cj[7]) in doubles: two random camera poses `baseline` apart and a measurement whose error rotation has the angle
    `angle` (up to the rounding of qz) and whose position residual has components of 0.05 to 0.15; angle 0: qz holds the bits of conj(q_i) (x) q_j as
    the factor forms it, the rotation residual is exactly 0.  negate: which of the three quaternions is stored as -q"""
    rng = np.random.default_rng(seed)
    ci = np.concatenate([M.quat_double(M.axis_angle(rng, rng.uniform(0.2, 2.5))), rng.normal(size=3)])
    dirn = rng.normal(size=3)
    cj = np.concatenate([M.quat_double(M.axis_angle(rng, rng.uniform(0.2, 2.5))), ci[4:] + baseline * dirn / np.linalg.norm(dirn)])
    th = P.angle_value(angle)
    if th == 0:
        qz = np.array(_qmul_conj_a(ci[:4].tolist(), cj[:4].tolist()))
    else:
        a = M.rot_to_quat(M.mm(M.tr(M.quat_to_rot(ci[:4])), M.quat_to_rot(cj[:4])))
        e = M.quat_from_axis_angle([-v for v in M.axis_angle(rng, th)])
        qz = M.f64([a[3] * e[0] + a[0] * e[3] + a[1] * e[2] - a[2] * e[1], a[3] * e[1] - a[0] * e[2] + a[1] * e[3] + a[2] * e[0],
                    a[3] * e[2] + a[0] * e[1] - a[1] * e[0] + a[2] * e[3], a[3] * e[3] - a[0] * e[0] - a[1] * e[1] - a[2] * e[2]])
    v = L.quat_to_rot(ci[None, :4])[0].T @ (cj[4:] - ci[4:])
    # (every component of the position residual between 0.05 and 0.15 in size: none small by chance against what t_j - t_i carries)
    meas = np.concatenate([qz, v - rng.choice([-1.0, 1.0], 3) * rng.uniform(0.05, 0.15, 3)])
    if negate == "meas":
        meas[:4] = -meas[:4]
    elif negate == "i":
        ci[:4] = -ci[:4]
    elif negate == "j":
        cj[:4] = -cj[:4]
    return meas, ci, cj


@functools.lru_cache(maxsize=None)
def grid():
    """the edge grid of the CPU and the GPU test: every angle x which quaternion is negated x {full random W, position-only W} x
    {t_j - t_i small (0.05), ~10 units}, the pairs of mask kinds dealt round (each of the 25 several times).  Edge k runs between the
    cameras 2 k and 2 k + 1 of its own.  dict: cams[2 n, 7], cam_fixed[2 n, 6], cam_i, cam_j[n], meas[n, 7], W[n, 6, 6], names[n]"""
    cams, fixed, meas, W, names = [], [], [], [], []
    rng = np.random.default_rng(77)
    k = 0
    for ia, angle in enumerate(ANGLES):
        for neg in NEGATE:
            for wkind in ("full", "pos"):
                for baseline in (0.05, 10.0):
                    z, ci, cj = grid_edge(angle, neg, baseline, 1000 + k)
                    mi, mj = MASK_PAIRS[k % len(MASK_PAIRS)]
                    cams += [ci, cj]; fixed += [MASKS[mi], MASKS[mj]]; meas.append(z)
                    W.append(P.random_W(rng)[0] if wkind == "full" else P.position_only_W()[0])
                    names.append(f"{angle}/{neg}/{wkind}/{baseline}/{mi}-{mj}")
                    k += 1
    n = len(meas)
    out = dict(cams=np.array(cams), cam_fixed=np.array(fixed, np.uint8), cam_i=np.arange(0, 2 * n, 2, dtype=np.int32),
               cam_j=np.arange(1, 2 * n, 2, dtype=np.int32), meas=np.array(meas), W=np.array(W), names=names)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grid_reference(k):
    """edge k of the grid (as the host holds it: the measurement's quaternion normalised): (50-digit (r', J_i', J_j'), the restatement's
    error against it, eps sum |W||entry|), each a triple for r', J_i', J_j'"""
    g = grid()
    z = g["meas"][k].copy()
    z[:4] = P.normalise_like_the_host(z[None, :4])[0]
    i, j = g["cam_i"][k], g["cam_j"][k]
    args = (z, g["cams"][i], g["cams"][j], g["W"][k], g["cam_fixed"][i], g["cam_fixed"][j])
    ref = between_eval_mp(*args)
    return ref, err_vs_mp(between_eval_np(*args), ref), scales(g["W"][k], *args[:3], *args[4:])


def worst_ratio(k, got):
    """max over the entries of err / bound for `got` = (r'[6], J_i'[6, 6], J_j'[6, 6]) of grid edge k, under this module's bound; an
    entry whose bound is 0 (a structural zero, a constant dof's column) must be exactly 0: inf otherwise"""
    ref, own, sc = grid_reference(k)
    worst = 0.0
    for e, o, s in zip(err_vs_mp(got, ref), own, sc):
        bound = np.maximum(4 * o, C_FLOOR * s)
        if np.any(e[bound == 0] != 0):
            return float("inf")
        if np.any(bound > 0):
            worst = max(worst, float(np.max(e[bound > 0] / bound[bound > 0])))
    return worst


# ------------------------------------------------------------------------------------------ the problems
class BetweenMixin:
    """adds edges (cam_i[n], cam_j[n], meas[n, 7], W[n, 6, 6]) to a BA problem: lin pads the base problem's blocks to twelve columns and
    appends the edges' whitened rows, cost gains their 1/2 |r'|^2"""

    def set_edges(self, cam_i, cam_j, meas, W):
        self.bt_i, self.bt_j = np.asarray(cam_i, np.int64).reshape(-1), np.asarray(cam_j, np.int64).reshape(-1)
        self.bt_meas = np.asarray(meas, float).reshape(-1, 7).copy()
        self.bt_meas[:, :4] = P.normalise_like_the_host(self.bt_meas[:, :4])
        n = len(self.bt_i)
        self.bt_W = np.broadcast_to(np.eye(6), (n, 6, 6)).copy() if W is None else np.broadcast_to(np.asarray(W, float), (n, 6, 6)).copy()
        self.bt_cols = np.repeat(np.concatenate([6 * self.bt_i[:, None] + np.arange(6), 6 * self.bt_j[:, None] + np.arange(6)], 1), 3, axis=0)
        return self

    def lin_edges(self, cams, jac=True):
        """(r'[n, 6], J_i'[n, 6, 6], J_j'[n, 6, 6]) at the cameras `cams`, columns of constant dofs zero"""
        n = len(self.bt_i)
        r, Ji, Jj = np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
        for k in range(n):
            i, j = self.bt_i[k], self.bt_j[k]
            r[k], Ji[k], Jj[k] = between_eval_np(self.bt_meas[k], cams[i], cams[j], self.bt_W[k], self.cam_fixed[i], self.cam_fixed[j])
        return r, Ji, Jj

    def lin(self, x, jac=True):
        r, J, cols = super().lin(x, jac)
        pad = 12 - cols.shape[1]
        cols = np.concatenate([cols, np.repeat(cols[:, -1:], pad, axis=1)], 1)
        cams, _ = self.split(x)
        re, Ji, Jj = self.lin_edges(cams, jac)
        r = np.concatenate([r, re.reshape(-1, 2)])
        if jac:
            J = np.concatenate([J, np.zeros(J.shape[:2] + (pad,))], 2)
            J = np.concatenate([J, np.concatenate([Ji, Jj], 2).reshape(-1, 2, 12)])
        return r, (J if jac else None), np.concatenate([cols, self.bt_cols])

    def edge_cost(self, x):
        cams, _ = self.split(x)
        return float(0.5 * np.sum(self.lin_edges(cams, False)[0].astype(LD) ** 2))

    def edge_blocks(self, x):
        """the edges' sums in longdouble: (H[nc, 6, 6] = sum J_x'^T J_x', g[nc, 6] = sum J_x'^T r', their sums of |terms| Ha, ga, and
        S: dict (hi, lo) -> (sum J_hi'^T J_lo' [6, 6], its sum of |terms|))"""
        cams, _ = self.split(x)
        r, Ji, Jj = (a.astype(LD) for a in self.lin_edges(cams))
        H, g = np.zeros((self.nc, 6, 6), LD), np.zeros((self.nc, 6), LD)
        Ha, ga = np.zeros((self.nc, 6, 6), LD), np.zeros((self.nc, 6), LD)
        S = {}
        for k in range(len(self.bt_i)):
            for c, J in ((self.bt_i[k], Ji[k]), (self.bt_j[k], Jj[k])):
                H[c] += J.T @ J; g[c] += J.T @ r[k]
                Ha[c] += np.abs(J).T @ np.abs(J); ga[c] += np.abs(J).T @ np.abs(r[k])
            hi_is_j = self.bt_j[k] > self.bt_i[k]
            Jh, Jl = (Jj[k], Ji[k]) if hi_is_j else (Ji[k], Jj[k])
            key = (int(max(self.bt_i[k], self.bt_j[k])), int(min(self.bt_i[k], self.bt_j[k])))
            s, sa = S.get(key, (np.zeros((6, 6), LD), np.zeros((6, 6), LD)))
            S[key] = (s + Jh.T @ Jl, sa + np.abs(Jh).T @ np.abs(Jl))
        return H, g, Ha, ga, S


class BetweenBAProblem(BetweenMixin, L.BAProblem):
    def __init__(self, s, cam_i, cam_j, meas, W, cam_fixed="scene"):
        cf = s["cam_fixed"] if isinstance(cam_fixed, str) else cam_fixed
        L.BAProblem.__init__(self, s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], cf, s.get("pt_fixed"))
        self.set_edges(cam_i, cam_j, meas, W)


class BetweenPriorBAProblem(BetweenMixin, P.PriorMixin, L.BAProblem):
    """edges and pose priors"""

    def __init__(self, s, cam_i, cam_j, meas, W, pr_cams, pr_poses, pr_W, cam_fixed="scene"):
        cf = s["cam_fixed"] if isinstance(cam_fixed, str) else cam_fixed
        L.BAProblem.__init__(self, s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], cf, s.get("pt_fixed"))
        self.set_priors(pr_cams, pr_poses, pr_W)
        self.set_edges(cam_i, cam_j, meas, W)


class BetweenWeightedBAProblem(BetweenMixin, I.WeightedBAProblem):
    """whitened and corrected observations (ba_information_ref) plus edges: cost = 1/2 sum rho + 1/2 sum |r'|^2"""

    def __init__(self, s, Wobs, table, cam_i, cam_j, meas, W):
        I.WeightedBAProblem.__init__(self, s, Wobs, table)
        self.set_edges(cam_i, cam_j, meas, W)

    def cost(self, x):
        return I.WeightedBAProblem.cost(self, x) + self.edge_cost(x)


# ------------------------------------------------------------------------------------------ scenes and measurements
def relative_pose(cams, i, j):
    """[q_i^-1 (x) q_j, R_i^T (t_j - t_i)] of the poses cams[n, 7] for the index arrays i, j"""
    qi = cams[i, :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    R = L.quat_to_rot(cams[i, :4])
    return np.concatenate([L.quat_mul(qi, cams[j, :4]), np.einsum("nji,nj->ni", R, cams[j, 4:] - cams[i, 4:])], 1)


def odometry(s, i, j, rng, rot=0.01, pos=0.02):
    """measurements of the edges (i, j): the true relative poses disturbed by the sensor's sigma"""
    i, j = np.asarray(i), np.asarray(j)
    z = relative_pose(s["cams_true"], i, j)
    d = rng.normal(size=(len(i), 6)) * np.array([rot] * 3 + [pos] * 3)
    z[:, :4] = L.quat_mul(z[:, :4], L.quat_exp(d[:, :3]))
    z[:, 4:] += d[:, 3:]
    return z


def shared_landmarks(s):
    """[nc, nc] number of landmarks two cameras both observe"""
    nc, npt = len(s["cams0"]), len(s["pts0"])
    V = np.zeros((nc, npt), np.int64)
    V[s["obs_cam"], s["obs_pt"]] = 1
    return V @ V.T


@functools.lru_cache(maxsize=None)
def disjoint_scene(n_cams=8):
    """(scene, (a, b)): lm_step_ref.ba_scene with the observations that camera b has of landmarks camera a sees too taken out, for the
    pair that shares the fewest -- a and b then share no landmark, so the pair plan has no block (b, a) or (a, b) -- every landmark
    keeping two observations at least and both cameras four"""
    s = dict(L.ba_scene(n_cams=n_cams))
    sh = shared_landmarks(s).astype(float)
    np.fill_diagonal(sh, np.inf)
    fx = s["cam_fixed"].astype(bool).any(1)          # (not the cameras that hold the gauge: their columns are zero)
    sh[fx] = np.inf; sh[:, fx] = np.inf
    a, b = np.unravel_index(np.argmin(sh), sh.shape)
    a, b = int(min(a, b)), int(max(a, b))
    seen_a = set(s["obs_pt"][s["obs_cam"] == a].tolist())
    drop = (s["obs_cam"] == b) & np.isin(s["obs_pt"], list(seen_a))
    keep = ~drop
    s["obs_cam"], s["obs_pt"], s["obs_feat"] = s["obs_cam"][keep], s["obs_pt"][keep], s["obs_feat"][keep]
    counts = np.bincount(s["obs_pt"], minlength=len(s["pts0"]))
    assert counts.min() >= 2 and (s["obs_cam"] == a).sum() >= 4 and (s["obs_cam"] == b).sum() >= 4, (counts.min(), a, b)
    assert shared_landmarks(s)[a, b] == 0
    return s, (a, b)


# ------------------------------------------------------------------------------------------ the solve cases
K = 3
SOLVE_CASES = ("a_chain", "b_chain_loop_disjoint", "c_chain_two_priors", "d_chain_huber_info", "e_weak_position_only")


@functools.lru_cache(maxsize=None)
def case(name):
    """dict of a solve case: s (scene), cam_fixed (or None: nothing constant), cam_i, cam_j, meas, information | sqrt_information (one is
    None), priors (None | dict cams, poses, information), Wobs, table"""
    rng = np.random.default_rng(300 + SOLVE_CASES.index(name))
    s = disjoint_scene()[0] if name == "b_chain_loop_disjoint" else L.ba_scene()
    nc = len(s["cams0"])
    ci, cj = np.arange(nc - 1), np.arange(1, nc)
    out = dict(s=s, cam_fixed=s["cam_fixed"], priors=None, Wobs=None, table=None, information=None, sqrt_information=None)
    if name == "b_chain_loop_disjoint":
        a, b = disjoint_scene()[1]
        ci, cj = np.append(ci, b), np.append(cj, a)          # (the closure runs from the later camera to the earlier: i > j)
    if name == "e_weak_position_only":
        out["sqrt_information"] = P.position_only_W(len(ci), sigma=1.0)
        out["meas"] = odometry(s, ci, cj, rng, pos=0.3)
    else:
        out["information"] = P.random_spd(rng, len(ci), rot_sigma=0.01, pos_sigma=0.02)
        out["meas"] = odometry(s, ci, cj, rng)
    if name == "c_chain_two_priors":
        out["cam_fixed"] = None
        pc = np.array([0, nc - 1], np.int32)
        poses = s["cams_true"][pc].copy()
        d = rng.normal(size=(2, 6)) * np.array([0.02] * 3 + [0.05] * 3)
        poses[:, :4] = L.quat_mul(poses[:, :4], L.quat_exp(d[:, :3]))
        poses[:, 4:] += d[:, 3:]
        out["priors"] = dict(cams=pc, poses=poses, information=P.random_spd(rng, 2))
    if name == "d_chain_huber_info":
        n = len(s["obs_cam"])
        out["Wobs"] = I.weights("mild", n, seed=3)
        out["table"] = B.table_of(B.KINDS.index("huber"), 2e-3, 1.0, 1.0, n)
    out["cam_i"], out["cam_j"] = ci.astype(np.int32), cj.astype(np.int32)
    return out


def case_W(name):
    c = case(name)
    return P.sqrt_of_information(c["information"]) if c["information"] is not None else c["sqrt_information"]


def problem(name):
    c = case(name)
    e = (c["cam_i"], c["cam_j"], c["meas"], case_W(name))
    if c["Wobs"] is not None:
        return BetweenWeightedBAProblem(c["s"], c["Wobs"], c["table"], *e)
    if c["priors"] is not None:
        p = c["priors"]
        return BetweenPriorBAProblem(c["s"], *e, p["cams"], p["poses"], P.sqrt_of_information(p["information"]), cam_fixed=c["cam_fixed"])
    return BetweenBAProblem(c["s"], *e, cam_fixed=c["cam_fixed"])


def options(name):
    return L.lm_options()


@functools.lru_cache(maxsize=None)
def reference(name, k=K):
    prob = problem(name)
    lm = B.lm_reference if isinstance(prob, BetweenWeightedBAProblem) else L.lm_reference
    return lm(prob, options(name), k)
