"""Reference for the landmark position priors (control points) of the bundle adjustment (include/stba.h).  CPU only.

A prior k on landmark j: r = p_j - ph, J = I (0 for a constant landmark); whitened r' = W r, J' = W J; the cost gains 1/2 |r'|^2.

Two evaluations of one prior:
  lp_eval_mp   50 digits (mpmath), the double inputs taken as exact.
  lp_eval_np   float64, scalar: the factor as the library documents it -- r = p - ph, then row i of W r as
               (W_i0 r_0 + W_i1 r_1) + W_i2 r_2, no fused multiply-add.
The error of lp_eval_np against lp_eval_mp on an input is the yardstick of the device's on the same input (the GPU test).

The problems: LandmarkPriorBAProblem (lm_step_ref.BAProblem) and LandmarkPriorFullBAProblem (ba_prior_ref.PriorWeightedBAProblem:
whitened and corrected observations plus camera pose priors) append the whitened prior rows to r and J -- two residual blocks of two
rows per prior, the fourth row zero, on the landmark's three columns (and, to keep the blocks' shape, camera 0's six with zeros) --
so that lm_step_ref.lm_reference / ba_loss_ref.lm_reference / dogleg_ref.dogleg_reference, tolerances and compare apply unchanged.

drop_prior_rows states the two mistakes a half-built engine makes where a model term is summed from the observation records alone:
the reference's trace with the priors' rows left out of the inexact-step model (ITERATIVE_SCHUR) or of DOGLEG's |J u|^2 sums."""
import functools

import mpmath as mp
import numpy as np

import ba_information_ref as I
import ba_loss_ref as B
import ba_prior_ref as P
import dogleg_ref as D
import lm_step_ref as L

EPS = L.EPS
LD = np.longdouble
mp.mp.dps = max(mp.mp.dps, 50)


# ------------------------------------------------------------------------------------------ one prior
def lp_eval_np(pos, p, W, fixed=False):
    """(r'[3], J'[3, 3]) of one prior in float64; fixed: a constant landmark (J' exactly 0)"""
    W = np.asarray(W, float).reshape(3, 3)
    r = [float(p[k]) - float(pos[k]) for k in range(3)]
    rw = np.array([(W[i, 0] * r[0] + W[i, 1] * r[1]) + W[i, 2] * r[2] for i in range(3)])
    return rw, (np.zeros((3, 3)) if fixed else W.copy())


def lp_eval_mp(pos, p, W, fixed=False):
    """(r'[3], J'[3][3]) as mpf, the double inputs taken as exact"""
    Wm = [[mp.mpf(float(v)) for v in row] for row in np.asarray(W, float).reshape(3, 3)]
    r = [mp.mpf(float(p[k])) - mp.mpf(float(pos[k])) for k in range(3)]
    rw = [sum(Wm[i][k] * r[k] for k in range(3)) for i in range(3)]
    J = [[mp.mpf(0) if fixed else Wm[i][k] for k in range(3)] for i in range(3)]
    return rw, J


def floor_r(pos, p, W):
    """4 eps x (row's sum |W_ik| |r_k|), r at 50 digits"""
    r = np.array([abs(float(mp.mpf(float(p[k])) - mp.mpf(float(pos[k])))) for k in range(3)])
    return 4 * EPS * np.abs(np.asarray(W, float).reshape(3, 3)) @ r


def err_vs_mp(got_r, got_J, ref_r, ref_J):
    er = np.array([float(abs(mp.mpf(float(got_r[i])) - ref_r[i])) for i in range(3)])
    eJ = np.array([[float(abs(mp.mpf(float(got_J[i][a])) - ref_J[i][a])) for a in range(3)] for i in range(3)])
    return er, eJ


def chol3_mp(Om):
    """W = L^T of Omega = L L^T at 50 digits, from the lower triangle of the doubles given (None: not positive definite)"""
    A = mp.matrix([[mp.mpf(float(Om[max(a, b)][min(a, b)])) for b in range(3)] for a in range(3)])
    Lm = mp.zeros(3)
    for c in range(3):
        d = A[c, c] - sum(Lm[c, k] ** 2 for k in range(c))
        if not d > 0:
            return None
        Lm[c, c] = mp.sqrt(d)
        for a in range(c + 1, 3):
            Lm[a, c] = (A[a, c] - sum(Lm[a, k] * Lm[c, k] for k in range(c))) / Lm[c, c]
    return [[Lm[b, a] for b in range(3)] for a in range(3)]


def random_spd3(rng, n, sigma=0.05, spread=3.0):
    """random symmetric positive definite 3 x 3 information matrices: a random rotation of diag(1 / sigma_i^2)"""
    out = np.zeros((n, 3, 3))
    for k in range(n):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        A = Q @ np.diag(1.0 / (sigma * spread ** rng.uniform(-1, 1, 3)) ** 2) @ Q.T
        out[k] = 0.5 * (A + A.T)
    return out


def spd3_with_cond(rng, cond, top=1.0):
    """a full symmetric positive definite 3 x 3 with eigenvalues top, top / sqrt(cond), top / cond"""
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    A = Q @ np.diag([top, top / np.sqrt(cond), top / cond]) @ Q.T
    return 0.5 * (A + A.T)


def sqrt_of_information(Om):
    """W = L^T of Omega = L L^T, the 50-digit factor rounded (the engine's is within 1 eps of it per entry)"""
    out = []
    for o in np.asarray(Om, float).reshape(-1, 3, 3):
        W = chol3_mp(o)
        out.append([[float(v) for v in row] for row in W])
    return np.array(out)


# ------------------------------------------------------------------------------------------ the problems
class LandmarkPriorMixin:
    """adds priors (points[n], positions[n, 3], W[n, 3, 3]) to a BA problem: lin appends their whitened rows"""

    def set_landmark_priors(self, points, positions, W):
        self.lp_pt = np.asarray(points, np.int64).reshape(-1)
        self.lp_pos = np.asarray(positions, float).reshape(-1, 3).copy()
        n = len(self.lp_pt)
        self.lp_W = np.broadcast_to(np.eye(3), (n, 3, 3)).copy() if W is None else np.broadcast_to(np.asarray(W, float), (n, 3, 3)).copy()
        cols = np.concatenate([np.broadcast_to(np.arange(6), (n, 6)), 6 * self.nc + 3 * self.lp_pt[:, None] + np.arange(3)[None, :]], 1)
        self.lp_cols = np.repeat(cols, 2, axis=0)
        return self

    def lin_landmark_priors(self, pts, jac=True):
        """(r'[n, 3], J'[n, 3, 3]) at the landmarks `pts`, J' of a constant landmark zero"""
        n = len(self.lp_pt)
        r, J = np.zeros((n, 3)), np.zeros((n, 3, 3))
        for k, j in enumerate(self.lp_pt):
            r[k], J[k] = lp_eval_np(self.lp_pos[k], pts[j], self.lp_W[k], bool(self.pt_fixed[j]))
        return r, (J if jac else None)

    def lin(self, x, jac=True):
        r, J, cols = super().lin(x, jac)
        _, pts = self.split(x)
        rp, Jp = self.lin_landmark_priors(pts, jac)
        n = len(rp)
        r4 = np.zeros((n, 4)); r4[:, :3] = rp
        r = np.concatenate([r, r4.reshape(-1, 2)])
        if jac:
            J9 = np.zeros((n, 4, 9))
            J9[:, :3, 6:] = Jp
            J = np.concatenate([J, J9.reshape(-1, 2, 9)])
        return r, J, np.concatenate([cols, self.lp_cols])

    def landmark_prior_cost(self, x):
        _, pts = self.split(x)
        return float(0.5 * np.sum(self.lin_landmark_priors(pts, False)[0].astype(LD) ** 2))

    def landmark_blocks(self, x):
        """(sum W^T W [np, 3, 3], sum W^T r' [np, 3], and the sums of |terms| of both) of the priors per landmark, in longdouble;
        nothing for a constant landmark"""
        _, pts = self.split(x)
        rp, Jp = self.lin_landmark_priors(pts)
        H, g = np.zeros((self.np_, 3, 3), LD), np.zeros((self.np_, 3), LD)
        Ha, ga = np.zeros((self.np_, 3, 3), LD), np.zeros((self.np_, 3), LD)
        JL, rL = Jp.astype(LD), rp.astype(LD)
        for k, j in enumerate(self.lp_pt):
            H[j] += JL[k].T @ JL[k]; g[j] += JL[k].T @ rL[k]
            Ha[j] += np.abs(JL[k]).T @ np.abs(JL[k]); ga[j] += np.abs(JL[k]).T @ np.abs(rL[k])
        return H, g, Ha, ga


class LandmarkPriorBAProblem(LandmarkPriorMixin, L.BAProblem):
    def __init__(self, s, points, positions, W, cam_fixed="scene"):
        cf = s["cam_fixed"] if isinstance(cam_fixed, str) else cam_fixed
        L.BAProblem.__init__(self, s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], cf, s.get("pt_fixed"))
        self.set_landmark_priors(points, positions, W)


class LandmarkPriorFullBAProblem(LandmarkPriorMixin, P.PriorWeightedBAProblem):
    """whitened and corrected observations, camera pose priors and landmark priors"""

    def __init__(self, s, Wobs, table, cams, poses, Wc, points, positions, W):
        P.PriorWeightedBAProblem.__init__(self, s, Wobs, table, cams, poses, Wc)
        self.set_landmark_priors(points, positions, W)

    def cost(self, x):
        return P.PriorWeightedBAProblem.cost(self, x) + self.landmark_prior_cost(x)


def drop_prior_rows(prob, ref, what):
    """the reference's trace rows 0..k as a device that forgot the priors' rows would print them: what == "model": the whole term
    -(W d)^T (r' + W d / 2) is missing from the model change (ITERATIVE_SCHUR's sum over the records); what == "quadratic": only
    |W d|^2 / 2 is (DOGLEG's |J u|^2 sums; its gradient terms come from gp).  Only rho moves (cost_change / the wrong model)"""
    rows = L.trace_rows(ref)
    x = prob.x0
    for i, it in enumerate(ref):
        _, pts = prob.split(x)
        rp, Jp = prob.lin_landmark_priors(pts)
        d = it["delta"][6 * prob.nc:].reshape(-1, 3)[prob.lp_pt]
        f = np.einsum("kia,ka->ki", Jp.astype(LD), d.astype(LD))
        term = -np.sum(f * (rp.astype(LD) + f / 2)) if what == "model" else -np.sum(f * f / 2)
        rows[i][4] = it["cost_change"] / float(it["model_change"] - term)
        x = it["x"]
    st = ref[0]["start"]
    return np.vstack([[st["cost"], 0.0, st["gmax"], 0.0, 0.0, st["radius"], 1.0], rows])


# ------------------------------------------------------------------------------------------ the solve cases
K = 3
SOLVE_CASES = ("a_several_on_one", "b_on_fixed", "c_height_only", "d_full_cond1e8", "e_combined")
# (the ITERATIVE_SCHUR case: every reference rho of its K iterations is above 0.937, where the radius rule's factor sits at its cap of
# 3 -- the radius then does not depend on rho, and the direct and the iterative engine must agree on it to rounding)
ITERATIVE_CASE, DOGLEG_CASE = "b_on_fixed", "f_dogleg"
DOGLEG_SCENE = (dict(n_lm=33, seed=12, pts_jitter=3.0), dict(initial_trust_region_radius=1.0))


@functools.lru_cache(maxsize=None)
def case(name):
    """(scene, points[n], positions[n, 3], information[n, 3, 3] or None, sqrt_information or None, obs W or None, loss table or
    None, camera-prior (cams, poses, information) or None) of a solve case.  Positions: the true ones disturbed by the prior's own
    sigma (a surveyed point)"""
    names = SOLVE_CASES + (DOGLEG_CASE,)
    rng = np.random.default_rng(300 + names.index(name))
    s = L.ba_scene(**(DOGLEG_SCENE[0] if name == DOGLEG_CASE else {}))
    npt = len(s["pts0"])
    Om = W = Wobs = table = cam_priors = None

    def surveyed(points, sigma):
        return s["pts_true"][points] + rng.normal(0, 1.0, (len(points), 3)) * np.reshape(sigma, (-1, 1))
    if name == "a_several_on_one":
        # one prior on every second landmark, three on landmark 3 (not adjacent in the caller's order), one tight control point far
        # from the start: its W^T r' is the largest entry of the gradient
        points = np.concatenate([[3], np.arange(0, npt, 2), [3, 7], [3]]).astype(np.int32)
        Om = random_spd3(rng, len(points))
        pos = surveyed(points, 0.05)
        Om[-2] = np.eye(3) / 0.01 ** 2
        pos[-2] = s["pts0"][7] + np.array([0.05, -0.08, 0.06])
    elif name == "b_on_fixed":
        pf = np.zeros(npt, np.uint8); pf[[0, 5, 9]] = 1
        s = dict(s, pt_fixed=pf)
        points = np.array([0, 5, 5, 6, 11, 20], np.int32)
        Om = random_spd3(rng, len(points))
        pos = surveyed(points, 0.05)
    elif name == "c_height_only":
        points = np.arange(1, npt, 3).astype(np.int32)
        W = np.zeros((len(points), 3, 3)); W[:, 0, 2] = 1.0 / 0.02
        pos = surveyed(points, 0.02)
    elif name == "d_full_cond1e8":
        points = np.array([2, 9, 9, 17, 30], np.int32)
        Om = np.stack([spd3_with_cond(rng, 1e8, top=1.0 / 0.02 ** 2) for _ in points])
        pos = surveyed(points, 0.02)
    elif name == "e_combined":
        n = len(s["obs_cam"])
        Wobs = I.weights("mild", n, seed=3)
        table = B.table_of(B.KINDS.index("huber"), 2e-3, 1.0, 1.0, n)
        free = np.nonzero(~s["cam_fixed"].astype(bool).all(1))[0]
        cpose = s["cams_true"][free].copy(); cpose[:, 4:] += rng.normal(0, 0.05, (len(free), 3))
        cam_priors = (free.astype(np.int32), cpose, P.random_spd(rng, len(free)))
        points = np.concatenate([np.arange(0, npt, 4), [4]]).astype(np.int32)
        Om = random_spd3(rng, len(points))
        pos = surveyed(points, 0.05)
    else:
        # f_dogleg: sigma 1 on every eighth landmark -- weak enough that the trace keeps the plain scene's variety (Cauchy steps, an
        # interpolated one, Gauss-Newton steps, rejections of both of the latter), strong enough that their rows count in |J u|^2
        rng = np.random.default_rng(1)
        points = np.arange(0, npt, 8).astype(np.int32)
        Om = random_spd3(rng, len(points), sigma=1.0)
        pos = s["pts_true"][points] + rng.normal(0, 1.0, (len(points), 3))
    return s, points, pos, Om, W, Wobs, table, cam_priors


def case_W(name):
    s, points, pos, Om, W, Wobs, table, cam_priors = case(name)
    return sqrt_of_information(Om) if Om is not None else W


def problem(name):
    s, points, pos, Om, W, Wobs, table, cam_priors = case(name)
    if cam_priors is not None:
        return LandmarkPriorFullBAProblem(s, Wobs, table, cam_priors[0], cam_priors[1], P.sqrt_of_information(cam_priors[2]), points, pos,
                                          case_W(name))
    return LandmarkPriorBAProblem(s, points, pos, case_W(name))


def options(name):
    return L.lm_options(**(DOGLEG_SCENE[1] if name == DOGLEG_CASE else {}))


@functools.lru_cache(maxsize=None)
def reference(name, k=K):
    prob = problem(name)
    lm = B.lm_reference if isinstance(prob, LandmarkPriorFullBAProblem) else L.lm_reference
    return lm(prob, options(name), k)


@functools.lru_cache(maxsize=None)
def dogleg_reference(k):
    return D.dogleg_reference(problem(DOGLEG_CASE), options(DOGLEG_CASE), k)


# ------------------------------------------------------------------------------------------ the gauge scene
@functools.lru_cache(maxsize=None)
def gauge_case():
    """NO constant camera dof; priors on four landmarks that are not coplanar (the four whose tetrahedron is the largest of a few
    hundred random picks): (scene, points, positions, W)"""
    s = L.ba_scene()
    rng = np.random.default_rng(77)
    T = s["pts_true"]
    best = None
    for _ in range(300):
        q = rng.choice(len(T), 4, replace=False)
        v = abs(np.linalg.det(T[q[1:]] - T[q[0]]))
        if best is None or v > best[0]:
            best = (v, np.sort(q))
    points = best[1].astype(np.int32)
    pos = T[points] + rng.normal(0, 0.01, (4, 3))
    W = np.broadcast_to(np.eye(3) / 0.05, (4, 3, 3)).copy()
    return s, points, pos, W


def gauge_problem(with_priors=True):
    s, points, pos, W = gauge_case()
    if not with_priors:
        points, pos, W = points[:0], pos[:0], W[:0]
    return LandmarkPriorBAProblem(s, points, pos, W, cam_fixed=None)


# ------------------------------------------------------------------------------------------ the pinned scene
@functools.lru_cache(maxsize=None)
def pinned_case():
    """NO constant camera dof, a tight prior (sigma 1 cm, the position 1 mm off) on EVERY landmark, pixel noise 1e-4: a problem whose
    minimiser is sharp -- the smallest eigenvalue of J^T J is 1.8e-3 and the converged cost 2e-6, so two points whose costs agree to
    1e-15 relative are at most sqrt(2 * 1e-15 * cost / lambda_min) = 1.6e-9 apart (test_pinned_scene_has_a_sharp_minimiser), and
    every strategy that reaches the minimiser ends within 1e-8 of every other: (scene, points, positions, W)"""
    s = L.ba_scene(pix_noise=1e-4)
    rng = np.random.default_rng(5)
    npt = len(s["pts0"])
    points = np.arange(npt, dtype=np.int32)
    pos = s["pts_true"] + rng.normal(0, 1e-3, (npt, 3))
    W = np.broadcast_to(np.eye(3) / 0.01, (npt, 3, 3)).copy()
    return s, points, pos, W


def pinned_problem():
    s, points, pos, W = pinned_case()
    return LandmarkPriorBAProblem(s, points, pos, W, cam_fixed=None)
