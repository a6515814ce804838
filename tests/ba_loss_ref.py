"""Reference for bundle adjustment's robust loss functions (BAEngine(loss=), stba_ba_set_loss): Ceres' losses and Ceres' corrector per
observation on top of lm_step_ref.BAProblem.  CPU only (numpy; mpmath where a test asks for 50 digits).

Nothing is restated that another reference module has: the losses, the corrector (pg_loss_ref.rho / factors / correct, written for
residual blocks of any size) and the LM loop with the cost 1/2 sum rho (pg_loss_ref.lm_reference) are pg_loss_ref's, the problem,
the scenes, the bounds and the comparison lm_step_ref's.  Two things are new here: the evaluate bound for 2 x 2 correction matrices
(pg_loss_ref.corrected_bound builds 6 x 6 ones), and a dogleg loop -- dogleg_ref.dogleg_reference takes its START cost from
1/2 |r|^2, which with a loss is not the cost (the reason pg_loss_ref has an LM loop of its own); it uses dogleg_ref's step and is
compared by dogleg_ref.compare.

Per observation, with s = |r|^2: the cost term is rho(s), and with sq = sqrt(rho')
    s == 0 or rho'' <= 0:   r' = sq r,                J' = sq J
    otherwise:              D = 1 + 2 s rho'' / rho', alpha = 1 - sqrt(D),
                            r' = sq / (1 - alpha) r,   J' = sq (J - (alpha / s) r (r^T J))           (J = [Jc | Jp], 2 x 9)

Scenes (lm_step_ref.ba_scene):
  A  n_lm = 33, extras: 139 observations, 10 cameras; constant dofs, constant landmarks, a camera that observes nothing
  B  n_lm = 300, n_cams = 10, seed = 7: 708 observations
  C  n_lm = 1000, n_cams = 10, seed = 7: more than two tiles of the correcting kernel, the last one partial (evaluate only)
  D  A plus cameras that observe nothing, enough to push the kernel off its cameras-in-LDS variant (evaluate only; built by the test
     from the kernel's own camera limit: with_idle_cameras)
At the start point the median sqrt(s) is 0.032 on A and 0.015 on B (tests/test_ba_loss_cpu.py asserts the fractions below).

Loss sets, on every observation (thresholds per scene; C and D use A's):
  "huber"     huber(0.03) on A, huber(0.015) on B
  "cauchy"    cauchy with the same a
  "tolerant"  tolerant(a, b) with a the scene's median s and b = a / 4: x = (s - a) / b passes 36.7 at s = 10.2 a, both branches occur
  "tukey"     tukey(a) with a at 1.5 x the huber threshold: the observations beyond a^2 have weight zero
  "mixed"     every kind, kind 0 and scales != 1 included, spread over ALL observations (evaluate only)
Tolerant's b is not small against a on purpose.  r' = rs(s) r depends on s through rho' = e^x / (1 + e^x), x = (s - a) / b: a relative
error d of s moves rho' by (s / b) (1 - rho') d, at most about (a / b) d.  The device's and numpy's r agree to some 4e-16 on residuals
of 0.03 (xn - f cancels), so d is 1e-14 .. 1e-13; with b = a / 60 that alone put r' 1e-14 apart, more than the evaluate bound -- which
carries the uncorrected entry's bound through the correction factor, not through the factor's derivative -- allows.  a / b <= 8 keeps
that term below the uncorrected bound itself."""
import functools

import numpy as np

import dogleg_ref as D
import lm_step_ref as L
import pg_loss_ref as G

EPS = L.EPS
LD = L.LD
KINDS = G.KINDS
SOLVE_SETS = ("huber", "cauchy", "tolerant", "tukey")
LOSS_SETS = SOLVE_SETS + ("mixed",)

# The worst relative error of the numpy rho' and rho'' against the 50-digit ones (pg_loss_ref.rho_mp) over the s of every loss set at
# the start points of A and B, per kind, in units of eps -- measured and asserted by
# tests/test_ba_loss_cpu.py::test_numpy_losses_match_the_50_digit_ones, which prints them; rounded up here.  (Not the pose graph's
# figures: s is 1e-6 .. 1e-1 here, not 1e-1 .. 1e3, and the thresholds sit inside the data.)
# The evaluate bound's c per kind is 8 x this figure (the margin for the device's libm) + CORRECTOR_ROUNDINGS (pg_loss_ref's count of
# the operations between rho', rho'' and an entry of r' or J'; the 2-term r^T J of an observation needs fewer, the figure is kept).
# Measured: trivial 0, huber 0.98, softlone 1.76, cauchy 2.13, arctan 2.39, tolerant 18.4 (e^x at x up to 36.7 carries |x| eps), tukey 4693
# (1 - s / a^2 cancels for the observations next to a^2 -- the threshold sits in the middle of the data -- where the entries themselves
# go to zero).
RHO_EPS = {"trivial": 0.0, "huber": 1.0, "softlone": 1.8, "cauchy": 2.2, "arctan": 2.4, "tolerant": 19.0, "tukey": 4700.0}
CORRECTOR_ROUNDINGS = G.CORRECTOR_ROUNDINGS


def c_of(kind):
    return 8.0 * np.array([RHO_EPS[KINDS[k]] for k in np.atleast_1d(kind)]) + CORRECTOR_ROUNDINGS


# ------------------------------------------------------------------------------------------ scenes
SCENES = {"A": dict(n_lm=33, extras=True), "B": dict(n_lm=300, n_cams=10, seed=7), "C": dict(n_lm=1000, n_cams=10, seed=7)}
HUBER_A = {"A": 0.03, "B": 0.015, "C": 0.03, "M": 0.03}
TOLERANT_A = {"A": 0.032 ** 2, "B": 0.015 ** 2, "C": 0.032 ** 2, "M": 0.032 ** 2}
TOLERANT_B_FRACTION = 0.25
TUKEY_FACTOR = 1.5


def masked_scene():
    """M: A's masks without A's extreme landmarks -- lm_step_ref.ba_scene(n_lm=33) with the per-dof constant masks of its extras
    (0b000111, 0b111000, one rotation bit, one translation bit on cameras 1..4), a camera that observes nothing and three constant
    landmarks.  124 observations, 9 cameras.  The far, the near and the near-parallel landmark of A put the dogleg's factorisation at
    mu = 1e-8 to kappa 1e12 with or without a loss; M is an accuracy case for it (kappa 5e4 .. 5e5 with Huber, Cauchy, Tolerant)"""
    s = L.ba_scene(n_lm=33)
    cams0, cams_true, cf = s["cams0"].copy(), s["cams_true"].copy(), s["cam_fixed"].copy()
    lone = cams0[2].copy(); lone[4:] += 0.5
    cams0, cams_true = np.vstack([cams0, lone]), np.vstack([cams_true, lone])
    cf = np.vstack([cf, np.zeros((1, 6), np.uint8)])
    for c, m in zip((1, 2, 3, 4), (0b000111, 0b111000, 0b000010, 0b010000)):
        cf[c] = [(m >> a) & 1 for a in range(6)]
    pf = np.zeros(len(s["pts0"]), np.uint8); pf[[0, 5, 9]] = 1
    return dict(s, cams0=cams0, cams_true=cams_true, cam_fixed=cf, pt_fixed=pf)


@functools.lru_cache(maxsize=None)
def scene(name):
    return masked_scene() if name == "M" else L.ba_scene(**SCENES[name])


def with_idle_cameras(s, n_total):
    """the scene with cameras that observe nothing appended (copies of camera 2, shifted), up to n_total cameras"""
    extra = n_total - len(s["cams0"])
    assert extra > 0
    idle = np.tile(s["cams0"][2], (extra, 1))
    idle[:, 4:] += 0.5 + 1e-3 * np.arange(extra)[:, None]
    return dict(s, cams0=np.vstack([s["cams0"], idle]), cams_true=np.vstack([s["cams_true"], idle]),
                cam_fixed=np.vstack([s["cam_fixed"], np.zeros((extra, 6), np.uint8)]))


def table_of(kind, a, b, scale, n):
    return dict(kind=np.broadcast_to(np.asarray(kind, np.int32), (n,)).copy(), a=np.broadcast_to(np.asarray(a, float), (n,)).copy(),
                b=np.broadcast_to(np.asarray(b, float), (n,)).copy(), scale=np.broadcast_to(np.asarray(scale, float), (n,)).copy())


def loss_table(sname, name, n):
    """the per-observation table (kind int32[n], a, b, scale float64[n]) of a loss set on scene sname (n observations)"""
    a = HUBER_A[sname]
    if name == "huber":
        return table_of(1, a, 1.0, 1.0, n)
    if name == "cauchy":
        return table_of(3, a, 1.0, 1.0, n)
    if name == "tolerant":
        return table_of(5, TOLERANT_A[sname], TOLERANT_A[sname] * TOLERANT_B_FRACTION, 1.0, n)
    if name == "tukey":
        return table_of(6, TUKEY_FACTOR * a, 1.0, 1.0, n)
    assert name == "mixed"
    rng = np.random.default_rng(91 + "ABCM".index(sname))
    kind = (np.arange(n) % 7).astype(np.int32)[rng.permutation(n)]
    ta = np.where(kind == 5, TOLERANT_A[sname] * rng.uniform(0.5, 2.0, n), a * rng.uniform(0.5, 3.0, n))
    tb = TOLERANT_A[sname] * rng.uniform(0.25, 1.0, n)
    scale = np.where(rng.uniform(size=n) < 0.5, 1.0, rng.uniform(0.25, 4.0, n))
    return dict(kind=kind, a=ta, b=tb, scale=scale)


def threshold(table):
    """s beyond which an observation is an outlier to its loss: a^2 (tolerant: a, which is compared with s itself); inf for trivial"""
    k = np.asarray(table["kind"])
    return np.where(k == 0, np.inf, np.where(k == 5, table["a"], table["a"] ** 2))


# ------------------------------------------------------------------------------------------ the corrector on BA blocks
def corrected_bound(r, table, x_corrected, base):
    """the evaluate bound of a corrected entry, as pg_loss_ref.corrected_bound for 2-vectors: the bound `base` of the uncorrected entry
    times the magnitude of the correction factor -- |rs| for r', |M| = |sq (I - k r r^T)| as a matrix for J' -- plus
    c eps |entry| (c_of)"""
    s = np.sum(r * r, 1)
    _, sq, rs, k = G.factors(table, s)
    keep = G.untouched(table)
    M = np.where(keep[:, None, None], np.eye(2), sq[:, None, None] * (np.eye(2) - k[:, None, None] * r[:, :, None] * r[:, None, :]))
    rs = np.where(keep, 1.0, rs)
    c = c_of(table["kind"])
    base = np.broadcast_to(base, x_corrected.shape)
    if x_corrected.ndim == 2:
        return np.abs(rs)[:, None] * base + c[:, None] * EPS * np.abs(x_corrected)
    return np.abs(M) @ base + c[:, None, None] * EPS * np.abs(x_corrected)


class RobustBAProblem(L.BAProblem):
    """bundle adjustment with every observation corrected: lin returns r' and J', cost is 1/2 sum rho"""

    def __init__(self, s, table):
        super().__init__(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], s.get("pt_fixed"))
        self.table = table

    def lin_obs_corrected(self, cams, pts, jac=True):
        """(r', Jc', Jp', rho[no]) per observation, every column (constant ones included)"""
        r, Jc, Jp = self.lin_obs(cams, pts, jac)
        return G.correct(r, Jc, Jp, self.table)

    def lin(self, x, jac=True):
        cams, pts = self.split(x)
        rc, Jc, Jp, _ = self.lin_obs_corrected(cams, pts, jac)
        return rc, (None if not jac else np.concatenate([Jc, Jp], 2)), self.cols

    def cost(self, x):
        cams, pts = self.split(x)
        return float(0.5 * np.sum(self.lin_obs_corrected(cams, pts, False)[3].astype(LD)))

    def s_of(self, x):
        cams, pts = self.split(x)
        r = self.lin_obs(cams, pts, False)[0]
        return np.sum(r * r, 1)


lm_reference = G.lm_reference          # the LM loop whose start cost is prob.cost (1/2 sum rho)


def dogleg_reference(prob, opt, k):
    """dogleg_ref.dogleg_reference's loop (its rules, its per-iteration dicts, its step: dogleg_ref.traditional_dogleg) with the START
    cost taken from prob.cost; no mutations.  dogleg_ref.compare works on the result unchanged."""
    n = prob.n_local
    fidx = np.nonzero(prob.free)[0]
    x = prob.x0.copy()
    radius, mu = float(opt["initial_trust_region_radius"]), D.MIN_MU
    dmin, dmax = opt["min_lm_diagonal"], opt["max_lm_diagonal"]

    def linearise(x):
        r, J, cols = prob.lin(x, True)
        H, g = L.normal_equations(n, r, J, cols)
        return r, J, cols, H, g

    def jdot(J, cols, v):
        return np.einsum("bea,ba->be", J.astype(LD), v.astype(LD)[cols])

    def gmax_of(g):
        return float(np.abs(g.astype(np.float64)[fidx]).max())

    r, J, cols, H, g = linearise(x)
    cost = prob.cost(x)
    start = dict(cost=cost, gmax=gmax_of(g), radius=radius)
    s, lin, out = None, None, []
    for _ in range(k):
        reused, escalations = lin is not None, 0
        if lin is None:
            Hd = np.diag(H).astype(np.float64)
            if s is None:
                s = 1.0 / (1.0 + np.sqrt(Hd)) if opt["jacobi_scaling"] else np.ones(n)
            d = np.sqrt(np.clip(s * s * Hd, dmin, dmax))[fidx]
            sL = s.astype(LD)
            A0 = (H * sL[:, None] * sL[None, :])[np.ix_(fidx, fidx)]
            gh = (sL * g)[fidx]
            gamma = (gh / d).astype(np.float64)
            du = np.zeros(n); du[fidx] = s[fidx] * (gamma / d)
            ju = jdot(J, cols, du)
            alpha = float(np.sum(gamma.astype(LD) ** 2) / np.sum(ju * ju))
            y_gn, A = None, None
            while mu < D.MAX_MU:
                A = A0 + np.diag((mu * d * d).astype(LD))
                try:
                    np.linalg.cholesky(A.astype(np.float64))
                    y = L.refined_solve(A, -gh).astype(np.float64)
                    ok = bool(np.all(np.isfinite(y)))
                except np.linalg.LinAlgError:
                    ok = False
                if ok:
                    y_gn = y
                    break
                mu *= D.MU_INCREASE
                escalations += 1
            lin = None if y_gn is None else dict(gamma=gamma, alpha=alpha, z_gn=d * y_gn, d=d, kappa=L.kappa2(A))
        valid = lin is not None
        if valid:
            gamma, alpha, d = lin["gamma"], lin["alpha"], lin["d"]
            z, kase, beta = D.traditional_dogleg(-alpha * gamma, lin["z_gn"], radius)
            delta = np.zeros(n)
            delta[fidx] = s[fidx] * (z / d)
            f = jdot(J, cols, delta)
            model = float(-np.sum(f * (r.astype(LD) + f / 2)))
            valid = bool(np.isfinite(model) and model > 0.0)
            kappa = lin["kappa"]
        else:
            z, kase, beta, delta, model, kappa = np.zeros(len(fidx)), -1, 0.0, np.zeros(n), 0.0, 1.0
        xt = prob.plus(x, delta)
        trial_cost = prob.cost(xt) if valid else cost
        ok = valid and np.isfinite(trial_cost)
        step_norm = float(np.linalg.norm(xt - x)) if ok else 0.0
        x_norm = float(np.linalg.norm(x[prob.x_norm_mask]))
        cost_change = cost - trial_cost if ok else 0.0
        rho = cost_change / model if ok else 0.0
        accepted = bool(ok and rho > opt["min_relative_decrease"])
        radius_before, z_norm = radius, float(np.linalg.norm(z))
        if accepted:
            if rho > 0.75:
                radius = max(radius, 3.0 * z_norm)
            elif rho < 0.25:
                radius *= 0.5
            radius = min(opt["max_trust_region_radius"], radius)
            mu = max(D.MIN_MU, 2.0 * mu / D.MU_INCREASE)
            x, cost = xt, trial_cost
            r, J, cols, H, g = linearise(x)
            lin = None
        elif not valid:
            mu *= D.MU_INCREASE
            lin = None
        else:
            radius *= 0.5
        out.append(dict(delta=delta, x=x.copy(), x_trial=xt, cost=cost, trial_cost=trial_cost if ok else cost,
                        cost_change=cost_change, model_change=model, rho=rho, step_norm=step_norm, x_norm=x_norm, gmax=gmax_of(g),
                        radius=radius, radius_before=radius_before, accepted=accepted, kappa=kappa, start=start, case=kase,
                        beta=beta, z=z, z_norm=z_norm, mu=mu, reused=reused, escalations=escalations, valid=valid))
    return out


# ------------------------------------------------------------------------------------------ the cases
def problem(sname, name):
    s = scene(sname)
    return RobustBAProblem(s, loss_table(sname, name, len(s["obs_cam"])))


# name -> (scene, loss set, option overrides); every case runs k = 1 and k = 3
SOLVE_CASES = {
    "A_huber": ("A", "huber", dict(initial_trust_region_radius=1e-3)),
    "A_cauchy": ("A", "cauchy", dict(initial_trust_region_radius=1.0)),
    "A_tolerant": ("A", "tolerant", dict(initial_trust_region_radius=1e-3)),
    "A_tukey": ("A", "tukey", dict(initial_trust_region_radius=1e-3)),
    "B_huber": ("B", "huber", dict(initial_trust_region_radius=1e-3)),
    "B_cauchy": ("B", "cauchy", dict(initial_trust_region_radius=1e16)),
    "B_tolerant": ("B", "tolerant", dict(initial_trust_region_radius=1e-3)),
    "B_tukey": ("B", "tukey", dict(initial_trust_region_radius=1e-3)),
    # (DOGLEG only)
    "M_huber": ("M", "huber", dict(initial_trust_region_radius=1.0)),
    "M_cauchy": ("M", "cauchy", dict(initial_trust_region_radius=1.0)),
    "M_tolerant": ("M", "tolerant", dict(initial_trust_region_radius=1e-2)),
    "M_tukey": ("M", "tukey", dict(initial_trust_region_radius=1e-2)),
}
LM_CASES = tuple(c for c in SOLVE_CASES if not c.startswith("M_"))


# DOGLEG factors the reduced system at mu = 1e-8.  On scene A (the far, the near and the near-parallel landmark) kappa is then 1e12 with
# or without a loss: A is no accuracy case for dogleg.  Its masks are: scene M carries A's constant dofs, constant landmarks and idle
# camera, and with Huber (an interpolated, then Gauss-Newton steps), Cauchy (Gauss-Newton) and Tolerant (Cauchy steps) it is one; so is B
# with Huber, Cauchy and Tolerant.  Tukey's zero weights leave landmark blocks that mu = 1e-8 alone holds up (kappa 1e10 on M, 3e13 on B):
# DOGLEG_LOOSE_CASES are compared with the same formulas at THAT kappa -- looser, but asserted, decisions and dogleg cases included.
DOGLEG_CASES = ("M_huber", "M_cauchy", "M_tolerant", "B_huber", "B_cauchy", "B_tolerant")
DOGLEG_LOOSE_CASES = ("M_tukey", "B_tukey")


@functools.lru_cache(maxsize=None)
def reference(case, k, strategy="lm"):
    """the robust reference loop, computed once per case and shared (read-only) by the tests"""
    sname, name, ok = SOLVE_CASES[case]
    o = L.lm_options(**ok)
    return (lm_reference if strategy == "lm" else dogleg_reference)(problem(sname, name), o, k)


# a rejected step inside three iterations: lm_step_ref's "reject_then_accept" scene (landmarks 3 m off) with a loss
# (sqrt(s) has its median at 0.40 there: huber(0.4) has half of the observations beyond a^2.  At the scene's own radius of 100 the
# robust cost accepts the first step; from 1000 the reference rejects two steps and accepts the third)
REJECT_SCENE = L.BA_CASES["reject_then_accept"][0]
REJECT_HUBER_A, REJECT_RADIUS = 0.4, 1e3


@functools.lru_cache(maxsize=None)
def reject_case():
    s = L.ba_scene(**REJECT_SCENE)
    table = table_of(1, REJECT_HUBER_A, 1.0, 1.0, len(s["obs_cam"]))
    return s, table, L.lm_options(initial_trust_region_radius=REJECT_RADIUS)


@functools.lru_cache(maxsize=None)
def reject_reference(k):
    s, table, o = reject_case()
    return lm_reference(RobustBAProblem(s, table), o, k)


# ------------------------------------------------------------------------------------------ outliers
OUTLIER_FRACTION, OUTLIER_SHIFT, OUTLIER_CAUCHY_A = 0.1, 0.5, 0.015


@functools.lru_cache(maxsize=None)
def outlier_scene():
    """B with 10 % of the features displaced by 0.5 (a seeded choice, a seeded direction): one observation each of landmarks that
    three or four cameras see -- two thirds of B's landmarks are seen twice, and with one of two rays wrong no loss can place them"""
    s = scene("B")
    rng = np.random.default_rng(2027)
    n = len(s["obs_cam"])
    seen = np.bincount(s["obs_pt"])
    pick = rng.choice(np.flatnonzero(seen >= 3), int(round(OUTLIER_FRACTION * n)), replace=False)
    bad = np.sort(np.array([rng.choice(np.flatnonzero(s["obs_pt"] == j)) for j in pick]))
    ang = rng.uniform(0, 2 * np.pi, len(bad))
    feat = s["obs_feat"].copy()
    feat[bad] += OUTLIER_SHIFT * np.stack([np.cos(ang), np.sin(ang)], 1)
    return dict(s, obs_feat=feat), bad


def distance_to_truth(prob, s, x):
    """|x - truth| over the parameters (lm_step_ref.point_error's norm)"""
    return L.point_error(prob, x, np.concatenate([s["cams_true"].reshape(-1), s["pts_true"].reshape(-1)]))


@functools.lru_cache(maxsize=None)
def outlier_references():
    """(x of the L2 reference solve, x and final cost of the Cauchy reference solve, the Cauchy table) on the outlier scene"""
    s, _ = outlier_scene()
    o = L.lm_options()
    plain = L.lm_reference(L.ba_problem(s), o, o["max_num_iterations"])
    table = table_of(3, OUTLIER_CAUCHY_A, 1.0, 1.0, len(s["obs_cam"]))
    rob = lm_reference(RobustBAProblem(s, table), o, o["max_num_iterations"])
    return plain[-1]["x"], rob[-1]["x"], rob[-1]["cost"], table


# ------------------------------------------------------------------------------------------ s == 0
def zero_scene():
    """s == 0 EXACTLY on every implementation, fused multiply-adds or not: three cameras with the identity rotation at (0, 0, 0),
    (1, 0, 0), (2, 0, 0), fourteen landmarks at depth 2 with dyadic coordinates, every one seen by every camera, the features what the
    projection gives -- L - t, the rotation (entries 0 and 1), 1 / z = 0.5 and the products with it are all exact.  Every kind six
    times, scales 1 and 2 (tolerant has rho'' > 0 there: the corrector must take its first branch because s == 0); camera 0 constant"""
    nc, nl = 3, 14
    cams = np.tile(np.array([0.0, 0, 0, 1, 0, 0, 0]), (nc, 1))
    cams[:, 4] = np.arange(nc)
    pts = np.stack([0.25 * np.arange(nl) - 1.5, 0.125 * np.arange(nl) - 0.5, np.full(nl, 2.0)], 1)
    op = np.repeat(np.arange(nl), nc).astype(np.int32)
    oc = np.tile(np.arange(nc), nl).astype(np.int32)
    feat = (pts[op] - cams[oc, 4:])[:, :2] * 0.5
    fixed = np.zeros((nc, 6), np.uint8); fixed[0] = 1
    s = dict(cams0=cams, pts0=pts, obs_cam=oc, obs_pt=op, obs_feat=feat, cam_fixed=fixed, pt_fixed=np.zeros(nl, np.uint8))
    n = nc * nl
    kind = (np.arange(n) % 7).astype(np.int32)
    return s, dict(kind=kind, a=np.full(n, 0.5), b=np.full(n, 0.4), scale=np.where(np.arange(n) < n // 2, 1.0, 2.0))
