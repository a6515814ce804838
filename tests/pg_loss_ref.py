"""Reference for the pose graph's robust loss functions (PGEngine(loss=), stba_pg_set_loss): Ceres' losses and Ceres' corrector in numpy
on top of tests/pg_information_ref.py's whitened problem.  CPU only (numpy, + mpmath for the 50-digit losses).

Per edge, with r~ = W r and J~ = W J (W = I without weights) and s = |r~|^2, a loss rho(s) (Ceres' loss_function.h):

    kind 0 trivial         rho = s
    kind 1 huber(a)        s for s <= a^2, else 2 a sqrt(s) - a^2
    kind 2 softlone(a)     2 a^2 (sqrt(1 + s / a^2) - 1)
    kind 3 cauchy(a)       a^2 log(1 + s / a^2)
    kind 4 arctan(a)       a atan2(s, a)
    kind 5 tolerant(a, b)  b log(1 + e^((s - a) / b)) - b log(1 + e^(-a / b)); linear once (s - a) / b > 36.7
    kind 6 tukey(a)        (a^2 / 3) (1 - (1 - s / a^2)^3) for s <= a^2, else a^2 / 3 with rho' = rho'' = 0

rho' is clamped from below by DBL_MIN where Ceres clamps it; `scale` multiplies rho, rho', rho'' (ScaledLoss).  The corrector
(Ceres' corrector.cc): with sq = sqrt(rho'),
    s == 0 or rho'' <= 0:   r' = sq r~,               J' = sq J~
    otherwise:              D = 1 + 2 s rho'' / rho', alpha = 1 - sqrt(D),
                            r' = sq / (1 - alpha) r~,  J' = sq (J~ - (alpha / s) r~ (r~^T J~))
and the edge's cost term is rho(s); the cost is 1/2 sum rho.  J'^T r' = rho' J~^T r~ in both branches.

The inputs of the tests (tests/test_pg_loss_cpu.py checks their properties): the graphs "n60" (179 edges) and "n40_pad" (304 edges) of
pg_information_ref.  At poses0 the odometry edges (the first n - 1) have s = 0 up to rounding (below 1e-28); the loop closures carry the loss:
  "huber"     huber(0.5) on the loops
  "cauchy_w"  cauchy(20) on the loops on top of the "dense" weights (s is the whitened one: a median of some hundreds)
  "tolerant"  tolerant(0.3, 0.02) on the loops: x = (s - a) / b passes 36.7 at s = 1.034, so both branches occur
  "tukey"     tukey(0.6) on the loops
  "mixed"     every kind, kind 0 and scales != 1 included, spread over ALL edges (evaluate only)."""
import functools

import numpy as np

import lm_step_ref as L
import pg_information_ref as P

EPS = L.EPS
LD = L.LD
DBL_MIN = np.finfo(np.float64).tiny
KINDS = ("trivial", "huber", "softlone", "cauchy", "arctan", "tolerant", "tukey")
SOLVE_SETS = ("huber", "cauchy_w", "tolerant", "tukey")
LOSS_SETS = SOLVE_SETS + ("mixed",)
TOLERANT_LINEAR = 36.7

# The worst relative error of the numpy rho' and rho'' (what the corrector's factors are made of) against the 50-digit ones over the s
# of every loss set at poses0, per kind, in units of eps -- measured and asserted by
# tests/test_pg_loss_cpu.py::test_numpy_losses_match_the_50_digit_ones, which prints: trivial 0, huber 1.01, softlone 1.37,
# cauchy 2.06, arctan 1.98, tolerant 25.0 (e^x at x up to 36.7 carries |x| eps), tukey 428 (1 - s / a^2 cancels for the loops next to
# a^2, where the entries themselves go to zero); rounded up here.
# The evaluate bound's c per kind is 8 x this figure (the margin for the device's libm) + CORRECTOR_ROUNDINGS, the operations
# between rho', rho'' and an entry of r' or J' (sqrt, D, sqrt, 1 - alpha, two divisions, the 6-term r^T J, a product, a difference,
# a product).
RHO_EPS = {"trivial": 0.0, "huber": 1.1, "softlone": 1.4, "cauchy": 2.1, "arctan": 2.0, "tolerant": 26.0, "tukey": 430.0}
CORRECTOR_ROUNDINGS = 16.0


def c_of(kind):
    return 8.0 * np.array([RHO_EPS[KINDS[k]] for k in np.atleast_1d(kind)]) + CORRECTOR_ROUNDINGS


# ------------------------------------------------------------------------------------------ the losses
def rho(kind, a, b, scale, s):
    """rho, rho', rho'' (each [m]) of the per-edge table at s[m], in FP64 -- Ceres' formulas operation for operation"""
    kind, s = np.asarray(kind), np.asarray(s, float)
    a, b, scale = (np.broadcast_to(np.asarray(v, float), s.shape) for v in (a, b, scale))
    out = np.stack([s, np.ones_like(s), np.zeros_like(s)])
    with np.errstate(all="ignore"):
        b2 = a * a
        q = np.sqrt(s)
        r1 = np.maximum(DBL_MIN, a / q)
        hub = np.stack([2 * a * q - b2, r1, -r1 / (2 * s)])
        out = np.where((kind == 1) & (s > b2), hub, out)
        c = 1 / b2
        su = 1 + s * c; t = np.sqrt(su); r1 = np.maximum(DBL_MIN, 1 / t)
        out = np.where(kind == 2, np.stack([2 * b2 * (t - 1), r1, -(c * r1) / (2 * su)]), out)
        inv = 1 / su
        out = np.where(kind == 3, np.stack([b2 * np.log(su), np.maximum(DBL_MIN, inv), -c * (inv * inv)]), out)
        su = 1 + s * s * c; inv = 1 / su
        out = np.where(kind == 4, np.stack([a * np.arctan2(s, a), np.maximum(DBL_MIN, inv), -2 * s * c * (inv * inv)]), out)
        cc = b * np.log(1 + np.exp(-a / b)); x = (s - a) / b; ex = np.exp(x)
        tol = np.stack([b * np.log(1 + ex) - cc, np.maximum(DBL_MIN, ex / (1 + ex)), 0.5 / (b * (1 + np.cosh(x)))])
        tol = np.where(x > TOLERANT_LINEAR, np.stack([s - a - cc, np.ones_like(s), np.zeros_like(s)]), tol)
        out = np.where(kind == 5, tol, out)
        v = 1 - s / b2; v2 = v * v
        tuk = np.where(s <= b2, np.stack([b2 / 3 * (1 - v2 * v), v2, -2 / b2 * v]), np.stack([b2 / 3, np.zeros_like(s), np.zeros_like(s)]))
        out = np.where(kind == 6, tuk, out)
    return out * scale


def rho_mp(kind, a, b, scale, s):
    """one edge at 50 digits (the FP64 inputs taken as exact): (rho, rho', rho'') as mpmath numbers"""
    import mpmath as mp
    with mp.workdps(50):
        a, b, scale, s = mp.mpf(float(a)), mp.mpf(float(b)), mp.mpf(float(scale)), mp.mpf(float(s))
        tiny = mp.mpf(float(DBL_MIN))
        if kind == 0:
            out = (s, mp.mpf(1), mp.mpf(0))
        elif kind == 1:
            out = (s, mp.mpf(1), mp.mpf(0)) if s <= a * a else (2 * a * mp.sqrt(s) - a * a, max(tiny, a / mp.sqrt(s)), -max(tiny, a / mp.sqrt(s)) / (2 * s))
        elif kind == 2:
            su = 1 + s / (a * a)
            out = (2 * a * a * (mp.sqrt(su) - 1), max(tiny, 1 / mp.sqrt(su)), -max(tiny, 1 / mp.sqrt(su)) / (a * a) / (2 * su))
        elif kind == 3:
            su = 1 + s / (a * a)
            out = (a * a * mp.log(su), max(tiny, 1 / su), -1 / (a * a * su * su))
        elif kind == 4:
            su = 1 + s * s / (a * a)
            out = (a * mp.atan2(s, a), max(tiny, 1 / su), -2 * s / (a * a * su * su))
        elif kind == 5:
            c = b * mp.log(1 + mp.exp(-a / b)); x = (s - a) / b
            if x > mp.mpf(TOLERANT_LINEAR):
                out = (s - a - c, mp.mpf(1), mp.mpf(0))
            else:
                out = (b * mp.log(1 + mp.exp(x)) - c, max(tiny, mp.exp(x) / (1 + mp.exp(x))), mp.mpf(0.5) / (b * (1 + mp.cosh(x))))
        else:
            v = 1 - s / (a * a)
            out = (a * a / 3 * (1 - v ** 3), v * v, -2 / (a * a) * v) if s <= a * a else (a * a / 3, mp.mpf(0), mp.mpf(0))
        return tuple(scale * o for o in out)


# ------------------------------------------------------------------------------------------ the corrector
def factors(table, s):
    """(rho[3, m], sq, rs, k): r' = rs r~, J' = sq (J~ - k r~ (r~^T J~))"""
    rh = rho(table["kind"], table["a"], table["b"], table["scale"], s)
    sq = np.sqrt(rh[1])
    second = (s != 0) & (rh[2] > 0)
    with np.errstate(all="ignore"):
        alpha = np.where(second, 1 - np.sqrt(1 + 2 * s * rh[2] / rh[1]), 0.0)
        rs = np.where(second, sq / (1 - alpha), sq)
        k = np.where(second, alpha / s, 0.0)
    return rh, sq, rs, k


def untouched(table):
    """edges the corrector leaves alone: kind 0 with scale 1"""
    return (np.asarray(table["kind"]) == 0) & (np.asarray(table["scale"]) == 1.0)


def correct(r, Ji, Jj, table):
    """(r', Ji', Jj', rho[m]) of the whitened r[m, 6], Ji, Jj[m, 6, 6] (Ji, Jj None: the residual and the cost terms only)"""
    s = np.sum(r * r, 1)
    rh, sq, rs, k = factors(table, s)
    keep = untouched(table)
    rc = np.where(keep[:, None], r, rs[:, None] * r)
    cost_terms = np.where(keep, s, rh[0])
    if Ji is None:
        return rc, None, None, cost_terms

    def jac(J):
        t = np.einsum("ea,eac->ec", r, J)
        return np.where(keep[:, None, None], J, sq[:, None, None] * (J - k[:, None, None] * r[:, :, None] * t[:, None, :]))
    return rc, jac(Ji), jac(Jj), cost_terms


def correction_matrix(r, table):
    """M[m, 6, 6] = sq (I - k r r^T): J' = M J~"""
    s = np.sum(r * r, 1)
    _, sq, rs, k = factors(table, s)
    M = sq[:, None, None] * (np.eye(6) - k[:, None, None] * r[:, :, None] * r[:, None, :])
    keep = untouched(table)
    return np.where(keep[:, None, None], np.eye(6), M), np.where(keep, 1.0, rs)


def corrected_bound(r, table, x_corrected, base):
    """the evaluate bound of a corrected entry: the bound `base` of the uncorrected (whitened) entry times the magnitude of the
    correction factor -- |rs| for r, |M| as a matrix for J -- plus c eps |entry| (c_of: what evaluating rho and the corrector costs)"""
    M, rs = correction_matrix(r, table)
    c = c_of(table["kind"])
    base = np.broadcast_to(base, x_corrected.shape)
    if x_corrected.ndim == 2:
        return np.abs(rs)[:, None] * base + c[:, None] * EPS * np.abs(x_corrected)
    return np.abs(M) @ base + c[:, None, None] * EPS * np.abs(x_corrected)


# ------------------------------------------------------------------------------------------ the problem and its LM loop
class RobustPGProblem(P.WeightedPGProblem):
    """the whitened problem with every edge corrected: lin returns r' and J', cost is 1/2 sum rho"""

    def __init__(self, g, W, table):
        super().__init__(g, W)
        self.table = table

    def lin(self, x, jac=True):
        r, J, cols = super().lin(x, jac)
        if J is None:
            return correct(r, None, None, self.table)[0], None, cols
        rc, Ji, Jj, _ = correct(r, J[:, :, :6], J[:, :, 6:], self.table)
        return rc, np.concatenate([Ji, Jj], 2), cols

    def cost(self, x):
        r = P.WeightedPGProblem.lin(self, x, False)[0]
        return float(0.5 * np.sum(correct(r, None, None, self.table)[3].astype(LD)))


def lm_reference(prob, opt, k):
    """lm_step_ref.lm_reference's loop (its step policy, its per-iteration dicts) with the START cost taken from prob.cost: with a
    loss 1/2 |r'|^2 is not the cost.  The model is Ceres': 1/2 |r'|^2 - 1/2 |r' + J' delta|^2 on the corrected r', J'.  No mutations,
    no Gauss-Newton mode, no bounds (lm_step_ref.compare, tolerances and rho_margin_ok work on the result unchanged)."""
    n, free = prob.n_local, prob.free
    fidx = np.nonzero(free)[0]
    x = prob.x0.copy()
    radius, v = float(opt["initial_trust_region_radius"]), 2.0

    def linearise(x):
        r, J, cols = prob.lin(x, True)
        H, g = L.normal_equations(n, r, J, cols)
        return r, J, cols, H, g

    def gmax_of(g):
        return float(np.abs(g.astype(np.float64)[fidx]).max())

    r, J, cols, H, g = linearise(x)
    cost = prob.cost(x)
    start = dict(cost=cost, gmax=gmax_of(g), radius=radius, hdiag=np.diag(H).astype(np.float64))
    out, scale = [], None
    for _ in range(k):
        Hd = np.diag(H).astype(np.float64)
        if scale is None:
            scale = 1.0 / (1.0 + np.sqrt(Hd)) if opt["jacobi_scaling"] else np.ones(n)
        s = scale
        D = np.clip(s * s * Hd, opt["min_lm_diagonal"], opt["max_lm_diagonal"]) / radius
        sL = s.astype(LD)
        A = (H * sL[:, None] * sL[None, :])[np.ix_(fidx, fidx)] + np.diag(D[fidx].astype(LD))
        y = L.refined_solve(A, -(sL * g)[fidx])
        delta = np.zeros(n)
        delta[fidx] = (sL[fidx] * y).astype(np.float64)
        kappa = L.kappa2(A)
        f = np.einsum("bea,ba->be", J.astype(LD), delta.astype(LD)[cols])
        model = float(-np.sum(f * (r.astype(LD) + f / 2)))
        xt = prob.plus(x, delta)
        trial_cost = prob.cost(xt)
        step_norm = float(np.linalg.norm(xt - x))
        x_norm = float(np.linalg.norm(x[prob.x_norm_mask]))
        cost_change = cost - trial_cost
        rho_ = cost_change / model if model != 0 else 0.0
        accepted = bool(rho_ > opt["min_relative_decrease"])
        radius_before = radius
        if accepted:
            t3 = 2.0 * rho_ - 1.0
            divisor = max(1.0 / 3.0, 1.0 - t3 * t3 * t3)
            radius = min(opt["max_trust_region_radius"], radius / divisor)
            v = 2.0
            x, cost = xt, trial_cost
            r, J, cols, H, g = linearise(x)
        else:
            divisor = v
            radius /= v
            v *= 2.0
        out.append(dict(delta=delta, x=x.copy(), x_trial=xt, cost=cost, trial_cost=trial_cost, cost_change=cost_change,
                        model_change=model, rho=rho_, step_norm=step_norm, x_norm=x_norm, gmax=gmax_of(g), radius=radius,
                        radius_before=radius_before, divisor=divisor, accepted=accepted, kappa=kappa, start=start))
    return out


# ------------------------------------------------------------------------------------------ the loss sets
def n_odometry(g):
    return len(g["poses0"]) - 1


def _on_loops(g, kind, a, b=1.0, scale=1.0):
    m = len(g["edge_i"])
    loop = np.arange(m) >= n_odometry(g)
    return dict(kind=np.where(loop, kind, 0).astype(np.int32), a=np.where(loop, a, 1.0), b=np.where(loop, b, 1.0), scale=np.full(m, scale))


HUBER_A, CAUCHY_W_A, TOLERANT_AB, TUKEY_A = 0.5, 20.0, (0.3, 0.02), 0.6


@functools.lru_cache(maxsize=None)
def loss_set(gname, name):
    """(table, weight set | None): the per-edge table (kind int32[m], a, b, scale float64[m]) and the weights it runs on"""
    g = P.graph(gname)
    m = len(g["edge_i"])
    if name == "huber":
        return _on_loops(g, 1, HUBER_A), None
    if name == "cauchy_w":
        return _on_loops(g, 3, CAUCHY_W_A), "dense"
    if name == "tolerant":
        return _on_loops(g, 5, *TOLERANT_AB), None
    if name == "tukey":
        return _on_loops(g, 6, TUKEY_A), None
    assert name == "mixed"
    rng = np.random.default_rng(77 + P.GRAPHS.index(gname))
    kind = (np.arange(m) % 7).astype(np.int32)[rng.permutation(m)]
    a = rng.uniform(0.3, 1.2, m)
    b = rng.uniform(0.02, 0.3, m)
    scale = np.where(rng.uniform(size=m) < 0.5, 1.0, rng.uniform(0.25, 4.0, m))
    return dict(kind=kind, a=a, b=b, scale=scale), None


def sqrt_information(gname, name):
    _, wname = loss_set(gname, name)
    g = P.graph(gname)
    return np.tile(np.eye(6), (len(g["edge_i"]), 1, 1)) if wname is None else P.weights(gname, wname)[1]


def problem(gname, name, g=None):
    return RobustPGProblem(g or P.graph(gname), sqrt_information(gname, name), loss_set(gname, name)[0])


@functools.lru_cache(maxsize=None)
def reference(gname, name, k):
    """the robust reference LM, computed once per case and shared (read-only) by the tests"""
    return lm_reference(problem(gname, name), L.lm_options(**P.LM_OPTIONS), k)


def engine_kwargs(gname, name):
    table, wname = loss_set(gname, name)
    kw = dict(loss=dict(table))
    if wname is not None:
        kw.update(P.engine_kwargs(gname, wname))
    return kw


def s_at_start(gname, name):
    """s = |W r|^2 per edge at poses0"""
    g = P.graph(gname)
    r = P.WeightedPGProblem(g, sqrt_information(gname, name)).lin(np.asarray(g["poses0"], float).reshape(-1), False)[0]
    return np.sum(r * r, 1)


def zero_graph():
    """s == 0 EXACTLY on every implementation: 15 nodes at the identity pose, identity measurements, 14 chain edges; every kind twice
    (tolerant has rho'' > 0 there: the corrector must take its first branch because s == 0, not because of rho'')"""
    n = 15
    poses = np.tile(np.array([0.0, 0, 0, 1, 0, 0, 0]), (n, 1))
    fixed = np.zeros(n, np.uint8); fixed[0] = 1
    ei = np.arange(n - 1, dtype=np.int32)
    g = dict(poses0=poses, edge_i=ei, edge_j=ei + 1, meas=np.tile(poses[0], (n - 1, 1)), node_fixed=fixed)
    kind = (np.arange(n - 1) % 7).astype(np.int32)
    return g, dict(kind=kind, a=np.full(n - 1, 0.5), b=np.full(n - 1, 0.4), scale=np.where(np.arange(n - 1) < 7, 1.0, 2.0))


# ------------------------------------------------------------------------------------------ outliers
@functools.lru_cache(maxsize=None)
def outlier_graph():
    """n60 with six loop-closure measurements replaced by seeded random poses"""
    g = P.graph("n60")
    rng = np.random.default_rng(2026)
    m, n0 = len(g["edge_i"]), n_odometry(g)
    bad = np.sort(rng.choice(np.arange(n0, m), 6, replace=False))
    xi = np.concatenate([rng.uniform(-4, 4, (6, 3)), rng.uniform(-1.5, 1.5, (6, 3))], 1)
    meas = g["meas"].copy()
    meas[bad] = L.rt_pose(*L.se3_exp(xi))
    return dict(g, meas=meas), bad


OUTLIER_CAUCHY_A = 0.5


@functools.lru_cache(maxsize=None)
def outlier_references():
    """(x of the L2 reference solve, x and final cost of the Cauchy reference solve, the Cauchy table) on the outlier graph"""
    g, _ = outlier_graph()
    m = len(g["edge_i"])
    o = L.lm_options(**P.LM_OPTIONS)
    plain = L.lm_reference(L.pg_problem(g), o, o["max_num_iterations"])
    table = _on_loops(g, 3, OUTLIER_CAUCHY_A)
    rob = lm_reference(RobustPGProblem(g, np.tile(np.eye(6), (m, 1, 1)), table), o, o["max_num_iterations"])
    return plain[-1]["x"], rob[-1]["x"], rob[-1]["cost"], table
