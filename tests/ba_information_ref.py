"""Reference for bundle adjustment's per-observation information matrices (BAEngine(information=), stba_ba_set_information,
stba_ba_set_sqrt_information): a 2 x 2 square-root information W_i per observation in front of ba_loss_ref's corrector.  CPU only
(numpy; mpmath for the 50-digit Cholesky factor of a 2 x 2).

Per observation: r~ = W r, Jc~ = W Jc, Jp~ = W Jp, s = |r~|^2 = r^T Omega r (Omega = W^T W); then pg_loss_ref.correct on the whitened
triple if the observation has a loss.  The cost is 1/2 sum rho(s).  Nothing else is restated: the problem, the scenes, the loss
tables, the LM and dogleg loops and the comparisons are ba_loss_ref's, lm_step_ref's and dogleg_ref's.

Weight families, seeded, W = s Rot(phi) diag(1, tau) with phi uniform in [0, 2 pi):
  "mild"   s in [0.7, 1.4], tau in [1, 2]        (solves: kappa of the damped system stays where lm_step_ref.tolerances applies)
  "wide"   s in [0.1, 10] (log-uniform), tau in [1, 100] (log-uniform)        (evaluate and the factorisation only)
Omega = W^T W = s^2 diag(1, tau^2) does not see Rot(phi): the factor the engine makes from Omega, W' = L^T, differs from W by an
orthogonal factor, so cost, J^T J and J^T r agree while r does not.

The evaluate bound of a whitened entry: the two-term product sum_k W_jk x_k of entries x_k known to base_k carries
sum_k |W_jk| base_k, plus 4 eps |entry| for the product's own roundings (two products and a sum, fused or not; where the two terms
cancel, their roundings -- eps |W_jk x_k| each -- sit far below the first term: base is 1e-14 on residuals of 1e-2, 1e-12 on
Jacobian entries of 1 .. 10)."""
import functools

import numpy as np

import ba_loss_ref as B
import dogleg_ref as D
import lm_step_ref as L
import pg_loss_ref as G

EPS = L.EPS
LD = L.LD
FACTOR_BOUND = 4.0 * EPS          # relative, per entry of W = L^T against the exact factor (include/stba.h)


# ------------------------------------------------------------------------------------------ weights
def rot(phi):
    c, s = np.cos(phi), np.sin(phi)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


def weights(family, n, seed=0):
    """W[n, 2, 2] = s Rot(phi) diag(1, tau) of a family"""
    rng = np.random.default_rng(1000 + seed)
    phi = rng.uniform(0, 2 * np.pi, n)
    if family == "mild":
        s, tau = rng.uniform(0.7, 1.4, n), rng.uniform(1.0, 2.0, n)
    else:
        assert family == "wide"
        s, tau = 10.0 ** rng.uniform(-1, 1, n), 10.0 ** rng.uniform(0, 2, n)
    W = rot(phi) * s[:, None, None]
    W[:, :, 1] *= tau[:, None]
    return W


def information_of(W):
    """Omega = W^T W, made exactly symmetric"""
    Om = np.einsum("nki,nkj->nij", W, W)
    Om[:, 1, 0] = Om[:, 0, 1]
    return Om


def is_identity(W):
    return np.all(W == np.eye(2), axis=(1, 2))


def chol2_mp(Om):
    """W = L^T with Omega = L L^T, from the lower triangle of each 2 x 2 of Om[n, 2, 2], at 50 digits: a list of 4-tuples of mpf
    (row-major W), None where the matrix is not positive definite"""
    import mpmath as mp
    out = []
    with mp.workdps(50):
        for M in np.asarray(Om, float).reshape(-1, 2, 2):
            a, b, c = mp.mpf(float(M[0, 0])), mp.mpf(float(M[1, 0])), mp.mpf(float(M[1, 1]))
            if not a > 0 or not c - b * b / a > 0:
                out.append(None)
                continue
            l11 = mp.sqrt(a)
            l21 = b / l11
            out.append((l11, l21, mp.mpf(0), mp.sqrt(c - b * b / a)))
    return out


def factor_error(W_dev, Om):
    """the worst relative error per entry of W_dev[n, 2, 2] against the 50-digit factor of Om, in units of eps (a zero must be a zero)"""
    import mpmath as mp
    worst = 0.0
    with mp.workdps(50):
        for Wd, ref in zip(np.asarray(W_dev).reshape(-1, 4), chol2_mp(Om)):
            assert ref is not None
            for got, want in zip(Wd, ref):
                if want == 0:
                    assert got == 0.0
                    continue
                worst = max(worst, float(abs(mp.mpf(float(got)) - want) / abs(want)) / EPS)
    return worst


def ill_conditioned(n, seed=3):
    """Omega[n, 2, 2] = Q diag(1, 1 / kappa) Q^T scale with kappa log-uniform in [1, 1e12], Q a rotation, scale log-uniform in
    [1e-6, 1e6]: the pivot c - b^2 / a cancels up to 12 digits"""
    rng = np.random.default_rng(seed)
    kap = 10.0 ** rng.uniform(0, 12, n)
    kap[:4] = 1e12
    Q = rot(rng.uniform(0, 2 * np.pi, n))
    sc = 10.0 ** rng.uniform(-6, 6, n)
    Om = np.einsum("nik,nk,njk->nij", Q, np.stack([np.ones(n), 1.0 / kap], 1) * sc[:, None], Q)
    Om[:, 1, 0] = Om[:, 0, 1]
    return Om, kap


# ------------------------------------------------------------------------------------------ the problem
def whiten(W, r, Jc, Jp):
    keep = is_identity(W)

    def w(x):
        if x is None:
            return None
        y = np.einsum("nij,nj...->ni...", W, x)
        return np.where(keep.reshape((-1,) + (1,) * (x.ndim - 1)), x, y)
    return w(r), w(Jc), w(Jp)


def trivial_table(n):
    return B.table_of(0, 1.0, 1.0, 1.0, n)


class WeightedBAProblem(B.RobustBAProblem):
    """bundle adjustment with every observation whitened by W[n, 2, 2], then corrected by `table` (None: no loss)"""

    def __init__(self, s, W, table=None):
        n = len(s["obs_cam"])
        super().__init__(s, trivial_table(n) if table is None else table)
        self.W = np.broadcast_to(np.eye(2), (n, 2, 2)).copy() if W is None else np.asarray(W, float).reshape(n, 2, 2)

    def lin_obs_whitened(self, cams, pts, jac=True):
        return whiten(self.W, *self.lin_obs(cams, pts, jac))

    def lin_obs_corrected(self, cams, pts, jac=True):
        r, Jc, Jp = self.lin_obs_whitened(cams, pts, jac)
        return G.correct(r, Jc, Jp, self.table)

    def s_of(self, x):
        cams, pts = self.split(x)
        r = self.lin_obs_whitened(cams, pts, False)[0]
        return np.sum(r * r, 1)


def whitened_base(W, x, base):
    """the bound of a whitened entry (this module's docstring): x[n, 2] or x[n, 2, k] the UNWHITENED entries, base their bound;
    identity rows keep base"""
    aW = np.abs(W)
    if x.ndim == 2:
        lin = np.einsum("nij,nj->ni", aW, np.broadcast_to(base, x.shape))
        y = np.einsum("nij,nj->ni", W, x)
    else:
        lin = np.einsum("nij,njk->nik", aW, np.broadcast_to(base, x.shape))
        y = np.einsum("nij,njk->nik", W, x)
    out = lin + 4 * EPS * np.abs(y)
    keep = is_identity(W).reshape((-1,) + (1,) * (x.ndim - 1))
    return np.where(keep, np.broadcast_to(base, x.shape), out)


# ------------------------------------------------------------------------------------------ the cases
LOSSES = (None, "huber", "cauchy")
# name -> (scene, loss set or None, option overrides): mild weights, seed = the scene's index; every case runs k = 1 and k = 3
SOLVE_CASES = {
    "A_none": ("A", None, dict(initial_trust_region_radius=1e-3)),
    "A_huber": ("A", "huber", dict(initial_trust_region_radius=1e-3)),
    "A_cauchy": ("A", "cauchy", dict(initial_trust_region_radius=1.0)),
    "B_none": ("B", None, dict(initial_trust_region_radius=1e-3)),
    "B_huber": ("B", "huber", dict(initial_trust_region_radius=1e-3)),
    "B_cauchy": ("B", "cauchy", dict(initial_trust_region_radius=1e16)),
    # (DOGLEG only)
    "M_none": ("M", None, dict(initial_trust_region_radius=1.0)),
    "M_huber": ("M", "huber", dict(initial_trust_region_radius=1.0)),
}
LM_CASES = ("A_none", "A_huber", "A_cauchy", "B_none", "B_huber", "B_cauchy")
DOGLEG_CASES = ("M_none", "M_huber", "B_none", "B_huber")


@functools.lru_cache(maxsize=None)
def scene_weights(sname, family="mild"):
    W = weights(family, len(B.scene(sname)["obs_cam"]), seed="ABCM".index(sname))
    W.setflags(write=False)
    return W


def table_for(sname, name):
    return None if name is None else B.loss_table(sname, name, len(B.scene(sname)["obs_cam"]))


def problem(sname, name, family="mild"):
    return WeightedBAProblem(B.scene(sname), scene_weights(sname, family), table_for(sname, name))


@functools.lru_cache(maxsize=None)
def reference(case, k, strategy="lm"):
    """the weighted reference loop, computed once per case and shared (read-only) by the tests"""
    sname, name, ok = SOLVE_CASES[case]
    o = L.lm_options(**ok)
    return (B.lm_reference if strategy == "lm" else B.dogleg_reference)(problem(sname, name), o, k)


def normal_parts(prob, x=None):
    """(cost, the 6 x 6 camera blocks sum J_c^T J_c per camera, the 3 x 3 landmark blocks, J^T r) of the whitened, corrected problem"""
    x = prob.x0 if x is None else x
    cams, pts = prob.split(x)
    r, Jc, Jp, terms = prob.lin_obs_corrected(cams, pts)
    return normal_parts_of(prob, r, Jc, Jp, float(0.5 * np.sum(terms.astype(LD))))


def normal_parts_of(prob, r, Jc, Jp, cost):
    Hc = np.zeros((prob.nc, 6, 6)); Hp = np.zeros((prob.np_, 3, 3)); g = np.zeros(prob.n_local)
    np.add.at(Hc, prob.oc, np.einsum("nki,nkj->nij", Jc, Jc))
    np.add.at(Hp, prob.op, np.einsum("nki,nkj->nij", Jp, Jp))
    J = np.concatenate([Jc, Jp], 2)
    np.add.at(g, prob.cols, np.einsum("nki,nk->ni", J, r))
    return cost, Hc, Hp, g
