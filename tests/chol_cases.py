"""The inputs that tests/test_chol_reference_cpu.py and tests/test_gpu_chol_conditioning.py share: symmetric positive definite
systems that are ill conditioned and badly scaled, at the sizes where chol_run (dense_chol.hip) changes path.  Host only, numpy,
seeded.

With d = sqrt(diag A) and H = A / (d d^T), kappa(H) is the condition number that matters for Cholesky: the factorisation is invariant
under diagonal scaling.  Every case satisfies (tests/test_chol_reference_cpu.py asserts it)
    kappa(H) <= 1e11   and   min_k l_kk^2 / a_kk >= 1e3 n eps  (LAPACK's factor),
so that LAPACK's factor, the reference, is itself far from marginal.

Families
    spectrum   A = Q diag(lambda) Q^T, lambda log-spaced from 1 to 1/kappa, then A <- A * (g g^T), g log-uniform in [1e-3, 1e3]:
               badly scaled rows, but the diagonal tiles of every Schur complement are well conditioned
    rbf        A_ij = exp(-((t_i - t_j) / 0.3)^2) + delta [i = j], t sorted uniform on [0, 1]: neighbouring rows nearly equal,
               every 16 x 16 and 128 x 128 diagonal tile as ill conditioned as A -- what explicit tile inverses are sensitive to
    pow2       a spectrum and an rbf case scaled EXACTLY by D = diag(2^k_i), k_i uniform integers in [-200, 200]: H, the exact
               factor D L and the exact solution D^-1 x are the unscaled ones, any difference is a scale dependence of the kernel
    ba         the reduced camera system of st20_scene(n_cams=100, n_pts=2000) at the initial point, constant cameras dropped,
               LM damping mu diag(J^T J) with mu the smallest power of ten for which kappa(H) <= 1e10, searched upwards from
               1e-16 (below the rounding of the diagonal).  With the first and the last camera constant the gauge is fixed and
               the system is benign: 1e-16 already passes, kappa(H) is below 1e3

Sizes (lda = chol_padded_dim(n), nblk = lda / 128, nwide = (nblk - 1) / 4)
    127   nblk 1   one block, the rhs row inside it
    128   nblk 2
    500   nblk 4   no wide step of the backward substitution
    520   nblk 5   one wide step, chol_bwd_apply_kernel<4> only
    1100  nblk 9   two wide steps, <16> and <4>
    1151  nblk 9   the last real row next to the rhs row
Every family runs at 520 and 1100; the other sizes with spectrum kappa = 1e8 and rbf delta = 1e-8.

Right-hand side: b = d * gaussian, so that no row dominates.
"""
import numpy as np

import chol_ref as R
from chol_ref import factor_ref, kappa_H

EPS = np.finfo(np.float64).eps
KAPPA_H_MAX = 1e11
MAIN_SIZES = [520, 1100]
EDGE_SIZES = [127, 128, 500, 1151]
BA_KAPPA_H_MAX = 1e10

_cache = {}


def min_scaled_pivot_floor(n):
    return 1e3 * n * EPS


def spectrum(n, kappa, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = np.logspace(0.0, -np.log10(kappa), n)
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    g = 10.0 ** rng.uniform(-3.0, 3.0, n)
    return A * np.outer(g, g)


def rbf(n, delta, seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(0.0, 1.0, n))
    A = np.exp(-(((t[:, None] - t[None, :]) / 0.3) ** 2))
    A[np.diag_indices(n)] += delta
    return A


def rhs(A, seed):
    return np.sqrt(np.diag(A)) * np.random.default_rng(seed).normal(size=A.shape[0])


def pow2_exponents(n, seed):
    return np.random.default_rng(seed).integers(-200, 201, n)


def _spec(family, n, **kw):
    if family == "spectrum":
        name = f"spectrum-k1e{round(np.log10(kw['kappa']))}-n{n}"
    elif family == "rbf":
        name = f"rbf-d1e{round(np.log10(kw['delta']))}-n{n}"
    else:
        name = f"pow2-{kw['base']}"
    return name, dict(family=family, n=n, **kw)


def _specs():
    out = []
    for n in MAIN_SIZES:
        out += [_spec("spectrum", n, kappa=k) for k in (1e4, 1e8, 1e11)]
        out += [_spec("rbf", n, delta=d) for d in (1e-4, 1e-8)]
    for n in EDGE_SIZES:
        out += [_spec("spectrum", n, kappa=1e8), _spec("rbf", n, delta=1e-8)]
    for n in MAIN_SIZES:
        for base in (_spec("spectrum", n, kappa=1e8)[0], _spec("rbf", n, delta=1e-8)[0]):
            out.append(_spec("pow2", n, base=base))
    return dict(out)


SPECS = _specs()
SYNTHETIC = list(SPECS)
ALL = SYNTHETIC + ["ba"]
POW2 = [c for c in SYNTHETIC if SPECS[c]["family"] == "pow2"]

# the explicit inverse (chol_spd_inverse_dev) pads n to np, a multiple of 128, with identity rows and runs np / 128 panels: every
# case above (np / 128 = 1, 1, 4, 5, 9, 9 at the sizes above) and n = 129, np = 256 with 127 padding rows.  The two cases of 129
# are not part of ALL: the factorisation's tests keep their lists.
INVERSE_EXTRA_SIZES = [129]
INVERSE_EXTRA = dict(s for n in INVERSE_EXTRA_SIZES for s in (_spec("spectrum", n, kappa=1e8), _spec("rbf", n, delta=1e-8)))
SPECS.update(INVERSE_EXTRA)
INVERSE_SYNTHETIC = SYNTHETIC + list(INVERSE_EXTRA)
INVERSE_ALL = INVERSE_SYNTHETIC + ["ba"]


def family(name):
    """'spectrum' | 'rbf' | 'pow2-spectrum' | 'pow2-rbf' | 'ba'"""
    if name == "ba":
        return "ba"
    s = SPECS[name]
    return s["family"] if s["family"] != "pow2" else "pow2-" + SPECS[s["base"]]["family"]


def tiles_well_conditioned(name):
    """the families in which the diagonal tiles of every Schur complement are well conditioned (spectrum and its exact
    rescaling); 'ba' is classified by measurement, see test_gpu_chol_conditioning.py"""
    return family(name) in ("spectrum", "pow2-spectrum")


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31)


def case(name, O=None, scenes=None):
    """-> dict(name, A, b) (A exactly symmetric); a pow2 case also holds base (the unscaled case's name) and k (A = D A_base D,
    b = D b_base, D = diag(2^k)).  'ba' needs the oracle module O and the scenes module."""
    if name in _cache:
        return _cache[name]
    if name == "ba":
        c = ba_case(O, scenes)
    else:
        s = SPECS[name]
        if s["family"] == "pow2":
            base = case(s["base"])
            k = pow2_exponents(s["n"], _seed(name))
            c = dict(name=name, A=np.ldexp(base["A"], k[:, None] + k[None, :]), b=np.ldexp(base["b"], k), base=s["base"], k=k)
        else:
            A = spectrum(s["n"], s["kappa"], _seed(name)) if s["family"] == "spectrum" else rbf(s["n"], s["delta"], _seed(name))
            c = dict(name=name, A=A, b=rhs(A, _seed(name) + 1))
    _cache[name] = c
    return c


def ba_case(O, scenes):
    s = scenes.st20_scene(n_cams=100, n_pts=2000)
    ba = O.BA(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
    _, r, Jc, Jp = ba.evaluate()
    Hcc, _, Hpp, _ = ba.normal_blocks(r, Jc, Jp)
    dHc = np.einsum("cii->ci", Hcc.reshape(-1, 6, 6)); dHp = np.einsum("pii->pi", Hpp.reshape(-1, 3, 3))
    free = ~np.asarray(s["cam_fixed"], dtype=bool).reshape(-1)
    for e in range(-16, 1):
        mu = 10.0 ** e
        S, g = ba.reduced_system(r, Jc, Jp, mu * dHc, mu * dHp)
        S = np.tril(S) + np.tril(S, -1).T
        A = np.ascontiguousarray(S[np.ix_(free, free)])
        if kappa_H(A) <= BA_KAPPA_H_MAX:
            return dict(name="ba", A=A, b=rhs(A, 7), mu=mu)
    raise AssertionError("no damping up to 1 brings kappa(H) of the reduced camera system below 1e10")


def reference(name, O=None, scenes=None):
    """what both test modules need of a case, computed once: kappa(H), LAPACK's factor L and its backward error E_lapack on `rows`,
    the refined solution x_ref with the relative size `last_correction` of its last refinement step, and the forward tolerance"""
    key = ("ref", name)
    if key not in _cache:
        c = case(name, O, scenes)
        A, b = c["A"], c["b"]
        L, info = factor_ref(A)
        assert info == 0, f"{name}: LAPACK finds the matrix not positive definite (info = {info})"
        rows = R.error_rows(A.shape[0])
        kappa = kappa_H(A)
        x_ref, rel = R.solve_ref(A, b)
        _cache[key] = dict(kappa=kappa, L=L, rows=rows, E_lapack=R.backward_error(A, L, rows), x_ref=x_ref, last_correction=rel,
                           tol=R.forward_tolerance(kappa))
    return _cache[key]


def inverse_reference(name, O=None, scenes=None):
    """what the tests of the explicit inverse need of a case, computed once: kappa(H) and the forward tolerance, the columns `cols`
    of the refined reference X_ref (n x len(cols)) with its last_correction, LAPACK's factor L, LAPACK's own inverse (dpotri) with
    its forward error fe_lapack and right residual rr_lapack on the same columns, and the pivot ratio min l_ii^2 / max l_ii^2"""
    key = ("inv", name)
    if key not in _cache:
        A = case(name, O, scenes)["A"]
        L, info = factor_ref(A)
        assert info == 0, f"{name}: LAPACK finds the matrix not positive definite (info = {info})"
        kappa = kappa_H(A)
        cols = R.inverse_columns(A.shape[0])
        X_ref, rel = R.inverse_ref(A, cols)
        X_lapack = R.inverse_lapack(A)
        piv = np.diag(L) ** 2
        _cache[key] = dict(kappa=kappa, tol=R.forward_tolerance(kappa), cols=cols, X_ref=X_ref, last_correction=rel, L=L,
                           X_lapack=X_lapack, fe_lapack=R.inverse_forward_error(A, X_lapack, X_ref, cols),
                           rr_lapack=R.inverse_right_residual(A, X_lapack, cols), pivot_ratio=float(piv.min() / piv.max()))
    return _cache[key]


def inverse_restatement(name, O=None, scenes=None):
    """forward error of chol_ref.partial_factorisation_inverse at tb = 16 and tb = 128 and its right residual at tb = 16, once per case"""
    key = ("inv-restated", name)
    if key not in _cache:
        A, ref = case(name, O, scenes)["A"], inverse_reference(name, O, scenes)
        X16, X128 = R.partial_factorisation_inverse(A, 16), R.partial_factorisation_inverse(A, 128)
        _cache[key] = dict(fe16=R.inverse_forward_error(A, X16, ref["X_ref"], ref["cols"]),
                           fe128=R.inverse_forward_error(A, X128, ref["X_ref"], ref["cols"]),
                           rr16=R.inverse_right_residual(A, X16, ref["cols"]))
    return _cache[key]


# ---- the failing-pivot construction ----
FAIL_N = 520
FAIL_KAPPA = 1e6
FAIL_MARGIN = 1e-6


def fail_pivots():
    return [0, 15, 16, 127, 128, 300, FAIL_N - 1]


def fail_case(k):
    """A spectrum matrix (kappa = 1e6, n = 520) whose pivot k is negative by 1e-6 a_kk, a margin far above the backward error, and
    whose earlier pivots are untouched: a_kk := l_k,:k . l_k,:k - 1e-6 a_kk with l LAPACK's factor of the unmodified matrix."""
    if "fail" not in _cache:
        A = spectrum(FAIL_N, FAIL_KAPPA, 4242)
        L, info = factor_ref(A)
        assert info == 0
        _cache["fail"] = (A, L)
    A, L = _cache["fail"]
    A = A.copy()
    A[k, k] = L[k, :k] @ L[k, :k] - FAIL_MARGIN * A[k, k]
    return A
