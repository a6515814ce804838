"""The reference of tests/test_gpu_chol_inverse.py, checked without a GPU: a rounding-level test of the explicit SPD inverse
(chol_spd_inverse_dev, dense_chol.hip, through st.cholesky_inverse) is only worth what its reference is worth.  On every case the
GPU test uses (chol_cases.INVERSE_ALL), with tolerance = 50 kappa(H) eps, H = A / (d d^T), d = sqrt(diag A):

  * the refined reference (chol_ref.inverse_ref: dpotrf / dpotrs on identity columns + extended-precision residuals) has
    converged: its last correction is <= 1e-3 of the tolerance;
  * it is symmetric to its own accuracy: the square block on its own columns differs from its transpose by <= 1e-3 of the tolerance;
  * LAPACK's own inverse (dpotri) meets a tenth of the tolerance;
  * the design restated in numpy (chol_ref.partial_factorisation_inverse: [A; I] factored right-looking through explicit tile
    inverses, X X^T summed per panel) meets the tolerance at tb = 16 and at tb = 128 -- the design is entitled to the bound;
  * the reference of a power-of-two rescaling is exactly D^-1 X_base D^-1.

Measured, as forward error / (kappa(H) eps), LAPACK dpotri | restatement tb = 16 | tb = 128 ("Accuracy"): see the
docstrings of the first two tests.
"""
import importlib

import numpy as np
import pytest

import chol_cases as C
import chol_ref as R


@pytest.fixture(scope="module")
def scenes_mod():
    return importlib.import_module("slam-tricks_amd.scenes")


@pytest.mark.parametrize("name", C.INVERSE_ALL)
def test_reference_has_converged_and_lapack_meets_a_tenth_of_the_tolerance(name, O, scenes_mod):
    """Measured: last correction 6.6e-8 - 1.6e-6 of the tolerance, asymmetry 5.4e-8 - 9.3e-6 of it; dpotri's forward error
    0.019 - 0.101 kappa(H) eps against 50 (the largest on ba, kappa(H) = 7.8e2)."""
    A = C.case(name, O, scenes_mod)["A"]
    ref = C.inverse_reference(name, O, scenes_mod)
    n, cols, X, tol = A.shape[0], ref["cols"], ref["X_ref"], ref["tol"]
    assert X.shape == (n, len(cols)) and np.all(np.isfinite(X))
    assert len(cols) == n if n <= 600 else 64 <= len(cols) < n
    d = np.sqrt(np.diag(A))
    sub = X[cols, :]
    asym = float(np.max(np.abs(sub - sub.T) * np.outer(d[cols], d[cols])) / np.max(np.abs(X) * d[:, None] * d[None, cols]))
    print(f"{name}: n {n}, kappa(H) {ref['kappa']:.3e}, {len(cols)} columns, last correction {ref['last_correction'] / tol:.1e} tol, asymmetry "
          f"{asym / tol:.1e} tol; dpotri: forward error {ref['fe_lapack'] / (ref['kappa'] * R.EPS):.3f} kappa(H) eps, right residual "
          f"{ref['rr_lapack'] / R.EPS:.3g} eps; pivot ratio {ref['pivot_ratio']:.3e}")
    assert ref["kappa"] <= C.KAPPA_H_MAX
    assert ref["last_correction"] <= 1e-3 * tol
    assert asym <= 1e-3 * tol
    assert ref["fe_lapack"] <= tol / 10.0
    assert 0.0 < ref["rr_lapack"] < np.inf and 0.0 < ref["pivot_ratio"] <= 1.0


@pytest.mark.parametrize("name", C.INVERSE_ALL)
def test_the_design_restated_in_numpy_meets_the_tolerance(name, O, scenes_mod):
    """chol_ref.partial_factorisation_inverse at tb = 16 and tb = 128.  Measured, forward error / (kappa(H) eps), tb = 16 | tb = 128:
    spectrum 0.004 - 0.019 | 0.012 - 0.059; rbf delta = 1e-4 0.007 - 0.013 | 0.051 - 0.106; rbf delta = 1e-8 0.021 - 3.0 | 0.041 -
    5.5 (the largest: n = 500, tb = 128; the power-of-two rescalings give the base's numbers); ba 0.38 | 0.11.  Its right residual
    at tb = 16 is 0.3 - 2.1 x dpotri's on spectrum and ba and 13 - 2400 x on rbf (it varies a little with the BLAS), where every diagonal tile is as ill conditioned as
    A: what the GPU test's split between asserted and printed residuals rests on."""
    ref, rs = C.inverse_reference(name, O, scenes_mod), C.inverse_restatement(name, O, scenes_mod)
    ke = ref["kappa"] * R.EPS
    print(f"{name}: kappa(H) {ref['kappa']:.3e}; forward error / (kappa(H) eps): dpotri {ref['fe_lapack'] / ke:.3f}, restatement tb = 16 "
          f"{rs['fe16'] / ke:.3f}, tb = 128 {rs['fe128'] / ke:.3f}; right residual / dpotri's: restatement tb = 16 {rs['rr16'] / ref['rr_lapack']:.2f}")
    assert rs["fe16"] <= ref["tol"] and rs["fe128"] <= ref["tol"]
    if C.tiles_well_conditioned(name) or name == "ba":
        assert rs["rr16"] <= R.E_FACTOR * ref["rr_lapack"]


def test_case_list_covers_the_panel_counts():
    """np = n rounded up to 128; panels = np / 128; padding rows = np - n: one panel with one padding row and with none, two panels
    with 127, several panels, and the last real row next to the lower block (1151: np = 1152, one padding row)"""
    def panels(n):
        return (n + 127) // 128
    sizes = sorted({C.SPECS[c]["n"] for c in C.INVERSE_SYNTHETIC})
    assert sizes == [127, 128, 129, 500, 520, 1100, 1151]
    assert [panels(n) for n in sizes] == [1, 1, 2, 4, 5, 9, 9]
    assert [panels(n) * 128 - n for n in sizes] == [1, 0, 127, 12, 120, 52, 1]
    for n in (127, 128, 129, 500, 520, 1100, 1151):
        assert f"spectrum-k1e8-n{n}" in C.INVERSE_SYNTHETIC and f"rbf-d1e-8-n{n}" in C.INVERSE_SYNTHETIC
    assert set(C.INVERSE_ALL) - set(C.ALL) == {"spectrum-k1e8-n129", "rbf-d1e-8-n129"}


@pytest.mark.parametrize("name", C.POW2)
def test_pow2_reference_is_the_rescaled_base_reference(name):
    """(D A D)^-1 = D^-1 A^-1 D^-1 with D = diag(2^k): LAPACK's factor and solves commute with powers of two, the residuals are
    formed in extended precision on exactly scaled numbers, so the refined reference is the base's, rescaled, bit for bit"""
    c = C.case(name)
    ref, base = C.inverse_reference(name), C.inverse_reference(c["base"])
    k, cols = c["k"], ref["cols"]
    assert np.array_equal(cols, base["cols"])
    assert np.array_equal(ref["X_ref"], np.ldexp(base["X_ref"], -(k[:, None] + k[None, cols])))
    assert ref["kappa"] == base["kappa"]


def test_partial_factorisation_inverse_is_an_inverse():
    """the restatement itself: on a well-conditioned matrix it gives LAPACK's inverse to rounding, at block sizes that divide n and
    at ones that do not"""
    rng = np.random.default_rng(6)
    B = rng.normal(size=(100, 100))
    A = B @ B.T + 100 * np.eye(100)
    X = R.inverse_lapack(A)
    for tb in (4, 16, 37, 128):
        Y = R.partial_factorisation_inverse(A, tb)
        assert np.array_equal(Y, Y.T)
        assert np.allclose(Y, X, rtol=0, atol=1e-12 * np.abs(X).max())


def test_inverse_measures():
    """inverse_forward_error is invariant under diagonal scaling and sees one wrong entry; inverse_right_residual is zero to rounding
    on an inverse and sees the same entry"""
    rng = np.random.default_rng(7)
    B = rng.normal(size=(40, 40))
    A = B @ B.T + 40 * np.eye(40)
    cols = np.array([0, 5, 39])
    X_ref, rel = R.inverse_ref(A, cols)
    assert rel <= 1e-16
    X = R.inverse_lapack(A)
    assert R.inverse_forward_error(A, X, X_ref, cols) <= 50 * R.kappa_H(A) * R.EPS
    assert R.inverse_right_residual(A, X, cols) <= 100 * R.EPS
    bad = X.copy()
    bad[7, 5] *= 1.0 + 1e-6
    fe = R.inverse_forward_error(A, bad, X_ref, cols)
    assert fe > 1e-9 and R.inverse_right_residual(A, bad, cols) > 1e-9
    k = rng.integers(-30, 31, 40)
    As, bads = np.ldexp(A, k[:, None] + k[None, :]), np.ldexp(bad, -(k[:, None] + k[None, :]))
    Xs_ref = np.ldexp(X_ref, -(k[:, None] + k[None, cols]))
    assert abs(R.inverse_forward_error(As, bads, Xs_ref, cols) - fe) <= 1e-12 * fe
