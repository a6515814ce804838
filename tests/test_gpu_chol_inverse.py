"""The explicit SPD inverse behind every covariance and the pose graph's coarse operator (chol_spd_inverse_dev in dense_chol.hip,
laid out and packed by cov_spd_inverse_packed in covariance.hip, through st.cholesky_inverse) at rounding level on ill-conditioned,
badly scaled matrices.  It is not the factor-and-solve program that test_gpu_chol_conditioning.py tests: it is a partial
right-looking factorisation of W = [A .; I 0] (2 np rows, np = n rounded up to 128 with identity rows on the padding) with the stage
kernels, stopped after np / 128 panels so that -A^-1 = -sum over panels X X^T survives in the lower right block.
tests/chol_cases.py holds the inputs (INVERSE_ALL: every case of the factorisation's test, np / 128 = 1, 4, 5 and 9 panels, and
n = 129: two panels, 127 padding rows), tests/chol_ref.py the reference and the measures, tests/test_chol_inverse_reference_cpu.py
checks both without a GPU.  With d = sqrt(diag A), H = A / (d d^T), D = diag(d):

  (a) no false "not positive definite"; the result is finite, exactly symmetric, with a positive diagonal;
  (b) forward error, every case: max |d_i d_j (X - X_ref)_ij| / max |d_i d_j (X_ref)_ij| <= 50 kappa(H) eps, the project's bound.
      An inverse through explicit tile inverses is forward stable: the design is entitled to no more;
  (c) right residual max |H (D X D) - I|, in extended precision on the reference's columns, <= 10 x the same measure of LAPACK
      dpotri on the same matrix, where the diagonal tiles are well conditioned (spectrum, its power-of-two rescaling, ba): one order
      of magnitude separates another summation order from lost bits.  On rbf and its rescaling it is printed, (b) covers them;
  (d) A -> D2 A D2 with D2 = diag(2^k), |k| <= 200: the scaled problem meets (b) (and (c)); whether D2 X_scaled D2 == X_base bit for
      bit is printed, not asserted (it rests on v_rsq_f64's seed, see test_gpu_chol_conditioning.py);
  (e) the pivot ratio against min l_ii^2 / max l_ii^2 of LAPACK's factor, within 50 kappa(H) eps relative: the smallest pivot is
      1 / (A^-1)_nn and has the conditioning of the inverse;
  (f) a pivot that fails by 1e-6 a_kk is reported as status -4 with LAPACK's info k + 1, at the tile, panel and matrix edges, and
      neither output is written.

Measured on an MI355X ("Accuracy", has the table): see the docstrings of the tests.
"""
import ctypes
import importlib
import re

import numpy as np
import pytest

import chol_cases as C
import chol_ref as R

pytestmark = pytest.mark.gpu

ASSERT_RR = [c for c in C.INVERSE_ALL if C.tiles_well_conditioned(c) or c == "ba"]
REPORT_RR = [c for c in C.INVERSE_ALL if c not in ASSERT_RR]


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


@pytest.fixture(scope="module")
def scenes_mod():
    return importlib.import_module("slam-tricks_amd.scenes")


_results = {}


def inverse(st, name, O=None, scenes_mod=None):
    """the case's inverse on the device, once: X, the pivot ratio, the forward error and the right residual on the reference's columns"""
    if name not in _results:
        A, ref = C.case(name, O, scenes_mod)["A"], C.inverse_reference(name, O, scenes_mod)
        X, rc = st.cholesky_inverse(A)                      # (raises StbaError on a false "not positive definite")
        out = dict(X=X, rc=rc, fe=np.inf, rr=np.inf)
        if np.all(np.isfinite(X)):
            out["fe"] = R.inverse_forward_error(A, X, ref["X_ref"], ref["cols"])
            out["rr"] = R.inverse_right_residual(A, X, ref["cols"])
        _results[name] = out
    return _results[name]


def report_line(name, O, scenes_mod, out):
    n = C.case(name, O, scenes_mod)["A"].shape[0]
    ref, rs = C.inverse_reference(name, O, scenes_mod), C.inverse_restatement(name, O, scenes_mod)
    ke = ref["kappa"] * R.EPS
    return (f"{name}: n {n}, {(n + 127) // 128} panels, kappa(H) {ref['kappa']:.2e}; forward error / (kappa(H) eps): gpu {out['fe'] / ke:.3f}, dpotri "
            f"{ref['fe_lapack'] / ke:.3f}, restatement tb = 16 {rs['fe16'] / ke:.3f}, tb = 128 {rs['fe128'] / ke:.3f}; right residual / dpotri's: gpu "
            f"{out['rr'] / ref['rr_lapack']:.2f}, restatement tb = 16 {rs['rr16'] / ref['rr_lapack']:.2f} (dpotri {ref['rr_lapack'] / R.EPS:.3g} eps)")


# ------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", C.INVERSE_ALL)
def test_no_false_failure_and_a_symmetric_finite_inverse(st, O, scenes_mod, name):
    out = inverse(st, name, O, scenes_mod)
    n = C.case(name, O, scenes_mod)["A"].shape[0]
    X = out["X"]
    assert X.shape == (n, n)
    assert np.all(np.isfinite(X)) and np.isfinite(out["rc"])
    assert np.array_equal(X, X.T)
    assert np.all(np.diag(X) > 0.0)
    assert 0.0 < out["rc"] <= 1.0


# ------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("name", C.INVERSE_ALL)
def test_forward_error_of_the_inverse(st, O, scenes_mod, name):
    """max |d_i d_j (X - X_ref)_ij| / max |d_i d_j (X_ref)_ij| <= 50 kappa(H) eps.
    Measured on an MI355X, forward error / (kappa(H) eps), gpu | LAPACK dpotri | restatement tb = 16 | tb = 128:
      spectrum (every kappa and size)   0.010 - 0.073 | 0.021 - 0.065 | 0.004 - 0.020 | 0.011 - 0.041
      rbf delta = 1e-4                  0.027 - 0.036 | 0.019 - 0.029 | 0.007 - 0.013 | 0.051 - 0.106
      rbf delta = 1e-8                  0.025 - 0.698 | 0.019 - 0.060 | 0.021 - 3.0   | 0.041 - 5.5     (gpu's largest: n = 129)
      ba (kappa(H) = 7.8e2)             1.117         | 0.101         | 0.383         | 0.114           (the smallest margin, 45 x)
    and the power-of-two rescalings give their base case's numbers."""
    out, ref = inverse(st, name, O, scenes_mod), C.inverse_reference(name, O, scenes_mod)
    print(report_line(name, O, scenes_mod, out))
    assert out["fe"] <= ref["tol"]


# ------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("name", ASSERT_RR)
def test_right_residual_at_lapack_level_where_the_tiles_are_well_conditioned(st, O, scenes_mod, name):
    """max |H (D X D) - I| <= 10 x LAPACK dpotri's on the same matrix and columns.
    Measured on an MI355X, right residual / dpotri's, gpu | restatement tb = 16: spectrum 1.02 - 2.19 | 0.34 - 2.09 at every kappa
    and size (dpotri's own: 5e2 eps at kappa = 1e4 to 3e9 eps at 1e11 -- the residual of an explicit inverse grows with kappa, which is
    why the bound is relative to dpotri's); ba 4.41 | 1.48, the smallest margin (dpotri: 247 eps)."""
    out, ref = inverse(st, name, O, scenes_mod), C.inverse_reference(name, O, scenes_mod)
    print(report_line(name, O, scenes_mod, out))
    assert out["rr"] <= R.E_FACTOR * ref["rr_lapack"]


@pytest.mark.parametrize("name", REPORT_RR)
def test_right_residual_report_where_the_tiles_are_ill_conditioned(st, O, scenes_mod, name):
    """rbf and its rescaling: every diagonal tile is as ill conditioned as A, multiplying by its explicit inverse is forward but not
    backward stable (the numpy restatement's right residual is ~1000 x dpotri's): printed, the forward bound (b) covers these
    cases.  Asserted: the residual is a number.
    Measured on an MI355X, right residual / dpotri's, gpu | restatement tb = 16: delta = 1e-4 15 - 19 | 13 - 18; delta = 1e-8
    1031 - 1938 | 1449 - 2396 -- the kernel loses what the design loses, no more."""
    out = inverse(st, name, O, scenes_mod)
    print(report_line(name, O, scenes_mod, out))
    assert np.isfinite(out["rr"])


# ------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("name", C.POW2)
def test_scale_invariance_under_powers_of_two(st, name):
    """(D2 A D2)^-1 = D2^-1 A^-1 D2^-1: the scaled problem meets the same bounds against its own reference (which is the base's,
    rescaled, bit for bit: test_chol_inverse_reference_cpu.py); the bitwise agreement of the kernel's two results is printed."""
    c, ref = C.case(name), C.inverse_reference(name)
    out, base = inverse(st, name), inverse(st, c["base"])
    k = c["k"]
    back = np.ldexp(out["X"], k[:, None] + k[None, :])
    same = np.array_equal(back, base["X"])
    dX = R.inverse_forward_error(C.case(c["base"])["A"], back, base["X"][:, ref["cols"]], ref["cols"])
    print(report_line(name, None, None, out))
    print(f"{name}: D2 X_scaled D2 == X_base bit for bit: {same}; scaled difference {dX / (ref['kappa'] * R.EPS):.3g} kappa(H) eps; "
          f"forward error unscaled {base['fe'] / (ref['kappa'] * R.EPS):.3f}, scaled {out['fe'] / (ref['kappa'] * R.EPS):.3f} kappa(H) eps")
    assert out["fe"] <= ref["tol"]
    if name in ASSERT_RR:
        assert out["rr"] <= R.E_FACTOR * ref["rr_lapack"]


# ------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("name", C.INVERSE_ALL)
def test_pivot_ratio_against_lapack(st, O, scenes_mod, name):
    """smallest / largest l_ii^2 of the device's factor against LAPACK's, within 50 kappa(H) eps relative.
    Measured on an MI355X: 0.000 - 0.057 kappa(H) eps on the synthetic cases, 0.079 on ba."""
    out, ref = inverse(st, name, O, scenes_mod), C.inverse_reference(name, O, scenes_mod)
    rel = abs(out["rc"] - ref["pivot_ratio"]) / ref["pivot_ratio"]
    print(f"{name}: pivot ratio gpu {out['rc']:.6e}, LAPACK {ref['pivot_ratio']:.6e}, relative difference {rel / (ref['kappa'] * R.EPS):.3f} kappa(H) eps")
    assert rel <= ref["tol"]


# ------------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("k", C.fail_pivots())
def test_pivot_failing_by_a_small_margin_is_reported_and_nothing_is_returned(st, k):
    """pivot k negative by 1e-6 a_kk (kappa = 1e6, n = 520: panels 0, 1, 2 and 4), every earlier pivot untouched: status -4, the
    message names pivot k + 1 as LAPACK's info does, and the C entry point leaves both outputs as they were"""
    A = C.fail_case(k)
    with pytest.raises(st.StbaError) as e:
        st.cholesky_inverse(A)
    assert e.value.code == -4
    m = re.search(r"pivot (\d+)", str(e.value))
    assert m is not None, str(e.value)
    assert int(m.group(1)) == k + 1, str(e.value)
    out = np.full_like(A, np.nan)
    rc = ctypes.c_double(-7.0)
    status = st.lib().stba_cholesky_inverse(A.ctypes.data_as(ctypes.c_void_p), A.shape[0], out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rc),
                                            ctypes.c_void_p(0))
    assert status == -4
    assert np.all(np.isnan(out)) and rc.value == -7.0
