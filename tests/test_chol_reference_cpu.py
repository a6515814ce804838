"""The inputs and the reference of tests/test_gpu_chol_conditioning.py, checked without a GPU: a rounding-level test of the dense
Cholesky is only worth what its reference is worth.  On every case of tests/chol_cases.py

  * the input conditions hold: kappa(H) <= 1e11, and the smallest scaled pivot of LAPACK's factor is >= 1e3 n eps, so the matrix
    is far from the edge of definiteness where the reference itself would be marginal;
  * the refined reference solution has converged: its last correction is <= 1e-3 of the forward tolerance 50 kappa(H) eps;
  * LAPACK's own backward error E is <= 1/10 of the bound the GPU test uses (10 E_lapack: by construction) and inside the bound
    of a plain Cholesky, (n+1) eps / (1 - (n+1) eps);
  * LAPACK's own forward error is <= 1/10 of the forward tolerance (measured: 0.02 - 0.14 kappa(H) eps against 50).

One test documents what the design's explicit tile inverses cost (tile_inverse_cholesky, a numpy restatement of the class), one
the failing-pivot construction the GPU test reuses.
"""
import importlib

import numpy as np
import pytest

import chol_cases as C
import chol_ref as R


@pytest.fixture(scope="module")
def scenes_mod():
    return importlib.import_module("slam-tricks_amd.scenes")


@pytest.mark.parametrize("name", C.ALL)
def test_inputs_and_reference(name, O, scenes_mod):
    c = C.case(name, O, scenes_mod)
    ref = C.reference(name, O, scenes_mod)
    A, b, n = c["A"], c["b"], c["A"].shape[0]
    assert np.array_equal(A, A.T) and np.all(np.isfinite(A)) and np.all(np.isfinite(b))
    tiny = np.finfo(np.float64).tiny
    assert np.abs(A[A != 0]).min() > tiny / R.EPS, "an entry is close to the subnormal range"
    minpiv = R.min_scaled_pivot(A, ref["L"])
    x_lapack = R.solve_lapack(A, b)
    fe = R.forward_error(A, x_lapack, ref["x_ref"])
    print(f"{name}: n {n}, kappa(H) {ref['kappa']:.3e}, min scaled pivot {minpiv / (n * R.EPS):.2e} n eps, E_lapack {ref['E_lapack'] / R.EPS:.1f} eps "
          f"on {len(ref['rows'])} rows, last correction {ref['last_correction'] / ref['tol']:.1e} tol, LAPACK forward error "
          f"{fe / (ref['kappa'] * R.EPS):.3f} kappa eps")
    assert ref["kappa"] <= C.KAPPA_H_MAX
    if name == "ba":
        assert ref["kappa"] <= C.BA_KAPPA_H_MAX
    assert minpiv >= C.min_scaled_pivot_floor(n)
    assert ref["last_correction"] <= 1e-3 * ref["tol"]
    # (the GPU test's bound is E_FACTOR * E_lapack: LAPACK sits at 1/10 of it by construction -- what has to hold is that E_lapack is a number)
    assert R.E_FACTOR == 10.0 and 0.0 < ref["E_lapack"] < np.inf
    assert ref["E_lapack"] <= R.cholesky_E_bound(n)
    assert fe <= ref["tol"] / 10.0


def test_case_list_covers_the_paths_of_chol_run():
    """every family at 520 and 1100, the edge sizes with spectrum kappa = 1e8 and rbf delta = 1e-8; and the sizes meet the paths
    they are there for (lda = chol_padded_dim(n), nblk = lda / 128, nwide = (nblk - 1) / 4)"""
    def nblk(n):
        return (n + 1 + 127) // 128
    assert [nblk(n) for n in (127, 128, 500, 520, 1100, 1151)] == [1, 2, 4, 5, 9, 9]
    assert [(nblk(n) - 1) // 4 for n in (500, 520, 1100)] == [0, 1, 2]
    assert nblk(1151) * 128 - 1 == 1151                      # the rhs row is the row after the last real one
    for n in C.MAIN_SIZES:
        fams = {C.family(c) for c in C.SYNTHETIC if C.SPECS[c]["n"] == n}
        assert fams == {"spectrum", "rbf", "pow2-spectrum", "pow2-rbf"}
        assert {C.SPECS[c].get("kappa") for c in C.SYNTHETIC if C.SPECS[c]["n"] == n and C.family(c) == "spectrum"} == {1e4, 1e8, 1e11}
        assert {C.SPECS[c].get("delta") for c in C.SYNTHETIC if C.SPECS[c]["n"] == n and C.family(c) == "rbf"} == {1e-4, 1e-8}
    for n in C.EDGE_SIZES:
        assert f"spectrum-k1e8-n{n}" in C.SPECS and f"rbf-d1e-8-n{n}" in C.SPECS


@pytest.mark.parametrize("name", C.POW2)
def test_pow2_scaling_is_exact(name):
    """A = D A_base D and b = D b_base hold bit for bit, nothing overflows or goes subnormal, and LAPACK's factor of the scaled
    matrix is D L_base bit for bit: an unblocked or blocked Cholesky without explicit thresholds commutes with powers of two"""
    c = C.case(name)
    base = C.case(c["base"])
    k = c["k"]
    assert k.min() >= -200 and k.max() <= 200 and len(np.unique(k)) > 100
    assert np.array_equal(np.ldexp(c["A"], -(k[:, None] + k[None, :])), base["A"])
    assert np.array_equal(np.ldexp(c["b"], -k), base["b"])
    L, Lb = C.reference(name)["L"], C.reference(c["base"])["L"]
    assert np.array_equal(L, np.ldexp(Lb, k[:, None]))
    assert C.reference(name)["kappa"] == C.reference(c["base"])["kappa"]


TILE_CASES = [c for c in C.SYNTHETIC if C.family(c) in ("spectrum", "rbf") and C.SPECS[c]["n"] <= 600]


@pytest.mark.parametrize("name", TILE_CASES)
def test_explicit_tile_inverses_cost_backward_stability_on_ill_conditioned_tiles(name):
    """The design effect, in a numpy restatement (right-looking, panel = rows times the explicit inverse of the 16 x 16 diagonal
    tile's factor).  Solving by explicit inverse is forward stable but not backward stable when the tile is ill conditioned:
      * rbf delta = 1e-8 (every diagonal tile as ill conditioned as A): E_tile16 > 2 E_lapack.  Measured: 3 - 80 times; the spread
        between seeds is up to 6 x, so only the ordering is asserted;
      * spectrum (well-conditioned tiles): E_tile16 <= 10 E_lapack, in fact below E_lapack.
    At the sizes where E is taken over ALL rows (n <= 600): above that E looks at a subset of the rows, which need not hold the
    restatement's worst entry (measured on the subset at n = 1100 / 1151: 2.1 / 1.4 times on rbf delta = 1e-8).  The GPU test
    prints E_tile16 for every case."""
    A, ref = C.case(name)["A"], C.reference(name)
    E16 = R.backward_error(A, R.tile_inverse_cholesky(A, 16), ref["rows"])
    print(f"{name}: E_lapack {ref['E_lapack'] / R.EPS:.1f} eps, E_tile16 {E16 / R.EPS:.1f} eps on {len(ref['rows'])} rows")
    if C.family(name) == "spectrum":
        assert E16 <= 10.0 * ref["E_lapack"]
    elif C.SPECS[name]["delta"] == 1e-8:
        assert E16 > 2.0 * ref["E_lapack"]


def test_ba_tiles_are_well_conditioned(O, scenes_mod):
    """the restatement on the workload's own matrix stays at LAPACK's level: the GPU test asserts the rounding-level bound on ba"""
    A, ref = C.case("ba", O, scenes_mod)["A"], C.reference("ba", O, scenes_mod)
    E16 = R.backward_error(A, R.tile_inverse_cholesky(A, 16), ref["rows"])
    print(f"ba: E_lapack {ref['E_lapack'] / R.EPS:.1f} eps, E_tile16 {E16 / R.EPS:.1f} eps")
    assert E16 <= 10.0 * ref["E_lapack"]


def test_tile_inverse_cholesky_is_a_cholesky():
    """the restatement itself: on a well-conditioned matrix it gives LAPACK's factor to rounding, at a block size that divides n
    and at one that does not"""
    rng = np.random.default_rng(5)
    B = rng.normal(size=(100, 100))
    A = B @ B.T + 100 * np.eye(100)
    L, _ = R.factor_ref(A)
    for tb in (4, 16, 37, 128):
        assert np.allclose(R.tile_inverse_cholesky(A, tb), L, rtol=0, atol=1e-12 * np.abs(L).max())


@pytest.mark.parametrize("k", C.fail_pivots())
def test_failing_pivot_construction(k):
    """pivot k negative by 1e-6 a_kk, every earlier pivot unchanged: dpotrf returns info = k + 1"""
    A = C.fail_case(k)
    assert np.array_equal(A, A.T)
    L, info = R.factor_ref(A)
    assert info == k + 1
    A0, L0 = C._cache["fail"]
    pivot = A[k, k] - L0[k, :k] @ L0[k, :k]
    assert -2e-6 * A0[k, k] < pivot < -0.5e-6 * A0[k, k]
