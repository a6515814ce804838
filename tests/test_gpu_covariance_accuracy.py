"""The routes over the explicit SPD inverse (chol_spd_inverse_dev, tested on its own in test_gpu_chol_inverse.py) at rounding level:
st.dense_covariance (stba_dense_covariance, "gpu-dense") and BAEngine.covariance (stba_ba_covariance_compute, "gpu-ba").
test_gpu_covariance.py compares them with np.linalg.inv under 50 kappa(J^T J) eps, the unscaled condition number of the whole
problem; here the reference is chol_ref.inverse_ref (LAPACK + extended-precision refinement) of the very matrix the device inverts,
the measure is the scaled one, max |d_i d_j (X - X_ref)_ij| / max |d_i d_j (X_ref)_ij| with d = sqrt(diag A), and the bound is
50 kappa(H) eps with H = A / (d d^T).

  dense_covariance   J (2n x n) Gaussian with columns scaled by 10^U(-3, 3), n = 129 (two panels, 127 padding rows) and n = 300;
                     the reference inverts J^T J formed in extended precision from the double J.  The device forms J^T J in
                     doubles: a relative perturbation of n_res eps of H, inside the bound as long as kappa(H) is moderate
                     (asserted: <= 1e8; measured: 34 and 30).
  BAEngine.covariance   camera blocks only (the landmark blocks have their 50-digit test, test_gpu_schur_elim.py).  The reference
                     inverts the free part of the engine's OWN zero-damped S, read through reduced_system(0, 0) and symmetrised
                     from its lower triangle: stba_ba_covariance_compute builds S through the same launches (ba_cov_build in
                     ba_linear.hip: ba_linearize, the landmark blocks, ba_build_reduced with explicit zero damping --
                     evaluate / normal_blocks / reduced_system run exactly these; the camera-side kernel normal_blocks adds writes
                     Hcc, which the Schur kernel writes again), in the pair plan, whose S is bitwise reproducible.  Comparing with
                     the device's S keeps the cancellation in U - E V^-1 E^T out of the bound.

Measured on an MI355X: see the docstrings of the tests.
"""
import importlib

import numpy as np
import pytest

import chol_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def scaled_error(d, rows, cols, X, X_ref):
    """max |d_i d_j (X - X_ref)_ij| over the block rows x cols"""
    return float(np.max(np.abs(X - X_ref) * d[rows, None] * d[None, cols]))


# ------------------------------------------------------------------------------- dense_covariance
@pytest.mark.parametrize("n", [129, 300])
def test_dense_covariance_forward_error(st, n):
    """Measured on an MI355X, forward error / (kappa(H) eps), device | LAPACK dpotri on the extended-precision J^T J: n = 129
    0.196 | 0.078 (kappa(H) = 34, kappa(J^T J) = 2.1e12); n = 300 0.502 | 0.121 (kappa(H) = 30).  The pivot ratio agrees with LAPACK's
    in all seven digits printed."""
    rng = np.random.default_rng(1000 + n)
    n_res = 2 * n
    J = rng.normal(size=(n_res, n)) * 10.0 ** rng.uniform(-3.0, 3.0, n)
    b = rng.normal(size=n_res)
    x0 = rng.normal(size=n)
    Jx = J.astype(LD)
    A = (Jx.T @ Jx).astype(np.float64)
    A = np.tril(A) + np.tril(A, -1).T
    kappa = R.kappa_H(A)
    tol = R.forward_tolerance(kappa)
    assert kappa <= 1e8
    cols = np.arange(n)
    X_ref, rel = R.inverse_ref(A, cols)
    assert rel <= 1e-3 * tol
    cov, rc = st.dense_covariance(lambda x: (J @ x - b, J), x0, n_res)
    assert cov.shape == (n, n) and np.all(np.isfinite(cov)) and np.array_equal(cov, cov.T) and np.all(np.diag(cov) > 0.0)
    fe = R.inverse_forward_error(A, cov, X_ref, cols)
    L, _ = R.factor_ref(A)
    piv = np.diag(L) ** 2
    print(f"dense_covariance n = {n}, n_res = {n_res}: kappa(H) {kappa:.3e} (kappa(J^T J) {np.linalg.cond(A):.2e}), forward error "
          f"{fe / (kappa * R.EPS):.3f} kappa(H) eps, dpotri {R.inverse_forward_error(A, R.inverse_lapack(A), X_ref, cols) / (kappa * R.EPS):.3f}; "
          f"pivot ratio {rc:.6e}, LAPACK {piv.min() / piv.max():.6e}")
    assert fe <= tol
    assert abs(rc - piv.min() / piv.max()) <= tol * piv.min() / piv.max()


# ------------------------------------------------------------------------------- BAEngine.covariance
def st20_default(scenes):
    return scenes.st20_scene()


def st20_weak_gauge(scenes):
    """only camera 0 and the x position of the last camera constant: n = 167, kappa(H) = 1.5e5 on the oracle"""
    s = scenes.st20_scene()
    cf = np.zeros_like(s["cam_fixed"])
    cf[0] = 1
    cf[-1, 3] = 1
    s["cam_fixed"] = cf
    return s


def st20_100_cameras(scenes):
    """100 cameras, 2000 landmarks: five panels; single constant dofs on middle cameras next to the constant first and last one"""
    s = scenes.st20_scene(n_cams=100, n_pts=2000)
    cf = s["cam_fixed"].copy()
    cf[37, 1] = 1; cf[50, 4] = 1; cf[63, 0] = 1; cf[63, 5] = 1
    s["cam_fixed"] = cf
    return s


BA_SCENES = {"st20": (st20_default, 162), "st20-weak-gauge": (st20_weak_gauge, 167), "st20-100-cameras": (st20_100_cameras, 584)}


@pytest.mark.parametrize("scene", list(BA_SCENES))
def test_ba_camera_covariance_forward_error(st, scenes, scene):
    """Measured on an MI355X, forward error of the requested camera blocks / (kappa(H) eps), device | dpotri on the same S (all
    entries): st20 0.311 | 0.091 (kappa(H) = 6.2e2); st20-weak-gauge 0.068 | 0.002 (1.5e5); st20-100-cameras 1.445 | 0.196 (7.6e2)."""
    make, n_free = BA_SCENES[scene]
    s = make(scenes)
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
    e.set_schur_mode(e.SCHUR_PAIRS)
    nc = e.nc
    e.evaluate(residuals=False, jac=False)
    e.normal_blocks()
    S, _ = e.reduced_system(np.zeros(6 * nc), np.zeros((e.np_, 3)))
    S = np.tril(S) + np.tril(S, -1).T
    fixed = np.asarray(s["cam_fixed"], dtype=bool).reshape(-1)
    free = ~fixed
    A = np.ascontiguousarray(S[np.ix_(free, free)])
    assert A.shape[0] == n_free
    kappa = R.kappa_H(A)
    tol = R.forward_tolerance(kappa)
    X_ref, rel = R.inverse_ref(A, np.arange(n_free))
    assert rel <= 1e-3 * tol
    d = np.zeros(6 * nc)
    d[free] = np.sqrt(np.diag(A))
    C_ref = np.zeros((6 * nc, 6 * nc))
    C_ref[np.ix_(free, free)] = X_ref
    scale = float(np.max(np.abs(C_ref) * np.outer(d, d)))
    # every diagonal block and 30 seeded cross pairs; some touch a camera with constant dofs
    rng = np.random.default_rng(77)
    touched = np.flatnonzero(np.asarray(s["cam_fixed"], dtype=bool).any(1))
    cross = [(int(a), int(b)) for a, b in rng.integers(0, nc, (24, 2))]
    cross += [(int(a), int(b)) for a, b in zip(rng.choice(touched, 6), rng.integers(0, nc, 6))]
    pairs = [(c, c) for c in range(nc)] + cross
    cam, _, rc = e.covariance(cam_pairs=pairs, points=[0])
    worst = 0.0
    for (a, b), blk in zip(pairs, cam):
        ra, rb = np.arange(6 * a, 6 * a + 6), np.arange(6 * b, 6 * b + 6)
        assert np.all(np.isfinite(blk))
        assert np.all(blk[fixed[ra], :] == 0.0) and np.all(blk[:, fixed[rb]] == 0.0)      # constant dofs: exactly zero
        worst = max(worst, scaled_error(d, ra, rb, blk, C_ref[np.ix_(ra, rb)]))
    fe = worst / scale
    X_lapack = R.inverse_lapack(A)
    print(f"{scene}: {nc} cameras, n = {n_free}, {(6 * nc + 127) // 128} panels, kappa(H) {kappa:.3e}, pivot ratio {rc:.3e}; camera blocks of "
          f"{len(pairs)} pairs: forward error {fe / (kappa * R.EPS):.3f} kappa(H) eps (dpotri on the same S, all entries: "
          f"{R.inverse_forward_error(A, X_lapack, X_ref, np.arange(n_free)) / (kappa * R.EPS):.3f})")
    assert fe <= tol
