"""The reference the dense Cholesky (dense_chol.hip) is tested against on ill-conditioned systems, and the measures and bounds of
tests/test_chol_reference_cpu.py and tests/test_gpu_chol_conditioning.py.  Host only.

    factor_ref        LAPACK dpotrf
    backward_error    E = max_ij |A - L L^T|_ij / sqrt(a_ii a_jj), product and difference in 80-bit extended precision.  It is the
                      scale-invariant backward error: a plain Cholesky satisfies E <= (n+1) eps / (1 - (n+1) eps) whatever
                      kappa is (Demmel; Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.5)
    solve_ref         dpotrf solve + 8 steps of refinement with extended-precision residuals
    forward_error     max |d (x - x_ref)| / max |d x_ref|, d = sqrt(diag A)
    kappa_H           condition number of H = A / (d d^T)
    tile_inverse_cholesky   the design's class restated in numpy: a right-looking blocked Cholesky whose panel solve multiplies by
                      the explicit inverse of the diagonal tile's factor.  For reporting and for one CPU assertion that documents
                      the effect; it is no source of a tolerance

    inverse_ref       the explicit inverse: dpotrf / dpotrs on identity columns + refinement with extended-precision residuals
    inverse_forward_error   max |d_i d_j (X - X_ref)_ij| / max |d_i d_j (X_ref)_ij|: the error of the inverse of H
    inverse_right_residual  max |H (D X D) - I| in extended precision
    partial_factorisation_inverse   chol_spd_inverse_dev's design restated in numpy ([A; I] factored right-looking through explicit
                      tile inverses, X X^T summed per panel): reporting and one CPU assertion, no source of a tolerance

The bounds the GPU tests assert
    forward_tolerance(kappa) = 50 kappa(H) eps    the project's convention (test_gpu_covariance.py); a solve through explicit
                      inverses is forward stable, so the design is entitled to no more
    E_gpu <= 10 E_lapack on the same matrix and rows, where the diagonal tiles are well conditioned: E is an extreme over n^2
                      rounding errors, the references' own spread from blocking and summation order is 1-9 eps, and one order of
                      magnitude separates "another summation order" from "lost bits" (a 2^-42 reciprocal square root would show
                      as thousands of eps)
    the inverse: the same two.  forward_tolerance(kappa) on every case -- an inverse through explicit tile inverses is forward
                      stable and entitled to no more -- and the right residual <= 10 x LAPACK dpotri's on the same matrix and
                      columns where the diagonal tiles are well conditioned
"""
import numpy as np
from scipy.linalg import lapack, solve_triangular

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "chol_ref needs an extended-precision long double (x86-64) for its residuals"

EPS = np.finfo(np.float64).eps
E_FACTOR = 10.0
REFINE_STEPS = 8


def forward_tolerance(kappa):
    return 50.0 * kappa * EPS


def cholesky_E_bound(n):
    return (n + 1) * EPS / (1.0 - (n + 1) * EPS)


def factor_ref(A):
    """-> (L, info): LAPACK dpotrf, lower factor with a zero upper triangle; info as LAPACK returns it"""
    L, info = lapack.dpotrf(A, lower=1, clean=1)
    return L, info


def min_scaled_pivot(A, L):
    return float(np.min(np.diag(L) ** 2 / np.diag(A)))


def kappa_H(A):
    d = np.sqrt(np.diag(A))
    w = np.linalg.eigvalsh(A / np.outer(d, d))
    return float(w[-1] / w[0])


def error_rows(n, seed=0):
    """rows on which backward_error looks: all of them up to n = 600; above, the rows at the tile and block edges (index = 0, 15,
    16, 127 mod 128), the last 16 and 64 seeded random ones"""
    if n <= 600:
        return np.arange(n)
    i = np.arange(n)
    edge = i[np.isin(i % 128, (0, 15, 16, 127))]
    rnd = np.random.default_rng(seed).choice(n, 64, replace=False)
    return np.unique(np.concatenate([edge, i[-16:], rnd]))


def backward_error(A, L, rows=None):
    n = A.shape[0]
    rows = error_rows(n) if rows is None else np.asarray(rows)
    Lx = np.tril(L).astype(LD)
    d = np.sqrt(np.diag(A).astype(LD))
    R = A[rows].astype(LD) - Lx[rows] @ Lx.T
    return float(np.max(np.abs(R) / (d[rows, None] * d[None, :])))


def forward_error(A, x, x_ref):
    d = np.sqrt(np.diag(A))
    return float(np.max(np.abs(d * (x - x_ref))) / np.max(np.abs(d * x_ref)))


def solve_ref(A, b):
    """-> (x, rel): x the solution in doubles, rel the size of the last correction, max |d dx| / max |d x|"""
    L, info = factor_ref(A)
    assert info == 0
    Ax, bx = A.astype(LD), b.astype(LD)
    d = np.sqrt(np.diag(A))
    x = lapack.dpotrs(L, b, lower=1)[0].astype(LD)
    rel = np.inf
    for _ in range(REFINE_STEPS):
        r = (bx - Ax @ x).astype(np.float64)
        dx = lapack.dpotrs(L, r, lower=1)[0]
        x = x + dx
        rel = float(np.max(np.abs(d * dx)) / np.max(np.abs(d * x.astype(np.float64))))
    return x.astype(np.float64), rel


def solve_lapack(A, b):
    """LAPACK's plain solve, no refinement"""
    L, info = factor_ref(A)
    assert info == 0
    return lapack.dpotrs(L, b, lower=1)[0]


def tile_inverse_cholesky(A, tb):
    """right-looking blocked Cholesky, block size tb, in doubles: the panel below a diagonal tile is multiplied by the explicit
    inverse of the tile's factor"""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    for k in range(0, n, tb):
        e = min(k + tb, n)
        Lkk = np.linalg.cholesky(A[k:e, k:e])
        A[k:e, k:e] = Lkk
        if e < n:
            inv = solve_triangular(Lkk, np.eye(e - k), lower=True)
            P = A[e:, k:e] @ inv.T
            A[e:, k:e] = P
            A[e:, e:] -= P @ P.T
    return np.tril(A)


# ---- the explicit inverse (chol_spd_inverse_dev through st.cholesky_inverse): tests/test_chol_inverse_reference_cpu.py,
# tests/test_gpu_chol_inverse.py, tests/test_gpu_covariance_accuracy.py
INVERSE_REFINE_STEPS = 4


def inverse_columns(n):
    """the columns of the inverse the reference holds: all of them up to n = 600, error_rows(n) above (the extended-precision
    residuals of a full reference at n = 1100 take most of a minute)"""
    return error_rows(n)


def _scaled_max(d, cols, M):
    return float(np.max(np.abs(M) * d[:, None] * d[None, cols]))


def inverse_ref(A, cols=None):
    """-> (X, last_correction): X (n x len(cols), doubles) the columns `cols` of A^-1 -- dpotrf / dpotrs on the identity columns,
    then refinement with the residual I - A X in 80-bit extended precision until the correction stops shrinking, 4 steps at the
    most; last_correction = max |d_i d_j dX_ij| / max |d_i d_j X_ij| of the last step applied"""
    n = A.shape[0]
    cols = inverse_columns(n) if cols is None else np.asarray(cols)
    L, info = factor_ref(A)
    assert info == 0
    I = np.zeros((n, len(cols)))
    I[cols, np.arange(len(cols))] = 1.0
    d = np.sqrt(np.diag(A))
    Ax, Ix = A.astype(LD), I.astype(LD)
    X = lapack.dpotrs(L, I, lower=1)[0].astype(LD)
    rel = np.inf
    for _ in range(INVERSE_REFINE_STEPS):
        r = (Ix - Ax @ X).astype(np.float64)
        dX = lapack.dpotrs(L, r, lower=1)[0]
        step = _scaled_max(d, cols, dX) / _scaled_max(d, cols, X.astype(np.float64))
        if step >= rel:
            break
        X, rel = X + dX, step
    return X.astype(np.float64), rel


def inverse_forward_error(A, X, X_ref, cols):
    """max |d_i d_j (X - X_ref)_ij| / max |d_i d_j (X_ref)_ij| on the columns `cols`, d = sqrt(diag A): the error of the inverse of
    H = A / (d d^T), invariant under diagonal scaling.  X is the full n x n inverse, X_ref what inverse_ref returned."""
    cols = np.asarray(cols)
    d = np.sqrt(np.diag(A))
    return _scaled_max(d, cols, X[:, cols] - X_ref) / _scaled_max(d, cols, X_ref)


def inverse_right_residual(A, X, cols):
    """max |H (D X D) - I| on the columns `cols`, H = A / (d d^T), D = diag(d): (A X)_ij d_j / d_i - [i = j], product and difference
    in extended precision"""
    cols = np.asarray(cols)
    d = np.sqrt(np.diag(A).astype(LD))
    R = (A.astype(LD) @ X[:, cols].astype(LD)) * d[None, cols] / d[:, None]
    R[cols, np.arange(len(cols))] -= 1.0
    return float(np.max(np.abs(R)))


def inverse_lapack(A):
    """LAPACK's plain inverse, dpotrf + dpotri, full and exactly symmetric"""
    L, info = factor_ref(A)
    assert info == 0
    X, info = lapack.dpotri(L, lower=1)
    assert info == 0
    return np.tril(X) + np.tril(X, -1).T


def partial_factorisation_inverse(A, tb):
    """chol_spd_inverse_dev's design restated in numpy, in doubles: the right-looking blocked factorisation of W = [A .; I 0], block
    size tb, stopped after the panels of A.  Every panel below a diagonal tile -- the rows of A and the identity rows alike -- is
    multiplied by the explicit inverse of the tile's factor, and the trailing update subtracts X X^T per panel from the lower right
    block, which ends as -A^-1.  -> A^-1, full and exactly symmetric"""
    n = A.shape[0]
    W = np.zeros((2 * n, 2 * n))
    W[:n, :n] = A
    W[n:, :n] = np.eye(n)
    for k in range(0, n, tb):
        e = min(k + tb, n)
        Lkk = np.linalg.cholesky(W[k:e, k:e])
        inv = solve_triangular(Lkk, np.eye(e - k), lower=True)
        P = W[e:n + e, k:e] @ inv.T             # (identity row i is still zero left of column i: the rows from n + e on have nothing here)
        W[e:n + e, k:e] = P
        Pa, Px = P[:n - e], P[n - e:]           # the rows of A | the identity rows
        W[e:n, e:n] -= Pa @ Pa.T
        W[n:n + e, e:n] -= Px @ Pa.T
        W[n:n + e, n:n + e] -= Px @ Px.T
    X = -W[n:, n:]
    return np.tril(X) + np.tril(X, -1).T
