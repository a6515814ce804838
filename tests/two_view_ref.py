"""A 50-digit reference for the two-view initialiser (mpmath, mp.dps = 50), in the style of mp_ref.py.

Independent of oracle/two_view_np.py and of the device code.  The double inputs (pixels, K, and a pose where one is given)
are taken as exact; every product and sum below is carried at 50 digits, so forming Gram matrices -- which squares the
condition number, at most (1e7)^2 here -- costs 14 of the 50 digits and leaves the results exact to far below a double's ulp.

  fundamental()            unit null vector of the n x 9 epipolar system x1^T F x2 = 0 and its nine singular values
  GramPrefix               the same for nested prefixes of one correspondence list (the Gram matrix is a prefix sum)
  essential_hypotheses()   E = K^T F K, its SVD, and the four (R, t) of the decomposition as an unordered list
  triangulate()            6 x 4 DLT null vector, X = h[:3] / h[3], with the four singular values
  cheirality()             per hypothesis and point, the depths z1 and z2 and |X|
"""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = 2.0 ** -52
ZERO, ONE = mp.mpf(0), mp.mpf(1)


def _row9(a, b):
    u1, v1, u2, v2 = mp.mpf(float(a[0])), mp.mpf(float(a[1])), mp.mpf(float(b[0])), mp.mpf(float(b[1]))
    return [u1 * u2, u1 * v2, u1, v1 * u2, v1 * v2, v1, u2, v2, ONE]


def _null_and_sigmas(G, n):
    """eigen-decomposition of the symmetric n x n Gram matrix G (list of lists): (unit eigenvector of the smallest
    eigenvalue as a list of mpf, singular values sqrt(|lambda|) descending as a list of mpf)"""
    ev, Q = mp.eigsy(mp.matrix(G))
    order = sorted(range(n), key=lambda i: ev[i])
    k = order[0]
    v = [Q[i, k] for i in range(n)]
    nv = mp.sqrt(mp.fsum(x * x for x in v))
    return [x / nv for x in v], [mp.sqrt(abs(ev[i])) for i in reversed(order)]


class GramPrefix:
    """A^T A of the n x 9 system, accumulated once over the rows in order; at(n) decomposes the Gram matrix of the first n
    rows.  The accumulation runs at 60 digits so that the running sums carry no error at the 50 the rest works with."""

    def __init__(self, f1, f2, sizes):
        self.sizes = sorted(set(int(s) for s in sizes))
        self.out = {}
        want = set(self.sizes)
        with mp.workdps(60):
            G = [[ZERO] * 9 for _ in range(9)]
            for i in range(self.sizes[-1]):
                r = _row9(f1[i], f2[i])
                for p in range(9):
                    rp, Gp = r[p], G[p]
                    for q in range(p, 9):
                        Gp[q] += rp * r[q]
                if i + 1 in want:
                    self.out[i + 1] = [[G[min(p, q)][max(p, q)] for q in range(9)] for p in range(9)]

    def at(self, n):
        """(F as a 9-list of mpf, sigma[0..8] descending)"""
        return _null_and_sigmas(self.out[n], 9)


def fundamental(f1, f2):
    """unit null vector (row-major F, x1^T F x2 = 0) of the n x 9 system and all nine singular values, descending"""
    n = len(f1)
    rows = [_row9(f1[i], f2[i]) for i in range(n)]
    G = [[ZERO] * 9 for _ in range(9)]
    for p in range(9):
        for q in range(p, 9):
            G[p][q] = G[q][p] = mp.fsum(r[p] * r[q] for r in rows)
    return _null_and_sigmas(G, 9)


def gram(A):
    """A^T A of a double matrix (numpy, m x n), every entry taken as exact, as a list of lists of mpf"""
    A = np.asarray(A, dtype=float)
    n = A.shape[1]
    rows = [[mp.mpf(float(x)) for x in r] for r in A]
    G = [[ZERO] * n for _ in range(n)]
    for p in range(n):
        for q in range(p, n):
            G[p][q] = G[q][p] = mp.fsum(r[p] * r[q] for r in rows)
    return G


def null_vector(A):
    """unit right singular vector of the smallest singular value of the double matrix A, and all singular values descending"""
    return _null_and_sigmas(gram(A), np.asarray(A).shape[1])


def cholesky_upper(G):
    """the upper-triangular R with R^T R = G and a non-negative diagonal (list of lists of mpf).  A pivot that comes out
    below zero -- G exactly singular, up to the 50th digit -- is taken as zero and so is the rest of its row"""
    n = len(G)
    R = [[ZERO] * n for _ in range(n)]
    for k in range(n):
        d = G[k][k] - mp.fsum(R[i][k] ** 2 for i in range(k))
        if d <= 0:
            continue
        R[k][k] = mp.sqrt(d)
        for j in range(k + 1, n):
            R[k][j] = (G[k][j] - mp.fsum(R[i][k] * R[i][j] for i in range(k))) / R[k][k]
    return R


# ---------------------------------------------------------------- 3x3 helpers on lists of mpf
def _m(A):
    return [[mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in row] for row in A]


def _mm(A, B):
    return [[mp.fsum(A[i][k] * B[k][j] for k in range(len(B))) for j in range(len(B[0]))] for i in range(len(A))]


def _tr(A):
    return [[A[j][i] for j in range(len(A))] for i in range(len(A[0]))]


def _mv(A, v):
    return [mp.fsum(A[i][k] * v[k] for k in range(len(v))) for i in range(len(A))]


def _det3(M):
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
            + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _unit(v):
    n = mp.sqrt(mp.fsum(x * x for x in v))
    return [x / n for x in v]


def svd3(M):
    """(U, s, V) of a 3x3 with s descending: V and s^2 from eigsy of M^T M, u1 and u2 = M v / s, and u3 the eigenvector of
    the smallest eigenvalue of M M^T (defined even when s3 = 0), signed so that u3 = M v3 / s3 wherever s3 > 0"""
    M = _m(M)
    ev, Q = mp.eigsy(mp.matrix(_mm(_tr(M), M)))
    order = sorted(range(3), key=lambda i: -ev[i])
    s = [mp.sqrt(abs(ev[i])) for i in order]
    V = [[Q[r, order[c]] for c in range(3)] for r in range(3)]
    cols = []
    for c in range(2):
        cols.append(_unit(_mv(M, [V[r][c] for r in range(3)])))
    ev2, Q2 = mp.eigsy(mp.matrix(_mm(M, _tr(M))))
    k = min(range(3), key=lambda i: ev2[i])
    u3 = _unit([Q2[r, k] for r in range(3)])
    mv3 = _mv(M, [V[r][2] for r in range(3)])
    if mp.fsum(a * b for a, b in zip(u3, mv3)) < 0:
        u3 = [-x for x in u3]
    cols.append(u3)
    return [[cols[c][r] for c in range(3)] for r in range(3)], s, V


def essential_hypotheses(F, K):
    """F: 9 values row-major (mpf or float), K: 3x3 doubles.  Returns dict(E, U, s, V, hyps) with hyps the four (R, t) of
    two_view_geometry.cpp:61-64 -- R = U W V^T | U W^T V^T with the determinant made positive, t = +-u3 -- as an UNORDERED
    collection: which of them comes first depends on the sign conventions of whoever computes the SVD"""
    Fm = [[F[3 * i + j] if isinstance(F[3 * i + j], mp.mpf) else mp.mpf(float(F[3 * i + j])) for j in range(3)] for i in range(3)]
    Km = _m(np.asarray(K, dtype=float).tolist())
    E = _mm(_mm(_tr(Km), Fm), Km)
    U, s, V = svd3(E)
    W = [[ZERO, -ONE, ZERO], [ONE, ZERO, ZERO], [ZERO, ZERO, ONE]]
    Rs = []
    for Wk in (W, _tr(W)):
        R = _mm(_mm(U, Wk), _tr(V))
        if _det3(R) < 0:
            R = [[-x for x in row] for row in R]
        Rs.append(R)
    u3 = [U[r][2] for r in range(3)]
    m3 = [-x for x in u3]
    return dict(E=E, U=U, s=s, V=V, hyps=[(Rs[0], u3), (Rs[0], m3), (Rs[1], u3), (Rs[1], m3)])


def _projection(K, R, t):
    """K [R^T | -R^T t]: the camera with pose (R, t) in frame 1"""
    Rt = _tr(R)
    c = _mv(Rt, t)
    return _mm(K, [Rt[i] + [-c[i]] for i in range(3)])


def _hat_rows(u, v, P):
    """hat([u, v, 1]) P, three rows of four"""
    return [[-P[1][c] + v * P[2][c] for c in range(4)], [P[0][c] - u * P[2][c] for c in range(4)],
            [-v * P[0][c] + u * P[1][c] for c in range(4)]]


class Triangulator:
    """the 6 x 4 DLT of one pair of cameras (identity and (R, t)), both taken as the exact matrices given"""

    def __init__(self, R, t, K):
        Km = _m(np.asarray(K, dtype=float).tolist())
        I3 = [[ONE if i == j else ZERO for j in range(3)] for i in range(3)]
        self.R = _m(R.tolist()) if isinstance(R, np.ndarray) else R
        self.t = [mp.mpf(float(x)) if not isinstance(x, mp.mpf) else x for x in t]
        self.P1 = _projection(Km, I3, [ZERO] * 3)
        self.P2 = _projection(Km, self.R, self.t)

    def point(self, x1, x2):
        """(X as 3 mpf, sigma[0..3] descending)"""
        A = (_hat_rows(mp.mpf(float(x1[0])), mp.mpf(float(x1[1])), self.P1)
             + _hat_rows(mp.mpf(float(x2[0])), mp.mpf(float(x2[1])), self.P2))
        G = [[mp.fsum(A[r][p] * A[r][q] for r in range(6)) for q in range(4)] for p in range(4)]
        h, sig = _null_and_sigmas(G, 4)
        return [h[0] / h[3], h[1] / h[3], h[2] / h[3]], sig

    def depths(self, X):
        """(z1, z2): the depth of X in camera 1 and in camera 2, p2 = R^T (X - t)"""
        d = [X[i] - self.t[i] for i in range(3)]
        return X[2], mp.fsum(self.R[i][2] * d[i] for i in range(3))


def project(K, R, t, X):
    """(u, v) as mpf: the pixel of the frame-1 point X in the camera with pose (R, t), every double taken as exact"""
    Km = _m(np.asarray(K, dtype=float).tolist())
    Rm = _m(np.asarray(R, dtype=float).tolist())
    d = [mp.mpf(float(X[i])) - mp.mpf(float(t[i])) for i in range(3)]
    p = _mv(_tr(Rm), d)
    return Km[0][0] * p[0] / p[2] + Km[0][2], Km[1][1] * p[1] / p[2] + Km[1][2]


def triangulate(x1, x2, R, t, K):
    """X (3 mpf) and sigma1..sigma4 of the 6 x 4 system [hat(x1) P1; hat(x2) P2] (two_view_geometry.cpp:105-126)"""
    return Triangulator(R, t, K).point(x1, x2)


def cheirality(f1, f2, hyps, K):
    """per hypothesis a list over the points of (z1, z2, |X|) as mpf; a point passes where z1 > 0 and z2 > 0 (:91, :96)"""
    out = []
    for R, t in hyps:
        T = Triangulator(R, t, K)
        rows = []
        for a, b in zip(f1, f2):
            X, _ = T.point(a, b)
            z1, z2 = T.depths(X)
            rows.append((z1, z2, mp.sqrt(mp.fsum(x * x for x in X))))
        out.append(rows)
    return out


def fail_counts(ch):
    """the number of points that fail each hypothesis, from cheirality()'s output"""
    return [sum(1 for z1, z2, _ in rows if not (z1 > 0 and z2 > 0)) for rows in ch]


def f64(x):
    if isinstance(x, (list, tuple)):
        return np.array([f64(y) for y in x], dtype=float)
    return float(x)
