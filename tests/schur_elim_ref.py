"""A 50-digit reference for the elimination of the landmarks from the normal equations of bundle adjustment, and the error
units the device is judged in.  CPU only (mpmath, as mp_ref.py).

Input: float64 r [n, 2], Jc [n, 2, 6], Jp [n, 2, 3] per observation (whitened where information matrices are set; the columns of
constant dofs and constant landmarks zero, as evaluate() returns them), the diagonals dc [n_cams, 6], dp [n_pts, 3] and the
constant masks.  With W_i = Jc_i^T Jp_i, V_j = sum_i Jp_i^T Jp_i + diag(dp_j), gp_j = sum_i Jp_i^T r_i:
    S   = sum_i Jc_i^T Jc_i + diag(dc | 1 for a constant dof) - sum_j W_aj V_j^-1 W_bj^T        (lower block triangle)
    rhs = -sum_i Jc_i^T r_i + sum_j W_aj V_j^-1 gp_j                                            (0 for a constant dof)
    dxc = S^-1 rhs,    dxp_j = V_j^-1 (-gp_j - sum_i W_i^T dxc_c(i))                            (test_reduced_system_and_step's signs)
where W_aj is the sum of W_i over the observations of landmark j by camera a.  A constant landmark, and one whose V_j is singular
at 50 digits (one observation and dp = 0), is left out: its inverse is zero and so is its dxp.

Error units (no constant from the code under test in them; lambda_1 >= lambda_2 >= lambda_3 the eigenvalues of V_j + D_j,
|.| the Frobenius norm, |W_aj| the sum of |W_i| over camera a's observations of j, |V_j^-1| = 1 / lambda_3):
  (a block: the 3 x 3 piece of a camera pair's block that belongs to one half -- rotation or position -- of each camera, and the
   matching 3 entries of rhs: the halves scale differently, and a unit per half is exact under a change of the unit of length)
    S block (a, b)   u_wide = EPS sum_j (lambda_1 / lambda_3)_j |W_aj| |V_j^-1| |W_bj|  +  EPS n_ab max|term|
    rhs block a      u_wide = EPS sum_j (lambda_1 / lambda_3)_j |W_aj| |V_j^-1| |gp_j|  +  EPS n_a max|term|
    dxp_j            u_wide = EPS (lambda_1 / lambda_3)_j |V_j^-1| (|gp_j| + sum_i |W_i| |dxc_c(i)|)  +  EPS n_j |V_j^-1| max|term|
    Hpp_j, gp_j      u = EPS n_j max|term|
The first part is what an inverse known to EPS lambda_1 / lambda_3 -- a factorisation's accuracy -- costs the product; the second
is the accumulation of n terms (pairs of observations for S; the camera block's observations counted in on the diagonal) the
largest of which has the entry max|term|.  An error is its largest entry over the block, and a result is judged as err / u.

The units the tests ASSERT are narrower than these.  Every Jp_i^T Jp_i is a part of V_j, so |Jp_i V_j^-1/2| <= 1 and a term
W_aj V_j^-1 W_bj^T is no larger than |Jc_a| |Jc_b| however ill-conditioned V_j is, while |W_aj| |V_j^-1| |W_bj| grows with
lambda_1 / lambda_3: on a landmark of kappa 1e10, C u_wide is larger than the term itself and a DROPPED landmark passes.  A
Cholesky factor of V_j + D_j has a backward error of EPS |V_j|, which moves the term by EPS (lambda_1 / lambda_3)
|W_aj V_j^-1/2| |W_bj V_j^-1/2| (|W V^-1/2|^2 = trace(W V^-1 W^T), evaluated at 50 digits), and a solve by EPS
(lambda_1 / lambda_3) |x|; so
    S block (a, b)   u = EPS sum_j (lambda_1 / lambda_3)_j |W_aj V_j^-1/2| |W_bj V_j^-1/2|  +  EPS n_ab max|term|
    rhs block a      u = EPS sum_j (lambda_1 / lambda_3)_j |W_aj V_j^-1/2| |V_j^-1/2 gp_j|  +  EPS n_a max|term|
    dxp_j            u = EPS (lambda_1 / lambda_3)_j |dxp_j|  +  EPS n_j |V_j^-1| max|term|
(u <= u_wide always: |W V^-1/2|^2 <= |W|^2 |V^-1|.)  The tests print err / u_wide next to err / u.

The constant C.  A plain float64 elimination (numpy: LAPACK Cholesky of V_j + D_j, triangular solves, sums in observation
order -- `lapack_elimination`) reaches at worst err / u = 5.89 on the cases of schur_elim_cases.py (measured by
test_schur_elim_reference_cpu.py, per quantity in DESIGN.md "Accuracy"); C is 8 times that, rounded up to a power of two -- the
factor 8 for FMA contraction and the device's different but fixed summation order:
    C = 64"""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = float(np.finfo(np.float64).eps)
C = 64.0
LAPACK_WORST = 5.89          # Hpp of the 260-observation landmark, summed in sequence
_mpf = np.frompyfunc(mp.mpf, 1, 1)
_flt = np.frompyfunc(float, 1, 1)


def mpa(a):
    """float array -> object array of mpf (exact)"""
    return _mpf(np.asarray(a, dtype=np.float64))


def f64(a):
    return np.asarray(_flt(a), dtype=np.float64)


def _inv3(A):
    """inverse of a 3 x 3 object array by cofactors AT 50 DIGITS (kappa^2 1e-50 is nothing here); None if singular there"""
    a, b, c, d, e, f = A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]
    C00, C01, C02 = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * C00 + b * C01 + c * C02
    if a <= 0 or d <= 0 or f <= 0 or not det > mp.mpf("1e-40") * a * d * f:
        return None
    out = np.empty((3, 3), object)
    out[0, 0], out[0, 1], out[0, 2] = C00 / det, C01 / det, C02 / det
    out[1, 1], out[1, 2], out[2, 2] = (a * f - c * c) / det, (b * c - a * e) / det, (a * d - b * b) / det
    out[1, 0], out[2, 0], out[2, 1] = out[0, 1], out[0, 2], out[1, 2]
    return out


def _fro(a):
    return float(np.sqrt(np.sum(np.asarray(a, np.float64) ** 2)))


def _groups(idx):
    """{value: positions} in order of appearance"""
    out = {}
    for n, v in enumerate(idx):
        out.setdefault(int(v), []).append(n)
    return out


class Reference:
    """the quantities of the module docstring as float64 arrays (rounded from 50 digits) and their units:
    Vd [np, 3, 3], Vinv [np, 3, 3] (zero where left out), lam [np, 3] descending (nan where left out), out [np] left out,
    Hpp, gp and u_Hpp, u_gp; S [6nc, 6nc] lower block triangle, rhs, u_S [2nc, 2nc], u_rhs [2nc], s_worst / rhs_worst of those shapes:
    the landmark with the largest share of the unit; dxc; dxp(dxc) -> (dxp, u_dxp)"""

    def __init__(self, r, Jc, Jp, obs_cam, obs_pt, n_cams, n_pts, dc, dp, cam_fixed=None, pt_fixed=None, solve=True, keep_terms=None):
        oc, op = np.asarray(obs_cam, np.int64), np.asarray(obs_pt, np.int64)
        r, Jc, Jp = np.asarray(r, float), np.asarray(Jc, float), np.asarray(Jp, float)
        self.nc, self.np_, self.oc, self.op = n_cams, n_pts, oc, op
        cf = np.zeros((n_cams, 6), bool) if cam_fixed is None else np.asarray(cam_fixed).reshape(-1, 6) != 0
        pf = np.zeros(n_pts, bool) if pt_fixed is None else np.asarray(pt_fixed) != 0
        dc, dp = np.asarray(dc, float).reshape(n_cams, 6), np.asarray(dp, float).reshape(n_pts, 3)
        rm, Jcm, Jpm = mpa(r), mpa(Jc), mpa(Jp)
        n = 6 * n_cams
        S = np.full((n, n), mp.mpf(0), object)
        rhs = np.full(n, mp.mpf(0), object)
        h = 2 * n_cams          # units per HALF of a camera block (rotation | position): the two scale differently
        uS1, uSn, uSt, uS0 = np.zeros((h, h)), np.zeros((h, h)), np.zeros((h, h)), np.zeros((h, h))
        uS1max, self.s_worst = np.zeros((h, h)), np.full((h, h), -1)
        uR1, uRn, uRt, uR0 = np.zeros(h), np.zeros(h), np.zeros(h), np.zeros(h)
        uR1max, self.rhs_worst = np.zeros(h), np.full(h, -1)

        def halves(M):
            """largest |entry| per 3-row (and, for a matrix, 3-column) half of one camera's block"""
            M = np.abs(np.asarray(M, np.float64))
            return M.reshape(2, 3, 2, 3).max(axis=(1, 3)) if M.ndim == 2 else M.reshape(2, 3).max(1)
        # camera blocks
        for a, idx in _groups(oc).items():
            A = Jcm[idx].reshape(-1, 6)
            H = A.T.dot(A)
            g = A.T.dot(rm[idx].reshape(-1))
            sl = slice(6 * a, 6 * a + 6)
            S[sl, sl] += H
            rhs[sl] -= g
            ha = slice(2 * a, 2 * a + 2)
            uSn[ha, ha] += len(idx); uRn[ha] += len(idx)
            uSt[ha, ha] = np.abs(np.einsum("nki,nkj->nij", Jc[idx], Jc[idx])).max(0).reshape(2, 3, 2, 3).max(axis=(1, 3))
            uRt[ha] = np.abs(np.einsum("nki,nk->ni", Jc[idx], r[idx])).max(0).reshape(2, 3).max(1)
        for a in range(n_cams):
            for q in range(6):
                S[6 * a + q, 6 * a + q] += mp.mpf(1) if cf[a, q] else mp.mpf(float(dc[a, q]))
                if cf[a, q]:
                    rhs[6 * a + q] = mp.mpf(0)
        # landmarks
        self.Hpp, self.gp = np.zeros((n_pts, 3, 3)), np.zeros((n_pts, 3))
        self.u_Hpp, self.u_gp = np.zeros(n_pts), np.zeros(n_pts)
        self.Vd, self.Vinv, self.lam = np.zeros((n_pts, 3, 3)), np.zeros((n_pts, 3, 3)), np.full((n_pts, 3), np.nan)
        self.out = np.ones(n_pts, bool)
        self._lm = {}
        self.terms = {}          # keep_terms: landmarks whose blocks W_aj V_j^-1 W_bj^T are kept, {j: {(a, b): 6 x 6}}
        Wn = np.linalg.norm(np.einsum("nki,nkj->nij", Jc, Jp).reshape(-1, 2, 3, 3), axis=(2, 3))      # [n, half]
        self._Wn = Wn
        by_pt = _groups(op)
        for j in range(n_pts):
            idx = by_pt.get(j, [])
            P = Jpm[idx].reshape(-1, 3) if idx else np.empty((0, 3), object)
            V = P.T.dot(P) if idx else np.full((3, 3), mp.mpf(0), object)
            g = P.T.dot(rm[idx].reshape(-1)) if idx else np.full(3, mp.mpf(0), object)
            self.Hpp[j], self.gp[j] = f64(V), f64(g)
            if idx:
                self.u_Hpp[j] = EPS * len(idx) * float(np.abs(np.einsum("nki,nkj->nij", Jp[idx], Jp[idx])).max())
                self.u_gp[j] = EPS * len(idx) * float(np.abs(np.einsum("nki,nk->ni", Jp[idx], r[idx])).max())
            Vd = V.copy()
            for q in range(3):
                Vd[q, q] += mp.mpf(float(dp[j, q]))
            self.Vd[j] = f64(Vd)
            Vi = None if pf[j] else _inv3(Vd)
            if Vi is None:
                continue
            self.out[j] = False
            self.Vinv[j] = f64(Vi)
            ev = mp.eigsy(mp.matrix(Vd.tolist()), eigvals_only=True)
            lam = sorted((float(x) for x in ev), reverse=True)
            self.lam[j] = lam
            kap, vin = lam[0] / lam[2], 1.0 / lam[2]
            cams_j = _groups(oc[idx])
            Wa, Wna, Ea, Yna = {}, {}, {}, {}
            for a, loc in cams_j.items():
                ii = [idx[t] for t in loc]
                Wi = [Jcm[i].T.dot(Jpm[i]) for i in ii]
                Wa[a] = sum(Wi)
                Wna[a] = Wn[ii].sum(0)
                Ea[a] = Wa[a].dot(Vi)
                # |W_i V_j^-1/2| per half: the square root of the trace of that half of W_i V_j^-1 W_i^T, at 50 digits
                q = np.array([f64((Wk.dot(Vi) * Wk).sum(1)) for Wk in Wi])
                Yna[a] = np.sqrt(np.maximum(q, 0.0).reshape(-1, 2, 3).sum(2)).sum(0)
            gn = _fro(f64(g))
            gy = float(mp.sqrt(g.dot(Vi).dot(g)))
            self._lm[j] = (Vi, g, Wa, kap, vin, idx)
            for a in Wa:
                sa, ha = slice(6 * a, 6 * a + 6), slice(2 * a, 2 * a + 2)
                t = Ea[a].dot(g)
                rhs[sa] += np.where(cf[a], mp.mpf(0), t)
                uR0[ha] += kap * Wna[a] * vin * gn
                part = kap * Yna[a] * gy
                uR1[ha] += part; uRn[ha] += len(cams_j[a]); uRt[ha] = np.maximum(uRt[ha], halves(f64(t)))
                self.rhs_worst[ha] = np.where(part > uR1max[ha], j, self.rhs_worst[ha])
                uR1max[ha] = np.maximum(uR1max[ha], part)
                for b in Wa:
                    if b > a:
                        continue
                    T = Ea[a].dot(Wa[b].T)
                    if keep_terms is not None and j in keep_terms:
                        self.terms.setdefault(j, {})[(a, b)] = f64(T)
                    S[sa, 6 * b:6 * b + 6] -= T
                    hb = slice(2 * b, 2 * b + 2)
                    uS0[ha, hb] += kap * vin * np.outer(Wna[a], Wna[b])
                    part = kap * np.outer(Yna[a], Yna[b])
                    uS1[ha, hb] += part; uSn[ha, hb] += len(cams_j[a]) * len(cams_j[b])
                    uSt[ha, hb] = np.maximum(uSt[ha, hb], halves(f64(T)))
                    self.s_worst[ha, hb] = np.where(part > uS1max[ha, hb], j, self.s_worst[ha, hb])
                    uS1max[ha, hb] = np.maximum(uS1max[ha, hb], part)
        for a in range(n_cams):          # the lower block triangle only, the diagonal blocks' lower triangles only
            for b in range(a + 1, n_cams):
                S[6 * a:6 * a + 6, 6 * b:6 * b + 6] = mp.mpf(0)
        self._S, self._rhs = S, rhs
        self.S = np.tril(f64(S))
        self.rhs = f64(rhs)
        self.u_S = EPS * uS1 + EPS * uSn * uSt
        self.u_rhs = EPS * uR1 + EPS * uRn * uRt
        self.u_S_wide = EPS * uS0 + EPS * uSn * uSt
        self.u_rhs_wide = EPS * uR0 + EPS * uRn * uRt
        self.dxc = None
        if solve:
            Sf = mp.matrix(n, n)
            for i in range(n):
                for k in range(i + 1):
                    Sf[i, k] = S[i, k]; Sf[k, i] = S[i, k]
            x = mp.cholesky_solve(Sf, mp.matrix(list(rhs)))
            self._dxc = np.array([x[i] for i in range(n)], object)
            self.dxc = f64(self._dxc)

    def _full(self):
        S = self._S
        return np.where(np.tri(len(S), dtype=bool), S, S.T)

    def apply(self, x):
        """(S x, u [2nc]): the product at 50 digits and its unit per half block, sum_b 3 u_S[a, b] max|x_b| -- what errors of
        u_S in the blocks of S cost the product"""
        x = np.asarray(x, float).reshape(-1)
        y = f64(self._full().dot(mpa(x)))
        U = np.tril(self.u_S) + np.tril(self.u_S, -1).T
        return y, 3.0 * U @ np.abs(x).reshape(-1, 3).max(1)

    def block_jacobi(self, x):
        """(z, u) with S_aa z_a = x_a per camera (the Schur-Jacobi preconditioner) and the first-order bound per ENTRY,
        u = |S_aa^-1| (U_aa + 6 EPS |S_aa|) |z_a|: U_aa the units of the block's entries, 6 EPS |S_aa| the backward error of a
        6 x 6 Cholesky solve"""
        x = np.asarray(x, float).reshape(-1)
        Sf = self._full()
        z, u = np.zeros(len(x)), np.zeros(len(x))
        for a in range(self.nc):
            sl = slice(6 * a, 6 * a + 6)
            A = mp.matrix(Sf[sl, sl].tolist())
            Ai = A ** -1
            za = Ai * mp.matrix(list(mpa(x[sl])))
            z[sl] = [float(v) for v in za]
            Ua = np.kron(np.maximum(self.u_S[2 * a:2 * a + 2, 2 * a:2 * a + 2], self.u_S[2 * a:2 * a + 2, 2 * a:2 * a + 2].T), np.ones((3, 3)))
            Aabs, Aiabs = np.abs(f64(Sf[sl, sl])), np.abs(np.array([[float(Ai[i, k]) for k in range(6)] for i in range(6)]))
            u[sl] = Aiabs @ ((Ua + 6 * EPS * Aabs) @ np.abs(z[sl]))
        return z, u

    def kappa_S(self):
        """2-norm condition number of S scaled to a unit diagonal (float64; what a Cholesky solve's error follows)"""
        Sf = self.S + np.tril(self.S, -1).T
        d = 1.0 / np.sqrt(np.diag(Sf))
        w = np.linalg.eigvalsh(Sf * d[:, None] * d[None, :])
        return float(w.max() / w.min())

    def point_covariance(self, js):
        """(blocks [m, 3, 3], u [m]) of (J^T J)^-1 restricted to the landmarks js, for a reference built with dc = dp = 0:
        Sigma_jj = V_j^-1 + V_j^-1 F_j^T S^-1 F_j V_j^-1, F_j the landmark's W blocks stacked.  A factorisation of V_j and one
        of S move it by EPS ((lambda_1 / lambda_3)_j (|V_j^-1| + 2 |second term|) + kappa(S) |second term|) (Frobenius), and S
        itself is only known to its units U (u_S, entry by entry), which S^-1 carries into the second term:
            u = EPS ((lambda_1 / lambda_3)_j (|V_j^-1| + 2 |second term|) + kappa(S) |second term|) + | |H|^T U |H| |,  H = S^-1 F_j V_j^-1"""
        n = 6 * self.nc
        Sf = self._full()
        Si = mp.matrix(Sf.tolist()) ** -1
        Si = np.array([[Si[i, k] for k in range(n)] for i in range(n)], object)
        kS = self.kappa_S()
        U = np.kron(np.tril(self.u_S) + np.tril(self.u_S, -1).T, np.ones((3, 3)))
        out, u = np.zeros((len(js), 3, 3)), np.zeros(len(js))
        for m, j in enumerate(js):
            Vi, g, Wa, kap, vin, idx = self._lm[int(j)]
            F = np.full((n, 3), mp.mpf(0), object)
            for a, W in Wa.items():
                F[6 * a:6 * a + 6] = W
            G = F.dot(Vi)
            H = Si.dot(G)
            second = G.T.dot(H)
            out[m] = f64(Vi + second)
            Ha = np.abs(f64(H))
            u[m] = EPS * (kap * (_fro(f64(Vi)) + 2 * _fro(f64(second))) + kS * _fro(f64(second))) + _fro(Ha.T @ U @ Ha)
        return out, u

    def dxp(self, dxc=None):
        """(dxp [np, 3], u [np]) at the given camera step (float64; default the reference's own, at 50 digits)"""
        d = self._dxc if dxc is None else mpa(np.asarray(dxc, float).reshape(-1))
        dn = np.linalg.norm(f64(d).reshape(-1, 2, 3), axis=2)          # [camera, half]
        out, u, wide = np.zeros((self.np_, 3)), np.zeros(self.np_), np.zeros(self.np_)
        for j, (Vi, g, Wa, kap, vin, idx) in self._lm.items():
            v = -g
            for a, W in Wa.items():
                v = v - W.T.dot(d[6 * a:6 * a + 6])
            out[j] = f64(Vi.dot(v))
            terms = (self._Wn[idx] * dn[self.oc[idx]]).sum(1)
            gn = _fro(self.gp[j])
            acc = EPS * (len(idx) + 1) * vin * max(gn, terms.max() if len(idx) else 0.0)
            u[j] = EPS * kap * np.linalg.norm(out[j]) + acc
            wide[j] = EPS * kap * vin * (gn + terms.sum()) + acc
        self.u_dxp_wide = wide
        return out, u


def block_err(X, Y):
    """largest entry of |X - Y| per 3 x 3 block of a matrix, or per 3 entries of a vector (the units' halves)"""
    E = np.abs(np.asarray(X) - np.asarray(Y))
    h = E.shape[0] // 3
    if E.ndim == 2:
        return E.reshape(h, 3, h, 3).max(axis=(1, 3))
    return E.reshape(h, 3).max(1)


def ratio(err, u):
    """err / u, 0 where both are zero and inf where only u is"""
    err, u = np.asarray(err, float), np.asarray(u, float)
    return np.where(u > 0, err / np.where(u > 0, u, 1.0), np.where(err == 0, 0.0, np.inf))


def lapack_elimination(r, Jc, Jp, obs_cam, obs_pt, n_cams, n_pts, dc, dp, cam_fixed, pt_fixed, left_out):
    """the same quantities in plain float64: LAPACK Cholesky of V_j + D_j and triangular solves, sums in observation order.
    Returns dict(Hpp, gp, S (lower), rhs, dxc, dxp_of(dxc))"""
    oc, op = np.asarray(obs_cam, np.int64), np.asarray(obs_pt, np.int64)
    cf = np.asarray(cam_fixed).reshape(-1, 6) != 0
    dc, dp = np.asarray(dc, float).reshape(n_cams, 6), np.asarray(dp, float).reshape(n_pts, 3)
    n = 6 * n_cams
    Hcc, gc = np.zeros((n_cams, 6, 6)), np.zeros((n_cams, 6))
    Hpp, gp = np.zeros((n_pts, 3, 3)), np.zeros((n_pts, 3))
    np.add.at(Hcc, oc, np.einsum("nki,nkj->nij", Jc, Jc)); np.add.at(gc, oc, np.einsum("nki,nk->ni", Jc, r))
    np.add.at(Hpp, op, np.einsum("nki,nkj->nij", Jp, Jp)); np.add.at(gp, op, np.einsum("nki,nk->ni", Jp, r))
    W = np.einsum("nki,nkj->nij", Jc, Jp)
    S, rhs = np.zeros((n, n)), -gc.reshape(-1).copy()
    for a in range(n_cams):
        S[6 * a:6 * a + 6, 6 * a:6 * a + 6] = Hcc[a] + np.diag(np.where(cf[a], 1.0, dc[a]))
    chol = {}
    for j, idx in _groups(op).items():
        if left_out[j]:
            continue
        Lc = np.linalg.cholesky(Hpp[j] + np.diag(dp[j]))
        chol[j] = (Lc, idx)
        Y = [np.linalg.solve(Lc, W[i].T) for i in idx]               # L^-1 W_i^T  (3 x 6)
        y = np.linalg.solve(Lc, gp[j])
        for p, i in enumerate(idx):
            a = oc[i]
            rhs[6 * a:6 * a + 6] += Y[p].T @ y
            for q, l in enumerate(idx):
                b = oc[l]
                if b <= a:
                    S[6 * a:6 * a + 6, 6 * b:6 * b + 6] -= Y[p].T @ Y[q]
    rhs[cf.reshape(-1)] = 0.0
    S = np.tril(S)
    for a in range(n_cams):
        for b in range(a + 1, n_cams):
            S[6 * a:6 * a + 6, 6 * b:6 * b + 6] = 0.0
    Sf = S + np.tril(S, -1).T
    dxc = np.linalg.solve(Sf, rhs)

    def dxp_of(d):
        d = np.asarray(d, float).reshape(-1, 6)
        out = np.zeros((n_pts, 3))
        for j, (Lc, idx) in chol.items():
            v = -gp[j].copy()
            for i in idx:
                v -= Jp[i].T @ (Jc[i] @ d[oc[i]])
            out[j] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, v))
        return out
    return dict(Hpp=Hpp, gp=gp, S=S, rhs=rhs, dxc=dxc, dxp_of=dxp_of)


def brute_force(r, Jc, Jp, obs_cam, obs_pt, n_cams, n_pts, dc, dp, cam_fixed, left_out):
    """(dxc, dxp) from ONE dense solve of (J^T J + D) x = -J^T r at 50 digits over the cameras and the landmarks that are not
    left out (constant camera dofs: a unit pivot and a zero right-hand side; their Jacobian columns are zero already)"""
    oc, op = np.asarray(obs_cam, np.int64), np.asarray(obs_pt, np.int64)
    cf = np.asarray(cam_fixed).reshape(-1, 6) != 0
    dc, dp = np.asarray(dc, float).reshape(n_cams, 6), np.asarray(dp, float).reshape(n_pts, 3)
    keep = [j for j in range(n_pts) if not left_out[j]]
    pos = {j: 6 * n_cams + 3 * t for t, j in enumerate(keep)}
    n = 6 * n_cams + 3 * len(keep)
    H, g = mp.zeros(n, n), mp.zeros(n, 1)
    for i in range(len(oc)):
        cols = list(range(6 * oc[i], 6 * oc[i] + 6)) + (list(range(pos[op[i]], pos[op[i]] + 3)) if op[i] in pos else [])
        J = np.concatenate([mpa(Jc[i]), mpa(Jp[i])], 1)[:, :len(cols)]
        Hb, gb = J.T.dot(J), J.T.dot(mpa(r[i]))
        for x, cx in enumerate(cols):
            g[cx] -= gb[x]
            for y, cy in enumerate(cols):
                H[cx, cy] += Hb[x, y]
    for a in range(n_cams):
        for q in range(6):
            H[6 * a + q, 6 * a + q] += mp.mpf(1) if cf[a, q] else mp.mpf(float(dc[a, q]))
    for j in keep:
        for q in range(3):
            H[pos[j] + q, pos[j] + q] += mp.mpf(float(dp[j, q]))
    x = mp.lu_solve(H, g)
    dxc = np.array([float(x[i]) for i in range(6 * n_cams)])
    dxp = np.zeros((n_pts, 3))
    for j in keep:
        dxp[j] = [float(x[pos[j] + q]) for q in range(3)]
    return dxc, dxp
