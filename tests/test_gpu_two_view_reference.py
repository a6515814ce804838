"""The two-view initialiser on the device (csrc/two_view.hip, stba_two_view_init) against the 50-digit reference of
tests/two_view_ref.py: F at the sizes where the reduction changes path, the pose, the cheirality counts, degenerate inputs
and reproducibility.  tests/test_two_view.py (device against the numpy oracle, at 1e-7) stays as it is.

Unit of every bound on F and the pose: u = EPS sigma_1 / sigma_8 of the case's own n x 9 system, the first-order perturbation
bound of its null vector.  F is held to 64 u (a ceiling for a backward-stable reduction: each entry meets about 30 rotations --
the rows of its lane, 7 levels of the tree, 9 columns -- and the 9 x 9 Jacobi follows), and each case first shows that
EPS (sigma_1 / sigma_8)^2, where a normal-equations method lands, lies 100 times above that.

`python tests/test_gpu_two_view_reference.py` prints, without a device, what the numpy oracle (oracle/two_view_np.py: the same
double arithmetic with LAPACK) reaches in the same units (with the argument `tri`: the fixture and the oracle's figures of the triangulation test); the
constants of the pose and triangulation tests were set from those runs."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import two_view_cases as TC  # noqa: E402
import two_view_ref as TR  # noqa: E402

EPS = TR.EPS
C_F = 64.0                       # derived, see above
# Pose: the numpy oracle's worst max(|R - R_ref|, |t - t_ref|) over the 22 cases of (a) and the three noisy cases is 1.84e-3 u
# (case n512, 7.5e-15 as an absolute figure; the others lie between 1.8e-5 u and 1.3e-3 u), measured on the host by this
# file's main(); 8 x that for one-sided Jacobi in place of LAPACK.  The bound is 2.7e-13 at n = 8 and below 5e-14 elsewhere
C_POSE_ORACLE = 1.84e-3
C_POSE = 8 * C_POSE_ORACLE
NO_SOLUTION = -8                 # STBA_ERR_NO_SOLUTION, include/stba.h

# 0.01 px of pixel noise.  Two things only these cases can show: s3 of E lies far above the 1e-12 switch of svd3 (the Jacobi
# branch), and F depends on EVERY row -- in the noise-free cases any rows of rank 8 have the same null vector, so a merge that
# loses a lane's or a block's rows goes unseen there, while here it moves F by thousands of u (1 block, 2 blocks, 10 blocks)
NOISY = ["n300-noise", "n513-noise", "n5000-noise"]
_noisy = {}


def _case(cid):
    if cid in NOISY:
        if not _noisy:
            _noisy.update(TC.scenes.two_view_pairs(n_pts=5000, seed=22, pix_noise=0.01))
        n = int(cid[1:].partition("-")[0])
        return dict(f1=_noisy["f1"][:n], f2=_noisy["f2"][:n], K=_noisy["K"], cam="noise", n=n)
    return TC.f_case(cid)


class Reference:
    """built once per module: the Gram matrix of every case is a prefix sum of one of three accumulations"""

    def __init__(self):
        s = TC.base()
        self.gram = {"K1": TR.GramPrefix(s["f1"], s["f2"], TC.SIZES), "K2": TR.GramPrefix(s["g1"], s["g2"], TC.VARIANT_SIZES)}
        c = _case(NOISY[-1])
        self.gram["noise"] = TR.GramPrefix(c["f1"], c["f2"], [300, 513, 5000])
        self._f, self._pose = {}, {}

    def F(self, c):
        """(F as 9 doubles, u = EPS s1 / s8, s1 / s8, the 9 mpf of F)"""
        key = (c["cam"], c["n"])
        if key not in self._f:
            F, sig = self.gram[c["cam"]].at(c["n"])
            k = float(sig[0] / sig[7])
            self._f[key] = (TR.f64(F), EPS * k, k, F)
        return self._f[key]

    def pose(self, c):
        """(R, t) of the reference pipeline run from the reference's F.  The four hypotheses differ in the sign of a depth
        at EVERY point of a valid scene, so the first eight correspondences name the winner"""
        key = (c["cam"], c["n"])
        if key not in self._pose:
            H = TR.essential_hypotheses(self.F(c)[3], c["K"])
            fails = TR.fail_counts(TR.cheirality(c["f1"][:8], c["f2"][:8], H["hyps"], c["K"]))
            assert sorted(fails)[:2] == [0, 8] or fails.count(0) == 1, fails
            R, t = H["hyps"][fails.index(0)]
            self._pose[key] = (TR.f64(R), TR.f64(t))
        return self._pose[key]


def err_up_to_sign(F, Fref):
    F = np.asarray(F).reshape(-1)
    return np.abs(np.sign(F @ Fref) * F - Fref).max()


def svd3_branch(F, K):
    """s3 / s1 of E = K^T F K and the branch of svd3 that it implies (small_linalg.hpp switches at 1e-12)"""
    s = np.linalg.svd(K.T @ np.asarray(F).reshape(3, 3) @ K, compute_uv=False)
    return s[2] / s[0], "Jacobi" if s[2] > 1e-12 * s[0] else "cross-product"


# ---------------------------------------------------------------- device tests
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    return importlib.import_module("slam-tricks_amd")


@pytest.fixture(scope="module")
def ref():
    return Reference()


def raw_call(st, f1, f2, K):
    """stba_two_view_init through ctypes: the status and every output, whatever the status (the wrapper raises instead)"""
    f1, f2, K = (np.ascontiguousarray(a, dtype=np.float64) for a in (f1, f2, K))
    n = len(f1)
    F = np.zeros((3, 3)); R = np.zeros((3, 3)); t = np.zeros(3); pts = np.zeros((n, 3))
    fails = np.full(4, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    code = st.lib().stba_two_view_init(n, p(f1), p(f2), p(K), p(F), p(R), p(t), p(pts), fails.ctypes.data_as(C.POINTER(C.c_int)),
                                       C.c_void_p(0))
    return code, dict(F=F, R=R, t=t, pts=pts, fails=fails)


def check_F(st, ref, cid):
    c = _case(cid)
    Fref, u, kappa, _ = ref.F(c)
    # the precondition: a method that squares the condition number must land at least 100 tolerances away
    assert EPS * kappa ** 2 >= 100 * C_F * u, f"{cid}: sigma_1 / sigma_8 = {kappa:.3g} does not separate the two methods"
    g = st.two_view_init(c["f1"], c["f2"], c["K"])
    err = err_up_to_sign(g["F"], Fref)
    print(f"{cid}: F error {err / u:.3g} u  (u = EPS s1/s8 = {u:.3g}, s1/s8 = {kappa:.3g})")
    assert err <= C_F * u, f"{cid}: F is {err / u:.3g} u from the reference, allowed {C_F} u (u = {u:.3g})"
    return c, g, u


@pytest.mark.parametrize("cid", TC.f_case_ids() + NOISY)
def test_F_against_the_reference(st, ref, cid):
    check_F(st, ref, cid)


@pytest.mark.parametrize("cid", TC.f_case_ids() + NOISY)
def test_pose_against_the_reference(st, ref, cid):
    c = _case(cid)
    _, u, _, _ = ref.F(c)
    Rr, tr = ref.pose(c)
    g = st.two_view_init(c["f1"], c["f2"], c["K"], points=False)
    ratio, branch = svd3_branch(g["F"], c["K"])
    err = max(np.abs(g["R"] - Rr).max(), np.abs(g["t"] - tr).max())
    print(f"{cid}: pose error {err / u:.3g} u = {err:.3g}; s3/s1 of E = {ratio:.3g} -> {branch} branch of svd3")
    assert branch == ("Jacobi" if cid in NOISY else "cross-product")
    assert err <= C_POSE * u, f"{cid}: pose is {err / u:.3g} u from the reference, allowed {C_POSE:.3g} u (u = {u:.3g})"


# ---------------------------------------------------------------- (c) triangulation, point by point
N_TRI = [255, 256, 257, 1000]
# the added points for which the reference and the numpy oracle disagree on a cheirality flag of some hypothesis (found on the
# host by main(); at most 10 % of the added points may be listed)
DROPPED = ()
# the numpy oracle's worst |X - X_ref| / (EPS sigma_1 / sigma_3 |X_ref|) over the points of the four cases, measured on the host
# by `main tri`: 164 (n = 255, an added point at 1e4 baselines; 83 to 145 in the other three cases, always at such a point, and
# none of the 32 added points had to be dropped); 8 x that for the one-sided Jacobi in registers in place of LAPACK
C_TRI_ORACLE = 164.0
C_TRI = 8 * C_TRI_ORACLE


def _added_points():
    """correspondences added to the st22 cloud, projected at 50 digits and rounded, so that they agree with its F:
    low parallax (depths of 1e2, 1e3 and 1e4 baselines), camera 1's optical axis (u1 = cx and v1 = cy: exact zeros in the
    DLT rows) and pixels within 1 px of camera 1's image border.  All lie in front of both cameras"""
    s = TC.base()
    R, t, K = s["R_true"], s["t_true"], s["K"]
    rng = np.random.default_rng(7)
    b = float(np.linalg.norm(t))
    X = []
    for depth in (1e2 * b, 1e3 * b, 1e4 * b):
        X += [np.array([depth * rng.uniform(0.1, 0.6), depth * rng.uniform(-0.3, 0.3), depth]) for _ in range(6)]
    X += [np.array([0.0, 0.0, z]) for z in (3.0, 4.0, 5.5, 7.0, 8.0, 10.0)]
    for u, v in [(0.4, 120.0), (0.9, 310.0), (598.3, 77.0), (598.9, 250.0), (150.0, 0.6), (420.0, 0.2), (333.0, 398.5), (75.0, 398.1)]:
        z = rng.uniform(4.0, 9.0)
        X.append(np.array([z * (u - K[0, 2]) / K[0, 0], z * (v - K[1, 2]) / K[1, 1], z]))
    X = np.array(X)
    assert np.all(X[:, 2] > 0) and np.all(((X - t) @ R)[:, 2] > 0.05 * np.linalg.norm(X, axis=1))
    f1 = np.array([[float(c) for c in TR.project(K, np.eye(3), np.zeros(3), x)] for x in X])
    f2 = np.array([[float(c) for c in TR.project(K, R, t, x)] for x in X])
    return f1, f2


def _tri_case(n, dropped=DROPPED):
    """the first n st22 correspondences, the kept added points written over places 2, 7, 12, ... (all below 255)"""
    s = TC.base()
    f1, f2 = s["f1"][:n].copy(), s["f2"][:n].copy()
    a1, a2 = _added_points()
    keep = [j for j in range(len(a1)) if j not in dropped]
    assert len(a1) - len(keep) <= len(a1) // 10
    idx = [5 * k + 2 for k in range(len(keep))]
    f1[idx], f2[idx] = a1[keep], a2[keep]
    return f1, f2, s["K"], idx


def _tri_ratios(f1, f2, K, R, t, pts):
    """per point |X - X_ref| / (EPS sigma_1 / sigma_3 |X_ref|), X_ref the 50-digit DLT of the SAME cameras (R, t, K)"""
    T = TR.Triangulator(np.asarray(R), np.asarray(t), K)
    out = np.zeros(len(f1))
    for i in range(len(f1)):
        Xr, sig = T.point(f1[i], f2[i])
        Xr = TR.f64(Xr)
        out[i] = np.linalg.norm(pts[i] - Xr) / (EPS * float(sig[0] / sig[2]) * np.linalg.norm(Xr))
    return out


@pytest.mark.parametrize("n", N_TRI)
def test_triangulation_point_by_point(st, n):
    f1, f2, K, idx = _tri_case(n)
    g = st.two_view_init(f1, f2, K)
    assert all(np.all(np.isfinite(g[k])) for k in ("F", "R", "t", "pts"))
    r = _tri_ratios(f1, f2, K, g["R"], g["t"], g["pts"])
    w = int(np.argmax(r))
    print(f"n = {n}: worst point {w} ({'added' if w in idx else 'st22'}) at {r[w]:.3g}, added points at most {r[idx].max():.3g}, "
          f"allowed {C_TRI:.3g}  [units of EPS s1/s3 |X|]")
    assert r.max() <= C_TRI, f"point {w}: {r[w]:.3g} > {C_TRI:.3g}"


# ---------------------------------------------------------------- (d) cheirality counts
def _behind_scene(n, k_random, seed):
    """the st22 scene with correspondences replaced by projections of points BEHIND camera 1 (even picks) or behind camera 2
    (odd picks) -- they satisfy the epipolar constraint like every other pair -- at 0, 255, 256 (where n allows), n - 1 and
    a few random places"""
    s = TC.base()
    rng = np.random.default_rng(seed)
    f1, f2 = s["f1"][:n].copy(), s["f2"][:n].copy()
    where = sorted(set([0, 255, n - 1] + ([256] if n > 257 else []) + list(rng.choice(np.arange(1, n - 1), k_random, replace=False))))
    R, t, K = s["R_true"], s["t_true"], s["K"]
    for j, i in enumerate(where):
        p = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), -rng.uniform(4.0, 9.0)])      # behind, in its own camera
        X = p if j % 2 == 0 else R @ p + t
        f1[i] = TC.project(K, np.eye(3), np.zeros(3), X[None])[0]
        f2[i] = TC.project(K, R, t, X[None])[0]
    return f1, f2, K, where


def _reference_counts(f1, f2, K):
    F, _ = TR.fundamental(f1, f2)
    H = TR.essential_hypotheses(F, K)
    ch = TR.cheirality(f1, f2, H["hyps"], K)
    # every depth is far from zero, so that no rounding of the device can turn a flag
    margin = min(min(abs(z1), abs(z2)) / nx for rows in ch for z1, z2, nx in rows)
    assert margin > 1e-6, f"a reference depth is only {float(margin):.3g} |X|"
    return TR.fail_counts(ch)


@pytest.mark.parametrize("n", [256, 257, 1023])
def test_cheirality_counts_with_points_behind_a_camera(st, n):
    f1, f2, K, where = _behind_scene(n, 4, seed=n)
    want = _reference_counts(f1, f2, K)
    code, g = raw_call(st, f1, f2, K)
    print(f"n = {n}: replaced {where}; device counts {sorted(g['fails'])}, reference {sorted(want)}")
    assert code == NO_SOLUTION, code
    assert sorted(int(x) for x in g["fails"]) == sorted(want)
    assert min(want) == len(where)


def test_cheirality_counts_of_a_valid_scene(st):
    n = 256
    s = TC.base()
    want = _reference_counts(s["f1"][:n], s["f2"][:n], s["K"])
    code, g = raw_call(st, s["f1"][:n], s["f2"][:n], s["K"])
    assert code == 0, code
    assert sorted(int(x) for x in g["fails"]) == sorted(want) and sorted(want)[0] == 0 and sorted(want)[1] > 0


# ---------------------------------------------------------------- (e) degenerate inputs
def _degenerate(name):
    K = np.array([[400.0, 0, 300], [0, 400.0, 200], [0, 0, 1]])
    if name == "pure-rotation":                          # the scene of test_oracle_survives_a_degenerate_configuration
        rng = np.random.default_rng(1)
        P = rng.uniform([-2, -2, 4], [2, 2, 9], (60, 3))
        a = 0.2
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        return TC.project(K, np.eye(3), np.zeros(3), P), TC.project(K, R, np.zeros(3), P), K
    s = TC.base()
    if name == "planar":                                 # every landmark on the plane z = 6 of frame 1
        rng = np.random.default_rng(2)
        P = np.concatenate([rng.uniform([-1.5, -1.5], [3.0, 1.5], (80, 2)), np.full((80, 1), 6.0)], 1)
        return TC.project(K, np.eye(3), np.zeros(3), P), TC.project(K, s["R_true"], s["t_true"], P), K
    if name == "eight-twice":
        return np.tile(s["f1"][:8], (2, 1)), np.tile(s["f2"][:8], (2, 1)), K
    if name == "eight-identical":
        return np.tile(s["f1"][:1], (8, 1)), np.tile(s["f2"][:1], (8, 1)), K
    raise KeyError(name)


@pytest.mark.parametrize("name", ["pure-rotation", "planar", "eight-twice", "eight-identical"])
def test_degenerate_input_ends_well_and_leaves_no_state(st, ref, name):
    f1, f2, K = _degenerate(name)
    n = len(f1)
    code, g = raw_call(st, f1, f2, K)
    print(f"{name}: status {code}, counts {g['fails']}")
    assert code in (0, NO_SOLUTION), code
    assert all(0 <= int(k) <= n for k in g["fails"]), g["fails"]
    assert np.all(np.isfinite(g["F"]))
    if code == 0:
        assert np.abs(g["R"] @ g["R"].T - np.eye(3)).max() <= 1e-8 and np.linalg.det(g["R"]) > 0
        assert abs(np.linalg.norm(g["t"]) - 1.0) <= 1e-8
        assert np.count_nonzero(g["fails"] == 0) == 1
    else:
        assert np.count_nonzero(g["fails"] == 0) != 1
    check_F(st, ref, "n129")                            # a valid call right after: nothing carried over


# ---------------------------------------------------------------- (f) reproducibility
@pytest.mark.parametrize("cid", ["n513", "n32769"])
def test_two_calls_give_the_same_bits(st, cid):
    c = _case(cid)
    a = st.two_view_init(c["f1"], c["f2"], c["K"])
    b = st.two_view_init(c["f1"], c["f2"], c["K"])
    for k in ("F", "R", "t", "pts", "fails"):
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- the oracle's figures, on the host
def main():
    import two_view_np as TV
    ref = Reference()
    worst = 0.0
    for cid in TC.f_case_ids() + NOISY:
        c = _case(cid)
        Fref, u, kappa, _ = ref.F(c)
        Fo = TV.fundamental(c["f1"], c["f2"])
        pose, fails = TV.decompose(Fo, c["K"], c["f1"][:8], c["f2"][:8])
        Rr, tr = ref.pose(c)
        ep = max(np.abs(pose[0] - Rr).max(), np.abs(pose[1] - tr).max())
        worst = max(worst, ep / u)
        print(f"{cid}: s1/s8 {kappa:.3g} u {u:.3g}  oracle F {err_up_to_sign(Fo, Fref) / u:.3g} u  pose {ep / u:.3g} u = {ep:.3g}"
              f"  svd3 {svd3_branch(Fo, c['K'])}  bound vs 1e-8: {C_POSE * u:.3g}")
    print(f"worst oracle pose error: {worst:.3g} u")


def main_triangulation():
    """the fixture of (c): which added points to drop, and the oracle's worst ratio"""
    import two_view_np as TV
    f1, f2, K, idx = _tri_case(1000, dropped=())
    F, _ = TR.fundamental(f1, f2)
    H = TR.essential_hypotheses(F, K)
    drop = set()
    for R, t in H["hyps"]:
        T = TR.Triangulator(R, t, K)
        Rd, td = TR.f64(R), TR.f64(t)
        for j, i in enumerate(idx):
            z1, z2 = T.depths(T.point(f1[i], f2[i])[0])
            p1 = TV.triangulate(f1[i], f2[i], np.eye(3), np.zeros(3), Rd, td, K)
            p2 = Rd.T @ p1 - Rd.T @ td
            if (z1 > 0, z2 > 0) != (p1[2] > 0.0, p2[2] > 0.0):
                drop.add(j)
    print(f"added points: {len(idx)}, reference and oracle disagree on a flag at {sorted(drop)}")
    worst = 0.0
    for n in N_TRI:
        f1, f2, K, idx = _tri_case(n, dropped=tuple(sorted(drop)))
        o = TV.two_view_init(f1, f2, K)
        assert o["R"] is not None, o["fails"]
        r = _tri_ratios(f1, f2, K, o["R"], o["t"], o["pts"])
        worst = max(worst, r.max())
        print(f"n = {n}: oracle worst ratio {r.max():.3g} (point {int(np.argmax(r))}), added points {r[idx].max():.3g}")
    print(f"worst oracle triangulation ratio: {worst:.3g}")


if __name__ == "__main__":
    main_triangulation() if "tri" in sys.argv[1:] else main()
