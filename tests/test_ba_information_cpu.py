"""CPU leg of bundle adjustment's information matrices: the reference of the GPU tests (tests/ba_information_ref.py) against itself,
and the properties of its inputs that those tests lean on -- conditions asserted here, not measurements."""
import importlib

import numpy as np
import pytest

import ba_information_ref as I
import ba_loss_ref as B
import lm_step_ref as L

K = 3


# ------------------------------------------------------------------------------- the reference against itself
@pytest.mark.parametrize("name", [None, "mixed"])
@pytest.mark.parametrize("sname", ["A", "B"])
def test_identity_weights_reproduce_the_robust_problem_bit_for_bit(sname, name):
    s = B.scene(sname)
    n = len(s["obs_cam"])
    table = I.trivial_table(n) if name is None else B.loss_table(sname, name, n)
    p0 = B.RobustBAProblem(s, table)
    for W in (None, np.broadcast_to(np.eye(2), (n, 2, 2))):
        p1 = I.WeightedBAProblem(s, W, None if name is None else table)
        a, b = p0.lin(p0.x0), p1.lin(p1.x0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert p0.cost(p0.x0) == p1.cost(p1.x0) and np.array_equal(p0.s_of(p0.x0), p1.s_of(p1.x0))
    if name is None:                                   # ... and without a loss the lossless problem
        pl = L.ba_problem(s)
        assert np.array_equal(pl.lin(pl.x0)[1], p1.lin(p1.x0)[1]) and abs(pl.cost(pl.x0) - p1.cost(p1.x0)) <= 1e-15 * pl.cost(pl.x0)


@pytest.mark.parametrize("name", [None, "huber", "cauchy"])
@pytest.mark.parametrize("family", ["mild", "wide"])
def test_the_whitened_pair_is_the_gradient_of_the_whitened_cost(family, name):
    """central differences of 1/2 sum rho(|W r|^2) along random tangent directions against J'^T r' (for rho'' <= 0 losses -- Huber,
    Cauchy -- and without one the corrected pair gives the exact gradient)"""
    prob = I.problem("A", name, family)
    r, J, cols = prob.lin(prob.x0)
    g = np.zeros(prob.n_local)
    np.add.at(g, cols, np.einsum("nki,nk->ni", J, r))
    rng = np.random.default_rng(4)
    worst = 0.0
    for _ in range(4):
        d = rng.standard_normal(prob.n_local) * prob.free                # (plus leaves a constant rotation alone)
        d /= np.linalg.norm(d)
        h = 1e-6
        fd = (prob.cost(prob.plus(prob.x0, h * d)) - prob.cost(prob.plus(prob.x0, -h * d))) / (2 * h)
        worst = max(worst, abs(fd - g @ d) / np.linalg.norm(g))
    print(f"  {family} {name}: central difference against J'^T r', worst {worst:.2e} of |g|")
    assert worst <= 1e-6
    W = prob.W
    s = prob.s_of(prob.x0)
    cams, pts = prob.split(prob.x0)
    ro = prob.lin_obs(cams, pts, False)[0]
    assert np.allclose(s, np.einsum("ni,nij,nj->n", ro, I.information_of(W), ro), rtol=1e-12)      # s = r^T Omega r


def test_the_families_and_the_50_digit_factor():
    import mpmath as mp
    for family, (slo, shi, thi) in {"mild": (0.7, 1.4, 2.0), "wide": (0.1, 10.0, 100.0)}.items():
        W = I.weights(family, 500, seed=1)
        Om = I.information_of(W)
        sv = np.linalg.svd(W, compute_uv=False)
        assert sv[:, 1].min() >= slo * (1 - 1e-12) and (sv[:, 0] / sv[:, 1]).max() <= thi * (1 + 1e-12) and sv[:, 1].max() <= shi * (1 + 1e-12)
        assert np.array_equal(Om[:, 0, 1], Om[:, 1, 0]) and not I.is_identity(W).any()
        Wc = np.array([[float(x) for x in row] for row in I.chol2_mp(Om)]).reshape(-1, 2, 2)
        assert np.allclose(np.einsum("nki,nkj->nij", Wc, Wc), Om, rtol=1e-13, atol=1e-13 * np.abs(Om).max())
        assert np.all(Wc[:, 1, 0] == 0) and not np.allclose(Wc, W)           # Rot(phi) dropped out
    Om, kap = I.ill_conditioned(354)
    ev = np.linalg.eigvalsh(Om)
    assert kap.max() == 1e12 and np.all(ev[:, 0] > 0) and np.allclose(ev[:, 1] / ev[:, 0], kap, rtol=1e-3)
    assert I.chol2_mp(np.array([[[1.0, 2.0], [2.0, 1.0]]]))[0] is None and I.chol2_mp(np.array([[[1.0, 1.0], [1.0, 1.0]]]))[0] is None
    # the factor of a numpy Cholesky, seen through factor_error: a well-conditioned matrix is within the bound
    Om = I.information_of(I.weights("mild", 50, seed=2))
    assert I.factor_error(np.linalg.cholesky(Om).transpose(0, 2, 1), Om) <= 4.0
    with mp.workdps(50):
        w = I.chol2_mp(np.array([[[4.0, 2.0], [2.0, 10.0]]]))[0]
        assert [float(x) for x in w] == [2.0, 1.0, 0.0, 3.0]


# ------------------------------------------------------------------------------- conditions of the solve cases
@pytest.mark.parametrize("case", list(I.LM_CASES))
def test_lm_cases_are_accuracy_cases(case):
    sname, name, ok = I.SOLVE_CASES[case]
    o = L.lm_options(**ok)
    for k in (1, K):
        ref = I.reference(case, k)
        kap = max(it["kappa"] for it in ref)
        print(f"  {case} k={k}: kappa {kap:.2e}, accepted {[it['accepted'] for it in ref]}")
        assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6 and L.rho_margin_ok(ref, o)
    assert len(I.LM_CASES) >= 4


@pytest.mark.parametrize("case", list(I.DOGLEG_CASES))
def test_dogleg_cases_are_accuracy_cases(case):
    sname, name, ok = I.SOLVE_CASES[case]
    o = L.lm_options(**ok)
    for k in (1, K):
        ref = I.reference(case, k, "dogleg")
        kap = max(it["kappa"] for it in ref)
        print(f"  {case} k={k}: kappa {kap:.2e}, dogleg cases {[it['case'] for it in ref]}")
        assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6 and L.rho_margin_ok(ref, o)
    assert len(I.DOGLEG_CASES) >= 4 and {I.SOLVE_CASES[c][0] for c in I.DOGLEG_CASES} == {"M", "B"}


def test_the_weights_change_the_problem():
    """the mild family is no near-identity: the weighted start cost and first step differ from the unweighted ones by far more than
    any bound of the GPU comparison"""
    for case in ("A_none", "B_none"):
        sname, _, ok = I.SOLVE_CASES[case]
        ref = I.reference(case, 1)
        plain = L.lm_reference(L.ba_problem(B.scene(sname)), L.lm_options(**ok), 1)
        assert abs(ref[0]["start"]["cost"] / plain[0]["start"]["cost"] - 1) > 0.1
        assert np.linalg.norm(ref[0]["delta"] - plain[0]["delta"]) > 1e-3 * np.linalg.norm(plain[0]["delta"])


# ------------------------------------------------------------------------------- the Python layer, without a device
def test_python_weight_shapes():
    st = importlib.import_module("slam-tricks_amd")
    e = object.__new__(st.BAEngine)
    e.no = 5
    assert np.array_equal(e._weight_array(4.0, "information"), np.tile([4.0, 0, 0, 4.0], (5, 1)))
    w = np.arange(1.0, 6.0)
    assert np.array_equal(e._weight_array(w, "information"), np.stack([w, 0 * w, 0 * w, w], 1))
    M = np.array([[1.0, 2.0], [3.0, 4.0]])
    assert np.array_equal(e._weight_array(M, "information"), np.tile([1.0, 2, 3, 4], (5, 1)))
    Ms = np.arange(20.0).reshape(5, 2, 2)
    out = e._weight_array(Ms, "sqrt_information")
    assert np.array_equal(out, Ms.reshape(5, 4)) and out.flags["C_CONTIGUOUS"] and out.dtype == np.float64
    for bad, word in ((np.ones(4), "length 5"), (np.ones((4, 2, 2)), "(5, 2, 2)"), (np.ones((5, 4)), "(5, 2, 2)")):
        with pytest.raises(ValueError, match="information") as err:
            e._weight_array(bad, "information")
        assert word in str(err.value)
    for name in ("stba_ba_set_information", "stba_ba_set_sqrt_information", "stba_ba_has_information", "stba_ba_get_sqrt_information"):
        assert name in st.EXPORTS
