"""CPU leg of bundle adjustment's robust losses: the inputs of the GPU tests (tests/ba_loss_ref.py) have the properties those tests
lean on -- they are conditions asserted here, not measurements --, the numpy corrector agrees with a 50-digit one on the BA inputs
(the measured figure behind the evaluate bound's c), the corrected pair is the gradient of 1/2 sum rho, and the Python layer builds the
per-observation table without a device."""
import importlib

import numpy as np
import pytest

import ba_loss_ref as B
import dogleg_ref as D
import lm_step_ref as L
import pg_loss_ref as G

K = 3


def s_at_start(sname):
    p = L.ba_problem(B.scene(sname))
    r = p.lin(p.x0, False)[0]
    return np.sum(r * r, 1)


# ------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("sname", ["A", "B"])
def test_loss_sets_cover_every_branch_at_the_start(sname):
    s = s_at_start(sname)
    n = len(s)
    assert n == {"A": 139, "B": 708}[sname] and len(B.scene(sname)["cams0"]) == 10
    print(f"{sname}: {n} observations, sqrt(s) median {np.median(np.sqrt(s)):.4f} max {np.sqrt(s.max()):.3f}")
    assert abs(np.median(np.sqrt(s)) - {"A": 0.032, "B": 0.015}[sname]) < 1e-3
    for name in B.LOSS_SETS:
        t = B.loss_table(sname, name, n)
        has = t["kind"] != 0
        beyond = float(np.mean(s[has] > B.threshold(t)[has]))
        print(f"  {name}: {beyond:.2f} of the observations with a threshold lie beyond it")
        assert 0.2 <= beyond <= 0.8
    assert np.all(B.loss_table(sname, "huber", n)["a"] == {"A": 0.03, "B": 0.015}[sname])
    t = B.loss_table(sname, "tolerant", n)
    x = (s - t["a"]) / t["b"]
    print(f"  tolerant: {np.mean(x > G.TOLERANT_LINEAR):.2f} on the linear branch")
    assert 1 <= np.sum(x > G.TOLERANT_LINEAR) < n
    rh, _, _, k = G.factors(t, s)
    assert np.sum(k != 0) >= 5 and np.all(rh[2] >= 0)                    # the second corrector branch runs (rho'' > 0)
    t = B.loss_table(sname, "tukey", n)
    assert np.any(G.rho(t["kind"], t["a"], t["b"], t["scale"], s)[1] == 0.0)      # observations of weight zero
    t = B.loss_table(sname, "mixed", n)
    assert set(t["kind"].tolist()) == set(range(7)) and np.any(t["scale"] != 1.0)
    assert np.any(G.untouched(t)) and np.any((t["kind"] == 0) & (t["scale"] != 1.0))
    if sname == "A":
        sc = B.scene("A")
        assert sc["cam_fixed"].any() and sc["pt_fixed"].any() and not np.any(sc["obs_cam"] == len(sc["cams0"]) - 1)
    else:                                                             # the second tile of the correcting kernel sees every kind too
        assert set(t["kind"][512:].tolist()) == set(range(7))


def test_scene_c_has_more_than_two_tiles():
    n = len(B.scene("C")["obs_cam"])
    assert n > 2 * 512 and n % 512 != 0, n


def test_idle_cameras_observe_nothing():
    s = B.scene("A")
    d = B.with_idle_cameras(s, 25)
    assert len(d["cams0"]) == 25 == len(d["cam_fixed"]) and d["obs_cam"].max() < len(s["cams0"])
    assert np.array_equal(d["cams0"][:len(s["cams0"])], s["cams0"])


# ------------------------------------------------------------------------------- the numpy reference
def test_numpy_losses_match_the_50_digit_ones():
    """the measured figure behind ba_loss_ref.RHO_EPS (and so behind the c of the GPU evaluate bound), by DESIGN.md 7g's recipe on the BA
    inputs: over the s of every loss set at the start points of A and B, the worst relative error of rho' and rho'' per kind in units
    of eps; and rho where it matters, in the summed cost"""
    worst = {k: 0.0 for k in B.KINDS}
    worst_cost = 0.0
    for sname in "AB":
        s = s_at_start(sname)
        for name in B.LOSS_SETS:
            t = B.loss_table(sname, name, len(s))
            got = G.rho(t["kind"], t["a"], t["b"], t["scale"], s)
            total = 0
            for e in range(len(s)):
                want = G.rho_mp(int(t["kind"][e]), t["a"][e], t["b"][e], t["scale"][e], s[e])
                total = total + want[0]
                for q in (1, 2):
                    if float(want[q]) == 0.0:
                        assert got[q][e] == 0.0
                        continue
                    rel = abs(float((got[q][e] - want[q]) / want[q])) / L.EPS
                    kn = B.KINDS[int(t["kind"][e])]
                    worst[kn] = max(worst[kn], rel)
            worst_cost = max(worst_cost, abs(float((float(np.sum(got[0].astype(L.LD))) - total) / total)))
    print("worst |numpy - 50 digits| / (eps |value|) of rho', rho'' per kind: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    print(f"worst relative error of sum rho: {worst_cost:.2e}")
    assert worst_cost <= 1e-13
    for k, v in worst.items():
        assert v <= B.RHO_EPS[k], (k, v)
        assert B.c_of(B.KINDS.index(k))[0] == 8.0 * B.RHO_EPS[k] + 16.0


@pytest.mark.parametrize("name", B.LOSS_SETS)
def test_corrector_against_50_digits(name):
    """r' and J' of the numpy corrector against the corrector evaluated at 50 digits from the same FP64 r and J, on scene A: within
    c eps of the terms it is made of (the share of the evaluate bound that is the corrector's)"""
    import mpmath as mp
    prob = B.problem("A", name)
    cams, pts = prob.split(prob.x0)
    r, Jc, Jp = prob.lin_obs(cams, pts)
    rc, Jcc, Jpc, _ = prob.lin_obs_corrected(cams, pts)
    t = prob.table
    J, Jx = np.concatenate([Jc, Jp], 2), np.concatenate([Jcc, Jpc], 2)
    c = B.c_of(t["kind"])
    worst = 0.0
    with mp.workdps(50):
        for e in range(len(r)):
            if G.untouched(t)[e]:
                assert np.array_equal(rc[e], r[e]) and np.array_equal(Jx[e], J[e])
                continue
            r0, r1 = mp.mpf(float(r[e, 0])), mp.mpf(float(r[e, 1]))
            s = r0 * r0 + r1 * r1
            # (the branch is taken at the FP64 s, as every implementation takes it)
            rho = G.rho_mp(int(t["kind"][e]), t["a"][e], t["b"][e], t["scale"][e], float(np.sum(r[e] * r[e])))
            sq = mp.sqrt(rho[1])
            if s != 0 and rho[2] > 0:
                alpha = 1 - mp.sqrt(1 + 2 * s * rho[2] / rho[1])
                rs, k = sq / (1 - alpha), alpha / s
            else:
                rs, k = sq, mp.mpf(0)
            for a, ra in enumerate((r0, r1)):
                want = rs * ra
                worst = max(worst, abs(float(rc[e, a] - want)) / max(c[e] * L.EPS * abs(float(want)), 1e-300))
            for col in range(9):
                j0, j1 = mp.mpf(float(J[e, 0, col])), mp.mpf(float(J[e, 1, col]))
                tt = k * (r0 * j0 + r1 * j1)
                for a, (ra, ja) in enumerate(((r0, j0), (r1, j1))):
                    want = sq * (ja - ra * tt)
                    # (the terms the entry is made of: J, and r k (r^T J) with the two products of r^T J taken by magnitude; and the
                    # column it mixes: alpha = 1 - sqrt(D) has an absolute error of eps, so k = alpha / s one of eps / s, which
                    # r_a r_b / s <= 1 carries from the column's other entry into this one)
                    scale = float(sq) * (abs(float(j0)) + abs(float(j1)) + abs(float(ra * k)) * (abs(float(r0 * j0)) + abs(float(r1 * j1))))
                    worst = max(worst, abs(float(Jx[e, a, col] - want)) / max(c[e] * L.EPS * scale, 1e-300))
    print(f"A {name}: worst |numpy - 50 digits| / (c eps |terms|) = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("sname,name", [("A", n) for n in B.LOSS_SETS] + [("B", "mixed")])
def test_corrected_pair_is_the_gradient_of_the_robust_cost(sname, name):
    """J'^T r' (constant columns included: the reference drops them later) against central differences of 1/2 sum rho along every
    tangent direction; observations within 2 h |J| of a kink (Huber's and Tukey's a^2, Tolerant's switch) make the difference
    quotient wrong by O(h), so the comparison is 1e-5 of the gradient's largest entry"""
    prob = B.problem(sname, name)
    x = prob.x0
    rc, Jx, cols = prob.lin(x)
    g = np.zeros(prob.n_local)
    np.add.at(g, cols.reshape(-1), np.einsum("nkc,nk->nc", Jx, rc).reshape(-1))
    rng = np.random.default_rng(3)
    idx = rng.choice(np.flatnonzero(prob.free), 40, replace=False)       # (plus() does not move a constant rotation)
    h = 1e-6
    fd = np.zeros(len(idx))
    for q, i in enumerate(idx):
        d = np.zeros(prob.n_local); d[i] = h
        fd[q] = (prob.cost(prob.plus(x, d)) - prob.cost(prob.plus(x, -d))) / (2 * h)
    err = np.abs(fd - g[idx]).max() / np.abs(g).max()
    print(f"{sname} {name}: |central difference - J'^T r'| / |g|max = {err:.2e}")
    assert err <= 1e-5


# ------------------------------------------------------------------------------- the solve cases
@pytest.mark.parametrize("case,strategy", [(c, "lm") for c in B.LM_CASES] + [(c, "dogleg") for c in B.DOGLEG_CASES])
def test_solve_cases_are_accuracy_cases(case, strategy):
    sname, name, ok = B.SOLVE_CASES[case]
    o = L.lm_options(**ok)
    ref = B.reference(case, K, strategy)
    kap = max(it["kappa"] for it in ref)
    print(f"{case} {strategy}: kappa {kap:.2e}, cost {ref[0]['start']['cost']:.6e} -> {ref[-1]['cost']:.6e}, "
          f"rho {[round(it['rho'], 3) for it in ref]}, accepted {[it['accepted'] for it in ref]}")
    assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6
    assert L.rho_margin_ok(ref, o, 1e-2)
    assert ref[-1]["cost"] < ref[0]["start"]["cost"]
    prob = B.problem(sname, name)
    rc = prob.lin(prob.x0, False)[0]
    assert abs(0.5 * np.sum(rc * rc) - ref[0]["start"]["cost"]) > 1e-3 * ref[0]["start"]["cost"]      # 1/2 |r'|^2 is not the cost


def test_scene_m_carries_the_masks_of_a():
    s = B.scene("M")
    prob = L.ba_problem(s)
    assert s["pt_fixed"].sum() == 3 and not np.any(s["obs_cam"] == len(s["cams0"]) - 1)
    assert sorted(s["cam_fixed"].sum(1).tolist()).count(3) == 2 and sorted(s["cam_fixed"].sum(1).tolist()).count(1) == 2
    r = prob.lin(prob.x0, False)[0]
    ss = np.sum(r * r, 1)
    for name in B.SOLVE_SETS:
        t = B.loss_table("M", name, len(ss))
        assert 0.2 <= np.mean(ss > B.threshold(t)) <= 0.8, name


@pytest.mark.parametrize("case", B.DOGLEG_LOOSE_CASES)
def test_loose_dogleg_cases_keep_their_decisions_clear(case):
    """no accuracy cases (kappa 1e10 and more), compared at their own kappa: the decisions must not hang on rounding all the same"""
    o = L.lm_options(**B.SOLVE_CASES[case][2])
    ref = B.reference(case, K, "dogleg")
    kap = max(it["kappa"] for it in ref)
    print(f"{case}: kappa {kap:.2e}, rho {[round(it['rho'], 3) for it in ref]}, cases {[it['case'] for it in ref]}")
    assert L.rho_margin_ok(ref, o, 1e-2) and all(it["valid"] and it["escalations"] == 0 for it in ref)
    assert all(min(abs(it["rho"] - 0.25), abs(it["rho"] - 0.75)) > 1e-2 for it in ref)


def test_the_dogleg_loop_is_dogleg_refs_on_a_lossless_problem():
    """ba_loss_ref.dogleg_reference repeats dogleg_ref.dogleg_reference's loop with one difference, where the start cost comes from:
    on a problem without a loss the two must agree in every bit of every iteration (they may not drift apart)"""
    for sk, ok in ((dict(n_lm=33, seed=12, pts_jitter=3.0), dict(initial_trust_region_radius=1.0)), (dict(n_lm=33, extras=True), dict())):
        prob = L.ba_problem(L.ba_scene(**sk))
        o = L.lm_options(**ok)
        a, b = D.dogleg_reference(prob, o, 6), B.dogleg_reference(prob, o, 6)
        assert any(not it["accepted"] for it in a) or sk.get("extras")
        for ia, ib in zip(a, b):
            for key in ("delta", "x", "x_trial", "z"):
                assert np.array_equal(ia[key], ib[key]), key
            for key in ("cost", "trial_cost", "cost_change", "model_change", "rho", "step_norm", "x_norm", "gmax", "radius", "radius_before",
                        "accepted", "kappa", "case", "beta", "z_norm", "mu", "reused", "escalations", "valid"):
                assert ia[key] == ib[key], (key, ia[key], ib[key])


def test_reject_case_holds_a_rejected_step():
    s, table, o = B.reject_case()
    ref = B.reject_reference(K)
    kap = max(it["kappa"] for it in ref)
    print(f"reject: kappa {kap:.2e}, rho {[round(it['rho'], 3) for it in ref]}, accepted {[it['accepted'] for it in ref]}")
    assert any(not it["accepted"] for it in ref) and any(it["accepted"] for it in ref)
    assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6 and L.rho_margin_ok(ref, o, 1e-2)
    p = L.ba_problem(s)
    r = p.lin(p.x0, False)[0]
    assert 0.2 <= np.mean(np.sum(r * r, 1) > B.REJECT_HUBER_A ** 2) <= 0.8


def test_the_robust_reference_resists_outliers():
    s, bad = B.outlier_scene()
    assert len(bad) == round(0.1 * len(s["obs_cam"])) and len(set(s["obs_pt"][bad].tolist())) == len(bad)
    assert np.all(np.bincount(s["obs_pt"])[s["obs_pt"][bad]] >= 3)
    x_l2, x_rob, cost, table = B.outlier_references()
    prob = L.ba_problem(s)
    d_l2, d_rob = B.distance_to_truth(prob, s, x_l2), B.distance_to_truth(prob, s, x_rob)
    print(f"outliers: |x - truth| L2 {d_l2:.4f}, Cauchy {d_rob:.4f}; robust cost {cost:.6e}")
    assert d_rob < 0.5 * d_l2


# ------------------------------------------------------------------------------- the Python layer
def test_table_helper_takes_the_spec_forms():
    st = importlib.import_module("slam-tricks_amd")
    n = 5
    k, a, b, sc = st.pg_loss_table(n, "huber", 0.03, who="BAEngine", what="observation")
    assert k.dtype == np.int32 and np.all(k == 1) and np.all(a == 0.03) and np.all(b == 1.0) and np.all(sc == 1.0)
    k, a, b, sc = st.pg_loss_table(n, ["huber", None, "tukey", 5, "cauchy"], np.arange(1.0, 6.0), 0.5, [1, 2, 3, 4, 5])
    assert k.tolist() == [1, 0, 6, 5, 3] and np.all(b == 0.5) and sc.tolist() == [1, 2, 3, 4, 5]
    with pytest.raises(ValueError, match="BAEngine: per-observation loss kinds must have length 5"):
        st.pg_loss_table(n, ["huber"], who="BAEngine", what="observation")
    with pytest.raises(ValueError, match="BAEngine: unknown loss kind"):
        st.pg_loss_table(n, "hubert", who="BAEngine", what="observation")
    for name in ("set_loss", "has_loss", "loss_kernel_geometry"):
        assert hasattr(st.BAEngine, name)
