"""Self-tests of the dense dogleg reference (dogleg_ref.py): the three cases by construction, the same minimum as lm_step_ref's LM
reference, and every deliberate mistake of MUTATIONS moving a trace row by more than the GPU tests' C * kappa * eps bound."""
import numpy as np
import pytest

import dogleg_ref as D
import lm_step_ref as L

SCENE = (dict(n_lm=33, seed=12, pts_jitter=3.0), dict(initial_trust_region_radius=1.0))     # test_gpu_dogleg.py's "jitter3_r1"


def test_cases_by_construction():
    rng = np.random.default_rng(0)
    seen = set()
    for k in range(200):
        g = rng.normal(size=6)
        gn = -rng.uniform(0.5, 4.0) * g + rng.normal(size=6)
        alpha = rng.uniform(0.1, 1.0)
        cauchy = -alpha * g
        radius = rng.uniform(0.01, 1.2) * np.linalg.norm(gn)
        z, kase, beta = D.traditional_dogleg(cauchy, gn, radius)
        seen.add(kase)
        if kase == 0:
            assert np.linalg.norm(gn) <= radius and np.array_equal(z, gn)
            continue
        assert abs(np.linalg.norm(z) - radius) <= 1e-14 * radius
        if kase == 1:
            assert np.linalg.norm(cauchy) >= radius
        else:
            assert 0.0 <= beta <= 1.0
            assert np.allclose(z, cauchy + beta * (gn - cauchy), rtol=0, atol=1e-14 * radius)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("scene", ["st20", "ba_scene"])
def test_same_minimum_as_lm(scene):
    if scene == "st20":
        import importlib
        S = importlib.import_module("slam-tricks_amd.scenes")
        s = S.st20_scene()
        s["pt_fixed"] = np.zeros(len(s["pts0"]), np.uint8)
        o = L.lm_options()
        k = 25
    else:
        s = L.ba_scene(**SCENE[0])
        o = L.lm_options(**SCENE[1])
        k = 30
    prob = L.ba_problem(s)
    dl = D.dogleg_reference(prob, o, k)
    lm = L.lm_reference(prob, o, k)
    assert abs(dl[-1]["cost"] - lm[-1]["cost"]) <= 1e-8 * lm[-1]["cost"], (dl[-1]["cost"], lm[-1]["cost"])
    assert L.point_error(prob, dl[-1]["x"], lm[-1]["x"]) <= 1e-5 * np.linalg.norm(lm[-1]["x"])


# no Jacobi scaling and min_lm_diagonal = 1e-316: the camera that observes nothing has d^2 = 1e-316, and mu d^2 is 0 in binary64 at
# mu = 1e-8 and 2e-8 (a zero pivot: mu rises tenfold) but 1e-323 at 1e-7 -- the escalation the GPU tests assert, on the same scene
ESCALATION = (dict(n_lm=33, extras=True), dict(min_lm_diagonal=1e-316, jacobi_scaling=0, initial_trust_region_radius=1.0))


@pytest.mark.parametrize("mut", D.MUTATIONS)
def test_every_mutation_moves_the_trace(mut):
    """the first four on the parity scene, mu_never_decreased on the escalation scene (decisions and the factorisation count:
    that scene's kappa is too large for value bounds, which is how the GPU test compares it)"""
    if mut == "mu_never_decreased":
        s = L.ba_scene(**ESCALATION[0])
        o = L.lm_options(**ESCALATION[1])
        prob = L.ba_problem(s)
        ref = D.dogleg_reference(prob, o, 10)
        bad = D.dogleg_reference(prob, o, 10, mut={mut})
        assert sum(it["escalations"] for it in ref) >= 2
        assert (D.decisions(ref) != D.decisions(bad)), "mu_never_decreased leaves the decisions and the escalations as they were"
        return
    s = L.ba_scene(**SCENE[0])
    o = L.lm_options(**SCENE[1])
    prob = L.ba_problem(s)
    k = 10
    ref = D.dogleg_reference(prob, o, k)
    bad = D.dogleg_reference(prob, o, k, mut={mut})
    trace = np.vstack([np.zeros(7), D.trace_rows(bad)])
    trace[0, 5] = o["initial_trust_region_radius"]
    fails, _ = D.compare(prob, ref, o, bad[-1]["x"], trace)
    assert fails, f"mutation {mut} stays inside the GPU tests' bounds"


def test_mu_rule_of_the_reference():
    """a failed factorisation raises mu tenfold within the iteration; an accepted step lowers it to max(1e-8, mu / 5)"""
    s = L.ba_scene(**ESCALATION[0])
    o = L.lm_options(**ESCALATION[1])
    ref = D.dogleg_reference(L.ba_problem(s), o, 10)
    mu = D.MIN_MU
    for it in ref:
        mu *= D.MU_INCREASE ** it["escalations"]
        if it["accepted"]:
            mu = max(D.MIN_MU, 2.0 * mu / D.MU_INCREASE)
        assert it["mu"] == mu
    assert ref[0]["escalations"] == 1 and ref[0]["accepted"]


def test_the_reference_crawls_where_a_landmark_is_barely_constrained():
    """Why DOGLEG need not reach LM's minimum in 50 iterations at C5: a landmark whose Jacobian column is below
    sqrt(min_lm_diagonal) has d clamped, so the radius in z = d .* y barely bounds its step; the Gauss-Newton step at mu = 1e-8
    pushes it along its ray, every step is accepted with rho near 1, and the cost creeps.  The dense reference, which shares
    nothing with the device, does the same on the extras scene (a landmark at depth 1e3, near-parallel rays) with Ceres' defaults."""
    s = L.ba_scene(n_lm=33, extras=True)
    o = L.lm_options()
    prob = L.ba_problem(s)
    dl = D.dogleg_reference(prob, o, 40)
    lm = L.lm_reference(prob, o, 40)
    late = dl[20:]
    assert all(it["accepted"] and it["case"] == 0 and it["rho"] > 0.9 for it in late)
    assert min(it["step_norm"] for it in late) > 1e2                 # metres per step, long after the cost stopped moving much
    assert dl[-1]["cost"] > (1 + 1e-3) * lm[-1]["cost"]
