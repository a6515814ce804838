"""The 50-digit reference of the landmark elimination (tests/schur_elim_ref.py) and its cases (tests/schur_elim_cases.py), checked
on the CPU: the reference against one brute-force dense solve of the full system, the planted spectra against the case table,
and the plain float64 LAPACK-Cholesky elimination whose err / u fixes the constant C that the device is held to."""
import functools
import math

import numpy as np
import pytest

import schur_elim_cases as SC
import schur_elim_ref as SR

EPS = SR.EPS
QUANTITIES = ("Hpp", "gp", "S", "rhs", "dxp")


@functools.lru_cache(maxsize=None)
def cpu_reference(name):
    c = SC.build(*SC.CASES[name])
    r, Jc, Jp = SC.linearize(c)
    ref = SR.Reference(r, Jc, Jp, c["obs_cam"], c["obs_pt"], len(c["cams"]), len(c["pts"]), c["dc"], c["dp"], c["cam_fixed"], c["pt_fixed"])
    return c, (r, Jc, Jp), ref


def test_reference_reproduces_a_brute_force_solve_of_the_full_system():
    """the planted landmarks and twelve of the control scene, all cameras: Schur elimination at 50 digits against ONE dense LU of
    (J^T J + D) at 50 digits.  Both are rounded to doubles from values that agree to ~1e-25: equal to a few ulps"""
    c = SC.build("general", 0)
    r, Jc, Jp = SC.linearize(c)
    planted = np.nonzero(c["cls"] != "control")[0]
    chosen = np.concatenate([np.arange(0, 120, 10), planted])
    new = -np.ones(len(c["pts"]), int); new[chosen] = np.arange(len(chosen))
    m = new[c["obs_pt"]] >= 0
    big = c["obs_pt"] == np.nonzero(c["cls"] == "big")[0][0]
    m &= ~big | (np.cumsum(big) <= 30)                     # thirty of the 260 observations are enough here
    args = (r[m], Jc[m], Jp[m], c["obs_cam"][m], new[c["obs_pt"][m]], len(c["cams"]), len(chosen), c["dc"], c["dp"][chosen], c["cam_fixed"])
    ref = SR.Reference(*args, c["pt_fixed"][chosen])
    assert list(c["cls"][chosen][ref.out]) == ["fixed"] * 4
    dxc, dxp = SR.brute_force(*args, ref.out)
    rp, _ = ref.dxp()
    ec = np.abs(dxc - ref.dxc).max() / np.abs(dxc).max()
    ep = (np.abs(dxp - rp).max(1) / np.maximum(np.abs(dxp).max(1), 1e-300)).max()
    print(f"reference vs brute force: dxc {ec / EPS:.2f} EPS, dxp {ep / EPS:.2f} EPS (relative, per landmark)")
    assert ec <= 4 * EPS and ep <= 4 * EPS
    assert np.all(rp[ref.out] == 0)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_planted_spectra_are_what_the_case_table_claims(name):
    c, _, ref = cpu_reference(name)
    planted = np.nonzero(~np.isnan(c["claim"][:, 0]))[0]
    assert {"depth", "anisotropic", "single"} == set(c["cls"][planted])
    for j in planted:
        got, want = ref.lam[j] / ref.lam[j, 0], np.sort(c["claim"][j])[::-1]
        print(f"{name} landmark {j} {c['cls'][j]}: spectrum {got[1]:.3e} {got[2]:.3e}, claimed {want[1]:.1e} {want[2]:.1e}")
        assert np.all(got[1:] <= 4 * want[1:]) and np.all(got[1:] >= want[1:] / 4), (name, j, got, want)
    an = planted[c["cls"][planted] == "anisotropic"]
    k2 = ref.lam[an, 0] ** 2 / (ref.lam[an, 1] * ref.lam[an, 2])
    assert k2.min() <= 4e6 and k2.max() >= 2.5e17 and (ref.lam[an, 0] / ref.lam[an, 2]).max() <= SC.ACCURACY_KAPPA
    dk = ref.lam[c["cls"] == "depth"]
    assert (dk[:, 0] / dk[:, 2]).min() <= 2e4 and (dk[:, 0] / dk[:, 2]).max() >= 5e11
    # the constant and the unobserved landmarks, and nothing else, are outside the elimination / trivially in it
    assert set(c["cls"][ref.out]) == {"fixed"}
    assert np.bincount(c["obs_pt"], minlength=len(c["pts"])).max() > 256


def lapack_ratios(name):
    """err / u of the float64 LAPACK-Cholesky elimination per quantity and landmark class (S, rhs: the class of the landmark
    with the largest share of the block's unit)"""
    c, (r, Jc, Jp), ref = cpu_reference(name)
    nc, npts = len(c["cams"]), len(c["pts"])
    la = SR.lapack_elimination(r, Jc, Jp, c["obs_cam"], c["obs_pt"], nc, npts, c["dc"], c["dp"], c["cam_fixed"], c["pt_fixed"], ref.out)
    out = {}

    def note(q, ratios, classes):
        for k in np.unique(classes):
            out[(q, str(k))] = float(np.max(ratios[classes == k]))
    note("Hpp", SR.ratio(np.abs(la["Hpp"] - ref.Hpp).max((1, 2)), ref.u_Hpp), c["cls"])
    note("gp", SR.ratio(np.abs(la["gp"] - ref.gp).max(1), ref.u_gp), c["cls"])
    low = np.tril(np.ones((2 * nc, 2 * nc), bool))
    note("S", SR.ratio(SR.block_err(la["S"], ref.S), ref.u_S)[low], np.where(ref.s_worst >= 0, c["cls"][ref.s_worst], "none")[low])
    note("rhs", SR.ratio(SR.block_err(la["rhs"], ref.rhs), ref.u_rhs), np.where(ref.rhs_worst >= 0, c["cls"][ref.rhs_worst], "none"))
    dxp, u = ref.dxp(la["dxc"])
    note("dxp", SR.ratio(np.abs(la["dxp_of"](la["dxc"]) - dxp).max(1), u), c["cls"])
    return out


def test_lapack_elimination_fixes_the_constant():
    worst, where = 0.0, None
    table = {}
    for name in SC.CASES:
        for key, v in lapack_ratios(name).items():
            table[key] = max(table.get(key, 0.0), v)
            if v > worst:
                worst, where = v, (name,) + key
    for q in QUANTITIES:
        print(f"LAPACK err/u {q}: " + "  ".join(f"{k}={v:.3g}" for (qq, k), v in sorted(table.items()) if qq == q))
    print(f"worst err / u of the LAPACK elimination: {worst:.3f} at {where}; C = {SR.C}")
    assert np.isfinite(worst) and worst > 0
    assert SR.C == 2.0 ** math.ceil(math.log2(8 * worst)), (worst, SR.C)
    assert abs(SR.LAPACK_WORST - worst) <= 0.1 * worst


@pytest.mark.parametrize("name", list(SC.CASES))
def test_bound_stays_meaningful_on_every_accuracy_case(name):
    """lambda_1 / lambda_3 EPS C <= 1e-3 on every landmark that is held to C u: the bound leaves three digits at least"""
    c, _, ref = cpu_reference(name)
    kap = ref.lam[:, 0] / ref.lam[:, 2]
    acc = ~ref.out & (kap <= SC.ACCURACY_KAPPA)
    assert set(c["cls"][acc]) >= {"control", "depth", "anisotropic", "single", "big"}
    assert set(c["cls"][~ref.out & ~acc]) <= {"depth"}
    assert np.all(kap[acc] * EPS * SR.C <= 1e-3), (kap[acc].max(), SR.C)


def test_rescaled_cases_are_exact_powers_of_two():
    base = SC.build("general", 0)
    r0, Jc0, Jp0 = SC.linearize(base)
    for k in (-40, 40):
        c = SC.build("general", k)
        r, Jc, Jp = SC.linearize(c)
        sc = 2.0 ** k
        assert np.array_equal(r, r0) and np.array_equal(Jp * sc, Jp0)
        assert np.array_equal(Jc[:, :, :3], Jc0[:, :, :3]) and np.array_equal(Jc[:, :, 3:] * sc, Jc0[:, :, 3:])
        assert np.array_equal(c["dp"] * sc * sc, base["dp"]) and np.array_equal(c["dc"][:, 3:] * sc * sc, base["dc"][:, 3:])


def test_lm_case_passes_the_lm_judges_guards_on_the_reference_alone():
    """the weighted LM scene of the full-LM GPU test: three reference iterations at Ceres' default radius, all accepted, with
    64 kappa EPS <= 1e-6 and every rho a margin away from the acceptance threshold -- the preconditions of the LM tests' judge"""
    import ba_information_ref as I
    import ba_loss_ref as B
    import lm_step_ref as L
    s, W = SC.lm_scene()
    assert len(s["cams0"]) <= 12 and (np.linalg.cond(W[-8:]) >= 99).all() and np.linalg.cond(W[-8:]).max() >= 9e3
    o = L.lm_options()
    ref = B.lm_reference(I.WeightedBAProblem(s, W), o, 3)
    kap = max(it["kappa"] for it in ref)
    print(f"LM case: kappa {kap:.3g}, accepted {[it['accepted'] for it in ref]}, rho {[round(it['rho'], 3) for it in ref]}")
    assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6 and L.rho_margin_ok(ref, o) and all(it["accepted"] for it in ref)
