"""DOGLEG bundle adjustment on the device against the independent dense reference of dogleg_ref.py: the pair-plan
and the dense-visibility Schur form and a host lineariser, k = 1, 3 and 10 iterations, the end point and every trace column within
lm_step_ref's C * kappa * eps bounds and the accept / reject decisions identical.  Then what makes the strategy worth having: one
factorisation per linearisation, a rejected step re-uses it; the solve is bitwise reproducible; switching back to LM leaves LM
untouched; the C ABI refuses what DOGLEG does not support."""
import ctypes as C
import importlib

import numpy as np
import pytest

import dogleg_ref as D
import lm_step_ref as L

pytestmark = pytest.mark.gpu

# landmarks 3 m off, radius 1: Cauchy steps, a rejection (rho -158) at iteration 3, an interpolated step at 4, three rejections
# in a row from 6, Gauss-Newton steps; the 300-landmark scene: Cauchy and interpolated steps, all accepted
SCENES = {
    "jitter3_r1": (dict(n_lm=33, seed=12, pts_jitter=3.0), dict(initial_trust_region_radius=1.0)),
    "lm300_r1e-2": (dict(n_lm=300, n_cams=10, seed=7), dict(initial_trust_region_radius=1e-2)),
}


@pytest.fixture(scope="module")
def st():
    mod = importlib.import_module("slam-tricks_amd")
    assert mod.device_count() > 0, "GPU tests need a HIP device"
    return mod


def engine(st, s):
    e = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"])
    e.set_trust_region("dogleg")
    return e


def x_of(e):
    cams, pts = e.get_params()
    return np.concatenate([cams.reshape(-1), pts.reshape(-1)])


def run(st, e, o, k, callback=None):
    summ, tr = e.solve(st.default_options(**dict(o, max_num_iterations=k)), callback=callback)
    assert summ.num_iterations == k and len(tr) == k + 1, summ.as_dict()
    return summ, tr


def check(prob, ref, o, e, tr, label):
    kap = max(it["kappa"] for it in ref)
    assert L.C_PATH["ba"] * kap * L.EPS <= 1e-6, f"{label}: kappa {kap:.2e} too large for an accuracy case"
    assert L.rho_margin_ok(ref, o), f"{label}: a reference rho sits within 1e-2 of min_relative_decrease"
    fails, ratios = D.compare(prob, ref, o, x_of(e), tr)
    print(f"DOGLEG {label} kappa={kap:.2e} " + " ".join(f"{k}={v:.2e}" for k, v in sorted(ratios.items())))
    assert not fails, f"{label}: " + "; ".join(fails)


def test_reference_trace_covers_every_case():
    """the parity runs below are not vacuous: the reference's 10 iterations hold all three cases and rejected steps"""
    sk, ok = SCENES["jitter3_r1"]
    ref = D.dogleg_reference(L.ba_problem(L.ba_scene(**sk)), L.lm_options(**ok), 10)
    assert {it["case"] for it in ref} == {0, 1, 2}
    assert sum(1 for it in ref if not it["accepted"]) >= 1
    assert all(it["valid"] for it in ref)


# (the 300-landmark scene stops at 5: from iteration 6 on its gradient is at the level of its rounding, ~1e-13, where a
# relative bound on |g|max means nothing)
PARITY = [(sc, k) for sc in SCENES for k in ((1, 3, 10) if sc == "jitter3_r1" else (1, 3, 5))]


# (watched: the pair plan with an iteration callback -- the loop reads every new linearisation's scalars at once)
@pytest.mark.parametrize("form", ["pairs", "dense", "host", "watched"])
@pytest.mark.parametrize("scene,k", PARITY)
def test_parity_with_reference(st, scene, form, k):
    sk, ok = SCENES[scene]
    s = L.ba_scene(**sk)
    o = L.lm_options(**ok)
    prob = L.ba_problem(s)
    ref = D.dogleg_reference(prob, o, k)
    e = engine(st, s)
    if form == "dense":
        e.set_schur_mode(e.SCHUR_DENSE)
    elif form == "host":
        e.set_host_linearizer(lambda cams, pts, want: prob.lin_obs(cams.copy(), pts.copy(), want))
    _, tr = run(st, e, o, k, callback=(lambda *a: 0) if form == "watched" else None)
    check(prob, ref, o, e, tr, f"{scene} {form} k={k}")
    ds = e.dogleg_summary()
    assert list(ds.steps_by_case) == [sum(1 for it in ref if it["case"] == c) for c in range(3)], ds.as_dict()


def test_one_factorisation_per_linearisation(st):
    sk, ok = SCENES["jitter3_r1"]
    s = L.ba_scene(**sk)
    o = L.lm_options(**ok)
    k = 10
    ref = D.dogleg_reference(L.ba_problem(s), o, k)
    rejected = sum(1 for it in ref if not it["accepted"])
    escalations = sum(it["escalations"] for it in ref)
    linearisations = sum(1 for it in ref if not it["reused"])
    assert rejected >= 1
    e = engine(st, s)
    summ, tr = run(st, e, o, k)
    ds = e.dogleg_summary()
    print("DOGLEG summary", ds.as_dict(), "successful", summ.num_successful_steps, "unsuccessful", summ.num_unsuccessful_steps)
    assert ds.factorizations == ds.gauss_newton_solves == linearisations + escalations
    assert ds.factorizations < summ.num_iterations
    assert ds.reused_steps == sum(1 for it in ref if it["reused"]) == rejected - (0 if ref[-1]["accepted"] else 1)
    assert ds.invalid_steps == 0 and summ.num_unsuccessful_steps == rejected
    assert ds.final_mu == ref[-1]["mu"]
    assert summ.final_radius == tr[-1][5]


def test_bitwise_reproducible(st):
    sk, ok = SCENES["lm300_r1e-2"]
    s = L.ba_scene(**sk)
    o = L.lm_options(**ok)
    out = []
    for _ in range(2):
        e = engine(st, s)
        _, tr = run(st, e, o, 10)
        out.append((x_of(e).tobytes(), tr.tobytes()))
    assert out[0] == out[1]


def test_two_solves_on_one_engine(st):
    """the second solve of an engine is the solve of a fresh engine at the same point (what a solve resets, it resets per solve)"""
    sk, ok = SCENES["jitter3_r1"]
    s = L.ba_scene(**sk)
    e = engine(st, s)
    e.solve(st.default_options(**dict(ok, max_num_iterations=2)))
    cams, pts = e.get_params()
    sa, ta = e.solve(st.default_options(**ok))
    f = st.BAEngine(cams, pts, s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"])
    f.set_trust_region("dogleg")
    sb, tb = f.solve(st.default_options(**ok))
    print("DOGLEG two solves", sa.as_dict(), e.dogleg_summary().as_dict())
    assert sa.num_iterations == sb.num_iterations and sa.termination_reason == sb.termination_reason, (sa.as_dict(), sb.as_dict())
    assert e.dogleg_summary().as_dict() == f.dogleg_summary().as_dict()
    assert ta.tobytes() == tb.tobytes() and x_of(e).tobytes() == x_of(f).tobytes()


def test_watched_equals_unwatched(st):
    """to convergence at the library's defaults: the deferred read of a new linearisation's scalars against the immediate one"""
    sk, ok = SCENES["jitter3_r1"]
    s = L.ba_scene(**sk)
    out = []
    for cb in (None, lambda *a: 0):
        e = engine(st, s)
        summ, tr = e.solve(st.default_options(**ok), callback=cb)
        out.append((summ, tr, x_of(e), e.dogleg_summary().as_dict()))
    (su, tu, xu, du), (sw, tw, xw, dw) = out
    print("DOGLEG watched/unwatched", su.as_dict(), du, "max|d trace|", np.abs(tu - tw).max() if tu.shape == tw.shape else None)
    assert su.termination_type == 0
    assert (su.num_iterations, su.termination_reason, su.num_successful_steps, su.num_unsuccessful_steps) == \
           (sw.num_iterations, sw.termination_reason, sw.num_successful_steps, sw.num_unsuccessful_steps)
    assert du == dw and np.array_equal(tu[:, 6], tw[:, 6])
    assert tu.tobytes() == tw.tobytes() and xu.tobytes() == xw.tobytes()


def test_progress_text(st, capfd):
    """minimizer_progress_to_stdout: the header, then one row per trace row, numbered 0 .. num_iterations"""
    import ctypes
    sk, ok = SCENES["jitter3_r1"]
    s = L.ba_scene(**sk)
    e = engine(st, s)
    libc = ctypes.CDLL(None)
    libc.fflush(None)
    capfd.readouterr()
    summ, tr = e.solve(st.default_options(**dict(L.lm_options(**ok), max_num_iterations=5, minimizer_progress_to_stdout=1)))
    libc.fflush(None)
    lines = capfd.readouterr().out.splitlines()
    assert summ.num_iterations == 5 and len(tr) == 6
    assert lines[0].split()[:2] == ["iter", "cost"], lines
    assert len(lines) == 1 + len(tr), lines
    assert [int(ln.split()[0]) for ln in lines[1:]] == list(range(summ.num_iterations + 1))


def test_switching_back_to_lm_is_lm(st):
    sk, ok = SCENES["jitter3_r1"]
    s = L.ba_scene(**sk)
    o = st.default_options(**dict(L.lm_options(**ok), max_num_iterations=6))
    e = engine(st, s)
    e.solve(o)
    e.set_params(s["cams0"], s["pts0"])
    e.set_trust_region("lm")
    s1, t1 = e.solve(o)
    assert e.dogleg_summary().factorizations == 0
    f = st.BAEngine(s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"], pt_fixed=s["pt_fixed"])
    s2, t2 = f.solve(o)
    assert t1.tobytes() == t2.tobytes() and x_of(e).tobytes() == x_of(f).tobytes()


def test_c_abi_refusals(st):
    s = L.ba_scene(n_lm=31)
    lib = st.lib()
    args = (s["cams0"], s["pts0"], s["obs_cam"], s["obs_pt"], s["obs_feat"], s["cam_fixed"])
    it = st.BAEngine(*args, pt_fixed=s["pt_fixed"], linear_solver="iterative_schur")
    with pytest.raises(st.StbaError) as ei:
        it.set_trust_region("dogleg")
    assert ei.value.code == -1
    e = st.BAEngine(*args, pt_fixed=s["pt_fixed"])
    assert lib.stba_ba_set_trust_region(e._h, 7) == -1
    e.set_allreduce(lambda user, ptr, count, stream: 0, 0, 1)
    assert lib.stba_ba_set_trust_region(e._h, 1) == -1
    f = engine(st, s)
    with pytest.raises(st.StbaError) as ei:
        f.set_allreduce(lambda user, ptr, count, stream: 0, 0, 1)
    assert ei.value.code == -1
    # the refused calls left the engines as they were: f still solves DOGLEG, e LM
    o = st.default_options(**dict(L.lm_options(), max_num_iterations=2))
    f.solve(o)
    assert f.dogleg_summary().factorizations >= 1
    bad = st.DoglegSummary()
    bad.struct_size = 4
    assert lib.stba_ba_last_dogleg_summary(f._h, C.byref(bad)) == -1


def test_mu_escalation_matches_the_reference(st):
    """the escalation path on the device: the reference's trace (tests/test_dogleg_reference.py ESCALATION) raises mu inside the
    iteration; the device takes the same decisions, the same cases, and one factorisation per linearisation plus one per escalation.
    Decisions only: with no Jacobi scaling this scene's kappa is far beyond a value bound."""
    from test_dogleg_reference import ESCALATION
    s = L.ba_scene(**ESCALATION[0])
    o = L.lm_options(**ESCALATION[1])
    k = 10
    ref = D.dogleg_reference(L.ba_problem(s), o, k)
    escalations = sum(it["escalations"] for it in ref)
    assert escalations >= 2 and L.rho_margin_ok(ref, o)
    e = engine(st, s)
    _, tr = run(st, e, o, k)
    ds = e.dogleg_summary()
    print("DOGLEG escalation", ds.as_dict(), "reference", D.decisions(ref))
    assert [bool(v) for v in tr[1:, 6]] == [it["accepted"] for it in ref]
    assert list(ds.steps_by_case) == [sum(1 for it in ref if it["case"] == c) for c in range(3)]
    assert ds.factorizations == sum(1 for it in ref if not it["reused"]) + escalations
    assert ds.final_mu == ref[-1]["mu"]
