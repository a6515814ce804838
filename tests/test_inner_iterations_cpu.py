"""CPU checks of the inner iterations: every deliberate mistake of inner_iterations_ref.MUTATIONS moves a result on the GPU tests'
scenes by far more than their tolerance (so that the device comparison of test_gpu_inner_iterations.py means something), the
reference's ordering rules, and the Python wrapper's argument checks (no device needed)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import inner_iterations_ref as I
import lm_step_ref as L


def _solve(prob, mut=(), tol=1e-3, k=8, order=None, **kw):
    rows, _ = I.outer_reference(prob, dict(L.lm_options(**kw), function_tolerance_takes_step=1), k,
                                order if order is not None else I.ordering(prob), tol, frozenset(mut))
    return rows


def _moved(a, b):
    """how far two reference runs are apart: decisions, trace values and end points"""
    if len(a) != len(b) or any(x["accepted"] != y["accepted"] or x["inner_on"] != y["inner_on"] for x, y in zip(a, b)):
        return np.inf
    d = 0.0
    for x, y in zip(a, b):
        d = max(d, abs(x["trial_cost"] - y["trial_cost"]) / max(abs(y["trial_cost"]), 1e-300),
                abs(x["step_norm"] - y["step_norm"]) / max(y["step_norm"], 1e-300),
                float(np.abs(x["x"] - y["x"]).max()))
    return d


@pytest.fixture(scope="module")
def scenes():
    s = L.ba_scene()
    return {"ba": L.ba_problem(s), "useful": L.ba_problem(L.ba_scene(n_lm=32, ang_noise_deg=6.0, pos_noise=0.5))}


def test_every_mutation_is_caught(scenes):
    prob = scenes["ba"]
    base = {"default": _solve(prob), "tol": _solve(prob, tol=0.5), "ftol": _solve(prob, function_tolerance=1e-6, k=20),
            "useful": _solve(scenes["useful"], initial_trust_region_radius=1e16, k=6),
            "split": _solve(prob, order=I.ordering(prob, np.zeros(prob.nc, int), np.ones(prob.nc, int), np.full(prob.np_, 2)))}
    caught = {}
    for m in I.MUTATIONS:
        worst = 0.0
        for name, rows in base.items():
            kw = {"tol": dict(tol=0.5), "ftol": dict(function_tolerance=1e-6, k=20),
                  "useful": dict(initial_trust_region_radius=1e16, k=6)}.get(name, {})
            p = scenes["useful"] if name == "useful" else prob
            order = I.ordering(prob, np.zeros(prob.nc, int), np.ones(prob.nc, int), np.full(prob.np_, 2)) if name == "split" else None
            mrows = _solve(p, mut=(m,), order=order, **kw)
            worst = max(worst, _moved(mrows, rows))
        caught[m] = worst
        print(f"MUTATION {m}: moved {worst:.2e}")
    # the GPU tests' bounds are 1e-7 (costs) / 1e-6 (steps, end points): every mutation moves something by far more, or flips a decision
    assert all(v > 1e-4 for v in caught.values()), caught


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KY = np.array([2.0, 2.2663, 2.5681, 2.9099, 3.2974])
STOPS = {1: "gradient", 2: "function", 3: "parameter", 4: "max_iter", 5: "min_radius", 6: "invalid"}
# family, max_num_iterations, function / gradient / parameter tolerance, initial radius, min radius, x0 (tests/cpp/test_inner_policy.cpp)
POLICY_CASES = [
    (0, 50, 1e-6, 1e-10, 1e-8, 1e4, 1e-32, 1.0, 2.0),      # gradient at the start
    (0, 50, 1e-6, 1e-10, 1e-8, 1e4, 1e-32, 5.0, -3.0),
    (1, 50, 1e-6, 1e-10, 1e-8, 1e4, 1e-32, -1.2, 1.0),
    (2, 50, 1e-6, 1e-10, 1e-8, 1e4, 1e-32, 0.0, 1.0),
    (2, 50, 1e-3, 1e-10, 1e-8, 1e4, 1e-32, 0.0, 1.0),      # function
    (1, 50, 1e-2, 0.0, 0.0, 1e4, 1e-32, -1.2, 1.0),         # function
    (1, 50, 1e-6, 1e-10, 1e-2, 1e4, 1e-32, -1.2, 1.0),     # parameter
    (1, 3, 0.0, 0.0, 0.0, 1e4, 1e-32, -1.2, 1.0),          # max_iter
    (1, 50, 0.0, 0.0, 0.0, 1e-3, 1e-32, -1.2, 1.0),
    (0, 50, 1e-6, 1e-10, 1e-8, 1e4, 1e5, 3.0, 3.0),        # min_radius
    (3, 50, 1e-6, 1e-10, 1e-8, 1e4, 1e-32, 0.0, 0.0),      # invalid (an indefinite system: every factorisation fails)
]


def _family(fam):
    """(lin, cost_at) of a case family, as tests/cpp/test_inner_policy.cpp computes it"""
    def res(x):
        if fam == 0:
            return np.array([x[0] - 1.0, x[1] - 2.0]), np.eye(2)
        if fam == 1:
            return np.array([10.0 * (x[1] - x[0] ** 2), 1.0 - x[0]]), np.array([[-20.0 * x[0], 10.0], [-1.0, 0.0]])
        t = 0.25 * np.arange(5)
        e = np.exp(x[0] * t)
        return x[1] * e - KY, np.stack([x[1] * t * e, e], 1)

    def cost_at(x):
        return 1.0 if fam == 3 else float(0.5 * np.sum(res(x)[0].astype(I.LD) ** 2))

    def lin(x):
        if fam == 3:
            return 1.0, np.array([[1, 100], [100, 1]], dtype=I.LD), np.array([1, 0], dtype=I.LD)
        r, J = res(x)
        return cost_at(x), (J.T.astype(I.LD) @ J.astype(I.LD)), (J.T.astype(I.LD) @ r.astype(I.LD))
    return lin, cost_at


@pytest.fixture(scope="module")
def policy_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("inner_policy") / "test_inner_policy")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_inner_policy.cpp"), "-o", out])
    return out


def test_block_policy_header_matches_reference(policy_exe):
    """inner_policy.hpp (the device's block LM) compiled with g++ against inner_iterations_ref.block_lm: iterations, stop reason and
    end point on a table of cases that reaches every stop reason"""
    inp = "".join(" ".join(repr(v) for v in c) + "\n" for c in POLICY_CASES)
    p = subprocess.run([policy_exe], input=inp, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.split("\n")
    seen = set()
    for case, line in zip(POLICY_CASES, lines):
        fam, max_it, ftol, gtol, ptol, r0, rmin, x0, x1 = case
        it_c, stop_c, xa, xb = line.split()
        opts = dict(I.BLOCK_OPTIONS, max_num_iterations=max_it, function_tolerance=ftol, gradient_tolerance=gtol, parameter_tolerance=ptol,
                    initial_trust_region_radius=r0, min_trust_region_radius=rmin)
        lin, cost_at = _family(fam)
        x, it, why = I.block_lm(lin, cost_at, lambda x, d: x + d, np.array([x0, x1]), np.ones(2, bool), np.ones(2, bool), opts)
        assert (int(it_c), STOPS[int(stop_c)]) == (it, why), (case, line, it, why)
        assert np.allclose([float(xa), float(xb)], x, rtol=1e-9, atol=1e-12), (case, line, x)
        seen.add(why)
    assert len(lines) >= len(POLICY_CASES)
    assert seen == set(STOPS.values()), seen


def test_reference_ordering_rules(scenes):
    prob = scenes["ba"]
    o = I.ordering(prob)
    assert [g for g, _, _ in o] == [0, 1] and all(k == 3 for _, cams, _ in o[:1] for _, k in cams)
    assert len(o[1][2]) == prob.np_ - int(prob.pt_fixed.sum())
    with pytest.raises(ValueError, match="not an independent set"):
        I.ordering(prob, np.zeros(prob.nc, int), None, np.zeros(prob.np_, int))
    o = I.ordering(prob, None, None, np.zeros(prob.np_, int))          # landmarks only: the cameras are held fixed
    assert len(o) == 1 and o[0][1] == []


def test_python_wrapper_argument_checks():
    st = importlib.import_module("slam-tricks_amd")
    assert st.inner_ordering(3, 4) == (1e-3, None, None, None)
    tol, r, q, p = st.inner_ordering(3, 4, 0.0, [0, 0, -1], None, [1, 1, 1, 1])
    assert tol == 0.0 and r.dtype == np.int32 and q is None and p.tolist() == [1, 1, 1, 1]
    for bad in (dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(rot_group=[0, 0]), dict(pt_group=[0, 0, 0, -2]),
                dict(pos_group=[0.5, 0, 0])):
        with pytest.raises(ValueError):
            st.inner_ordering(3, 4, **{"tolerance": 1e-3, **bad})
    # the engine method checks before it reaches the library
    e = st.BAEngine.__new__(st.BAEngine)
    e.nc, e.np_, e._h = 3, 4, None
    with pytest.raises(ValueError):
        e.set_inner_iterations(True, -1.0)
    s = st.InnerSummary()
    assert s.struct_size == 0 and len(s.group_size) == st.INNER_MAX_GROUPS_REPORTED


def test_header_declares_the_inner_iteration_abi():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stba.h")).read()
    for name in ("stba_ba_set_inner_iterations", "stba_ba_inner_sweep", "stba_ba_last_inner_summary", "stba_inner_summary"):
        assert name in hdr
