"""The bundle adjustment's feature table and factor-input checks (slam-tricks_amd/csrc/ba_features.hpp, ba_factor_input.hpp) without a
device: tests/cpp/ba_factor_input_driver.cpp, compiled with g++ -- plain, with the address + undefined-behaviour sanitizers and with
the thread sanitizer, which must run without a report and print the same.

  table      the rows equal tests/golden/ba_refusals.json (asker, held feature, code, full text, in order); for every asker and every
             one of the 2^9 held masks ba_conflict answers with the FIRST golden row the mask meets, for a setting and for a clearing
             call; if asking A with B held is refused, so is asking B with A held, but for the exceptions listed in ASYMMETRIC
  pose, W    pose7_check_normalise and sqrt_information6 on a row per branch; codes and texts against the same golden file (as the
             setters gave them before the checks moved), W in every bit what prior_information_factor gives
  grouping   group_csr against a stable numpy argsort, by camera and by unordered pair
  6 x 6      prior_information_factor = information6_factor (dd6.hpp, the one double-double factorisation of the tree: the pose graph's kernel calls the same
             function) against the 50-digit Cholesky factor (mp_ref.chol6_T), well conditioned and at cond 1e12: every entry of W within
             FACTOR6_BOUND = 1 eps of the exact one, relative -- 1/2 eps is the rounding of the double-double result to FP64, the
             other half is room for the double-double arithmetic's own error, about cond 2^-104 per operation, 1e-19 at cond 1e12;
             an FP64 Cholesky must MISS the bound at cond 1e12 (it loses cond eps), or the bound would not notice a dropped low word.
             Also W^T W, formed at 50 digits, within the 1e-13 of the matrix that test_sqrt_information_rows holds
             sqrt_information6 to, on matrices of that case's scale; rank-deficient matrices and a NaN are refused
  2 x 2      ba_information_factor within the 4 eps per entry its comment claims of the 50-digit factor (ba_information_ref.chol2_mp,
             mpmath at mp_ref's 50 digits), condition numbers 1 to 1e15; the refused matrices"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import ba_information_ref as I
import mp_ref  # (mp.dps = 50)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"], "tsan": ["-fsanitize=thread", "-g"]}
EPS = 2.0 ** -52
INV, NPD = -1, -4
FEATURE_OF = {"stba_ba_set_host_linearizer": "HOST_LINEARIZER", "stba_ba_set_loss": "LOSS", "stba_ba_set_information": "INFORMATION",
              "stba_ba_set_sqrt_information": "INFORMATION", "stba_ba_set_pose_priors": "POSE_PRIORS",
              "stba_ba_set_relative_poses": "RELATIVE_POSES", "stba_ba_set_allreduce": "ALLREDUCE", "stba_ba_set_trust_region": "DOGLEG",
              "stba_ba_set_inner_iterations": "INNER_ITERATIONS", "stba_ba_inner_sweep": "INNER_ITERATIONS"}
# refusals without a mirror image, and why
ASYMMETRIC = {"ITERATIVE_SCHUR": "fixed at creation: no call asks for it",
              ("DOGLEG", "INNER_ITERATIONS"): "refused by stba_ba_solve, by neither setter"}


def _no_address_randomisation():
    """(ThreadSanitizer's fixed shadow layout does not take every placement a kernel with 32 bits of mmap randomisation hands out)"""
    ctypes.CDLL(None).personality(0x0040000)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "ba_refusals.json")) as f:
        return json.load(f)


def hexes(a):
    return " ".join(float(x).hex() for x in np.asarray(a, float).reshape(-1))


# ------------------------------------------------------------------------------------------ the cases of the second mode
def unit_quaternion(seed):
    q = np.random.default_rng(seed).normal(size=4)
    return q / np.linalg.norm(q)


def spd6(seed):
    A = np.random.default_rng(seed).normal(size=(6, 6))
    return A @ A.T + 0.1 * np.eye(6)


T3 = [0.5, -1.25, 2.0]
POSES = {"valid": list(unit_quaternion(1)) + T3,
         "nan": list(unit_quaternion(1)) + [0.5, np.nan, 2.0],
         "zero_quaternion": [0.0] * 4 + T3,
         "one_plus_4_eps": [0.0, 0.0, 0.0, 1.0 + 4 * EPS] + T3,        # |n^2 - 1| = 8 eps: the bits are kept
         "one_plus_5_eps": [0.0, 0.0, 0.0, 1.0 + 5 * EPS] + T3,        # 10 eps: normalised
         "norm_3": list(3.0 * unit_quaternion(2)) + T3}
INF6 = np.eye(6); INF6[2, 3] = np.inf
INDEFINITE = np.eye(6); INDEFINITE[4, 4] = -1.0
RANK_DEFICIENT = np.diag([0.0, 0.0, 0.0, 1.0, 2.0, 3.0])
SQRT6 = {"valid_information": ("I", spd6(3)), "valid_sqrt": ("S", np.random.default_rng(4).normal(size=(6, 6))),
         "inf_sqrt": ("S", INF6), "inf_information": ("I", INF6), "indefinite_information": ("I", INDEFINITE),
         "rank_deficient_sqrt": ("S", RANK_DEFICIENT), "neither": ("N", None)}


def spd6_cond(kappa, seed):
    """Q diag(lambda) Q^T with lambda log-spaced from 10 down to 10 / kappa, exactly symmetric"""
    Q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(6, 6)))
    A = Q @ np.diag(10.0 ** (1.0 - np.linspace(0.0, np.log10(kappa), 6))) @ Q.T
    return 0.5 * (A + A.T)


NAN6 = spd6(3); NAN6[4, 1] = np.nan                       # in the lower triangle, which is factored
NAN6_UPPER = spd6(3); NAN6_UPPER[1, 4] = np.nan           # in the upper one, which is not: refused all the same
SINGULAR_BLOCK = np.eye(6); SINGULAR_BLOCK[:2, :2] = [[4.0, 2.0], [2.0, 1.0]]      # the second pivot is 1 - 1 exactly
FACTOR6_BOUND = 1.0          # eps, relative, per entry of W against the 50-digit factor (the module's docstring)
FACTOR6_GOOD = {"spd6_3": spd6(3), "spd6_7": spd6(7), "identity": np.eye(6), "cond_1e2": spd6_cond(1e2, 11), "cond_1e6": spd6_cond(1e6, 12),
                "cond_1e12": spd6_cond(1e12, 13), "cond_1e12_b": spd6_cond(1e12, 14)}
FACTOR6_REFUSED = {"rank_3_diagonal": (RANK_DEFICIENT, NPD), "rank_1_ones": (np.ones((6, 6)), NPD), "rank_5_block": (SINGULAR_BLOCK, NPD),
                   "indefinite": (INDEFINITE, NPD), "nan_lower": (NAN6, INV), "nan_upper": (NAN6_UPPER, INV), "inf": (INF6, INV)}


def omega2(kappa, phi=0.7, scale=3.0):
    Q = I.rot(np.array([phi]))[0]
    Om = Q @ np.diag([1.0, 1.0 / kappa]) @ Q.T * scale
    Om[1, 0] = Om[0, 1]
    return Om


KAPPAS = [1.0, 1e4, 1e8, 1e12, 1e15]
INFO2_BAD = {"indefinite": [[1.0, 2.0], [2.0, 1.0]], "negative_a": [[-1.0, 0.0], [0.0, 1.0]], "nan": [[1.0, 0.0], [np.nan, 1.0]],
             "inf_upper": [[1.0, np.inf], [0.0, 1.0]], "semidefinite": [[1.0, 1.0], [1.0, 1.0]]}

_shuffled = np.random.default_rng(5)
EDGES = {"one_edge": ([2], [0]),
         "a_pair_in_both_directions": ([0, 1, 0, 1], [1, 0, 1, 2]),
         "a_camera_only_as_j": ([0, 1, 0], [3, 3, 1]),
         "seventeen_over_five": None}
_ci = _shuffled.integers(0, 5, 17)
EDGES["seventeen_over_five"] = (list(_ci), list((_ci + _shuffled.integers(1, 5, 17)) % 5))


def case_lines():
    lines, names = [], []
    for what in ("the_pose", "the_measurement"):
        for k, p in POSES.items():
            lines.append(f"pose7 {what} {hexes(p)}"); names.append(("pose7", what.replace("_", " "), k))
    for k, (mode, m) in SQRT6.items():
        lines.append(f"sqrt6 {mode}" + ("" if m is None else " " + hexes(m))); names.append(("sqrt6", k))
    for k, m in FACTOR6_GOOD.items():
        lines.append(f"sqrt6 I {hexes(m)}"); names.append(("factor6", k))
    for k, (m, _) in FACTOR6_REFUSED.items():
        lines.append(f"sqrt6 I {hexes(m)}"); names.append(("factor6", k))
    for kap in KAPPAS:
        lines.append(f"info2 {hexes(omega2(kap))}"); names.append(("info2", kap))
    for k, m in INFO2_BAD.items():
        lines.append(f"info2 {hexes(m)}"); names.append(("info2", k))
    for k, (ci, cj) in EDGES.items():
        lines.append(f"group_cam {len(ci)} " + " ".join(map(str, ci))); names.append(("group_cam", k))
        lines.append(f"group_edges {len(ci)} " + " ".join(map(str, list(ci) + list(cj)))); names.append(("group_edges", k))
    return lines, names


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """kind -> (the table mode's JSON, {case name: the case mode's JSON}); every kind is built and run once"""
    base = tmp_path_factory.mktemp("ba_factor_input")
    lines, names = case_lines()
    (base / "cases.txt").write_text("\n".join(lines) + "\n")
    out = {}
    for kind, flags in SANITIZERS.items():
        exe = str(base / f"driver_{kind}")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *flags, os.path.join(ROOT, "tests", "cpp", "ba_factor_input_driver.cpp"), "-o", exe])
        got = []
        for args in (["table"], ["cases", str(base / "cases.txt")]):
            p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120,
                               preexec_fn=_no_address_randomisation if kind == "tsan" else None)
            assert p.returncode == 0 and p.stderr == "", (kind, args, p.returncode, p.stderr[-2000:])
            got.append(p.stdout)
        res = [json.loads(l) for l in got[1].splitlines()]
        assert len(res) == len(names)
        out[kind] = (json.loads(got[0]), dict(zip(names, res)))
    return out


def floats(v):
    return np.array([float.fromhex(x) for x in v])


# ------------------------------------------------------------------------------------------ the table
def test_the_rows_are_the_golden_rows_in_order(runs, golden):
    rows = runs["plain"][0]["rows"]
    assert len(rows) == len(golden["rows"])
    for got, want in zip(rows, golden["rows"]):
        assert got == want


def test_every_mask_meets_the_first_golden_row(runs, golden):
    table = runs["plain"][0]
    feats = table["features"]
    assert len(feats) == 9
    askers = list(dict.fromkeys(r["asker"] for r in golden["rows"]))
    assert sorted(table["setting"]) == sorted(table["clearing"]) == sorted(askers)
    for mode in ("setting", "clearing"):
        for asker in askers:
            answers = table[mode][asker]
            assert len(answers) == 512
            for mask, (code, text) in enumerate(answers):
                held = {f for k, f in enumerate(feats) if mask >> k & 1}
                want = next((r for r in golden["rows"] if r["asker"] == asker and set(r["held"]) <= held
                             and (mode == "setting" or r["when_clearing"])), None)
                assert (code, text) == ((want["code"], asker + ": " + want["text"]) if want else (0, "")), (mode, asker, sorted(held))


def test_refusals_are_symmetric_but_for_the_listed_exceptions(golden):
    rows = golden["rows"]
    refused = {(r["asker"], tuple(r["held"])) for r in rows}
    n_mirrored = 0
    for r in rows:
        held = tuple(r["held"])
        if held in ASYMMETRIC or held[0] in ASYMMETRIC:
            continue
        assert len(held) == 1
        mine = FEATURE_OF[r["asker"]]
        for other, f in FEATURE_OF.items():
            if f == held[0]:
                assert (other, (mine,)) in refused, (r["asker"], held, other)
                n_mirrored += 1
    assert n_mirrored > 30
    assert [r for r in rows if tuple(r["held"]) == ("DOGLEG", "INNER_ITERATIONS")] == [r for r in rows if r["asker"] == "stba_ba_solve"]
    assert not any(r["when_clearing"] for r in rows if FEATURE_OF.get(r["asker"]) in ("LOSS", "INFORMATION", "POSE_PRIORS", "RELATIVE_POSES"))
    assert [(r["asker"], r["held"]) for r in rows if r["when_clearing"]] == [("stba_ba_set_allreduce", ["ITERATIVE_SCHUR"]),
                                                                             ("stba_ba_set_allreduce", ["DOGLEG"])]


# ------------------------------------------------------------------------------------------ poses and 6 x 6 weights
def golden_error(golden, who, case):
    (e,) = [e for e in golden["input_errors"] if e["who"] == who and e["case"] == case]
    return e["code"], e["text"]


WHO = {"the pose": ("stba_ba_set_pose_priors", "prior"), "the measurement": ("stba_ba_set_relative_poses", "edge")}


@pytest.mark.parametrize("what", sorted(WHO))
def test_pose_rows(runs, golden, what):
    res = runs["plain"][1]
    who, row = WHO[what]
    prefix = f"{who}: {row} 1: "
    get = lambda k: res[("pose7", what, k)]
    for k in ("valid", "one_plus_4_eps"):
        r = get(k)
        assert r["rc"] == 0 and r["why"] == ""
    assert np.array_equal(floats(get("one_plus_4_eps")["out"]), POSES["one_plus_4_eps"]), "unit to 8 eps: the bits are kept"
    assert floats(get("one_plus_5_eps")["out"])[3] == 1.0 and get("one_plus_5_eps")["rc"] == 0
    # (an input that is unit to 8 eps in n^2 keeps its bits, so its norm is within 4 eps; one that is scaled comes out within 2 eps)
    for k, bound in (("valid", 4 * EPS), ("norm_3", 2 * EPS)):
        out = floats(get(k)["out"])
        n = np.sqrt(np.sum(out[:4].astype(np.longdouble) ** 2))
        print(f"pose7 {k}: | |q| - 1 | = {abs(float(n - 1)) / EPS:.3f} eps")
        assert get(k)["rc"] == 0 and abs(float(n - 1)) <= bound and np.array_equal(out[4:], T3)
    q = np.array(POSES["norm_3"][:4])
    assert np.allclose(floats(get("norm_3")["out"])[:4], q / 3.0, rtol=4 * EPS, atol=0)
    for k, case in (("nan", "nan_pose"), ("zero_quaternion", "zero_quaternion")):
        assert (get(k)["rc"], prefix + get(k)["why"]) == golden_error(golden, who, case)
        assert get(k)["rc"] == INV


def test_sqrt_information_rows(runs, golden):
    res = runs["plain"][1]
    get = lambda k: res[("sqrt6", k)]
    r = get("valid_information")
    assert r["rc"] == 0 and r["direct_ok"] and r["W"] == r["direct"], "the bits of prior_information_factor called directly"
    W = floats(r["W"]).reshape(6, 6)
    assert np.allclose(W.T @ W, SQRT6["valid_information"][1], rtol=0, atol=1e-13) and np.all(np.tril(W, -1) == 0)
    for k in ("valid_sqrt", "rank_deficient_sqrt"):
        assert get(k)["rc"] == 0 and np.array_equal(floats(get(k)["W"]).reshape(6, 6), SQRT6[k][1]), k
    assert get("neither")["rc"] == 0 and np.array_equal(floats(get("neither")["W"]).reshape(6, 6), np.eye(6))
    for who, row in WHO.values():
        for k, code in (("inf_sqrt", INV), ("inf_information", INV), ("indefinite_information", NPD)):
            assert (get(k)["rc"], f"{who}: {row} 1: " + get(k)["why"]) == golden_error(golden, who, k)
            assert get(k)["rc"] == code
    assert not get("indefinite_information")["direct_ok"] and not get("inf_information")["direct_ok"]


def test_information6_factor_against_the_50_digit_factor(runs):
    mp = mp_ref.mp
    res = runs["plain"][1]
    for k, Om in FACTOR6_GOOD.items():
        r = res[("factor6", k)]
        assert r["rc"] == 0 and r["direct_ok"] and r["W"] == r["direct"], k
        W = floats(r["direct"]).reshape(6, 6)
        assert np.all(np.tril(W, -1) == 0) and np.all(np.diag(W) > 0), k
        assert mp.mp.dps == 50
        Wm, Am = mp.matrix(W.tolist()), mp.matrix(Om.tolist())
        back = max(abs((Wm.T * Wm)[a, b] - Am[a, b]) for a in range(6) for b in range(a + 1))      # (the lower triangle is what is factored)
        W50 = mp_ref.chol6_T(Om)
        rel = lambda X: max(float(abs(mp.mpf(float(X[a, b])) - W50[a, b]) / abs(W50[a, b])) for a in range(6) for b in range(a, 6) if W50[a, b] != 0)
        assert all(W[a, b] == 0.0 for a in range(6) for b in range(a, 6) if W50[a, b] == 0), "a zero of the exact factor is a zero"
        fwd, fwd64 = rel(W), rel(np.linalg.cholesky(Om).T)
        print(f"information6_factor {k}: cond {np.linalg.cond(Om):.2e}  |W^T W - Omega| {float(back):.2e}  worst entry against the 50-digit factor "
              f"{fwd / EPS:.2f} eps (an FP64 Cholesky: {fwd64 / EPS:.3g} eps)")
        assert np.abs(Om).max() <= 20.0, "the scale at which 1e-13 is the bound (spd6's)"
        assert float(back) <= 1e-13, k
        assert fwd <= FACTOR6_BOUND * EPS, (k, fwd / EPS)
        if k.startswith("cond_1e12"):
            assert np.linalg.cond(Om) > 5e11 and fwd64 > 1e6 * FACTOR6_BOUND * EPS, "an FP64 factorisation misses the bound here by far"
    for k, (Om, code) in FACTOR6_REFUSED.items():
        r = res[("factor6", k)]
        assert not r["direct_ok"] and r["rc"] == code, k


# ------------------------------------------------------------------------------------------ grouping
def csr_of(keys_sorted):
    start = np.flatnonzero(np.concatenate([[True], keys_sorted[1:] != keys_sorted[:-1]]))
    return np.append(start, len(keys_sorted)), keys_sorted[start]


@pytest.mark.parametrize("name", sorted(EDGES))
def test_grouping_against_a_stable_argsort(runs, name):
    res = runs["plain"][1]
    ci, cj = (np.array(a, np.int64) for a in EDGES[name])
    n = len(ci)
    # priors by camera: the key of reference k is ci[k]
    g = res[("group_cam", name)]
    order = np.argsort(ci, kind="stable")
    ptr, keys = csr_of(ci[order])
    assert np.array_equal(g["refs"], order) and np.array_equal(g["ptr"], ptr) and np.array_equal(g["keys"], keys)
    # edges by camera: reference 2 k + side, side 1 where the camera is the edge's j
    g = res[("group_edges", name)]
    cam_of = np.stack([ci, cj], 1).reshape(-1)
    order = np.argsort(cam_of, kind="stable")
    ptr, keys = csr_of(cam_of[order])
    assert np.array_equal(g["cg_ref"], order) and np.array_equal(g["cg_ptr"], ptr) and np.array_equal(g["cg_cam"], keys)
    assert len(g["cg_ref"]) == 2 * n
    # edges by unordered pair (hi, lo), ordered as pairs; the reference's side is 1 where hi is the edge's j
    hi, lo = np.maximum(ci, cj), np.minimum(ci, cj)
    key = hi * 1000 + lo
    order = np.argsort(key, kind="stable")
    ptr, keys = csr_of(key[order])
    assert np.array_equal(g["pg_ref"], 2 * order + (cj > ci)[order]) and np.array_equal(g["pg_ptr"], ptr)
    assert np.array_equal(g["pg_hi"], keys // 1000) and np.array_equal(g["pg_lo"], keys % 1000)


def test_the_grouping_cases_reach_their_branches():
    ci, cj = (np.array(a) for a in EDGES["a_pair_in_both_directions"])
    assert ((ci == 0) & (cj == 1)).sum() == 2 and ((ci == 1) & (cj == 0)).sum() == 1
    ci, cj = (np.array(a) for a in EDGES["a_camera_only_as_j"])
    assert 3 in cj and 3 not in ci
    ci, cj = (np.array(a) for a in EDGES["seventeen_over_five"])
    assert len(ci) == 17 and set(ci) | set(cj) == set(range(5)) and np.all(ci != cj) and np.any(np.diff(ci) < 0)


# ------------------------------------------------------------------------------------------ the 2 x 2 factor
def test_information_factor_2x2_within_four_eps_of_the_50_digit_factor(runs):
    res = runs["plain"][1]
    for kap in KAPPAS:
        Om = omega2(kap)
        assert I.chol2_mp(Om[None])[0] is not None, kap
        r = res[("info2", kap)]
        assert r["ok"], kap
        err = I.factor_error(floats(r["W"])[None], Om[None])
        print(f"ba_information_factor: kappa {kap:g}: worst entry error {err:.3f} eps")
        assert err <= 4.0, kap
    for k in INFO2_BAD:
        assert not res[("info2", k)]["ok"], k


@pytest.mark.parametrize("kind", ["asan_ubsan", "tsan"])
def test_sanitized_driver_runs_clean(runs, kind):
    """(the fixture asserts exit code 0 and an empty stderr: a sanitizer report is neither)"""
    assert runs[kind] == runs["plain"]
