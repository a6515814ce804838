"""The reference of the camera-to-camera relative-pose factors (tests/ba_between_ref.py) checked against itself, and the host code
against it, without a device:
  - the float64 restatement against the 50-digit evaluation on the edge grid of the GPU test; its worst error in units of
    eps sum |W_jk||entry_k| is printed and pinned under C_FLOOR, the yardstick of the header and of the device;
  - the Jacobians of the issue's formulas against central differences at 50 digits, and against the problem's own plus;
  - slam-tricks_amd/csrc/ba_between.hpp compiled with g++ (tests/cpp/ba_between_driver.cpp) on the same grid, under the bound of
    ba_between_ref's docstring; negating any quaternion leaves every bit;
  - ceres::CameraRelativePoseFactor::Evaluate (tests/cpp/test_ba_between_shim.cpp, host mode) composed with the chart, and DetectBa;
  - the solve cases of the GPU test (each reference converges, no rho near the threshold)."""
import os
import shutil
import subprocess

import mpmath as mp
import numpy as np
import pytest

import ba_between_ref as T
import ba_prior_ref as P
import lm_step_ref as L
import mp_ref as M

EPS = L.EPS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float64_restatement_against_50_digits_on_the_grid():
    g = T.grid()
    n = len(g["meas"])
    assert n == len(T.ANGLES) * len(T.NEGATE) * 2 * 2
    assert {nm.rsplit("/", 1)[1] for nm in g["names"]} == {f"{a}-{b}" for a, b in T.MASK_PAIRS}      # every pair of mask kinds occurs
    worst, at = 0.0, None
    for k in range(n):
        _, own, sc = T.grid_reference(k)
        for o, s in zip(own, sc):
            assert np.all(o[s == 0] == 0), g["names"][k]          # structural zeros and constant columns are exact
            q = float(np.max(o[s > 0] / s[s > 0])) if np.any(s > 0) else 0.0
            if q > worst:
                worst, at = q, g["names"][k]
    print(f"restatement: worst err / (eps sum |W||entry|) = {worst:.1f} at {at}; C_FLOOR = {T.C_FLOOR}")
    assert T.C_FLOOR / 2 < worst <= T.C_FLOOR          # (C_FLOOR is this figure rounded up to a power of two)


def test_negating_a_quaternion_leaves_the_restatements_bits():
    g = T.grid()
    for k in range(0, len(g["meas"]), 7):
        i, j = g["cam_i"][k], g["cam_j"][k]
        base = T.between_eval_np(g["meas"][k], g["cams"][i], g["cams"][j], g["W"][k])
        for which in range(3):
            a = [g["meas"][k].copy(), g["cams"][i].copy(), g["cams"][j].copy()]
            a[which][:4] = -a[which][:4]
            got = T.between_eval_np(*a, g["W"][k])
            assert all(np.array_equal(x, y) for x, y in zip(base, got)), (g["names"][k], which)
        if g["names"][k].startswith("0/"):
            r, _, Jj = T.between_eval_np(g["meas"][k], g["cams"][i], g["cams"][j], np.eye(6))
            assert np.array_equal(r[:3], np.zeros(3)) and np.array_equal(Jj[:3, :3], np.eye(3))


def test_the_angle_set_is_what_it_says():
    g = T.grid()
    for k in range(len(g["meas"])):
        name = g["names"][k].split("/")[0]
        (r, _, _) = T.between_eval_mp(g["meas"][k], g["cams"][g["cam_i"][k]], g["cams"][g["cam_j"][k]], np.eye(6))
        assert abs(M.norm(r[:3]) - P.angle_value(name)) <= 1e-15, (g["names"][k], M.norm(r[:3]))
        assert all(0.04 <= abs(x) <= 0.16 for x in r[3:])


@pytest.mark.parametrize("name", ["1e-8", "0.3", "1.5", "3.0", "pi-1e-6"])
@pytest.mark.parametrize("baseline", [0.05, 10.0])
def test_jacobians_against_central_differences_at_50_digits(name, baseline):
    """the issue's formulas (between_eval_mp builds them from the LU inverse of Jr) against (r(+h) - r(-h)) / 2h, h = 1e-20, under
    R <- R Exp(dtheta), t <- t + dt: truncation h^2 |r'''| ~ 1e-38 (x 1 / (pi - theta) near pi), well under 1e-25"""
    meas, ci, cj = T.grid_edge(name, "none", baseline, 50 + T.ANGLES.index(name))
    _, Ji, Jj = T.between_eval_mp(meas, ci, cj, np.eye(6))
    Ni, Nj = T.between_jacobians_numeric_mp(meas, ci, cj)
    err = max(max(abs(Ji[a, b] - Ni[a, b]), abs(Jj[a, b] - Nj[a, b])) for a in range(6) for b in range(6))
    print(f"angle {name} baseline {baseline}: analytic against numeric at 50 digits {float(err):.2e}")
    assert err <= mp.mpf("1e-25")


def test_jacobians_are_the_derivatives_under_the_problems_own_plus():
    """float64: r'(x (+) h e_a) - r'(x (-) h e_a) = 2 h J'[:, a] with (+) lm_step_ref.BAProblem.plus on the edge's two cameras"""
    c = T.case("a_chain")
    prob = T.problem("a_chain")
    x = prob.x0
    k = 2
    i, j = prob.bt_i[k], prob.bt_j[k]
    _, Ji, Jj = prob.lin_edges(prob.split(x)[0])
    assert not prob.cam_fixed[i].any() and not prob.cam_fixed[j].any()
    h = 1e-6
    for cam, J in ((i, Ji[k]), (j, Jj[k])):
        for a in range(6):
            d = np.zeros(prob.n_local); d[6 * cam + a] = h
            rp = prob.lin_edges(prob.split(prob.plus(x, d))[0], False)[0][k]
            rm = prob.lin_edges(prob.split(prob.plus(x, -d))[0], False)[0][k]
            num = (rp - rm) / (2 * h)
            assert np.allclose(num, J[:, a], rtol=0, atol=1e-7 * (1 + np.abs(J).max())), (cam, a, num, J[:, a])
    assert len(c["cam_i"]) == 7


def test_problem_pads_to_twelve_columns_and_appends_the_edge_rows():
    name = "c_chain_two_priors"
    prob = T.problem(name)
    c = T.case(name)
    base = P.PriorBAProblem(c["s"], c["priors"]["cams"], c["priors"]["poses"], P.sqrt_of_information(c["priors"]["information"]), cam_fixed=None)
    r0, J0, c0 = base.lin(base.x0)
    r, J, cols = prob.lin(prob.x0)
    n, nb = len(prob.bt_i), len(r0)
    assert J.shape == (nb + 3 * n, 2, 12) and cols.shape == (nb + 3 * n, 12) and len(r) == nb + 3 * n
    assert np.array_equal(r[:nb], r0) and np.array_equal(J[:nb, :, :9], J0) and np.all(J[:nb, :, 9:] == 0.0) and np.array_equal(cols[:nb, :9], c0)
    assert np.array_equal(cols[nb:, :6], np.repeat(6 * prob.bt_i[:, None] + np.arange(6), 3, axis=0))
    assert np.array_equal(cols[nb:, 6:], np.repeat(6 * prob.bt_j[:, None] + np.arange(6), 3, axis=0))
    # the padding changes nothing of the normal equations, and the edges' part of them is edge_blocks
    H0, g0 = L.normal_equations(base.n_local, r0, J0, c0)
    H1, g1 = L.normal_equations(prob.n_local, r[:nb], J[:nb], cols[:nb])
    assert np.array_equal(H0, H1) and np.array_equal(g0, g1)
    He, ge = L.normal_equations(prob.n_local, r[nb:], J[nb:], cols[nb:])
    H, g, Ha, ga, S = prob.edge_blocks(prob.x0)
    for cam in range(prob.nc):
        sl = slice(6 * cam, 6 * cam + 6)
        assert np.allclose(np.asarray(H[cam], float), np.asarray(He[sl, sl], float), rtol=1e-13, atol=1e-13 * float(np.abs(Ha[cam]).max()))
        assert np.allclose(np.asarray(g[cam], float), np.asarray(ge[sl], float), rtol=1e-13, atol=1e-13 * float(np.abs(ga[cam]).max()))
    for (hi, lo), (blk, ab) in S.items():
        assert hi > lo
        assert np.allclose(np.asarray(blk, float), np.asarray(He[6 * hi:6 * hi + 6, 6 * lo:6 * lo + 6], float), rtol=1e-13, atol=1e-13 * float(ab.max()))
    assert len(S) == n                                  # (a chain: every edge its own pair)
    want = base.cost(base.x0) + prob.edge_cost(prob.x0)
    assert abs(prob.cost(prob.x0) - want) <= 1e-14 * want


def test_the_disjoint_scene_has_a_pair_without_a_common_landmark():
    s, (a, b) = T.disjoint_scene()
    sh = T.shared_landmarks(s)
    assert sh[a, b] == 0 and sh[a, a] >= 4 and sh[b, b] >= 4
    assert not s["cam_fixed"][a].any() and not s["cam_fixed"][b].any()
    c = T.case("b_chain_loop_disjoint")
    assert (c["cam_i"][-1], c["cam_j"][-1]) == (b, a) and b > a


@pytest.mark.parametrize("name", T.SOLVE_CASES)
def test_every_solve_case_converges_away_from_the_acceptance_threshold(name):
    ref, o = T.reference(name), T.options(name)
    kap = max(it["kappa"] for it in ref)
    print(f"{name}: start cost {ref[0]['start']['cost']:.6g}, costs {[round(it['cost'], 8) for it in ref]}, rho {[round(it['rho'], 4) for it in ref]}, kappa {kap:.2e}")
    assert all(it["accepted"] for it in ref)
    assert ref[-1]["cost"] < 1e-1 * ref[0]["start"]["cost"] and ref[-1]["gmax"] < 1e-2 * ref[0]["start"]["gmax"]
    assert L.rho_margin_ok(ref, o)
    assert L.C_PATH["ba"] * kap * EPS <= 1e-6
    if name == "c_chain_two_priors":
        assert T.problem(name).free.all()


# ------------------------------------------------------------------------------- ba_between.hpp on the host
def _need_gxx():
    if shutil.which("g++") is None:
        pytest.skip("needs g++")


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    """the grid through tests/cpp/ba_between_driver.cpp: run(list of (meas, ci, cj, W, fixed_i, fixed_j)) -> list of (r', J_i', J_j')"""
    _need_gxx()
    exe = str(tmp_path_factory.mktemp("between") / "ba_between_driver")
    # (-ffp-contract=off: the header's `#pragma clang fp contract(off)` is clang's; -Wno-unknown-pragmas for the same reason)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cpp", "ba_between_driver.cpp"), "-o", exe])

    def run(edges):
        hexs = lambda a: " ".join(float(x).hex() for x in np.asarray(a, float).ravel())
        bits = lambda m: sum(int(bool(v)) << a for a, v in enumerate(m))
        text = [str(len(edges))] + [f"{hexs(z)} {hexs(ci)} {hexs(cj)} {hexs(W)} {bits(fi)} {bits(fj)}" for z, ci, cj, W, fi, fj in edges]
        p = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.returncode, p.stderr[-500:])
        out = []
        for line in p.stdout.strip().split("\n"):
            v = np.array([float.fromhex(w) for w in line.split()])
            assert np.array_equal(v[:6], v[78:84])          # the residual-only call: the same bits
            out.append((v[:6], v[6:42].reshape(6, 6), v[42:78].reshape(6, 6)))
        return out
    return run


def _grid_edges(negated=None):
    g = T.grid()
    edges = []
    for k in range(len(g["meas"])):
        i, j = g["cam_i"][k], g["cam_j"][k]
        z = g["meas"][k].copy()
        z[:4] = P.normalise_like_the_host(z[None, :4])[0]
        a = [z, g["cams"][i].copy(), g["cams"][j].copy()]
        if negated is not None:
            a[negated][:4] = -a[negated][:4]
        edges.append((*a, g["W"][k], g["cam_fixed"][i], g["cam_fixed"][j]))
    return edges


def test_the_header_on_the_host_against_50_digits(header):
    got = header(_grid_edges())
    g = T.grid()
    worst, at = 0.0, None
    for k, e in enumerate(got):
        q = T.worst_ratio(k, e)
        if q > worst:
            worst, at = q, g["names"][k]
    print(f"ba_between.hpp on the host: worst err / bound {worst:.3f} at {at}")
    assert worst <= 1.0
    # what the restatement restates: the same operations in the same order, so the same bits
    same = sum(all(np.array_equal(x, y) for x, y in zip(e, T.between_eval_np(*a))) for e, a in zip(got, _grid_edges()))
    print(f"  {same} of {len(got)} edges agree with the restatement in every bit")
    for which in range(3):
        neg = header(_grid_edges(which))
        for k, (a, b) in enumerate(zip(got, neg)):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (g["names"][k], which)


# ------------------------------------------------------------------------------- the host factor of include/stba/ceres.h
@pytest.fixture(scope="module")
def between_shim(tmp_path_factory):
    _need_gxx()
    pkg = os.path.join(ROOT, "slam-tricks_amd")
    exe = str(tmp_path_factory.mktemp("between_shim") / "test_ba_between_shim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_ba_between_shim.cpp"), "-L", pkg, "-lstba", f"-Wl,-rpath,{pkg}", "-lpthread",
                    "-o", exe], check=True)

    def run(cases):
        text = [str(len(cases))]
        for z, ci, cj, W in cases:
            Wm = np.eye(6) if W is None else np.asarray(W, float).reshape(6, 6)
            text.append(" ".join(repr(float(v)) for v in np.concatenate([z, ci, cj])) + f" {0 if W is None else 1} " +
                        " ".join(repr(float(v)) for v in Wm.reshape(-1)))
        out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.strip().split("\n")
        vals = [np.array([float(v) for v in line.split()]) for line in out[:len(cases)]]
        return [(v[:6], v[6:42].reshape(6, 6), v[42:78].reshape(6, 6)) for v in vals], out[len(cases)]
    return run


def test_ceres_camera_relative_pose_factor_against_the_restatement(between_shim):
    """the compiled host CameraRelativePoseFactor::Evaluate, its Jacobians composed with QuaternionRightPlus, against between_eval_np:
    the residual and the position columns in every bit (the same operations), the rotation columns to the composition's error: row i
    of the local Jacobian goes through P^+ (3 x 4) and P (4 x 3), two products of O(1) entries that mix its three rotation entries,
    8 eps (sum_k |W_ik||J_ka| + sum_b |J'_ib|); every quaternion negated in turn leaves the residual's bits"""
    g = T.grid()
    cases, idx = [], []
    for k in range(0, len(g["meas"]), 3):
        for W in (g["W"][k], None):
            cases.append((g["meas"][k], g["cams"][g["cam_i"][k]], g["cams"][g["cam_j"][k]], W))
            idx.append(k)
    got, detect = between_shim(cases)
    worst = 0.0
    for (z, ci, cj, W), (r, Ji, Jj) in zip(cases, got):
        Wm = np.eye(6) if W is None else W
        zn = z.copy(); zn[:4] = P.normalise_like_the_host(z[None, :4])[0]
        rr, Jir, Jjr = T.between_eval_np(zn, ci, cj, Wm)
        assert np.array_equal(r, rr)
        _, si, sj = T.scales(Wm, zn, ci, cj)
        for J, Jr, s in ((Ji, Jir, si), (Jj, Jjr, sj)):
            assert np.array_equal(J[:, 3:], Jr[:, 3:])             # (the position blocks' Jacobians pass through no chart)
            bound = 8 * s[:, :3] + 8 * EPS * np.abs(Jr[:, :3]).sum(1, keepdims=True)
            err = np.abs(J - Jr)[:, :3]
            assert np.all(err[bound == 0] == 0)
            if np.any(bound > 0):
                worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
    print(f"CameraRelativePoseFactor (host): Jacobians against the restatement, worst err / bound {worst:.3f}")
    assert worst <= 1.0
    neg = []
    for which in range(3):
        for z, ci, cj, W in cases[:16]:
            a = [z.copy(), ci.copy(), cj.copy()]
            a[which][:4] = -a[which][:4]
            neg.append((*a, W))
    got_neg, _ = between_shim(neg)
    for n, e in enumerate(got_neg):
        assert np.array_equal(e[0], got[n % 16][0]), n
    # DetectBa, without a device: no edge (as always; nothing of the bookkeeping is made) | an edge between two cameras, set aside with
    # the observations' arrays compact | refused: position blocks swapped, a camera no observation names, a LossFunction
    assert detect == "detect 1 1 0 0 0", detect
