"""ceres::LandmarkPriorFactor of include/stba/ceres.h without a device (tests/cpp/test_ba_landmark_prior_shim.cpp, its host mode):
Evaluate against tests/ba_landmark_prior_ref.py (the float64 restatement in every bit, the 50-digit values within the GPU test's
bound), the recognition (BaStructure sets the blocks aside and keeps the observation -> residual-block map; a block with a loss, on
a 3-block no observation names or on a camera's position block is not taken) and the route decision, which needs no device:
"gpu-ba" under the default options, ITERATIVE_SCHUR and DOGLEG, a refusal for use_inner_iterations, and the dense callback route --
not "gpu-ba-hostjac" -- where the observations are a user's own cost functions."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ba_landmark_prior_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    pkg = os.path.join(ROOT, "slam-tricks_amd")
    exe = str(tmp_path_factory.mktemp("landmark_prior_shim") / "test_ba_landmark_prior_shim")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_ba_landmark_prior_shim.cpp"), "-L", pkg, "-lstba", f"-Wl,-rpath,{pkg}", "-lpthread",
                    "-o", exe], check=True)

    def run(cases):
        text = [str(len(cases))]
        for pos, p, W in cases:
            Wm = np.eye(3) if W is None else np.asarray(W, float).reshape(3, 3)
            text.append(" ".join(repr(float(v)) for v in np.concatenate([pos, p])) + f" {0 if W is None else 1} " +
                        " ".join(repr(float(v)) for v in Wm.reshape(-1)))
        out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.strip().split("\n")
        vals = [np.array([float(v) for v in line.split()]) for line in out[:len(cases)]]
        return [(v[:3], v[3:].reshape(3, 3)) for v in vals], out[len(cases):]
    return run


def test_evaluate_is_the_reference(shim):
    rng = np.random.default_rng(31)
    p = rng.normal(size=3)
    tight = np.array([[1e6, -1e6, 0.0], [0.0, 1e6, -1e6], [1e6, 0.0, -1e6]])
    height = np.zeros((3, 3)); height[0, 2] = 50.0
    cases = [(rng.normal(size=3), rng.normal(size=3), rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-2, 2)) for _ in range(6)]
    cases += [(p + 1e-3 * (1.0 + 1e-9 * rng.normal(size=3)), p, tight), (rng.normal(size=3), p, height), (rng.normal(size=3), p, None), (p, p, tight)]
    got, _ = shim(cases)
    worst = 0.0
    for (pos, x, W), (r, J) in zip(cases, got):
        Wm = np.eye(3) if W is None else W
        rn, Jn = R.lp_eval_np(pos, x, Wm)
        assert np.array_equal(r, rn) and np.array_equal(J, Jn)
        rm, Jm = R.lp_eval_mp(pos, x, Wm)
        er, eJ = R.err_vs_mp(r, J, rm, Jm)
        fl = R.floor_r(pos, x, Wm)
        assert np.all(eJ == 0.0)
        worst = max(worst, float(np.max(np.where(fl > 0, er / np.where(fl > 0, fl, 1.0), np.where(er == 0, 0.0, np.inf)))))
    print(f"LandmarkPriorFactor::Evaluate against 50 digits: worst err / (4 eps sum |W||r|) {worst:.3f}")
    assert worst <= 1.0
    assert np.array_equal(got[-1][0], np.zeros(3))


def test_recognition_and_routes(shim):
    _, lines = shim([])
    assert lines[0] == "detect 1 1 0 0 0 1", lines[0]
    routes = {}
    for line in lines[1:]:
        head, why = line.split(" | ") if " | " in line else (line.rstrip(" |"), "")
        _, variant, option, stage, path = head.split()
        routes[(variant, option)] = (int(stage), path, why.strip())
    GO, LOSS, INNER = 0, 1, 3
    for option in ("default", "iterative", "dogleg"):
        assert routes[("lp", option)] == (GO, "gpu-ba", ""), (option, routes[("lp", option)])
    stage, _, why = routes[("lp", "inner")]
    assert stage == INNER and "inner iterations with LandmarkPriorFactor blocks are not implemented" in why
    assert all(routes[("loss", option)][0] == LOSS for option in ("default", "iterative", "dogleg", "inner"))
    # the shape-only recognition does not take these blocks: nothing is dropped, the factor evaluates itself on the dense route
    assert routes[("user_plain", "default")][:2] == (GO, "gpu-ba-hostjac")
    assert routes[("user", "default")][:2] == (GO, "gpu-dense-callback") and routes[("user", "iterative")][:2] == (GO, "gpu-dense-callback")
    assert routes[("user", "dogleg")][0] != GO and routes[("user", "inner")][0] != GO


def test_evaluate_is_not_contracted_where_the_target_has_fma(tmp_path):
    """g++ -mfma contracts by default; LandmarkPriorFactor::Evaluate must not be (compiled to assembly, never run), and with the guard
    taken away the same compiler does contract"""
    def fused(*flags):
        out = tmp_path / f"probe{len(flags)}.s"
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-S", "-DPROBE_CERES", *flags, "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", "ba_landmark_prior_fma_probe.cpp"), "-o", str(out)])
        return sum(1 for line in out.read_text().splitlines() if line.strip().startswith("vfm"))
    assert fused() == 0
    assert fused("-DSTBA_CERES_NO_CONTRACT=") > 0
