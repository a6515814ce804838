"""The Levenberg-Marquardt step policy (slam-tricks_amd/csrc/lm_policy.hpp) shared by the BA engine, the pose graph and the dense
loop: the stop tests, acceptance, the trust-region radius and the trace rows, compiled with g++ and run on the host (no device)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lm_policy(tmp_path):
    exe = str(tmp_path / "test_lm_policy")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_lm_policy.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "lm_policy ok" in p.stdout, p.stdout[-2000:]
