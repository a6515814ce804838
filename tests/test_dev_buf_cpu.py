"""DevBuf, the one owner of device memory (slam-tricks_amd/csrc/common.hpp), and the loss-table check both set_loss entry points
share (robust_loss.hpp), in a stand-alone driver (tests/cpp/test_dev_buf.cpp) that defines hipMalloc / hipFree itself over malloc /
free: every address is tracked, a double free ends the run, and the library's live count must equal the table's size at every step.
The driver is built plain and with the address + undefined-behaviour sanitizers; both runs must end with status 0 and say nothing
on stderr (a sanitizer report is neither)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]}


@pytest.mark.parametrize("kind", sorted(SANITIZERS))
def test_dev_buf_driver_runs_clean(tmp_path, kind):
    exe = str(tmp_path / ("test_dev_buf_" + kind))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", *SANITIZERS[kind], "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "cpp", "test_dev_buf.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "dev_buf ok" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])
    assert p.stderr == "", p.stderr[-2000:]
