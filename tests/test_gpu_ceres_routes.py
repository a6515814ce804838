"""The front door's routing (include/stba/ceres.h) on the device: every case of ceres_route_cases.py through
tests/cpp/ceres_routes_driver.cpp, against the record made with the header as it was before its routing was rewritten
(tests/golden/ceres_routes_gpu.json, same library).  Strings exactly; Evaluate counts at most the recorded ones; iteration counts and
final costs (for Covariance: the sum of the requested blocks) in every bit -- the library and the sequence of C-ABI calls are the
same, and the record itself repeats bit for bit from run to run."""
import pytest

import ceres_route_cases as C


@pytest.mark.gpu
def test_routes_on_the_device(tmp_path):
    exe = C.build_driver(str(tmp_path / "ceres_routes_driver"))
    C.compare(C.run_driver(exe, tmp_path), C.golden("gpu"), bitwise=True)
