"""The front door's routing (include/stba/ceres.h) without a device: every case of ceres_route_cases.py through
tests/cpp/ceres_routes_driver.cpp, against what the header did before its routing was rewritten
(tests/golden/ceres_routes_nodevice.json): every refusal, every message and stderr line, which route was taken, the parameters'
bits, and no more calls of the user's Evaluate than before.  Engines cannot be created here, so every accepted case ends in the
engine's "no HIP device" failure -- after the whole recognition and route decision, which is what this checks."""
import importlib

import pytest

import ceres_route_cases as C


def test_cases_are_well_formed():
    names = [c.split()[0] for c in C.cases()]
    assert len(names) == len(set(names)) and list(C.golden("nodevice")) == names and list(C.golden("gpu")) == names


def test_every_refusal_of_the_routing_is_recorded():
    """each text the routing can refuse with is produced by at least one recorded case (the engine-side failures that need a
    broken device are not)"""
    texts = [v["message"] for which in ("nodevice", "gpu") for v in C.golden(which).values()]
    for needle in ("carry a LossFunction; robust losses are not implemented by this layer (the reference",
                   "SUBSPACE_DOGLEG is not implemented", "DOGLEG only supports exact factorization", "DOGLEG with CameraRelativePoseFactor",
                   "DOGLEG with PosePriorFactor", "DOGLEG is implemented for bundle adjustment", "inner iterations are not implemented with DOGLEG",
                   "inner_iteration_tolerance must be >= 0", "inner iterations with CameraRelativePoseFactor", "inner iterations with PosePriorFactor",
                   "inner iterations are implemented for bundle adjustment on the gpu-ba path only", "not on gpu-ba-hostjac (force_callback_path)",
                   "names a pointer that is not a parameter block", "the rotation and the position of camera", "share a residual",
                   "cost functions are not the reprojection factor (gpu-ba-hostjac)", "weighted ReprojectionFactors (sqrt_information)",
                   "CLUSTER_JACOBI, CLUSTER_TRIDIAGONAL or SUBSET", "not implemented on the gpu-ba-hostjac path (LossFunction)",
                   "solved again with the user's Evaluate.", "The second solve ran without inner iterations", "recognised as the reprojection factor",
                   "nothing to optimise", "limited to 4096 local parameters and 2.7e8 Jacobian entries; use ReprojectionFactor",
                   "stba_ba_create: ", "stba_ba_set_sqrt_information: ", "stba_ba_set_loss: ", "stba_ba_set_relative_poses (relative pose factors): ",
                   "stba_ba_set_pose_priors: ", "stba_pg_create: ", "stba_pg_set_sqrt_information: ", "stba_pg_set_loss: ", "stba_dense_solve: ",
                   "no covariance computed", "this layer has no pseudo-inverse", "names a parameter block that is not in the problem",
                   "LocalParameterization::ComputeJacobian failed", "need Covariance::Options::bundle_adjustment_cross_blocks = true",
                   "no residual block of the bundle adjustment uses", "no residual block of the pose graph uses", "stba_pg_covariance: ",
                   "stba_ba_covariance_compute: ", "stba_dense_covariance: ", "nothing to compute", "2.7e8 Jacobian entries"):
        assert any(needle in t for t in texts), needle


def test_routes_without_a_device(tmp_path):
    st = importlib.import_module("slam-tricks_amd")
    if st.device_count() > 0:
        pytest.skip("a device is present: test_gpu_ceres_routes.py compares against the record made on one")
    exe = C.build_driver(str(tmp_path / "ceres_routes_driver"))
    C.compare(C.run_driver(exe, tmp_path), C.golden("nodevice"), bitwise=False)


def test_routes_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same driver as a stand-alone program built with -fsanitize=address,undefined (the header is all of the code under test;
    libstba.so is linked as it is): no report, and the same record"""
    st = importlib.import_module("slam-tricks_amd")
    if st.device_count() > 0:
        pytest.skip("a device is present: the device runtime's own allocations are not this test's subject")
    exe = C.build_driver(str(tmp_path / "ceres_routes_driver_san"), extra_flags=("-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    C.compare(C.run_driver(exe, tmp_path), C.golden("nodevice"), bitwise=False)
