"""Pose-graph covariance, the part that needs no device: the C ABI's symbols and defaults, and the gauge refusal -- a connected
component without a constant node makes J^T J exactly singular, and stba_pg_covariance / stba_pg_covariance_columns refuse it through
stba_pg_gauge_check before they touch the device (an engine itself cannot exist without one, so the check is called directly here;
tests/test_gpu_pg_covariance.py sees the same refusal from the two entry points with `out` untouched)."""
import ctypes as C
import importlib

import numpy as np
import pytest

STBA_ERR_INVALID_ARGUMENT = -1
STBA_ERR_NOT_POSITIVE_DEFINITE = -4


@pytest.fixture(scope="module")
def st():
    return importlib.import_module("slam-tricks_amd")


def test_symbols_are_exported_and_version_is_unchanged(st):
    L = st.lib()
    for name in ("stba_pg_covariance", "stba_pg_covariance_columns", "stba_pg_covariance_default_options", "stba_pg_gauge_check"):
        assert hasattr(L, name), name
        assert name in st.EXPORTS
    assert L.stba_version() == 6


def test_default_options(st):
    o = st.PGCovarianceOptions()
    st.lib().stba_pg_covariance_default_options(C.byref(o))
    assert o.struct_size == C.sizeof(st.PGCovarianceOptions)
    assert o.relative_tolerance == 1e-12
    assert o.max_iterations == 0            # 6 x the number of free nodes
    assert o.check_every == 4
    assert hasattr(st.PGEngine, "covariance") and hasattr(st.PGEngine, "covariance_columns")


def chain(lo, hi):
    return list(range(lo, hi - 1)), list(range(lo + 1, hi))


def test_graph_without_a_constant_node_is_refused(st):
    ei, ej = chain(0, 7)
    for fixed in (None, np.zeros(7, np.uint8)):
        with pytest.raises(st.StbaError) as err:
            st.pg_gauge_check(7, ei, ej, fixed)
        assert err.value.code == STBA_ERR_NOT_POSITIVE_DEFINITE
        assert "component of 7 nodes" in str(err.value) and "first node 0" in str(err.value)
    fixed = np.zeros(7, np.uint8); fixed[4] = 1
    st.pg_gauge_check(7, ei, ej, fixed)          # one constant node anywhere in the component is enough


def test_component_without_a_constant_node_is_refused(st):
    a, b = chain(0, 6)
    c, d = chain(6, 10)
    ei, ej = a + c, b + d                        # {0..5} and {6..9}
    fixed = np.zeros(10, np.uint8); fixed[0] = 1
    with pytest.raises(st.StbaError) as err:
        st.pg_gauge_check(10, ei, ej, fixed)
    assert err.value.code == STBA_ERR_NOT_POSITIVE_DEFINITE
    assert "component of 4 nodes" in str(err.value) and "first node 6" in str(err.value)
    fixed[8] = 1
    st.pg_gauge_check(10, ei, ej, fixed)
    # a node no edge touches is a component of its own
    with pytest.raises(st.StbaError) as err:
        st.pg_gauge_check(11, ei, ej, np.append(fixed, 0))
    assert "component of 1 node " in str(err.value) and "first node 10" in str(err.value)


def test_null_engine_is_refused_and_out_untouched(st):
    out = np.full(36, 7.0)
    a = np.zeros(1, np.int32)
    rc = st.lib().stba_pg_covariance(None, 1, st._p(a), st._p(a), None, st._p(out), None)
    assert rc == STBA_ERR_INVALID_ARGUMENT and np.all(out == 7.0)
    out = np.full(36, 7.0)
    rc = st.lib().stba_pg_covariance_columns(None, 0, None, st._p(out), None)
    assert rc == STBA_ERR_INVALID_ARGUMENT and np.all(out == 7.0)
