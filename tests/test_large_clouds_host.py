"""CPU-side checks of the sort capacity (include/rrl.h rrl_sort_capacity): the library reports at least 2^20 triangles per
cloud, and the Python side takes its bound from there instead of a literal of its own.  No GPU needed."""
import inspect

import pytest


@pytest.fixture(scope="module")
def lib():
    from rrl_hip import build, _lib
    build.build_lib()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_library_sort_capacity(lib):
    assert lib.rrl_sort_capacity() >= 2 ** 20


def test_python_reads_the_library_capacity(lib):
    from rrl_hip import callsites, ops
    assert ops.sort_capacity() == lib.rrl_sort_capacity()
    assert not hasattr(callsites, "_SORT_CAP")
    for obj in (ops.cloud_order, ops._Step.__init__, ops._Chamfer.forward, callsites):
        src = inspect.getsource(obj)
        assert "65536" not in src and "sort_capacity()" in src, obj


def test_cloud_order_workspace_covers_the_capacity(lib):
    n = lib.rrl_sort_capacity()
    assert lib.rrl_cloud_order_workspace_bytes(1, n) >= 8 * n  # keys and indices of the padded power of two
    assert lib.rrl_chamfer_workspace_bytes(1, n, n) > 0
