"""CPU: the C ABI of the cell-index kNN (genie_knn_index_plan / genie_knn_index_build / genie_knn_indexed: declared in the header, bound
in `_lib.SYMBOLS`, exported by the cross-compiled library), the host-only plan through ctypes, and the arguments the host refuses before
anything reaches a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from genie_amd import _lib, engine

INDEX_SYMBOLS = ("genie_knn_index_plan", "genie_knn_index_build", "genie_knn_indexed")
MAX_CELLS = 1 << 20
ERR_ARG = -1


def plan_of(n, lo, hi):
    lib = _lib.load()
    bbox = (ctypes.c_float * 6)(*(list(lo) + list(hi)))
    plan = _lib.KnnIndexPlan()
    rc = lib.genie_knn_index_plan(int(n), bbox, ctypes.byref(plan))
    return rc, plan


def test_index_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in INDEX_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in genie_hip.h"
        assert name in bound, name + " is not in _lib.SYMBOLS"
        assert getattr(lib, name).restype is not None
    assert "genie_knn_index_plan_t" in header
    assert ctypes.sizeof(_lib.KnnIndexPlan) == 80                    # the header's struct: 12 four-byte fields, a double, three int64


BOXES = [((0, 0, 0), (100e3, 100e3, 40e3)), ((-1, -1, -1), (1, 1, 1)), ((6.3e6, 6.3e6, 6.3e6), (6.4e6, 6.4e6, 6.4e6)),
         ((0, 0, 0), (1e-3, 1e6, 1e6)), ((0, 0, 0), (1e30, 1e-20, 3.0)), ((-4e37, -4e37, -4e37), (4e37, 4e37, 4e37)),
         ((0, 0, 0), (1e-35, 1e-35, 1.0))]


@pytest.mark.parametrize("n", [1, 9, 4099, 10000, 50000, 2000000, 2**31 - 1])
@pytest.mark.parametrize("box", BOXES)
def test_plan_counts_and_sizes(n, box):
    rc, p = plan_of(n, *box)
    assert rc == 0
    cells = [int(c) for c in p.cells]
    assert all(c >= 1 for c in cells)
    assert cells[0] * cells[1] * cells[2] == p.n_cells <= MAX_CELLS
    assert p.cell_start_bytes == 4 * (p.n_cells + 1) and p.records_bytes == 16 * n and p.scratch_bytes == 4 * p.n_cells
    assert [float(o) for o in p.origin] == [float(np.float32(v)) for v in box[0]]
    assert p.inv_cell > 0 and math.isfinite(p.inv_cell) and p.cell == 1.0 / float(p.inv_cell)
    for a in range(3):                                               # the cells cover the box (up to the rounding the kernels clamp away)
        assert cells[a] * p.cell >= (float(np.float32(box[1][a])) - float(np.float32(box[0][a]))) * (1 - 1e-6) or p.n_cells == MAX_CELLS \
            or cells[a] == 1


def test_plan_mean_occupancy_is_a_small_constant():
    for n in (4099, 10000, 50000):
        rc, p = plan_of(n, (0, 0, 0), (100e3, 80e3, 40e3))
        assert rc == 0 and 1.0 <= n / p.n_cells <= 8.0, (n, p.n_cells)


@pytest.mark.parametrize("axes", [(0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)])
def test_plan_zero_extent_axis_gets_one_cell(axes):
    lo, hi = [5.0, -7.0, 1e6], [50e3, 70e3, 1.1e6]      # (an axis much shorter than the cell edge gets one cell too: none here)
    for a in axes:
        hi[a] = lo[a]
    rc, p = plan_of(4099, lo, hi)
    assert rc == 0
    for a in range(3):
        assert (p.cells[a] == 1) == (a in axes), (axes, list(p.cells))


def test_plan_refuses_bad_arguments():
    inf, nan = float("inf"), float("nan")
    assert plan_of(0, (0, 0, 0), (1, 1, 1))[0] == ERR_ARG
    assert plan_of(10, (0, 0, 0), (1, inf, 1))[0] == ERR_ARG
    assert plan_of(10, (-inf, 0, 0), (1, 1, 1))[0] == ERR_ARG
    assert plan_of(10, (0, 0, nan), (1, 1, 1))[0] == ERR_ARG
    assert plan_of(10, (0, 0, 0), (1, 1, -1))[0] == ERR_ARG
    assert plan_of(10, (-3e38, 0, 0), (3e38, 1, 1))[0] == ERR_ARG        # x - origin would overflow fp32
    lib = _lib.load()
    assert lib.genie_knn_index_plan(10, None, ctypes.byref(_lib.KnnIndexPlan())) == ERR_ARG
    assert b"genie_knn_index_plan" in lib.genie_last_error()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    plan = _lib.KnnIndexPlan()
    assert lib.genie_knn_index_build(None, 10, None, ctypes.byref(plan), None, None, None, None) == ERR_ARG
    assert lib.genie_knn_indexed(None, None, ctypes.byref(plan), 10, None, 1, 3, 0, None, None) == ERR_ARG
    buf = (ctypes.c_float * 72)()                                    # host memory: every call below must return before touching it
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)          # 16-byte aligned, as the entry asks of the records
    for k in (0, 17):
        assert lib.genie_knn_indexed(p, p, ctypes.byref(plan), 10, p, 1, k, 0, p, None) == ERR_ARG
    assert lib.genie_knn_indexed(p, p, ctypes.byref(plan), 10, p, 1, 3, 0, p, None) == ERR_ARG           # an all-zero plan
    rc, good = plan_of(10, (0, 0, 0), (1, 1, 1))
    assert rc == 0
    assert lib.genie_knn_indexed(p, p, ctypes.byref(good), 11, p, 1, 3, 0, p, None) == ERR_ARG           # a plan for another n_context
    assert lib.genie_knn_index_build(p, 11, p, ctypes.byref(good), p, p, p, None) == ERR_ARG
    assert lib.genie_knn_indexed(p, p, ctypes.byref(good), 10, p, 0, 3, 0, p, None) == 0                 # no query: nothing to do
    odd = ctypes.c_void_p(p.value + 4)
    assert lib.genie_knn_indexed(p, odd, ctypes.byref(good), 10, p, 0, 3, 0, p, None) == ERR_ARG         # misaligned records
    for field, value in (("cell", good.cell * 1.5), ("inv_cell", good.inv_cell * 2), ("n_cells", good.n_cells + 1)):
        edited = _lib.KnnIndexPlan.from_buffer_copy(good)                                                # a plan edited by the caller
        setattr(edited, field, value)
        assert lib.genie_knn_indexed(p, p, ctypes.byref(edited), 10, p, 0, 3, 0, p, None) == ERR_ARG, field
    edited = _lib.KnnIndexPlan.from_buffer_copy(good)
    edited.origin[1], edited.upper[1] = 1.0, 0.0                                                         # origin above upper
    assert lib.genie_knn_indexed(p, p, ctypes.byref(edited), 10, p, 0, 3, 0, p, None) == ERR_ARG


class UnbuiltIndex(engine.KnnIndex):
    """A KnnIndex without its device buffers: what the host checks before a search needs no device."""

    def _build(self):
        pass


def test_host_refuses_before_the_device():
    xc, xq = torch.zeros(20, 3), torch.zeros(5, 3)
    idx = UnbuiltIndex(xc)
    assert idx.n_context == 20 and idx.matches(xc) and idx.calls == 0
    for k in (0, -1, 17):
        with pytest.raises(ValueError, match="1 <= k <= 16"):
            engine.knn_device(xc, xq, k, index=idx)
    with pytest.raises(ValueError, match="1 <= k <= 16"):
        engine.knn_device(torch.zeros(1, 3), xq, 1, exclude_self=True, index=UnbuiltIndex(torch.zeros(1, 3)))
    for bad in (torch.zeros(20, 2), torch.zeros(20), torch.zeros(20, 3, 1)):
        with pytest.raises(ValueError, match=r"\[n, 3\]"):
            engine.knn_device(bad, xq, 3, index=idx)
        with pytest.raises(ValueError, match=r"\[n, 3\]"):
            engine.knn_device(xc, bad, 3, index=idx)
        with pytest.raises(ValueError, match=r"\[n, 3\]"):
            engine.KnnIndex(bad)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        engine.KnnIndex(torch.zeros(0, 3))
    with pytest.raises(ValueError, match="another context"):       # another tensor with the same contents
        engine.knn_device(xc.clone(), xq, 3, index=idx)
    with pytest.raises(ValueError, match="another context"):       # another shape on the same storage
        engine.knn_device(xc[:10], xq, 3, index=idx)
    xc.add_(1.0)                                                     # the same tensor, rewritten in place
    assert not idx.matches(xc)
    with pytest.raises(ValueError, match="another context"):
        engine.knn_device(xc, xq, 3, index=idx)
    assert idx.calls == 0


def test_switches_default_off():
    import inspect
    from genie_amd import apply, module
    assert inspect.signature(apply.GridLeg.__init__).parameters["knn_index"].default is False
    assert inspect.signature(engine.knn_device).parameters["index"].default is None
    att = module.SpatialAttention(30, 30, 3, 15)
    assert att.knn_index is False
    assert isinstance(module.GCN_Detection_Network_extended.knn_index, property)
    assert engine.KNN_INDEX_MIN_QUERIES == 16384
