"""CPU: the host half of the batched refine pass (`apply.refine_sources(source_batch=)`, `module.flush_windows_clouds`): the three new
C ABI symbols are declared, bound and exported with matching argument counts; `source_batch` / `refine_batch` and the query-set table
are validated, and a sharded leg is refused, before anything touches a device."""
import os
import re
import types

import numpy as np
import pytest

from genie_amd import _lib, apply, module

NEW = ("genie_tail_batched_q", "genie_refine_select_batch", "genie_refine_cloud_batch")


def _legs():
    return [types.SimpleNamespace(net=types.SimpleNamespace(is_sharded=False))]        # no device: the checks come first


def _refine(legs, **kw):
    return apply.refine_sources(legs, None, np.zeros((4, 5)), None, None, 1.0, None, None, 10, None, None, None, None, None, **kw)


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    lib = _lib.load()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m, "%s is not declared in genie_hip.h" % name
        assert name in bound, "%s is not in _lib.SYMBOLS" % name
        assert len(bound[name]) == len(m.group(1).split(",")), "%s: the binding and the header disagree on the argument count" % name
        assert getattr(lib, name).restype is not None
    # the shared body keeps the old entry point's refusals under its own name, the new one adds its own, all before any launch
    assert lib.genie_tail_batched_q(None, 0, 1, None, 1, None, None, None, 5, 10, None, 9, None, None, None, None, None) == -1
    assert b"genie_tail_batched_q: null query-set table" in lib.genie_last_error()
    assert lib.genie_refine_select_batch(None, 0, 2, 10, 9, None, 2.0, None, None, None) == -1
    assert b"genie_refine_select_batch: 1 <= n_batch" in lib.genie_last_error()
    assert lib.genie_refine_select_batch(None, 2, 33, 10, 9, None, 2.0, None, None, None) == -1
    assert lib.genie_refine_cloud_batch(1, 2, 0, 0, 10, None, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, None, None, None) == -1
    assert b"genie_refine_cloud_batch: 1 <= n_batch" in lib.genie_last_error()
    assert lib.genie_refine_cloud_batch(1, 2, 0, 3, 10, None, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, None, None, None) == -1
    assert b"null argument" in lib.genie_last_error()
    assert lib.genie_refine_cloud_batch(1, 2, 0, 3, 0, None, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, None, None, None) == 0      # nothing to draw


@pytest.mark.parametrize("bad", [0, 17, 2.5, -1, True, "4", None])
def test_source_batch_outside_its_range_is_refused(bad):
    with pytest.raises(ValueError, match="source_batch"):
        _refine(_legs(), ftrns2_device=lambda x: x, source_batch=bad)
    with pytest.raises(ValueError, match="source_batch"):
        apply.detect_refine_associate(_legs(), None, None, None, None, None, None, None, 1.0, None, None, None, None, None, None, None, 10,
                                      0.1, 5.0, 0.75, 15.0, 6.75, 20e3, ftrns2_device=lambda x: x, refine_batch=bad)


def test_a_batch_needs_the_device_transform():
    with pytest.raises(ValueError, match="source_batch > 1 needs ftrns2_device"):
        _refine(_legs(), source_batch=2)
    with pytest.raises(ValueError, match="needs ftrns2_device"):
        apply.detect_refine_associate(_legs(), None, None, None, None, None, None, None, 1.0, None, None, None, None, None, None, None, 10,
                                      0.1, 5.0, 0.75, 15.0, 6.75, 20e3, refine_batch=2)
    assert apply._check_source_batch(1, None) == 1 and apply._check_source_batch(np.int64(16), len) == 16


def test_a_sharded_leg_is_refused_with_the_message_of_push_window():
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device="cpu", shard=(0, 2))
    with pytest.raises(NotImplementedError) as pushed:
        net._not_sharded("push_window / flush_windows (batched tails; use forward_fixed_source_pipelined)")
    with pytest.raises(NotImplementedError, match="is not available on a source-node-sharded model") as refused:
        _refine([types.SimpleNamespace(net=net)], ftrns2_device=lambda x: x, source_batch=2)       # (no device, no picks: refused first)
    assert str(refused.value).split(" is not available ")[1] == str(pushed.value).split(" is not available ")[1]
    assert "source_batch" in str(refused.value)


def test_the_query_set_table_is_checked_on_the_host():
    got = module.checked_qset([2, 0, 2], 3, 3)
    assert got.dtype == np.int32 and got.tolist() == [2, 0, 2] and got.flags["C_CONTIGUOUS"]
    assert module.checked_qset(np.array([1, 0], dtype=np.int64)[::-1], 2, 2).tolist() == [0, 1]
    assert module.checked_qset([], 0, 1).shape == (0,)
    for bad, n, sets in (([0, 1], 3, 2), ([0, 1, 1, 0], 3, 2), ([0, 2], 2, 2), ([-1, 0], 2, 2), ([0.0, 1.0], 2, 2), ([[0, 1]], 2, 2),
                         (0, 1, 1)):
        with pytest.raises(ValueError, match="qset"):
            module.checked_qset(bad, n, sets)
