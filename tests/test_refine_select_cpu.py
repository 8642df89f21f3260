"""CPU: the host half of the refined-source selection and of the source-parallel passes (genie_amd/apply.py): the C ABI symbol is
declared, bound and exported; `source_parallel` is validated before anything touches a device and cuts the source list with
`window_blocks`; `refined_from_found` finishes a pass from its fixed-size rows; the linear-index rule the kernel reduces with is the
nested first-maximum argmax (numpy restatement)."""
import os
import re
import types

import numpy as np
import pytest

from genie_amd import _lib, apply


def _legs(sharded=False):
    return [types.SimpleNamespace(net=types.SimpleNamespace(is_sharded=sharded))]      # no device: the checks come first


def test_refine_select_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    for name, ret in (("genie_refine_select", "int"), ("genie_refine_select_scratch_bytes", "size_t")):
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), header), "%s is not declared in genie_hip.h" % name
        assert name in {n for n, _, _ in _lib.SYMBOLS}, "%s is not in _lib.SYMBOLS" % name
        assert getattr(_lib.load(), name).restype is not None
    n = _lib.load().genie_refine_select_scratch_bytes()
    assert n > 0 and n % 16 == 0


@pytest.mark.parametrize("bad", [(2, 2), (-1, 2), (0, 0), (0, -3), (5, 3)])
def test_source_parallel_rank_and_world_are_validated_first(bad):
    srcs = np.zeros((4, 5))
    with pytest.raises(ValueError):
        apply.refine_sources(_legs(), None, srcs, None, None, 1.0, None, None, 10, None, None, None, None, None, ftrns2_device=lambda x: x,
                             source_parallel=bad)
    with pytest.raises(ValueError):
        apply.associate_sources(_legs(), None, srcs, None, None, 1.0, None, None, None, source_parallel=bad)
    with pytest.raises(ValueError):
        apply.detect_refine_associate(_legs(), None, None, None, None, None, None, None, 1.0, None, None, None, None, None, None, None, 10,
                                      0.1, 5.0, 0.75, 15.0, 6.75, 20e3, source_parallel=bad)


def test_source_parallel_refusals():
    srcs = np.zeros((4, 5))
    with pytest.raises(NotImplementedError, match="source_parallel on a source-node-sharded model"):
        apply.refine_sources(_legs(True), None, srcs, None, None, 1.0, None, None, 10, None, None, None, None, None, source_parallel=(0, 2))
    with pytest.raises(NotImplementedError, match="source_parallel"):
        apply.associate_sources(_legs(True), None, srcs, None, None, 1.0, None, None, None, source_parallel=(0, 2))
    with pytest.raises(NotImplementedError, match="source_parallel"):
        apply.detect_refine_associate(_legs(True), None, None, None, None, None, None, None, 1.0, None, None, None, None, None, None, None,
                                      10, 0.1, 5.0, 0.75, 15.0, 6.75, 20e3, source_parallel=(0, 1))
    with pytest.raises(ValueError, match="ftrns2_device"):         # the ranks exchange the device branch's rows
        apply.refine_sources(_legs(), None, srcs, None, None, 1.0, None, None, 10, None, None, None, None, None, source_parallel=(0, 2))
    with pytest.raises(ValueError, match="process group"):         # a tuple has no transport between the two passes
        apply.detect_refine_associate(_legs(), None, None, None, None, None, None, None, 1.0, None, None, None, None, None, None, None, 10,
                                      0.1, 5.0, 0.75, 15.0, 6.75, 20e3, source_parallel=(1, 2))


class _Reached(Exception):
    pass


def test_source_parallel_cuts_the_source_list_with_window_blocks(monkeypatch):
    calls = []

    def recorder(n, world):
        calls.append((n, world))
        raise _Reached()

    monkeypatch.setattr(apply, "window_blocks", recorder)
    with pytest.raises(_Reached):
        apply.refine_sources(_legs(), None, np.zeros((7, 5)), None, None, 1.0, None, None, 10, None, None, None, None, None,
                             ftrns2_device=lambda x: x, source_parallel=(1, 3))
    with pytest.raises(_Reached):
        apply.associate_sources(_legs(), None, np.zeros((5, 5)), None, None, 1.0, None, None, None, source_parallel=(0, 4))
    assert calls == [(7, 3), (5, 4)]


def test_refined_from_found_finishes_a_pass():
    rng = np.random.default_rng(3)
    n, tq = 6, np.arange(-3.0, 3.75, 0.75)
    srcs = np.c_[rng.uniform(0, 1, (n, 3)), rng.uniform(100.0, 101.0, n), np.full(n, 0.5)]
    found = np.c_[rng.integers(0, 50, n), rng.integers(0, 9, n), rng.uniform(0, 1, n), np.ones(n), rng.uniform(0, 9, (n, 3))].astype(np.float64)
    got, order = apply.refined_from_found(found, srcs, tq.reshape(-1, 1), lambda x: 2.0 * x)
    want = np.c_[2.0 * found[:, 4:7], srcs[:, 3] + tq[found[:, 1].astype(int)], found[:, 2]]
    assert np.array_equal(order, np.argsort(want[:, 3])) and np.array_equal(got, want[order])
    # the rows of the ranks, side by side in rank order, are the rows of one GPU: any cut gives the same end
    for world in (2, 5, 8):
        parts = [found[lo:hi] for lo, hi in apply.window_blocks(n, world)]
        again, order2 = apply.refined_from_found(np.concatenate(parts), srcs, tq, lambda x: 2.0 * x)
        assert np.array_equal(again, got) and np.array_equal(order2, order)
    found[2, 3] = 0.0
    with pytest.raises(ValueError, match="source 2"):
        apply.refined_from_found(found, srcs, tq, lambda x: x)
    empty, o = apply.refined_from_found(np.zeros((0, 7)), np.zeros((0, 5)), tq, lambda x: x)
    assert empty.shape == (0, 5) and o.shape == (0,)


def test_smallest_linear_index_of_the_maximum_is_the_nested_first_argmax():
    """What the kernel's reduction relies on: among the elements equal to the global maximum, the one of smallest q * n_t + t is
    (argmax of the row maxima, argmax of that row), first maximum in both -- on tie-rich data, with masked rows."""
    rng = np.random.default_rng(11)
    for Q, T in ((1, 1), (5, 2), (64, 9), (257, 21)):
        for _ in range(20):
            acc = (rng.integers(0, 4, (Q, T)) / 8.0).astype(np.float32)
            keep = rng.random(Q) < 0.7
            if not keep.any():
                continue
            m = np.where(keep[:, None], acc, -np.inf)
            ip = int(np.argmax(m.max(1)))
            it = int(np.argmax(m[ip]))
            lin = int(np.flatnonzero(m.reshape(-1) == m.max())[0])
            assert (ip, it) == divmod(lin, T)
