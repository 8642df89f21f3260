"""CPU: the host side of saving and resuming the online objects -- the fingerprint comparison
(`checkpoint.fingerprint_diff` / `check_fingerprint`), the copy of a state to the host (`checkpoint.to_host`, here on CPU tensors), the
`PickStore` state round trip on a CPU store (a `PickStore` runs on the CPU, so this is the whole round trip: host arrays, the four
views and `meta`, then further appends and trims in step with the store that went on), and the two new C-ABI entries' declarations."""
import io
import os
import re

import numpy as np
import pytest
import torch

from genie_amd import _lib, apply, checkpoint

S_ALL = 30
IND_USE = np.random.default_rng(3).permutation(S_ALL)[:20]               # 10 stations are not the model's


def _chunk(rng, m, t_lo, t_hi, decimals=1):
    t = np.round(rng.uniform(t_lo, t_hi, m), decimals)                   # ties inside and across chunks
    return np.stack([t, rng.integers(0, S_ALL, m).astype(np.float64), rng.random(m), rng.random(m), rng.integers(0, 2, m).astype(np.float64)], axis=1)


def _same(store, ref):
    for f in ("t", "sta", "phase", "phase_f", "index"):
        a, b = getattr(store, f), getattr(ref, f)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f
    assert np.array_equal(store.t_host, ref.t_host) and np.array_equal(store.index_host, ref.index_host) and len(store) == len(ref)
    assert store.n_fed == ref.n_fed and store.frozen_t == ref.frozen_t
    assert np.array_equal(store.meta(store.index), ref.meta(ref.index))


def _through_torch_save(state):
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


# ---- the fingerprint ------------------------------------------------------------------------------------------------------------------------

def _fp():
    return {"tsteps_abs": np.arange(0.0, 10.0, 0.5), "times": np.array([1.0, 2.0]), "step_size": "half", "scale": 0.25, "tail_batch": 16,
            "ranges": (0.0, 60e3), "key": np.array([7, 0], dtype=np.uint64), "flag": True, "nothing": None}


def test_equal_fingerprints_agree_whatever_container_holds_the_numbers():
    own = _fp()
    saved = _through_torch_save(checkpoint.to_host(_fp()))
    assert checkpoint.fingerprint_diff(saved, own) is None
    saved["ranges"], saved["tsteps_abs"], saved["tail_batch"] = [0.0, 60e3], torch.arange(0.0, 10.0, 0.5, dtype=torch.float64), np.int64(16)
    assert checkpoint.fingerprint_diff(saved, own) is None
    checkpoint.check_fingerprint("X", {"fingerprint": saved}, own)


@pytest.mark.parametrize("name,value", [("tsteps_abs", np.arange(0.0, 10.0, 0.5) + 1e-9), ("tsteps_abs", np.arange(0.0, 10.5, 0.5)),
                                        ("times", np.array([1.0])), ("step_size", 1.0), ("step_size", "Half"), ("scale", 0.5),
                                        ("tail_batch", 1), ("ranges", (0.0, 61e3)), ("key", np.array([7, 1], dtype=np.uint64)),
                                        ("flag", False), ("flag", 1), ("nothing", 0.0)])
def test_the_first_differing_field_is_named(name, value):
    own, saved = _fp(), _fp()
    saved[name] = value
    saved["tail_batch"] = saved["tail_batch"] if name == "tail_batch" else 3             # a later difference: the FIRST one is named
    first = name if list(own).index(name) <= list(own).index("tail_batch") else "tail_batch"
    assert checkpoint.fingerprint_diff(saved, own) == first
    with pytest.raises(ValueError, match=r"X\.load_state_dict: .* another %s " % first):
        checkpoint.check_fingerprint("X", {"fingerprint": saved}, own)


def test_missing_and_extra_fields_and_a_state_without_fingerprint():
    own, saved = _fp(), _fp()
    del saved["scale"]
    assert checkpoint.fingerprint_diff(saved, own) == "scale"
    saved = dict(_fp(), more=1)
    assert checkpoint.fingerprint_diff(saved, own) == "more"
    for bad in (None, {}, {"fingerprint": 3}):
        with pytest.raises(ValueError, match="fingerprint"):
            checkpoint.check_fingerprint("X", bad, own)


def test_to_host_copies_and_keeps_dtype_shape_and_bytes():
    x = torch.arange(12, dtype=torch.int32).reshape(3, 4)[:, 1:3]        # a view: the copy is compact
    a = np.arange(5.0)
    state = {"a": a, "n": 3, "s": "half", "nested": [(x, a[:2]), {"y": torch.zeros(0, dtype=torch.float64)}]}
    out = checkpoint.to_host(state)
    assert out["n"] == 3 and out["s"] == "half" and isinstance(out["nested"][0], tuple)
    got = out["nested"][0][0]
    assert got.dtype == x.dtype and got.shape == x.shape and torch.equal(got, x) and got.data_ptr() != x.data_ptr()
    assert got.untyped_storage().nbytes() == 6 * 4
    assert out["a"] is not a and np.array_equal(out["a"], a) and out["nested"][1]["y"].shape == (0,)
    a[0] = -1.0
    x[0, 0] = -1
    assert out["a"][0] == 0.0 and int(got[0, 0]) == 1                   # the state does not alias the object


# ---- the PickStore ----------------------------------------------------------------------------------------------------------------------------

def _fed_store(capacity=8):
    """A store after merges, growth, a trim past half the capacity and a moved `frozen_t`: base > 0, a capacity above the default."""
    rng = np.random.default_rng(21)
    store = apply.PickStore(IND_USE, S_ALL, "cpu", capacity=capacity)
    for c in range(12):
        store.append(_chunk(rng, 12, 4.0 * c - 3.0, 4.0 * c + 6.0))      # every chunk reaches back below the resident tail
    store.frozen_t = 30.0
    store.trim(27.35)
    assert store._base > 0 and 0 < len(store) < store.n_fed and (store.t_host < store.frozen_t).any()
    return store, rng


@pytest.mark.parametrize("capacity", [4, 4096])
def test_pick_store_round_trip_and_both_stores_go_on_in_step(capacity):
    store, rng = _fed_store()
    state = store.state_dict()
    assert set(state) == {"fingerprint", "frozen_t", "n_fed", "t", "rows", "index"}
    assert all(isinstance(v, (float, int, np.ndarray, dict)) for v in state.values())
    loaded = _through_torch_save(state)
    new = apply.PickStore(IND_USE, S_ALL, "cpu", capacity=capacity)
    new.load_state_dict(loaded)
    _same(new, store)
    assert new._base == 0 and new.capacity >= len(store)
    state["t"][:] = -1.0                                                 # the state does not alias the saved store
    _same(new, store)
    late = _chunk(rng, 4, 40.0, 50.0)
    late[1, 0], late[1, 1] = 29.9, float(IND_USE[0])                     # older than the restored frozen_t
    for s in (store, new):
        with pytest.raises(ValueError, match="frozen_t = 30.0"):
            s.append(late)
    _same(new, store)
    for c in range(12, 20):                                              # appends (in order and merged), trims, compaction: in step
        P = _chunk(rng, 12, max(30.0, 4.0 * c - 3.0), 4.0 * c + 6.0)
        assert store.append(P) == new.append(P) == 0
        assert store.trim(4.0 * c - 12.0) == new.trim(4.0 * c - 12.0)
        _same(new, store)
        for t0 in (4.0 * c - 6.0, 4.0 * c - 1.0):
            assert np.subtract(*store.embed_range(t0, 5.0, 1.0)) == np.subtract(*new.embed_range(t0, 5.0, 1.0))


def test_an_empty_store_round_trips():
    store = apply.PickStore(IND_USE, S_ALL, "cpu")
    new = apply.PickStore(IND_USE, S_ALL, "cpu")
    new.load_state_dict(_through_torch_save(store.state_dict()))
    _same(new, store)
    assert len(new) == 0 and new.frozen_t == -np.inf


def test_pick_store_refusals_change_nothing():
    store, _ = _fed_store()
    state = store.state_dict()
    other = apply.PickStore(IND_USE[::-1].copy(), S_ALL, "cpu")          # the same stations in another order: another `sta`
    with pytest.raises(ValueError, match="station_map"):
        other.load_state_dict(state)
    no_phase = apply.PickStore(IND_USE, S_ALL, "cpu", use_phase_types=False)
    with pytest.raises(ValueError, match="use_phase_types"):
        no_phase.load_state_dict(state)
    bad = dict(state, t=state["t"][::-1].copy())
    fresh = apply.PickStore(IND_USE, S_ALL, "cpu")
    with pytest.raises(ValueError, match="time-sorted"):
        fresh.load_state_dict(bad)
    for s in (other, no_phase, fresh):
        assert len(s) == 0 and s.n_fed == 0 and s.frozen_t == -np.inf
    before = [getattr(store, f).clone() for f in ("t", "sta", "phase", "index")] + [store.n_fed, store.frozen_t]
    with pytest.raises(RuntimeError, match="has been fed"):
        store.load_state_dict(state)                                     # a store that has been fed
    after = [getattr(store, f) for f in ("t", "sta", "phase", "index")] + [store.n_fed, store.frozen_t]
    assert all(torch.equal(x, y) for x, y in zip(before[:4], after[:4])) and before[4:] == after[4:]


def test_use_phase_types_false_is_rebuilt_as_append_builds_it():
    rng = np.random.default_rng(5)
    store = apply.PickStore(IND_USE, S_ALL, "cpu", use_phase_types=False)
    store.append(_chunk(rng, 40, 0.0, 20.0))
    new = apply.PickStore(IND_USE, S_ALL, "cpu", use_phase_types=False)
    new.load_state_dict(store.state_dict())
    _same(new, store)
    assert int(new.phase.abs().sum()) == 0 and new.meta(new.index)[:, 4].sum() > 0     # the fed rows keep their phase column


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["genie_ring_save", "genie_ring_load"])
def test_ring_checkpoint_symbols_are_declared_bound_and_exported(name):
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, header), "%s is not declared in genie_hip.h" % name
    sig = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    assert name in sig, "%s is not in _lib.SYMBOLS" % name
    assert sig[name] == sig["genie_ring_close"]                          # (ring, n_query, ring_cols, c_lo, c_hi, block, stream) -> int
    fn = getattr(_lib.load(), name)
    assert fn.restype is sig[name][0] and list(fn.argtypes) == sig[name][1]


def test_ring_checkpoint_signatures_in_the_header():
    header = re.sub(r"\s+", " ", open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read())
    assert ("int genie_ring_save(const float* ring, int64_t n_query, int64_t ring_cols, int64_t c_lo, int64_t c_hi, float* out, "
            "void* stream);") in header
    assert ("int genie_ring_load(float* ring, int64_t n_query, int64_t ring_cols, int64_t c_lo, int64_t c_hi, const float* block, "
            "void* stream);") in header
