"""CPU: the C ABI of the device builder of the association heads' time-pointer tables (genie_time_pointers and its scratch size) --
declared in the header, bound in `_lib.SYMBOLS` with the header's argument types, exported by the built library -- and the argument
errors `engine.time_pointers_device` / `set_adjacencies_base(time_pointers=)` raise before anything touches a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from genie_amd import _lib, engine, module


def _declared(header, ret, name):
    m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), header)
    assert m, "%s is not declared in genie_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_time_pointer_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    assert _declared(header, "size_t", "genie_time_pointers_scratch_bytes") == ["int64_t n_prod", "int n_sta", "int n_t"]
    assert _declared(header, "int", "genie_time_pointers") == [
        "const float* trv", "int64_t n_prod", "int n_sta", "const int32_t* sta_of_prod", "const double* dt_partition", "int n_t", "int k",
        "void* scratch", "int32_t* edges_p", "int32_t* edges_s", "int32_t* status", "void* stream"]
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert bound.get("genie_time_pointers_scratch_bytes") == (ctypes.c_size_t, [L, I, I])
    assert bound.get("genie_time_pointers") == (I, [P, L, I, P, P, I, I, P, P, P, P, P])
    lib = _lib.load()
    for name in ("genie_time_pointers_scratch_bytes", "genie_time_pointers"):
        assert getattr(lib, name).restype is not None


def test_scratch_size_and_host_side_refusals_of_the_entry():
    """The size function is host arithmetic and the entry refuses out-of-contract arguments before any launch: neither needs a device."""
    lib = _lib.load()
    P, S, n_t = 200 * 10000, 200, 226
    nbytes = lib.genie_time_pointers_scratch_bytes(P, S, n_t)
    assert nbytes >= 16 * P + 4 * 2 * S * (2 * n_t + 3) and nbytes < 16 * P + (1 << 20)
    assert lib.genie_time_pointers_scratch_bytes(1 << 31, S, n_t) == 0           # P >= 2^31
    assert lib.genie_time_pointers_scratch_bytes(P, S, 1) == 0                   # n_t < 2
    one = ctypes.c_void_p(256)                                                   # (never dereferenced: every call below is refused)
    call = lambda n_prod, n_t_, k: lib.genie_time_pointers(one, n_prod, 4, None, one, n_t_, k, one, one, one, one, None)
    for args in ((400, 10, 0), (400, 10, 33), (400, 1, 10), (1 << 31, 10, 10), (402, 10, 10)):
        assert call(*args) != 0, args
        assert lib.genie_last_error()


@pytest.mark.parametrize("k", [0, 33])
def test_k_outside_1_to_32_is_a_value_error(k):
    assert engine.TIME_POINTERS_MAX_K == 32
    trv = np.zeros((6, 3, 2), dtype=np.float32)
    with pytest.raises(ValueError, match="k"):
        engine.time_pointers_device(trv, 3, max_t=5.0, k=k)


def test_a_station_of_pairs_without_a_product_node_is_a_value_error():
    pairs = np.array([[0, 2, 0, 2], [0, 0, 1, 1]])            # station 1 of 3 has no product node
    with pytest.raises(ValueError, match="without a product node"):
        engine.time_pointers_device(np.zeros((4, 2), dtype=np.float32), 3, max_t=5.0, pairs=pairs)


def test_tables_and_time_pointers_together_are_a_value_error():
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device="cpu")
    S, G = 3, 4
    z = torch.zeros(S * 6, dtype=torch.long)
    pos = torch.zeros(S, 3), torch.zeros(G, 3)
    kw = dict(tlatent=torch.zeros(S * G, 2), time_pointers=dict(max_t=5.0, dt=1.0, k=2, win=1.0))
    for tables in (dict(A_edges_p=z), dict(A_edges_s=z), dict(dt_partition=np.arange(3.0)), dict(A_edges_p=z, A_edges_s=z, dt_partition=np.arange(3.0))):
        with pytest.raises(ValueError, match="not both"):
            net.set_adjacencies_base(None, None, None, pos[0], pos[1], **tables, **kw)
    with pytest.raises(ValueError, match="tlatent"):
        net.set_adjacencies_base(None, None, None, pos[0], pos[1], time_pointers=kw["time_pointers"])
