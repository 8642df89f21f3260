"""GPU: every kNN kernel against the exact host search on tie-laden inputs.

`genie_knn` picks one of three kernels by the sizes -- a lane per query (`k_knn_t<8|10>`: at least 16 384 queries, k <= 10), a workgroup
per query (`k_knn_b<8|10>`: at most 64 queries, at least 4 096 context points, k <= 10), a wave per query (`k_knn<8|10|16>`: the rest) --
and `genie_knn_indexed` has a fourth (`k_knn_ix<8|10|16>`). Each keeps and orders lists of (float64 distance, index) pairs; on random
clouds no two distances are equal and the tie rule (smaller index first) is never used. Here every list is full of exactly equal
distances: integer lattices with queries on the points, at cell centres, edge midpoints and face centres and far outside, the same at
ECEF magnitude, every point three times, all points identical (tests/knn_tie_cases.py; tests/test_knn_ties_cpu.py shows how tie-laden
they are). Every assertion is exact equality with `knn_tie_cases.exact_knn`, a float64 stable argsort on the host; one reference per
input, at the largest k, whose first k columns are the table of every smaller k (a stable argsort; test_knn_ties_cpu.py checks it).
Every case runs a second time through a `KnnIndex`, compared with the host search as well, not with the brute-force kernel.

The shapes are the smallest that reach each kernel; `kernel_of` restates the dispatch of `genie_knn` so that a case says which kernel
it means and fails if the shape would no longer reach it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from genie_amd import _lib, engine
from tests import knn_tie_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INDEXED = pytest.mark.parametrize("indexed", [False, True], ids=["brute", "indexed"])


def kernel_of(n_context, n_query, k):
    """The kernel `genie_knn` runs for these sizes (genie_hip.hip, genie_knn)."""
    if n_query >= 16384 and k <= 10:
        return "k_knn_t"
    if n_query <= 64 and n_context >= 4096 and k <= 10:
        return "k_knn_b"
    return "k_knn"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _inputs(name):
    if name in ("lattice", "ecef", "triples"):
        xc = {"lattice": lambda: C.lattice(12)[0], "ecef": lambda: C.lattice_ecef(12)[0], "triples": lambda: C.triples(6)[0]}[name]()
        return xc, C.big_queries(name == "ecef")
    if name.startswith("identical"):                             # identical<n_context>x<n_query>
        nc, nq = name[len("identical"):].split("x")
        return C.identical(int(nc), int(nq))
    if name == "lattice16":                                      # 4 096 context points, 64 queries over the five families
        xc, xq = C.lattice(16)
        return xc, np.ascontiguousarray(xq[_five_families(xq, 64)])
    raise KeyError(name)


def _five_families(xq, n):
    """Row numbers: `n` queries of `lattice(m)`'s query set, the five families in turn."""
    m = xq.shape[0] // 5
    pick = np.random.default_rng(16).permutation(m)[:n]
    return (np.arange(n) % 5) * m + pick


@functools.lru_cache(maxsize=None)
def case(name, rows=None, k_ref=16):
    """(context, queries) on the device, the `KnnIndex` of the context, and the host table at `k_ref`; `rows`: "mixed" cuts the query
    set to 1 000 rows over all families (the last 37, the outside rows, among them), "one" to a single row."""
    xc, xq = _inputs(name)
    if rows == "mixed":
        xq = np.ascontiguousarray(xq[C.mixed_rows(xq.shape[0], 1000, 37)])
    elif rows == "one":
        xq = np.ascontiguousarray(xq[7:8])
    dxc = _t(xc)
    return dxc, _t(xq), engine.KnnIndex(dxc), C.exact_knn(xc, xq, k_ref)


def compare(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        raise AssertionError("%s: %s" % (what, C.explain(got, want)))


def check(name, k, indexed, kernel, rows=None, k_ref=16):
    dxc, dxq, index, want = case(name, rows, k_ref)
    assert kernel_of(dxc.shape[0], dxq.shape[0], k) == kernel
    got = engine.knn_device(dxc, dxq, k, index=index if indexed else None)
    compare(got, want[:, :k], "%s %s k=%d %s" % (name, rows or "all", k, "k_knn_ix" if indexed else kernel))


# ---- a lane per query ---------------------------------------------------------------------------------------------------------------


@INDEXED
@pytest.mark.parametrize("k", [1, 3, 8, 9, 10])
@pytest.mark.parametrize("name", ["lattice", "ecef", "triples"])
def test_lane_per_query(name, k, indexed):
    """16 384 + 37 queries (the threshold and a partial last workgroup) against the 12^3 lattice (one LDS tile), the same at ECEF
    magnitude, and the 6^3 lattice with every point three times. k = 3 takes the first three of a K = 8 list, 9 and 10 the K = 10
    instantiation."""
    check(name, k, indexed, "k_knn_t")


@INDEXED
@pytest.mark.parametrize("n_context", [300, 2049])
def test_lane_per_query_all_points_identical(n_context, indexed):
    """Every candidate ties with the worst of a full list: the first k indices stay. 2 049 is one point past an LDS tile."""
    name = "identical%dx16384" % n_context
    for k in (1, 3, 8, 9, 10):
        check(name, k, indexed, "k_knn_t", k_ref=10)
    assert np.array_equal(case(name, None, 10)[3], np.tile(np.arange(10, dtype=np.int32), (16384, 1)))


@functools.lru_cache(maxsize=None)
def self_case():
    """The 26^3 lattice (17 576 points) as its own query set; the host table by the integer form of the reference (squared distances
    of small integers are exact either way; test_knn_ties_cpu.py pins it to `exact_knn`)."""
    xc = C.lattice(26)[0]
    dxc = _t(xc)
    return dxc, engine.KnnIndex(dxc), C.exact_knn_integers(xc.astype(np.int64), 10)


@INDEXED
def test_lane_per_query_exclude_self(indexed):
    dxc, index, want = self_case()
    assert kernel_of(dxc.shape[0], dxc.shape[0], 10) == "k_knn_t"
    for k in (8, 10):
        got = engine.knn_device(dxc, dxc, k, exclude_self=True, index=index if indexed else None)
        compare(got, want[:, :k], "lattice(26) exclude_self k=%d %s" % (k, "k_knn_ix" if indexed else "k_knn_t"))
    if not indexed:
        tab, edges = engine.knn_graph_device(dxc, 8)
        compare(tab, want[:, :8], "knn_graph_device lattice(26) k=8")
        n = dxc.shape[0]
        assert edges.dtype == torch.int64 and tuple(edges.shape) == (2, n * 8)
        assert np.array_equal(edges[0].cpu().numpy(), want[:, :8].reshape(-1).astype(np.int64))
        assert np.array_equal(edges[1].cpu().numpy(), np.repeat(np.arange(n), 8))


@INDEXED
def test_lane_per_query_fewer_context_points_than_k(indexed):
    """The C entry keeps k as asked (the host wrapper clamps it): 5 identical context points, k = 10, rows `0 1 2 3 4 -1 -1 -1 -1 -1`."""
    xc, xq = C.identical(5, 16384)
    dxc, dxq = _t(xc), _t(xq)
    lib = _lib.load()
    got = torch.full((16384, 10), -7, dtype=torch.int32, device=DEV)
    if indexed:
        index = engine.KnnIndex(dxc)
        _lib.check(lib.genie_knn_indexed(engine._ptr(index.cell_start), engine._ptr(index.records), ctypes.byref(index._plan), 5,
                                         engine._ptr(dxq), 16384, 10, 0, engine._ptr(got), engine._stream()))
    else:
        _lib.check(lib.genie_knn(engine._ptr(dxc), 5, engine._ptr(dxq), 16384, 10, 0, engine._ptr(got), engine._stream()))
    want = C.exact_knn(xc, xq, 10)
    assert want[0].tolist() == [0, 1, 2, 3, 4, -1, -1, -1, -1, -1]
    compare(got, want, "5 identical context points, k=10")


# ---- a wave per query ---------------------------------------------------------------------------------------------------------------


@INDEXED
@pytest.mark.parametrize("k", [1, 8, 10, 15, 16])
@pytest.mark.parametrize("name", ["lattice", "ecef", "triples"])
def test_wave_per_query(name, k, indexed):
    """The same inputs cut to 1 000 queries over all families: k_knn<8>, <10> and <16>."""
    check(name, k, indexed, "k_knn", rows="mixed")


@INDEXED
@pytest.mark.parametrize("name", ["lattice", "ecef", "triples"])
def test_wave_per_query_k16_of_the_large_set(name, indexed):
    """At k = 16 the 16 384 + 37 queries stay with a wave per query (the lane-per-query kernel stops at k = 10)."""
    check(name, 16, indexed, "k_knn")


@INDEXED
def test_wave_per_query_all_points_identical(indexed):
    """4 099 equal context points: every lane's private list is all ties, and so is every round of the wave-wide minimum."""
    for k in (1, 8, 10, 15, 16):
        check("identical4099x257", k, indexed, "k_knn")


@INDEXED
def test_wave_per_query_exclude_self(indexed):
    """The 12^3 lattice against itself at k = 15, the k of the source base graph."""
    xc = C.lattice(12)[0]
    dxc, _, index, _ = case("lattice", "mixed")
    assert kernel_of(1728, 1728, 15) == "k_knn"
    got = engine.knn_device(dxc, dxc, 15, exclude_self=True, index=index if indexed else None)
    compare(got, C.exact_knn(xc, xc, 15, exclude_self=True), "lattice(12) exclude_self k=15")


def test_wave_per_query_fewer_context_points_than_k():
    """5 identical context points through the C entry at k = 10 and k = 16: after five rounds the wave-wide minimum is the empty slot,
    which every lane pops at once; rows `0 1 2 3 4 -1 ...`, nothing of the pre-filled table left."""
    xc, xq = C.identical(5, 257)
    dxc, dxq = _t(xc), _t(xq)
    lib = _lib.load()
    for k in (10, 16):
        assert kernel_of(5, 257, k) == "k_knn"
        got = torch.full((257, k), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.genie_knn(engine._ptr(dxc), 5, engine._ptr(dxq), 257, k, 0, engine._ptr(got), engine._stream()))
        want = C.exact_knn(xc, xq, k)
        assert want[0].tolist() == [0, 1, 2, 3, 4] + [-1] * (k - 5)
        compare(got, want, "5 identical context points, k=%d k_knn" % k)


# ---- a workgroup per query ----------------------------------------------------------------------------------------------------------


@INDEXED
@pytest.mark.parametrize("k", [1, 8, 10])
@pytest.mark.parametrize("rows", [None, "one"], ids=["64", "1"])
@pytest.mark.parametrize("name", ["lattice16", "identical4099x64"])
def test_workgroup_per_query(name, rows, k, indexed):
    """64 queries over the five families, and a single query, against the 16^3 lattice (4 096 points, the smallest context the kernel
    takes) and against 4 099 equal points: 16 waves' lists of ties, merged by wave 0."""
    check(name, k, indexed, "k_knn_b", rows=rows, k_ref=10)


# ---- through the model ---------------------------------------------------------------------------------------------------------------


def test_query_table_on_a_lattice_with_the_switch_off_and_on():
    """`SpatialAttention.query_table` of the 16 384 + 37 lattice queries against a 500-point piece of the lattice (the 8^3 lattice less
    twelve points, shuffled), `knn_index` off and on: both are the host table, and therefore each other."""
    from tests.test_knn_index_gpu import setup
    s = setup()
    net, att = s.net, s.net.SpatialAttention
    xc = C.lattice(8)[0][:500]
    xq = C.big_queries()
    want = C.exact_knn(xc, xq, 10)
    d = C.exact_knn_sorted_distances(xc, xq, C.exact_knn(xc, xq, 11))
    assert C.tie_shares(d, 10)[0] > 0.3
    dxc, dxq = _t(xc), _t(xq)
    try:
        tables = []
        for on in (False, True):
            net.knn_index = on
            att.invalidate_query_cache()
            tables.append(att.query_table(dxq, dxc).clone())
            assert (att._context_index is not None) == on
            compare(tables[-1], want, "query_table, knn_index %s" % on)
        assert torch.equal(tables[0], tables[1])
    finally:
        net.knn_index = False
        att.invalidate_query_cache()
