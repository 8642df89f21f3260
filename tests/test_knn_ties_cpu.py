"""CPU: the tie-laden kNN inputs of tests/knn_tie_cases.py are what they claim to be, and `exact_knn` is the search it says it is.

tests/test_knn_ties_gpu.py compares device tables with `exact_knn` for exact equality and takes no tolerance; what has to be guarded
is that those comparisons are not vacuous. So, from the reference alone: the share of query rows whose k best hold a run of at least
three equal float64 distances (what the ordering step of a kernel has to get right), and the share with a tie across the k-th /
(k+1)-th boundary (what its accept step has to get right). These are conditions on the inputs, not measurements of any kernel."""
import functools

import numpy as np
import pytest

from tests import knn_tie_cases as C

KS = (8, 10, 16)
K_REF = 17                      # one reference per input: the first k columns of a stable argsort are the table of every k <= 17


@functools.lru_cache(maxsize=None)
def reference(name, n):
    xc, xq = getattr(C, name)(n)
    idx = C.exact_knn(xc, xq, K_REF)
    return xc, xq, idx, C.exact_knn_sorted_distances(xc, xq, idx)


def shares(d, k, rows=slice(None)):
    d = d[rows]
    assert np.all(np.diff(d, axis=1) >= 0)
    return C.tie_shares(d, k)


@pytest.mark.parametrize("name,n", [("lattice", 6), ("lattice", 12), ("lattice_ecef", 12)])
def test_lattice_families_are_tie_laden(name, n):
    xc, xq, idx, d = reference(name, n)
    assert xc.shape == (n ** 3, 3) and xq.shape == (5 * n ** 3, 3) and xc.dtype == xq.dtype == np.float32
    m = n ** 3
    for k in KS:
        for i, fam in enumerate(C.FAMILIES):
            run3, boundary = shares(d, k, slice(i * m, (i + 1) * m))
            if fam == "out":
                assert run3 > 0 and boundary > 0, (fam, k, run3, boundary)
            else:
                assert run3 >= 0.95 and boundary > 0.2, (fam, k, run3, boundary)


def test_ecef_lattice_is_the_lattice_moved():
    """The ties exist in the fp32 coordinates themselves: the moved lattice has the table of the lattice at the origin."""
    assert np.array_equal(reference("lattice_ecef", 12)[2], reference("lattice", 12)[2])
    xc = C.lattice_ecef(12)[0].astype(np.float64)
    assert np.array_equal((xc - np.array([C.ECEF_ORIGIN])) / C.ECEF_SPACING, C.lattice(12)[0].astype(np.float64))


def test_index_order_is_unrelated_to_position():
    xc = C.lattice(12)[0]
    ints = C.lattice_integers(12)
    assert sorted(map(tuple, xc.astype(np.int64))) == sorted(map(tuple, ints)) and not np.array_equal(xc, ints)
    t = C.triples(6)[0]
    pts, counts = np.unique(t, axis=0, return_counts=True)
    assert pts.shape[0] == 216 and np.all(counts == 3)
    first = {}
    for i, p in enumerate(map(tuple, t)):
        first.setdefault(p, []).append(i)
    gaps = np.array([np.diff(v).min() for v in first.values()])
    assert np.median(gaps) > 20                                  # the three copies of a point are not neighbours in index


@pytest.mark.parametrize("n", [6, 12])
def test_triples_come_in_threes(n):
    xc, xq, idx, d = reference("triples", n)
    assert xc.shape == (3 * n ** 3, 3)
    for k in KS:
        assert shares(d, k)[0] >= 0.95
    assert np.all(d[:, 0] == d[:, 2]) and np.all(d[:, 3] == d[:, 5])


@pytest.mark.parametrize("n_context", [300, 2049, 4099])
def test_identical_context_is_all_ties(n_context):
    xc, xq = C.identical(n_context)
    assert np.all(xc == xc[0]) and np.array_equal(xq[0], xc[0]) and not np.array_equal(xq[1], xc[0])
    idx = C.exact_knn(xc, xq, K_REF)
    assert np.array_equal(idx, np.tile(np.arange(K_REF, dtype=np.int32), (xq.shape[0], 1)))
    d = C.exact_knn_sorted_distances(xc, xq, idx)
    for k in KS:
        assert shares(d, k) == (1.0, 1.0)


def test_the_large_query_set_is_tie_laden_against_the_small_contexts():
    """The 16 384 + 37 queries the lane-per-query cases use come from a 16^3 lattice laid over the 12^3 context with two steps outside
    on every side. At least (11 / 16)^3 = 0.32 of every in-box family lie inside the context's box, where they are rows of
    `lattice(12)`'s own families (run share >= 0.95): more than 0.3 of the rows hold a run of three. Measured here it is far more, the
    outside rows being lattice-aligned too; the figures are printed."""
    xq = C.big_queries()
    assert xq.shape == (C.N_BIG, 3) and C.N_BIG % 256 == 37
    for xc in (C.lattice(12)[0], C.triples(6)[0]):
        idx = C.exact_knn(xc, xq, 11)
        d = C.exact_knn_sorted_distances(xc, xq, idx)
        for k in (8, 10):
            run3, boundary = shares(d, k)
            print("n_context %d k %d: rows with a run >= 3 %.3f, with a boundary tie %.3f" % (xc.shape[0], k, run3, boundary))
            assert run3 > 0.3 and boundary > 0
        assert shares(d[16384:], 8)[0] > 0                       # the 37 outside rows as well
    assert np.array_equal(C.big_queries(True), (xq.astype(np.float64) * C.ECEF_SPACING + np.array([C.ECEF_ORIGIN])).astype(np.float32))


def test_exact_knn_against_lexsort():
    """300 rows of every family against an independent ordering: `np.lexsort((index, distance))` per row."""
    for name, n in (("lattice", 6), ("lattice", 12), ("lattice_ecef", 12), ("triples", 6)):
        xc, xq, idx, _ = reference(name, n)
        rows = C.mixed_rows(xq.shape[0], 300, 20, seed=n)
        c = xc.astype(np.float64)
        for r in rows:
            d = ((xq[r].astype(np.float64)[None, :] - c) ** 2).sum(-1)
            assert np.array_equal(idx[r], np.lexsort((np.arange(c.shape[0]), d))[:K_REF]), (name, n, r)


def test_exact_knn_options():
    """`exclude_self`, fewer candidates than k (-1), the prefix property the tests lean on, and the integer form used for the large
    self-search."""
    xc, xq = C.lattice(6)
    full = C.exact_knn(xc, xc, 16)
    assert np.array_equal(full[:, 0], np.arange(216))            # a point is its own nearest neighbour (distance 0, unique)
    ex = C.exact_knn(xc, xc, 15, exclude_self=True)
    assert np.array_equal(ex, full[:, 1:])
    for k in (1, 3, 8, 9, 10, 15):
        assert np.array_equal(C.exact_knn(xc, xq[:400], k), C.exact_knn(xc, xq[:400], 16)[:, :k])
    five = C.identical(5)[0]
    few = C.exact_knn(five, xq[:50], 10)
    assert np.array_equal(few, np.tile(np.array([0, 1, 2, 3, 4, -1, -1, -1, -1, -1], dtype=np.int32), (50, 1)))
    assert np.array_equal(C.exact_knn(five, five, 10, exclude_self=True)[2], [0, 1, 3, 4, -1, -1, -1, -1, -1, -1])
    ints = xc.astype(np.int64)
    assert np.array_equal(C.exact_knn_integers(ints, 10), C.exact_knn(xc, xc, 10, exclude_self=True))
    assert np.array_equal(C.exact_knn_integers(ints, 10, exclude_self=False), full[:, :10])
    old = C._CHUNK_BYTES
    try:                                                         # several chunks, a partial last one
        C._CHUNK_BYTES = 8 * 216 * 50
        assert np.array_equal(C.exact_knn(xc, xc, 15, exclude_self=True), ex)
        assert np.array_equal(C.exact_knn_integers(ints, 10), C.exact_knn(xc, xc, 10, exclude_self=True))
    finally:
        C._CHUNK_BYTES = old
