"""Tie-laden inputs of the kNN kernels and the exact host search they are compared with (no GPU needed; a plain module, not a conftest).

The reference is `exact_knn`: float64 of the fp32 coordinates, `(q0 - c0)^2 + (q1 - c1)^2 + (q2 - c2)^2` summed left to right as the
kernels sum it, a stable argsort per row, so equal distances are decided by the smaller context index. The input families all hold
EXACT ties by construction -- integer lattices and what lies symmetrically between their points -- with the context's index order
shuffled by a fixed seed, so that index order says nothing about position. tests/test_knn_ties_cpu.py checks that the families are as
tie-laden as they claim; tests/test_knn_ties_gpu.py compares every kNN kernel with `exact_knn` on them."""
import functools

import numpy as np

FAMILIES = ("on", "centre", "edge", "face", "out")          # the order of the blocks of `lattice(n)[1]`, n^3 rows each
IN_BOX = FAMILIES[:4]
ECEF_SPACING = 1000.0                                       # a multiple of the fp32 ulp at 6.4e6 (0.5): the lattice is exact in fp32
ECEF_ORIGIN = (6.4e6, -1.2e6, 3.3e5)
_CHUNK_BYTES = 100e6


def exact_knn(xc, xq, k, exclude_self=False):
    """int32 [n_query, k]: the k nearest context points of every query, nearest first, ties by the smaller index; -1 where the context
    has fewer than k candidates. `exclude_self`: query i never lists context i (the query set is the context set). Rows are processed
    in chunks whose float64 distance block stays near 100 MB; the three squares are added per axis, left to right: the sum
    `((q - c) ** 2).sum(-1)` without its [rows, n_context, 3] temporary."""
    xc, xq = np.asarray(xc), np.asarray(xq)
    assert xc.dtype == np.float32 and xq.dtype == np.float32 and xc.ndim == 2 and xq.ndim == 2 and xc.shape[1] == 3 and xq.shape[1] == 3
    nc, nq = xc.shape[0], xq.shape[0]
    assert not exclude_self or nq == nc
    c = xc.astype(np.float64)
    out = np.full((nq, k), -1, dtype=np.int32)
    have = min(k, nc - (1 if exclude_self else 0))
    rows = max(1, int(_CHUNK_BYTES // (8 * nc)))
    for a in range(0, nq, rows):
        q = xq[a:a + rows].astype(np.float64)
        d = (q[:, None, 0] - c[None, :, 0]) ** 2
        d += (q[:, None, 1] - c[None, :, 1]) ** 2
        d += (q[:, None, 2] - c[None, :, 2]) ** 2
        if exclude_self:
            d[np.arange(q.shape[0]), np.arange(a, a + q.shape[0])] = np.inf
        out[a:a + rows, :have] = np.argsort(d, axis=1, kind="stable")[:, :have]
    return out


def exact_knn_sorted_distances(xc, xq, idx):
    """float64 [n_query, idx.shape[1]]: the reference's distances of the neighbours `idx` lists (the statements of `exact_knn`)."""
    c, q = np.asarray(xc).astype(np.float64)[idx], np.asarray(xq).astype(np.float64)[:, None, :]
    return ((q[..., 0] - c[..., 0]) ** 2 + (q[..., 1] - c[..., 1]) ** 2) + (q[..., 2] - c[..., 2]) ** 2


def exact_knn_integers(ic, k, exclude_self=True):
    """`exact_knn(ic, ic, k, exclude_self)` of a point set with SMALL INTEGER coordinates (int64 [n, 3]) against itself, for sets too
    large for a row-wise argsort: squared distances of small integers are the same numbers in int64 and in float64, (distance, index)
    becomes one integer key `distance * n + index` per pair, and the k smallest keys of a row, sorted, are the first k of the stable
    argsort. The keys are int64, or int32 where the largest of them fits (integers either way; half the memory traffic, which is
    what the search of 17 576 points among themselves costs on the host)."""
    ic = np.asarray(ic, dtype=np.int64)
    n = ic.shape[0]
    span = int(ic.max() - ic.min())
    assert k < n and (3 * span * span + 2) * n < 2 ** 62
    dt = np.int32 if (3 * span * span + 2) * n < 2 ** 31 else np.int64
    ic = (ic - ic.min()).astype(dt)
    out = np.empty((n, k), dtype=np.int32)
    rows = max(1, int(_CHUNK_BYTES // (np.dtype(dt).itemsize * n)))
    idx = np.arange(n, dtype=dt)
    for a in range(0, n, rows):
        q = ic[a:a + rows]
        d = (q[:, None, 0] - ic[None, :, 0]) ** 2
        d += (q[:, None, 1] - ic[None, :, 1]) ** 2
        d += (q[:, None, 2] - ic[None, :, 2]) ** 2
        if exclude_self:
            d[np.arange(q.shape[0]), np.arange(a, a + q.shape[0])] = 3 * span * span + 1
        d *= n
        d += idx[None, :]
        out[a:a + rows] = np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1) % n
    return out


def lattice_integers(n):
    """int64 [n^3, 3]: the integer lattice 0 .. n - 1 on every axis, x slowest."""
    g = np.arange(n, dtype=np.int64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def _shuffled(a, seed):
    return a[np.random.default_rng(seed).permutation(a.shape[0])]


def _families(n, shift=0.0):
    """The five query families of the n^3 lattice in lattice units (float64 [5 n^3, 3], blocks in the order of FAMILIES): on the
    points, cell centres, edge midpoints (+0.5 on one axis, the axis cycling with the row), face centres (+0.5 on two axes), and
    lattice-aligned points far outside the box; `shift` moves the four in-box families (so that a larger lattice of queries also
    covers the outside of a smaller context's box)."""
    lat = lattice_integers(n).astype(np.float64)
    one = np.eye(3)[np.arange(lat.shape[0]) % 3] * 0.5
    return np.concatenate((lat + shift, lat + 0.5 + shift, lat + one + shift, lat + 0.5 - one + shift, lat * 7.0 - 30.0), 0)


def _ecef(p):
    return p * ECEF_SPACING + np.array([ECEF_ORIGIN])


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def lattice(n, shift=0.0):
    """(context: the n^3 integer lattice, shuffled; queries: the five families of FAMILIES, n^3 rows each), both float32."""
    return _f32(_shuffled(lattice_integers(n).astype(np.float64), 100 + n)), _f32(_families(n, shift))


@functools.lru_cache(maxsize=None)
def lattice_ecef(n, shift=0.0):
    """`lattice(n)` times 1000 plus (6.4e6, -1.2e6, 3.3e5), rounded to fp32 BEFORE anything else is derived from it: the spacing is a
    multiple of the fp32 ulp at that magnitude, so the ties exist in the fp32 coordinates the kernels read."""
    xc, xq = lattice(n, shift)
    return _f32(_ecef(xc.astype(np.float64))), _f32(_ecef(xq.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def triples(n, shift=0.0):
    """Every point of the n^3 lattice three times in the context, at unrelated indices; the queries of `lattice(n)`. Every distance
    then occurs a multiple of three times, decided by index alone."""
    return _f32(_shuffled(np.tile(lattice_integers(n).astype(np.float64), (3, 1)), 300 + n)), lattice(n, shift)[1]


@functools.lru_cache(maxsize=None)
def identical(n_context, n_query=257):
    """All context points equal; the queries are that point and `n_query - 1` others. Every row of the table is 0 .. k - 1."""
    p = np.array([[3.5, -2.25, 100.0]])
    rng = np.random.default_rng(500 + n_context)
    xq = np.concatenate((p, p + rng.uniform(-50.0, 50.0, (n_query - 1, 3))), 0)
    return _f32(np.tile(p, (n_context, 1))), _f32(xq)


def family(xq, name):
    """The block of family `name` in the queries of `lattice` / `lattice_ecef` / `triples`."""
    m = xq.shape[0] // len(FAMILIES)
    i = FAMILIES.index(name)
    return xq[i * m:(i + 1) * m]


N_BIG = 16384 + 37          # genie_knn's lane-per-query threshold plus a partial last workgroup


@functools.lru_cache(maxsize=None)
def big_queries(ecef=False):
    """16 384 + 37 queries for a 12^3 (or smaller) context at the origin: the four in-box families of `lattice(16)` shifted by -2 -- two
    lattice steps of them lie outside the 12^3 box on every side -- and 37 rows of the "out" family."""
    xq = (lattice_ecef if ecef else lattice)(16, -2.0)[1]
    out = np.ascontiguousarray(np.concatenate((xq[:4 * 4096], family(xq, "out")[5::110][:37]), 0))
    assert out.shape == (N_BIG, 3)
    return out


def mixed_rows(n_total, n_rows, n_tail, seed=7):
    """`n_rows` row numbers of a query set of `n_total` rows, sorted: a seeded draw over the whole set, and its last `n_tail` rows."""
    head = np.random.default_rng(seed).permutation(n_total - n_tail)[:n_rows - n_tail]
    return np.sort(np.concatenate((head, np.arange(n_total - n_tail, n_total))))


def tie_shares(d, k):
    """Of the rows of `d` (float64 [rows, > k], the reference's distances in table order): the share whose first k hold a run of at least
    3 equal values, and the share whose k-th and (k+1)-th are equal."""
    first = d[:, :k]
    run3 = (first[:, 2:] == first[:, :-2]).any(1) if k >= 3 else np.zeros(d.shape[0], dtype=bool)
    return float(run3.mean()), float((d[:, k - 1] == d[:, k]).mean())


def explain(got, want):
    """The failure message of a table comparison: how many rows differ, the first of them, both versions."""
    bad = np.nonzero((got != want).any(1))[0]
    i = int(bad[0])
    return "%d of %d rows differ; row %d: device %s exact host search %s" % (bad.size, got.shape[0], i, got[i].tolist(), want[i].tolist())
