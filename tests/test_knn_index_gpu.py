"""GPU: the cell-index kNN (`engine.KnnIndex`, genie_knn_index_build / genie_knn_indexed) returns the table of the brute-force search.

The yardstick everywhere is `engine.knn_device(..., index=None)` on the same tensors, compared with `torch.equal`: that call is pinned
to an exact fp64 host search by tests/test_hip_parity.py and, on tie-laden inputs and for each of its three kernels, by
tests/test_knn_ties_gpu.py (which holds the indexed search to the host as well), so it is the reference here and not the code under
test; index on and off are bit-equal at every size, the lattice with at least 16 384 queries included. Shapes are small
because what can go wrong is structural: the order of candidates (ties), the stop rule at cell faces, degenerate boxes, queries outside
the box, empty cells. Then the switch: `knn_index` on a model, through `SpatialAttention.query_table`, `forward_fixed_source` and
`refine_sources`, bit-equal with it on and off."""
import functools

import numpy as np
import pytest
import torch

from genie_amd import apply, engine, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = (1, 8, 10, 16)
N_CONTEXT = (1, 9, 10, 11, 257, 4099)
N_QUERY = (1, 63, 64, 65, 257)
N_LARGE = 20001                      # above engine.KNN_INDEX_MIN_QUERIES: the size the model's switch acts on


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def check(xc, xq, ks=(10,), exclude_self=False, index=None):
    """The indexed table equals the brute-force one for every k of `ks`; returns the index."""
    index = index or engine.KnnIndex(xc)
    assert index.matches(xc) and index.n_context == xc.shape[0]
    for k in ks:
        want = engine.knn_device(xc, xq, k, exclude_self=exclude_self)
        got = engine.knn_device(xc, xq, k, exclude_self=exclude_self, index=index)
        assert got.dtype == torch.int32 and got.shape == want.shape
        if not torch.equal(got, want):
            bad = torch.nonzero((got != want).any(1)).reshape(-1)
            i = int(bad[0])
            raise AssertionError("k=%d: %d of %d rows differ; row %d: indexed %s brute force %s" % (
                k, bad.numel(), got.shape[0], i, got[i].tolist(), want[i].tolist()))
    return index


@functools.lru_cache(maxsize=None)
def context(n, seed=3):
    rng = np.random.default_rng(seed + n)
    return _t(rng.uniform((0, 0, -40e3), (60e3, 60e3, 2e3), (n, 3)))


@functools.lru_cache(maxsize=None)
def queries(n, seed=11):
    """Around the contexts' box and a fifth beyond it on every side."""
    rng = np.random.default_rng(seed + n)
    return _t(rng.uniform((-12e3, -12e3, -48e3), (72e3, 72e3, 10e3), (n, 3)))


@pytest.mark.parametrize("n_context", N_CONTEXT)
def test_sizes(n_context):
    """Every context size against every query size and k (n_context < k included: `knn_device` clamps k), one index per context."""
    xc = context(n_context)
    index = engine.KnnIndex(xc)
    assert int(np.prod(index.cells)) >= 1 and index.cell > 0
    for nq in N_QUERY:
        check(xc, queries(nq), KS, index=index)
    check(xc, queries(N_LARGE), (10,), index=index)
    assert index.calls == len(N_QUERY) * len(KS) + 1
    cs = index.cell_start.cpu().numpy()
    assert cs[0] == 0 and cs[-1] == n_context and np.all(np.diff(cs) >= 0) and cs.shape[0] == int(np.prod(index.cells)) + 1
    assert sorted(index.records[:, 3].contiguous().view(torch.int32).cpu().tolist()) == list(range(n_context))


@pytest.mark.parametrize("n", [257, 4099])
def test_exclude_self(n):
    xc = context(n)
    check(xc, xc, KS, exclude_self=True)


def test_too_few_candidates_give_minus_one():
    """The C entry keeps k as asked (the host clamps it): missing neighbours are -1, as genie_knn writes them."""
    import ctypes
    from genie_amd import _lib
    lib = _lib.load()
    xc, xq = context(9), queries(65)
    index = engine.KnnIndex(xc)
    for k, ex in ((10, 0), (16, 0), (9, 1), (10, 1)):
        got = torch.empty((65, k), dtype=torch.int32, device=DEV)
        want = torch.empty_like(got)
        q = xc if ex else xq
        nq = q.shape[0]
        _lib.check(lib.genie_knn(engine._ptr(xc), 9, engine._ptr(q), nq, k, ex, engine._ptr(want), engine._stream()))
        _lib.check(lib.genie_knn_indexed(engine._ptr(index.cell_start), engine._ptr(index.records), ctypes.byref(index._plan), 9,
                                         engine._ptr(q), nq, k, ex, engine._ptr(got), engine._stream()))
        assert torch.equal(got[:nq], want[:nq]) and int((got[:nq] == -1).sum()) == nq * (k - 9 + ex)


def test_ties_on_a_lattice():
    """An integer lattice 12 x 12 x 12: queries on the lattice points (6, 12, 8, ... equal distances) and at the cell centres (8 equal
    nearest, 24 next): dozens of ties per query, decided by index."""
    g = np.arange(12, dtype=np.float64)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lat = lat[np.random.default_rng(0).permutation(lat.shape[0])]              # index order unrelated to position
    xc = _t(lat)
    index = check(xc, xc, KS)
    check(xc, xc, KS, exclude_self=True, index=index)
    check(xc, _t(lat + 0.5), KS, index=index)
    check(xc, _t(lat * 7.0 - 30.0), (10, 16), index=index)                    # lattice-aligned queries far outside as well
    # the size the model's switch acts on, where the brute-force arm is genie_knn's lane-per-query kernel: the lattice ten times
    # (17 280 rows, on the points) and its cell centres ten times
    big = np.tile(lat, (10, 1))
    assert big.shape[0] >= engine.KNN_INDEX_MIN_QUERIES
    check(xc, _t(big), (1, 8, 10), index=index)
    check(xc, _t(big + 0.5), (8, 10), index=index)


def test_all_points_identical():
    xc = _t(np.tile([[3.5, -2.25, 100.0]], (4099, 1)))
    index = check(xc, queries(257), KS)
    assert index.cells == (1, 1, 1)
    check(xc, xc[:257].contiguous(), KS, index=index)
    check(xc, xc, (10,), exclude_self=True, index=index)


@pytest.mark.parametrize("shape", ["collinear", "collinear_axis", "coplanar", "coplanar_axis", "single"])
def test_degenerate_boxes(shape):
    rng = np.random.default_rng(17)
    n = 257
    if shape == "collinear":
        p = np.array([[1e3, 2e3, -3e3]]) + rng.uniform(0, 1, (n, 1)) * np.array([[40e3, 25e3, -7e3]])
    elif shape == "collinear_axis":
        p = np.array([[1e3, 2e3, -3e3]]) + rng.uniform(0, 1, (n, 1)) * np.array([[0.0, 50e3, 0.0]])
    elif shape == "coplanar":
        uv = rng.uniform(0, 1, (n, 2))
        p = uv[:, :1] * np.array([[30e3, 10e3, 5e3]]) + uv[:, 1:] * np.array([[-5e3, 20e3, 9e3]])
    elif shape == "coplanar_axis":
        p = np.concatenate((rng.uniform(0, 50e3, (n, 2)), np.full((n, 1), -7e3)), 1)
    else:
        p = np.array([[5.0, 6.0, 7.0]])
    xc = _t(p)
    index = check(xc, queries(257), KS)
    if shape == "collinear_axis":
        assert index.cells[0] == 1 and index.cells[2] == 1 and index.cells[1] > 1
    if shape == "coplanar_axis":
        assert index.cells[2] == 1
    if shape == "single":
        assert index.cells == (1, 1, 1)
    else:
        check(xc, xc, KS, exclude_self=True, index=index)


def test_empty_space_between_two_clusters():
    """Two clusters 10^6 m apart: most cells are empty. Queries inside the clusters, between them, and 10 x the extent outside the box
    on every side (the whole grid is then the candidate set)."""
    rng = np.random.default_rng(23)
    a = rng.uniform(0, 5e3, (500, 3))
    xc = _t(np.concatenate((a, a[::-1] * 0.9 + np.array([[1e6, 0, 0]])), 0))
    ext = 1e6
    far = [c * 10 * ext * s + rng.uniform(0, 5e3, (8, 3)) for c in np.eye(3) for s in (-1.0, 1.0)]
    far.append(np.array([[s0, s1, s2] for s0 in (-1, 1) for s1 in (-1, 1) for s2 in (-1, 1)]) * 10 * ext)
    xq = np.concatenate([rng.uniform(0, 5e3, (64, 3)), rng.uniform(0, 5e3, (64, 3)) + np.array([[1e6, 0, 0]]),
                         rng.uniform((5e3, 0, 0), (0.995e6, 5e3, 5e3), (129, 3)), np.array([[0.5e6, 2.5e3, 2.5e3]])] + far, 0)
    check(xc, _t(xq), KS)


def _faces(index, a):
    """fp32 coordinates of the cell faces of axis a, rebuilt from the index's geometry."""
    return (np.float64(np.float32(index.origin[a])) + np.arange(index.cells[a] + 1) * index.cell).astype(np.float32)


def _on_faces(index, rng, n_fill, box):
    """Points exactly on, one ulp below and one ulp above the cell faces: per axis and face a few points with that coordinate (the
    others random), every intersection of three faces with a random choice of the three variants per coordinate, random fill."""
    lo, hi = box
    f = [_faces(index, a) for a in range(3)]
    var = lambda v, s: v if s == 0 else np.nextafter(v, np.float32(np.inf if s > 0 else -np.inf), dtype=np.float32)
    pts = []
    for a in range(3):
        for v in f[a]:
            for s in (-1, 0, 1):
                p = rng.uniform(lo, hi, (6, 3)).astype(np.float32)
                p[:, a] = var(v, s)
                pts.append(p)
    corners = np.stack(np.meshgrid(*f, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    s = rng.integers(-1, 2, corners.shape)
    corners = np.where(s == 0, corners, np.where(s > 0, np.nextafter(corners, np.float32(np.inf)), np.nextafter(corners, np.float32(-np.inf))))
    pts.append(corners.astype(np.float32))
    pts = np.concatenate(pts, 0)
    assert pts.shape[0] <= n_fill
    return np.concatenate((pts, rng.uniform(lo, hi, (n_fill - pts.shape[0], 3)).astype(np.float32)), 0)


@pytest.mark.parametrize("origin", [0.0, 6.4e6, -1234.5678])
def test_cell_faces(origin):
    """Context points and queries exactly on, one ulp below and one ulp above the faces of the cells: the binning is fp32 arithmetic,
    so such a point may sit in either neighbour cell, and the stop rule must not count on which. The geometry of an index depends on
    the point count and the bounding box only, so it is read from an index of random points with the same count and corners."""
    rng = np.random.default_rng(29)
    n = 2600
    lo, hi = np.array([origin, origin - 500.0, origin + 250.0]), np.array([origin + 9e3, origin + 7.5e3, origin + 8.25e3])
    pin = np.stack((lo, hi)).astype(np.float32)                                # the two corners fix the box
    probe = engine.KnnIndex(_t(np.concatenate((pin, rng.uniform(lo, hi, (n - 2, 3))), 0)))
    assert min(probe.cells) >= 4
    inside = lambda p: np.clip(p, pin[0], pin[1])                              # (one ulp beyond an outer face would move the box)
    xc = _t(np.concatenate((pin, inside(_on_faces(probe, rng, n - 2, (lo, hi)))), 0))
    index = engine.KnnIndex(xc)
    assert index.cells == probe.cells and index.cell == probe.cell and index.origin == probe.origin
    xq = _t(_on_faces(probe, np.random.default_rng(31), n, (lo - 1e3, hi + 1e3)))      # queries also one ulp outside the box
    check(xc, xq, KS, index=index)
    check(xc, xc, (1, 10), exclude_self=True, index=index)


def test_magnitude_ecef_like():
    """Coordinates around 6.4e6 (fp32 ulp 0.5 m) on a 100 m lattice, queries on the lattice, at half spacings and anywhere."""
    g = np.arange(16, dtype=np.float64) * 100.0
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.array([[6.4e6, -6.3e6, 6.35e6]])
    rng = np.random.default_rng(37)
    xc = _t(lat[rng.permutation(lat.shape[0])])
    index = check(xc, xc, KS, exclude_self=True)
    check(xc, _t(lat + 50.0), KS, index=index)
    check(xc, _t(lat[:2000] + rng.uniform(-300, 300, (2000, 3))), KS, index=index)


def test_refine_style_cloud():
    """One seeded cloud shaped like the refine pass's: a box around a grid node near the grid's corner, partly outside the grid."""
    xc = context(4099)
    rng = np.random.default_rng(41)
    p = xc.cpu().numpy()
    node = p[np.argmax(p[:, 0] / 60e3 - p[:, 1] / 60e3 + (p[:, 2] + 40e3) / 42e3)]            # the node nearest the corner (+x, -y, +z)
    cloud = node[None, :] + rng.uniform(0, 1, (N_LARGE, 3)) * np.array([[10e3, 10e3, 6e3]]) + np.array([[-5e3, -5e3, -3e3]])
    assert (cloud[:, 0] > 60e3).any() and (cloud[:, 1] < 0).any() and (cloud[:, 2] > 2e3).any()
    check(xc, _t(cloud), (10,))


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_context_is_refused(bad):
    from genie_amd import _lib
    q = context(257).clone()
    q[100, 1] = bad
    with pytest.raises(_lib.GenieHipError, match="not finite"):
        engine.KnnIndex(q)
    check(context(257), queries(65))                                           # (and the library goes on working)


# ---- the switch -------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def setup():
    from tests.test_day_loops_gpu import _Setup
    return _Setup()


def _cloud_around(s, n, seed):
    rng = np.random.default_rng(seed)
    node = s.geom_all.x_grid[3]
    return _t(node[None, :] + rng.uniform(0, 1, (n, 3)) * np.array([[10e3, 10e3, 6e3]]) + np.array([[-5e3, -5e3, -3e3]]))


def test_query_table_is_equal_with_the_switch_on():
    s = setup()
    net, att, xg = s.net, s.net.SpatialAttention, s.leg.x_grid_cart
    xq, xs = _cloud_around(s, N_LARGE, 1), _cloud_around(s, 300, 2)
    try:
        net.knn_index = False
        att.invalidate_query_cache()
        off = att.query_table(xq, xg).clone()
        assert att._context_index is None
        assert torch.equal(off, engine.knn_device(xg, xq, 10))
        net.knn_index = True
        assert att.knn_index is True
        att.invalidate_query_cache()
        on = att.query_table(xq, xg).clone()
        index = att._context_index
        assert torch.equal(on, off) and index.calls == 1 and index.matches(xg)
        att.query_table(xq, xg)                                                # the cached table: no search
        small = att.query_table(xs, xg)                                        # a small set keeps genie_knn
        assert index.calls == 1 and torch.equal(small, engine.knn_device(xg, xs, 10))
        att.query_table(_cloud_around(s, N_LARGE, 3), xg)                      # a new cloud, the same grid: the same index
        assert att._context_index is index and index.calls == 2
    finally:
        net.knn_index = False
        att.invalidate_query_cache()


def _window(s, t0=7002.0):
    em = s.leg.embed(s.picks, t0, s.max_t, s.sig, s.dt)
    assert em is not None
    return em


def test_forward_fixed_source_is_bit_equal_with_the_switch_on():
    s = setup()
    net, att = s.net, s.net.SpatialAttention
    Slice, Mask = _window(s)
    xq, tq, locs = _cloud_around(s, N_LARGE, 5), _t(s.tq), _t(s.locs)
    try:
        outs = []
        for on in (False, True):
            net.knn_index = on
            att.invalidate_query_cache()
            with torch.no_grad():
                y, x = net.forward_fixed_source(Slice, Mask, None, None, None, locs, s.leg.x_grid_cart, xq, tq)
            outs.append((y.clone(), x.clone()))
        assert att._context_index.calls == 1
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert float(outs[0][1].abs().max()) > 0
    finally:
        net.knn_index = False
        att.invalidate_query_cache()


def test_refine_sources_rows_are_bit_equal_with_the_switch_on():
    s = setup()
    ga = s.geom_all
    n_rand = engine.KNN_INDEX_MIN_QUERIES + 16
    srcs = np.concatenate((ga.x_grid[[3, 40, 66]], [[7001.0], [7004.5], [30000.0]], np.full((3, 1), 0.5)), axis=1)   # the last: no pick
    off_min, off_rng = np.array([[-5e3, -5e3, -3e3]]), np.array([[10e3, 10e3, 6e3]])
    ident = lambda x: x
    ranges = ((0.0, 60e3), (0.0, 60e3), (-40e3, 2e3))
    att = s.net.SpatialAttention
    try:
        rows = []
        for on in (False, True):
            leg = apply.GridLeg(s.net, ga.x_grid, s.trv_use, knn_index=on)
            assert s.net.knn_index is on
            att.invalidate_query_cache()
            rows.append(apply.refine_sources([leg], s.picks, srcs, s.locs, s.tq, s.max_t, off_min, off_rng, n_rand, ident, ident, *ranges,
                                             kernel_sig_t=s.sig, dt_embed=s.dt, rand=apply.PhiloxCloud(2024), ftrns2_device=ident,
                                             source_parallel=(0, 1)))
            if not on:
                assert att._context_index is None
        assert att._context_index is not None and att._context_index.calls == 2          # one search per source with a window
        assert rows[0][1] == rows[1][1] == (0, 3) and np.array_equal(rows[0][0], rows[1][0])
        assert np.all(rows[0][0][:, 3] == 1.0)                                           # every cloud has queries inside the region
    finally:
        s.net.knn_index = False
        att.invalidate_query_cache()


def test_a_new_grid_rebuilds_the_index():
    """`set_adjacencies*` on other positions: the next cloud is searched in an index of the new grid (the index is keyed by the context
    tensor it holds), and rewriting a grid tensor in place rebuilds it too. No stale neighbour either way."""
    from tests.test_day_loops_gpu import _Setup
    s = _Setup()                                                                # a model of its own: its grid is replaced
    net, att = s.net, s.net.SpatialAttention
    xq = _cloud_around(s, N_LARGE, 7)
    net.knn_index = True
    first = att.query_table(xq, s.leg.x_grid_cart).clone()
    index = att._context_index
    assert torch.equal(first, engine.knn_device(s.leg.x_grid_cart, xq, 10))
    gb = synthetic.Geometry(15, s.G, L=60e3, n_query=8, seed=92)
    xg_b = _t(gb.x_grid)
    assert not torch.equal(xg_b, s.leg.x_grid_cart)
    ea = ((gb.x_grid[:, None, :] - s.locs[None, :, :]) / gb.scale_x_extend.reshape(1, 1, 3)).reshape(-1, 3).astype(np.float32)
    net.set_adjacencies_base(torch.from_numpy(s.A_sta_sta), torch.from_numpy(gb.A_src_src), _t(ea), _t(s.locs), xg_b)
    second = att.query_table(xq, xg_b).clone()
    assert att._context_index is not index and att._context_index.matches(xg_b)
    assert torch.equal(second, engine.knn_device(xg_b, xq, 10)) and not torch.equal(second, first)
    index = att._context_index
    xg_b.mul_(0.5)                                                              # the same tensor, other positions
    assert not index.matches(xg_b)
    third = att.query_table(xq, xg_b)
    assert att._context_index is not index
    assert torch.equal(third, engine.knn_device(xg_b, xq, 10)) and not torch.equal(third, second)
    with pytest.raises(ValueError, match="another context"):
        engine.knn_device(xg_b, xq, 10, index=index)
