"""GPU: the refine pass's query cloud drawn on the device (`genie_refine_cloud`, csrc/cloud_kernels.hpp; `postproc.refine_cloud_device`;
`apply.refine_sources(rand=apply.PhiloxCloud(key))`).

* the kernel against numpy, bit for bit: the draw is `Generator(Philox(key, counter=[0, source, 0, 0])).random((n, 3))`, the cloud
  `src + (r * rng + mn)` in float64 and its float32 rounding -- sizes around a Philox block, a workgroup and the grid cap, extreme keys
  and sources, guards around every buffer;
* the pass: `rand=PhiloxCloud(k)` against the staged path fed the same numbers from the host (rows, refined sources and order
  bit-equal), source-parallel blocks side by side against one GPU with the launches of every rank counted, and the host-cloud branch
  against the device branch (exact, as tests/test_day_loops_gpu.py compares the two branches)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from genie_amd import _lib, apply, postproc
from tests.test_day_loops_gpu import _Setup

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
M64 = (1 << 64) - 1
KEYS = [(0, 0), (M64, (1 << 63) + 5), (0x6A09E667F3BCC908, 0x3C6EF372FE94F82B)]      # the last: a random pair, fixed
SOURCES = [0, 1, (1 << 32) + 7]
N_STRIDE = postproc.REFINE_CLOUD_SWEEP // 3 + 1001            # 3 n = one sweep of the capped grid + 3 005 elements: threads stride
SIZES = [1, 2, 3, 4, 5, 341, 342, 1365, 1366, N_STRIDE]
SRC = np.array([12345.678, -54321.0123, -7000.5])
RNG = np.array([2e5, 2e5, 3e4])                               # ranges an order of magnitude apart and negative minima: a swapped
MN = np.array([-1e5, -0.75e5, -2.5e4])                        # axis cannot pass
GUARD = 4                                                     # elements either side of a buffer: 32 B (fp64) / 16 B (fp32)


@functools.lru_cache(maxsize=32)
def _want(key, source, n):
    r = apply.PhiloxCloud(key).host(source, n)
    Xc = SRC.reshape(1, 3) + (r * RNG.reshape(1, 3) + MN.reshape(1, 3))
    return r, Xc, Xc.astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _raw(key, source, n, with_r=True, null_xc=False, n_arg=None):
    """One call of the C function on guarded buffers. Returns (rc, r, xc, xq) with the guards still attached (host arrays)."""
    fill64, fill32 = -7.25, np.float32(-3.5)
    r = torch.full((3 * n + 2 * GUARD,), fill64, dtype=torch.float64, device=DEV)
    xc = torch.full((3 * n + 2 * GUARD,), fill64, dtype=torch.float64, device=DEV)
    xq = torch.full((3 * n + 2 * GUARD,), float(fill32), dtype=torch.float32, device=DEV)
    p = lambda t, on=True: ctypes.c_void_p(t.data_ptr() + GUARD * t.element_size()) if on else ctypes.c_void_p(0)     # noqa: E731
    vec = [float(v) for a in (SRC, RNG, MN) for v in a]
    st = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    rc = _lib.load().genie_refine_cloud(key[0], key[1], source, n if n_arg is None else n_arg, *vec, p(r, with_r), p(xc, not null_xc), p(xq),
                                        st)
    torch.cuda.synchronize()
    return rc, r.cpu().numpy(), xc.cpu().numpy(), xq.cpu().numpy()


def _guards_intact(a):
    return bool((a[:GUARD] == a[0]).all() and (a[-GUARD:] == a[0]).all() and a[0] < 0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("source", SOURCES)
def test_kernel_equals_numpy_bit_for_bit(n, key, source):
    r_w, Xc_w, xq_w = _want(key, source, n)
    Xc, xq, r = postproc.refine_cloud_device(key, source, n, SRC, RNG, MN, DEV, want_draw=True)
    assert r.dtype == Xc.dtype == torch.float64 and xq.dtype == torch.float32 and r.shape == Xc.shape == xq.shape == (n, 3)
    r, Xc, xq = r.cpu().numpy(), Xc.cpu().numpy(), xq.cpu().numpy()
    assert np.array_equal(_bits(r), _bits(r_w))                     # the draw, as uint64 bit patterns
    assert np.array_equal(_bits(Xc), _bits(Xc_w))                   # src + (r * rng + mn), each operation rounded
    assert np.array_equal(_bits(xq), _bits(xq_w))                   # the float32 rounding
    assert float(r.min()) >= 0.0 and float(r.max()) < 1.0


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 342, N_STRIDE])
def test_nothing_outside_the_buffers_is_written_and_the_draw_is_optional(n):
    key, source = KEYS[1], SOURCES[2]
    r_w, Xc_w, xq_w = _want(key, source, n)
    rc, r, xc, xq = _raw(key, source, n)
    assert rc == 0 and all(_guards_intact(a) for a in (r, xc, xq))
    assert np.array_equal(_bits(r[GUARD:-GUARD]), _bits(r_w.reshape(-1)))
    assert np.array_equal(_bits(xc[GUARD:-GUARD]), _bits(Xc_w.reshape(-1)))
    assert np.array_equal(_bits(xq[GUARD:-GUARD]), _bits(xq_w.reshape(-1)))
    rc, r0, xc0, xq0 = _raw(key, source, n, with_r=False)          # r = NULL: the same cloud, the draw is not stored
    assert rc == 0 and all(_guards_intact(a) for a in (xc0, xq0)) and (r0 == r0[0]).all()
    assert np.array_equal(_bits(xc0), _bits(xc)) and np.array_equal(_bits(xq0), _bits(xq))


def test_zero_queries_succeed_and_touch_nothing():
    rc, r, xc, xq = _raw(KEYS[2], 3, 4, n_arg=0)                    # room for four queries, none asked for
    assert rc == 0
    assert (r == r[0]).all() and (xc == xc[0]).all() and (xq == xq[0]).all()
    Xc, xq = postproc.refine_cloud_device(KEYS[2], 3, 0, SRC, RNG, MN, DEV)
    assert Xc.shape == (0, 3) and xq.shape == (0, 3)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    rc, r, xc, xq = _raw(KEYS[0], 0, 4, null_xc=True)
    assert rc == -1 and "null" in lib.genie_last_error().decode()                 # GENIE_ERR_ARG
    assert (r == r[0]).all() and (xc == xc[0]).all() and (xq == xq[0]).all()
    rc, r, xc, xq = _raw(KEYS[0], 0, 4, n_arg=-1)
    assert rc == -1 and "n_query" in lib.genie_last_error().decode()
    assert (r == r[0]).all() and (xc == xc[0]).all() and (xq == xq[0]).all()
    buf = torch.zeros(64, dtype=torch.float64, device=DEV)
    ok64, ok32 = torch.zeros(12, dtype=torch.float64, device=DEV), torch.zeros(12, dtype=torch.float32, device=DEV)
    vec = [float(v) for a in (SRC, RNG, MN) for v in a]
    rc = lib.genie_refine_cloud(1, 2, 0, 4, *vec, None, ctypes.c_void_p(buf.data_ptr() + 8), ctypes.c_void_p(ok32.data_ptr()), None)
    assert rc == -1 and "aligned" in lib.genie_last_error().decode()
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0 and float(ok64.abs().max()) == 0.0 and float(ok32.abs().max()) == 0.0
    with pytest.raises(ValueError):
        postproc.refine_cloud_device(KEYS[0], -1, 4, SRC, RNG, MN, DEV)
    with pytest.raises(ValueError):
        postproc.refine_cloud_device(KEYS[0], 0, -4, SRC, RNG, MN, DEV)


def test_launches_repeat_and_sources_differ():
    n = 1366
    a = [t.cpu().numpy() for t in postproc.refine_cloud_device(KEYS[2], 5, n, SRC, RNG, MN, DEV, want_draw=True)]
    b = [t.cpu().numpy() for t in postproc.refine_cloud_device(KEYS[2], 5, n, SRC, RNG, MN, DEV, want_draw=True)]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    c = [t.cpu().numpy() for t in postproc.refine_cloud_device(KEYS[2], 6, n, SRC, RNG, MN, DEV, want_draw=True)]
    assert not (a[2] == c[2]).any() and not (a[0] == c[0]).all()                  # another source: another draw, element by element
    d = postproc.refine_cloud_device((KEYS[2][0], KEYS[2][1] + 1), 5, n, SRC, RNG, MN, DEV, want_draw=True)[2].cpu().numpy()
    assert not (a[2] == d).any()                                                  # another key word 1 too


def test_an_int_key_is_its_two_words():
    k = (KEYS[1][1] << 64) | KEYS[1][0]
    a = postproc.refine_cloud_device(k, 2, 7, SRC, RNG, MN, DEV, want_draw=True)[2].cpu().numpy()
    assert a.tobytes() == _want(KEYS[1], 2, 7)[0].tobytes()
    assert a.tobytes() == np.random.Generator(np.random.Philox(key=k, counter=[0, 2, 0, 0])).random((7, 3)).tobytes()


# ------------------------------------------------------------------------------------------------
# the pass: the small day of tests/test_day_loops_gpu.py, the six candidates of tests/test_source_parallel_gpu.py, two grid legs
# ------------------------------------------------------------------------------------------------
IDENT = lambda x: x                                                                        # noqa: E731
RANGES = ((0.0, 60e3), (0.0, 60e3), (-40e3, 2e3))
OFF_MIN, OFF_RNG = np.array([[-5e3, -5e3, -3e3]]), np.array([[10e3, 10e3, 6e3]])
N_QUERY = 300
KEY = (0x9E3779B97F4A7C15, 77)
QUIET = 4                                       # the candidate in a quiet stretch of the day: no pick, no leg produces a window


@functools.lru_cache(maxsize=None)
def _setup():
    return _Setup()


def _candidates(s):
    """Four near events, one in a quiet stretch (index QUIET), one at the region's corner (part of its cloud is masked)."""
    rng = np.random.default_rng(5)
    nodes = rng.choice(s.G, 4, replace=False)
    srcs = np.concatenate((s.geom_all.x_grid[nodes], rng.uniform(6995.0, 7010.0, (4, 1)), np.full((4, 1), 0.5)), axis=1)
    return np.concatenate((srcs, [[20e3, 30e3, -5e3, 30000.0, 0.5]], [[500.0, 59.6e3, 1500.0, 7002.0, 0.5]]), axis=0)


class _HostFeed(object):
    """A plain callable `rand`: its i-th call returns `PhiloxCloud(key).host(i, n)` -- the staged path, fed the keyed path's numbers."""

    def __init__(self, key):
        self.cloud, self.calls = apply.PhiloxCloud(key), 0

    def __call__(self, n, three):
        assert three == 3
        self.calls += 1
        return self.cloud.host(self.calls - 1, n)


def _refine(rand, device_branch=True, **kw):
    s = _setup()
    return apply.refine_sources([s.leg, s.leg], s.picks, _candidates(s), s.locs, s.tq, s.max_t, OFF_MIN, OFF_RNG, N_QUERY, IDENT, IDENT, *RANGES,
                                kernel_sig_t=s.sig, dt_embed=s.dt, rand=rand, ftrns2_device=IDENT if device_branch else None, **kw)


@functools.lru_cache(maxsize=None)
def _staged():
    """The staged path (today's: host draw, pinned copy) fed the keyed numbers: (rows [6, 7], srcs_refined, order)."""
    feed = _HostFeed(KEY)
    rows, block = _refine(feed, source_parallel=(0, 1))
    assert block == (0, 6) and rows.shape == (6, 7) and feed.calls == 6
    ref, order = _refine(_HostFeed(KEY))
    return rows, ref, order


def _count_cloud_calls(monkeypatch):
    calls, real = [], postproc.refine_cloud_device

    def counted(key, source, *a, **kw):
        calls.append((key, int(source)))
        return real(key, source, *a, **kw)

    monkeypatch.setattr(postproc, "refine_cloud_device", counted)
    return calls


def test_keyed_pass_equals_the_staged_path_fed_the_same_numbers(monkeypatch):
    rows_w, ref_w, order_w = _staged()
    assert rows_w[:, 3].all() and len(np.unique(rows_w[:, 0])) > 1 and float(rows_w[:, 2].max()) > 1e-3
    assert rows_w[QUIET, 2] == 0.0 and rows_w[QUIET, 1] == 0.0                    # the window without picks: all-zero read-out
    calls = _count_cloud_calls(monkeypatch)

    def no_staging(*a):
        raise AssertionError("the keyed path needs no pinned pair")

    monkeypatch.setattr(apply, "_pinned_pair", no_staging)
    rows, block = _refine(apply.PhiloxCloud(KEY), source_parallel=(0, 1))
    assert block == (0, 6) and rows.dtype == np.float64 and rows.tobytes() == rows_w.tobytes()
    assert calls == [(KEY, i) for i in range(6)]
    ref, order = _refine(apply.PhiloxCloud(KEY))
    assert ref.tobytes() == ref_w.tobytes() and np.array_equal(order, order_w)
    other, _ = _refine(apply.PhiloxCloud((KEY[0], KEY[1] + 1)))
    assert other.tobytes() != ref_w.tobytes()                                     # the key matters


@pytest.mark.parametrize("world", [2, 3, 7])
def test_ranks_draw_their_own_sources_only_and_give_the_one_gpu_rows(world, monkeypatch):
    rows_w, ref_w, order_w = _staged()
    s = _setup()
    blocks = apply.window_blocks(6, world)
    calls = _count_cloud_calls(monkeypatch)
    parts = []
    for r in range(world):
        del calls[:]
        rows, block = _refine(apply.PhiloxCloud(KEY), source_parallel=(r, world))
        assert block == blocks[r] and rows.shape == (block[1] - block[0], 7)
        assert calls == [(KEY, i) for i in range(*block)]                         # one launch per own source, none for another rank's
        parts.append(rows)
    assert world <= 6 or any(p.shape[0] == 0 for p in parts)                      # more ranks than sources: empty blocks, no error
    found = np.concatenate(parts)
    assert found.tobytes() == rows_w.tobytes()
    got, order = apply.refined_from_found(found, _candidates(s), s.tq, IDENT)
    assert got.tobytes() == ref_w.tobytes() and np.array_equal(order, order_w)


def test_host_cloud_branch_refines_the_same_sources(monkeypatch):
    _, ref_w, order_w = _staged()
    calls = _count_cloud_calls(monkeypatch)
    got, order = _refine(apply.PhiloxCloud(KEY), device_branch=False)
    assert calls == []                                                            # drawn with PhiloxCloud.host, nothing on the device
    assert np.array_equal(order, order_w) and np.array_equal(got, ref_w)          # exact: the comparison of test_day_loops_gpu.py
