"""GPU: the merge kernel of the growable pick store (genie_picks_merge through `engine.picks_merge`) against a numpy stable merge, and
`apply.PickStore` on the device -- appends, merges, capacity doubling, trim and compaction -- against a freshly built `ResidentPicks`."""
import itertools

import numpy as np
import pytest
import torch

from genie_amd import apply, engine

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENGTHS = (0, 1, 63, 64, 65, 1000)


def _run(rng, n, t_lo, t_hi, first_index, decimals=1):
    t = np.sort(np.round(rng.uniform(t_lo, t_hi, n), decimals))
    return (t, rng.integers(0, 50, n).astype(np.int32), rng.integers(0, 2, n).astype(np.int32), first_index + rng.permutation(n).astype(np.int64))


def _merged(a, b):
    """numpy: a stable sort by time of the run a followed by the run b."""
    order = np.argsort(np.concatenate([a[0], b[0]]), kind="stable")
    return [np.concatenate([x, y])[order] for x, y in zip(a, b)]


def _check(a, b):
    d = lambda run: tuple(torch.from_numpy(x).to(DEV) for x in run)
    n = len(a[0]) + len(b[0])
    out = tuple(torch.full((n,), -7, dtype=dtype, device=DEV) for _, dtype in engine.PICK_FIELDS)
    got = engine.picks_merge(d(a), d(b), out)
    torch.cuda.synchronize()
    for g, w, (field, _) in zip(got, _merged(a, b), engine.PICK_FIELDS):
        assert np.array_equal(g.cpu().numpy(), w), (field, len(a[0]), len(b[0]))


@pytest.mark.parametrize("n_a,n_b", list(itertools.product(LENGTHS, LENGTHS)))
def test_merge_equals_a_stable_sort_of_the_concatenation(n_a, n_b):
    """Times rounded to 0.1 s over 20 s: at 1000 picks a run repeats every time about five times, ties inside and across the runs."""
    rng = np.random.default_rng([n_a, n_b])
    _check(_run(rng, n_a, 100.0, 120.0, 0), _run(rng, n_b, 100.0, 120.0, n_a))


@pytest.mark.parametrize("n_a,n_b", [(65, 64), (1000, 1), (1, 1000), (1000, 1000)])
def test_merge_of_all_equal_times_and_of_disjoint_runs(n_a, n_b):
    rng = np.random.default_rng(7)
    a, b = _run(rng, n_a, 100.0, 120.0, 0), _run(rng, n_b, 100.0, 120.0, n_a)
    same = lambda run: (np.full_like(run[0], 110.0),) + run[1:]
    _check(same(a), same(b))                                             # all equal: the resident run first, then the chunk
    _check(a, _run(rng, n_b, 10.0, 20.0, n_a))                           # the chunk entirely before the resident run
    _check(a, _run(rng, n_b, 120.0, 130.0, n_a))                         # entirely after it (touching at 120.0)


def test_merge_rejects_mismatched_runs():
    rng = np.random.default_rng(1)
    d = lambda run: tuple(torch.from_numpy(x).to(DEV) for x in run)
    a, b = d(_run(rng, 5, 0.0, 1.0, 0)), d(_run(rng, 3, 0.0, 1.0, 5))
    out = tuple(torch.empty(7, dtype=dtype, device=DEV) for _, dtype in engine.PICK_FIELDS)        # one element short
    with pytest.raises(ValueError):
        engine.picks_merge(a, b, out)
    with pytest.raises(ValueError):
        engine.picks_merge((a[0].float(),) + a[1:], b, tuple(torch.empty(8, dtype=dtype, device=DEV) for _, dtype in engine.PICK_FIELDS))


S_ALL = 30
IND_USE = np.random.default_rng(3).permutation(S_ALL)[:20]


def _chunk(rng, m, t_lo, t_hi):
    t = np.round(rng.uniform(t_lo, t_hi, m), 1)
    return np.stack([t, rng.integers(0, S_ALL, m).astype(np.float64), rng.random(m), rng.random(m), rng.integers(0, 2, m).astype(np.float64)], axis=1)


def _same(store, ref, live=slice(None)):
    for f in ("t", "sta", "phase", "phase_f", "index"):
        a, b = getattr(store, f), getattr(ref, f)[live if isinstance(live, slice) else torch.from_numpy(live).to(DEV)]
        assert a.is_cuda and a.dtype == b.dtype and torch.equal(a, b), f
    assert np.array_equal(store.t_host, ref.t_host[live])


@pytest.mark.parametrize("use_phase_types", [True, False])
def test_pick_store_on_the_device_grows_merges_and_compacts(use_phase_types):
    """Capacity 8 and chunks of up to 300 rows: doubling several times; chunks that reach below the resident tail: the merge kernel;
    a trim behind the feed: compaction. After every step the views equal a `ResidentPicks` built from everything fed."""
    rng = np.random.default_rng(31)
    store = apply.PickStore(IND_USE, S_ALL, DEV, use_phase_types=use_phase_types, capacity=8)
    chunks, caps, t_before = [], [], -np.inf
    for c in range(14):
        in_order = c % 3 == 0
        lo = 10.0 * c + (12.0 if in_order else -4.0)
        chunks.append(_chunk(rng, int(rng.integers(100, 300)) if c != 5 else 0, lo, lo + 15.0))
        if in_order and len(store):
            chunks[-1][:, 0] = np.maximum(chunks[-1][:, 0], store.t_host[-1])       # starts no earlier than the resident tail: appended
        store.append(chunks[-1])
        caps.append(store.capacity)
        ref = apply.ResidentPicks(np.concatenate(chunks), IND_USE, S_ALL, DEV, use_phase_types=use_phase_types)
        _same(store, ref, ref.t_host > t_before)
        if c >= 6:
            t_before = 10.0 * c - 30.0
            store.trim(t_before)
            _same(store, ref, ref.t_host > t_before)
            a = store.embed_args(10.0 * c - 10.0, 8.0, 1.0)
            b = ref.embed_args(10.0 * c - 10.0, 8.0, 1.0)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert caps[0] > 8 and max(caps) < len(ref)                          # grew at first, then stayed below everything fed: compaction
