"""GPU: the multi-leg stacking kernel (genie_stack_windows_legs through `engine.stack_windows_legs`) and the day's apply loop over
several source grids (`apply.apply_windows_legs`).

* the kernel alone, on random tensors: bit-equal to `for window: for leg: out.index_add_(...)`, to its one-leg sibling, untouched elements
  keep their bits, a column listed twice adds twice in (k, j, l) order, 64-bit offsets, bad arguments;
* the loop: one leg == `apply_windows_device(stack_on_device=True)`, and both == the reference loop; two and three legs (and a `use_subgraph` leg) == the reference loop
  written here from public calls, window-major, and NOT the leg-major sum a caller had to form before; refusals; window-parallel in
  the tuple form (every rank in this process) and the group form (one process per rank).

No tolerance anywhere: every comparison is against torch statements or an in-order fp32 loop on the same inputs."""
import ctypes
import datetime
import functools
import os
import socket
import types

import numpy as np
import pytest
import torch

from genie_amd import _lib, apply, engine, graph, module, synthetic
from tests.util import Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------------------

def _table(B, T, rng, first=3, stride=2, drop=0.15):
    """[B, T] int32: window k lists columns first + k * stride + (0..T-1), so consecutive windows overlap in all but `stride` columns; some
    entries dropped (-1). No row lists a column twice."""
    cols = (first + stride * np.arange(B)[:, None] + np.arange(T)[None, :]).astype(np.int32)
    cols[rng.random((B, T)) < drop] = -1
    if not (cols >= 0).any():
        cols[0, 0] = first
    return cols


def _torch_loop(out, xs, cols, d):
    """The statements the kernel replaces: for every window, for every leg, one `index_add_` of that leg's read-out divided by d."""
    ref = out.clone()
    for k in range(cols.shape[0]):
        valid = torch.from_numpy(np.flatnonzero(cols[k] >= 0)).to(DEV)
        c = torch.from_numpy(cols[k][cols[k] >= 0].astype(np.int64)).to(DEV)
        for x in xs:
            ref.index_add_(1, c, x[k][:, valid] / d)
    return ref


def _case(L, B, T, Q, seed):
    rng = np.random.default_rng(seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    cols = _table(B, T, rng)
    n_cols = int(cols.max()) + 6                                   # [c_min, c_max] is narrower than the axis on both sides
    xs = [torch.randn((B, Q, T), device=DEV, generator=g) for _ in range(L)]
    out = torch.randn((Q, n_cols), device=DEV, generator=g)
    used = cols[cols >= 0]
    return xs, cols, out, int(used.min()), int(used.max())


def _scale(d):
    return float(np.float32(1.0) / np.float32(d))


@pytest.mark.parametrize("L", [1, 2, 3, 5, 32])
def test_stack_legs_is_bit_equal_to_the_torch_loop(L):
    """B x T x Q over {1, 3, 16} x {9, 64} x {1, 7, 300} (one block and several, sizes that are no multiple of the block), the divisor
    cycling through 2 / 6 / 9 / 15 (for all but 2, `x / d` and `x * (1 / d)` differ in fp32: torch multiplies by the fp32 reciprocal, and
    so does the kernel); every divisor again on one shape; a second call on the same inputs gives the same bits."""
    ds = [2.0, 6.0, 9.0, 15.0]
    shapes = [(B, T, Q) for B in (1, 3, 16) for T in (9, 64) for Q in (1, 7, 300)]
    runs = [(s, ds[i % 4]) for i, s in enumerate(shapes)] + [((3, 9, 7), d) for d in ds]
    for i, ((B, T, Q), d) in enumerate(runs):
        xs, cols, out, c_min, c_max = _case(L, B, T, Q, 100 * L + i)
        assert c_min > 0 and c_max < out.shape[1] - 1
        want = _torch_loop(out, xs, cols, d)
        d_cols = torch.from_numpy(cols).to(DEV)
        got = engine.stack_windows_legs(out.clone(), xs, d_cols, _scale(d), c_min, c_max)
        again = engine.stack_windows_legs(out.clone(), xs, d_cols, _scale(d), c_min, c_max)
        assert not torch.equal(got, out), (B, T, Q, d)
        assert torch.equal(got, want), (B, T, Q, d)
        assert torch.equal(again, got), (B, T, Q, d)


def test_stack_legs_with_one_leg_equals_the_sibling():
    for i, (B, T, Q) in enumerate([(1, 9, 1), (3, 64, 7), (16, 9, 300), (16, 64, 300)]):
        xs, cols, out, c_min, c_max = _case(1, B, T, Q, 900 + i)
        d_cols = torch.from_numpy(cols).to(DEV)
        want = engine.stack_windows(out.clone(), xs[0], d_cols, _scale(6.0), c_min, c_max)
        got = engine.stack_windows_legs(out.clone(), xs, d_cols, _scale(6.0), c_min, c_max)
        assert not torch.equal(got, out) and torch.equal(got, want)


def test_stack_legs_leaves_untouched_elements_alone():
    """`out` pre-filled with a pattern that holds -0.0 (adding +0.0 would turn it into +0.0): the columns outside [c_min, c_max] and the
    columns inside it that no entry lists keep their bits."""
    Q, T, L = 7, 9, 3
    cols = np.stack([np.arange(10, 19), np.arange(14, 23)]).astype(np.int32)
    cols[0, 6] = -1
    cols[1, 2] = -1                                                # column 16 is listed by these two entries only
    cols[1, 8] = -1
    n_cols = 40
    g = torch.Generator(device=DEV).manual_seed(3)
    xs = [torch.randn((2, Q, T), device=DEV, generator=g) for _ in range(L)]
    out = torch.randn((Q, n_cols), device=DEV, generator=g)
    out[:, ::2] = -0.0
    before = out.clone().view(torch.int32)
    engine.stack_windows_legs(out, xs, torch.from_numpy(cols).to(DEV), _scale(6.0), 8, 30)     # a range wider than the listed columns
    after = out.view(torch.int32)
    listed = np.unique(cols[cols >= 0])
    assert 16 not in listed and listed[0] == 10 and listed[-1] == 21
    quiet = np.setdiff1d(np.arange(n_cols), listed)
    quiet_d = torch.from_numpy(quiet).to(DEV)
    assert torch.equal(after[:, quiet_d], before[:, quiet_d])
    assert int((before[:, quiet_d] == -2 ** 31).sum()) >= Q * 10   # the pattern's -0.0 is among them, inside and outside the range
    assert bool((after[:, torch.from_numpy(listed).to(DEV)] != before[:, torch.from_numpy(listed).to(DEV)]).all())
    assert torch.equal(out, _torch_loop(before.view(torch.float32), xs, cols, 6.0))


def test_stack_legs_column_listed_twice_adds_twice_in_kjl_order():
    """`window_cols_table` never makes such a row; the kernel's answer to one is pinned all the same: both entries add, in (k, j, l) order
    -- which for that column is NOT `for leg: index_add_`."""
    Q, L, T = 3, 2, 9
    cols = np.stack([np.array([5, 6, 5, 7, 8, -1, 9, 10, 6]), np.array([6, 7, 8, 9, 9, 10, 11, 12, -1])]).astype(np.int32)
    g = torch.Generator(device=DEV).manual_seed(4)
    xs = [torch.randn((2, Q, T), device=DEV, generator=g) for _ in range(L)]
    out = torch.randn((Q, 16), device=DEV, generator=g)
    scale = np.float32(1.0) / np.float32(6.0)
    want = out.cpu().numpy().copy()
    h = [x.cpu().numpy() for x in xs]
    for k in range(2):
        for j in range(T):
            if cols[k, j] >= 0:
                for l in range(L):
                    want[:, cols[k, j]] = want[:, cols[k, j]] + h[l][k, :, j] * scale          # float32: product rounded, then added
    assert want.dtype == np.float32
    got = engine.stack_windows_legs(out.clone(), xs, torch.from_numpy(cols).to(DEV), float(scale), 5, 12)
    assert np.array_equal(got.cpu().numpy(), want)


def test_stack_legs_64_bit_offsets():
    """`Out_2` of 70 000 x 32 768 = 2.29e9 elements (rows 65 536.. lie beyond element 2^31), two overlapping windows of two legs at the far
    end of the axis; the touched columns against `index_add_` on a [Q, n_touched] reference, the columns around them untouched."""
    Q, n_cols, T = 70000, 32768, 9
    if torch.cuda.mem_get_info(torch.device(DEV))[0] < 24 * 2 ** 30:
        pytest.skip("needs 24 GB of free device memory for an Out_2 of more than 2^31 elements")
    cols = np.stack([np.arange(n_cols - 12, n_cols - 3), np.arange(n_cols - 9, n_cols)]).astype(np.int32)
    cols[0, 2] = -1
    cols[1, 8] = -1
    touched = np.unique(cols[cols >= 0])
    assert Q * n_cols > 2 ** 31 and touched[0] == n_cols - 12 and touched[-1] == n_cols - 2
    g = torch.Generator(device=DEV).manual_seed(7)
    xs = [torch.randn((2, Q, T), device=DEV, generator=g) for _ in range(2)]
    out = torch.zeros((Q, n_cols), dtype=torch.float32, device=DEV)
    engine.stack_windows_legs(out, xs, torch.from_numpy(cols).to(DEV), _scale(6.0), int(touched[0]), int(touched[-1]))
    ref = torch.zeros((Q, len(touched)), dtype=torch.float32, device=DEV)
    for k in range(2):
        keep = np.flatnonzero(cols[k] >= 0)
        local = torch.from_numpy(np.searchsorted(touched, cols[k][keep])).to(DEV)
        for x in xs:
            ref.index_add_(1, local, x[k][:, torch.from_numpy(keep).to(DEV)] / 6.0)
    torch.cuda.synchronize()
    got = out[:, torch.from_numpy(touched).to(DEV).long()]
    assert torch.equal(got, ref)
    assert float(got[65536:].abs().min()) > 0                  # written beyond element 2^31, every touched column
    assert not bool(out[:, 0].any()) and not bool(out[:, n_cols - 13].any()) and not bool(out[:, n_cols - 1].any())
    assert not bool(out[:, n_cols - 10].any())                 # inside [c_min, c_max], listed by no window (its only entry was dropped)
    assert not bool(out[Q - 1, :n_cols - 12].any()) and not bool(out[0, :n_cols - 12].any())
    del out
    torch.cuda.empty_cache()


def test_stack_legs_rejects_bad_arguments():
    lib = _lib.load()
    z = torch.zeros((4, 9), dtype=torch.float32, device=DEV)
    x = torch.ones((1, 4, 9), dtype=torch.float32, device=DEV)
    c = torch.arange(9, dtype=torch.int32, device=DEV).view(1, 9)
    p = lambda t: t.data_ptr()
    tab = lambda *ptrs: (ctypes.c_void_p * len(ptrs))(*ptrs)
    many = tab(*([p(x)] * 33))
    one, two_null = tab(p(x)), tab(p(x), None)
    good = (one, 1, p(c), 1, 4, 9, 1.0, p(z), 9, 0, 8)
    bad = [(None, 1) + good[2:],                                               # a null table
           (two_null, 2) + good[2:],                                           # a null pointer inside the table
           (one, 0) + good[2:], (many, 33) + good[2:],                         # n_legs outside 1..32
           (one, 1, p(c), 17, 4, 9, 1.0, p(z), 9, 0, 8), (one, 1, p(c), 0, 4, 9, 1.0, p(z), 9, 0, 8),      # the sibling's range errors
           (one, 1, p(c), 1, 4, 65, 1.0, p(z), 9, 0, 8), (one, 1, p(c), 1, 4, 0, 1.0, p(z), 9, 0, 8),
           (one, 1, p(c), 1, -1, 9, 1.0, p(z), 9, 0, 8), (one, 1, p(c), 1, 4, 9, 1.0, p(z), 0, 0, 0),
           (one, 1, p(c), 1, 4, 9, 1.0, p(z), 2 ** 31, 0, 8), (one, 1, p(c), 1, 4, 9, 1.0, p(z), 9, 0, 9),
           (one, 1, p(c), 1, 4, 9, 1.0, p(z), 9, 5, 4), (one, 1, p(c), 1, 4, 9, 1.0, p(z), 9, -1, 4),
           (one, 1, None, 1, 4, 9, 1.0, p(z), 9, 0, 8), (one, 1, p(c), 1, 4, 9, 1.0, None, 9, 0, 8)]
    for args in bad:
        assert lib.genie_stack_windows_legs(*args, None) == -1                 # GENIE_ERR_ARG
        assert b"genie_stack_windows_legs" in lib.genie_last_error()
    torch.cuda.synchronize()
    assert not bool(z.any())
    with pytest.raises(ValueError):
        engine.stack_windows_legs(z, [], c, 1.0, 0, 8)
    with pytest.raises(ValueError):
        engine.stack_windows_legs(z, [x] * 33, c, 1.0, 0, 8)
    with pytest.raises(ValueError):
        engine.stack_windows_legs(z, [x, x[:, :2]], c, 1.0, 0, 8)
    with pytest.raises(ValueError):
        engine.stack_windows_legs(z, [x.cpu()], c, 1.0, 0, 8)
    assert not bool(z.any())
    assert lib.genie_stack_windows_legs(*good, None) == 0                      # (the good call those were derived from)
    torch.cuda.synchronize()
    assert bool((z == 1.0).all())


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------

S = 17


def _new_net(dev):
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=dev)
    net.load_state_dict({k: v.clone() for k, v in Case("tiny_6x40").weights.items()})
    net.eval()
    return net


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)


def _grid_leg(geom, dev):
    net = _new_net(dev)
    net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), _t(geom.edge_attr(), dev),
                             _t(geom.locs, dev), _t(geom.x_grid, dev))
    return apply.GridLeg(net, geom.x_grid, geom.travel_times().astype(np.float32))


def _subgraph_leg(geom, dev):
    """A `use_subgraph` leg: every source node keeps its 5 nearest stations (the irregular product graph of
    test_sign_input_flag_reaches_every_context_builder, at this size)."""
    G = geom.n_grid
    d = np.linalg.norm(geom.x_grid[:, None, :2] - geom.locs[None, :, :2], axis=2)
    keep = np.zeros(d.shape, dtype=bool)
    keep[np.arange(G)[:, None], np.argsort(d, axis=1)[:, :5]] = True
    src_i, sta_i = np.nonzero(keep)
    pairs = np.stack((sta_i, src_i))
    A_in_sta, A_in_src, A_src_in_prod = graph.subgraph_product_edges(geom.A_sta_sta, geom.A_src_src, pairs)
    gea = graph.GraphEdges(x=_t(geom.edge_attr().reshape(G, S, 3)[src_i, sta_i], dev), edge_index=A_src_in_prod.to(dev))
    net = _new_net(dev)
    net.set_adjacencies(A_in_sta.to(dev), A_in_src.to(dev), gea, gea, torch.from_numpy(pairs).long().to(dev),
                        torch.from_numpy(geom.A_src_src).to(dev), None, None, None, None, _t(geom.locs, dev), _t(geom.x_grid, dev))
    assert pairs.shape[1] == 5 * G
    return apply.GridLeg(net, geom.x_grid, geom.travel_times().astype(np.float32), pairs=pairs)


@functools.lru_cache(maxsize=None)
def _setup(dev=DEV):
    """17 stations, the picks of `_tiny` in test_window_parallel_gpu.py (a run has more windows than one flush of 16), and legs on two
    grids of the same stations (same seed and station count: same stations): G = 64 three times over (a model each), G = 48, and G = 48
    as an irregular product graph. The queries of the G = 64 geometry serve every leg."""
    g64 = synthetic.Geometry(S, 64, L=60e3, n_query=12, seed=71)
    g48 = synthetic.Geometry(S, 48, L=60e3, n_query=12, seed=71)
    assert np.array_equal(g64.locs, g48.locs)
    P = synthetic.make_picks(g64, 300, seed=72)
    P[:, 0] = P[:, 0] * 0.75 + 5000.0
    P = P[np.argsort(P[:, 0], kind="stable")]
    trv = g64.travel_times().astype(np.float32)
    max_t = float(np.ceil(max(trv.max(), g48.travel_times().max()) + 1.0))      # one max_t for the day, whichever grids run
    s = types.SimpleNamespace(g64=g64, g48=g48, P=P, trv=trv, max_t=max_t, dev=dev)
    s.picks = apply.ResidentPicks(P, np.arange(S), S, dev)
    s.legs = {"a": _grid_leg(g64, dev), "b": _grid_leg(g48, dev), "a2": _grid_leg(g64, dev), "sub": _subgraph_leg(g48, dev)}
    s.xq, s.locs = g64.x_query, g64.locs
    s.kw = dict(min_required_picks=5)
    return s


def _legs_run(names, **kw):
    s = _setup()
    out = apply.apply_windows_legs([s.legs[n] for n in names], s.picks, s.xq, s.locs, s.max_t, **dict(s.kw, **kw))
    torch.cuda.synchronize()
    return out


def _coarse_axis(step_size):
    """The 1.5 s-spacing axis of test_fused_stacking_with_a_column_listed_twice_in_a_window: every window lists columns twice."""
    s = _setup()
    tsteps, offsets, step, n_overlap, dt_win = apply.window_schedule(s.P[:, 0], s.max_t, t_win=6.0, step_size=step_size)
    coarse = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, 2.0 * dt_win)
    table = apply.window_cols_table(coarse, tsteps, offsets, step_size == "half")
    assert ((table >= 0).sum(1) < len(offsets) - (1 if step_size == "half" else 0)).all()
    return coarse


@functools.lru_cache(maxsize=None)
def _reference(names, step_size, coarse=False):
    """The reference's day loop from existing public calls (process_continuous_days.py:761-810): per kept window, per leg, the embedding,
    the literal `forward_fixed_source` and `Out_2.index_add_(1, cols, x[:, keep, 0] / (n_overlap * L))`. Returns (Out_2 window-major,
    the leg-major sum of the L single-leg stacks of the same read-outs -- what a caller had to form before --, times used)."""
    s = _setup()
    dev, sig = s.dev, synthetic.KERNEL_SIG_T
    legs = [s.legs[n] for n in names]
    tsteps, offsets, step, n_overlap, dt_win = apply.window_schedule(s.P[:, 0], s.max_t, t_win=6.0, step_size=step_size)
    axis = _coarse_axis(step_size) if coarse else np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)
    times = apply.windows_with_enough_picks(s.P[:, 0], tsteps, s.max_t, 6.0, 5)
    xq, tq, locs = _t(s.xq, dev), _t(offsets.reshape(-1, 1), dev), _t(s.locs, dev)
    d = n_overlap * len(legs)
    Out_2 = torch.zeros((xq.shape[0], len(axis)), dtype=torch.float32, device=dev)
    per_leg = [torch.zeros_like(Out_2) for _ in legs]
    used = []
    with torch.no_grad():
        for t0 in times:
            cols, keep = apply.window_columns(axis, t0, offsets, step_size == "half")
            cols, keep = torch.from_numpy(cols).to(dev), torch.from_numpy(keep).to(dev)
            for l, leg in enumerate(legs):
                em = leg.embed(s.picks, t0, s.max_t, sig, apply._dt_embed(sig, None))
                if em is None:
                    continue                                                                   # :792-793
                x = leg.net.forward_fixed_source(em[0], em[1], None, None, None, locs, leg.x_grid_cart, xq, tq)[1]
                Out_2.index_add_(1, cols, x[:, keep, 0] / d)
                per_leg[l].index_add_(1, cols, x[:, keep, 0] / d)
                if l == 0:
                    used.append(t0)
    leg_major = per_leg[0]
    for o in per_leg[1:]:
        leg_major = leg_major + o
    torch.cuda.synchronize()
    return Out_2, leg_major, np.asarray(used)


@pytest.mark.parametrize("tail_batch", [1, 3, 16])
@pytest.mark.parametrize("step_size", ["full", "partial", "half"])
def test_one_leg_is_the_single_grid_loop(step_size, tail_batch):
    s = _setup()
    kw = dict(step_size=step_size, tail_batch=tail_batch)
    want, times = apply.apply_windows_device(s.legs["a"].net, s.g64, s.P, s.trv, stack_on_device=True, max_t=s.max_t, **dict(s.kw, **kw))
    torch.cuda.synchronize()
    got, times_l = _legs_run(("a",), **kw)
    assert len(times) >= (17 if step_size != "full" else 6) and np.array_equal(times, times_l)
    assert float(want.abs().max()) > 0 and torch.equal(got, want)


@pytest.mark.parametrize("step_size", ["full", "partial", "half"])
def test_both_entries_with_one_grid_are_the_reference_loop(step_size):
    """The two entries share one loop, so comparing them with each other pins neither: each is held here against the reference loop
    written from public calls (embed, the literal `forward_fixed_source`, `index_add_`), the single-grid entry on its torch arm and on
    its fused arm, at three flush sizes."""
    s = _setup()
    want, _, times = _reference(("a",), step_size)
    single = lambda **kw: apply.apply_windows_device(s.legs["a"].net, s.g64, s.P, s.trv, max_t=s.max_t, step_size=step_size, **dict(s.kw, **kw))
    runs = [single(stack_on_device=False, tail_batch=3), single(stack_on_device=True, tail_batch=16),
            _legs_run(("a",), step_size=step_size, tail_batch=1)]
    torch.cuda.synchronize()
    assert len(times) >= (17 if step_size != "full" else 6) and int((want != 0).sum()) > 100
    for got, times_used in runs:
        assert np.array_equal(times, times_used)
        assert torch.equal(got, want)


@pytest.mark.parametrize("names", [("a", "b"), ("a", "b", "a2")])
@pytest.mark.parametrize("step_size", ["full", "partial", "half"])
def test_two_and_three_legs_are_the_reference_loop(step_size, names):
    """Window-major, as the reference adds: `((a_0 + b_0) + a_1) + b_1 ...`. The leg-major sum `(a_0 + a_1) + (b_0 + b_1)` of L single-leg
    stacks differs from it in rounding wherever a column is fed by more than one window ('partial': 3, 'half': 2; picks of seed 72) --
    and cannot differ with 'full', where one window feeds a column and both orders are `(0 + a) + b`."""
    want, leg_major, times = _reference(names, step_size)
    got, times_l = _legs_run(names, step_size=step_size, tail_batch=3 if step_size == "half" else 16)
    assert len(times) >= (17 if step_size != "full" else 6) and np.array_equal(times, times_l)
    assert int((want != 0).sum()) > 100
    assert torch.equal(got, want)
    assert torch.equal(got, leg_major) == (step_size == "full")


def test_three_legs_with_a_column_listed_twice_in_a_window():
    names = ("a", "b", "a2")
    want, _, times = _reference(names, "half", coarse=True)
    got, times_l = _legs_run(names, step_size="half", tsteps_abs=_coarse_axis("half"))
    assert np.array_equal(times, times_l) and int((want != 0).sum()) > 100
    assert torch.equal(got, want)


def test_a_use_subgraph_leg_beside_an_ordinary_one():
    want, leg_major, times = _reference(("a", "sub"), "half")
    got, times_l = _legs_run(("a", "sub"))
    assert np.array_equal(times, times_l) and int((want != 0).sum()) > 100
    assert torch.equal(got, want) and not torch.equal(got, leg_major)
    assert not torch.equal(got, _reference(("a", "b"), "half")[0])             # (the irregular graph does change that leg's read-out)


def test_refusals_come_before_any_launch():
    s = _setup()
    a = s.legs["a"]
    args = (s.picks, s.xq, s.locs, s.max_t)
    sharded = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, shard=(0, 2))
    assert sharded.is_sharded
    torch.cuda.synchronize()
    pending = a.net.pending_windows
    with pytest.raises(NotImplementedError, match="sharded"):
        apply.apply_windows_legs([a, types.SimpleNamespace(net=sharded, device=a.device, n_sta=S)], *args)
    with pytest.raises(ValueError, match="no grid leg"):
        apply.apply_windows_legs([], *args)
    with pytest.raises(ValueError, match="at most 32"):
        apply.apply_windows_legs([a] * 33, *args)
    with pytest.raises(ValueError, match="share one model"):
        apply.apply_windows_legs([a, a], *args)
    fewer = apply.ResidentPicks(s.P[s.P[:, 1] < 16], np.arange(16), S, DEV)
    with pytest.raises(ValueError, match="17 stations, the picks 16"):
        apply.apply_windows_legs([a, s.legs["b"]], fewer, s.xq, s.locs[:16], s.max_t)
    with pytest.raises(ValueError, match="lives on"):
        apply.apply_windows_legs([a], apply.ResidentPicks(s.P, np.arange(S), S, "cpu"), s.xq, s.locs, s.max_t)
    assert a.net.pending_windows == pending == 0


# ---- window-parallel -----------------------------------------------------------------------------------------------------------------------------

WP_LEGS = ("a", "b")


def _rank_ordered_sum(parts):
    tot = np.zeros_like(parts[0])
    for p in parts:
        tot = tot + p                                          # fp32, rank order
    return tot


@functools.lru_cache(maxsize=None)
def _one_gpu():
    out, times = _legs_run(WP_LEGS)
    return out.cpu().numpy(), times


@functools.lru_cache(maxsize=None)
def _partials(world, n_times=None):
    """([partial Out_2 (numpy) per rank], [times per rank], info of rank 0); `n_times`: of the day's first windows only."""
    kw = {} if n_times is None else dict(times=_one_gpu()[1][:n_times])
    outs, times, info = [], [], None
    for r in range(world):
        res = _legs_run(WP_LEGS, window_parallel=(r, world), return_info=(r == 0), **kw)
        outs.append(res[0].cpu().numpy())
        times.append(res[1])
        info = res[2] if r == 0 else info
    return outs, times, info


@pytest.mark.parametrize("world", [2, 3, 5])
def test_window_parallel_partials(world):
    ref, ref_times = _one_gpu()
    parts, times, info = _partials(world)
    blocks = apply.window_blocks(len(ref_times), world)
    assert info["windows"] == blocks and info["rank"] == 0 and info["exact_merge"]
    assert np.array_equal(np.concatenate(times), ref_times)
    for r, (lo, hi) in enumerate(blocks):                      # a rank's partial: one GPU over that block of windows, bit for bit
        alone, t_alone = _legs_run(WP_LEGS, times=ref_times[lo:hi])
        assert np.array_equal(t_alone, times[r]) and hi > lo
        assert np.array_equal(alone.cpu().numpy(), parts[r]) and parts[r].any()
    tot = _rank_ordered_sum(parts)
    single = info["ranks_per_column"] == 1
    assert single.sum() > (info["ranks_per_column"] >= 2).sum() >= world - 1
    assert np.abs(ref[:, single]).max() > 0 and np.array_equal(tot[:, single], ref[:, single])


def test_window_parallel_empty_blocks_contribute_zeros():
    ref_times = _one_gpu()[1]
    parts, times, info = _partials(5, 3)
    assert [len(t) for t in times] == [1, 1, 1, 0, 0] and info["columns"][3:] == [None, None]
    assert all(p.any() for p in parts[:3]) and not parts[3].any() and not parts[4].any()
    whole, t_whole = _legs_run(WP_LEGS, times=ref_times[:3])
    assert np.array_equal(np.concatenate(times), t_whole)
    single = info["ranks_per_column"] == 1
    assert np.array_equal(_rank_ordered_sum(parts)[:, single], whole.cpu().numpy()[:, single]) and single.any()


def _free_port():
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    return port


def _worker(rank, world, port, backend, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(DEV)
    timeout = datetime.timedelta(seconds=60)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(DEV), timeout=timeout)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timeout)
    try:
        out, times, info = _legs_run(WP_LEGS, window_parallel=True, return_info=True)
        ret[rank] = (out.cpu().numpy(), np.asarray(times), info["windows"], info["rank"], dist.get_backend())
    finally:
        dist.destroy_process_group()


def _run_group(world, backend):
    import torch.multiprocessing as mp
    ref, ref_times = _one_gpu()
    parts, _, info = _partials(world)
    want = _rank_ordered_sum(parts)
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), backend, ret), nprocs=world, join=True)
    assert len(ret) == world
    for rank in range(world):
        out, times, windows, r, be = ret[rank]
        assert r == rank and windows == info["windows"] and be == backend
        assert np.array_equal(times, ref_times)                # every rank returns the full list
        assert np.array_equal(out, want)                       # the rank-ordered sum of the tuple-form partials, on every rank
    if world == 1:
        assert np.array_equal(want, ref)


def test_window_parallel_two_processes_on_one_gpu_over_gloo():
    _run_group(2, "gloo")


def test_window_parallel_three_processes_on_one_gpu_over_gloo():
    _run_group(3, "gloo")


def test_window_parallel_world1_rccl_device_all_reduce():
    _run_group(1, "nccl")
