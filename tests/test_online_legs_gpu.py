"""GPU: the online chain over several source grids -- `apply.OnlineDay` given a list of `GridLeg`s, and `apply.OnlineCatalogue` on such a
day -- against the offline multi-leg twin, `apply_windows_legs(legs, ...)` -> `detect_refine_associate(legs, ...)`, bit for bit.

The day is the small one of tests/test_online_catalogue_gpu.py (17 stations x 64 source nodes, 100 queries, 300 picks over ~100 s,
`tiny_6x40` weights, time-pointer tables set), whose model is leg a. Legs b and c are built the way tests/test_apply_legs_gpu.py builds
its legs -- a model each, the same stations, grids of 48 and 56 nodes -- with the weights perturbed deterministically, so that the legs'
read-outs differ and a wrong leg order or a dropped leg changes the bits (asserted in `_setup`). The chunkings, the blobs added to
`Out_2` on both sides and the fixture's requirements on the catalogue are those of that file. No tolerance anywhere."""
import functools
import types

import numpy as np
import pytest
import torch

from genie_amd import apply, graph, module, postproc, synthetic
from tests import test_online_catalogue_gpu as cat_t
from tests import test_online_resume_gpu as res_t
from tests.util import Case

pytestmark = pytest.mark.gpu

DEV = cat_t.DEV
S = 17


def _perturbed(weights, phase):
    """The fixture's weights plus 2 % of each tensor's mean magnitude times sin(index + phase): deterministic, another model."""
    out = {}
    for name, v in weights.items():
        v = v.clone()
        if v.is_floating_point() and v.numel():
            wave = torch.sin(torch.arange(v.numel(), dtype=torch.float64) + phase).reshape(v.shape).to(v.dtype)
            v = v + 0.02 * float(v.abs().mean()) * wave
        out[name] = v
    return out


def _leg(G, phase, max_t, n_sta=S, pointers=True):
    """A model of its own on a grid of G nodes over the first `n_sta` stations of seed 71, as `cat_t._setup` sets leg a up."""
    geom = synthetic.Geometry(n_sta, G, L=60e3, n_query=100, seed=71)
    trv_t = geom.travel_times().astype(np.float32)
    assert float(trv_t.max()) < max_t                            # one max_t for the day, whichever grids run
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV)
    net.load_state_dict(_perturbed(Case("tiny_6x40").weights, phase))
    net.eval()
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)
    args = [torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), torch.from_numpy(geom.edge_attr()).to(DEV), f(geom.locs),
            f(geom.x_grid)]
    if pointers:
        sig = synthetic.KERNEL_SIG_T
        edges_p, edges_s, dt_partition = graph.time_pointers(trv_t, max_t=max_t, dt=sig / 5.0, k=10, win=2.0 * sig)
        args += [torch.from_numpy(edges_p).to(DEV), torch.from_numpy(edges_s).to(DEV), f(dt_partition), f(trv_t.reshape(-1, 2))]
    net.set_adjacencies_base(*args)
    return apply.GridLeg(net, geom.x_grid, trv_t), geom


@functools.lru_cache(maxsize=None)
def _setup():
    net, geom, P, trv_t, max_t, tsteps, ts = cat_t._setup()
    s = types.SimpleNamespace(net=net, geom=geom, P=P, trv=trv_t, max_t=max_t, tsteps=tsteps, ts=ts)
    s.legs = [apply.GridLeg(net, geom.x_grid, trv_t)]
    for G, phase in ((48, 1.0), (56, 2.0)):
        leg, g = _leg(G, phase, max_t)
        assert np.array_equal(g.locs, geom.locs) and g.x_grid.shape[0] == G
        s.legs.append(leg)
    s.picks = apply.ResidentPicks(P, np.arange(S), S, DEV)
    s.xq = np.asarray(geom.x_query, dtype=np.float64)
    # the legs' own days differ, so leg order and every leg's presence show in the stacked bits
    singles = [_offline([leg], 16)[0] for leg in s.legs]
    assert all(float(o.abs().max()) > 0 for o in singles)
    assert not torch.equal(singles[0], singles[1]) and not torch.equal(singles[0], singles[2]) and not torch.equal(singles[1], singles[2])
    return s


def _offline(legs, tail_batch, picks=None, **kw):
    net, geom, P, trv_t, max_t, tsteps, ts = cat_t._setup()
    picks = picks if picks is not None else apply.ResidentPicks(P, np.arange(S), S, DEV)
    kw.setdefault("times", tsteps)
    out, used = apply.apply_windows_legs(legs, picks, geom.x_query, geom.locs, max_t, tsteps_abs=ts, tail_batch=tail_batch, **kw)
    torch.cuda.synchronize()
    return out, used


@functools.lru_cache(maxsize=None)
def _twin_day(n_legs, tail_batch):
    out, used = _offline(_setup().legs[:n_legs], tail_batch)
    assert float(out.abs().max()) > 0 and len(used) >= 20
    return out, used


def _day(legs, tail_batch=16, **kw):
    s = _setup()
    kw.setdefault("times", s.tsteps)
    return apply.OnlineDay(legs, s.geom, None, s.ts, max_t=s.max_t, tail_batch=tail_batch, **kw)


def _chunks(how):
    P = _setup().P
    return cat_t._chunks(how) or [(P, float(P[0, 0]))]


def _feed_all(day, how):
    blocks, at = [], 0
    for rows, t_now in _chunks(how):
        first, block = day.feed(rows, t_now)
        assert first == at and day.closed == first + block.shape[1]
        at = day.closed
        blocks.append(block)
    first, block = day.finish()
    assert first == at and day.closed == len(day.tsteps_abs) == at + block.shape[1]
    return torch.cat(blocks + [block], dim=1)


# ---- 1. the day ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _leg_major(tail_batch):
    """Half the sum of the two single-leg online days of legs a and b: `(sum_w a_w) + (sum_w b_w)`, what a caller without the multi-leg
    day had to form (halving is exact in fp32, so this is the sum of the two days stacked with the two-leg scale)."""
    a, b = (_feed_all(_day(leg, tail_batch), "whole") for leg in _setup().legs[:2])
    return 0.5 * (a + b)


@pytest.mark.parametrize("how", ["whole", "second", "random"])
@pytest.mark.parametrize("tail_batch", [1, 16])
@pytest.mark.parametrize("n_legs", [2, 3])
def test_online_day_over_legs_equals_apply_windows_legs(n_legs, tail_batch, how):
    s = _setup()
    want, used = _twin_day(n_legs, tail_batch)
    day = _day(s.legs[:n_legs], tail_batch)
    assert day.lanes == s.legs[:n_legs] and day.lane is day.lanes[0] and day._fingerprint()["n_legs"] == n_legs
    one = _day(s.legs[0], tail_batch)                            # nothing of the plan depends on L but the scale
    assert np.array_equal(day.h_cols, one.h_cols) and np.array_equal(day.frontiers, one.frontiers)
    assert (day.ring_min, day.ring_cols) == (one.ring_min, one.ring_cols) and day.scale != one.scale
    got = _feed_all(day, how)
    assert np.array_equal(day.times_used, used) and len(day.picks) == 0
    assert got.dtype == want.dtype and torch.equal(got, want)
    if n_legs == 2:
        assert not torch.equal(got, _leg_major(tail_batch))      # window-major, not the leg-major sum of two days


def test_a_list_of_one_leg_is_the_single_leg_day():
    s = _setup()
    days = [_day([s.legs[0]]), _day(s.legs[0]), apply.OnlineDay(s.net, s.geom, s.trv, s.ts, times=s.tsteps, max_t=s.max_t, tail_batch=16)]
    assert all(len(d.lanes) == 1 and d.lane is d.lanes[0] and d._fingerprint()["n_legs"] == 1 for d in days)
    assert days[0].scale == days[2].scale
    n_blocks = 0
    for rows, t_now in _chunks("random") + [(None, np.inf)]:
        outs = [d.feed(rows, t_now) for d in days]
        for first, block in outs[:2]:
            assert first == outs[2][0] and torch.equal(block, outs[2][1])
        n_blocks += outs[2][1].shape[1] > 0
    assert n_blocks >= 5 and days[2].closed == len(s.ts)
    assert torch.equal(_feed_all(_day([s.legs[0]]), "whole"), _twin_day(1, 16)[0])


def test_a_window_dropped_inside_a_batch():
    """A gap of 20 s in the picks and `min_required_picks = 15`: the count rule keeps windows 3..25 and 30..35 of the 41 candidates, so
    the batch of windows 16..31 (the whole day in one call: batches start at 0, 16, 32) runs 16..25 and 30, 31 -- the rows of the column
    table are gathered on the device -- with two legs' read-outs behind them."""
    s = _setup()
    centre = s.tsteps[24] + s.max_t / 2.0
    P2 = s.P[(s.P[:, 0] < centre - 10.0) | (s.P[:, 0] > centre + 10.0)]
    assert np.array_equal(apply.window_schedule(P2[:, 0], s.max_t, t_win=6.0, step_size="half")[0], s.tsteps)
    kept = np.isin(s.tsteps, apply.windows_with_enough_picks(P2[:, 0], s.tsteps, s.max_t, 6.0, 15))
    in_batch = np.flatnonzero(kept[16:32])
    assert kept[16] and kept[31] and 0 < len(in_batch) < 16 and in_batch[-1] - in_batch[0] + 1 > len(in_batch)
    want, used = _offline(s.legs[:2], 16, picks=apply.ResidentPicks(P2, np.arange(S), S, DEV), times=None, min_required_picks=15)
    assert np.array_equal(used, s.tsteps[kept]) and want.shape[1] == len(s.ts)
    day = _day(s.legs[:2], 16, min_required_picks=15)
    batches, add = [], day._add
    day._add = lambda xs, ws: batches.append((len(xs), list(ws))) or add(xs, ws)
    blocks = [day.feed(P2, float(P2[0, 0]))[1], day.finish()[1]]
    assert all(n == 2 for n, _ in batches)
    assert any(ws[-1] - ws[0] + 1 > len(ws) for _, ws in batches)            # a window was dropped between two that ran
    assert day.n_run == len(s.tsteps) and len(day.times_used) == int(kept.sum()) < len(s.tsteps)
    assert np.array_equal(day.times_used, used)
    assert torch.equal(torch.cat(blocks, dim=1), want)


# ---- 4. the catalogue ----------------------------------------------------------------------------------------------------------------------

def _detect(Out_2, legs):
    s = _setup()
    a = cat_t._chain_args()
    D = cat_t.DETECT
    return apply.detect_refine_associate(legs, s.picks, Out_2, s.xq, s.ts, a[0], a[1], a[2], s.max_t, *a[3:], D["thresh"], D["src_t_kernel"],
                                         D["dt_win"], D["break_win"], D["tc_win"], D["sp_win"], rand=apply.PhiloxCloud(cat_t.KEY),
                                         ftrns2_device=cat_t.IDENT, detect_on_device=True)


@functools.lru_cache(maxsize=None)
def _twin_catalogue():
    """The offline dict over legs a and b, computed once, with the requirements of `cat_t._twin` asserted on it."""
    s = _setup()
    Out_2 = _twin_day(2, 16)[0] + cat_t._field()
    want = _detect(Out_2, s.legs[:2])
    torch.cuda.synchronize()
    det = postproc.OnlineDetector(*cat_t._detect_args(s.xq, s.ts), device=DEV)
    units = sum(len(det.push(c, Out_2[:, c:c + 1].contiguous())) > 0 for c in range(len(s.ts))) + (len(det.finish()) > 0)
    print("twin over two legs: %d detections, %d retained, %d detector units" % (len(want["srcs"]), len(want["srcs_refined"]), units))
    assert len(want["srcs_refined"]) >= 3 and units >= 2 and len(want["srcs_refined"]) < len(want["srcs"])
    assert len(np.unique(want["srcs_refined"][:, 3])) == len(want["srcs_refined"])
    assert sum(o.numel() > 0 for o in want["Out_p_save"]) >= 3
    # both legs are read: leg a alone, on the same field, gives other likelihoods
    alone = _detect(_twin_day(1, 16)[0] + cat_t._field(), s.legs[:1])
    assert len(alone["Out_p_save"]) != len(want["Out_p_save"]) or not all(torch.equal(x, y) for x, y in zip(alone["Out_p_save"], want["Out_p_save"]))
    return want


def _catalogue(legs, pick_lists="device", **day_kw):
    s = _setup()
    day = _day(legs, 16, **day_kw)
    feed, field = day.feed, cat_t._field()
    day.feed = lambda P_chunk, t_now: (lambda first, block: (first, block + field[:, first:first + block.shape[1]]))(*feed(P_chunk, t_now))
    det = postproc.OnlineDetector(*cat_t._detect_args(s.xq, s.ts), device=DEV)
    cat = apply.OnlineCatalogue(day, det, *cat_t._chain_args(), cat_t.DETECT["tc_win"], cat_t.DETECT["sp_win"],
                                rand=apply.PhiloxCloud(cat_t.KEY), ftrns2_device=cat_t.IDENT, pick_lists=pick_lists)
    return day, det, cat


@pytest.mark.parametrize("pick_lists", ["torch", "device"])
@pytest.mark.parametrize("how", ["whole", "second", "random"])
def test_online_catalogue_over_legs_equals_the_offline_twin(how, pick_lists):
    s = _setup()
    want = _twin_catalogue()
    day, det, cat = _catalogue(s.legs[:2], pick_lists)
    assert cat.legs == s.legs[:2]
    parts = [cat.push(rows, t_now) for rows, t_now in _chunks(how)]
    parts.append(cat.finish())
    assert cat.pending == 0 and cat.undecided == 0 and det.held == 0 and day.closed == len(s.ts) and len(day.picks) == 0
    res_t._assert_same_return(cat_t._concat(parts), want)
    if how == "second":
        assert sum(len(p["srcs_refined"]) for p in parts[:-1]) >= 1          # sources came out final before the day ended


# ---- 5. save and resume --------------------------------------------------------------------------------------------------------------------

def _day_chunks():
    """[(rows of P, t_now)] at irregular cuts, then one `t_now` behind the last window's reads (before `finish`)."""
    s = _setup()
    rng = np.random.default_rng(9)
    cuts = list(s.P[0, 0] + np.cumsum(rng.uniform(0.5, 9.0, 14))) + [float(s.P[-1, 0]) + s.max_t + 30.0]
    out, lo = [], 0
    for t_now in cuts:
        hi = int(np.searchsorted(s.P[:, 0], t_now, side="left"))
        out.append((s.P[lo:max(lo, hi)], float(t_now)))
        lo = max(lo, hi)
    assert lo == len(s.P)
    return out


@pytest.mark.parametrize("tail_batch", [1, 16])
def test_a_saved_two_leg_day_resumes_bit_equal(tail_batch):
    s = _setup()
    legs = s.legs[:2]
    want, used = _twin_day(2, tail_batch)
    chunks = _day_chunks()
    day = _day(legs, tail_batch)
    blocks, resumed, cut = [], [], None                          # resumed: (object, its blocks)
    for i, (rows, t_now) in enumerate(chunks):
        first, block = day.feed(rows, t_now)
        blocks.append(block)
        for new, theirs in resumed:
            first_n, block_n = new.feed(rows, t_now)
            assert first_n == first and torch.equal(block_n, block), i
            res_t._assert_same_day(new, day)
            theirs.append(block_n)
        if cut is not None or not res_t._early_cut_ok(day):
            continue
        cut = i                                                  # windows unrun, open non-zero columns, a retained pick behind t_now
        state = day.state_dict()
        assert res_t._host_only(state) and state["fingerprint"]["n_legs"] == 2
        assert state["ring_block"].shape == (want.shape[0], day.last_col + 1 - day.closed) and bool(state["ring_block"].any())
        assert day.n_run < len(day.times) and sorted(state) == sorted(_day(legs[0], tail_batch).state_dict())      # nothing else joins
        loaded = res_t._through_torch_save(state)
        for ring_cols in (None, day.ring_min + 3):
            new = _day(legs, tail_batch, ring_cols=ring_cols)
            assert new.ring_cols == (day.ring_min if ring_cols is None else day.ring_min + 3)
            new.load_state_dict(loaded)
            res_t._assert_same_day(new, day)
            resumed.append((new, []))
        # a state of two legs in a day of one: the first differing field is named, and the day stays a newly constructed one
        # (a one-leg day differs in `scale` first; given the two-leg divisor through `n_grids`, in `n_legs` alone)
        for field, other in (("scale", _day(legs[0], tail_batch)), ("n_legs", _day([legs[1]], tail_batch, n_grids=2.0)),
                             ("scale", _day(s.legs, tail_batch))):
            with pytest.raises(ValueError, match=r"another %s " % field):
                other.load_state_dict(loaded)
            assert res_t._untouched(other), field
    assert cut is not None and cut < len(chunks) - 2
    first, block = day.finish()
    blocks.append(block)
    assert np.array_equal(day.times_used, used) and torch.equal(torch.cat(blocks, dim=1), want)
    for new, theirs in resumed:
        first_n, block_n = new.finish()
        assert first_n == first and torch.equal(block_n, block)
        assert torch.equal(torch.cat(blocks[:cut + 1] + theirs + [block_n], dim=1), want)    # saved + resumed = the offline day


def test_a_saved_two_leg_catalogue_resumes_bit_equal():
    s = _setup()
    want = _twin_catalogue()
    chunks = _chunks("random")
    day, det, cat = _catalogue(s.legs[:2])
    parts, resumed, theirs, cut = [], None, [], None
    for i, (rows, t_now) in enumerate(chunks):
        parts.append(cat.push(rows, t_now))
        if resumed is not None:
            theirs.append(resumed[2].push(rows, t_now))
            res_t._assert_same_return(theirs[-1], parts[-1])
            assert (resumed[2].pending, resumed[2].undecided, resumed[1].held, resumed[1].seen, resumed[0].closed) == \
                (cat.pending, cat.undecided, det.held, det.seen, day.closed)
        if cut is None and cat.undecided > 0 and i < len(chunks) - 1:
            cut = i
            assert any(r[1].numel() > 0 for r in cat._results)               # a likelihood vector with content travels
            state = cat.state_dict()
            assert sorted(state) == ["catalogue", "day", "det"] and res_t._host_only(state) and state["day"]["fingerprint"]["n_legs"] == 2
            loaded = res_t._through_torch_save(state)
            day_x, det_x, cat_x = _catalogue(s.legs[:1], n_grids=2.0)        # a one-leg chain with the two-leg scale: all three or none
            with pytest.raises(ValueError, match="another n_legs "):
                cat_x.load_state_dict(loaded)
            assert res_t._untouched(day_x) and det_x.seen == 0 and det_x.held == 0 and cat_x.n_released == 0 and cat_x.undecided == 0
            resumed = _catalogue(s.legs[:2])
            resumed[2].load_state_dict(loaded)
            assert len(resumed[2]._results) == cat.undecided
            assert all(r[k].device == s.legs[0].x_grid_cart.device for r in resumed[2]._results for k in (0, 1, 2))
            assert resumed[0].retain_from == day.retain_from
    assert cut is not None
    parts.append(cat.finish())
    theirs.append(resumed[2].finish())
    res_t._assert_same_return(theirs[-1], parts[-1])
    assert sum(len(p["srcs_refined"]) for p in theirs) >= 1      # a source that was undecided at the cut came out of the resumed one
    for whole in (parts, parts[:cut + 1] + theirs):
        res_t._assert_same_return(cat_t._concat(whole), want)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_online_day_and_come_before_any_launch():
    s = _setup()
    a, b, c = s.legs
    fewer, _ = _leg(48, 3.0, s.max_t, n_sta=16, pointers=False)
    sharded = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, shard=(0, 2))
    assert sharded.is_sharded and fewer.n_sta == 16
    stand_in = apply.GridLeg.__new__(apply.GridLeg)              # a leg whose model is sharded (a shard cannot be set up in one process)
    stand_in.net, stand_in.device, stand_in.n_sta = sharded, a.device, S
    torch.cuda.synchronize()
    allocations = lambda: torch.cuda.memory_stats().get("allocation.all.allocated", 0)        # a running count: frees do not lower it
    before = allocations()
    cases = [(ValueError, [a, fewer], {}, "stations"), (NotImplementedError, [a, stand_in], {}, "sharded"), (ValueError, [a] * 33, {}, "at most 32"),
             (ValueError, [a, b, c], {"n_grids": 2.0}, "n_grids"), (ValueError, [a, b.net], {}, "bare model"),
             (NotImplementedError, [a, a], {}, "one model per leg"), (ValueError, [], {}, "no grid leg")]
    for exc, legs, kw, word in cases:
        with pytest.raises(exc) as err:
            _day(legs, 16, **kw)
        assert type(err.value) is exc and "OnlineDay" in str(err.value) and word in str(err.value), word
    assert allocations() == before and all(leg.net.pending_windows == 0 for leg in s.legs)
    assert _day([a, b, c], 16, n_grids=3.0).scale == _day([a, b, c], 16).scale         # (n_grids = L is what the default means)
