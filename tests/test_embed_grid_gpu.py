"""GPU: the pick -> Slice/Mask embedding (k_embed_scatter, k_embed_edges, k_embed_gather behind `HipPath.embed_window`) against
oracle/embed_oracle.py on the quantised, grid-aligned inputs of tests/embed_grid_cases.py, where every truncation of the embedding sits
on or next to an integer. tests/test_embed_grid_cpu.py asserts, on the oracle's arithmetic alone, that the inputs are what they claim.

Mask: equal, every element (no reference value lies within 1e-5 of the 0.01 threshold). Slice: within one float32 ulp at 1, 2^-23 -- both
sides cast a float64 `exp` of the same argument to float32, the arguments differ by a contracted multiply-add in the sample time
(~1e-12) and, for dt = 0.3, by the step numpy's `arange` takes (`(start + dt) - start`, within 1e-11 of dt, times up to 194 samples), so
the results differ by at most one rounding step of a value <= 1. A larger difference is a wrong index (a Gaussian moved by dt: 3e-3 or
more), not noise."""
import functools

import numpy as np
import pytest
import torch

from genie_amd import apply, engine, graph, module, synthetic
from oracle import embed_oracle as E
from tests import embed_grid_cases as C
from tests.util import Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ULP = 2.0 ** -23
ids = C.case_id


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)


def _model(shape, **kw):
    c = Case("tiny_6x40")
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, **kw)
    net.load_state_dict({k: v.clone() for k, v in c.weights.items()})
    net.eval()
    return net


def _base_model(shape, **kw):
    """A model on the Cartesian product of the shape's base graphs (station processing order: the space-filling curve of the stations)."""
    geom = C.geometry(shape)
    net = _model(shape, **kw)
    net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), _t(geom.edge_attr()), _t(geom.locs), _t(geom.x_grid))
    return net


@functools.lru_cache(maxsize=None)
def _context(shape, irregular):
    """The HIP context the cases of a shape embed on: a bare one on the Cartesian product, the model's own (`set_adjacencies` from
    product edge lists) on the irregular product graph."""
    S, G = C.SHAPES[shape]
    geom = C.geometry(shape)
    if not irregular:
        return engine.HipPath(S, G, engine.csr_from_edges(torch.from_numpy(geom.A_sta_sta), S),
                              engine.csr_from_edges(torch.from_numpy(geom.A_src_src), G), device=DEV)
    pairs = C.product_pairs(shape, True)
    assert pairs.shape[1] < S * G
    A_in_sta, A_in_src, A_src_in_prod = graph.subgraph_product_edges(geom.A_sta_sta, geom.A_src_src, pairs)
    gea = graph.GraphEdges(x=_t(geom.edge_attr().reshape(G, S, 3)[pairs[1], pairs[0]]), edge_index=A_src_in_prod.to(DEV))
    net = _model(shape)
    net.set_adjacencies(A_in_sta.to(DEV), A_in_src.to(DEV), gea, gea, torch.from_numpy(pairs).long().to(DEV),
                        torch.from_numpy(geom.A_src_src).to(DEV), None, None, None, None, _t(geom.locs), _t(geom.x_grid))
    _context.keep = getattr(_context, "keep", []) + [net]
    return net._hip


@functools.lru_cache(maxsize=None)
def _device_inputs(c, no_phase=False, only=None):
    """What `embed_window` takes for a case: the picks of the window's range, found by the product's own range search on the
    time-sorted picks (stations S, S + 1 and phases 2, -1 included: the kernel has to skip them), and the travel-time rows.
    `only`: a key of the case's sets -- the day holds those picks alone."""
    (P, t0, max_t, sig, dt, trv, pairs), sets = C.case(*c)
    if only is not None:
        P = P[sets[only]]
    Pt = P[np.argsort(P[:, 0], kind="stable")]
    lo, hi = apply.picks_in_embed_range(Pt[:, 0], t0, max_t, sig)
    ph = np.zeros(hi - lo) if no_phase else Pt[lo:hi, 4]
    return (torch.from_numpy(Pt[lo:hi, 0].copy()).to(DEV), torch.from_numpy(Pt[lo:hi, 1].astype(np.int32)).to(DEV),
            torch.from_numpy(ph.astype(np.int32)).to(DEV), t0, max_t, sig, dt, _t(trv[pairs[1], pairs[0]]))


def _compare(what, Slice, Mask, want_S, want_M):
    want_S, want_M = torch.from_numpy(np.array(want_S)), torch.from_numpy(np.array(want_M))      # (the shared reference stays read-only)
    err = float((Slice.cpu().double() - want_S.double()).abs().max())
    print("%s: max|Slice - oracle| = %.3g (%.2f ulp at 1), Mask mismatches %d" % (what, err, err / ULP, int((Mask.cpu() != want_M).sum())))
    assert torch.equal(Mask.cpu(), want_M), what
    assert err <= ULP, what


@pytest.mark.parametrize("use_phase_types", [True, False], ids=["phases", "no-phases"])
@pytest.mark.parametrize("use_sign_input", [False, True], ids=["plain", "sign"])
@pytest.mark.parametrize("c", C.CASES, ids=ids)
def test_embedding_matches_the_oracle_on_grid_aligned_times(c, use_sign_input, use_phase_types):
    sets = C.case(*c)[1]
    hp = _context(c[1], c[3])
    hp.set_sign_input(use_sign_input)
    hp.set_phase_types(use_phase_types)
    args = _device_inputs(c, no_phase=not use_phase_types)
    assert args[0].numel() > 150
    Slice, Mask = hp.embed_window(*args)
    want_S, want_M = C.reference(c, use_sign_input, not use_phase_types)
    what = "%s sign %d phases %d" % (ids(c), use_sign_input, use_phase_types)
    if use_phase_types:
        _compare(what, Slice, Mask, want_S, want_M)
    else:       # columns 2, 3 are zero; columns 0, 1 are those of the reference run with every phase 0
        assert float(Slice[:, 2:].abs().max()) == 0.0 and float(Mask[:, 2:].abs().max()) == 0.0
        _compare(what, Slice[:, :2], Mask[:, :2], np.ascontiguousarray(want_S[:, :2]), np.ascontiguousarray(want_M[:, :2]))
    for tag in ("node_first", "node_last", "node_empty"):                            # (g), (e): zeroed edge samples, a station without picks
        rows = torch.from_numpy(sets.get(tag, np.zeros(0, dtype=np.int64))).to(DEV)
        cols = torch.from_numpy(want_S[sets.get(tag, np.zeros(0, dtype=np.int64))] == 0).to(DEV)
        assert bool((Slice[rows][cols] == 0).all())
    if c[0] == "E" and use_sign_input:                                              # (h): bit-equal neighbours, sign 0, feature +0.0
        rows = torch.from_numpy(sets["half_nodes"]).to(DEV)
        assert rows.numel() >= 2 and not bool(Slice[rows].view(torch.int32).any()) and not bool(Mask[rows].any())
    again = hp.embed_window(*args)
    assert torch.equal(again[0].view(torch.int32), Slice.view(torch.int32)) and torch.equal(again[1], Mask)


@pytest.mark.parametrize("c", [C.CASES[0], C.CASES[2], C.CASES[7]], ids=ids)
def test_a_window_whose_only_picks_sit_on_its_borders_embeds_to_zeros(c):
    hp = _context(c[1], c[3])
    hp.set_sign_input(True)
    hp.set_phase_types(True)
    args = _device_inputs(c, only="border_out")
    assert args[0].numel() == 0 and len(C.case(*c)[1]["border_out"]) == 2             # both are outside the strict range
    hp.embed_window(*_device_inputs(c))                                              # (the series workspace holds another window's samples)
    Slice, Mask = hp.embed_window(*args)
    assert not bool(Slice.view(torch.int32).any()) and not bool(Mask.any())
    assert C.reference(c, True)[0].any()


@pytest.mark.parametrize("use_sign_input", [False, True], ids=["plain", "sign"])
@pytest.mark.parametrize("c", [c for c in C.CASES if c[1] == "40x33"], ids=ids)
def test_presplit_embedding_in_station_processing_order(c, use_sign_input):
    """genie_embed_window_split at 40 x 33: the split rows and the message-mask row `mm` go to the workspace in the station processing
    order (`sta_inv`), 33 source nodes are no multiple of a node tile. The returned Slice / Mask are the plain call's, bit for bit, and
    the path run on them (split pass skipped) is the path a fresh context runs on the plain call's Slice / Mask. The workspace holds NaN
    bit patterns beforehand, as in test_presplit_embedding_with_poisoned_workspace."""
    S, G = C.SHAPES[c[1]]
    geom = C.geometry(c[1])
    assert not np.array_equal(np.asarray(engine.sfc_order(geom.locs)), np.arange(S))
    args = _device_inputs(c)
    pos = _t(geom.x_grid)
    fresh = _base_model(c[1], use_sign_input=use_sign_input)
    fresh._hip.sync_weights(fresh._path_params, fresh._weight_split())
    S0, M0 = fresh._hip.embed_window(*args)
    _compare("%s sign %d (plain call)" % (ids(c), use_sign_input), S0, M0, *C.reference(c, use_sign_input))
    out0, _, bip0 = fresh._hip.path_fwd(S0, M0, fresh._edge_attr, pos, want_bip=True)
    net = _base_model(c[1], use_sign_input=use_sign_input)
    net._hip.ws.fill_(255)
    net._hip.sync_weights(net._path_params, net._weight_split())
    assert net._hip.stage_precision()["f16x2_active"]                               # the split rows exist
    S1, M1 = net._hip.embed_window(*args, presplit=True)
    assert torch.equal(S1.view(torch.int32), S0.view(torch.int32)) and torch.equal(M1, M0)
    out1, _, bip1 = net._hip.path_fwd(S1, M1, net._edge_attr, pos, want_bip=True)
    assert bool(torch.isfinite(out1).all()) and float(out1.abs().max()) > 0
    assert torch.equal(bip1, bip0) and torch.equal(out1, out0)


def test_a_grid_aligned_day_end_to_end_offline_and_online():
    """A family-N day of 120 s at 14 x 60, window starts on whole multiples of 3 s: `apply_windows_device(stack_on_device=True)` against
    a host loop that embeds every window with the oracle and runs the same model's `forward_fixed_source` on the oracle's Slice / Mask
    (1e-5 absolute, the bound of test_device_apply_loop_matches_oracle); `OnlineDay` fed in chunks cut at times that are pick times --
    whole seconds among them, where a window's strict upper border, `t_now` and a pick coincide -- bit-equal to the offline loop."""
    shape = "14x60"
    S, G = C.SHAPES[shape]
    geom = C.geometry(shape)
    P, trv = C.day(shape)
    max_t, sig, dt = C.MAX_T, C.SIGMA, 0.3
    net = _base_model(shape)
    tsteps, offsets, step, n_overlap, dt_win = apply.window_schedule(P[:, 0], max_t, t_win=6.0, step_size="half")
    tsteps_abs = np.arange(tsteps.min() - 3.0, tsteps.max() + 3.0 + dt_win, dt_win)
    assert np.array_equal(tsteps, np.round(tsteps)) and step == 3.0
    A = C.product_pairs(shape, False)
    locs, xg, xq, tq = _t(geom.locs), _t(geom.x_grid), _t(geom.x_query), _t(offsets.reshape(-1, 1))
    want = torch.zeros((geom.x_query.shape[0], len(tsteps_abs)), dtype=torch.float64)
    lo, hi = apply._embed_ranges(P[:, 0], tsteps, max_t, sig)
    with torch.no_grad():
        for t0 in tsteps[hi > lo]:
            Slice, Mask = E.extract_input_from_data(P, float(t0), np.arange(S), S, trv, A, max_t, sig, dt)
            _, x = net.forward_fixed_source(torch.from_numpy(Slice).to(DEV), torch.from_numpy(Mask).to(DEV), None, None, None, locs, xg, xq, tq)
            cols, keep = apply.window_columns(tsteps_abs, float(t0), offsets, True)
            want[:, cols] += x[:, keep, 0].double().cpu() / n_overlap
    Out_2, used = apply.apply_windows_device(net, geom, P, trv, tsteps_abs=tsteps_abs, times=tsteps, step_size="half", max_t=max_t,
                                             kernel_sig_t=sig, dt_embed=dt, tail_batch=16, stack_on_device=True)
    torch.cuda.synchronize()
    assert np.array_equal(used, tsteps[hi > lo]) and len(used) >= 40
    err = float((Out_2.cpu().double() - want).abs().max())
    print("grid-aligned day, %d windows: max|Out_2 - oracle chain| = %.3g (max|Out_2| %.3g)" % (len(used), err, float(want.abs().max())))
    assert float(want.abs().max()) > 1e-3 and err <= 1e-5
    # online: every cut is a pick's time; that pick has not been fed when a window whose strict border it sits on becomes ready
    t = P[:, 0]
    whole = np.unique(t[t == np.round(t)])
    third = np.unique(t[np.abs(t / 0.3 - np.round(t / 0.3)) < 1e-9])
    cuts = np.unique(np.concatenate((whole[2::3], third[5::12], [t[-1]])))
    borders = np.concatenate((tsteps - 2 * sig, tsteps + max_t + 2 * sig))
    assert len(cuts) >= 12 and np.isin(cuts, borders).sum() >= 3
    day = apply.OnlineDay(net, geom, trv, tsteps_abs, times=tsteps, max_t=max_t, kernel_sig_t=sig, dt_embed=dt, tail_batch=16)
    fed = np.zeros(len(P), dtype=bool)
    blocks = []
    for t_now in cuts:
        take = ~fed & (t < t_now)
        fed |= take
        first, block = day.feed(P[take], float(t_now))
        assert first + block.shape[1] == day.closed
        blocks.append(block)
    assert not fed.all()
    blocks.append(day.feed(P[~fed], np.inf)[1])
    got = torch.cat(blocks, dim=1)
    assert np.array_equal(np.asarray(day.times_used), used)
    assert torch.equal(got, Out_2)
