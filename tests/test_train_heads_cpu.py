"""CPU: the cases and references of tests/train_head_cases.py are what they claim to be, before any kernel is compared with them
(tests/test_train_heads_gpu.py).

For every case: no pick lies within a margin of a decision boundary, and the fp32 and fp64 restatements take IDENTICAL discrete decisions
(kept edges, time bins, sign features, e0max), so that the two gradients differ by rounding alone; `e0max > 0` (`remainder(e1, e0max)`);
fewer than 150 000 kept edges; the shapes sit where the kernels change path; the rows that must come out exactly zero exist, in the
references too. The references themselves: the fp32 one is the existing restatement on the module's own layers bit for bit, the fp64
gradient agrees with central differences on a tiny case per head."""
import numpy as np
import pytest
import torch

from genie_amd import module
from tests import restatements as R
from tests import train_head_cases as C


# ---- LocalSliceLgCollapse P / S ------------------------------------------------------------------------------------------------------

def test_lslc_shapes_sit_on_the_kernels_boundaries():
    n = {name: C.lslc_case(name).n for name in C.LSLC_CASES}
    tile, wg = C.LS_TILE, C.LS_TILE * C.LS_WAVES
    assert (n["n1"], n["n16"], n["n17"], n["n65"]) == (1, tile, tile + 1, wg + 1)
    assert n["stride"] == C.LS_MAX_GRID * wg + 17 and (n["stride"] + tile - 1) // tile > C.LS_MAX_GRID * C.LS_WAVES     # tiles stride past the grid
    assert C.lslc_case("only_s").coef[0] is None and C.lslc_case("only_p").coef[1] is None
    assert all(c is not None for name in C.LSLC_CASES[:7] for c in C.lslc_case(name).coef)


@pytest.mark.parametrize("name", C.LSLC_CASES)
def test_lslc_case_margins_and_decisions(name):
    c = C.lslc_case(name)
    _, trv, ep, es, dtp = C.lslc_graph(c.slow)
    tp, ip = c.tpick.numpy(), c.ipick.numpy()
    assert tp.dtype == np.float32 and c.s.dtype == torch.float32
    x = C.lslc_bins(tp, dtp)
    assert (np.abs(x - np.round(x)) >= C.MARGIN_BIN).all() and (x > 0).all() and (np.floor(x) <= len(dtp) - 1).all()
    assert (ip >= 0).all() and (ip < C.LS_S).all()
    rel = C.lslc_rel(tp, ip, trv, (ep, es), dtp)
    assert (np.abs(np.abs(rel) - 2.0 * C.EPS) >= C.MARGIN_FILTER).all()
    ti64, keep64, node64 = C.lslc_decisions(c, torch.float64)
    ti32, keep32, node32 = C.lslc_decisions(c, torch.float32)
    assert torch.equal(ti64, ti32) and torch.equal(keep64, keep32) and torch.equal(node64, node32)
    assert torch.equal(ti64, torch.from_numpy(np.floor(x).astype(np.int64)))
    assert int(node64.min()) >= 0 and int(node64.max()) < C.LS_S * C.LS_G                 # every index the kernel reads is inside its table
    assert (c.ipick * len(dtp) * C.LS_K + ti64 * C.LS_K + C.LS_K <= c.tables[0].numel()).all()
    # the edge cap bounds the cost of one restatement call: here per head (10 257 picks x 10 nodes is the stride case's size by itself)
    assert int(keep64[0].sum()) < C.MAX_EDGES and int(keep64[1].sum()) < C.MAX_EDGES
    # zero rows of the cotangents, and picks that no node explains
    for h in range(2):
        if c.coef[h] is not None:
            z = ~c.coef[h].abs().amax(dim=1).bool()
            assert torch.equal(z, torch.from_numpy(c.zero_rows[h])) and (not z.all() if c.n > 1 else bool(z[0]) == (h == 0))
            assert z.any() or c.n == 1                                                  # (one pick: P's row is zero, S's is not)
    if name == "shared_bin":                                                           # one (station, time bin) for 24 picks
        k = c.planted["shared"]
        assert len(k) >= 20 and len(set(ip[k])) == 1 and len(set(ti64[k].tolist())) == 1
        for h in range(2):
            assert int(torch.bincount(node64[h][keep64[h]]).max()) >= 20              # runs of k_seg_rows longer than 1
    if name == "no_edge":                                                              # cnt = 0: den = 1
        assert len(c.planted["no_p"]) >= 5 and not keep64[0][c.planted["no_p"]].any() and keep64[1][c.planted["no_p"]].any()
        assert len(c.planted["no_s"]) >= 5 and not keep64[1][c.planted["no_s"]].any() and keep64[0][c.planted["no_s"]].any()
        for h, key in ((0, "no_p"), (1, "no_s")):                                       # ... and some of them carry a cotangent
            assert c.coef[h][c.planted[key]].abs().amax(dim=1).bool().sum() >= 3


@pytest.mark.parametrize("name", C.LSLC_CASES)
def test_lslc_references_agree_on_the_exactly_zero_rows(name):
    c, ref = C.lslc_case(name), C.lslc_reference(name)
    un = C.lslc_untouched(c)
    for key in ("f64", "f32"):
        assert not ref[key]["rows"]["d_s_rows"][un].any(), key
        for h, hn in enumerate("PS"):
            if c.coef[h] is None:                                                      # a head without a cotangent: no gradient at all
                assert all(not g.any() for k, g in ref[key]["params"].items() if k.startswith("LocalSliceLgCollapse" + hn))
    if name in ("n1", "n16", "n17", "shared_bin", "no_edge", "only_s", "only_p"):      # the cases meant for it
        assert un.float().mean() >= 0.10
    assert set(ref["f64"]["params"]) == set(C.LSLC_PARAMS)
    assert float(ref["f64"]["rows"]["d_s_rows"].abs().max()) > 1e-3


def test_lslc_fp32_reference_is_the_existing_restatement_bit_for_bit():
    c = C.lslc_case("n65")
    for h, hn in enumerate("PS"):
        mod = module.LocalSliceLgCollapse(30, 15)
        mod.load_state_dict({k.split(".", 1)[1]: v for k, v in C.weights().items() if k.startswith("LocalSliceLgCollapse%s." % hn)})
        with torch.no_grad():
            out = R.local_slice_collapse(mod, c.tables[h], c.dtp, c.tpick, c.ipick, c.phase.view(-1, 1), c.s, c.tlatent[:, h].reshape(-1, 1))
        assert torch.equal(out, C.lslc_reference("n65")["f32"]["out"]["arv_" + hn.lower()])


def _central_difference(loss, t, idx, h):
    """(loss(t[idx] + h) - loss(t[idx] - h)) / 2h of a float64 leaf tensor, restored afterwards."""
    with torch.no_grad():
        old = t[idx].clone()
        t[idx] = old + h
        up = float(loss())
        t[idx] = old - h
        down = float(loss())
        t[idx] = old
    return (up - down) / (2.0 * h)


def _check_against_differences(loss, tensors, grads, n_random=3):
    """For each tensor: the entry with the largest gradient and a few seeded random ones, 1e-6 of the tensor's largest gradient."""
    rng = np.random.default_rng(99)
    for key, t in tensors.items():
        g = grads[key]
        flat = [int(g.abs().argmax())] + [int(k) for k in rng.integers(0, g.numel(), n_random)]
        for k in flat:
            idx = tuple(int(i) for i in np.unravel_index(k, tuple(g.shape)))
            fd = _central_difference(loss, t, idx, 1e-5)
            assert abs(fd - float(g[idx])) <= 1e-6 * float(g.abs().max()), (key, idx, fd, float(g[idx]))


def test_lslc_fp64_reference_agrees_with_central_differences():
    c, ref = C.lslc_case("n17"), C.lslc_reference("n17")["f64"]
    heads = C.lslc_heads(torch.float64)
    s = c.s.double()
    loss = lambda: C.lslc_loss(c, torch.float64, heads, s)[0]
    tensors, grads = {"d_s_rows": s}, {"d_s_rows": ref["rows"]["d_s_rows"]}
    for hd in heads:
        for k, p in hd.params.items():
            tensors[k], grads[k] = p, ref["params"][k]
    with torch.no_grad():
        _check_against_differences(loss, tensors, grads)


# ---- the arrival head -----------------------------------------------------------------------------------------------------------------

def test_arrival_shapes_sit_on_the_kernels_boundaries():
    e = C.arrival_case("edges")
    assert e.counts == C.ARRIVAL_EDGE_L and e.n_src == 2 and C.arrival_case("edges_1src").n_src == 1
    L = set(e.counts)
    assert {0, 1} <= L and {C.AR_TILE - 1, C.AR_TILE} <= L                       # L + 1 entries (the null pick): one tile exactly, one over
    assert {C.AE_TCH - 1, C.AE_TCH, C.AE_TCH + 1} <= L                           # rounds of four waves / staged target chunks
    assert 2 * C.AE_TCH + 1 in L and C.AR_CAP + 1 in L                           # a third chunk; a second streaming-softmax chunk
    for k in ("tpick", "ipick", "arv_p", "arv_s", "phase"):
        assert torch.equal(getattr(e, k), getattr(C.arrival_case("edges_1src"), k))
    w = C.arrival_case("wide")
    assert w.n_src * w.n_sta > C.ARRT_GRID and w.n_src * w.n > 64 * C.ARRT_GRID
    nf = C.arrival_case("null_filtered")
    assert nf.n_src == 3 and (nf.stime.abs() >= 2.0 * C.EPS).sum() == 1
    assert (C.arrival_case("no_null").stime.abs() >= 2.0 * C.EPS).all()


@pytest.mark.parametrize("name", C.ARRIVAL_CASES)
def test_arrival_case_margins_and_decisions(name):
    c = C.arrival_case(name)
    tp, ip = c.tpick.numpy(), c.ipick.numpy()
    assert tp.dtype == np.float32 and (ip >= 0).all() and (ip < c.n_sta).all()
    assert np.array_equal(np.bincount(ip, minlength=c.n_sta), np.asarray(c.counts))
    rel = np.abs(C.arrival_rel(tp, ip, c.trv.numpy(), c.stime.numpy()))
    assert (np.abs(rel - 2.0 * C.EPS) >= C.MARGIN_FILTER).all() and (rel >= C.MARGIN_SIGN).all()
    st = c.stime.double().abs()
    assert ((st - 2.0 * C.EPS).abs() >= C.MARGIN_FILTER).all() and (st >= C.MARGIN_SIGN).all()       # the null pick: rel = -stime
    d64, d32 = C.arrival_decisions(c, torch.float64), C.arrival_decisions(c, torch.float32)
    for a, b in zip(d64[:3], d32[:3]):
        assert torch.equal(a, b)
    assert d64[3] == d32[3] and d64[3] > 0                                              # remainder(e1, e0max) is defined
    assert torch.equal(d64[4], d32[4].double()) and torch.equal(d64[5], d32[5].double())
    assert d64[4].abs().min() == 1 and d64[5].abs().min() == 1
    assert 0 < len(d64[0]) < C.MAX_EDGES
    if name == "no_null":
        assert d64[3] < c.n and not (d64[0] == c.n).any()                                # e0max is a real pick
    else:
        assert d64[3] == c.n
    if name == "null_filtered":
        assert not ((d64[0] == c.n) & (d64[2] == c.n_src - 1)).any() and ((d64[0] == c.n) & (d64[2] == 0)).any()
    # picks that no source explains, rows of the cotangent that are zero
    un = C.arrival_unexplained(c)
    assert un.float().mean() >= 0.10 and not un.all()
    z = ~c.coef.abs().amax(dim=2).bool()
    assert torch.equal(z, torch.from_numpy(c.zero_rows)) and z.any() and not z.all(dim=1).any()
    ref = C.arrival_reference(name)
    for key in ("f64", "f32"):
        for k in ("d_arrival_p", "d_arrival_s"):
            assert not ref[key]["rows"][k][un].any() and ref[key]["rows"][k][~un].abs().amax(dim=1).bool().any(), (key, k)
    assert set(ref["f64"]["params"]) == set(C.ARRIVAL_PARAMS)


def test_arrival_fp32_reference_is_the_existing_restatement_bit_for_bit():
    c = C.arrival_case("null_filtered")
    mod = module.StationSourceAttentionMergedPhases(30, 15, 2, 15, n_heads=3)
    mod.load_state_dict({k.split(".", 1)[1]: v for k, v in C.weights().items() if k.startswith("Arrivals.")})
    with torch.no_grad():
        out = R.arrivals(mod, c.n_src, c.stime, c.x_src, c.trv, c.arv_p, c.arv_s, c.tpick, c.ipick, c.phase.view(-1, 1))
    assert torch.equal(out, C.arrival_reference("null_filtered")["f32"]["out"]["out"])


@pytest.mark.parametrize("name", ["null_filtered", "no_null"])
def test_arrival_fp64_reference_agrees_with_central_differences(name):
    c, ref = C.arrival_case(name), C.arrival_reference(name)["f64"]
    head = C.arrival_head(torch.float64)
    x_src, arv_p, arv_s = c.x_src.double(), c.arv_p.double(), c.arv_s.double()
    loss = lambda: C.arrival_loss(c, torch.float64, head, x_src, arv_p, arv_s)[0]
    tensors = {"d_src_embed": x_src, "d_arrival_p": arv_p, "d_arrival_s": arv_s}
    grads = dict(ref["rows"])
    for k, p in head.params.items():
        tensors[k], grads[k] = p, ref["params"][k]
    with torch.no_grad():
        _check_against_differences(loss, tensors, grads, n_random=2)


def test_the_one_wider_factor_belongs_to_a_sum_of_cancelling_terms():
    """Arrivals.f_arrival_query_2.bias has the factor 16: its gradient is what a sum of far larger terms leaves over (the softmax's
    d score sums to zero per target), in the cases with the long stations most of all."""
    assert C.FACTORS == {"Arrivals.f_arrival_query_2.bias": 16.0}
    assert C.arrival_query_bias_cancellation("edges") > 1000.0 and C.arrival_query_bias_cancellation("no_null") > 1000.0


def test_references_are_built_once():
    a, b = C.lslc_reference("n16"), C.arrival_reference("no_null")
    assert a is C.lslc_reference("n16") and b is C.arrival_reference("no_null")
    assert C.FACTOR == 4.0 and C.FLOOR == 2.0 ** -20 and all(4.0 < f <= 16.0 for f in C.FACTORS.values())
