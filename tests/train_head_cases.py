"""Inputs and references of the backward of the two pick-sized training heads (no GPU needed; a plain module, not a conftest).

The heads are LocalSliceLgCollapse P / S (`engine.lslc_bwd`: k_lslc_bwd + k_seg_rows) and the arrival head (`engine.arrivals_fwd(train=True)`
+ `engine.arrivals_bwd`: k_arrt_tgt_bwd, k_arrt_ent_bwd, k_arrt_ctx_bwd, k_arrt_ctx_red, k_arrt_pick_sum). The reference of a case is
the restatement of the head (tests/restatements.py, pinned to the reference's fixtures by tests/test_assoc_cpu.py) run on the CPU in
float64 on float64 copies of the SAME fp32 inputs and parameters, with `(out * coef).sum()` backpropagated by torch's autograd for a
fixed seeded `coef`; the yardstick is the same computation in fp32. Both are built once per case (`functools.lru_cache`).

The shapes sit on the kernels' own boundaries (named below as the kernels name them). The heads take discrete decisions from
floating-point comparisons -- the 2-eps filters, the time bin `floor((tpick - t0) / dt)`, `sign(rel)`, the null pick's filter --, and a
pick on which fp32 and fp64 disagree changes a gradient by a whole term. The builders therefore redraw every pick that lies, in
float64, within a margin of such a boundary (`MARGIN_*`); tests/test_train_heads_cpu.py checks the margins, that fp32 and fp64 take
identical decisions, and the references themselves (central differences). tests/test_train_heads_gpu.py compares the kernels with
the references."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from genie_amd import graph, module, synthetic
from tests import restatements as R
from tests.util import Case

EPS = float(module.EPS)
WEIGHTS_OF = "cfg1_20x500"
LS_S, LS_G, LS_K = 7, 45, 10                         # the product graph of the LSLC cases (tests/test_hip_parity.py, the forward test)
LS_TILE, LS_WAVES, LS_MAX_GRID = 16, 4, 160          # k_lslc_bwd: picks per wave tile, waves per workgroup, tt_grid's cap
AR_TILE, AE_TCH, AR_CAP, ARRT_GRID = 16, 64, 192, 512    # k_arrt_ent_bwd tiles / staged targets, k_arrivals' softmax chunk, backward grids
MARGIN_FILTER = 1e-3 * EPS                           # | |rel| - 2 eps | of every pick against every node / source it is compared with
MARGIN_SIGN = 1e-4                                   # |rel|: sign(rel) is a feature of the arrival head
MARGIN_BIN = 1e-4                                    # distance of (tpick - t0) / dt from an integer
MAX_EDGES = 150000
REDRAWS = 200

LSLC_CASES = ("n1", "n16", "n17", "n65", "stride", "shared_bin", "no_edge", "only_s", "only_p")
ARRIVAL_CASES = ("edges", "edges_1src", "null_filtered", "no_null", "wide")
ARRIVAL_EDGE_L = (0, 1, 15, 16, 63, 64, 65, 129, 193)
LSLC_PARAMS = tuple("LocalSliceLgCollapse%s.%s" % (h, n) for h in "PS"
                    for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "activate1.weight", "activate2.weight"))
ARRIVAL_PARAMS = tuple("Arrivals.%s" % n for n in (
    "f_src_context_1.weight", "f_src_context_1.bias", "f_src_context_2.weight", "f_src_context_2.bias",
    "f_arrival_query_1.weight", "f_arrival_query_1.bias", "f_arrival_query_2.weight", "f_arrival_query_2.bias",
    "f_values_1.weight", "f_values_1.bias", "f_values_2.weight", "f_values_2.bias", "proj_1.weight", "proj_1.bias",
    "proj_2.weight", "proj_2.bias", "activate1.weight", "activate2.weight", "activate3.weight", "activate4.weight"))


@functools.lru_cache(maxsize=None)
def weights():
    return Case(WEIGHTS_OF).weights


class Head(object):
    """The layers of one head (state_dict prefix `prefix`) as leaf tensors of `dtype` on the CPU, callable like the module's layers:
    what the restatements need of `self`."""

    def __init__(self, prefix, dtype, **attrs):
        self.params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in weights().items() if k.startswith(prefix + ".")}
        assert self.params
        for layer in sorted({k[len(prefix) + 1:].rsplit(".", 1)[0] for k in self.params}):
            w, b = self.params["%s.%s.weight" % (prefix, layer)], self.params.get("%s.%s.bias" % (prefix, layer))
            setattr(self, layer, (lambda x, w=w, b=b: F.linear(x, w, b)) if w.dim() == 2 else (lambda x, w=w: F.prelu(x, w)))
        self.__dict__.update(attrs)

    def grads(self):
        return {k: (torch.zeros_like(p) if p.grad is None else p.grad).detach() for k, p in self.params.items()}


def _zero_rows(rng, n, always, never):
    z = rng.random(n) < 0.2
    z[always], z[never] = True, False
    return z


# ---- LocalSliceLgCollapse P / S ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lslc_graph(slow):
    """(trv [G, S, 2] fp32, table P, table S (int64), dt_partition fp32) of the 7 x 45 geometry of the forward test. `slow`: half the
    velocities and the S arrivals 30 s late, so that the table holds times further than 2 eps from every P arrival (late picks) and
    from every S arrival (early picks): picks there keep no edge."""
    geom = synthetic.Geometry(LS_S, LS_G, L=150e3, n_query=10, seed=LS_S)
    d = np.linalg.norm(geom.x_grid[:, None, :] - geom.locs[None, :, :], axis=2)
    trv = (np.stack((d / 3000.0, d / 1750.0 + 30.0), axis=2) if slow else np.stack((d / 6000.0, d / 3500.0), axis=2)).astype(np.float32)
    ep, es, dtp = graph.time_pointers(trv, max_t=float(trv.max()), dt=0.6, k=LS_K, win=6.0)
    return geom, trv, ep, es, dtp.astype(np.float32)


def lslc_bins(tp, dtp):
    """float64: (tpick - t0) / dt of fp32 picks on the fp32 partition (t0, dt = dtp[1] - dtp[0]: an exact difference in either format)."""
    t0, dt = float(dtp[0]), float(dtp[1]) - float(dtp[0])
    return (tp.astype(np.float64) - t0) / dt


def lslc_rel(tp, ip, trv, tables, dtp):
    """float64 [2, n, 10]: pick time minus the theoretical arrival of the 10 nodes its time bin points at, per head."""
    l_dt = len(dtp)
    ti = np.clip(np.floor(lslc_bins(tp, dtp)).astype(np.int64), 0, l_dt - 1)
    tl = trv.reshape(-1, 2).astype(np.float64)
    return np.stack([tp.astype(np.float64)[:, None] - tl[tab.reshape(LS_S, l_dt, LS_K)[ip, ti], col] for col, tab in enumerate(tables)])


def lslc_near_boundary(tp, ip, trv, tables, dtp):
    """bool [n]: the pick lies within a margin of a decision boundary (or outside the table)."""
    x = lslc_bins(tp, dtp)
    bad = (np.abs(x - np.round(x)) < MARGIN_BIN) | (x < 0) | (x >= len(dtp))
    rel = lslc_rel(tp, ip, trv, tables, dtp)
    return bad | (np.abs(np.abs(rel) - 2.0 * EPS) < MARGIN_FILTER).any(axis=(0, 2))


class LslcCase(object):
    pass


@functools.lru_cache(maxsize=None)
def lslc_case(name):
    assert name in LSLC_CASES
    seed = LSLC_CASES.index(name)
    rng = np.random.default_rng(4100 + seed)
    slow = name == "no_edge"
    geom, trv, ep, es, dtp = lslc_graph(slow)
    l_dt = len(dtp)
    n = {"n1": 1, "n16": LS_TILE, "n17": LS_TILE + 1, "n65": LS_WAVES * LS_TILE + 1, "stride": LS_MAX_GRID * LS_WAVES * LS_TILE + 17,
         "shared_bin": 48, "no_edge": 33, "only_s": 65, "only_p": 65}[name]
    ip = rng.integers(0, LS_S, n)
    lo, hi = np.full(n, float(dtp[0]) + 0.05), np.full(n, float(dtp[-1]) + 0.5)
    c = LslcCase()
    c.planted = {}
    if name == "shared_bin":                         # 24 picks of station 3 inside time bin 41: edges of many picks on the same 10 nodes
        ip[:24], lo[:24], hi[:24] = 3, float(dtp[41]) + 0.03, float(dtp[41]) + 0.57
        c.planted["shared"] = np.arange(24)
    if name == "no_edge":                            # 8 late picks (no P edge: P arrivals end at 55 s), 8 early ones (no S edge: S arrivals start at 30 s)
        lo[:8], hi[:8] = 2.0 * EPS + float(trv[:, :, 0].max()) + 1.0, float(dtp[-1]) + 0.5
        lo[8:16], hi[8:16] = float(dtp[0]) + 0.05, float(trv[:, :, 1].min()) - 2.0 * EPS - 1.0
        c.planted["no_p"], c.planted["no_s"] = np.arange(8), np.arange(8, 16)
    assert (lo < hi).all() and hi.max() < float(dtp[-1]) + 0.6
    tp = rng.uniform(lo, hi).astype(np.float32)
    for _ in range(REDRAWS):
        bad = lslc_near_boundary(tp, ip, trv, (ep, es), dtp)
        if not bad.any():
            break
        tp[bad] = rng.uniform(lo[bad], hi[bad]).astype(np.float32)
    assert not lslc_near_boundary(tp, ip, trv, (ep, es), dtp).any(), "a pick is still within a margin of a boundary"
    t = torch.from_numpy
    c.name, c.n, c.slow, c.geom = name, n, slow, geom
    c.tables = (t(ep).long(), t(es).long())
    c.dtp, c.tlatent = t(dtp), t(np.ascontiguousarray(trv.reshape(LS_G * LS_S, 2)))
    c.tpick, c.ipick = t(tp), t(ip).long()
    c.phase = t(rng.integers(0, 2, n).astype(np.float32))
    c.s = t(rng.normal(0, 1, (LS_G * LS_S, 30)).astype(np.float32))
    coef = [rng.normal(0, 1, (n, 15)).astype(np.float32) for _ in range(2)]
    c.zero_rows = (_zero_rows(rng, n, 0, []), _zero_rows(rng, n, n - 1 if n > 1 else [], 0))       # (n = 1: P's only row is zero, S's is not)
    for k in range(2):
        coef[k][c.zero_rows[k]] = 0.0
    c.coef = (None if name == "only_s" else t(coef[0]), None if name == "only_p" else t(coef[1]))
    return c


def lslc_decisions(c, dtype):
    """The discrete decisions of the restatement in `dtype`, by its own expressions: (time bin [n], kept [2, n, 10] bool, node [2, n, 10])."""
    dtp, tp = c.dtp.to(dtype), c.tpick.to(dtype)
    dt = dtp[1] - dtp[0]
    ti = torch.floor((tp - dtp[0]) / dt).long()
    idx = ((c.ipick * len(dtp) * LS_K + ti * LS_K).view(-1, 1) + torch.arange(LS_K).view(1, -1))
    keep, node = [], []
    for col, tab in enumerate(c.tables):
        e0 = tab[idx]
        keep.append((tp.view(-1, 1) - c.tlatent.to(dtype)[e0, col]).abs() < 2.0 * EPS)
        node.append(e0)
    return ti, torch.stack(keep), torch.stack(node)


def lslc_untouched(c):
    """bool [P]: product nodes that no kept edge of a head with a cotangent points at (their d s rows are exactly zero)."""
    _, keep, node = lslc_decisions(c, torch.float64)
    hit = torch.zeros(LS_G * LS_S, dtype=torch.bool)
    for h in range(2):
        if c.coef[h] is not None:
            hit[node[h][keep[h]]] = True
    return ~hit


def lslc_loss(c, dtype, heads, s, scale=(1.0, 1.0)):
    """(loss, outputs): the restatement of both heads in `dtype` and sum_h scale_h (out_h * coef_h).sum() over the heads with a cotangent."""
    outs, loss = [], 0.0
    for h in range(2):
        o = R.local_slice_collapse(heads[h], c.tables[h], c.dtp.to(dtype), c.tpick.to(dtype), c.ipick, c.phase.to(dtype).view(-1, 1), s,
                                   c.tlatent[:, h].reshape(-1, 1).to(dtype))
        outs.append(o)
        if c.coef[h] is not None:
            loss = loss + scale[h] * (o * c.coef[h].to(dtype)).sum()
    return loss, outs


def lslc_heads(dtype):
    return [Head("LocalSliceLgCollapse" + h, dtype, eps=EPS) for h in "PS"]


def _lslc_run(c, dtype):
    heads = lslc_heads(dtype)
    s = c.s.to(dtype).requires_grad_(True)
    loss, outs = lslc_loss(c, dtype, heads, s)
    loss.backward()
    params = {}
    for h in heads:
        params.update(h.grads())
    return {"out": {"arv_p": outs[0].detach(), "arv_s": outs[1].detach()}, "rows": {"d_s_rows": s.grad.detach()}, "params": params}


@functools.lru_cache(maxsize=None)
def lslc_reference(name):
    """{"f64": ..., "f32": ...}: each {"out": the two heads' outputs, "rows": {"d_s_rows"}, "params": {state_dict name: gradient}}."""
    c = lslc_case(name)
    return {"f64": _lslc_run(c, torch.float64), "f32": _lslc_run(c, torch.float32)}


# ---- the arrival head -----------------------------------------------------------------------------------------------------------------

class ArrivalCase(object):
    pass


def arrival_rel(tp, ip, trv, stime):
    """float64 [2, n_src, n]: pick time minus the theoretical P / S arrival of every source at the pick's station."""
    t = trv.astype(np.float64)[:, ip, :] + stime.astype(np.float64)[:, None, None]
    return np.moveaxis(tp.astype(np.float64)[None, :, None] - t, 2, 0)


def arrival_near_boundary(tp, ip, trv, stime):
    rel = np.abs(arrival_rel(tp, ip, trv, stime))
    return ((np.abs(rel - 2.0 * EPS) < MARGIN_FILTER) | (rel < MARGIN_SIGN)).any(axis=(0, 1))


def _arrival_spec(name):
    """(picks per station, stime, share of picks no source explains, seed)."""
    if name in ("edges", "edges_1src"):
        return list(ARRIVAL_EDGE_L), [3.0, -7.0], 0.15, 1
    if name == "null_filtered":                       # the last source's null pick is filtered (|stime| >= 2 eps)
        return [9, 0, 17, 5, 12], [4.0, -6.5, 2.5 * EPS], 0.15, 2
    if name == "no_null":                             # no source keeps the null pick: e0max is a real pick
        return [21, 16, 3, 25], [2.0 * EPS + 9.0, -2.0 * EPS - 4.0], 0.15, 3
    rng = np.random.default_rng(7)                    # wide: 9 x 57 > ARRT_GRID pairs, 9 x 3650 > 64 x ARRT_GRID targets, few edges
    return rng.multinomial(3650, np.full(57, 1.0 / 57)).tolist(), [-9.5, -7.0, -4.5, -2.0, 1.5, 3.0, 5.5, 8.0, 9.5], 0.94, 4


@functools.lru_cache(maxsize=None)
def arrival_case(name):
    assert name in ARRIVAL_CASES
    counts, stime, far_share, seed = _arrival_spec(name)
    rng = np.random.default_rng(5200 + seed)
    stime = np.asarray(stime, dtype=np.float32)
    n_src, n_sta, n = len(stime), len(counts), int(sum(counts))
    assert all(min(abs(abs(float(v)) - 2.0 * EPS), abs(float(v))) >= 1.0 for v in stime)          # the null pick's own filter and sign
    trv = rng.uniform(5.0, 60.0, (n_src, n_sta, 1)).astype(np.float32)
    trv = np.concatenate((trv, trv * np.float32(1.7)), axis=2)
    ip = rng.permutation(np.repeat(np.arange(n_sta), counts))
    src_of, ph_of = rng.integers(0, n_src, n), rng.integers(0, 2, n)
    far = rng.random(n) < far_share
    far[rng.permutation(n)[:max(1, n // 8)]] = True
    centre = trv[src_of, ip, ph_of].astype(np.float64) + stime[src_of] + np.where(far, 500.0, 0.0)
    draw = lambda m: rng.normal(0, 0.7 * EPS, m)
    tp = (centre + draw(n)).astype(np.float32)
    for _ in range(REDRAWS):
        bad = arrival_near_boundary(tp, ip, trv, stime)
        if not bad.any():
            break
        tp[bad] = (centre[bad] + draw(int(bad.sum()))).astype(np.float32)
    assert not arrival_near_boundary(tp, ip, trv, stime).any(), "a pick is still within a margin of a boundary"
    if name == "edges_1src":                          # the same picks, the first source alone
        n_src, stime, trv = 1, stime[:1], trv[:1]
    t = torch.from_numpy
    c = ArrivalCase()
    c.name, c.n, c.n_src, c.n_sta, c.counts, c.far = name, n, n_src, n_sta, tuple(counts), far
    c.stime, c.trv = t(stime.copy()), t(np.ascontiguousarray(trv))
    c.tpick, c.ipick = t(tp), t(ip).long()
    c.phase = t(rng.integers(0, 2, n).astype(np.float32))
    c.arv_p, c.arv_s = (t(rng.normal(0, 1, (n, 15)).astype(np.float32)) for _ in range(2))
    c.x_src = t(rng.normal(0, 1, (len(_arrival_spec(name)[1]), 30)).astype(np.float32)[:n_src].copy())
    coef = rng.normal(0, 1, (len(_arrival_spec(name)[1]), n, 2)).astype(np.float32)[:n_src].copy()
    c.zero_rows = rng.random((n_src, n)) < 0.2
    c.zero_rows[:, 0] = True
    coef[c.zero_rows] = 0.0
    c.coef = t(coef)
    return c


def arrival_decisions(c, dtype):
    """The discrete decisions of the restatement in `dtype`, by its own expressions: (e0, e1, source of every kept edge, e0max,
    sign(rel P), sign(rel S))."""
    n_src, n_arv, n_sta = c.n_src, c.n, c.n_sta
    stime, trv, tpick = c.stime.to(dtype), c.trv.to(dtype), c.tpick.to(dtype)
    edges = R.station_pick_pairs(c.ipick)
    n_edge = edges.shape[1]
    edges = edges.repeat(1, n_src) + torch.cat((torch.zeros(1, n_src * n_edge, dtype=torch.long),
                                                (torch.arange(n_src) * n_arv).repeat_interleave(n_edge).view(1, -1)), 0)
    sidx = torch.arange(n_src).repeat_interleave(n_edge)
    atime = torch.cat((tpick, tpick.new_full((1,), -EPS)))
    stindex = torch.cat((c.ipick, c.ipick.new_full((1,), n_sta)))
    tsrc = [torch.cat((trv[:, :, k], trv.new_full((n_src, 1), -EPS)), dim=1) for k in range(2)]
    rel = lambda k: atime[edges[0]] - (tsrc[k][sidx, stindex[edges[0]]] + stime[sidx])
    rp, rs = rel(0), rel(1)
    keep = torch.where((rp.abs() < 2.0 * EPS) | (rs.abs() < 2.0 * EPS))[0]
    e0, e1 = edges[0][keep], edges[1][keep]
    return e0, e1, sidx[keep], (int(e0.max()) if len(keep) else -1), torch.sign(rp[keep]), torch.sign(rs[keep])


def arrival_unexplained(c):
    """bool [n]: picks that are the entry (e0) of no kept edge of any source: their d arrival_p / d arrival_s rows are exactly zero."""
    e0 = arrival_decisions(c, torch.float64)[0]
    used = torch.zeros(c.n + 1, dtype=torch.bool)
    used[e0] = True
    return ~used[:c.n]


def arrival_head(dtype):
    return Head("Arrivals", dtype, eps=EPS, n_heads=3, n_latent=15)


def arrival_loss(c, dtype, head, x_src, arv_p, arv_s, coef=None):
    out = R.arrivals(head, c.n_src, c.stime.to(dtype), x_src, c.trv.to(dtype), arv_p, arv_s, c.tpick.to(dtype), c.ipick,
                     c.phase.to(dtype).view(-1, 1))
    return (out * (c.coef if coef is None else coef).to(dtype)).sum(), out


def arrival_query_bias_cancellation(name):
    """The largest per-channel sum over the kept edges of |d query|, over the largest entry of the f_arrival_query_2.bias gradient (the
    sum of d query; float64): how much larger the summed terms of that gradient are than the scale its error is measured on."""
    c, head, kept = arrival_case(name), arrival_head(torch.float64), {}
    layer = head.f_arrival_query_2

    def watched(x):
        kept["q"] = layer(x)
        kept["q"].retain_grad()
        return kept["q"]
    head.f_arrival_query_2 = watched
    x_src, arv_p, arv_s = (v.double().requires_grad_(True) for v in (c.x_src, c.arv_p, c.arv_s))
    arrival_loss(c, torch.float64, head, x_src, arv_p, arv_s)[0].backward()
    return float(kept["q"].grad.abs().sum(dim=0).max() / kept["q"].grad.sum(dim=0).abs().max())


def _arrival_run(c, dtype):
    head = arrival_head(dtype)
    x_src, arv_p, arv_s = (v.to(dtype).requires_grad_(True) for v in (c.x_src, c.arv_p, c.arv_s))
    loss, out = arrival_loss(c, dtype, head, x_src, arv_p, arv_s)
    loss.backward()
    return {"out": {"out": out.detach()}, "rows": {"d_src_embed": x_src.grad.detach(), "d_arrival_p": arv_p.grad.detach(),
                                                    "d_arrival_s": arv_s.grad.detach()}, "params": head.grads()}


@functools.lru_cache(maxsize=None)
def arrival_reference(name):
    c = arrival_case(name)
    return {"f64": _arrival_run(c, torch.float64), "f32": _arrival_run(c, torch.float32)}


# ---- errors ---------------------------------------------------------------------------------------------------------------------------

FLOOR = 2.0 ** -20          # 16 units of fp32 round-off at the tensor's scale: every quantity here is a sum of more than 16 products
FACTOR = 4.0                # a different summation order over the same terms
# Per-tensor factors above 4, by name, each with its reason. A factor above 16 would be a defect to find, not a tolerance to set.
# Arrivals.f_arrival_query_2.bias: the softmax's d score sums to zero over the entries of a target, and the query bias sees d score
# times a context vector that only the self / null link bits vary, so its gradient is what is left of a sum whose terms are 1 300 to
# 3 800 times larger (`arrival_query_bias_cancellation`, pinned by tests/test_train_heads_cpu.py). The kernel sums an entry over its
# targets first, autograd sums edge by edge: two orders of a cancelling sum differ by more than two orders of a plain one. Measured
# ratio up to 13.8 (L = 193 picks on a station), i.e. an error of 1.3e-8 of the summed magnitudes: a quarter of one fp32 round-off.
FACTORS = {"Arrivals.f_arrival_query_2.bias": 16.0}


def param_error(got, ref64):
    """max |got - ref64| / max |ref64| of a parameter gradient (a reference that is zero everywhere asks for exact zeros)."""
    got, ref64 = got.detach().cpu().double().reshape(ref64.shape), ref64.double()
    scale = float(ref64.abs().max())
    if scale == 0.0:
        return 0.0 if not got.any() else float("inf")
    return float((got - ref64).abs().max()) / scale


def row_error(got, ref64):
    """(max over rows of max |got row - ref64 row| / max(max |ref64 row|, 1e-3 max |ref64|), the row that has it)."""
    got, ref64 = got.detach().cpu().double().reshape(ref64.shape), ref64.double()
    scale = torch.clamp(ref64.abs().amax(dim=1), min=1e-3 * float(ref64.abs().max()))
    if float(scale.max()) == 0.0:
        return (0.0 if not got.any() else float("inf")), 0
    e = (got - ref64).abs().amax(dim=1) / scale
    k = int(e.argmax())
    return float(e[k]), k


def bound(name, e_cpu):
    return FACTORS.get(name, FACTOR) * max(e_cpu, FLOOR)
