"""Inputs and references of the P-sized training backward (no GPU needed; a plain module, not a conftest).

The passes are `engine.train_bwd` (k_train_b2, k_train_b1s / k_train_b1p, k_train_b0, k_train_reduce: the front, DataAggregation + the
P-sized half of Bipartite_ReadIn) and `engine.assoc_train_bwd` (k_as_b3, k_train_b1<true>, k_as_b1, k_as_b0, k_as_g: the association
heads, BipartiteGraphReadOutOperator + DataAggregationAssociationPhase). Almost all they return are weight gradients, sums over every
product row; the backward is linear in its cotangent, so a cotangent on one source node (`d_r`) or one product row (`d_s`) makes a
handful of rows the whole answer. The reference of a probe is the oracle's own functions (oracle/genie_oracle.py) run on the CPU in
float64 on float64 copies of the SAME fp32 inputs and weights, with `(r * d_r).sum()` / `(out * d_s).sum()` backpropagated by torch's
autograd; the yardstick is the same computation in fp32. Everything is built once per case (`functools.lru_cache`).

A PReLU gradient jumps at 0, and the kernels read the sign from the fp32 (default training forward: f16x2) pre-activations their
forward saved. A row with a pre-activation within `MARGIN_KINK` of zero (a *kink row*) may therefore not lie in the receptive field
of a probe: the builders search window seeds, `y_latent` seeds and candidate nodes until that holds (at most `REDRAWS` forward runs),
and for the cases small enough for a dense cotangent until the case has no kink row at all. tests/test_train_front_cpu.py checks the
cases and the references, tests/test_train_front_gpu.py compares the kernels with them."""
import contextlib
import functools
import os

import numpy as np
import torch

from genie_amd import graph, synthetic
from oracle import genie_oracle as O
from tests.util import GOLDEN_DIR, Case

FRONT_WEIGHTS_OF, ASSOC_WEIGHTS_OF = "cfg1_20x500", "assoc_7x45"
# k_train_b2 / b1s / b1p / b0, k_as_b3 / b1 / b0: rows per tile; train_grid's workgroups on the 256 CUs of an MI355X (two per CU), waves
# per workgroup, and of the light pass k_train_b2<false, TR_WPB_LIGHT>
TR_TILE, TR_GRID, TR_WAVES, TR_WAVES_LIGHT = 16, 512, 4, 8
MARGIN_KINK = 1e-5               # of a layer's largest |z|: seven times the 1.4e-6 by which the f16x2 forward's pre-activations differ
DENSE_MAX_P = 700                # dense cotangents (and no kink row at all) up to this many product rows
REDRAWS = 200
CASES = ("s3", "s16", "s17", "s33", "ragged", "long", "irregular")
SHAPES = {"s3": (3, 9), "s16": (16, 20), "s17": (17, 33), "s33": (33, 40), "ragged": (21, 40), "long": (3, 4500), "irregular": (14, 50)}
RAGGED_PLANTS = {"sta_no_in": 3, "src_no_in": 5, "sta_unlisted": 7, "src_unlisted": 11}
# a probe on the source node (station) without in-edges reads no source (station) neighbour in either layer, since every row it
# reads belongs to that node (station) too: the gradients of what feeds that mean alone are zero by structure
NO_MEAN = {"src_no_in": ("activate12.weight", "activate22.weight", "l1_t2_1.weight", "l1_t2_1.bias", "l2_t2_1.weight", "l2_t2_1.bias"),
           "sta_no_in": ("activate11.weight", "activate21.weight", "l1_t1_1.weight", "l1_t1_1.bias", "l2_t1_1.weight", "l2_t1_1.bias")}
FRONT_PREFIXES = ("DataAggregation.", "Bipartite_ReadIn.fc1.", "Bipartite_ReadIn.activate1.")
ASSOC_PREFIXES = ("BipartiteGraphReadOutOperator.", "DataAggregationAssociationPhase.")


@functools.lru_cache(maxsize=None)
def weights():
    """One state dict: the `cfg1_20x500` fixture's, with the two association modules of `assoc_7x45`."""
    w = dict(Case(FRONT_WEIGHTS_OF).weights)
    for k, v in O.weights_from_npz(np.load(os.path.join(GOLDEN_DIR, ASSOC_WEIGHTS_OF + ".npz"))).items():
        if k.startswith(ASSOC_PREFIXES):
            assert w[k].shape == v.shape
            w[k] = v
    return w


FRONT_UNUSED = ("DataAggregation.l1_t1_1.", "DataAggregation.l1_t2_1.")     # module.py:85-98 never applies them: their gradient is zero


def owned(prefixes):
    return tuple(sorted(k for k in weights() if k.startswith(prefixes) and not k.startswith(FRONT_UNUSED)))


def leaves(dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in weights().items()}


@contextlib.contextmanager
def recorded():
    """Collects (prefix, z) of every PReLU the oracle applies while the block runs."""
    seen, plain = [], O.act

    def act(x, w, prefix):
        seen.append((prefix, x.detach()))
        return plain(x, w, prefix)
    O.act = act
    try:
        yield seen
    finally:
        O.act = plain


def kink_rows(seen):
    """bool [P]: rows with a pre-activation within MARGIN_KINK x the layer's largest |z| of zero."""
    bad = None
    for _, z in seen:
        k = (z.abs() < MARGIN_KINK * float(z.abs().max())).any(dim=1)
        bad = k if bad is None else bad | k
    return bad


class Probe(object):
    """One cotangent: `cot` fp32, the probed `rows`, the receptive `field` (bool [P]), `field_src` (bool [G]), `gated`."""

    def __init__(self, cot, rows, field, field_src, gated=False, **attrs):
        self.cot, self.rows, self.field, self.field_src, self.gated = cot, rows, field, field_src, gated
        self.__dict__.update(attrs)


class FrontCase(object):
    def hops(self, rows, n=2):
        """bool [P]: `rows` and everything they read through n layers (each layer reads the station- and the source-neighbours)."""
        f = torch.zeros(self.P, dtype=torch.bool)
        f[rows] = True
        for _ in range(n):
            g = f.clone()
            for A in (self.A_in_sta, self.A_in_src):
                g[A[0][f[A[1]]]] = True
            f = g
        return f

    def rows_of(self, g):
        return torch.arange(int(self.seg[g]), int(self.seg[g + 1]))

    def node_field(self, nodes):
        return self.hops(torch.cat([self.rows_of(g) for g in nodes]))

    def row_field(self, rows):
        """The association heads: two hops, then every row of the source nodes met (y_latent[g] feeds every row of g)."""
        src = torch.zeros(self.G, dtype=torch.bool)
        src[self.src_of[self.hops(rows)]] = True
        return src[self.src_of], src


@functools.lru_cache(maxsize=None)
def graphs(name):
    """The case without inputs: shape, base graphs, product edge lists, the segment of every source node."""
    assert name in CASES
    S, G = SHAPES[name]
    c = FrontCase()
    c.name, c.S, c.G, c.kind = name, S, G, name if name in ("ragged", "irregular") else "cartesian"
    c.tables = None
    if name == "irregular":
        fx = Case("subgraph_14x50")
        assert (fx.S, fx.G) == (S, G) and np.array_equal(fx.z["pairs"], np.load(os.path.join(GOLDEN_DIR, "assoc_subgraph_14x50.npz"))["pairs"])
        c.geom = synthetic.Geometry(S, G, L=100e3, n_query=5, seed=14)
        c.A_sta, c.A_src = fx.A_sta_sta, fx.A_src_src
        pairs = torch.from_numpy(fx.z["pairs"]).long()
        c.A_in_sta, c.A_in_src, _ = graph.subgraph_product_edges(c.A_sta, c.A_src, pairs.numpy())
        c.sta_of, c.src_of = pairs[0].contiguous(), pairs[1].contiguous()
    else:
        if name == "ragged":                 # the base graphs of _ragged_graph_21x40 (tests/test_hip_parity.py), thinned further
            rng = np.random.default_rng(7)
            c.geom = geom = synthetic.Geometry(S, G, L=100e3, n_query=5, seed=8)
            keep_sta = rng.random(geom.A_sta_sta.shape[1]) < 0.6                 # (the draws of _ragged_graph_21x40, in its order)
            keep_src = rng.random(geom.A_src_src.shape[1]) < 0.6
            keep_sta &= rng.random(keep_sta.size) < 0.45                         # further: low degrees keep the receptive fields small
            keep_src &= rng.random(keep_src.size) < 0.3
            pl = RAGGED_PLANTS              # no in-edges: nothing points at the node; unlisted: the node is nobody's neighbour
            A_sta, A_src = geom.A_sta_sta, geom.A_src_src
            A_sta = A_sta[:, keep_sta & (A_sta[1] != pl["sta_no_in"]) & (A_sta[0] != pl["sta_unlisted"])]
            A_src = A_src[:, keep_src & (A_src[1] != pl["src_no_in"]) & (A_src[0] != pl["src_unlisted"])]
        else:                                # low degrees keep the receptive fields small
            c.geom = geom = synthetic.Geometry(S, G, L=150e3, n_query=5, seed=100 + S + G, k_sta=3, k_spc=2)
            A_sta, A_src = geom.A_sta_sta, geom.A_src_src
            c.tables = (graph.neighbour_table(A_sta, S), graph.neighbour_table(A_src, G))
        c.A_sta, c.A_src = torch.from_numpy(np.ascontiguousarray(A_sta)).long(), torch.from_numpy(np.ascontiguousarray(A_src)).long()
        c.A_in_sta, c.A_in_src, _, pairs = graph.cartesian_product_edges(c.A_sta, c.A_src, S, G)
        c.sta_of, c.src_of = pairs[0].contiguous(), pairs[1].contiguous()
    c.P = int(c.src_of.numel())
    c.seg = torch.zeros(G + 1, dtype=torch.long)
    c.seg[1:] = torch.cumsum(torch.bincount(c.src_of, minlength=G), 0)
    c.dense = c.P <= DENSE_MAX_P
    return c


def _window(c, seed):
    win = synthetic.make_window(c.geom, 25 * c.S, seed=seed)
    rows = c.src_of * c.S + c.sta_of
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()[rows].contiguous()
    return t(win["Slice"]), t(win["Mask"]), t(c.geom.edge_attr())


def front_forward(c, w, Slice, Mask, edge_attr):
    """(x_latent, r): DataAggregation, then the first lines of `bipartite_read_in` up to the station sum (genie_da_train_fwd's r_out)."""
    if c.tables is not None:
        x_latent = O.data_aggregation_structured(w, Slice, Mask, c.tables[0], c.tables[1], c.S, c.G)
    else:
        x_latent = O.data_aggregation(w, Slice, Mask, c.A_in_sta, c.A_in_src)
    pre = "Bipartite_ReadIn"
    msg = Mask.max(1, keepdim=True)[0] * O.act(O.linear(torch.cat((x_latent, edge_attr), dim=-1), w, pre + ".fc1"), w, pre + ".activate1")
    return x_latent, O.scatter_sum(msg, c.src_of, c.G)


def assoc_forward(c, w, y_latent, mask_src, x_latent, Mask, edge_attr):
    """(s, out): `bipartite_read_out`, then `data_aggregation_association` with x_latent a constant input (module.py:990)."""
    s, m1 = O.bipartite_read_out(w, y_latent, edge_attr, mask_src.view(-1, 1), c.S, src_of=c.src_of)
    return s, O.data_aggregation_association(w, s, x_latent, m1, Mask, c.A_in_sta, c.A_in_src)


@functools.lru_cache(maxsize=None)
def _w64():
    return {k: v.double() for k, v in weights().items()}


def _front_kinks(c, Slice, Mask, edge_attr):
    with torch.no_grad(), recorded() as seen:
        front_forward(c, _w64(), Slice.double(), Mask.double(), edge_attr.double())
    return kink_rows(seen)


def _star_positions(c):
    """Positions inside a source node's segment whose row alone stays unmasked: the last row of the ragged tile, and lane rows 15 / 16."""
    n = int((c.seg[1:] - c.seg[:-1]).max())
    return [("one_station_last", None)] + ([("one_station_15", 15), ("one_station_16", 16)] if n > TR_TILE else [])


@functools.lru_cache(maxsize=None)
def front_case(name):
    """The case with Slice / Mask / edge_attr and its front probes. Search (every forward run counts against REDRAWS): a window seed
    whose fixed probes (g_first, g_last, the planted source nodes of `ragged`) are admissible; then plant by plant the first
    candidate node whose plant keeps every accepted probe admissible. Dense cases: no kink row anywhere instead."""
    c = graphs(name)
    fixed = {"g_first": [0], "g_last": [c.G - 1]}
    plants = [(n, "one", pos) for n, pos in _star_positions(c)] + [("gated", "gated", None)]
    if name == "ragged":
        fixed.update({k: [RAGGED_PLANTS[k]] for k in ("src_no_in", "src_unlisted")})
        plants += [(k, "station", RAGGED_PLANTS[k]) for k in ("sta_no_in", "sta_unlisted")]
    taken = {g for gs in fixed.values() for g in gs}
    fields = {k: c.node_field(gs) for k, gs in fixed.items()}
    tries, done = 0, False
    for seed in range(REDRAWS):
        if tries >= REDRAWS:
            break
        Slice, Mask, ea = _window(c, 1000 * (1 + CASES.index(name)) + seed)
        tries += 1
        accepted, used, where = dict(fields), set(taken), {}
        ok = lambda kink: not kink.any() if c.dense else not any(bool((kink & f).any()) for f in accepted.values())
        if not ok(_front_kinks(c, Slice, Mask, ea)):
            continue
        for pname, kind, arg in plants:
            for g in range(1, c.G - 1):
                n_g = int(c.seg[g + 1] - c.seg[g])
                if g in used or tries >= REDRAWS or (kind == "one" and n_g <= (arg if arg is not None else 0)):
                    continue
                rows = c.rows_of(g)
                star = None if kind == "gated" else int(rows[arg if arg is not None else n_g - 1]) if kind == "one" else int(rows[c.sta_of[rows] == arg][0])
                M2 = Mask.clone()
                M2[rows] = 0.0
                if star is not None:
                    M2[star] = 1.0
                tries += 1
                kink, f = _front_kinks(c, Slice, M2, ea), c.node_field([g])
                if ok(kink) and not (kink & f).any():
                    Mask, accepted[pname], where[pname] = M2, f, (g, star)
                    used.add(g)
                    break
            if pname not in where:
                break
        done = len(where) == len(plants)
        if done:
            break
    assert done, "no admissible set of front probes within %d forward runs" % REDRAWS
    c = _copy(c)
    c.Slice, c.Mask, c.edge_attr, c.front_tries, c.front_where = Slice, Mask, ea, tries, where
    c.front_kink = _front_kinks(c, Slice, Mask, ea)
    gen = torch.Generator().manual_seed(7000 + CASES.index(name))
    probes = {}

    def add(pname, nodes, field, **kw):
        d = torch.zeros((c.G, 30))
        d[nodes] = torch.randn((len(nodes), 30), generator=gen)
        src = torch.zeros(c.G, dtype=torch.bool)
        src[c.src_of[field]] = True
        probes[pname] = Probe(d, torch.cat([c.rows_of(g) for g in nodes]), field, src, nodes=list(nodes), **kw)
    if c.dense:
        add("dense", list(range(c.G)), torch.ones(c.P, dtype=torch.bool))
    for pname, nodes in fixed.items():
        add(pname, nodes, accepted[pname])
    for pname, kind, _ in plants:
        add(pname, [where[pname][0]], accepted[pname], gated=kind == "gated", star=where[pname][1])
    c.front_probes = probes
    return c


def _copy(c):
    d = FrontCase()
    d.__dict__.update(c.__dict__)
    return d


def _assoc_kinks(c, y_latent, mask_src, x_latent):
    with torch.no_grad(), recorded() as seen:
        assoc_forward(c, _w64(), y_latent.double(), mask_src.double(), x_latent.double(), c.Mask.double(), c.edge_attr.double())
    return kink_rows(seen)


@functools.lru_cache(maxsize=None)
def assoc_case(name):
    """The front case's Slice / Mask / edge_attr, x_latent = its float64 DataAggregation rounded to fp32 (a constant input), and
    y_latent ~ N(0, 1), mask_src ~ Bernoulli(0.6) with zeros planted on g = 0, G - 1 and one more node. Search: the y_latent seed
    (and with it the third node) until every probe is admissible; dense cases: no kink row anywhere."""
    c = _copy(front_case(name))
    with torch.no_grad():
        c.x_latent = front_forward(c, _w64(), c.Slice.double(), c.Mask.double(), c.edge_attr.double())[0].float()
    rows = {"row_first": 0, "row_last": c.P - 1}
    if int(c.seg[1]) >= TR_TILE and c.P > TR_TILE:
        rows.update({"row_15": TR_TILE - 1, "row_16": TR_TILE})
    if name == "ragged":
        pl, mid = RAGGED_PLANTS, c.G // 2 + 3
        rows.update({"src_no_in": int(c.seg[pl["src_no_in"]]) + 1, "src_unlisted": int(c.seg[pl["src_unlisted"]]) + 2,
                     "sta_no_in": int(c.seg[mid]) + pl["sta_no_in"], "sta_unlisted": int(c.seg[mid + 1]) + pl["sta_unlisted"]})
    row_fields = {k: c.row_field(torch.tensor([p])) for k, p in rows.items()}
    for t in range(REDRAWS):
        rng = np.random.default_rng(9000 + 1000 * CASES.index(name) + t)
        y_latent = torch.from_numpy(rng.normal(0, 1, (c.G, 30)).astype(np.float32))
        mask_src = torch.from_numpy((rng.random(c.G) < 0.6).astype(np.float32))
        planted = [0, c.G - 1, 1 + (c.G // 2 + t) % (c.G - 2)]
        mask_src[planted] = 0.0
        gated_rows = torch.cat([c.rows_of(g) for g in planted])
        gated_field = (torch.ones(c.P, dtype=torch.bool), torch.ones(c.G, dtype=torch.bool)) if c.dense else c.row_field(gated_rows)
        if not all(bool(mask_src[f[1]].any()) for f in row_fields.values()):       # a probe that meets only gated source nodes says
            continue                                                               # nothing about the read-out's parameters
        kink = _assoc_kinks(c, y_latent, mask_src, c.x_latent)
        if not kink.any() if c.dense else not any(bool((kink & f[0]).any()) for f in list(row_fields.values()) + [gated_field]):
            break
    else:
        raise AssertionError("no admissible set of association probes within %d forward runs" % REDRAWS)
    c.y_latent, c.mask_src, c.assoc_tries, c.assoc_planted, c.assoc_kink = y_latent, mask_src, t + 1, planted, kink
    gen = torch.Generator().manual_seed(8000 + CASES.index(name))
    probes = {}

    def add(pname, prows, field, **kw):
        d = torch.zeros((c.P, 30))
        d[prows] = torch.randn((len(prows), 30), generator=gen)
        probes[pname] = Probe(d, prows, field[0], field[1], **kw)
    everything = (torch.ones(c.P, dtype=torch.bool), torch.ones(c.G, dtype=torch.bool))
    if c.dense:
        add("dense", torch.arange(c.P), everything)
    for pname, p in rows.items():
        add(pname, torch.tensor([p]), row_fields[pname], one_row=True)
    add("gated_src", torch.arange(c.P) if c.dense else gated_rows, gated_field, zero_src=list(planted))
    c.assoc_probes = probes
    return c


def _grads(loss, w, names):
    g = torch.autograd.grad(loss, [w[k] for k in names], retain_graph=True, allow_unused=True)
    return {k: (torch.zeros_like(w[k]) if v is None else v).detach() for k, v in zip(names, g)}


def _front_run(c, dtype):
    w, names = leaves(dtype), owned(FRONT_PREFIXES)
    with recorded() as seen:
        x_latent, r = front_forward(c, w, c.Slice.to(dtype), c.Mask.to(dtype), c.edge_attr.to(dtype))
    probes = {k: {"params": _grads((r * p.cot.to(dtype)).sum(), w, names)} for k, p in c.front_probes.items()}
    return {"out": {"r": r.detach(), "x_latent": x_latent.detach()}, "z": dict(seen), "probes": probes}


@functools.lru_cache(maxsize=None)
def front_reference(name):
    """{"f64": ..., "f32": ...}: each {"out": {r, x_latent}, "z": {PReLU name: pre-activations}, "probes": {probe: {"params": {name: gradient}}}}."""
    c = front_case(name)
    return {"f64": _front_run(c, torch.float64), "f32": _front_run(c, torch.float32)}


def _assoc_run(c, dtype):
    w, names = leaves(dtype), owned(ASSOC_PREFIXES)
    y = c.y_latent.to(dtype).requires_grad_(True)
    with recorded() as seen:
        s, out = assoc_forward(c, w, y, c.mask_src.to(dtype), c.x_latent.to(dtype), c.Mask.to(dtype), c.edge_attr.to(dtype))
    probes = {}
    for k, p in c.assoc_probes.items():
        loss = (out * p.cot.to(dtype)).sum()
        probes[k] = {"params": _grads(loss, w, names), "rows": {"d_y_latent": torch.autograd.grad(loss, y, retain_graph=True)[0].detach()}}
    return {"out": {"s": out.detach()}, "z": dict(seen), "probes": probes}


@functools.lru_cache(maxsize=None)
def assoc_reference(name):
    c = assoc_case(name)
    return {"f64": _assoc_run(c, torch.float64), "f32": _assoc_run(c, torch.float32)}


def front_loss(c, w):
    """float64 scalar of a front probe's cotangent as a function of the weights `w` (for central differences): returns r."""
    return front_forward(c, w, c.Slice.double(), c.Mask.double(), c.edge_attr.double())[1]


def assoc_loss(c, w):
    return assoc_forward(c, w, c.y_latent.double(), c.mask_src.double(), c.x_latent.double(), c.Mask.double(), c.edge_attr.double())[1]


def assoc_slope_cancellation(name, probe, tensor):
    """sum |terms| / |sum of terms| of the PReLU slope gradient `tensor` (state_dict name) of an association probe, float64: the
    slope gradient is the scalar sum over rows and channels of d out x min(z, 0); the activation gets one slope per element here."""
    c, kept, plain, layer = assoc_case(name), {}, O.act, tensor[:-len(".weight")]

    def act(x, w, prefix):
        if prefix != layer:
            return plain(x, w, prefix)
        kept["a"] = w[prefix + ".weight"].expand_as(x).clone().requires_grad_(True)
        return torch.where(x >= 0, x, kept["a"] * x)
    O.act = act
    try:
        out = assoc_loss(c, _w64())
    finally:
        O.act = plain
    terms = torch.autograd.grad((out * c.assoc_probes[probe].cot.double()).sum(), kept["a"])[0]
    return float(terms.abs().sum() / terms.sum().abs())


# Per-tensor factors above train_head_cases.FACTOR (4) for the P-sized backward, by name: twice the largest ratio e_hip / e_cpu measured
# over every probe of every case (profiles/EXPERIMENTS.md, "P-sized training backward against float64"). All are PReLU slope
# gradients of the association heads, each ONE number: the sum over rows and channels of d out x min(z, 0), whose terms cancel (the sum
# is about 100 to 2200 times smaller than its terms on the probes that set the factors: `assoc_slope_cancellation`, pinned by
# tests/test_train_front_cpu.py). k_as_b3 / k_train_b1<true> / k_as_b1 / k_as_b0 add a lane's terms tile after tile, then the lanes,
# then k_train_reduce the waves' partials in slot order; autograd sums row by row: two orders of a cancelling sum. The device's error
# is at most 1.2 fp32 round-offs (2^-24) of the summed magnitudes on every one of them, with the fp32 stage kernels and with the
# default ones bit for bit alike. And the yardstick of a scalar is ONE draw of the CPU's rounding error, which can come out small by
# chance (e_cpu 0.02 to 0.2 round-offs of the summed magnitudes on the probes below), where a tensor's e_cpu is the largest of many.
FACTORS = {
    "BipartiteGraphReadOutOperator.activate2.weight": 14.5,             # 7.25  (s3 row_last; cancellation 102)
    "DataAggregationAssociationPhase.activate1.weight": 14.7,           # 7.33  (s17 row_15)
    "DataAggregationAssociationPhase.activate12.weight": 23.8,          # 11.89 (ragged sta_no_in; cancellation 836; s17 dense 4.18: 2181)
    "DataAggregationAssociationPhase.activate21.weight": 12.7,          # 6.34  (s3 gated_src)
    "DataAggregationAssociationPhase.activate22.weight": 8.8,           # 4.37  (ragged sta_no_in; cancellation 306)
}
