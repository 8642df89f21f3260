"""CPU: the cases and references of tests/train_front_cases.py are what they claim to be, before any kernel is compared with them
(tests/test_train_front_gpu.py).

For every case: it builds, every named probe was found admissible within the redraw cap (no kink row in its receptive field; dense
cases have no kink row at all), and the fp32 and float64 CPU runs agree on the sign of every pre-activation there, with
|z32 - z64| <= MARGIN_KINK / 4 of the layer's scale. The planted properties hold (degrees 0 where promised, the Mask and mask_src
plants, more tiles than waves in `long`). The references themselves: central differences of the float64 scalar along a seeded
parameter direction agree with the autograd gradient; gated probes and `d_y_latent` rows outside the receptive field are exactly
zero; no probe is vacuous."""
import numpy as np
import pytest
import torch

from tests import train_front_cases as C
from tests import train_head_cases as H


def _probes(name, head):
    c = C.front_case(name) if head == "front" else C.assoc_case(name)
    return c, (c.front_probes if head == "front" else c.assoc_probes), (C.front_reference if head == "front" else C.assoc_reference)(name)


def test_shapes_sit_on_the_kernels_tile_edges():
    n = {name: C.graphs(name) for name in C.CASES}
    assert all((n[k].S, n[k].G) == C.SHAPES[k] for k in C.CASES)
    assert n["s3"].S < C.TR_TILE and n["s16"].S == C.TR_TILE and n["s17"].S == C.TR_TILE + 1 and n["s33"].S == 2 * C.TR_TILE + 1
    assert n["s17"].G % 2 == 1 and n["ragged"].S % C.TR_TILE not in (0, 1)
    tiles = n["long"].G * -(-n["long"].S // C.TR_TILE)
    # every wave of k_train_b2<false, 8> (8 waves per workgroup) and of the four-wave passes walks more than one tile
    assert tiles == 4500 and tiles > C.TR_GRID * C.TR_WAVES_LIGHT > C.TR_GRID * C.TR_WAVES == 2048
    assert n["long"].P == 13500 and not n["long"].dense
    irr = n["irregular"]
    assert irr.P == 338 < irr.S * irr.G and irr.tables is None and int((irr.seg[1:] - irr.seg[:-1]).min()) >= 1
    assert [k for k in C.CASES if n[k].dense] == ["s3", "s16", "s17", "irregular"]
    for k in ("s3", "s16", "s17", "s33", "long"):                                  # Cartesian numbering p = g S + s
        assert torch.equal(n[k].src_of * n[k].S + n[k].sta_of, torch.arange(n[k].P))


def test_ragged_graphs_hold_the_four_empty_neighbourhoods():
    c, pl = C.graphs("ragged"), C.RAGGED_PLANTS
    in_sta, out_sta = torch.bincount(c.A_sta[1], minlength=c.S), torch.bincount(c.A_sta[0], minlength=c.S)
    in_src, out_src = torch.bincount(c.A_src[1], minlength=c.G), torch.bincount(c.A_src[0], minlength=c.G)
    assert in_sta[pl["sta_no_in"]] == 0 and out_sta[pl["sta_no_in"]] > 0
    assert in_src[pl["src_no_in"]] == 0 and out_src[pl["src_no_in"]] > 0
    assert out_sta[pl["sta_unlisted"]] == 0 and in_sta[pl["sta_unlisted"]] > 0         # its transposed mean is empty
    assert out_src[pl["src_unlisted"]] == 0 and in_src[pl["src_unlisted"]] > 0
    assert len(set(in_sta.tolist())) >= 3 and len(set(in_src.tolist())) >= 3 and int(in_sta.max()) >= 2 and int(in_src.max()) >= 2


@pytest.mark.parametrize("name", C.CASES)
def test_front_probes_are_admissible_and_planted(name):
    c, probes, ref = _probes(name, "front")
    assert c.front_tries <= C.REDRAWS and c.Slice.dtype == torch.float32 and c.Mask.shape == (c.P, 4)
    want = {"g_first", "g_last", "one_station_last", "gated"} | ({"dense"} if c.dense else set())
    if int((c.seg[1:] - c.seg[:-1]).max()) > C.TR_TILE:
        want |= {"one_station_15", "one_station_16"}
    if name == "ragged":
        want |= set(C.RAGGED_PLANTS)
    assert set(probes) == want
    assert not c.front_kink.any() if c.dense else all(not (c.front_kink & p.field).any() for p in probes.values())
    gate = c.Mask.max(1)[0]
    for k, p in probes.items():
        assert set(torch.nonzero(p.cot.abs().amax(1)).view(-1).tolist()) == set(p.nodes)
        assert p.field[p.rows].all() and torch.equal(p.field, c.hops(p.rows)) or k == "dense"
        if k.startswith("one_station") or k.startswith("sta_"):                     # one unmasked row on the probed node
            (g,), rows = p.nodes, c.rows_of(p.nodes[0])
            assert gate[rows].sum() == 1 and gate[p.star] == 1 and int(c.src_of[p.star]) == g
            pos = int(p.star) - int(rows[0])
            assert pos == {"one_station_last": len(rows) - 1, "one_station_15": 15, "one_station_16": 16}.get(k, pos)
            if k.startswith("sta_"):
                assert int(c.sta_of[p.star]) == C.RAGGED_PLANTS[k]
        if p.gated:
            assert k == "gated" and not gate[p.rows].any() and 0 < p.nodes[0] < c.G - 1
    assert probes["g_first"].nodes == [0] and probes["g_last"].nodes == [c.G - 1]
    assert gate[c.rows_of(0)].any() and gate[c.rows_of(c.G - 1)].any()
    if name == "ragged":
        assert probes["src_no_in"].nodes == [5] and probes["src_unlisted"].nodes == [11]
        assert int(probes["src_no_in"].field.sum()) == c.S                           # nothing to read beyond its own rows' station hops


@pytest.mark.parametrize("name", C.CASES)
def test_assoc_probes_are_admissible_and_planted(name):
    c, probes, ref = _probes(name, "assoc")
    assert c.assoc_tries <= C.REDRAWS
    want = {"row_first", "row_last", "gated_src"} | ({"dense"} if c.dense else set())
    if name in ("s16", "s17", "s33", "ragged"):
        want |= {"row_15", "row_16"}
    if name == "ragged":
        want |= set(C.RAGGED_PLANTS)
    assert set(probes) == want
    assert not c.assoc_kink.any() if c.dense else all(not (c.assoc_kink & p.field).any() for p in probes.values())
    assert c.assoc_planted[:2] == [0, c.G - 1] and len(set(c.assoc_planted)) == 3 and not c.mask_src[c.assoc_planted].any()
    assert set(c.mask_src.tolist()) == {0.0, 1.0} and 0.3 < float(c.mask_src.mean()) < 0.8
    assert probes["gated_src"].zero_src == c.assoc_planted and probes["gated_src"].field[probes["gated_src"].rows].all()
    assert int(probes["row_first"].rows) == 0 and int(probes["row_last"].rows) == c.P - 1
    for k, p in probes.items():
        if getattr(p, "one_row", False):
            assert int(p.cot.abs().amax(1).bool().sum()) == 1 and p.field[p.rows].all() and p.field_src[c.src_of[p.rows]].all()
            assert torch.equal(p.field, p.field_src[c.src_of]) and (c.hops(p.rows) <= p.field).all()
    if "row_15" in probes:
        assert int(probes["row_15"].rows) == C.TR_TILE - 1 and int(probes["row_16"].rows) == C.TR_TILE
    if name == "ragged":
        pl = C.RAGGED_PLANTS
        assert int(c.src_of[probes["src_no_in"].rows]) == pl["src_no_in"] and int(c.src_of[probes["src_unlisted"].rows]) == pl["src_unlisted"]
        assert int(c.sta_of[probes["sta_no_in"].rows]) == pl["sta_no_in"] and int(c.sta_of[probes["sta_unlisted"].rows]) == pl["sta_unlisted"]


@pytest.mark.parametrize("head", ["front", "assoc"])
@pytest.mark.parametrize("name", C.CASES)
def test_fp32_and_float64_agree_on_every_sign_in_the_receptive_fields(name, head):
    c, probes, ref = _probes(name, head)
    field = torch.zeros(c.P, dtype=torch.bool)
    for p in probes.values():
        field |= p.field
    z64, z32 = ref["f64"]["z"], ref["f32"]["z"]
    assert set(z64) == set(z32) and len(z64) >= 8
    for k in sorted(z64):
        a, b = z64[k][field], z32[k][field].double()
        scale = float(z64[k].abs().max())
        assert float(a.abs().min()) >= C.MARGIN_KINK * scale, k
        assert torch.equal(torch.sign(a), torch.sign(b)), k
        assert float((a - b).abs().max()) <= C.MARGIN_KINK / 4 * scale, (k, float((a - b).abs().max()) / scale)


@pytest.mark.parametrize("head", ["front", "assoc"])
@pytest.mark.parametrize("name", C.CASES)
def test_references_are_zero_where_they_must_be_and_nowhere_vacuous(name, head):
    c, probes, ref = _probes(name, head)
    names = C.owned(C.FRONT_PREFIXES if head == "front" else C.ASSOC_PREFIXES)
    assert len(names) >= 20
    for k, p in probes.items():
        for key in ("f64", "f32"):
            g = ref[key]["probes"][k]["params"]
            assert set(g) == set(names)
            if p.gated:
                assert all(not v.any() for v in g.values()), (k, key)
            else:
                zero = {n for n in names if n.split(".", 1)[1] in C.NO_MEAN.get(k, ())}
                assert {n for n, v in g.items() if not v.any()} == zero and all(bool(torch.isfinite(v).all()) for v in g.values()), (k, key)
            if head == "assoc":
                dy = ref[key]["probes"][k]["rows"]["d_y_latent"]
                assert not dy[~p.field_src].any() and dy.any(), (k, key)
                if k == "gated_src":
                    assert not dy[p.zero_src].any() and (dy[c.mask_src.bool()].abs().amax(1).bool().all() or not c.dense)
    if head == "assoc":                      # a one-row cotangent: the last layers' gradients are one row's outer product
        for k, p in probes.items():
            if getattr(p, "one_row", False):
                for n in ("l2_t1_2", "l2_t2_2"):
                    g = ref["f64"]["probes"][k]["params"]["DataAggregationAssociationPhase.%s.weight" % n]
                    sv = torch.linalg.svdvals(g)
                    assert float(sv[1]) <= 1e-12 * float(sv[0]), (k, n)
    else:                                    # one unmasked row: Bipartite_ReadIn.fc1's gradient is that row's outer product
        for k, p in probes.items():
            if k.startswith("one_station") or k.startswith("sta_"):
                g = ref["f64"]["probes"][k]["params"]
                x = torch.cat((ref["f64"]["out"]["x_latent"][p.star], c.edge_attr[p.star].double()))
                outer = torch.outer(g["Bipartite_ReadIn.fc1.bias"], x)
                assert float((g["Bipartite_ReadIn.fc1.weight"] - outer).abs().max()) <= 1e-12 * float(outer.abs().max()), k


@pytest.mark.parametrize("head,name,probe", [("front", "s17", "one_station_16"), ("front", "ragged", "src_unlisted"),
                                             ("assoc", "s17", "row_16"), ("assoc", "ragged", "sta_no_in")])
def test_float64_references_agree_with_central_differences(head, name, probe):
    """Central differences (h = 1e-5) of the float64 scalar along a seeded direction over the parameters the call owns, against the
    autograd gradient's component along it: 1e-6 of the gradient's largest entry, as tests/test_train_heads_cpu.py asks."""
    c, probes, ref = _probes(name, head)
    names = C.owned(C.FRONT_PREFIXES if head == "front" else C.ASSOC_PREFIXES)
    g = ref["f64"]["probes"][probe]["params"]
    w = {k: v.double() for k, v in C.weights().items()}
    gen = torch.Generator().manual_seed(99)
    direction = {k: torch.randn(w[k].shape, generator=gen, dtype=torch.float64) for k in names}
    direction = {k: v / np.sqrt(sum(d.numel() for d in direction.values())) for k, v in direction.items()}
    cot = probes[probe].cot.double()

    def value(h):
        moved = dict(w)
        moved.update({k: w[k] + h * direction[k] for k in names})
        with torch.no_grad():
            return float(((C.front_loss if head == "front" else C.assoc_loss)(c, moved) * cot).sum())
    fd = (value(1e-5) - value(-1e-5)) / 2e-5
    along = float(sum((g[k] * direction[k]).sum() for k in names))
    gmax = max(float(v.abs().max()) for v in g.values())
    assert abs(fd - along) <= 1e-6 * gmax, (fd, along, gmax)
    assert abs(along) > 1e-3 * gmax


def test_references_are_built_once_and_share_the_heads_bound():
    assert C.front_reference("s3") is C.front_reference("s3") and C.assoc_reference("s3") is C.assoc_reference("s3")
    assert H.FACTOR == 4.0 and H.FLOOR == 2.0 ** -20 and not set(C.FACTORS) & set(H.FACTORS)


def test_the_wider_factors_belong_to_scalar_sums_of_cancelling_terms():
    """Every entry of FACTORS is a PReLU slope gradient of the association heads (one number per tensor), and on the probes that set
    the factors the sum is far smaller than its terms."""
    assert all(k in C.owned(C.ASSOC_PREFIXES) and C.weights()[k].numel() == 1 and ".activate" in k for k in C.FACTORS)
    assert all(4.0 < f < 24.0 for f in C.FACTORS.values())
    worst = {("s3", "row_last", "BipartiteGraphReadOutOperator.activate2.weight"): 100.0,
             ("s17", "row_15", "DataAggregationAssociationPhase.activate1.weight"): 20.0,
             ("ragged", "sta_no_in", "DataAggregationAssociationPhase.activate12.weight"): 800.0,
             ("s17", "dense", "DataAggregationAssociationPhase.activate12.weight"): 2000.0,
             ("s3", "gated_src", "DataAggregationAssociationPhase.activate21.weight"): 20.0,
             ("ragged", "sta_no_in", "DataAggregationAssociationPhase.activate22.weight"): 300.0}
    assert {k[2] for k in worst} == set(C.FACTORS)
    for (name, probe, tensor), least in worst.items():
        ratio = C.assoc_slope_cancellation(name, probe, tensor)
        print("train_front cancellation %-7s %-10s %-50s %.1f" % (name, probe, tensor, ratio))
        assert ratio >= least, (name, probe, tensor, ratio)
