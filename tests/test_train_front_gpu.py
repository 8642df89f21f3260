"""GPU: the P-sized training backward against float64 with localised cotangents, tensor by tensor and row by row.

`engine.train_bwd` (k_train_b2, k_train_b1s / k_train_b1p, k_train_b0, k_train_reduce) and `engine.assoc_train_bwd` (k_as_b3,
k_train_b1<true>, k_as_b1, k_as_b0, k_as_g) on the cases of tests/train_front_cases.py (tests/test_train_front_cpu.py pins the cases
and the references): partial, full and one-row tiles of 16 product rows, ragged graphs with empty neighbourhoods and empty reversed
neighbourhoods, more tiles than waves, an irregular product graph. Nearly all these passes return are weight gradients, sums over
every product row, which the whole-model tests compare with an fp32 oracle at 2e-4; a cotangent on one source node or one product
row makes a handful of rows the whole answer, and here

* every parameter gradient the call owns and every row of `d y_latent` is compared with the float64 autograd of the oracle: error
  e = max |got - ref64| / scale, bound e_hip <= 4 max(e_cpu, 2^-20) with e_cpu the same error of the fp32 CPU autograd for the same
  probe (`row_error`, `param_error`, `bound` of tests/train_head_cases.py). Measured figures: profiles/EXPERIMENTS.md, "P-sized
  training backward against float64";
* what must be exactly zero is: gradients of parameters the call does not own, the whole blob of a gated probe, rows of `d y_latent`
  outside the receptive field or of a gated source node;
* the backward is linear in its cotangent bit for bit under a scaling by 2, repeatable bit for bit, and additive over two probes with
  disjoint receptive fields within the bound;
* the front agrees between the fp32 stage kernels and the default training forward.

Five PReLU slope gradients of the association heads have a factor of their own (`train_front_cases.FACTORS`, twice the largest
measured ratio: 7.25, 7.33, 11.89, 6.34, 4.37): each is one number left over by a sum whose terms are about 100 to 2200 times larger,
summed by the kernels in another order than autograd's; the device's error is at most 1.2 fp32 round-offs of the summed magnitudes.

Out of scope: the 64-bit-offset forms of the passes (`tr_o32` false, P >= 4.79 M: no small shape reaches them); the non-split
k_train_b1<false> (the default build does not launch it on Cartesian graphs); the static-term model definitions (`edges`, `abspos`;
k_gr_sum_*, k_static_dw: they have their own 33 x 257 test); the G-sized tail backward
(test_tail_backward_is_deterministic_and_matches_the_oracle)."""
import functools

import pytest
import torch

from genie_amd import engine
from tests import train_front_cases as C
from tests import train_head_cases as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRONT, ASSOC = C.owned(C.FRONT_PREFIXES), C.owned(C.ASSOC_PREFIXES)


def bound(name, e_cpu):
    return C.FACTORS[name] * max(e_cpu, H.FLOOR) if name in C.FACTORS else H.bound(name, e_cpu)


@functools.lru_cache(maxsize=None)
def _hp(name, precision=None):
    """One context per case (and stage precision), with the weights of the cases."""
    c = C.graphs(name)
    src_csr = engine.csr_from_edges(c.A_src, c.G)
    if c.kind == "irregular":
        sub = {"n_prod": c.P, "sta_csr": engine.csr_from_edges(c.A_in_sta, c.P), "src_csr": engine.csr_from_edges(c.A_in_src, c.P),
               "seg_rowptr": c.seg.to(torch.int32)}
        hp = engine.HipPath(c.S, c.G, None, src_csr, device=DEV, subgraph=sub, stage_precision=precision)
    else:
        hp = engine.HipPath(c.S, c.G, engine.csr_from_edges(c.A_sta, c.S), src_csr, device=DEV, stage_precision=precision)
    hp.set_weights({k: v.to(DEV) for k, v in C.weights().items()})
    return hp


@functools.lru_cache(maxsize=None)
def _front_fwd(name, precision=None):
    c = C.front_case(name)
    args = tuple(t.to(DEV) for t in (c.Slice, c.Mask, c.edge_attr))
    r, x_latent, save = _hp(name, precision).train_fwd(*args)
    torch.cuda.synchronize()
    return args, r, x_latent, save


def _front_bwd(name, d_r, precision=None):
    args, _, _, save = _front_fwd(name, precision)
    g = _hp(name, precision).train_bwd(*args, save, d_r.to(DEV))
    torch.cuda.synchronize()
    return g


@functools.lru_cache(maxsize=None)
def _assoc_fwd(name):
    c = C.assoc_case(name)
    args = tuple(t.to(DEV) for t in (c.y_latent, c.mask_src, c.x_latent, c.Mask, c.edge_attr))
    s, asave = _hp(name).assoc_train_fwd(*args)
    torch.cuda.synchronize()
    return args, s, asave


def _assoc_bwd(name, d_s):
    args, _, asave = _assoc_fwd(name)
    d_y, g = _hp(name).assoc_train_bwd(*args, asave, d_s.to(DEV))
    torch.cuda.synchronize()
    return d_y, g


@functools.lru_cache(maxsize=None)
def _got(head, name, probe):
    if head == "front":
        return None, _front_bwd(name, C.front_case(name).front_probes[probe].cot)
    return _assoc_bwd(name, C.assoc_case(name).assoc_probes[probe].cot)


def _blob(g):
    return next(iter(g.values()))._base


def _bits(t):
    return t.contiguous().view(torch.int32)


def _close(names, g, h, r64, r32, what):
    """Two device results agree within the bound of the tensor, at the scale of its float64 reference."""
    for k in names:
        scale, diff = float(r64[k].abs().max()), float((g[k].double() - h[k].double()).abs().max())
        e_cpu = H.param_error(r32[k], r64[k])
        assert diff == 0.0 if scale == 0.0 else diff / scale <= bound(k, e_cpu), (what, k, diff, scale, e_cpu)


def _compare(head, name, probe, ref, got_params, got_rows, over=None):
    """Print the worst tensor of the probe (e_hip, e_cpu, ratio) and every tensor above half the common factor, then fail on every
    tensor over its bound, naming the probe and the worst entry or row (a row of d y_latent is a source node: its first product row,
    tile and lane row are named). `over`: a list that takes the failures instead, for a caller that goes through all its probes."""
    r64, r32 = ref["f64"]["probes"][probe], ref["f32"]["probes"][probe]
    fail, worst = [], (-1.0, None)
    for kname in sorted(got_params):
        e_hip = H.param_error(got_params[kname], r64["params"][kname])
        e_cpu = H.param_error(r32["params"][kname], r64["params"][kname])
        ratio = e_hip / max(e_cpu, H.FLOOR)
        worst = max(worst, (ratio, "%-46s e_hip %.3e e_cpu %.3e ratio %.2f" % (kname, e_hip, e_cpu, ratio)))
        if ratio > H.FACTOR / 2:
            print("train_front %-5s %-9s %-17s above 2 %-46s e_hip %.3e e_cpu %.3e ratio %.2f" % (head, name, probe, kname, e_hip, e_cpu, ratio))
        if not e_hip <= bound(kname, e_cpu):
            d = (got_params[kname].detach().cpu().double().reshape(r64["params"][kname].shape) - r64["params"][kname]).abs()
            fail.append("%s: e_hip %.3e > %g x max(e_cpu %.3e, 2^-20), worst entry %s" % (kname, e_hip, bound(kname, 1.0), e_cpu,
                                                                                        tuple(int(i) for i in (d == d.max()).nonzero()[0])))
    for kname in sorted(got_rows):
        (e_hip, row), (e_cpu, _) = H.row_error(got_rows[kname], r64["rows"][kname]), H.row_error(r32["rows"][kname], r64["rows"][kname])
        ratio = e_hip / max(e_cpu, H.FLOOR)
        worst = max(worst, (ratio, "%-46s e_hip %.3e e_cpu %.3e ratio %.2f" % (kname, e_hip, e_cpu, ratio)))
        if not e_hip <= bound(kname, e_cpu):
            p0 = int(C.graphs(name).seg[row])
            fail.append("%s: e_hip %.3e > %g x max(e_cpu %.3e, 2^-20), worst row %d (source node; product rows from %d: tile %d, lane row %d)"
                        % (kname, e_hip, bound(kname, 1.0), e_cpu, row, p0, p0 // 16, p0 % 16))
    print("train_front %-5s %-9s %-17s worst %s" % (head, name, probe, worst[1]))
    if over is not None:
        over.extend("%s %s probe %s: %s" % (head, name, probe, f) for f in fail)
    else:
        assert not fail, "%s %s probe %s\n%s" % (head, name, probe, "\n".join(fail))


@pytest.mark.parametrize("name", C.CASES)
def test_training_forwards_match_float64(name):
    """r and x_latent of genie_da_train_fwd, s of genie_assoc_train_fwd: 1e-5 x max(1, max |ref|), as the stand-alone forward tests."""
    fr, ar = C.front_reference(name)["f64"]["out"], C.assoc_reference(name)["f64"]["out"]
    _, r, x_latent, _ = _front_fwd(name)
    _, s, _ = _assoc_fwd(name)
    for what, got, ref in (("r", r, fr["r"]), ("x_latent", x_latent, fr["x_latent"]), ("s", s, ar["s"])):
        err, scale = float((got.cpu().double() - ref).abs().max()), max(1.0, float(ref.abs().max()))
        print("train_front forward %-9s %-8s max error %.3e, max |ref| %.3e" % (name, what, err, float(ref.abs().max())))
        assert got.shape == ref.shape and err <= 1e-5 * scale, (what, err, scale)


@pytest.mark.parametrize("name", C.CASES)
def test_front_backward_matches_float64_probe_by_probe(name):
    c, ref, over = C.front_case(name), C.front_reference(name), []
    for probe, p in c.front_probes.items():
        g = _got("front", name, probe)[1]
        assert torch.isfinite(_blob(g)).all()
        for k, v in g.items():
            if k not in FRONT:
                assert not v.any(), (probe, k)
        if p.gated:
            assert not _blob(g).any(), "a cotangent on a source node whose Mask rows are all zero reaches a gradient (%s)" % probe
        _compare("front", name, probe, ref, {k: g[k] for k in FRONT}, {}, over)
    assert not over, "\n".join(over)


@pytest.mark.parametrize("name", C.CASES)
def test_assoc_backward_matches_float64_probe_by_probe(name):
    c, ref, over = C.assoc_case(name), C.assoc_reference(name), []
    for probe, p in c.assoc_probes.items():
        d_y, g = _got("assoc", name, probe)
        assert d_y.shape == (c.G, 30) and torch.isfinite(d_y).all() and torch.isfinite(_blob(g)).all()
        for k, v in g.items():
            if k not in ASSOC:
                assert not v.any(), (probe, k)
        assert not d_y[~p.field_src.to(DEV)].any(), "a row of d y_latent outside the receptive field is not zero (%s)" % probe
        assert not d_y[~c.mask_src.bool().to(DEV)].any(), "a gated source node has a gradient (%s)" % probe
        if probe == "gated_src":
            assert not d_y[p.zero_src].any()
        _compare("assoc", name, probe, ref, {k: g[k] for k in ASSOC}, {"d_y_latent": d_y}, over)
    assert not over, "\n".join(over)


@pytest.mark.parametrize("name", C.CASES)
def test_backward_is_linear_and_repeatable_bit_for_bit(name):
    """Every call repeats bit for bit, and the blob of 2 d is twice the blob of d bit for bit (a power of two commutes with every rounding)."""
    fc, ac = C.front_case(name), C.assoc_case(name)
    for probe, p in fc.front_probes.items():
        b = _blob(_got("front", name, probe)[1])
        assert torch.equal(_bits(b), _bits(_blob(_front_bwd(name, p.cot)))), probe
        assert torch.equal(_bits(2.0 * b), _bits(_blob(_front_bwd(name, 2.0 * p.cot)))), probe
    for probe, p in ac.assoc_probes.items():
        d_y, g = _got("assoc", name, probe)
        d_y1, g1 = _assoc_bwd(name, p.cot)
        assert torch.equal(_bits(d_y), _bits(d_y1)) and torch.equal(_bits(_blob(g)), _bits(_blob(g1))), probe
        d_y2, g2 = _assoc_bwd(name, 2.0 * p.cot)
        assert torch.equal(_bits(2.0 * d_y), _bits(d_y2)) and torch.equal(_bits(2.0 * _blob(g)), _bits(_blob(g2))), probe


def _sum_of_references(ref, a, b):
    """The reference of the cotangent d_a + d_b: the sum of the two references, in either precision."""
    out = {}
    for key in ("f64", "f32"):
        pa, pb = ref[key]["probes"][a], ref[key]["probes"][b]
        out[key] = {"probes": {"sum": {kind: {k: pa[kind][k] + pb[kind][k] for k in pa[kind]} for kind in pa}}}
    return out


def test_two_probes_with_disjoint_receptive_fields_add_up():
    """`long`: the first and the last source node (product row) are far apart. The blob of d_a + d_b is compared with the float64 sum
    of the two references, and with the sum of the two blobs, both within the bound (not bitwise: the partial sums of a wave differ)."""
    fc, ac = C.front_case("long"), C.assoc_case("long")
    a, b = fc.front_probes["g_first"], fc.front_probes["g_last"]
    assert not (a.field & b.field).any()
    ref = _sum_of_references(C.front_reference("long"), "g_first", "g_last")
    g = _front_bwd("long", a.cot + b.cot)
    ga, gb = _got("front", "long", "g_first")[1], _got("front", "long", "g_last")[1]
    _compare("front", "long", "sum", ref, {k: g[k] for k in FRONT}, {})
    _close(FRONT, g, {k: ga[k] + gb[k] for k in FRONT}, ref["f64"]["probes"]["sum"]["params"], ref["f32"]["probes"]["sum"]["params"], "front")
    a, b = ac.assoc_probes["row_first"], ac.assoc_probes["row_last"]
    assert not (a.field & b.field).any()
    ref = _sum_of_references(C.assoc_reference("long"), "row_first", "row_last")
    d_y, g = _assoc_bwd("long", a.cot + b.cot)
    (ya, ga), (yb, gb) = _got("assoc", "long", "row_first"), _got("assoc", "long", "row_last")
    _compare("assoc", "long", "sum", ref, {k: g[k] for k in ASSOC}, {"d_y_latent": d_y})
    _close(ASSOC, g, {k: ga[k] + gb[k] for k in ASSOC}, ref["f64"]["probes"]["sum"]["params"], ref["f32"]["probes"]["sum"]["params"], "assoc")
    assert torch.equal(d_y, ya + yb)                  # the two probes touch different rows of d y_latent


@pytest.mark.parametrize("name", ["s17", "ragged"])
def test_front_agrees_between_the_two_training_forwards(name):
    """The fp32 stage kernels and the default training forward (f16x2 on `s17`; on `ragged` the fp32 kernels anyway) save
    pre-activations that agree on every sign inside the receptive fields (the admissibility margin), so both backward runs meet the
    float64 reference within the bound, and each other within the bound."""
    c, ref = C.front_case(name), C.front_reference(name)
    _, r32, x32, _ = _front_fwd(name, "f32")
    out = ref["f64"]["out"]
    assert float((r32.cpu().double() - out["r"]).abs().max()) <= 1e-5 * max(1.0, float(out["r"].abs().max()))
    assert float((x32.cpu().double() - out["x_latent"]).abs().max()) <= 1e-5 * max(1.0, float(out["x_latent"].abs().max()))
    for probe, p in c.front_probes.items():
        g32, g = _front_bwd(name, p.cot, "f32"), _got("front", name, probe)[1]
        if p.gated:
            assert not _blob(g32).any()
        _compare("f32", name, probe, ref, {k: g32[k] for k in FRONT}, {})
        _close(FRONT, g32, g, ref["f64"]["probes"][probe]["params"], ref["f32"]["probes"][probe]["params"], probe)
