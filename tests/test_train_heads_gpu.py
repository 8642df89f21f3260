"""GPU: the backward of the two pick-sized training heads against float64, tensor by tensor and row by row.

`engine.lslc_bwd` (k_lslc_bwd + k_seg_rows, both heads in one call) and `engine.arrivals_fwd(train=True)` + `engine.arrivals_bwd`
(k_arrt_tgt_bwd, k_arrt_ent_bwd, k_arrt_ctx_bwd, k_arrt_ctx_red, k_arrt_pick_sum) on the cases of tests/train_head_cases.py: shapes on
the kernels' tile, round, chunk and grid-stride boundaries, picks that share a time bin, picks without any edge, zero rows in the
cotangents (tests/test_train_heads_cpu.py pins the cases and the references). The whole-model training tests see these kernels' row
outputs only after the P-sized backward has mixed them into weight gradients, against an fp32 oracle at 2e-4; here

* every parameter gradient and every row of `d s`, `d src_embed`, `d arrival_p`, `d arrival_s` is compared with the float64 autograd
  of the restatement: error e = max |got - ref64| / scale (parameters: the tensor's largest entry; rows: the row's largest entry,
  at least 1e-3 of the tensor's), bound e_hip <= 4 max(e_cpu, 2^-20) with e_cpu the same error of the fp32 CPU autograd, computed
  for the same case (the factor: another summation order over the same terms; the floor: 16 fp32 round-offs at the tensor's scale).
  Measured figures: profiles/EXPERIMENTS.md, "Pick-sized training heads against float64";
* rows and entries that must be exactly zero are (bitwise +0.0 for the untouched rows of `d s`);
* the backward is linear in its cotangent bit for bit under a scaling by 2, local in the source, and repeatable bit for bit;
* calls with a wrong cotangent or without picks are refused before anything is launched."""
import functools

import pytest
import torch

from genie_amd import engine, module
from tests import train_head_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _net():
    """One model on the 7 x 45 product graph of the LSLC cases (the arrival head takes its station count from `trv_src`)."""
    geom = C.lslc_graph(False)[0]
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV)
    net.load_state_dict({k: v.clone() for k, v in C.weights().items()}, strict=True)
    net.eval()
    net.set_adjacencies_base(torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src), torch.from_numpy(geom.edge_attr()).to(DEV),
                             torch.from_numpy(geom.locs).float().to(DEV), torch.from_numpy(geom.x_grid).float().to(DEV))
    net._hip.sync_weights(net._path_params)
    return net


def _hp():
    return _net()._hip


def _report(head, case, ref, got_rows, got_params):
    """Print e_hip, e_cpu and their ratio for every tensor, then fail on those over their bound, naming the row."""
    over = []
    for kind, got in (("rows", got_rows), ("params", got_params)):
        for name in sorted(got):
            r64, r32 = ref["f64"][kind][name], ref["f32"][kind][name]
            if kind == "rows":
                (e_hip, row), (e_cpu, _) = C.row_error(got[name], r64), C.row_error(r32, r64)
            else:
                e_hip, row, e_cpu = C.param_error(got[name], r64), None, C.param_error(r32, r64)
            print("train_heads %s %-13s %-42s e_hip %.3e e_cpu %.3e ratio %.2f" % (head, case, name, e_hip, e_cpu, e_hip / max(e_cpu, C.FLOOR)))
            if not e_hip <= C.bound(name, e_cpu):
                where = "" if row is None else " worst row %d (tile %d, lane row %d)" % (row, row // 16, row % 16)
                over.append("%s: e_hip %.3e > %g x max(e_cpu %.3e, 2^-20)%s" % (name, e_hip, C.FACTORS.get(name, C.FACTOR), e_cpu, where))
    assert not over, "\n".join(over)


def _others_zero(g, names):
    """Every entry of the gradient dict that belongs to another module is exactly zero."""
    for k, v in g.items():
        if k not in names:
            assert not v.any(), k


def _same_bits(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


# ---- LocalSliceLgCollapse P / S ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lslc_inputs(name):
    c = C.lslc_case(name)
    d = lambda t: t.to(DEV)
    return (d(c.s), (d(c.tables[0].to(torch.int32)), d(c.tables[1].to(torch.int32))), d(c.dtp), d(c.tpick), d(c.ipick.to(torch.int32)),
            d(c.phase), d(c.tlatent), C.EPS)


def _lslc_call(name, scale=1.0):
    c = C.lslc_case(name)
    cot = [None if k is None else (k * scale).to(DEV) for k in c.coef]
    ds, g = _hp().lslc_bwd(*_lslc_inputs(name), cot[0], cot[1])
    torch.cuda.synchronize()
    return ds, g


@functools.lru_cache(maxsize=None)
def _lslc_got(name):
    return _lslc_call(name)


@pytest.mark.parametrize("name", C.LSLC_CASES)
def test_lslc_backward_matches_float64(name):
    c, ref = C.lslc_case(name), C.lslc_reference(name)
    ds, g = _lslc_got(name)
    assert ds.shape == (C.LS_S * C.LS_G, 30) and torch.isfinite(ds).all() and all(torch.isfinite(v).all() for v in g.values())
    un = C.lslc_untouched(c).to(DEV)
    assert not ds[un].contiguous().view(torch.int32).any(), "a row of d s that no kept edge points at is not +0.0"
    _others_zero(g, C.LSLC_PARAMS)
    for h, hn in enumerate("PS"):
        if c.coef[h] is None:
            assert all(not g[k].any() for k in C.LSLC_PARAMS if k.startswith("LocalSliceLgCollapse" + hn))
    _report("lslc", name, ref, {"d_s_rows": ds}, {k: g[k] for k in C.LSLC_PARAMS})


@pytest.mark.parametrize("name", C.LSLC_CASES)
def test_lslc_backward_is_linear_and_repeatable_bit_for_bit(name):
    ds, g = _lslc_got(name)
    ds1, g1 = _lslc_call(name)
    assert _same_bits([ds] + [g[k] for k in C.LSLC_PARAMS], [ds1] + [g1[k] for k in C.LSLC_PARAMS])
    ds2, g2 = _lslc_call(name, 2.0)
    assert _same_bits([2.0 * ds] + [2.0 * g[k] for k in C.LSLC_PARAMS], [ds2] + [g2[k] for k in C.LSLC_PARAMS])


# ---- the arrival head -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _arrival_forward(name):
    c = C.arrival_case(name)
    d = lambda t: t.to(DEV)
    out, state = _hp().arrivals_fwd(d(c.stime), d(c.x_src), d(c.trv), d(c.arv_p), d(c.arv_s), d(c.tpick), d(c.ipick), d(c.phase), C.EPS, train=True)
    torch.cuda.synchronize()
    return out, state


def _arrival_call(name, coef):
    res = _hp().arrivals_bwd(_arrival_forward(name)[1], coef.to(DEV))
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _arrival_got(name):
    return _arrival_call(name, C.arrival_case(name).coef)


def _arrival_tensors(res):
    return list(res[:3]) + [res[3][k] for k in C.ARRIVAL_PARAMS]


@pytest.mark.parametrize("name", C.ARRIVAL_CASES)
def test_arrivals_training_forward_and_backward_match_float64(name):
    c, ref = C.arrival_case(name), C.arrival_reference(name)
    out = _arrival_forward(name)[0]
    r = ref["f64"]["out"]["out"]
    err = float((out.cpu().double() - r).abs().max())
    print("train_heads arrivals %-13s training forward: max error %.3e, max |ref| %.3e" % (name, err, float(r.abs().max())))
    assert out.shape == r.shape and err <= 5e-6 * max(1.0, float(r.abs().max()))
    d_src, d_p, d_s, g = _arrival_got(name)
    assert all(torch.isfinite(t).all() for t in _arrival_tensors((d_src, d_p, d_s, g)))
    un = C.arrival_unexplained(c).to(DEV)
    assert not d_p[un].any() and not d_s[un].any(), "a pick without a surviving edge has a gradient"
    _others_zero(g, C.ARRIVAL_PARAMS)
    _report("arrivals", name, ref, {"d_src_embed": d_src, "d_arrival_p": d_p, "d_arrival_s": d_s}, {k: g[k] for k in C.ARRIVAL_PARAMS})


@pytest.mark.parametrize("name", C.ARRIVAL_CASES)
def test_arrivals_backward_is_linear_and_repeatable_bit_for_bit(name):
    c, got = C.arrival_case(name), _arrival_tensors(_arrival_got(name))
    assert _same_bits(got, _arrival_tensors(_arrival_call(name, c.coef)))
    assert _same_bits([2.0 * t for t in got], _arrival_tensors(_arrival_call(name, 2.0 * c.coef)))


@pytest.mark.parametrize("name", C.ARRIVAL_CASES)
def test_arrivals_backward_is_local_in_the_source(name):
    """The cotangent of one source alone: `d src_embed` of every other source is exactly zero, its own row is the full call's, and
    the one-source calls add up to the full call (float64 sums), all within the parity bound against the float64 reference."""
    c, ref = C.arrival_case(name), C.arrival_reference(name)
    rows = torch.zeros((c.n_src, 30), dtype=torch.float64)
    sums = None
    for i in range(c.n_src):
        coef = torch.zeros_like(c.coef)
        coef[i] = c.coef[i]
        res = _arrival_call(name, coef)
        other = torch.arange(c.n_src, device=DEV) != i
        assert not res[0][other].any(), "source %d's cotangent reaches another source's embedding" % i
        rows[i] = res[0][i].cpu().double()
        part = [t.cpu().double() for t in _arrival_tensors(res)[1:]]
        sums = part if sums is None else [a + b for a, b in zip(sums, part)]
    got_rows = {"d_src_embed": rows, "d_arrival_p": sums[0], "d_arrival_s": sums[1]}
    _report("arrivals", name + "/local", ref, got_rows, dict(zip(C.ARRIVAL_PARAMS, sums[2:])))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing_and_touch_nothing(monkeypatch):
    hp = _hp()
    ds, g = _lslc_got("n17")
    full = _arrival_tensors(_arrival_got("null_filtered"))
    c, a = C.lslc_case("n17"), C.arrival_case("null_filtered")
    args = _lslc_inputs("n17")
    state = _arrival_forward("null_filtered")[1]
    held = [t for t in args if torch.is_tensor(t)] + list(args[1]) + list(state[0]) + list(state[1]) + [state[2], state[3], state[4]]
    before = [t.clone() for t in held]
    calls = []
    checked = engine._lib.check
    monkeypatch.setattr(engine._lib, "check", lambda rc, what="": (calls.append(what), checked(rc, what))[1])      # every launch reports here
    cot = [k.to(DEV) for k in c.coef]
    s, tabs, dtp, tpick, ipick, phase, tlatent, eps = args
    bad = [(TypeError, dict(d_p=cot[0].double())), (TypeError, dict(d_s=cot[1].half())), (TypeError, dict(d_s=cot[1].cpu().numpy())),
           (ValueError, dict(d_p=cot[0][:-1])), (ValueError, dict(d_s=torch.cat((cot[1], cot[1][:1])))), (ValueError, dict(d_p=cot[0].t())),
           (ValueError, dict(d_s=cot[1].cpu())), (ValueError, dict(ipick=ipick.long())), (ValueError, dict(tabs=(tabs[0].long(), tabs[1]))),
           (ValueError, dict(tpick=tpick[:0], ipick=ipick[:0], phase=phase[:0], d_p=cot[0][:0], d_s=cot[1][:0]))]       # n == 0
    for exc, kw in bad:
        k = dict(s=s, tabs=tabs, dtp=dtp, tpick=tpick, ipick=ipick, phase=phase, tlatent=tlatent, d_p=cot[0], d_s=cot[1])
        k.update(kw)
        with pytest.raises(exc):
            hp.lslc_bwd(k["s"], k["tabs"], k["dtp"], k["tpick"], k["ipick"], k["phase"], k["tlatent"], eps, k["d_p"], k["d_s"])
    coef = a.coef.to(DEV)
    for exc, d_out in ((TypeError, coef.double()), (TypeError, coef.cpu().numpy()), (ValueError, coef[:, :-1]), (ValueError, coef[:1]),
                       (ValueError, coef.reshape(-1)), (ValueError, coef.cpu())):
        with pytest.raises(exc):
            hp.arrivals_bwd(state, d_out)
    d = lambda t: t.to(DEV)
    with pytest.raises(ValueError, match="at least one pick"):                                                   # n == 0
        hp.arrivals_fwd(d(a.stime), d(a.x_src), d(a.trv), d(a.arv_p[:0]), d(a.arv_s[:0]), d(a.tpick[:0]), d(a.ipick[:0]), d(a.phase[:0]),
                        C.EPS, train=True)
    assert calls == []
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(held, before))
    ds1, g1 = _lslc_call("n17")                                                                                  # and the next calls are as before
    assert _same_bits([ds] + [g[k] for k in C.LSLC_PARAMS], [ds1] + [g1[k] for k in C.LSLC_PARAMS])
    assert _same_bits(full, _arrival_tensors(_arrival_call("null_filtered", a.coef)))
