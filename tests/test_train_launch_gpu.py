"""GPU: the host side of the training backward (the three P-sized passes of DataAggregation, the four of the association heads, the
G- / Q-sized tail, LocalSliceLgCollapse P / S, Arrivals). One training step per fixture runs through the drop-in class with every
raw engine backward (`path_train_bwd`, `assoc_train_bwd`, `lslc_bwd`, `arrivals_bwd`) recorded; the recorded calls are then made
again on the engine, and the two halves of the fused call (`tail_train_bwd`, `train_bwd`) are called on its arguments. Fixtures:
Cartesian product graphs of 6 x 40 (one workgroup, partial last tile) and 33 x 257 (several workgroups, odd tails), the irregular
product graph of 14 x 50 (product-level passes), the two static-term model definitions at 12 x 60, and the association step
(four outputs) on a Cartesian (7 x 45) and an irregular (14 x 50) graph. Repeats and the fused call against its halves are
bitwise; the gradients are compared with the oracle's autograd at the bound tests/test_hip_parity.py uses for these fixtures."""
import functools
import os

import numpy as np
import pytest
import torch

from genie_amd import graph, module
from tests.util import GOLDEN_DIR, Case, max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH_CASES = ["tiny_6x40", "odd_33x257", "subgraph_14x50", "edges_12x60", "abspos_12x60"]      # forward_fixed_source (y, x)
ASSOC_CASES = ["assoc_7x45", "assoc_subgraph_14x50"]                                             # the four-output step
RECORDED = ("path_train_bwd", "assoc_train_bwd", "lslc_bwd", "arrivals_bwd")


def tensors(v):
    """The tensors of a backward's result (tensor, tuple or gradient dict), in a fixed order."""
    if torch.is_tensor(v):
        return [v]
    if isinstance(v, dict):
        return [v[k] for k in sorted(v)]
    return [t for item in v for t in tensors(item)]


def record(hp):
    """Wrap the raw backward entry points of an engine: name -> list of (args, kwargs, copies of the result's tensors)."""
    calls = {name: [] for name in RECORDED}
    for name in RECORDED:
        def wrapped(*a, _orig=getattr(hp, name), _log=calls[name], **k):
            out = _orig(*a, **k)
            _log.append((a, k, [t.clone() for t in tensors(out)]))
            return out
        setattr(hp, name, wrapped)
    return calls


def unwrap(hp):
    for name in RECORDED:
        delattr(hp, name)          # the instance attribute set by record(): the class's method is back


def bound(ref, gmax):
    """tests/test_hip_parity.py, the training steps of these fixtures: 2e-4 of the gradient's own scale, with a floor of 1e-3 of the
    model's largest gradient for scalars that are sums of cancelling terms."""
    return 2e-4 * max(float(ref.abs().max()), 1e-3 * gmax) + 1e-12


@functools.lru_cache(maxsize=None)
def step(name):
    """One training step of a fixture on the GPU and by the oracle's autograd for the same cotangents: computed once.
    Returns (net, recorded calls, {parameter: (gradient, oracle's gradient)})."""
    from oracle import genie_oracle as O
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    w0 = O.weights_from_npz(z)
    S, G = int(z["n_sta"]), int(z["n_grid"])
    four = name in ASSOC_CASES
    edges, abspos = w0["DataAggregation.l1_t1_2.weight"].shape[1] == 68, w0["DataAggregation.init_trns.weight"].shape[1] == 14
    t = lambda k, dt=torch.float32, dev=DEV: torch.from_numpy(np.asarray(z[k])).to(dt).to(dev)
    c = lambda k, dt=torch.float32: t(k, dt, "cpu")
    net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV, use_updated_model_definition=edges,
                                                use_absolute_pos=abspos)
    net.load_state_dict({k: v.clone() for k, v in w0.items()}, strict=True)
    net.train()
    if "pairs" in z.files:
        A_src_in_sta = torch.from_numpy(z["pairs"]).long()
        A_in_sta, A_in_src, A_src_in_prod = graph.subgraph_product_edges(z["A_sta_sta"], z["A_src_src"], z["pairs"])
    else:
        A_in_sta, A_in_src, A_src_in_prod, A_src_in_sta = graph.cartesian_product_edges(z["A_sta_sta"], z["A_src_src"], S, G)
    ea = graph.GraphEdges(x=t("edge_attr"), edge_index=A_src_in_prod.to(DEV))
    ea_flip = graph.GraphEdges(x=t("edge_attr"), edge_index=A_src_in_prod.flip(0).contiguous().to(DEV))
    base = (A_in_sta.to(DEV), A_in_src.to(DEV), ea, ea_flip, A_src_in_sta.to(DEV), t("A_src_src", torch.long))
    okw = {}
    if edges:
        okw["pos_rel"] = (O.edge_pos_features(c("locs"), A_in_sta, A_src_in_sta[0]), O.edge_pos_features(c("x_grid"), A_in_src, A_src_in_sta[1]))
    w = {k: v.clone().requires_grad_(True) for k, v in w0.items()}
    g = torch.Generator().manual_seed(11)
    if four:
        graphs = base + (t("A_edges_p", torch.long), t("A_edges_s", torch.long), t("dt_partition"), t("tlatent"))
        tail = (t("tpick"), t("ipick", torch.long), t("phase_label"), t("locs"), t("x_grid"), t("x_query"), t("x_query_src"),
                t("t_query"), t("tq_sample"), t("trv_out_q"))
        net.set_adjacencies(*graphs, t("locs"), t("x_grid"))
        calls = record(net._hip)
        outs = net.forward_fixed(t("Slice"), t("Mask"), *tail)
        if abspos:
            okw["abs_pos"] = (c("locs"), A_src_in_sta)
        ref = O.forward_fixed(w, c("Slice"), c("Mask"), A_in_sta, A_in_src, c("edge_attr"), A_src_in_prod, c("A_src_src", torch.long),
                              c("A_edges_p", torch.long), c("A_edges_s", torch.long), c("dt_partition"), c("tlatent"), c("tpick"),
                              c("ipick", torch.long), c("phase_label"), c("x_grid"), c("x_query"), c("x_query_src"), c("t_query"),
                              c("tq_sample"), c("trv_out_q"), S, **okw)
    else:
        net.set_adjacencies(*base, None, None, None, None, t("locs"), t("x_grid"))
        calls = record(net._hip)
        outs = net.forward_fixed_source(t("Slice"), t("Mask"), None, None, None, t("locs"), t("x_grid"), t("x_query"), t("t_query"))
        Slice = O.absolute_pos_inputs(c("Slice"), c("locs"), c("x_grid"), A_src_in_sta) if abspos else c("Slice")
        ref = O.forward_fixed_source(w, Slice, c("Mask"), A_in_sta, A_in_src, c("edge_attr"), A_src_in_prod, c("A_src_src", torch.long),
                                     c("x_grid"), c("x_query"), c("t_query"), **okw)
    coef = [torch.randn(o.shape, generator=g) for o in outs]
    for o, r in zip(outs, ref):
        assert max_abs(o.detach().cpu(), r.detach()) <= 1e-5
    sum((o * a.to(DEV)).sum() for o, a in zip(outs, coef)).backward()
    sum((o * a).sum() for o, a in zip(ref, coef)).backward()
    torch.cuda.synchronize()
    unwrap(net._hip)
    grads = {}
    for k, p in net.named_parameters():
        if w[k].grad is not None:
            assert p.grad is not None and tuple(p.grad.shape) == tuple(w[k].grad.shape), k
            grads[k] = (p.grad.detach().cpu().clone(), w[k].grad)
    return net, calls, grads


def recorded_names(name):
    return RECORDED if name in ASSOC_CASES else RECORDED[:1]


@pytest.mark.parametrize("name", PATH_CASES + ASSOC_CASES)
def test_every_recorded_backward_ran_once_and_repeats_bitwise(name):
    """(a) `path_train_bwd` (and `assoc_train_bwd`, `lslc_bwd` with both heads, `arrivals_bwd` in the four-output step) called twice
    more on the arguments of the training step: both results equal the step's own, tensor by tensor."""
    net, calls, _ = step(name)
    hp = net._hip
    for entry in recorded_names(name):
        assert len(calls[entry]) == 1, entry
        a, k, first = calls[entry][0]
        if entry == "lslc_bwd":
            assert a[8] is not None and a[9] is not None          # d_p and d_s: both heads ran
        for rep in range(2):
            again = tensors(getattr(hp, entry)(*a, **k))
            torch.cuda.synchronize()
            assert len(again) == len(first)
            for i, (x, y) in enumerate(zip(again, first)):
                assert torch.equal(x, y), (entry, rep, i)
        assert all(bool(torch.isfinite(x).all()) for x in first), entry
        assert any(float(x.abs().max()) > 0 for x in first), entry


def halves(name):
    """The fused call of a fixture's step without a gradient on the query rows' SpatialAttention output (the tail's own entry
    point takes none), its gradient blob, and the two halves on the same arguments."""
    net, calls, _ = step(name)
    hp = net._hip
    a, k, _ = calls["path_train_bwd"][0]
    assert not k
    Slice, Mask, edge_attr, pos, x_query, knn, t_query, save, tsave, d_y, d_x, d_xs, d_ylat = a[:13]
    knn = knn.contiguous()
    fused = lambda: next(iter(hp.path_train_bwd(Slice, Mask, edge_attr, pos, x_query, knn, t_query, save, tsave, d_y, d_x, d_xs, d_ylat).values()))._base
    tail = lambda: hp.tail_train_bwd(pos, x_query, knn, t_query, tsave, d_y, d_x, d_xs, d_ylat)
    front = lambda d_r: next(iter(hp.train_bwd(Slice, Mask, edge_attr, save, d_r[:, :30]).values()))._base
    return hp, fused, tail, front


@pytest.mark.parametrize("name", PATH_CASES + ASSOC_CASES)
def test_the_halves_repeat_bitwise_and_add_up_to_the_fused_call(name):
    """(a) for `tail_train_bwd` and `train_bwd`, and (b): over the weight mirror the fused blob is the tail's plus the front's
    driven by the tail's d r; past the mirror (the time-query gradient rows) it is the tail's."""
    hp, fused, tail, front = halves(name)
    d_r, tail_blob = tail()
    d_r2, tail_blob2 = tail()
    assert torch.equal(d_r, d_r2) and torch.equal(tail_blob, tail_blob2)
    front_blob, front_blob2 = front(d_r), front(d_r)
    assert torch.equal(front_blob, front_blob2)
    whole = fused()
    torch.cuda.synchronize()
    n = hp._blob.numel()
    assert front_blob.numel() == n and whole.numel() == tail_blob.numel() > n
    assert torch.equal(whole[:n], tail_blob[:n] + front_blob)
    assert torch.equal(whole[n:], tail_blob[n:])
    for b in (tail_blob[:n], front_blob, d_r):
        assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
    both = (tail_blob[:n] != 0) & (front_blob != 0)          # the halves own different parameters: nothing is added twice
    assert not bool(both.any())


@pytest.mark.parametrize("name", PATH_CASES + ASSOC_CASES)
def test_every_gradient_matches_the_oracle(name):
    """(c) every parameter gradient of the step (= what the recorded calls returned, by test (a)) against the oracle's autograd for
    the same cotangents."""
    net, calls, grads = step(name)
    gmax = max(float(ref.abs().max()) for _, ref in grads.values())
    worst = 0.0
    for k, (got, ref) in grads.items():
        err, tol = max_abs(got, ref), bound(ref, gmax)
        worst = max(worst, err / tol)
        print("%-28s %-60s err %.3e bound %.3e" % (name, k, err, tol))
    print("%s: %d gradients, worst error / bound %.3f" % (name, len(grads), worst))
    for k, (got, ref) in grads.items():
        assert max_abs(got, ref) <= bound(ref, gmax), (k, max_abs(got, ref), bound(ref, gmax))
    assert len(grads) >= (130 if name in ASSOC_CASES else 80)
    if name.startswith("edges"):
        assert float(grads["DataAggregation.l1_t1_2.weight"][1][:, 60:64].abs().max()) > 0
        assert float(grads["DataAggregation.l2_t2_2.weight"][1][:, 90:94].abs().max()) > 0
    if name.startswith("abspos"):
        assert float(grads["DataAggregation.init_trns.weight"][1][:, 4:10].abs().max()) > 0
