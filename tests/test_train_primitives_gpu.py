"""GPU: the stand-alone training primitives of the C ABI (genie_nbr_mean_bwd, genie_seg_rows, genie_prelu_bwd, genie_linear_bwd_wb;
genie_nbr_mean through the adjoint identity) against exact or fp64 references at their dispatch edges. The fused training passes
no longer call the first four, so the end-to-end gradient tests do not reach them; an integrator still can.

Tolerances are derived, never measured: where the inputs make every operation exact (integers, power-of-two weights) the result
must EQUAL the fp64 reference; genie_seg_rows fixes its summation order, so it is compared bit for bit with that order in fp32;
elsewhere the bound is the fp32 rounding of the number of operations per element (tests/restatements.py, pinned on the CPU by
tests/test_train_primitives_cpu.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from genie_amd import _lib, engine, synthetic
from genie_amd.engine import _ptr, _stream
from tests import restatements as R
from tests.util import GOLDEN_DIR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ERR_ARG, ERR_STATE = -1, -3          # GENIE_ERR_ARG / GENIE_ERR_STATE of include/genie_hip.h
S, G = R.HANDMADE_S, R.HANDMADE_G
NULL = ctypes.c_void_p(0)


def _ctx(n_sta, n_grid, A_sta, A_src):
    return engine.HipPath(n_sta, n_grid, engine.csr_from_edges(A_sta, n_sta), engine.csr_from_edges(A_src, n_grid), device=DEV)


@pytest.fixture(scope="module")
def hp_hand():
    """Context of the hand-made 20-station / 24-source-node graphs, with their fp64 mean matrices and degrees."""
    A_sta, A_src = R.handmade_graphs()
    return _ctx(S, G, A_sta, A_src), R.mean_adjacency(A_sta, S), R.mean_adjacency(A_src, G)


@pytest.fixture(scope="module")
def hp_any():
    """A context for the calls that use none of its graphs (the engine wrappers of genie_prelu_bwd / genie_linear_bwd_wb)."""
    none = torch.zeros((2, 0), dtype=torch.long)
    return _ctx(3, 4, none, none)


def _within(got, ref, bound, what):
    """|got - ref| <= bound element by element (fp64); prints the largest share of the bound that is used."""
    err = (got.double().cpu() - ref).abs()
    used = float((err / bound.clamp(min=1e-300)).max())
    print("%s: max err %.3g, at most %.3f of the bound" % (what, float(err.max()), used))
    assert bool((err <= bound).all()), (what, float(err.max()), used)


# ---- 1. genie_nbr_mean_bwd -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [15, 16, 30, 31, 32])
def test_nbr_mean_bwd_matches_the_dense_fp64_adjoint(hp_hand, C):
    """dx = A^T g on the hand-made graphs (in-degrees 0, 1, 7, 8, 9, 15, 16, 17, a hub of out-degree 18 / 22, a node nobody lists,
    a self-loop, a neighbour listed twice), at row widths that pad to 16, 30 and 32 floats (the three instantiations of
    k_nbr_mean). Per element |got - ref| <= (out-degree + 2) 2^-24 sum_i |A[i, j] g[i]| (restatements.nbr_mean_adjoint_bound); the
    row of a node that is nobody's neighbour is exactly zero. Either gradient alone gives the same bits."""
    hp, (As, _, out_s), (Ag, _, out_g) = hp_hand
    gen = torch.Generator().manual_seed(100 + C)
    g1, g2 = torch.randn((S * G, C), generator=gen), torch.randn((S * G, C), generator=gen)
    d1, d2 = hp.nbr_mean_bwd(g1.to(DEV), g2.to(DEV))
    assert tuple(d1.shape) == (S * G, C) and tuple(d2.shape) == (S * G, C)
    r1, r2 = R.nbr_mean_adjoint_ref(As, Ag, g1, g2, S, G)
    b1, b2 = R.nbr_mean_adjoint_bound(As, Ag, out_s, out_g, g1, g2, S, G)
    _within(d1, r1, b1, "dx_sta C=%d" % C)
    _within(d2, r2, b2, "dx_src C=%d" % C)
    assert float(d1.view(G, S, C)[:, 19].abs().max()) == 0.0 and float(d2.view(G, S, C)[23].abs().max()) == 0.0
    only1, none = hp.nbr_mean_bwd(g1.to(DEV), None)
    assert none is None and torch.equal(only1, d1)
    none, only2 = hp.nbr_mean_bwd(None, g2.to(DEV))
    assert none is None and torch.equal(only2, d2)


@pytest.mark.parametrize("C", [16, 30, 32])
def test_nbr_mean_bwd_is_exact_with_power_of_two_degrees(C):
    """Every in-degree a power of two (a ring with 1, 2, 4 or 8 neighbours) and small integer gradients: every weight, product and
    partial sum is exact in fp32, so dx equals the fp64 reference, and so do the means of genie_nbr_mean."""
    A_sta, A_src = R.power_of_two_ring(S), R.power_of_two_ring(G)
    hp = _ctx(S, G, A_sta, A_src)
    As, Ag = R.mean_adjacency(A_sta, S)[0], R.mean_adjacency(A_src, G)[0]
    gen = torch.Generator().manual_seed(C)
    g1 = torch.randint(-4, 5, (S * G, C), generator=gen).float()
    g2 = torch.randint(-4, 5, (S * G, C), generator=gen).float()
    d1, d2 = hp.nbr_mean_bwd(g1.to(DEV), g2.to(DEV))
    r1, r2 = R.nbr_mean_adjoint_ref(As, Ag, g1, g2, S, G)
    assert torch.equal(d1.double().cpu(), r1) and torch.equal(d2.double().cpu(), r2)
    o1, o2 = hp.nbr_mean(g1.to(DEV), g2.to(DEV))
    f1, f2 = R.nbr_mean_ref(As, Ag, g1, g2, S, G)
    assert torch.equal(o1.double().cpu(), f1) and torch.equal(o2.double().cpu(), f2)


@pytest.mark.parametrize("C", [16, 30, 32])
def test_nbr_mean_and_its_backward_are_adjoint(hp_hand, C):
    """<nbr_mean(x), g> = <x, nbr_mean_bwd(g)>, both summed in fp64 from the kernels' fp32 outputs: they differ by at most
    sum |g| bound(mean) + sum |x| bound(adjoint), the two per-element bounds of restatements.py carried through the inner products."""
    hp, (As, in_s, out_s), (Ag, in_g, out_g) = hp_hand
    gen = torch.Generator().manual_seed(200 + C)
    x1, x2, g1, g2 = (torch.randn((S * G, C), generator=gen) for _ in range(4))
    o1, o2 = hp.nbr_mean(x1.to(DEV), x2.to(DEV))
    d1, d2 = hp.nbr_mean_bwd(g1.to(DEV), g2.to(DEV))
    f1, f2 = R.nbr_mean_bound(As, Ag, in_s, in_g, x1, x2, S, G)
    b1, b2 = R.nbr_mean_adjoint_bound(As, Ag, out_s, out_g, g1, g2, S, G)
    for o, d, x, g, f, b, what in ((o1, d1, x1, g1, f1, b1, "station"), (o2, d2, x2, g2, f2, b2, "source")):
        lhs = float((o.double().cpu() * g.double()).sum())
        rhs = float((x.double() * d.double().cpu()).sum())
        tol = float((g.double().abs() * f).sum() + (x.double().abs() * b).sum())
        print("%s graph C=%d: <Ax, g> %.9g, <x, A^T g> %.9g, difference %.3g, bound %.3g" % (what, C, lhs, rhs, abs(lhs - rhs), tol))
        assert abs(lhs - rhs) <= tol, (what, lhs, rhs, tol)


def test_nbr_mean_bwd_large_cartesian_graph_strides_over_the_grid():
    """64 stations x 4500 source nodes, ragged kNN graphs: P = 288 000 product nodes against at most 4096 workgroups of 64 (16-float
    rows) or 32 (32-float rows) nodes, so the node loop of k_nbr_mean takes its grid stride. Reference: sparse fp64 products, computed
    once at 32 columns (the columns are independent: the 16-column call gets the first 16)."""
    Sn, Gn = 64, 4500
    geom = synthetic.Geometry(Sn, Gn, L=300e3, n_query=5, seed=41)
    rng = np.random.default_rng(1341)
    A_sta = torch.from_numpy(np.ascontiguousarray(geom.A_sta_sta[:, rng.random(geom.A_sta_sta.shape[1]) >= 0.25]))
    A_src = torch.from_numpy(np.ascontiguousarray(geom.A_src_src[:, rng.random(geom.A_src_src.shape[1]) >= 0.25]))
    hp = _ctx(Sn, Gn, A_sta, A_src)
    As, _, out_s = R.mean_adjacency(A_sta, Sn)
    Ag, _, out_g = R.mean_adjacency(A_src, Gn, sparse=True)
    gen = torch.Generator().manual_seed(42)
    g1, g2 = torch.randn((Sn * Gn, 32), generator=gen), torch.randn((Sn * Gn, 32), generator=gen)
    r1, r2 = R.nbr_mean_adjoint_ref(As, Ag, g1, g2, Sn, Gn)
    b1, b2 = R.nbr_mean_adjoint_bound(As, Ag, out_s, out_g, g1, g2, Sn, Gn)
    for C in (16, 32):
        d1, d2 = hp.nbr_mean_bwd(g1[:, :C].contiguous().to(DEV), g2[:, :C].contiguous().to(DEV))
        _within(d1, r1[:, :C], b1[:, :C], "large dx_sta C=%d" % C)
        _within(d2, r2[:, :C], b2[:, :C], "large dx_src C=%d" % C)


def test_nbr_mean_bwd_does_not_depend_on_who_built_the_reversed_graphs():
    """The reversed graphs of a context are built by the first genie_nbr_mean_bwd (without the pair arrays of the training kernels) or
    by the first training backward (whole), and a training backward after genie_nbr_mean_bwd replaces them: dx is bit-equal in all
    three states, and within the bound of the dense adjoint."""
    from oracle import genie_oracle as O
    Sn, Gn = 24, 120
    geom = synthetic.Geometry(Sn, Gn, L=150e3, n_query=10, seed=77)
    win = synthetic.make_window(geom, 600, seed=78)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)
    wd = {k: v.to(DEV) for k, v in O.weights_from_npz(np.load(os.path.join(GOLDEN_DIR, "assoc_7x45.npz"))).items()}
    Slice, Mask, ea = t(win["Slice"]), t(win["Mask"]), t(geom.edge_attr())
    A_sta, A_src = torch.from_numpy(geom.A_sta_sta), torch.from_numpy(geom.A_src_src)
    gen = torch.Generator().manual_seed(3)
    g1, g2 = torch.randn((Sn * Gn, 30), generator=gen), torch.randn((Sn * Gn, 30), generator=gen)

    def train_step(hp):
        r, _, save = hp.train_fwd(Slice, Mask, ea)
        grads = hp.train_bwd(Slice, Mask, ea, save, torch.ones_like(r))
        assert all(bool(torch.isfinite(v).all()) for v in grads.values())

    def context():
        hp = _ctx(Sn, Gn, A_sta, A_src)
        hp.set_weights(wd)
        return hp

    first = context()
    own = first.nbr_mean_bwd(g1.to(DEV), g2.to(DEV))                   # built by genie_nbr_mean_bwd itself
    train_step(first)
    replaced = first.nbr_mean_bwd(g1.to(DEV), g2.to(DEV))              # replaced whole by the training backward
    second = context()
    train_step(second)
    trained = second.nbr_mean_bwd(g1.to(DEV), g2.to(DEV))              # built by the training backward
    for k in range(2):
        assert torch.equal(own[k], replaced[k]) and torch.equal(own[k], trained[k]), k
    (As, _, out_s), (Ag, _, out_g) = R.mean_adjacency(A_sta, Sn), R.mean_adjacency(A_src, Gn)
    r = R.nbr_mean_adjoint_ref(As, Ag, g1, g2, Sn, Gn)
    b = R.nbr_mean_adjoint_bound(As, Ag, out_s, out_g, g1, g2, Sn, Gn)
    _within(own[0], r[0], b[0], "dx_sta 24x120")
    _within(own[1], r[1], b[1], "dx_src 24x120")


def test_nbr_mean_bwd_refuses_bad_calls_without_writing(hp_hand):
    """Through the raw entry point: a row width other than 16 / 30 / 32 and an input without its output are argument errors, a
    context of an irregular product graph is a state error; the output buffers keep their bytes and a refused call leaves the
    context as it was."""
    hp = hp_hand[0]
    lib = hp.lib
    g = torch.ones((S * G, 32), device=DEV)
    outs = [torch.full((S * G, 32), -7.0, device=DEV) for _ in range(2)]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((o == -7.0).all()) for o in outs)

    assert lib.genie_nbr_mean_bwd(hp.ctx, _ptr(g), _ptr(g), _ptr(outs[0]), _ptr(outs[1]), 24, _stream()) == ERR_ARG
    assert untouched()
    # on a FRESH context the refused width builds no reversed graphs either: the library's pool holds what it held, and the first
    # valid call is what allocates them
    fresh = _ctx(S, G, *R.handmade_graphs())
    dev_index = torch.device(DEV).index

    def live_blocks():
        b, n = ctypes.c_int64(-1), ctypes.c_int64(-1)
        _lib.check(lib.genie_pool_stats(dev_index, ctypes.byref(b), ctypes.byref(n), None), "genie_pool_stats")
        return b.value, n.value

    torch.cuda.synchronize()
    before = live_blocks()
    assert lib.genie_nbr_mean_bwd(fresh.ctx, _ptr(g), _ptr(g), _ptr(outs[0]), _ptr(outs[1]), 24, _stream()) == ERR_ARG
    assert live_blocks() == before and untouched()
    assert lib.genie_nbr_mean_bwd(fresh.ctx, _ptr(g), _ptr(g), _ptr(outs[0]), _ptr(outs[1]), 32, _stream()) == 0
    assert live_blocks()[1] > before[1]
    outs = [torch.full((S * G, 32), -7.0, device=DEV) for _ in range(2)]
    assert lib.genie_nbr_mean_bwd(hp.ctx, _ptr(g), _ptr(g), NULL, _ptr(outs[1]), 32, _stream()) == ERR_ARG
    assert lib.genie_nbr_mean_bwd(hp.ctx, _ptr(g), _ptr(g), _ptr(outs[0]), NULL, 32, _stream()) == ERR_ARG
    assert lib.genie_nbr_mean_bwd(None, _ptr(g), _ptr(g), _ptr(outs[0]), _ptr(outs[1]), 32, _stream()) == ERR_ARG
    assert untouched()
    # irregular product graph (genie_ctx_create_subgraph)
    Sn, Gn = 24, 120
    geom = synthetic.Geometry(Sn, Gn, L=150e3, n_query=10, seed=77)
    sta = engine.csr_from_edges(torch.from_numpy(geom.A_sta_sta), Sn)
    src = engine.csr_from_edges(torch.from_numpy(geom.A_src_src), Gn)
    pairs = engine.subgraph_pairs_device(torch.from_numpy(geom.locs).to(DEV), torch.from_numpy(geom.x_grid).to(DEV), max_deg_offset=0.3,
                                         k_nearest_pairs=12)
    sub = engine.subgraph_csr_device(pairs, Gn, sta, src)
    irregular = engine.HipPath(Sn, Gn, sta, src, grid_order=engine.morton_order(geom.x_grid), device=DEV, subgraph=sub)
    g = torch.ones((Sn * Gn, 32), device=DEV)
    outs = [torch.full((Sn * Gn, 32), -7.0, device=DEV) for _ in range(2)]
    assert lib.genie_nbr_mean_bwd(irregular.ctx, _ptr(g), _ptr(g), _ptr(outs[0]), _ptr(outs[1]), 32, _stream()) == ERR_STATE
    assert untouched()
    with pytest.raises(_lib.GenieHipError):
        irregular.nbr_mean_bwd(g[:sub["n_prod"]], None)


# ---- 2. genie_seg_rows ----------------------------------------------------------------------------------------------------------------

SEG_P = 4000


def _seg_targets(n):
    """Edge targets of the genie_seg_rows cases: -1 entries (dropped edges), runs of one, target 0 and target P - 1; the long case adds
    one run of 40 equal targets among 2570 edges, a count that is no multiple of the 32 edges of a workgroup."""
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    if n == 1:
        return np.array([SEG_P - 1], dtype=np.int32)
    if n == 10:
        return np.array([-1, 0, 0, 7, SEG_P - 1, -1, 7, 3, 0, SEG_P - 1], dtype=np.int32)
    rng = np.random.default_rng(n)
    t = rng.integers(0, SEG_P, n)
    t[t == 1234] = 1235
    t[rng.random(n) < 0.1] = -1
    t[rng.choice(n, 40, replace=False)] = 1234
    t[t == 0] = 1
    t[t == SEG_P - 1] = SEG_P - 2
    free = np.flatnonzero(t != 1234)
    t[free[0]], t[free[-1]] = SEG_P - 1, 0                  # the largest target on the first edge, target 0 on the last
    return t.astype(np.int32)


@pytest.mark.parametrize("n_edges", [0, 1, 10, 2570])
def test_seg_rows_equals_the_sequential_fp32_sum(hp_any, n_edges):
    """genie_seg_rows adds the 30 leading floats of every edge row into d_s [P, 30] per target: edges of one target in the order of
    `order` (the stable sort by target, as engine.lslc_bwd builds it), then ONE addition into d_s. That order is the contract, so the
    result is bit-equal to the same loop in fp32 on the host. d_s starts random (the kernel adds) and rows that are no target keep
    their bits; columns 30, 31 of the edge rows hold 1e30 and change nothing (the two-float tail of the eighth lane stays inside its
    row); two runs agree bit for bit."""
    lib = hp_any.lib
    etgt = _seg_targets(n_edges)
    counts = np.bincount(etgt[etgt >= 0], minlength=SEG_P)
    if n_edges >= 10:
        assert (etgt < 0).any() and counts[0] >= 1 and counts[SEG_P - 1] >= 1 and (counts == 1).any()
    if n_edges == 2570:
        assert counts[1234] == 40 and counts.max() == 40 and n_edges % 32 != 0
    rng = np.random.default_rng(50 + n_edges)
    erow = rng.normal(0, 1, (max(n_edges, 1), 32)).astype(np.float32)          # (one row at n_edges = 0: the pointers are not null)
    erow[:, 30:] = 0.0
    ds0 = rng.normal(0, 1, (SEG_P, 30)).astype(np.float32)
    order = torch.sort(torch.from_numpy(etgt), stable=True)[1].to(torch.int32)
    ref = R.seg_rows_sequential(erow[:n_edges], etgt, order.numpy(), ds0)
    d_etgt = torch.from_numpy(etgt).to(DEV) if n_edges else torch.zeros(1, dtype=torch.int32, device=DEV)
    d_order = order.to(DEV) if n_edges else torch.zeros(1, dtype=torch.int32, device=DEV)

    def run(rows):
        ds = torch.from_numpy(ds0).to(DEV)
        d_erow = torch.from_numpy(rows).to(DEV)
        assert lib.genie_seg_rows(_ptr(d_erow), _ptr(d_etgt), _ptr(d_order), n_edges, _ptr(ds), _stream()) == 0
        torch.cuda.synchronize()
        return ds.cpu()

    poisoned = erow.copy()
    poisoned[:, 30:] = 1e30
    got, again, clean = run(poisoned), run(poisoned), run(erow)
    assert torch.equal(got, torch.from_numpy(ref))
    assert torch.equal(got, again) and torch.equal(got, clean)
    no_target = torch.from_numpy(counts == 0)
    assert bool(no_target.any()) and torch.equal(got[no_target], torch.from_numpy(ds0)[no_target])


def test_seg_rows_refuses_null_pointers_and_negative_counts(hp_any):
    lib = hp_any.lib
    erow = torch.ones((4, 32), device=DEV)
    etgt = torch.zeros(4, dtype=torch.int32, device=DEV)
    order = torch.arange(4, dtype=torch.int32, device=DEV)
    ds = torch.full((3, 30), -7.0, device=DEV)
    for args in ((NULL, _ptr(etgt), _ptr(order), 4), (_ptr(erow), NULL, _ptr(order), 4), (_ptr(erow), _ptr(etgt), NULL, 4),
                 (_ptr(erow), _ptr(etgt), _ptr(order), -1)):
        assert lib.genie_seg_rows(args[0], args[1], args[2], args[3], _ptr(ds), _stream()) == ERR_ARG
    assert lib.genie_seg_rows(_ptr(erow), _ptr(etgt), _ptr(order), 4, NULL, _stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((ds == -7.0).all())


# ---- 3. genie_prelu_bwd at zero ------------------------------------------------------------------------------------------------------

PRELU_SPECIALS = [0.0, -0.0, 1e-40, -1e-40]          # both zeros and a subnormal of each sign (fp32: below 1.18e-38)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 4 * 256 * 2048 + 3, 4 * (256 * 2048 + 1) + 3])
def test_prelu_bwd_matches_autograd_at_zero_and_in_the_tail(hp_any, n):
    """torch.nn.functional.prelu's backward gives x > 0 ? dy : slope * dy: the slope applies AT zero, of either sign. dx of
    genie_prelu_bwd is bit-equal to it on inputs that hold +0.0, -0.0 and a subnormal of each sign, in the float4 body and in the
    sub-float4 tail (n = 5, 6, 7; below four elements there is only a tail; at 4 x 256 x 2048 + 3 every thread of the grid has one
    float4 and the tail runs; one float4 more and the first thread takes the grid stride into a second one). Short inputs consist of the four special values, rotated so that each one visits every position.
    The slope gradient is the sum over x <= 0 of dy x (zeros add nothing) within (depth + 1) 2^-24 sum |dy x|, depth = the longest
    chain of additions a term goes through: 4 per float4 of a thread and one for the tail, then three 256-wide trees and the
    8 partials per thread of the final pass (8 + 8 + 8 levels). A product below the normal range (the subnormal inputs) has no
    relative accuracy: it may lose up to its own size, or 2^-149 on the subnormal grid."""
    spec = torch.tensor(PRELU_SPECIALS, dtype=torch.float32)
    assert bool((spec[2:] != 0).all()) and bool((spec[2:].abs() < 1.17549435e-38).all())
    gen = torch.Generator().manual_seed(n)
    cases = []
    if n < 8:
        for rot in range(4):
            cases.append(spec[(torch.arange(n) + rot) % 4].clone())
    else:
        x = torch.randn(n, generator=gen)
        where = torch.randint(0, n, (4096,), generator=gen)
        x[where] = spec[torch.arange(4096) % 4]
        x[:8] = spec.repeat(2)
        x[n - 7:n - 3] = spec                           # the last float4 of the body
        x[n - 3:] = spec[:3]                            # the tail
        cases.append(x)
        y = x.clone()
        y[n - 3:] = spec[1:]
        cases.append(y)
    a = torch.tensor([0.25], device=DEV, requires_grad=True)
    n4 = n // 4
    depth = 4 * -(-n4 // (2048 * 256)) + 1 + 24
    for x in cases:
        x = x.to(DEV).requires_grad_(True)
        dy = torch.randn(n, generator=gen).to(DEV)
        a.grad = None
        torch.nn.functional.prelu(x, a).backward(dy)
        dx, da = hp_any.prelu_bwd(x.detach(), dy, a.detach())
        xd = x.detach()
        assert torch.equal(dx, x.grad), (n, xd[(dx != x.grad)][:8].tolist())
        assert torch.equal(dx, torch.where(xd > 0, dy, 0.25 * dy))          # (0.25 dy is exact: the convention itself, in words)
        terms = dy.double() * xd.double() * (xd <= 0)
        ref = float(terms.sum())
        tiny = terms.abs()[(terms != 0) & (terms.abs() < 2.0 ** -126)]
        tol = (depth + 1) * R.U32 * float(terms.abs().sum()) + float(tiny.clamp(min=2.0 ** -149).sum())
        assert abs(float(da[0]) - ref) <= tol, (float(da[0]), ref, tol)


# ---- 4. genie_linear_bwd_wb at its dispatch edges -------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,M", [(31, 64, 32), (32, 65, 33), (33, 128, 128), (1, 128, 128), (32 * 1024 + 1, 1, 1),
                                   (32 * 1024 + 33, 63, 31), (64, 127, 97)])
def test_linear_bwd_wb_is_exact_on_small_integers(hp_any, N, K, M):
    """x and dy are integers in [-2, 2]: every product and partial sum is an integer below 4 N < 2^24, so any summation order is
    exact in fp32 and dW, db must EQUAL dy^T x and the column sums (one dropped or doubled row cannot hide). The shapes sit on the
    dispatch edges: K = 64 / 65 (one or two 64-column chunks per lane), M = 32 / 33 (one or two 32-output passes over dy + m0 with
    pitch M), the limits K = M = 128, N around the 32-row tile and beyond the 32 x 1024 rows one sweep of the grid covers. A guard
    element behind dW and db keeps its value; without a bias pointer dW is the same."""
    assert 4 * N < 2 ** 24
    lib = hp_any.lib
    gen = torch.Generator().manual_seed(N + K + M)
    x = torch.randint(-2, 3, (N, K), generator=gen).float().to(DEV)
    dy = torch.randint(-2, 3, (N, M), generator=gen).float().to(DEV)
    refW, refb = (dy.double().t() @ x.double()).cpu(), dy.double().sum(0).cpu()
    scratch = torch.empty(int(lib.genie_linear_bwd_scratch_floats(K)), dtype=torch.float32, device=DEV)
    dW = torch.full((M * K + 1,), -7.0, device=DEV)
    db = torch.full((M + 1,), -7.0, device=DEV)
    assert lib.genie_linear_bwd_wb(_ptr(x), _ptr(dy), N, K, M, _ptr(dW), _ptr(db), _ptr(scratch), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dW[:M * K].view(M, K).double().cpu(), refW)
    assert torch.equal(db[:M].double().cpu(), refb)
    assert float(dW[M * K]) == -7.0 and float(db[M]) == -7.0
    dW2 = torch.full((M * K + 1,), -7.0, device=DEV)
    assert lib.genie_linear_bwd_wb(_ptr(x), _ptr(dy), N, K, M, _ptr(dW2), NULL, _ptr(scratch), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dW2, dW)
    # the engine wrapper is the same call
    eW, eb = hp_any.linear_bwd_wb(x, dy)
    assert torch.equal(eW.view(-1), dW[:M * K]) and torch.equal(eb, db[:M])


def test_linear_bwd_wb_refuses_sizes_beyond_its_limits(hp_any):
    """K = 129, M = 129 and N = 0 through the raw entry point: argument errors, nothing written."""
    lib = hp_any.lib
    x = torch.ones((4, 129), device=DEV)
    dy = torch.ones((4, 129), device=DEV)
    scratch = torch.empty(int(lib.genie_linear_bwd_scratch_floats(128)), dtype=torch.float32, device=DEV)
    dW = torch.full((129 * 129,), -7.0, device=DEV)
    db = torch.full((129,), -7.0, device=DEV)
    for N, K, M in ((4, 129, 8), (4, 8, 129), (0, 8, 8)):
        assert lib.genie_linear_bwd_wb(_ptr(x), _ptr(dy), N, K, M, _ptr(dW), _ptr(db), _ptr(scratch), _stream()) == ERR_ARG, (N, K, M)
    torch.cuda.synchronize()
    assert bool((dW == -7.0).all()) and bool((db == -7.0).all())
