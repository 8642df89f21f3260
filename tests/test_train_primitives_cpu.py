"""CPU: the references that tests/test_train_primitives_gpu.py holds the stand-alone training primitives of the C ABI against
(tests/restatements.py) are themselves pinned here: the dense fp64 adjoint of the neighbour means to fp64 autograd of the
index-gather formulation, the sequential fp32 segment sum of genie_seg_rows to an fp64 index_add_, and the hand-made graphs to the
properties the GPU tests rely on."""
import numpy as np
import torch

from genie_amd import engine, graph
from tests import restatements as R

S, G = R.HANDMADE_S, R.HANDMADE_G


def test_handmade_graphs_have_the_degrees_the_gpu_tests_rely_on():
    """Both sides of the 8-edge chunk as in-degrees, a node that is nobody's neighbour, a reversed out-degree >= 17, a self-loop and
    a neighbour listed twice, which `csr_from_edges` keeps (it sorts the edges by target and drops nothing)."""
    A_sta, A_src = R.handmade_graphs()
    for A, n, degrees, hub, lonely in ((A_sta, S, R.HANDMADE_STA_DEG, 8, 19), (A_src, G, R.HANDMADE_SRC_DEG, 10, 23)):
        indeg = torch.bincount(A[1], minlength=n).tolist()
        assert indeg == degrees and set((0, 1, 7, 8, 9, 15, 16, 17)) <= set(indeg)
        outdeg = torch.bincount(A[0], minlength=n)
        assert int(outdeg[lonely]) == 0 and int(outdeg[hub]) >= 17
        assert int((A[0] == A[1]).sum()) == 1                                     # the self-loop
        rowptr, col = engine.csr_from_edges(A, n)
        assert rowptr.tolist() == np.concatenate(([0], np.cumsum(degrees))).tolist() and col.numel() == A.shape[1]
        twice = [i for i in range(n) if len(set(col[rowptr[i]:rowptr[i + 1]].tolist())) < indeg[i]]
        assert twice == [4]                                                       # the duplicate survives the CSR builder
        Am, ind, od = R.mean_adjacency(A, n)
        assert torch.equal(od, outdeg) and ind.tolist() == indeg
        assert torch.equal(R.mean_adjacency(A, n, sparse=True)[0].to_dense(), Am)
        rows = Am.sum(1)
        assert all(abs(float(rows[i]) - (1.0 if indeg[i] else 0.0)) <= 1e-15 for i in range(n))
        assert float(Am[:, lonely].abs().max()) == 0.0
    ring = R.power_of_two_ring(S)
    assert torch.bincount(ring[1], minlength=S).tolist() == [1 << (i % 4) for i in range(S)]


def test_dense_adjoint_equals_fp64_autograd_of_the_gather_formulation():
    """d/dx of <mean(x), g> by autograd through the index-gather mean equals the dense adjoint A^T g, and the dense forward equals
    the gather mean, on the hand-made (ragged, self-loop, duplicate) graphs; on a uniform-degree graph the gather mean is the
    neighbour-table formulation of `_mean_over_sta` / `_mean_over_src`."""
    A_sta, A_src = R.handmade_graphs()
    Am_sta, Am_src = R.mean_adjacency(A_sta, S)[0], R.mean_adjacency(A_src, G)[0]
    gen = torch.Generator().manual_seed(5)
    C = 7
    x1 = torch.randn((G, S, C), dtype=torch.float64, generator=gen, requires_grad=True)
    x2 = torch.randn((G, S, C), dtype=torch.float64, generator=gen, requires_grad=True)
    g1 = torch.randn((G * S, C), dtype=torch.float64, generator=gen)
    g2 = torch.randn((G * S, C), dtype=torch.float64, generator=gen)
    m1, m2 = R.gather_mean_rows(x1, A_sta, S, 1), R.gather_mean_rows(x2, A_src, G, 0)
    o1, o2 = R.nbr_mean_ref(Am_sta, Am_src, x1.detach().reshape(G * S, C), x2.detach().reshape(G * S, C), S, G)
    assert torch.allclose(m1.detach().reshape(G * S, C), o1, rtol=0, atol=1e-13)
    assert torch.allclose(m2.detach().reshape(G * S, C), o2, rtol=0, atol=1e-13)
    ((m1.reshape(G * S, C) * g1).sum() + (m2.reshape(G * S, C) * g2).sum()).backward()
    d1, d2 = R.nbr_mean_adjoint_ref(Am_sta, Am_src, g1, g2, S, G)
    assert torch.allclose(x1.grad.reshape(G * S, C), d1, rtol=0, atol=1e-13)
    assert torch.allclose(x2.grad.reshape(G * S, C), d2, rtol=0, atol=1e-13)
    assert float(d1.view(G, S, C)[:, 19].abs().max()) == 0.0 and float(d2.view(G, S, C)[23].abs().max()) == 0.0
    # one gradient alone, and the sparse form of the matrices (the large GPU case uses it)
    only1, none = R.nbr_mean_adjoint_ref(Am_sta, Am_src, g1, None, S, G)
    assert none is None and torch.equal(only1, d1)
    sp1, sp2 = R.nbr_mean_adjoint_ref(R.mean_adjacency(A_sta, S, sparse=True)[0], R.mean_adjacency(A_src, G, sparse=True)[0], g1, g2, S, G)
    assert torch.allclose(sp1, d1, rtol=0, atol=1e-13) and torch.allclose(sp2, d2, rtol=0, atol=1e-13)
    # uniform degrees: the neighbour-table restatements
    ring = torch.tensor([((i + 1 + k) % S, i) for i in range(S) for k in range(3)], dtype=torch.long).t()
    x = x1.detach().reshape(G * S, C)
    t = R._mean_over_sta(x, graph.neighbour_table(ring, S).long(), S, G)
    assert torch.allclose(t, R.gather_mean_rows(x.view(G, S, C), ring, S, 1).reshape(G * S, C), rtol=0, atol=1e-13)
    ring_g = torch.tensor([((i + 1 + k) % G, i) for i in range(G) for k in range(3)], dtype=torch.long).t()
    t = R._mean_over_src(x, graph.neighbour_table(ring_g, G).long(), S, G)
    assert torch.allclose(t, R.gather_mean_rows(x.view(G, S, C), ring_g, G, 0).reshape(G * S, C), rtol=0, atol=1e-13)


def test_adjoint_bound_is_the_out_degree_times_the_absolute_sum():
    """The bound helper on a case small enough to write down: node j with out-degree n and terms t_i gets (n + 2) 2^-24 sum |t_i|."""
    A = torch.tensor([[0, 0, 1], [1, 2, 2]])                                    # 0 -> 1, 0 -> 2, 1 -> 2: in-degrees 0, 1, 2
    Am, ind, od = R.mean_adjacency(A, 3)
    assert ind.tolist() == [0, 1, 2] and od.tolist() == [2, 1, 0] and Am.tolist() == [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 0.5, 0.0]]
    g = torch.tensor([[3.0], [-5.0], [8.0]])
    one = R.mean_adjacency(torch.zeros((2, 0), dtype=torch.long), 1)
    b, _ = R.nbr_mean_adjoint_bound(Am, one[0], od, one[2], g, None, 3, 1)
    assert b.view(-1).tolist() == [4 * R.U32 * 9.0, 3 * R.U32 * 4.0, 0.0]
    f, _ = R.nbr_mean_bound(Am, one[0], ind, one[1], g, None, 3, 1)           # means 0, 3, (3 - 5) / 2: in-degrees 0, 1, 2
    assert f.view(-1).tolist() == [0.0, 3 * R.U32 * 3.0, 4 * R.U32 * 4.0]


def test_sequential_segment_sum_equals_fp64_index_add():
    """`seg_rows_sequential` (fp32, the kernel's order) against an fp64 index_add_ of the kept edges: every element within
    (run length + 1) 2^-24 (|d_s| + sum |terms|), the first-order bound of run-length additions in fp32 (one per edge from the second
    on, one into d_s); rows no edge points at are bit-unchanged, and columns 30, 31 of the edge rows are never read."""
    rng = np.random.default_rng(9)
    P, n = 37, 700
    etgt = rng.integers(-1, P - 1, n).astype(np.int32)                           # -1 = dropped; row P - 1 is no target
    etgt[100:140] = 5
    erow = rng.normal(0, 1, (n, 32)).astype(np.float32)
    erow[:, 30:] = 1e30
    ds0 = rng.normal(0, 1, (P, 30)).astype(np.float32)
    order = torch.sort(torch.from_numpy(etgt), stable=True)[1].to(torch.int32).numpy()
    got = R.seg_rows_sequential(erow, etgt, order, ds0)
    assert got.dtype == np.float32 and np.isfinite(got).all()
    keep = torch.from_numpy(etgt >= 0)
    idx = torch.from_numpy(etgt).long()[keep]
    terms = torch.from_numpy(erow[:, :30]).double()[keep]
    ref = torch.from_numpy(ds0).double().index_add_(0, idx, terms)
    mag = torch.from_numpy(ds0).double().abs().index_add_(0, idx, terms.abs())
    runs = torch.bincount(idx, minlength=P).double()
    assert int(runs[5]) >= 40
    bound = (runs + 1).view(P, 1) * R.U32 * mag
    assert bool(((torch.from_numpy(got).double() - ref).abs() <= bound).all())
    untouched = (runs == 0).numpy()
    assert untouched[P - 1] and np.array_equal(got[untouched], ds0[untouched])
    # no edge, and dropped edges only: d_s comes back as it was
    assert np.array_equal(R.seg_rows_sequential(erow[:0], etgt[:0], order[:0], ds0), ds0)
    drop = np.full(3, -1, dtype=np.int32)
    assert np.array_equal(R.seg_rows_sequential(erow[:3], drop, np.arange(3, dtype=np.int32), ds0), ds0)
