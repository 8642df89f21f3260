"""GPU: the refined-source selection kernel (genie_refine_select through `postproc.refine_select_device`) against the torch statements
of `apply.refine_sources` it replaces, evaluated on the same device tensors: `acc += x / n_scale` per leg, `where(keep, acc, -inf)`,
`argmax` of the row maxima, `argmax` of that row. Everything is compared exactly: indices, the value's bits, the any-kept flag.

Launch geometry the shapes are chosen from (csrc/select_kernels.hpp): 256 threads (4 waves) per workgroup, a workgroup spans 2 048
elements of [Q, n_t], at most 1 024 workgroups, beyond which every thread strides."""
import ctypes

import pytest
import torch

from genie_amd import _lib, postproc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SPAN = 2048


def _reference(xs, shape, keep, n_scale):
    """The statements of refine_sources (device branch before the kernel): (ip, it, value fp32 tensor, any_kept)."""
    acc = torch.zeros(shape, dtype=torch.float32, device=DEV)
    for x in xs:
        acc += x.view(shape[0], shape[1], 1)[:, :, 0] / n_scale
    if keep is None:
        keep = torch.ones(shape[0], dtype=torch.bool, device=DEV)
    ninf = torch.full((), float("-inf"), dtype=torch.float32, device=DEV)
    accm = torch.where(keep.view(-1, 1), acc, ninf)
    ip = torch.argmax(accm.max(1)[0]).view(1)
    row = accm.index_select(0, ip)[0]
    it = torch.argmax(row).view(1)
    return int(ip), int(it), row.index_select(0, it), bool(keep.any())


def _same(got, want):
    ip, it, value, any_kept = want
    g = got.cpu()
    assert (int(g[0]), int(g[1]), bool(g[3])) == (ip, it, any_kept), (g.tolist(), ip, it, float(value), any_kept)
    assert g[3].item() in (0.0, 1.0)
    assert torch.equal(g[2].view(1), value.double().cpu())          # fp32 -> fp64 is exact: the value's bits


def _tied(shape, n_legs, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.floor(torch.rand(shape, device=DEV, generator=g) * 8.0) / 8.0 for _ in range(n_legs)]


@pytest.mark.parametrize("n_legs", [1, 3])
@pytest.mark.parametrize("n_t", [1, 2, 21])
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 257, SPAN + 1, 3 * SPAN + 5])
def test_selection_equals_the_torch_chain_on_tie_rich_data(Q, n_t, n_legs):
    """Multiples of 1/8: the maximum is usually attained in several rows and columns. Q crosses a wave (63 / 64 / 65), a workgroup's
    256 threads (257), a workgroup's span (2 049 at n_t = 1; 257 at n_t = 21) and three workgroups (6 149 at n_t = 1)."""
    xs = _tied((Q, n_t), n_legs, 1000 * Q + 10 * n_t + n_legs)
    g = torch.Generator(device=DEV).manual_seed(Q + n_t)
    keep = torch.rand(Q, device=DEV, generator=g) < 0.8
    keep[Q // 2] = True
    for n_scale in (float(n_legs), 3.0):
        for k in (keep, None):
            got = postproc.refine_select_device(xs, (Q, n_t), k, n_scale)
            _same(got, _reference(xs, (Q, n_t), k, n_scale))


def test_selection_beyond_the_grid_cap_strides():
    """112 000 x 21 = 2.35 M elements > 1 024 workgroups x 2 048: threads stride over the buffer; the read-out shape of the day loop at
    its default cloud, with more offsets."""
    Q, n_t = 112000, 21
    xs = _tied((Q, n_t, 1), 2, 5)
    keep = torch.ones(Q, dtype=torch.bool, device=DEV)
    keep[:1000] = False
    got = postproc.refine_select_device(xs, (Q, n_t), keep, 2.0)
    _same(got, _reference(xs, (Q, n_t), keep, 2.0))
    # a single maximum in the very last element, reached only by the last stride
    x = torch.zeros((Q, n_t), dtype=torch.float32, device=DEV)
    x[Q - 1, n_t - 1] = 0.5
    got = postproc.refine_select_device([x], (Q, n_t), None, 1.0).cpu()
    assert got.tolist() == [Q - 1.0, n_t - 1.0, 0.5, 1.0]


@pytest.mark.parametrize("Q,n_t", [(65, 2), (257, 21), (3 * SPAN + 5, 1), (700, 9)])
def test_planted_ties_the_early_row_and_its_first_column_win(Q, n_t):
    x = _tied((Q, n_t), 1, 3)[0] * 0.5                   # below the planted 0.75
    early, late = Q // 5, Q - 2
    x[early, n_t - 1] = 0.75                             # the last column of an early row ...
    x[late, 0] = 0.75                                    # ... and the first column of a later row
    got = postproc.refine_select_device([x], (Q, n_t), None, 1.0)
    _same(got, _reference([x], (Q, n_t), None, 1.0))
    assert got.cpu().tolist() == [float(early), float(n_t - 1), 0.75, 1.0]
    if n_t > 2:
        x[early, 1] = 0.75                               # twice in the winning row: its first column
        got = postproc.refine_select_device([x], (Q, n_t), None, 1.0)
        _same(got, _reference([x], (Q, n_t), None, 1.0))
        assert got.cpu().tolist() == [float(early), 1.0, 0.75, 1.0]


@pytest.mark.parametrize("Q,n_t,K", [(65, 2, 10), (257, 21, 100), (3 * SPAN + 5, 1, SPAN + 3)])
def test_masked_rows_do_not_take_part(Q, n_t, K):
    xs = _tied((Q, n_t), 3, 9)
    xs[1][K // 2, n_t - 1] = 5.0                         # the global maximum sits in a dropped row
    keep = torch.ones(Q, dtype=torch.bool, device=DEV)
    keep[:K] = False
    got = postproc.refine_select_device(xs, (Q, n_t), keep, 3.0)
    want = _reference(xs, (Q, n_t), keep, 3.0)
    _same(got, want)
    assert want[0] >= K and int(_reference(xs, (Q, n_t), None, 3.0)[0]) == K // 2
    # keep = NULL is an all-ones mask (bool and uint8 masks are the same bytes)
    ones = torch.ones(Q, dtype=torch.uint8, device=DEV)
    assert torch.equal(postproc.refine_select_device(xs, (Q, n_t), None, 3.0), postproc.refine_select_device(xs, (Q, n_t), ones, 3.0))
    # every row dropped
    none = postproc.refine_select_device(xs, (Q, n_t), torch.zeros(Q, dtype=torch.bool, device=DEV), 3.0).cpu()
    assert none[3].item() == 0.0 and none[0].item() == 0.0 and none[1].item() == 0.0 and none[2].item() == float("-inf")


@pytest.mark.parametrize("n_t", [1, 21])
def test_no_query_at_all(n_t):
    got = postproc.refine_select_device([], (0, n_t), None, 1.0, device=DEV).cpu()
    assert got[3].item() == 0.0
    x = torch.zeros((0, n_t), dtype=torch.float32, device=DEV)
    got = postproc.refine_select_device([x], (0, n_t), torch.zeros(0, dtype=torch.bool, device=DEV), 1.0).cpu()
    assert got[3].item() == 0.0


@pytest.mark.parametrize("Q,n_t", [(1, 1), (65, 2), (3 * SPAN + 5, 9)])
def test_no_leg_produced_a_window(Q, n_t):
    """n_used = 0: an all-zero acc, whose first kept row and first column win, as in torch."""
    keep = torch.ones(Q, dtype=torch.bool, device=DEV)
    keep[: Q // 3] = False
    got = postproc.refine_select_device([], (Q, n_t), keep, 3.0)
    _same(got, _reference([], (Q, n_t), keep, 3.0))
    assert got.cpu().tolist() == [float(Q // 3), 0.0, 0.0, 1.0]
    assert postproc.refine_select_device([], (Q, n_t), None, 3.0, device=DEV).cpu().tolist() == [0.0, 0.0, 0.0, 1.0]


def test_three_legs_divided_by_three_carry_the_bits_of_the_torch_sum():
    """Untied random data: the per-leg scaling (torch's `x / 3.0` with a host scalar) and the order of the additions decide the last bit
    of the value, and which near-equal element wins."""
    Q, n_t = 5000, 9
    g = torch.Generator(device=DEV).manual_seed(21)
    xs = [torch.rand((Q, n_t, 1), device=DEV, generator=g) for _ in range(3)]
    want = _reference(xs, (Q, n_t), None, 3.0)
    _same(postproc.refine_select_device(xs, (Q, n_t), None, 3.0), want)
    # the test can tell the orders and the scalings apart: on this data they differ somewhere
    a = (xs[0][:, :, 0] / 3.0 + xs[1][:, :, 0] / 3.0) + xs[2][:, :, 0] / 3.0
    b = (xs[2][:, :, 0] / 3.0 + xs[1][:, :, 0] / 3.0) + xs[0][:, :, 0] / 3.0
    c = (xs[0][:, :, 0] + xs[1][:, :, 0] + xs[2][:, :, 0]) / 3.0
    assert not torch.equal(a, b) and not torch.equal(a, c)
    # every element in turn made the winner by masking all others: the value's bits of 64 sampled elements
    for q in range(0, Q, 79):
        keep = torch.zeros(Q, dtype=torch.bool, device=DEV)
        keep[q] = True
        _same(postproc.refine_select_device(xs, (Q, n_t), keep, 3.0), _reference(xs, (Q, n_t), keep, 3.0))


def test_same_call_twice_gives_equal_bits():
    Q, n_t = 3 * SPAN + 5, 21
    xs = _tied((Q, n_t), 3, 17)
    keep = torch.rand(Q, device=DEV) < 0.5
    scratch = postproc.refine_select_scratch(DEV)
    a = postproc.refine_select_device(xs, (Q, n_t), keep, 3.0, scratch=scratch)
    scratch.fill_(255)                                   # the scratch's contents do not matter
    b = postproc.refine_select_device(xs, (Q, n_t), keep, 3.0, scratch=scratch)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_refine_select_rejects_bad_arguments():
    lib = _lib.load()
    Q, n_t = 8, 3
    x = torch.ones((Q, n_t), dtype=torch.float32, device=DEV)
    out = torch.full((4,), 7.0, dtype=torch.float64, device=DEV)
    scratch = postproc.refine_select_scratch(DEV)
    ptrs = (ctypes.c_void_p * 1)(x.data_ptr())
    null = (ctypes.c_void_p * 1)(None)
    o, s = out.data_ptr(), scratch.data_ptr()
    for args in ((ptrs, -1, Q, n_t, None, 1.0, s, o), (ptrs, 33, Q, n_t, None, 1.0, s, o), (ptrs, 1, -1, n_t, None, 1.0, s, o),
                 (ptrs, 1, Q, 0, None, 1.0, s, o), (ptrs, 1, Q, -2, None, 1.0, s, o), (ptrs, 1, Q, n_t, None, 0.0, s, o),
                 (ptrs, 1, Q, n_t, None, -1.0, s, o), (ptrs, 1, Q, n_t, None, float("inf"), s, o), (None, 1, Q, n_t, None, 1.0, s, o),
                 (null, 1, Q, n_t, None, 1.0, s, o), (ptrs, 1, Q, n_t, None, 1.0, None, o), (ptrs, 1, Q, n_t, None, 1.0, s, None)):
        assert lib.genie_refine_select(*args, None) == -1                  # GENIE_ERR_ARG
        assert b"genie_refine_select" in lib.genie_last_error()
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [7.0] * 4                                 # refused before any launch
    with pytest.raises(ValueError):
        postproc.refine_select_device([x[:, :2]], (Q, 2), None, 1.0)       # not contiguous
    with pytest.raises(ValueError):
        postproc.refine_select_device([x], (Q, n_t), torch.ones(Q + 1, dtype=torch.bool, device=DEV), 1.0)
    with pytest.raises(ValueError):
        postproc.refine_select_device([x] * 33, (Q, n_t), None, 1.0)
