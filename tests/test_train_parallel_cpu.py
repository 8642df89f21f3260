"""CPU: the host side of the sample-parallel training step (genie_amd/train.py: FlatParams, train_step_parallel's block logic,
adam_reference) and the declaration of its kernel. Nothing here needs a GPU or the built library."""
import os
import re

import numpy as np
import pytest
import torch

from genie_amd import _lib, apply, module, train

IDENT = lambda x: x                                                                        # noqa: E731


@pytest.mark.parametrize("options", [{}, {"use_updated_model_definition": True}, {"use_absolute_pos": True},
                                     {"use_updated_model_definition": True, "use_absolute_pos": True}])
def test_flat_params_rehome_every_parameter_as_a_view(options):
    torch.manual_seed(1)
    net = module.GCN_Detection_Network_extended(IDENT, IDENT, device="cpu", **options)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    fp = train.FlatParams(net)
    assert fp.flat.dtype == torch.float32 and fp.flat.dim() == 1 and fp.grad.numel() == fp.flat.numel() + 1
    assert fp.names == [k for k, _ in net.named_parameters()]
    end = 0
    for (name, p), off, numel in zip(net.named_parameters(), fp.offsets, fp.numels):
        assert off % 4 == 0 and off >= end, name                                            # 16-byte aligned, no overlap
        assert numel == p.numel() and p.is_contiguous()
        assert p.data_ptr() == fp.flat.data_ptr() + 4 * off, name
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.data_ptr() == fp.grad.data_ptr() + 4 * off, name
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        end = off + numel
    assert end <= fp.n == fp.flat.numel() and fp.n % 4 == 0 and fp.n - end < 4
    assert sum(fp.numels) == sum(v.numel() for v in before.values())
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    # writes through the buffers are writes to the parameters; a strict load is an in-place copy and keeps the views
    other = {k: torch.randn_like(v) for k, v in before.items()}
    net.load_state_dict(other, strict=True)
    fp.check()
    for (name, p), off, numel in zip(net.named_parameters(), fp.offsets, fp.numels):
        assert torch.equal(fp.flat[off:off + numel].view(p.shape), other[name]), name
    fp.grad.fill_(3.0)
    assert all(bool((p.grad == 3.0).all()) for p in net.parameters())
    fp.zero_grad()
    assert all(bool((p.grad == 0.0).all()) for p in net.parameters()) and float(fp.grad.abs().sum()) == 0.0
    # autograd accumulates in place into the views
    (net.SpatialDirect.f_direct.weight.sum() * 2.0).backward()
    (net.SpatialDirect.f_direct.weight.sum() * 0.5).backward()
    fp.check()
    k = fp.names.index("SpatialDirect.f_direct.weight")
    off, numel = fp.offsets[k], fp.numels[k]
    assert bool((fp.grad[off:off + numel] == 2.5).all()) and float(fp.grad.sum()) == 2.5 * numel
    # what breaks a view is found
    net.zero_grad()
    with pytest.raises(RuntimeError, match="no longer lives in the flat buffer"):
        fp.check()


def test_flat_adam_has_no_cpu_fallback_and_carries_its_state():
    net = torch.nn.Linear(3, 2)
    opt = train.FlatAdam(train.FlatParams(net), lr=2e-3)
    with pytest.raises(_lib.GenieHipError, match="no CPU fallback"):
        opt.step()
    opt.exp_avg.fill_(1.0)
    opt.exp_avg_sq.fill_(2.0)
    opt.n_steps = 7
    sd = opt.state_dict()
    opt.exp_avg.zero_()                                                                     # the state dict holds copies
    other = train.FlatAdam(train.FlatParams(torch.nn.Linear(3, 2)))
    other.load_state_dict(sd)
    assert other.n_steps == 7 and other.lr == 2e-3 and bool((other.exp_avg == 1.0).all()) and bool((other.exp_avg_sq == 2.0).all())
    with pytest.raises(ValueError):
        train.FlatAdam(train.FlatParams(torch.nn.Linear(7, 2))).load_state_dict(sd)


class _StubNet(torch.nn.Module):
    """`forward(i)` = w * i: with the stub loss `out / n` the gradient of sample i is `i * (1 / n)`."""
    is_sharded = False

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))

    def _contexts(self):
        return ()

    def forward(self, i):
        return (self.w * i).sum()


@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
def test_blocks_partition_the_batch_and_every_rank_divides_by_the_batch(world, monkeypatch):
    n = 6
    divisors = []

    def stub_loss(out, labels, n_valid):
        divisors.append(n_valid)
        return out / n_valid

    monkeypatch.setattr(train, "reference_loss", stub_loss)
    net = _StubNet()
    opt = train.FlatAdam(train.FlatParams(net))
    batch = [((torch.tensor(float(i + 1)),), None) for i in range(n)]                       # sample i carries the index i + 1
    inv = torch.ones(1) / n
    seen, blocks = [], apply.window_blocks(n, world)
    for rank in range(world):
        part, block = train.train_step_parallel(net, opt, batch, sample_parallel=(rank, world))
        assert block == blocks[rank] and part.shape == (opt.params.n + 1,) and part.data_ptr() != opt.params.grad.data_ptr()
        want_g, want_l = torch.zeros(1), torch.zeros(1)
        for i in range(*block):
            want_g = want_g + inv * float(i + 1)                                            # in sample order, divided by 6, not by the block
            want_l = want_l + torch.tensor([float(i + 1)]) / n
        assert torch.equal(part[0:1], want_g) and torch.equal(part[-1:], want_l), (rank, part, want_g)
        assert float(part[1:-1].abs().sum()) == 0.0                                         # the padding stays zero
        seen += list(range(*block))
        # the same samples handed over as the rank's own, with the batch-wide count
        own, own_block = train.train_step_parallel(net, opt, batch[block[0]:block[1]], sample_parallel=(rank, world), n_valid=n)
        assert torch.equal(own, part) and own_block == (0, block[1] - block[0])
    assert seen == list(range(n)) and divisors == [n] * (2 * n)
    assert opt.n_steps == 0 and float(net.w.detach()) == 1.0                                       # the tuple form takes no step
    if world > n:
        assert any(lo == hi for lo, hi in blocks)
    with pytest.raises(ValueError, match="n_valid"):
        train.train_step_parallel(net, opt, batch, sample_parallel=(0, world), n_valid=n - 1)


def test_a_sharded_model_and_a_foreign_optimizer_are_refused():
    net = _StubNet()
    opt = train.FlatAdam(train.FlatParams(net))
    net.is_sharded = True
    with pytest.raises(NotImplementedError, match="sample_parallel"):
        train.train_step_parallel(net, opt, [], sample_parallel=(0, 2))
    with pytest.raises(ValueError, match="another model"):
        train.train_step_parallel(_StubNet(), opt, [], sample_parallel=(0, 2))


def test_adam_kernel_is_declared_and_bound():
    names = [s[0] for s in _lib.SYMBOLS]
    assert names.count("genie_adam_step") == 1
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    assert re.search(r"^int genie_adam_step\(float\* param, float\* exp_avg, float\* exp_avg_sq, int64_t n,", header, re.M)
    _, res, args = _lib.SYMBOLS[names.index("genie_adam_step")]
    assert len(args) == 14 and args[8:12] == [_lib._c.c_double] * 4 and args[3] == args[6] == args[12] == _lib._c.c_int64


def test_adam_reference_restates_torch_adam():
    """`train.adam_reference` (numpy fp64) against `torch.optim.Adam(foreach=False)` on CPU fp32, 3 steps from a zero state. Bounds from
    the fp32 format alone (u = 2^-24, inputs |g| <= G = max|g|): torch's `m` and `v` pass through three roundings per step (difference,
    product, sum) of values no larger than G resp. G^2 and carry the earlier steps' errors damped by beta < 1: <= 3 steps x 3 u x G
    (G^2). `p` takes one rounding of at most u |p| per step, plus an update lr * m_hat / (sqrt(v_hat) + eps) of magnitude <= 2 lr here
    (|m_hat| / sqrt(v_hat) <= 1 / sqrt(1 - beta2) in general, below 2 for three steps of this data -- asserted) whose own relative
    error (two divisions, a root, an add, a product on inputs already off by the bounds above) stays below 64 u."""
    rng = np.random.default_rng(11)
    n, lr, betas, eps = 4099, 1e-3, (0.9, 0.999), 1e-8
    p0 = rng.normal(0, 1, n).astype(np.float32)
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([param], lr=lr, betas=betas, eps=eps, foreach=False)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    u = 2.0 ** -24
    for step in (1, 2, 3):
        g = rng.normal(0, 1, n).astype(np.float32)
        g[::97] = 0.0
        param.grad = torch.from_numpy(g.copy())
        opt.step()
        p_old = p
        p, m, v = train.adam_reference(p, m, v, g, lr, betas, eps, step)
        assert np.abs(p - p_old).max() <= 2.0 * lr
        gmax = float(np.abs(g).max())
        st = opt.state[param]
        assert int(st["step"]) == step
        assert np.abs(st["exp_avg"].numpy() - m).max() <= step * 3 * u * gmax
        assert np.abs(st["exp_avg_sq"].numpy() - v).max() <= step * 3 * u * gmax ** 2
        assert (np.abs(param.detach().numpy() - p) <= step * (u * np.abs(p) + 2.0 * lr * 64 * u)).all()
    assert np.abs(p - p0).max() > lr                                                        # it moved
