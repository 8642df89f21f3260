"""GPU: the sample-parallel training step -- `genie_adam_step` alone (rank-ordered gradient sum, Adam against an fp64 restatement with
torch's own fp32 CPU Adam as the yardstick, refusals) and `train.FlatParams` / `FlatAdam` / `train_step_parallel` on the shapes of
test_training_loss_curve_matches_oracle_adam (7 stations x 45 source nodes, 90 picks, 20 queries) with a batch of six samples: world 1
against `train.train_step`, the ranks' parts, the merged step, a 20-step curve, process groups, a checkpoint."""
import datetime
import functools
import os
import time

import numpy as np
import pytest
import torch

from genie_amd import _lib, apply, module, synthetic, train
from genie_amd.engine import _ptr, _stream
from tests.test_source_parallel_gpu import _free_port
from tests.test_train_gpu import _inputs
from tests.util import Case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDENT = lambda x: x                                                                        # noqa: E731
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
N_BATCH = 6


# ---- the kernel alone ------------------------------------------------------------------------------------------------------------------

def _adam(p, m, v, n, parts, n_parts, stride, gout, step, lr=LR, betas=BETAS, eps=EPS):
    return _lib.load().genie_adam_step(_ptr(p), _ptr(m), _ptr(v), n, _ptr(parts), n_parts, stride, _ptr(gout), lr, betas[0], betas[1], eps,
                                       step, _stream())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _order_dependent_parts(n_parts, n, rng):
    """[n_parts, n] fp32: N(0, 1) everywhere; in every third element 1e8, -1e8 and 1 sit in three different parts, placed at random
    (fewer parts: what fits), so that the fp32 sum depends on the order of the parts."""
    parts = rng.normal(0, 1, (n_parts, n)).astype(np.float32)
    special = np.array([1e8, -1e8, 1.0], dtype=np.float32)[:n_parts]
    for j in range(0, n, 3):
        rows = rng.permutation(n_parts)[:len(special)]
        parts[rows, j] = special[rng.permutation(len(special))] if n_parts > 1 else special
    return parts


LAYOUTS = {"aligned": (0, 0, False), "odd_stride": (0, 0, True), "offset_state": (1, 0, False), "offset_parts": (0, 1, False),
           "offset_all": (1, 1, True)}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("n_parts", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [1003, 4, 0])
def test_gradient_is_the_rank_ordered_sum(n, n_parts, layout):
    """`grad_out` = ((0 + p0) + p1) + ... as torch adds make it on the device, bit for bit, for every access path of the kernel: 16-byte
    parts and state ("aligned": stride a multiple of 4), 4-byte parts ("odd_stride": an odd stride as the gathered gradient buffers of
    n + 1 floats have it; "offset_parts": the parts start one float past a 16-byte boundary), 4-byte state ("offset_state": p, m, v and
    grad_out start one float past a 16-byte boundary), both ("offset_all")."""
    rng = np.random.default_rng(100 * n_parts + n)
    shift_state, shift_parts, odd = LAYOUTS[layout]
    stride = (n | 1) + 2 if odd else -(-max(n, 1) // 4) * 4
    host = np.zeros((n_parts, stride), dtype=np.float32)
    host[:, :n] = _order_dependent_parts(n_parts, n, rng)
    buf = torch.zeros(n_parts * stride + 4, dtype=torch.float32, device=DEV)
    parts = buf[shift_parts:shift_parts + n_parts * stride].view(n_parts, stride)
    parts.copy_(_dev(host))
    state = torch.zeros((4, -(-(n + 8) // 4) * 4), dtype=torch.float32, device=DEV)
    state[0] = 1.0
    shift = shift_state
    p, m, v, gout = [state[i, shift:shift + n] for i in range(4)]
    if n:
        assert all((t.data_ptr() % 16 == 0) == (shift == 0) for t in (p, m, v, gout))
        assert all((parts[r].data_ptr() % 16 == 0) == ((shift_parts + r * stride) % 4 == 0) for r in range(n_parts))
        assert not odd or shift_parts or n_parts == 1 or parts[1].data_ptr() % 16 != 0           # an aligned base, an odd stride
    want = torch.zeros(n, dtype=torch.float32, device=DEV)
    for r in range(n_parts):
        want = want + parts[r, :n]
    before = state.clone()
    assert _adam(p, m, v, n, parts, n_parts, stride, gout, 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(gout, want)
    if n_parts >= 3 and n >= 4:                     # the data tell the orders apart (two parts cannot: fp32 addition commutes)
        back = torch.zeros(n, dtype=torch.float32, device=DEV)
        for r in reversed(range(n_parts)):
            back = back + parts[r, :n]
        assert not torch.equal(back, want)
    # nothing outside [0, n) of any array was written, p moved by one step of size lr (|g| >> eps), m and v hold the first moments
    mask = torch.ones_like(state, dtype=torch.bool)
    mask[:, shift:shift + n] = False
    assert torch.equal(state[mask], before[mask])
    if n:
        ref_p, ref_m, ref_v = train.adam_reference(np.ones(n), np.zeros(n), np.zeros(n), want.cpu().numpy(), LR, BETAS, EPS, 1)
        assert np.abs(p.cpu().numpy() - ref_p).max() <= 2.0 ** -23
        assert np.allclose(m.cpu().numpy(), ref_m, rtol=1e-6, atol=0) and np.allclose(v.cpu().numpy(), ref_v, rtol=1e-6, atol=0)


def test_threads_stride_past_the_grid_limit():
    """More than 1 024 workgroups x 1 024 floats: threads take a second sweep; three parts, odd n."""
    n, n_parts = 1024 * 1024 + 1027, 3
    g = torch.Generator(device=DEV).manual_seed(5)
    parts = torch.randn((n_parts, n + 1), generator=g, device=DEV)
    p, m, v, gout = [torch.zeros(n, device=DEV) for _ in range(4)]
    assert _adam(p, m, v, n, parts, n_parts, n + 1, gout, 1) == 0
    want = (torch.zeros(n, device=DEV) + parts[0, :n] + parts[1, :n]) + parts[2, :n]
    assert torch.equal(gout, want)
    big = want.abs() > 1e-3                                                                 # |g| >> eps: the first step has size lr
    assert bool((p.abs() < 1.01 * LR).all()) and bool((p.abs()[big] > 0.99 * LR).all()) and bool((p.sign() == -want.sign()).all())


def _torch_cpu_adam(p, m, v, g, step):
    """torch's own fp32 single-tensor Adam on the CPU from the state (m, v, step - 1): the yardstick."""
    param = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([param], lr=LR, betas=BETAS, eps=EPS, foreach=False)
    opt.state[param] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    param.grad = torch.from_numpy(g.copy())
    opt.step()
    st = opt.state[param]
    assert int(st["step"]) == step
    return param.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _ulps(out, ref):
    """Largest |out - ref| in units in the last place of the fp32 value of `ref`."""
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return float((np.abs(out.astype(np.float64) - ref) / ulp).max())


def _adam_inputs(n, step, seed):
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice([-1.0, 1.0], n)                                               # noqa: E731
    g = (10.0 ** rng.uniform(-12, 2, n) * sign()).astype(np.float32)
    g[::7] = 0.0
    p = (10.0 ** rng.uniform(-3, 1, n) * sign()).astype(np.float32)
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = (10.0 ** rng.uniform(-8, 1, n) * sign()).astype(np.float32)
        v = (10.0 ** rng.uniform(-14, 3, n)).astype(np.float32)
        m[::14], v[::14] = 0.0, 0.0                                                         # every other zero gradient meets a zero state
    return p, m, v, g


@pytest.mark.parametrize("n", [1003, 4])
@pytest.mark.parametrize("step", [1, 1000])
def test_adam_update_against_fp64_with_torch_cpu_adam_as_yardstick(n, step):
    """p, m, v after one call against `train.adam_reference` (fp64 on the same fp32 inputs). Per output, the kernel's largest deviation in
    ulps of the output may be at most twice that of torch's fp32 CPU Adam on these inputs, floor 1 ulp.
    Measured (MI355X, n = 1 003; yardstick | kernel): see profiles/EXPERIMENTS.md, "genie_adam_step"."""
    p0, m0, v0, g = _adam_inputs(n, step, seed=step + n)
    ref = train.adam_reference(p0, m0, v0, g, LR, BETAS, EPS, step)
    yard = [_ulps(a, r) for a, r in zip(_torch_cpu_adam(p0, m0, v0, g, step), ref)]
    p, m, v, parts = _dev(p0), _dev(m0), _dev(v0), _dev(g)
    assert _adam(p, m, v, n, parts, 1, 0, None, step) == 0
    got = [t.cpu().numpy() for t in (p, m, v)]
    mine = [_ulps(a, r) for a, r in zip(got, ref)]
    print("genie_adam_step n=%d step=%d: ulps from fp64 (p, m, v): torch CPU fp32 %s | kernel %s"
          % (n, step, ", ".join("%.3g" % y for y in yard), ", ".join("%.3g" % y for y in mine)))
    for name, y, k in zip("pmv", yard, mine):
        assert k <= max(2.0 * y, 1.0), (name, k, y)
    dead = (g == 0) & (m0 == 0) & (v0 == 0)
    assert dead.sum() >= 1
    for a, b in zip(got, (p0, m0, v0)):
        assert a[dead].tobytes() == b[dead].tobytes()
    assert np.abs(got[0] - p0)[~dead].max() > 0


def test_refused_calls_touch_nothing():
    n = 64
    arrays = [torch.full((n,), float(i + 1), device=DEV) for i in range(5)]
    p, m, v, parts, gout = arrays
    before = [a.clone() for a in arrays]
    null = None
    bad = [dict(n=-1), dict(n_parts=0), dict(n_parts=33), dict(step=0), dict(p=null), dict(m=null), dict(v=null), dict(parts=null),
           dict(betas=(1.0, 0.999)), dict(eps=-1.0), dict(lr=float("nan"))]
    for kw in bad:
        a = dict(p=p, m=m, v=v, n=n, parts=parts, n_parts=1, stride=0, gout=gout, step=1, lr=LR, betas=BETAS, eps=EPS)
        a.update(kw)
        assert _adam(**a) == -1, kw
        assert b"genie_adam_step" in _lib.load().genie_last_error()
    torch.cuda.synchronize()
    for a, b in zip(arrays, before):
        assert torch.equal(a, b)
    assert _adam(p, m, v, 0, parts, 1, 0, gout, 1) == 0 and _adam(null, null, null, 0, null, 1, 0, null, 1) == 0        # n = 0: nothing to do
    torch.cuda.synchronize()
    for a, b in zip(arrays, before):
        assert torch.equal(a, b)


# ---- the step --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _setup():
    geom = synthetic.Geometry(7, 45, L=100e3, n_query=20, seed=1)
    samples = [synthetic.training_sample(geom, 90, seed=3, window=k) for k in range(N_BATCH)]
    return geom, [_inputs(geom, smp, DEV) for smp in samples], Case("tiny_6x40").weights


def _model(state=None):
    net = module.GCN_Detection_Network_extended(IDENT, IDENT, device=DEV)
    net.load_state_dict({k: v.clone() for k, v in (state if state is not None else _setup()[2]).items()}, strict=True)
    net.train()
    return net


def _flat_model(state=None):
    net = _model(state)
    return net, train.FlatAdam(train.FlatParams(net), lr=LR)


@functools.lru_cache(maxsize=None)
def _per_sample_parts():
    """The six per-sample gradients (+ loss slot), each divided by the batch-wide count: six one-sample calls with n_valid = 6."""
    net, opt = _flat_model()
    batch = _setup()[1]
    out = []
    for k in range(N_BATCH):
        part, block = train.train_step_parallel(net, opt, [batch[k]], sample_parallel=(0, 1), n_valid=N_BATCH)
        assert block == (0, 1)
        out.append(part)
    assert opt.n_steps == 0
    return out


def _rank_parts(net, opt, world):
    batch = _setup()[1]
    return [train.train_step_parallel(net, opt, batch, sample_parallel=(r, world)) for r in range(world)]


class _NoStep(object):
    """The optimizer `train.train_step` expects, without the step."""

    def __init__(self, net):
        self.net = net

    def zero_grad(self):
        self.net.zero_grad()

    def step(self):
        pass


def test_world_one_accumulates_the_gradient_of_the_plain_step():
    batch = _setup()[1]
    net, opt = _flat_model()
    opt.step = lambda parts=None: None
    loss = train.train_step_parallel(net, opt, batch)
    ref = _model()
    want = train.train_step(ref, _NoStep(ref), batch)
    n_none = 0
    for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        if q.grad is None:
            n_none += 1
            assert not bool(p.grad.any()), k
        else:
            assert torch.equal(p.grad, q.grad), k
    assert 1 <= n_none < 20 and bool(opt.params.grad[:-1].any())
    assert abs(loss - want) <= 6 * 2.0 ** -24 * abs(want) and loss > 0, (loss, want)
    assert loss == float(opt.params.grad[-1])


@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_a_ranks_part_is_the_in_order_sum_of_its_block(world):
    """Catches a loss divided by the block's length: the per-sample gradients are divided by 6."""
    per = _per_sample_parts()
    assert all(bool(g[:-1].any()) and float(g[-1]) > 0 for g in per) and not torch.equal(per[0], per[1])
    net, opt = _flat_model()
    blocks = apply.window_blocks(N_BATCH, world)
    for r, (part, block) in enumerate(_rank_parts(net, opt, world)):
        assert block == blocks[r] and part.shape == per[0].shape
        want = torch.zeros_like(per[0])
        for k in range(*block):
            want = want + per[k]
        assert torch.equal(part, want), (world, r)
        if block[0] == block[1]:
            assert not bool(part.any())
    assert world <= N_BATCH or any(lo == hi for lo, hi in blocks)
    assert opt.n_steps == 0


def test_merged_step_at_world_three():
    """`optimizer.step(parts)` is `genie_adam_step` on the same parts; against the one-GPU flat step the weights differ by no more than
    the Adam tolerance (twice torch's fp32 CPU Adam's distance from fp64 on these inputs, floor 1 ulp, for each of the two results) plus
    what the two gradients' difference explains through the fp64 update. The blocked sum ((0 + P0) + P1) + P2 may be no further from the
    fp64 sum of the six per-sample gradients than twice the sequential sum's distance, each element's distance counted in ulps of its
    largest addend, floor 1."""
    per = _per_sample_parts()
    net, opt = _flat_model()
    n = opt.params.n
    flat0 = opt.params.flat.clone()
    parts = [p for p, _ in _rank_parts(net, opt, 3)]
    opt.step(parts)
    assert opt.n_steps == 1 and not torch.equal(opt.params.flat, flat0)
    # the same parts through the C ABI, from a buffer with an odd stride (4-byte loads; the optimizer gathers into 16-byte aligned rows)
    p, m, v, g_blk = flat0.clone(), torch.zeros_like(flat0), torch.zeros_like(flat0), torch.zeros_like(flat0)
    stacked = torch.stack(parts)
    assert stacked.stride(0) == n + 1
    assert _adam(p, m, v, n, stacked, 3, n + 1, g_blk, 1) == 0
    assert torch.equal(p, opt.params.flat) and torch.equal(m, opt.exp_avg) and torch.equal(v, opt.exp_avg_sq)
    # one GPU, flat
    net1, opt1 = _flat_model()
    train.train_step_parallel(net1, opt1, _setup()[1])
    g_seq = opt1.params.grad[:n]
    g64 = torch.stack([g[:n].double() for g in per]).sum(0).cpu().numpy()
    addend = torch.stack([g[:n].abs() for g in per]).max(0)[0].cpu().numpy()
    unit = np.spacing(addend).astype(np.float64)
    live = addend > 0
    d_seq = float((np.abs(g_seq.double().cpu().numpy() - g64)[live] / unit[live]).max())
    d_blk = float((np.abs(g_blk.double().cpu().numpy() - g64)[live] / unit[live]).max())
    print("world 3: distance from the fp64 sum of six per-sample gradients, in ulps of the largest addend: sequential %.3g, blocked %.3g"
          % (d_seq, d_blk))
    assert d_blk <= max(2.0 * d_seq, 1.0)
    assert not bool(g_blk[~torch.from_numpy(live).to(DEV)].any())
    zeros = np.zeros(n, np.float32)
    p0 = flat0.cpu().numpy()
    ref_blk = train.adam_reference(p0, zeros, zeros, g_blk.cpu().numpy(), LR, BETAS, EPS, 1)[0]
    ref_seq = train.adam_reference(p0, zeros, zeros, g_seq.cpu().numpy(), LR, BETAS, EPS, 1)[0]
    yard = max(_ulps(_torch_cpu_adam(p0, zeros, zeros, g.cpu().numpy(), 1)[0], ref) for g, ref in ((g_blk, ref_blk), (g_seq, ref_seq)))
    ulp = np.spacing(np.maximum(np.abs(p0), np.abs(ref_seq).astype(np.float32))).astype(np.float64)
    diff = np.abs(opt.params.flat.double().cpu().numpy() - opt1.params.flat.double().cpu().numpy())
    bound = np.abs(ref_blk - ref_seq) + 2.0 * max(2.0 * yard, 1.0) * ulp
    print("world 3 vs one GPU after one step: largest weight difference %.3g (%.3g of its bound), Adam yardstick %.3g ulps"
          % (diff.max(), (diff / bound).max(), yard))
    assert (diff <= bound).all()


def test_twenty_steps_follow_the_plain_curve():
    """World 1 through FlatAdam against `train.train_step` + `make_optimizer`: every loss within 1e-4 relative, the loss falls,
    the trained state_dict loads strictly into a fresh model that computes what the trained one computes. Without
    `mark_weights_changed` every step after the first would run on the weights of step 0 and the curve would stay flat."""
    batch = _setup()[1]
    net, opt = _flat_model()
    ref = _model()
    ref_opt = train.make_optimizer(ref)
    got = [train.train_step_parallel(net, opt, batch) for _ in range(20)]
    want = [train.train_step(ref, ref_opt, batch) for _ in range(20)]
    rel = [abs(a - b) / abs(b) for a, b in zip(got, want)]
    print("flat curve: first %.6g last %.6g (plain %.6g -> %.6g), max relative deviation %.3g" % (got[0], got[-1], want[0], want[-1], max(rel)))
    assert max(rel) <= 1e-4, rel
    assert got[-1] < 0.9 * got[0] and opt.n_steps == 20
    opt.params.check()
    fresh = _model(net.state_dict())
    inputs = batch[0][0]
    outs = []
    for mdl in (net, fresh):
        mdl.eval()
        with torch.no_grad():
            mdl(*inputs)                                        # the fresh model builds its context as the trained one did
            outs.append(mdl.forward_fixed_source(inputs[0], inputs[1], None, None, None, inputs[15], inputs[16], inputs[17], inputs[19]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    start = _model()
    start.eval()
    with torch.no_grad():
        start(*inputs)
        y0 = start.forward_fixed_source(inputs[0], inputs[1], None, None, None, inputs[15], inputs[16], inputs[17], inputs[19])[0]
    assert not torch.equal(y0, outs[0][0])


def test_checkpoint_resumes_with_the_same_bits():
    batch = _setup()[1][:2]
    net, opt = _flat_model()
    for _ in range(2):
        train.train_step_parallel(net, opt, batch)
    net_b, opt_b = _flat_model()
    train.train_step_parallel(net_b, opt_b, batch)
    model_state = {k: v.clone() for k, v in net_b.state_dict().items()}
    opt_state = opt_b.state_dict()
    train.train_step_parallel(net_b, opt_b, batch)              # the saved state is a copy: going on does not change it
    net_c, opt_c = _flat_model(model_state)
    opt_c.load_state_dict(opt_state)
    assert opt_c.n_steps == 1
    loss_c = train.train_step_parallel(net_c, opt_c, batch)
    assert torch.equal(opt_c.params.flat, opt.params.flat) and torch.equal(opt_c.exp_avg, opt.exp_avg) and torch.equal(opt_c.exp_avg_sq, opt.exp_avg_sq)
    assert torch.equal(opt_b.params.flat, opt.params.flat) and loss_c > 0


def _emulated(world, n_steps=2):
    """The group form's result made in this process: the tuple form per rank, then one step with the parts in rank order."""
    net, opt = _flat_model()
    losses = []
    for _ in range(n_steps):
        parts = [p for p, _ in _rank_parts(net, opt, world)]
        opt.step(parts)
        total = np.float32(0.0)
        for p in parts:
            total = np.float32(total + np.float32(p[-1].item()))
        losses.append(float(total))
    return opt.params.flat.cpu().numpy(), losses


def _worker(rank, world, port, backend, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(DEV)
    timeout = datetime.timedelta(seconds=60)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(DEV), timeout=timeout)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timeout)
    try:
        net, opt = _flat_model()
        losses = [train.train_step_parallel(net, opt, _setup()[1], sample_parallel=True) for _ in range(2)]
        torch.cuda.synchronize()
        ret[rank] = (opt.params.flat.cpu().numpy(), losses, dist.get_backend())
    finally:
        dist.destroy_process_group()


def _run_group(world, backend, limit=240.0):
    import torch.multiprocessing as mp
    want_flat, want_losses = _emulated(world)
    mgr = mp.Manager()
    ret = mgr.dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), backend, ret), nprocs=world, join=False)
    deadline = time.monotonic() + limit
    try:
        while not ctx.join(timeout=5.0):                  # returns as soon as a rank ends; raises what a rank raised
            assert time.monotonic() < deadline, "a rank of the %s group of %d is stuck" % (backend, world)
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join(10.0)
    assert len(ret) == world
    for rank in range(world):
        flat, losses, be = ret[rank]
        assert be == backend
        assert flat.tobytes() == want_flat.tobytes(), rank
        assert losses == want_losses, (rank, losses, want_losses)
    assert want_losses[1] < want_losses[0]


def test_two_processes_on_one_gpu_over_gloo():
    _run_group(2, "gloo")


def test_three_processes_on_one_gpu_over_gloo():
    _run_group(3, "gloo")


def test_world1_rccl_gathers_on_the_device():
    _run_group(1, "nccl")


def test_sample_parallel_on_a_sharded_model_is_refused():
    net = module.GCN_Detection_Network_extended(IDENT, IDENT, device=DEV, shard=(0, 2))
    assert net.is_sharded
    opt = train.FlatAdam(train.FlatParams(net))
    with pytest.raises(NotImplementedError, match="sample_parallel"):
        train.train_step_parallel(net, opt, _setup()[1], sample_parallel=(0, 2))
    assert opt.n_steps == 0
