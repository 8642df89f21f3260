"""Training step around `GCN_Detection_Network_extended.forward` -- the second caller of the hot path
(`/root/reference/Code/train_GENIE_model.py:1716-1861`).

Kept from the reference: the call `out = mz(*input_tensors)` with the 22 positional tensors (`:1770-1786`), the 4-term
weighted MSE `0.1 MSE(y) + 0.4 MSE(x) + 0.25 MSE(arv_p) + 0.25 MSE(arv_s)` divided by the number of valid samples of the batch
(`:1392, :1789`), `loss.backward()` per sample (`:1843-1846`) and ONE `optimizer.step()` per batch (`:1861`; Adam, lr 1e-3,
`:1383`). Not kept: the synthetic-event generator, label construction and plotting around it (out of scope).

`train_step` is that loop on one GPU around `torch.optim.Adam`. `FlatParams` + `FlatAdam` + `train_step_parallel` are the same step with
the parameters and their gradients in one flat buffer each and the optimizer in one HIP launch (`genie_adam_step`), which lets the
batch's samples split over the GPUs of a node (`sample_parallel=`, the forms of `window_parallel` / `source_parallel`): every rank
runs its block of the samples, ONE all-gather moves the ranks' gradient parts, and every rank sums them in rank order inside the
optimizer's launch -- the weights depend on (batch, world) alone, never on a collective's reduction schedule.
"""
import numpy as np
import torch

from . import _lib

LOSS_WEIGHTS = (0.1, 0.4, 0.25, 0.25)          # train_GENIE_model.py:1392


def reference_loss(out, labels, n_valid_samples=1):
    """`(w0 MSE(out[0][:,:,0], Lbls) + w1 MSE(out[1][:,:,0], Lbls_query) + w2 MSE(out[2][:,:,0], pick_lbls[:,:,0]) +
    w3 MSE(out[3][:,:,0], pick_lbls[:,:,1])) / n_valid_samples` (train_GENIE_model.py:1789). `labels` = (Lbls [G, T],
    Lbls_query [Q, T], pick_lbls [n_src, n_picks, 2])."""
    mse = torch.nn.functional.mse_loss
    lbl, lbl_q, pick = labels
    w = LOSS_WEIGHTS
    return (w[0] * mse(out[0][:, :, 0], lbl) + w[1] * mse(out[1][:, :, 0], lbl_q) + w[2] * mse(out[2][:, :, 0], pick[:, :, 0])
            + w[3] * mse(out[3][:, :, 0], pick[:, :, 1])) / n_valid_samples


def make_optimizer(net):
    return torch.optim.Adam(net.parameters(), lr=0.001)      # train_GENIE_model.py:1383


def train_step(net, optimizer, batch):
    """One iteration of the reference's training loop over `batch` = list of (input_tensors [22], labels): zero the gradients,
    forward + loss + backward per sample, one optimizer step. Returns the summed loss value (`losses[i]`, :1862)."""
    optimizer.zero_grad()
    total = 0.0
    n = len(batch)
    for inputs, labels in batch:
        out = net(*inputs)                                    # :1786
        loss = reference_loss(out, labels, n)
        loss.backward()                                       # :1843-1846
        total += float(loss.item())
    optimizer.step()                                          # :1861
    return total


# ---- the flat step: one parameter buffer, one gradient buffer, one optimizer launch, samples split over ranks -------------------------

def adam_reference(p, m, v, g, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, step=1):
    """The update `genie_adam_step` makes, restated in numpy float64 on arrays of any dtype: `torch.optim.Adam`'s defaults (no weight
    decay, no amsgrad, not maximize), `step >= 1` = the step being taken. Returns the new `(p, m, v)` as float64; the yardstick of the
    kernel's tests (tests/test_train_parallel_*.py)."""
    p, m, v, g = [np.asarray(a, dtype=np.float64) for a in (p, m, v, g)]
    b1, b2 = float(betas[0]), float(betas[1])
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (lr / (1.0 - b1 ** int(step))) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** int(step)) + eps)
    return p, m, v


class FlatParams(object):
    """Every parameter of `net` re-homed into ONE fp32 buffer `flat`, every `.grad` into ONE buffer `grad` (same offsets, plus one
    trailing float: the step's loss). Parameter k lives at `[offsets[k], offsets[k] + numel)`, offsets rounded up to 4 floats (16 bytes;
    the padding stays zero). `p.data` and `p.grad` are views, so the model, its `state_dict` (names, shapes, values), a strict
    `load_state_dict` (an in-place copy) and autograd (which accumulates in place into an existing `.grad`) work unchanged, whatever the
    model options; `zero_grad()` is one fill. What breaks the views -- `net.to(...)`, `net.zero_grad()` / `optimizer.zero_grad()` of
    torch (they set `.grad` to None) -- is found by `check()`, which `train_step_parallel` runs every step. Works on CPU tensors too
    (layout only: the optimizer's kernel needs the GPU)."""
    ALIGN = 4

    def __init__(self, net):
        named = list(net.named_parameters())
        if not named:
            raise ValueError("FlatParams: the model has no parameters")
        dev = named[0][1].device
        self.net, self.names, self.offsets, self.numels = net, [], [], []
        off = 0
        for name, p in named:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("FlatParams: parameter %s is %s on %s; every parameter must be float32 on %s" % (name, p.dtype, p.device, dev))
            self.names.append(name)
            self.offsets.append(off)
            self.numels.append(p.numel())
            off += -(-p.numel() // self.ALIGN) * self.ALIGN
        self.n = off
        self.flat = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.n + 1, dtype=torch.float32, device=dev)
        self._params = [p for _, p in named]
        with torch.no_grad():
            for p, o, k in zip(self._params, self.offsets, self.numels):
                view = self.flat[o:o + k].view(p.shape)
                view.copy_(p)
                p.data = view
                p.grad = self.grad[o:o + k].view(p.shape)

    @property
    def loss_slot(self):
        """The trailing float of `grad` (a view [1]): the step's summed loss, accumulated on the device."""
        return self.grad[self.n:]

    def zero_grad(self):
        self.grad.zero_()

    def check(self):
        """Raise when a parameter or its `.grad` is no longer the view this object made."""
        pb, gb = self.flat.data_ptr(), self.grad.data_ptr()
        for name, p, o in zip(self.names, self._params, self.offsets):
            if p.data_ptr() != pb + 4 * o or p.grad is None or p.grad.data_ptr() != gb + 4 * o:
                raise RuntimeError("FlatParams: %s%s no longer lives in the flat buffer (the model was moved, or a torch zero_grad() set the "
                                   "gradients to None); use FlatParams.zero_grad() and rebuild FlatParams after net.to(...)"
                                   % (name, "" if p.data_ptr() == pb + 4 * o else ".data"))


class FlatAdam(object):
    """Adam (torch.optim.Adam's defaults, train_GENIE_model.py:1383) on a `FlatParams`: `exp_avg`, `exp_avg_sq` (flat, zero at the start)
    and `n_steps`. `step(parts)` is ONE launch of `genie_adam_step`: the gradient parts summed in list order, then the update; there is
    no torch fallback."""

    def __init__(self, flat_params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.params = flat_params
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.exp_avg = torch.zeros_like(flat_params.flat)
        self.exp_avg_sq = torch.zeros_like(flat_params.flat)
        self.n_steps = 0
        self._parts = None

    def zero_grad(self):
        self.params.zero_grad()

    def parts_buffer(self, world):
        """[world, L] view (L = len(grad)) of a device buffer kept between steps whose rows are 16-byte aligned: where the ranks' parts
        are gathered, so that the kernel reads every part with 16-byte loads."""
        length = self.params.n + 1
        pitch = -(-length // 4) * 4
        if self._parts is None or self._parts.shape[0] < world:
            self._parts = torch.zeros((world, pitch), dtype=torch.float32, device=self.params.flat.device)
        return self._parts[:world, :length]

    def step(self, parts=None):
        """Take one step with the gradient `((0 + parts[0]) + parts[1]) + ...` (fp32, in that order). `parts`: None = the `grad` buffer
        of the `FlatParams`; a list of 1-D device tensors of at least `n` floats (what the tuple form of `train_step_parallel` returns,
        one per rank, in rank order); or a 2-D tensor [world, >= n] with unit column stride. At most 32 parts. Then the model is told
        that its weights changed (`mark_weights_changed`: the kernel writes through raw pointers)."""
        fp = self.params
        flat = fp.flat
        if not flat.is_cuda:
            raise _lib.GenieHipError("FlatAdam.step needs the parameters on the GPU: the optimizer is a HIP kernel, there is no CPU fallback")
        if parts is None:
            parts = [fp.grad]
        if not torch.is_tensor(parts):
            parts = list(parts)
            if len(parts) == 1:
                parts = parts[0].reshape(1, -1)
            else:
                buf = self.parts_buffer(max(len(parts), 1))
                for r, part in enumerate(parts):
                    buf[r, :part.numel()].copy_(part.reshape(-1))
                parts = buf
        if parts.dim() != 2 or parts.shape[1] < fp.n or parts.stride(1) != 1 or parts.dtype != torch.float32 or parts.device != flat.device:
            raise ValueError("FlatAdam.step: parts must be float32 [world, >= %d] on %s with unit column stride" % (fp.n, flat.device))
        from .engine import _ptr, _stream
        with torch.cuda.device(flat.device):
            _lib.check(_lib.load().genie_adam_step(_ptr(flat), _ptr(self.exp_avg), _ptr(self.exp_avg_sq), fp.n, _ptr(parts), parts.shape[0],
                                                   parts.stride(0), None, self.lr, self.betas[0], self.betas[1], self.eps, self.n_steps + 1,
                                                   _stream()), "genie_adam_step")
        self.n_steps += 1
        mark = getattr(fp.net, "mark_weights_changed", None)
        if mark is not None:
            mark()

    def state_dict(self):
        """What a checkpoint needs (train_GENIE_model.py:1580-1583 saves its optimizer): copies of the two moments and the step count."""
        return {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(), "step": int(self.n_steps),
                "lr": self.lr, "betas": self.betas, "eps": self.eps}

    def load_state_dict(self, state):
        for key in ("exp_avg", "exp_avg_sq"):
            if tuple(state[key].shape) != tuple(self.exp_avg.shape):
                raise ValueError("FlatAdam.load_state_dict: %s has %s elements, this model's flat buffer %d"
                                 % (key, tuple(state[key].shape), self.exp_avg.numel()))
        self.exp_avg.copy_(state["exp_avg"])
        self.exp_avg_sq.copy_(state["exp_avg_sq"])
        self.n_steps = int(state["step"])
        self.lr, self.betas, self.eps = float(state.get("lr", self.lr)), tuple(state.get("betas", self.betas)), float(state.get("eps", self.eps))


def _gather_parts(part, buf, group, timeout):
    """`buf[r]` <- rank r's `part` for every rank of `group`: one all-gather, on the device over RCCL ("nccl"), staged through the host
    over gloo, where the wait ends after `timeout` seconds -- as `apply._merge_partials` / `apply._gather_blocks` choose."""
    import datetime
    import torch.distributed as dist
    if dist.get_backend(group) == "nccl":
        dist.all_gather([buf[r] for r in range(buf.shape[0])], part, group=group)
        return
    h = part.cpu()
    outs = [torch.empty_like(h) for _ in range(buf.shape[0])]
    dist.all_gather(outs, h, group=group, async_op=True).wait(datetime.timedelta(seconds=float(timeout)))
    buf.copy_(torch.stack(outs))


def train_step_parallel(net, optimizer, batch, sample_parallel=None, n_valid=None, merge_timeout=60.0):
    """`train_step` on flat buffers (`optimizer` = a `FlatAdam` on `FlatParams(net)`), the batch's samples split over ranks.

    `sample_parallel`: None | `(rank, world)` | a `torch.distributed` process group | True (the default group), as `window_parallel` /
    `source_parallel`. `n_valid=None`: `batch` is the whole batch and rank r takes the block `apply.window_blocks(len(batch), world)[r]`;
    `n_valid` given: `batch` holds this rank's own samples and `n_valid` is the batch-wide count (ranks that generate only their own
    samples). EVERY sample's loss is divided by the batch-wide count. Per sample: forward, `reference_loss`, `backward()` into the flat
    `grad` (in sample order), the loss added on the device into `grad`'s trailing float; the host reads nothing per sample.

    * None: one part; the step is taken; returns the loss (one read, after the optimizer's launch).
    * tuple form: no collective, no step; returns `(part, (lo, hi))`, `part` = a copy of `grad` (the in-order sum of the block's
      per-sample gradients, then the loss slot; zeros for an empty block). The caller moves the parts and calls
      `optimizer.step([part_0, ..., part_{world-1}])`.
    * group form: one all-gather of the parts (`world x len(grad)` floats; on the device over RCCL, host-staged over gloo with the wait
      bounded by `merge_timeout`), the contexts' verdicts checked, then `optimizer.step(gathered)` on every rank: every rank holds the
      same weights bit for bit, those of the tuple form at the same `world`. Returns the rank-order fp32 sum of the ranks' losses.
    A source-node-sharded model is refused (NotImplementedError)."""
    from . import apply as _apply
    sp = _apply._rank_split(sample_parallel, "sample_parallel", bool(getattr(net, "is_sharded", False)))
    fp = optimizer.params
    if fp.net is not net:
        raise ValueError("train_step_parallel: the optimizer's FlatParams belong to another model")
    fp.check()
    if n_valid is None:
        n = len(batch)
        lo, hi = _apply.window_blocks(n, sp.world)[sp.rank] if sp is not None else (0, n)
        mine = batch[lo:hi]
    else:
        n = int(n_valid)
        if n < len(batch) or n < 1:
            raise ValueError("train_step_parallel: n_valid = %d, but this rank alone holds %d samples" % (n, len(batch)))
        lo, hi = 0, len(batch)
        mine = batch
    fp.zero_grad()
    slot = fp.loss_slot
    for inputs, labels in mine:
        out = net(*inputs)                                    # train_GENIE_model.py:1786
        loss = reference_loss(out, labels, n)                 # the batch-wide count, whatever the block (:1789)
        loss.backward()                                       # accumulates in place into the views of `grad` (:1843-1846)
        slot.add_(loss.detach().reshape(1))
    if sp is None:
        optimizer.step()                                      # :1861
        return float(slot.item())
    if not sp.collective:
        return fp.grad.clone(), (lo, hi)
    buf = optimizer.parts_buffer(sp.world)
    _gather_parts(fp.grad, buf, sp.group, merge_timeout)
    _apply._check_verdicts(net)                               # after the collective: a rank that raises leaves no other rank waiting
    optimizer.step(buf)
    total = np.float32(0.0)
    for v in buf[:, fp.n].cpu().numpy():
        total = np.float32(total + v)
    return float(total)
