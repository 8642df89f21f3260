"""What the `state_dict()` / `load_state_dict()` of the online objects (`apply.PickStore`, `apply.OnlineDay`, `postproc.StreamPeaks`,
`postproc.OnlineDetector`, `apply.OnlineCatalogue`) share: the fingerprint comparison and the one copy of a
state's device tensors to the host. Pure numpy / torch: nothing here touches the HIP library."""
import numpy as np
import torch


def _same(a, b):
    """Two fingerprint values: arrays (numpy, tensors, nested sequences of numbers) by shape and value, everything else by `==`."""
    if a is None or b is None or isinstance(a, (str, bool)) or isinstance(b, (str, bool)):
        return type(a) is type(b) and a == b
    a, b = (np.asarray(x.detach().cpu() if torch.is_tensor(x) else x) for x in (a, b))
    return a.shape == b.shape and bool(np.array_equal(a, b))


def fingerprint_diff(saved, own):
    """The name of the first field of the fingerprint `own` (a dict, in its own order) that `saved` lacks or holds another value of;
    then any field only `saved` has; None when the two agree."""
    for name, value in own.items():
        if name not in saved or not _same(saved[name], value):
            return name
    for name in saved:
        if name not in own:
            return name
    return None


def check_fingerprint(who, state, own):
    """ValueError naming the first differing field unless `state["fingerprint"]` is the fingerprint `own`."""
    if not isinstance(state, dict) or not isinstance(state.get("fingerprint"), dict):
        raise ValueError("%s.load_state_dict: not a state of this class (no fingerprint)" % who)
    name = fingerprint_diff(state["fingerprint"], own)
    if name is not None:
        short = lambda x: np.array2string(np.asarray(x.cpu() if torch.is_tensor(x) else x), threshold=6, edgeitems=2) if x is not None else "None"
        raise ValueError("%s.load_state_dict: the state belongs to another %s (saved: %s, this object: %s); a day resumes under the "
                         "schedule and options it was saved under" % (who, name, short(state["fingerprint"].get(name)), short(own.get(name))))


def to_host(state):
    """A deep copy of `state` (nested dicts, lists, tuples) in which every tensor is a CPU tensor of the same dtype, shape and bytes
    and every numpy array a copy. The GPU tensors are copied into page-locked memory on the current stream of their device, all of them
    queued first; then the host waits once per device -- the one synchronisation of a `state_dict()`."""
    devices = set()

    def walk(x):
        if torch.is_tensor(x):
            x = x.detach()
            if not x.is_cuda:
                return x.clone()
            devices.add(x.device)
            h = torch.empty(x.shape, dtype=x.dtype, pin_memory=True)
            with torch.cuda.device(x.device):
                h.copy_(x, non_blocking=True)
            return h
        if isinstance(x, np.ndarray):
            return x.copy()
        if isinstance(x, dict):
            return {k: walk(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return type(x)(walk(v) for v in x)
        return x

    out = walk(state)
    for dev in devices:
        torch.cuda.current_stream(dev).synchronize()
    return out
