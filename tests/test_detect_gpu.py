"""GPU: source detection on the device (genie_peak_distance / genie_time_groups / genie_local_marching through genie_amd.postproc)
against the host functions it restates -- `find_peaks_rows` / scipy.signal.find_peaks, `group_sources`, `local_marching` (pinned to the
reference's LocalMarching by tests/golden/localmarching.npz), `detect_sources`, `detect_refine_associate`. Index sets, flags and
surviving rows are compared exactly (integer and compare work)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy.signal import find_peaks

from genie_amd import _lib, apply, graph, module, postproc, synthetic
from tests.test_detect_cpu import SP_WIN, TC_WIN, dense_local_marching, marching_cases, pairs_on_time_radius
from tests.util import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDENT = lambda x: x


def _sorted_rows(a):
    a = np.asarray(a)
    return a[np.lexsort(a.T[::-1])] if len(a) else np.zeros((0, 5))


# ---------------------------------------------------------------------------------------------- LocalMarching
@pytest.mark.parametrize("tag", ["apply", "default", "wide"])
def test_local_marching_device_matches_reference(tag):
    z = np.load(os.path.join(GOLDEN_DIR, "localmarching.npz"))
    kw = {k[len("kw_%s_" % tag):]: float(z[k]) for k in z.files if k.startswith("kw_%s_" % tag)}
    if "n_steps_max" in kw:
        kw["n_steps_max"] = int(kw["n_steps_max"])
    if "use_directed" in kw:
        kw["use_directed"] = bool(kw["use_directed"])
    got = _sorted_rows(postproc.local_marching_device(z["srcs"], IDENT, device=DEV, **kw))
    want = z["keep_" + tag]
    assert got.shape == want.shape and np.array_equal(got, want)
    assert 0 < len(want) < len(z["srcs"])


def test_local_marching_device_equals_host_on_seeded_cases():
    n_cases = on_radius = 0
    for srcs, kw in marching_cases():
        srcs = srcs[np.random.default_rng(n_cases).permutation(len(srcs))]            # the wrapper sorts by time itself
        got = postproc.local_marching_device(srcs, IDENT, device=DEV, **kw)
        want = postproc.local_marching(srcs, IDENT, **kw)
        assert got.shape == want.shape and np.array_equal(got, want), (n_cases, kw)
        on_radius += pairs_on_time_radius(srcs)
        n_cases += 1
    assert n_cases >= 50 and on_radius > 1000


def _sized(n, kind, seed):
    rng = np.random.default_rng(seed)
    xq = np.c_[rng.uniform(0, 120e3, (max(n, 1), 2)), rng.uniform(-40e3, 0, max(n, 1))]
    val = np.round(rng.uniform(0.15, 1, n), 2).astype(np.float32)
    if kind == "one_window":                                  # every pair passes the time test
        t = 1.6e9 + 0.75 * rng.integers(0, 9, n)
    elif kind == "isolated":                                  # no pair passes it
        t = 1234.56 + 7.5 * rng.permutation(n)
    else:
        t = 0.75 * rng.integers(0, max(2, n // 4), n)
    return np.c_[xq[:n], t, val]


@pytest.mark.parametrize("n,kind", [(0, "mixed"), (1, "mixed"), (2, "mixed"), (2, "one_window"), (255, "mixed"), (256, "mixed"),
                                    (257, "mixed"), (5000, "mixed"), (5000, "one_window"), (5000, "isolated")])
@pytest.mark.parametrize("n_steps_max,use_directed", [(2, False), (100, True)])
def test_local_marching_device_equals_host_on_sizes(n, kind, n_steps_max, use_directed):
    srcs = _sized(n, kind, 1000 + n)
    kw = dict(tc_win=TC_WIN, sp_win=SP_WIN, scale_depth=0.2, n_steps_max=n_steps_max, use_directed=use_directed)
    got = postproc.local_marching_device(srcs, IDENT, device=DEV, **kw)
    want = postproc.local_marching(srcs, IDENT, **kw)
    assert got.shape == want.shape and np.array_equal(got, want)
    if kind == "isolated":
        assert len(got) == n
    if kind == "one_window" and n == 5000:
        assert 0 < len(got) < n


def test_local_marching_device_respects_groups_and_step_counts():
    """The group argument of the kernel (the wrappers of whole days pass it) and every n_steps_max, against the dense restatement:
    nodes closer than tc_win but in different groups are not linked."""
    srcs, kw = next(marching_cases(1, seed=5))
    srcs = srcs[np.argsort(srcs[:, 3], kind="stable")]
    group = (np.arange(len(srcs)) // 37).astype(np.int32)
    xs = torch.from_numpy(srcs[:, 0:3] * np.array([1.0, 1.0, 0.2])).to(DEV)
    t, v = torch.from_numpy(srcs[:, 3].copy()).to(DEV), torch.from_numpy(srcs[:, 4].astype(np.float32)).to(DEV)
    differs = 0
    for steps in (0, 1, 2, 3, 5, 100):
        for directed in (False, True):
            got = postproc._marching_keep(xs, t, v, torch.from_numpy(group).to(DEV), TC_WIN, SP_WIN, steps, 1e-12, directed)
            want = dense_local_marching(srcs, IDENT, TC_WIN, SP_WIN, steps, scale_depth=0.2, use_directed=directed, group=group)
            assert np.array_equal(got.cpu().numpy(), want), (steps, directed)
            differs += int(not np.array_equal(want, dense_local_marching(srcs, IDENT, TC_WIN, SP_WIN, steps, scale_depth=0.2,
                                                                         use_directed=directed)))
    assert differs > 0


# ---------------------------------------------------------------------------------------------- time groups
@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 20000])
def test_time_groups_match_group_sources(n):
    rng = np.random.default_rng(n)
    t = 1.6e9 + np.cumsum(np.where(rng.random(n) < 0.02, 15.0, 0.75 * rng.integers(0, 3, n)))      # gaps of exactly break_win
    srcs = np.c_[np.zeros((n, 3)), t, np.ones(n)]
    want = np.concatenate([np.full(len(g), k) for k, g in enumerate(postproc.group_sources(srcs, 15.0))])
    got = postproc.time_groups_device(torch.from_numpy(t).to(DEV), 15.0)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert n < 100 or want[-1] > 5


# ---------------------------------------------------------------------------------------------- distance rule
def _matrix(rows, cols, seed, quantise=False):
    rng = np.random.default_rng(seed)
    x = (rng.random((rows, cols)) * (rng.random((rows, cols)) < 0.15)).astype(np.float32)
    if quantise:
        x = np.round(x * 8.0) / 8.0                       # many exact ties and flat tops
    if cols > 4:
        x[0, :3] = 0.9                                    # flat run touching the first sample: not a peak
        x[-1, -3:] = 0.9                                  # ... and the last sample
        x[rows // 2, :] = 0.0
    return x


def _distance_rule_holds(x_row, cand, kept, d):
    """What every valid answer of the distance rule satisfies, whatever the order of equal heights: kept peaks are candidates, no two
    closer than d, and every dropped candidate has a kept one of greater-or-equal height within d."""
    kept = np.asarray(kept)
    ok = set(kept.tolist()) <= set(cand.tolist()) and (len(kept) < 2 or int(np.diff(kept).min()) >= d)
    for c in set(cand.tolist()) - set(kept.tolist()):
        near = kept[np.abs(kept - c) < d]
        ok = ok and len(near) > 0 and x_row[near].max() >= x_row[c]
    return bool(ok)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 2), (5, 3), (7, 255), (4, 256), (9, 257), (33, 1000), (120, 4099)])
@pytest.mark.parametrize("quantise", [False, True])
@pytest.mark.parametrize("distance", [None, 1, 6])
def test_row_peaks_device_match_host_and_scipy(rows, cols, quantise, distance):
    x = _matrix(rows, cols, rows * 77 + cols, quantise)
    h = 0.25
    xd = torch.from_numpy(x).to(DEV)
    r, c, v = postproc.find_peaks_rows_device(xd, h, distance)
    assert r.is_cuda and r.dtype == torch.int32 and c.dtype == torch.int32 and v.dtype == torch.float32
    r, c, v = r.cpu().numpy().astype(np.int64), c.cpu().numpy().astype(np.int64), v.cpu().numpy()
    assert np.array_equal(v, x[r, c])
    if quantise and distance not in (None, 1):
        d = int(np.ceil(distance))
        n_dropped = 0
        for i in range(rows):
            cand = find_peaks(x[i].astype(np.float64), height=h)[0]
            sci = find_peaks(x[i].astype(np.float64), height=h, distance=distance)[0]
            assert _distance_rule_holds(x[i], cand, sci, d)                     # the conditions are scipy's too: not vacuous
            assert _distance_rule_holds(x[i], cand, c[r == i], d), i
            n_dropped += len(cand) - int((r == i).sum())
        assert cols < 255 or n_dropped > 0
        r2, c2, v2 = postproc.find_peaks_rows_device(xd, h, distance)
        assert np.array_equal(r2.cpu().numpy(), r) and np.array_equal(c2.cpu().numpy(), c) and np.array_equal(v2.cpu().numpy(), v)
        return
    hr, hc, hv = postproc.find_peaks_rows(xd, h, distance)
    assert np.array_equal(r, hr) and np.array_equal(c, hc) and np.array_equal(v, hv)
    wr, wc, wv = [], [], []
    for i in range(rows):
        ip, props = find_peaks(x[i].astype(np.float64), height=h, distance=distance)
        wr.append(np.full(len(ip), i)); wc.append(ip); wv.append(props["peak_heights"])
    wr, wc, wv = np.concatenate(wr), np.concatenate(wc), np.concatenate(wv)
    assert np.array_equal(r, wr) and np.array_equal(c, wc) and np.array_equal(v.astype(np.float64), wv)


def test_equal_heights_keep_the_later_column():
    """The device's fixed rule for what scipy leaves open: of equal peaks closer than d the later one stays, and removal does not chain
    through a removed peak (1, 4, 7 equal with d = 4: 7 removes 4, so 1 stays)."""
    x = np.zeros((2, 40), dtype=np.float32)
    x[0, [1, 4, 7]] = 0.5
    x[1, [10, 12]] = 0.5
    x[1, 14] = 0.75
    x[1, [20, 23]] = [0.5, 0.25]
    r, c, _ = postproc.find_peaks_rows_device(torch.from_numpy(x).to(DEV), 0.2, 4)
    assert r.cpu().tolist() == [0, 0, 1, 1, 1] and c.cpu().tolist() == [1, 7, 10, 14, 20]


# ---------------------------------------------------------------------------------------------- detect_sources
def _bumps(seed=11, Q=400, T=3000, dt_win=0.75):
    """The synthetic Out_2 of test_detect_sources_end_to_end_matches_the_reference_statements."""
    rng = np.random.default_rng(seed)
    xq = np.c_[rng.uniform(0, 300e3, (Q, 2)), rng.uniform(-30e3, 0, Q)]
    ts = np.arange(T) * dt_win
    out = np.zeros((Q, T), dtype=np.float32)
    for _ in range(9):
        c, t0, a = xq[rng.integers(0, Q)], rng.uniform(50, T * dt_win - 50), rng.uniform(0.3, 1.0)
        d = np.linalg.norm((xq - c) * np.array([1, 1, 0.3]), axis=1)
        out += (a * np.exp(-0.5 * (d / 25e3) ** 2)[:, None] * np.exp(-0.5 * ((ts - t0) / 3.0) ** 2)[None, :]).astype(np.float32)
    out += (0.02 * rng.random((Q, T))).astype(np.float32)
    return out, xq, ts


def _grouped_day(seed=29, Q=1500, T=4000, dt_win=0.75):
    """25 events 110 s apart on epoch-sized times with a moveout (further queries peak later), one of them seen by a third of the
    queries, three doubled 8 s later somewhere else, and one query lit alone near the end."""
    rng = np.random.default_rng(seed)
    xq = np.c_[rng.uniform(0, 300e3, (Q, 2)), rng.uniform(-30e3, 0, Q)]
    ts = 1.6e9 + np.arange(T) * dt_win
    out = (0.02 * rng.random((Q, T))).astype(np.float32)
    events = [(xq[rng.integers(0, Q)], ts[0] + 60.0 + 110.0 * k + rng.uniform(0, 20), rng.uniform(0.3, 1.0), 25e3) for k in range(25)]
    events[7] = (xq[5], events[7][1], 1.0, 90e3)
    events += [(xq[rng.integers(0, Q)], events[k][1] + 8.0, 0.6, 25e3) for k in (2, 11, 19)]
    for c, t0, a, sig in events:
        d = np.linalg.norm((xq - c) * np.array([1, 1, 0.3]), axis=1)
        lit = np.flatnonzero(a * np.exp(-0.5 * (d / sig) ** 2) > 0.05)
        tp = t0 + d[lit] / 20e3
        out[lit] += (a * np.exp(-0.5 * (d[lit] / sig) ** 2)[:, None]
                     * np.exp(-0.5 * ((ts[None, :] - tp[:, None]) / 3.0) ** 2)).astype(np.float32)
    out[17, T - 60:T - 57] += np.array([0.2, 0.4, 0.2], dtype=np.float32)
    return out, xq, ts


DETECT_KW = dict(thresh=0.15, src_t_kernel=5.0, dt_win=0.75, break_win=15.0, tc_win=5.0 * 1.35, sp_win=20e3 * 1.35)


def _detect_both(out, xq, ts, ftrns1=IDENT):
    k = DETECT_KW
    args = (torch.from_numpy(out).to(DEV), xq, ts, ftrns1, k["thresh"], k["src_t_kernel"], k["dt_win"], k["break_win"], k["tc_win"],
            k["sp_win"])
    return postproc.detect_sources_device(*args), postproc.detect_sources(*args)


def test_detect_sources_device_equals_host_on_bumps():
    got, want = _detect_both(*_bumps())
    assert 5 <= len(want) and got.dtype == np.float64
    assert got.shape == want.shape and np.array_equal(_sorted_rows(got), _sorted_rows(want))
    assert np.all(np.diff(got[:, 3]) >= 0)


def test_detect_sources_device_equals_host_on_many_groups():
    out, xq, ts = _grouped_day()
    k = DETECT_KW
    init = postproc.initial_sources(torch.from_numpy(out).to(DEV), xq, ts, k["thresh"], k["src_t_kernel"], k["dt_win"])
    sizes = [len(g) for g in postproc.group_sources(init, k["break_win"])]
    assert len(sizes) >= 20 and min(sizes) == 1 and max(sizes) >= 500
    scale = lambda x: x * np.array([1.0, 1.0, 2.0]) + 7.0                        # a transform that is not the identity
    got, want = _detect_both(out, xq, ts, scale)
    assert len(sizes) <= len(want) < len(init) // 10
    assert got.shape == want.shape and np.array_equal(_sorted_rows(got), _sorted_rows(want))
    assert np.all(np.diff(got[:, 3]) >= 0)


def test_detect_sources_device_without_peaks():
    out, xq, ts = _bumps(T=300)
    got, want = _detect_both(np.minimum(out, np.float32(0.1)), xq, ts)
    assert got.shape == (0, 5) and want.shape == (0, 5)


# ---------------------------------------------------------------------------------------------- the chain of apply.py
class _Setup(object):
    """The small day of tests/test_day_loops_gpu.py: a station file of which the model uses a subset, a source grid, picks around a few
    events, the model with adjacencies and time-pointer tables set."""

    def __init__(self, S_all=15, n_use=11, G=70, n_picks=500, seed=91, weights="assoc_7x45"):
        from oracle import genie_oracle as O
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)
        rng = np.random.default_rng(seed)
        ga = synthetic.Geometry(S_all, G, L=60e3, n_query=8, seed=seed)
        self.ind_use = np.sort(rng.choice(S_all, n_use, replace=False))
        self.locs = ga.locs[self.ind_use]
        A_sta_sta = graph.knn_graph(self.locs / 1000.0, graph.k_sta_effective(8, n_use))
        P = synthetic.make_picks(ga, n_picks, seed=seed + 1)
        P[:, 0] = P[:, 0] * 0.5 + 7000.0
        P = P[rng.permutation(P.shape[0])]
        trv_all = ga.travel_times().astype(np.float32)
        trv_use = np.ascontiguousarray(trv_all[:, self.ind_use])
        self.max_t = float(np.ceil(trv_all.max() + 1.0))
        self.sig, self.dt = 3.0, 0.3
        ea = ((ga.x_grid[:, None, :] - self.locs[None, :, :]) / ga.scale_x_extend.reshape(1, 1, 3)).reshape(-1, 3).astype(np.float32)
        w = O.weights_from_npz(np.load(os.path.join(GOLDEN_DIR, weights + ".npz")))
        A_edges_p, A_edges_s, dt_partition = graph.time_pointers(trv_use, max_t=self.max_t, dt=self.sig / 5.0, k=10, win=2.0 * self.sig)
        net = module.GCN_Detection_Network_extended(lambda x: x, lambda x: x, device=DEV)
        net.load_state_dict({k: v.clone() for k, v in w.items()}, strict=True)
        net.eval()
        net.set_adjacencies_base(torch.from_numpy(A_sta_sta), torch.from_numpy(ga.A_src_src), f(ea), f(self.locs), f(ga.x_grid),
                                 torch.from_numpy(A_edges_p).to(DEV), torch.from_numpy(A_edges_s).to(DEV), f(dt_partition),
                                 f(trv_use.reshape(-1, 2)))
        self.picks = apply.ResidentPicks(P, self.ind_use, S_all, DEV)
        self.leg = apply.GridLeg(net, ga.x_grid, trv_use)
        self.tq = np.arange(-3.0, 3.75, 0.75).reshape(-1, 1)


def test_detection_chain_on_device_equals_the_host_chain():
    s = _Setup()
    rng = np.random.default_rng(23)
    Q, dt_win, src_t_kernel, thresh = 150, 0.75, 5.0, 0.15
    xq = np.c_[rng.uniform(0, 60e3, (Q, 2)), rng.uniform(-30e3, 0, Q)]
    ts = 6990.0 + np.arange(400) * dt_win
    out = np.zeros((Q, len(ts)), dtype=np.float32)
    far = int(np.argmax(np.linalg.norm(xq - xq[3], axis=1)))
    centres = [(xq[3], 7001.0), (xq[3] + [2e3, 0, 0], 7002.5), (xq[far], 7011.0), (xq[90], 7100.0), (xq[91], 7190.0)]
    for c, t0 in centres:
        d = np.linalg.norm((xq - c) * np.array([1, 1, 0.3]), axis=1)
        out += (0.7 * np.exp(-0.5 * (d / 12e3) ** 2)[:, None] * np.exp(-0.5 * ((ts - t0) / 3.0) ** 2)[None, :]).astype(np.float32)
    Out_2 = torch.from_numpy(out).to(DEV)
    ranges = ((0.0, 60e3), (0.0, 60e3), (-40e3, 2e3))
    off_min, off_rng = np.array([[-5e3, -5e3, -3e3]]), np.array([[10e3, 10e3, 6e3]])
    tc_win, sp_win, break_win = src_t_kernel * 1.35, 20e3, 15.0

    def trv(locs, srcs):
        d = torch.linalg.norm(locs[None, :, :] - srcs[:, None, :], dim=2)
        return torch.stack((d / 6000.0, d / 3500.0), dim=2)

    def run(**kw):
        return apply.detect_refine_associate([s.leg], s.picks, Out_2, xq, ts, s.locs, trv, s.tq, s.max_t, IDENT, IDENT, *ranges, off_min,
                                             off_rng, 200, thresh, src_t_kernel, dt_win, break_win, tc_win, sp_win,
                                             rand=np.random.RandomState(3).rand, ftrns2_device=IDENT, kernel_sig_t=s.sig, dt_embed=s.dt, **kw)

    want, got = run(), run(detect_on_device=True)
    assert 3 <= len(want["srcs"]) <= len(centres) and len(want["srcs_refined"]) >= 2
    assert np.array_equal(got["srcs"], want["srcs"]) and np.array_equal(got["srcs_refined"], want["srcs_refined"])
    for k in ("Out_p_save", "Out_s_save", "Save_picks", "lp_meta"):
        assert len(got[k]) == len(want[k]) == len(want["srcs_refined"])
    assert torch.equal(got["trv_out_srcs"], want["trv_out_srcs"])
    keep_h = apply.retained_after_marching(want["srcs_refined"], IDENT, tc_win, sp_win)
    keep_d = apply.retained_after_marching(want["srcs_refined"], IDENT, tc_win, sp_win, device=DEV)
    assert np.array_equal(keep_h, keep_d)


# ---------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    n = 8
    i64 = torch.zeros(4, dtype=torch.int64, device=DEV)
    col, val = torch.arange(n, dtype=torch.int32, device=DEV), torch.ones(n, dtype=torch.float32, device=DEV)
    t, xs = torch.arange(n, dtype=torch.float64, device=DEV), torch.zeros(n, 3, dtype=torch.float64, device=DEV)
    grp = torch.zeros(n, dtype=torch.int32, device=DEV)
    keep = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    scratch = torch.zeros(int(lib.genie_local_marching_scratch_bytes(n)), dtype=torch.uint8, device=DEV)
    P = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else ctypes.c_void_p(0)
    D = ctypes.c_double

    def refused(rc, word):
        assert rc == -1 and word in lib.genie_last_error().decode()               # GENIE_ERR_ARG

    refused(lib.genie_peak_distance(P(i64), 4, -1, P(col), P(val), 3, P(keep), None), "genie_peak_distance")
    refused(lib.genie_peak_distance(P(i64), 4, n, None, P(val), 3, P(keep), None), "null")
    refused(lib.genie_peak_distance(P(i64), 4, n, P(col), P(val), 0, P(keep), None), "d >= 1")
    refused(lib.genie_peak_distance(None, 4, n, P(col), P(val), 3, P(keep), None), "null")
    refused(lib.genie_time_groups(P(t), -1, D(15.0), P(grp), P(grp), None), "genie_time_groups")
    refused(lib.genie_time_groups(None, n, D(15.0), P(grp), P(grp), None), "null")
    refused(lib.genie_time_groups(P(t), n, D(float("nan")), P(grp), P(grp), None), "break_win")

    def march(xs_=xs, t_=t, val_=val, n_=n, tc=6.75, sp=27e3, scratch_=scratch, keep_=keep):
        return lib.genie_local_marching(P(xs_), P(t_), P(val_), P(grp), n_, D(tc), D(sp), 2, D(1e-12), 0, P(scratch_), P(keep_), None)

    refused(march(n_=-1), "genie_local_marching")
    for bad in (-1.0, float("inf"), float("nan")):
        refused(march(tc=bad), "tc_win")
        refused(march(sp=bad), "sp_win")
    for kw in (dict(xs_=None), dict(t_=None), dict(val_=None), dict(scratch_=None), dict(keep_=None)):
        refused(march(**kw), "null")
    torch.cuda.synchronize()
    assert bool((keep == 7).all())                                                # nothing ran
    assert lib.genie_local_marching(None, None, None, None, 0, D(6.75), D(27e3), 2, D(1e-12), 0, None, None, None) == 0
    assert march() == 0
    torch.cuda.synchronize()
    assert bool((keep == 1).all())                                                # eight nodes at one place: the equal values all stay
