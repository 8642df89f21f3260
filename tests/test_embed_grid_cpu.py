"""CPU: the conditions under which tests/test_embed_grid_gpu.py means something, asserted on the oracle's own arithmetic
(oracle/embed_oracle.py) and on the inputs of tests/embed_grid_cases.py alone, and the host side of the embedding (the range search of
a window's picks, `ResidentPicks`, `PickStore`, `pick_inputs`) against the oracle on the same quantised picks. Every comparison is exact."""
import numpy as np
import pytest
import torch

from genie_amd import apply
from oracle import embed_oracle as E
from tests import embed_grid_cases as C

E_CASES = [c for c in C.CASES if c[0] == "E"]
N_CASES = [c for c in C.CASES if c[0] == "N"]
HOST_CASES = [c for c in C.CASES if not c[3]]
ids = C.case_id


def _parts(c):
    (P, t0, max_t, sig, dt, trv, pairs), sets = C.case(*c)
    S = C.SHAPES[c[1]][0]
    return P, t0, max_t, sig, dt, trv, pairs, sets, S


def _node_trv(trv, pairs):
    """[N, 2]: the travel times of every product node, as the oracle gathers them."""
    return trv[pairs[1], pairs[0], :]


def _series(c):
    """The oracle's per-station series of the case's window: (embed_p, embed_s) [S, n_time]."""
    P, t0, max_t, sig, dt, trv, pairs, sets, S = _parts(c)
    P_slice = E.window_pick_slice(P, t0, np.arange(S), max_t, sig)
    ep, es, _ = E.embed_time_series(P_slice, t0, max_t, sig, dt, P_slice[:, 1].astype("int"), S)
    return ep, es


# ---- the inputs are as tie-laden as they claim ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", E_CASES, ids=ids)
def test_family_e_quotients_are_exact_integers_or_exact_halves(c):
    P, t0, max_t, sig, dt, trv, pairs, sets, S = _parts(c)
    assert dt == 0.25 and t0 / 0.25 == np.round(t0 / 0.25) and np.array_equal(P[:, 0] / 0.125, np.round(P[:, 0] / 0.125))
    q = C.scatter_quotients(P[:, 0], t0, sig, dt)
    aligned = P[:, 0] / 0.25 == np.round(P[:, 0] / 0.25)
    assert aligned.sum() >= 30 and np.array_equal(q[aligned], np.round(q[aligned]))
    assert (~aligned).sum() >= 30 and np.array_equal(q[~aligned] - np.floor(q[~aligned]), np.full((~aligned).sum(), 0.5))
    nt = _node_trv(trv, pairs)
    assert nt.dtype == np.float32 and np.array_equal(nt / np.float32(0.25), np.round(nt / np.float32(0.25)))
    qg = C.gather_quotients(nt, t0, sig, dt)
    assert np.array_equal(qg, np.round(qg))
    print("%s: %d aligned picks, %d half-sample picks, %d gather quotients, all exact" % (ids(c), aligned.sum(), (~aligned).sum(), qg.size))


@pytest.mark.parametrize("c", N_CASES, ids=ids)
def test_family_n_scatter_quotients_sit_next_to_integers(c):
    P, t0, max_t, sig, dt, trv, pairs, sets, S = _parts(c)
    assert dt == 0.3 == np.round(sig / 10.0, 2)
    assert np.array_equal(P[:, 0], np.round(P[:, 0] * 100.0) / 100.0)                   # the 0.01 s raster
    inside = E.window_pick_slice(P, t0, np.arange(S), max_t, sig)[:, 0]
    below, on_above, differ = C.tie_counts(C.scatter_quotients(inside, t0, sig, dt))
    print("%s: scatter quotients within 1e-9 of an integer: %d below, %d on or above; truncation != rounding for %d" % (ids(c), below, on_above, differ))
    assert below >= 20 and on_above >= 20 and differ >= 20


@pytest.mark.parametrize("c", N_CASES, ids=ids)
def test_family_n_gather_quotients_sit_on_and_next_to_integers(c):
    """On or above an integer within 1e-9: at least 5. Below: what float32 holds -- see `test_no_float32_travel_time_...`: the nearest
    float32 below a tie, at most one float32 spacing (2^-18 at 40 s) over dt = 1.3e-5 below the integer, truncation != rounding."""
    P, t0, max_t, sig, dt, trv, pairs, sets, S = _parts(c)
    nt = _node_trv(trv, pairs)
    q = C.gather_quotients(nt, t0, sig, dt)
    assert np.array_equal(q, C.gather_quotients(nt, 0.0, sig, dt))                      # (trv + t0) - (t0 - 9) is exact: t0 drops out
    below9, on_above9, _ = C.tie_counts(q)
    d = q - np.round(q)
    tight_below = (d < 0) & (d >= -2.0 ** -18 / dt)
    tight_above = (d > 0) & (d <= 2.0 ** -18 / dt)
    differ = int((q[tight_below].astype("int") != np.round(q[tight_below])).sum())
    print("%s: gather quotients within 1e-9: %d below, %d on or above; within one float32 step: %d below (largest gap %.3g), %d above; "
          "truncation != rounding for %d" % (ids(c), below9, on_above9, tight_below.sum(), -d[tight_below].min(), tight_above.sum(), differ))
    assert on_above9 >= 5 and tight_below.sum() >= 5 and tight_above.sum() >= 5 and differ >= 5
    in_range = (nt >= 0) & (nt <= np.float32(max_t))
    on_raster = nt == (np.round(nt.astype(np.float64) * 100.0) / 100.0).astype(np.float32)
    assert (~in_range).sum() == 4 and on_raster.mean() > 0.9


def test_no_float32_travel_time_is_within_1e_9_below_a_gather_integer():
    """Why the gather quotients of family N cannot show "at least 5 within 1e-9 below an integer": no float32 in [0, max_t] does. The
    multiples of 1.5 give exact integers (27 of them); the nearest other float32 below a tie misses it by 8e-8 or more."""
    vals, q = C.gather_tie_search()
    d = q - np.round(q)
    assert int(((d < 0) & (d >= -1e-9)).sum()) == 0
    on = vals[d == 0][vals[d == 0] != np.nextafter(np.float32(0), np.float32(1))]      # (the smallest subnormal adds nothing to 9)
    assert np.array_equal(on, (1.5 * np.arange(27)).astype(np.float32))
    assert -d[d < 0].max() > 5e-8
    k = np.arange(0, 4001)
    dr = C.gather_quotients((k / 100.0).astype(np.float32), 0.0, C.SIGMA, 0.3)
    dr = dr - np.round(dr)
    assert int(((dr < 0) & (dr >= -1e-9)).sum()) == 0                                   # the 0.01 s raster itself: none either


@pytest.mark.parametrize("c", C.CASES, ids=ids)
def test_no_reference_value_lies_near_the_mask_threshold(c):
    nearest = min(float(np.abs(np.abs(C.reference(c, sign, nop)[0]) - 0.01).min()) for sign in (False, True) for nop in (False, True))
    print("%s: nearest |Slice| to 0.01: %.3g" % (ids(c), nearest))
    assert nearest > 1e-5
    Slice, Mask = C.reference(c)
    assert 0.05 < Mask.mean() < 0.95 and (Slice > 0.5).sum() > 50


# ---- every planted set does what it says in the oracle's output ----------------------------------------------------------------------

@pytest.mark.parametrize("c", C.CASES, ids=ids)
def test_planted_picks(c):
    P, t0, max_t, sig, dt, trv, pairs, sets, S = _parts(c)
    n_time, n_extra = sets["n_time"], sets["n_extra"]
    ind = np.arange(S)
    without = lambda rows: np.delete(P, rows, axis=0)
    ref = lambda P_: E.extract_input_from_data(P_, t0, ind, S + 2, trv, pairs, max_t, sig, dt)
    Slice, Mask = C.reference(c)
    P_slice = E.window_pick_slice(P, t0, ind, max_t, sig)
    # (a)
    assert np.array_equal(np.sort(P[sets["border_out"], 0]), [t0 - 2 * sig, t0 + max_t + 2 * sig])
    assert not np.isin(P[sets["border_out"], 0], P_slice[:, 0]).any() and np.isin(P[sets["border_in"], 0], P_slice[:, 0]).all()
    assert np.array_equal(ref(without(sets["border_out"]))[0], Slice) and not np.array_equal(ref(without(sets["border_in"]))[0], Slice)
    inward = P.copy()                     # one raster step inside, the border picks would show: their phase's series of the station is theirs alone
    inward[sets["border_out"], 0] += np.where(P[sets["border_out"], 0] < t0, 1.0, -1.0) * C.STEP[c[0]]
    assert not np.array_equal(ref(inward)[0], Slice)
    # (b)
    near = lambda tag: C.scatter_quotients(P[sets[tag], 0], t0, sig, dt).astype("int")
    assert len(sets["fan_reach_first"]) and (near("fan_reach_first") - n_extra == 0).all() and (near("fan_past_first") - n_extra < 0).all()
    assert len(sets["fan_reach_last"]) and (near("fan_reach_last") + n_extra == n_time - 1).all() and (near("fan_past_last") + n_extra > n_time - 1).all()
    ep, es = _series(c)
    s_b = sets["stations"]["b"]
    for emb in (ep, es):
        assert emb.shape == (S, n_time) and emb[s_b, 0] == 0 and emb[s_b, n_time - 1] == 0
        assert emb[s_b, 1] > 0.01 and emb[s_b, n_time - 2] > 0.01                        # (what the zeroed edge samples would hold, nearly)
    # (c)
    a, b = P[sets["dup_phase_pair"]]
    assert np.array_equal(a[:2], b[:2]) and sorted((a[4], b[4])) == [0.0, 1.0]
    a, b = P[sets["dup_same_phase"]]
    assert np.array_equal(a, b)
    # (d)
    a, b = P[sets["whole_samples_apart"]]
    steps = abs(a[0] - b[0]) / dt
    assert a[1] == b[1] and a[4] == b[4] and abs(steps - 8.0) <= 1e-9
    if c[0] == "E":                       # a sample half-way between them gets bit-equal values from two different picks
        k = int(C.scatter_quotients(min(a[0], b[0]), t0, sig, dt)) + 4
        tr = t0 - 3 * sig + k * dt
        assert np.float32(np.exp(-0.5 * (a[0] - tr) ** 2 / sig ** 2)) == np.float32(np.exp(-0.5 * (b[0] - tr) ** 2 / sig ** 2))
    # (e)
    s_e = sets["empty_station"]
    assert not (P[:, 1] == s_e).any()
    for sign in (False, True):
        assert float(np.abs(C.reference(c, sign)[0][pairs[0] == s_e]).max(initial=0.0)) == 0.0
    assert (pairs[0] == s_e).sum() == 0 or len(sets["node_empty"]) == 1
    # (f)
    bad = np.concatenate((sets["bad_station"], sets["bad_phase"]))
    assert (P[sets["bad_station"], 1] >= S).all() and not np.isin(P[sets["bad_phase"], 4], (0.0, 1.0)).any() and len(bad) == 4
    assert ((P[bad, 0] > t0 - 2 * sig) & (P[bad, 0] < t0 + max_t + 2 * sig)).all()
    assert np.array_equal(ref(without(bad))[0], Slice)
    # the border picks of the other window starts and the ball query's radius
    assert len(sets["step_border"]) == 8 and len(sets["ball_on"]) == 2 and len(sets["ball_out"]) == 2


@pytest.mark.parametrize("c", C.CASES, ids=ids)
def test_planted_product_nodes(c):
    P, t0, max_t, sig, dt, trv, pairs, sets, S = _parts(c)
    n_time = sets["n_time"]
    ind = C.gather_quotients(_node_trv(trv, pairs), t0, sig, dt).astype("int")
    assert ind.min() == 0 and ind.max() == n_time - 1
    # (g)
    for tag, want in (("node_first", 0), ("node_last", n_time - 1), ("node_zero", sets["n_extra"])):
        assert len(sets[tag]) >= 1 and (ind[sets[tag]] == want).any(axis=1).all(), tag
    assert (_node_trv(trv, pairs)[sets["node_max_t"]] == np.float32(max_t)).all()
    for sign in (False, True):
        Slice = C.reference(c, sign)[0]
        for tag, want in (("node_first", 0), ("node_last", n_time - 1)):
            rows = sets[tag]
            at = ind[rows] == want
            assert float(np.abs(Slice[rows][:, [0, 1]][at]).max()) == 0.0 and float(np.abs(Slice[rows][:, [2, 3]][at]).max()) == 0.0
    # (h)
    if c[0] == "E":
        rows = sets["half_nodes"]
        assert len(rows) >= 2 and len(sets["half_picks"]) == 2 * len(sets["half"])
        for s, (kp, ks) in sets["half"].items():
            mine = rows[pairs[0, rows] == s]
            assert len(mine) >= 1 and (ind[mine] == [kp, ks]).all()
            ep, es = _series(c)
            assert ep[s, kp] == ep[s, kp + 1] > 0.99 and es[s, ks] == es[s, ks + 1] > 0.99
        Ss, Ms = C.reference(c, True)
        assert not Ss[rows].any() and not np.signbit(Ss[rows]).any() and not Ms[rows].any()                   # exactly +0.0
        assert (C.reference(c, False)[0][rows] > 0.99).all()
        assert (Ss < -0.5).sum() > 20 and (Ss > 0.5).sum() > 20
    else:
        for tag in ("gather_on", "gather_below", "gather_above"):
            assert len(sets[tag]) >= 20, tag


# ---- the host side: which picks a window sees ----------------------------------------------------------------------------------------

def _starts(t0):
    return [t0 + 0.5 * j for j in range(-4, 5)]          # whole multiples of half a second around the case's own start


@pytest.mark.parametrize("c", HOST_CASES, ids=ids)
def test_embed_range_matches_the_reference_on_border_picks(c):
    P, t0, max_t, sig, dt, trv, pairs, sets, S = _parts(c)
    ind, n_all = np.arange(S), S + 2
    rp = apply.ResidentPicks(P, ind, n_all, "cpu")
    t_sorted = np.sort(P[:, 0])
    on_lower = on_upper = 0
    for w in _starts(t0):
        want = E.window_pick_slice(P, w, ind, max_t, sig)
        lo, hi = rp.embed_range(w, max_t, sig)
        assert np.array_equal(P[np.sort(rp.index_host[lo:hi])], want)
        assert np.array_equal(rp.t[lo:hi].numpy(), np.sort(want[:, 0]))
        every = E.window_pick_slice(P, w, np.arange(n_all), max_t, sig)             # the range search itself, stations aside
        lo, hi = apply.picks_in_embed_range(t_sorted, w, max_t, sig)
        assert np.array_equal(t_sorted[lo:hi], np.sort(every[:, 0]))
        l2, h2 = apply._embed_ranges(t_sorted, np.array([w]), max_t, sig)
        assert (int(l2[0]), int(h2[0])) == (lo, hi)
        on_lower += int((P[:, 0] == w - 2 * sig).any())
        on_upper += int((P[:, 0] == w + max_t + 2 * sig).any())
    assert on_lower >= 4 and on_upper >= 4


@pytest.mark.parametrize("c", HOST_CASES, ids=ids)
def test_pick_inputs_match_the_reference_where_the_ball_query_cuts(c):
    P, t0, max_t, sig, dt, trv, pairs, sets, S = _parts(c)
    ind, n_all = np.arange(S), S + 2
    rp = apply.ResidentPicks(P, ind, n_all, "cpu")
    for w in _starts(t0):
        P_slice = E.window_pick_slice(P, w, ind, max_t, sig)
        for t_win in (2.0, 10.0):
            want = E.extract_pick_inputs_from_data(P_slice, n_all, ind, w, max_t, t_win=t_win)
            tp, ip, ph, idx = rp.pick_inputs(w, max_t, sig, t_win=t_win)
            for a, b in zip((tp.numpy(), ip.numpy(), ph.numpy(), rp.meta(idx)), want):
                assert a.shape == b.shape and np.array_equal(a, b)
            assert (len(want[0]) < len(P_slice)) == (t_win == 2.0)
    idx = rp.pick_inputs(t0, max_t, sig, t_win=2.0)[3].numpy()                        # exactly on the inclusive radius: kept; one step out: cut
    assert np.array_equal(np.sort(np.abs(P[sets["ball_on"], 0] - (t0 + max_t / 2.0))), [2.0 + max_t / 2.0] * 2)
    assert np.isin(sets["ball_on"], idx).all() and not np.isin(sets["ball_out"], idx).any()


@pytest.mark.parametrize("feed_order", [(0, 1, 2), (1, 0, 2)], ids=["in-order", "late-chunk"])
@pytest.mark.parametrize("c", HOST_CASES, ids=ids)
def test_pick_store_fed_in_chunks_that_split_runs_of_equal_times(c, feed_order):
    P, t0, max_t, sig, dt, trv, pairs, sets, S = _parts(c)
    ind, n_all = np.arange(S), S + 2
    Pt = P[np.argsort(P[:, 0], kind="stable")]
    valid = Pt[:, 1] < S
    run = np.nonzero((Pt[1:, 0] == Pt[:-1, 0]) & valid[1:] & valid[:-1])[0] + 1       # rows that continue a run of equal times
    cuts = [int(run[run > len(Pt) // 3][0]), int(run[run > 2 * len(Pt) // 3][0])]
    chunks = [Pt[:cuts[0]], Pt[cuts[0]:cuts[1]], Pt[cuts[1]:]]
    assert all(chunks[i][-1, 0] == chunks[i + 1][0, 0] for i in (0, 1))
    ps = apply.PickStore(ind, n_all, "cpu", capacity=64)
    fed = np.concatenate([chunks[i] for i in feed_order])
    for i in feed_order:
        ps.append(chunks[i])
    rp = apply.ResidentPicks(fed, ind, n_all, "cpu")
    assert np.array_equal(ps.index_host, rp.index_host) and np.array_equal(ps.t.numpy(), rp.t.numpy())
    assert np.array_equal(ps.sta.numpy(), rp.sta.numpy()) and np.array_equal(ps.phase.numpy(), rp.phase.numpy())
    for w in _starts(t0):
        P_slice = E.window_pick_slice(fed, w, ind, max_t, sig)
        lo, hi = ps.embed_range(w, max_t, sig)
        assert np.array_equal(fed[np.sort(ps.index_host[lo:hi])], P_slice)
        want = E.extract_pick_inputs_from_data(P_slice, n_all, ind, w, max_t, t_win=2.0)
        tp, ip, ph, idx = ps.pick_inputs(w, max_t, sig, t_win=2.0)
        for a, b in zip((tp.numpy(), ip.numpy(), ph.numpy(), ps.meta(idx)), want):
            assert a.shape == b.shape and np.array_equal(a, b)


def test_the_day_of_the_end_to_end_test_is_grid_aligned():
    P, trv = C.day()
    times = apply.window_schedule(P[:, 0], C.MAX_T, t_win=6.0, step_size="half")[0]
    assert np.array_equal(times, np.round(times)) and (times % 3.0 == 0).all() and 40 <= len(times) <= 60
    assert 110.0 <= P[-1, 0] - P[0, 0] <= 120.0 and (np.diff(P[:, 0]) >= 0).all() and (P[:, 1] < C.SHAPES["14x60"][0]).all()
    lo, hi = apply._embed_ranges(P[:, 0], times, C.MAX_T, C.SIGMA)
    ties = [C.tie_counts(C.scatter_quotients(P[a:b, 0], t0, C.SIGMA, 0.3)) for t0, a, b in zip(times, lo, hi) if b > a]
    on_border = sum(int((P[:, 0] == t0 - 2 * C.SIGMA).any()) + int((P[:, 0] == t0 + C.MAX_T + 2 * C.SIGMA).any()) for t0 in times)
    print("day: %d windows, near ties per window %d..%d below and %d..%d on or above; %d window borders carry a pick"
          % (len(ties), min(t[0] for t in ties), max(t[0] for t in ties), min(t[1] for t in ties), max(t[1] for t in ties), on_border))
    assert sum(t[0] for t in ties) >= 20 * 5 and sum(t[1] for t in ties) >= 20 * 5 and on_border >= 6
