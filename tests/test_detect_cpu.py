"""CPU: the rule the device LocalMarching implements (csrc/detect_kernels.hpp, include/genie_hip.h), restated densely in numpy and held
against the host `postproc.local_marching` (itself pinned to the reference's class by tests/golden/localmarching.npz) before any GPU is
involved; and the C ABI of the three device stages of source detection. Everything is compare work: results are equal, not close."""
import os
import re

import numpy as np

from genie_amd import _lib, postproc

DETECT_SYMBOLS = ("genie_peak_distance", "genie_time_groups", "genie_local_marching")
TC_WIN, SP_WIN, DT_WIN = 6.75, 27e3, 0.75                       # tc_win = 9 x 0.75 s: pairs exactly on the time radius are common
ORIGINS = (0.0, 1234.56, 1.6e9 + 0.1)                           # grid origins: zero, a two-decimal offset, an epoch-sized offset


def dense_local_marching(srcs, ftrns1, tc_win, sp_win, n_steps_max, tol=1e-12, scale_depth=1.0, use_directed=True, group=None):
    """The pair rule as the header words it, on [n, n] arrays: j is an in-neighbour of i when (t_i - t_j)^2 <= tc_win^2 and
    ((dx0^2 + dx1^2) + dx2^2) <= sp_win^2 in fp64 (numpy does not fuse), same group; active = has a neighbour other than itself;
    directed keeps val0[i] <= val0[j]; a step takes max(0, max over in-neighbours) in fp32. Returns the keep flags."""
    srcs = np.asarray(srcs, dtype=np.float64)
    xs = ftrns1(srcs[:, 0:3]) * np.array([1.0, 1.0, scale_depth]).reshape(1, -1)
    t = srcs[:, 3]
    dt = t[:, None] - t[None, :]
    d0, d1, d2 = (xs[:, None, k] - xs[None, :, k] for k in range(3))
    A = (dt * dt <= tc_win * tc_win) & (((d0 * d0 + d1 * d1) + d2 * d2) <= sp_win * sp_win)
    if group is not None:
        A &= group[:, None] == group[None, :]
    v0 = srcs[:, 4].astype(np.float32)
    active = A.sum(1) > 1
    if use_directed:
        A = A & (v0[:, None] <= v0[None, :])
    vals = v0.copy()
    for _ in range(int(n_steps_max)):
        new = np.where(A, vals[None, :], np.float32(0)).max(1)
        new = np.where(active, new, vals)
        done = float(np.abs(new - vals).max()) <= tol
        vals = new
        if done:
            break
    return ~active | (np.abs(v0 - vals) <= 1e-8 + tol * np.abs(vals))


def marching_cases(n_cases=60, seed=0):
    """Seeded cases (srcs [n, 5] sorted by time, kwargs of local_marching): times on the 0.75 s grid from three origins, values
    rounded to two decimals (ties) or not, n_steps_max in {1, 2, 3, 100}, both edge directions."""
    rng = np.random.default_rng(seed)
    steps = (2, 1, 100, 3)
    for k in range(n_cases):
        n = int(rng.integers(2, 500))
        grid = ORIGINS[k % 3] + np.arange(400) * DT_WIN
        xq = np.c_[rng.uniform(0, 120e3, (300, 2)), rng.uniform(-40e3, 0, 300)]
        val = np.round(rng.uniform(0.15, 1, n), 2 if k % 2 else 7).astype(np.float32)
        srcs = np.c_[xq[rng.integers(0, 300, n)], grid[rng.integers(0, 80, n)], val]
        srcs = srcs[np.argsort(srcs[:, 3], kind="stable")]
        yield srcs, dict(tc_win=TC_WIN, sp_win=SP_WIN, scale_depth=0.2, n_steps_max=steps[(k // 2) % 4], use_directed=bool((k // 8) % 2))


def pairs_on_time_radius(srcs, tc_win=TC_WIN):
    """Ordered pairs whose time difference is the radius itself up to the rounding of the grid (far below the grid step)."""
    return int((np.abs(np.abs(srcs[:, None, 3] - srcs[None, :, 3]) - tc_win) < 1e-6).sum())


def test_detect_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(_lib.INCLUDE, "genie_hip.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in DETECT_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in genie_hip.h"
        assert name in bound, name + " is not in _lib.SYMBOLS"
        assert getattr(lib, name).restype is not None


def test_dense_rule_equals_host_local_marching():
    ident = lambda x: x
    n_cases, on_radius, seen = 0, 0, set()
    for srcs, kw in marching_cases():
        want = postproc.local_marching(srcs, ident, **kw)
        keep = dense_local_marching(srcs, ident, **kw)
        assert np.array_equal(srcs[keep], want), (n_cases, kw)
        assert 0 < keep.sum()
        on_radius += pairs_on_time_radius(srcs)
        seen.add((kw["n_steps_max"], kw["use_directed"]))
        n_cases += 1
    assert n_cases >= 50 and on_radius > 1000                  # the inclusive radius is decided, not avoided
    assert seen == {(s, d) for s in (1, 2, 3, 100) for d in (False, True)}


def test_dense_rule_marches_somewhere():
    """The cases are not trivial: nodes are removed, and some marches need more than one step."""
    ident = lambda x: x
    removed = multi = 0
    for srcs, kw in marching_cases(12):
        k100 = dense_local_marching(srcs, ident, **dict(kw, n_steps_max=100))
        removed += int((~k100).sum())
        multi += int(not np.array_equal(k100, dense_local_marching(srcs, ident, **dict(kw, n_steps_max=1))))
    assert removed > 100 and multi > 0
