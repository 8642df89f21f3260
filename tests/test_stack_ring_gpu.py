"""GPU: the ring form of the stacking kernel (genie_stack_windows_ring through `engine.stack_windows_ring`) against the dense form
(`engine.stack_windows_legs`) bit for bit, the refusal of a range that spans the ring, and genie_ring_close (`engine.ring_close`)."""
import numpy as np
import pytest
import torch

from genie_amd import _lib, engine

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
Q, T, N_COLS = 37, 9, 400


def _case(n, legs, seed, c0=150):
    """n windows at a stride of two columns from column c0: overlapping columns inside the call; -1 entries, and window 0 lists one
    column twice."""
    rng = np.random.default_rng([n, legs, seed])
    cols = (c0 + 2 * np.arange(n).reshape(-1, 1) + np.arange(T).reshape(1, -1)).astype(np.int32)
    cols[rng.random(cols.shape) < 0.15] = -1
    cols[0, 2], cols[0, 5] = c0 + 3, c0 + 3
    xs = [torch.from_numpy(rng.random((n, Q, T, 1)).astype(np.float32)).to(DEV) for _ in range(legs)]
    used = cols[cols >= 0]
    return xs, cols, int(used.min()), int(used.max())


@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("legs", [1, 2])
def test_ring_stacking_is_bit_equal_to_dense_stacking(n, legs):
    """Two calls in a row into the same targets (a column's sum continues across launches), W = 50 against columns 150..: the range of
    the 16-window call, 39 columns from column 150, wraps the ring's end (150 % 50 = 0 for the first call, 172 % 50 = 22 for the next)."""
    W = 50
    rng = np.random.default_rng(n)
    start = torch.from_numpy(rng.random((Q, N_COLS)).astype(np.float32)).to(DEV)
    dense = start.clone()
    ring = torch.zeros((Q, W), dtype=torch.float32, device=DEV)
    wrapped = False
    for call, c0 in enumerate((150, 172)):
        xs, cols, c_min, c_max = _case(n, legs, call, c0)
        ring[:, torch.arange(c_min, c_min + W, device=DEV) % W] = dense[:, c_min:c_min + W]      # the ring holds the open columns
        d_cols = torch.from_numpy(cols).to(DEV)
        engine.stack_windows_legs(dense, xs, d_cols, 1.0 / 6.0, c_min, c_max)
        engine.stack_windows_ring(ring, xs, d_cols, 1.0 / 6.0, c_min, c_max)
        torch.cuda.synchronize()
        wrapped |= c_min % W > c_max % W
        for c in range(c_min, c_min + W):
            assert torch.equal(ring[:, c % W], dense[:, c]), (call, c)
        assert not torch.equal(dense[:, c_min:c_max + 1], start[:, c_min:c_max + 1])
    assert wrapped or n < 16


def test_a_range_that_spans_the_ring_is_refused_and_writes_nothing():
    xs, cols, c_min, c_max = _case(16, 2, 0)
    W = c_max - c_min                                                     # one slot short
    ring = torch.full((Q, W), 3.0, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.GenieHipError) as err:
        engine.stack_windows_ring(ring, xs, torch.from_numpy(cols).to(DEV), 0.5, c_min, c_max)
    torch.cuda.synchronize()
    assert "genie_stack_windows_ring" in str(err.value) and bool((ring == 3.0).all())
    ring = torch.zeros((Q, W + 1), dtype=torch.float32, device=DEV)       # the smallest ring that takes the call
    dense = torch.zeros((Q, N_COLS), dtype=torch.float32, device=DEV)
    engine.stack_windows_ring(ring, xs, torch.from_numpy(cols).to(DEV), 0.5, c_min, c_max)
    engine.stack_windows_legs(dense, xs, torch.from_numpy(cols).to(DEV), 0.5, c_min, c_max)
    assert torch.equal(ring[:, torch.arange(c_min, c_max + 1, device=DEV) % (W + 1)], dense[:, c_min:c_max + 1])


@pytest.mark.parametrize("c_lo,c_hi", [(100, 100), (100, 101), (103, 140), (130, 165), (150, 200), (149, 199)])
def test_ring_close_returns_the_block_and_zeroes_its_slots(c_lo, c_hi):
    """W = 50: [130, 165) and [149, 199) wrap the ring's end; [150, 200) is the whole ring."""
    W = 50
    rng = np.random.default_rng(c_lo)
    ring = torch.from_numpy(rng.random((Q, W)).astype(np.float32) + 1.0).to(DEV)
    before = ring.clone()
    block = engine.ring_close(ring, c_lo, c_hi)
    torch.cuda.synchronize()
    slots = torch.arange(c_lo, c_hi, device=DEV) % W
    assert block.shape == (Q, c_hi - c_lo) and torch.equal(block, before[:, slots])
    assert bool((ring[:, slots] == 0).all())
    rest = torch.ones(W, dtype=torch.bool, device=DEV)
    rest[slots] = False
    assert torch.equal(ring[:, rest], before[:, rest])
    with pytest.raises(ValueError):
        engine.ring_close(ring, c_lo, c_lo + W + 1)
    lib = _lib.load()
    assert lib.genie_ring_close(ring.data_ptr(), Q, W, c_lo, c_lo + W + 1, block.data_ptr(), None) == -1      # GENIE_ERR_ARG
    assert b"genie_ring_close" in lib.genie_last_error()
