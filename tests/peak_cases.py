"""The planted-plateau matrix that the band and the stream candidate kernels are pinned to `row_select` on, and the triplet helpers of
those tests (a plain module, not a conftest; the matrix goes to a GPU).

`matrix(rows, n_cols, seed, device, streamed)`: seeded noise on 8 levels (k / 8, k < 8: runs, ties and flat tops everywhere) plus the
planted cases the sizes have room for, one row each:

* BAND_ROW (needs n_cols >= 3): a peak at global column 1 and one at n_cols - 2; from n_cols >= 40 an even flat top on columns 10..13,
  an odd one on 20..22 and a peak of exactly the threshold at column 30;
* STREAM_ROW (needs n_cols >= 64): a flat top on columns 18..25 (midpoint 21), a top of exactly the threshold on 41..42 (midpoint 41)
  and a peak at column 62, whose right neighbour is the last lane of the first chunk;
* row 1: runs that hold column 0 and column n_cols - 1 (no peaks; on an axis of up to 6 columns they are one run over all of it); from
  n_cols >= 40 steps on a slope at columns 9..14 (flat, at a cut undecidable, no peak) and a run on 20..25 below its left neighbour
  (decidable, no peak); from n_cols >= 64 a second slope on 30..35;
* row 2: all zero;
* row 3: one run over the whole axis (no peak; a band that touches neither end of the axis cannot decide it and flags).

BAND_ROW and STREAM_ROW cannot share a row: both centre a flat top on column 21, of different lengths, the band test counts on cuts
20 and 23 being decidable in a one-row matrix, and with n_cols = 65 one asks for a peak at column 62 and the other at column 63.
So one of them is row 0 and the other row 4, and `streamed` says which: False puts BAND_ROW first, True STREAM_ROW. That order is all
the flag changes; a matrix of five rows or more holds every case. A case whose row the matrix does not have is left out.

The matrix is returned as (host array, GPU view); the view lies inside a wider buffer, so that it and every band or block cut from it
have a row stride larger than their width."""
import numpy as np
import torch

TOP = 0.9375                        # above every level of the quantised noise (k / 8, k < 8)
THR = 0.5                           # one of those levels: a value equal to the threshold is common


def _band_row(x, r):
    n_cols = x.shape[1]
    if n_cols >= 3:
        x[r, 0], x[r, 1], x[r, 2] = 0.0, TOP, 0.0                          # a peak at global column 1 ...
        x[r, n_cols - 3], x[r, n_cols - 2], x[r, n_cols - 1] = 0.0, TOP, 0.0      # ... and at n_cols - 2
    if n_cols >= 40:
        x[r, 9:15] = [0.0, TOP, TOP, TOP, TOP, 0.0]                        # an even flat top, columns 10..13
        x[r, 19:24] = [0.0, TOP, TOP, TOP, 0.0]                            # an odd one, columns 20..22
        x[r, 29:32] = [0.25, THR, 0.25]                                    # a peak of exactly the threshold


def _stream_row(x, r):
    if x.shape[1] >= 64:
        x[r, 17:27] = [0.0, TOP, TOP, TOP, TOP, TOP, TOP, TOP, TOP, 0.0]   # a flat top on columns 18..25: midpoint 21
        x[r, 40:44] = [0.25, THR, THR, 0.25]                               # a top of exactly the threshold, midpoint 41
        x[r, 61:64] = [0.0, TOP, 0.0]                                      # a peak next to the last lane of the first chunk


def matrix(rows, n_cols, seed, device, streamed):
    rng = np.random.default_rng(seed)
    x = (np.floor(rng.random((rows, n_cols)) * 8.0) / 8.0).astype(np.float32)
    first, second = (_stream_row, _band_row) if streamed else (_band_row, _stream_row)
    first(x, 0)
    if rows >= 2:
        x[1, 0:min(3, n_cols)] = TOP                                       # runs that hold column 0 / column n_cols - 1: no peaks
        x[1, max(n_cols - 3, 0):] = TOP                                    # (up to 6 columns: one run over the whole axis)
        if n_cols >= 40:
            x[1, 9:15] = [0.25, THR, THR, 0.75, 0.75, 1.0]                 # steps on a slope: flat, at a cut undecidable, no peak
            x[1, 19:27] = [1.0, TOP, TOP, TOP, TOP, TOP, TOP, 0.0]         # a run below its left neighbour: decidable, no peak
        if n_cols >= 64:
            x[1, 3], x[1, n_cols - 4] = 0.0, 0.0
            x[1, 30:36] = [0.25, THR, THR, 0.75, 0.75, 1.0]                # steps on a slope: no peak
    if rows >= 3:
        x[2, :] = 0.0                                                      # an all-zero row
    if rows >= 4:
        x[3, :] = TOP                                                      # a run that covers the whole axis
    if rows >= 5:
        second(x, 4)
    buf = torch.zeros((rows, n_cols + 5), dtype=torch.float32, device=device)
    buf[:, 2:2 + n_cols] = torch.from_numpy(x).to(device)
    return x, buf[:, 2:2 + n_cols]


def trip(r, c, v):
    """GPU triplets (row, col, value) as one host int32 array [n, 3]: the values by their bits."""
    return np.stack((r.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy().view(np.int32)), axis=1).reshape(-1, 3)


def by_row_col(t):
    return t[np.lexsort((t[:, 1], t[:, 0]))]
