"""Crop boxes shared by the batched-sharpness tests (CPU and GPU).

The twelve boxes are written for 480 x 640 and rescaled to each size so that
the flush ones stay flush: single pixels at two corners, a one-pixel row and
column, the whole image, boxes one pixel larger than a 64 x 16 tile and exactly
one tile, a duplicate, a box flush with the bottom-right corner.  None has an
all-black border ring on the synthetic kinds used (its mean Laplacian would be
0 and var / mean rounding noise in the reference itself)."""
import numpy as np

FLOAT_RTOL = 1e-4          # the contract (tests/test_gpu_parity.py)
TIGHT_RTOL = 1e-9          # the tracked bar
KINDS = ["uniform", "structured", "hblur", "dominant", "grayish"]


def box(top, bottom, left, right):
    return {"top": int(top), "bottom": int(bottom), "left": int(left), "right": int(right)}


def twelve(h, w):
    mid = box(100 * h // 480, 357 * h // 480, 200 * w // 640, 329 * w // 640)
    return [
        box(0, 1, 0, 1),                       # 1 x 1 at (0, 0)
        box(0, 1, 0, w),                       # 1 x W top row
        box(0, h, w - 1, w),                   # H x 1 last column
        box(0, h, 0, w),                       # the whole image
        box(h - 1, h, w - 1, w),               # 1 x 1 at the bottom-right corner
        box(7, 24, 3, 68),                     # 17 x 65: one more than a tile wide and high
        mid,
        dict(mid),                             # the same box again
        box(h - 17, h, w - 65, w),             # flush bottom-right
        box(1, 3, 1, 3),                       # 2 x 2 at (1, 1)
        box(30, 33, 0, w),                     # 3 x W at row 30
        box(200, 216, 64, 128),                # exactly one tile
    ]


def three(h, w):
    return [box(5, h // 2, 9, w // 3), box(h // 3, h, 0, w - 1), box(h - 40, h - 1, w - 200, w - 3)]


def assert_sharp(got, want):
    """both bars; `want` is the oracle's (finite, mean away from 0: asserted)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.isfinite(want))
    nz = want != 0                                   # (a single pixel has variance 0: both sides exactly 0)
    if nz.any():
        print("sharpness worst relative difference", float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))))
    np.testing.assert_allclose(got, want, rtol=FLOAT_RTOL, atol=0)
    np.testing.assert_allclose(got, want, rtol=TIGHT_RTOL, atol=0)
