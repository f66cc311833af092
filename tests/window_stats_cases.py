"""Windows, images and references shared by the window statistics tests (CPU and
GPU): the host twin's call, the reference's restatement per window, the special
windows and their hand values.

Exact expectations and tolerances are the box statistics' own
(tests/box_stats_cases.py: expected_sums, expected_u8, expected_doubles,
assert_close -- DESIGN.md section 23's bars); window lists and images are the
window sharpness tests' (tests/window_sharp_cases.py)."""
import ctypes
import math

import numpy as np

from tests import box_stats_cases as bsc
from tests.window_sharp_cases import (SIZES, boundaries, grid4, kind_image, odd_image,  # noqa: F401  (re-exported)
                                      odd_windows)

H, W = 353, 350                       # random_image's size: every case of the saturation formula
REC = bsc.REC
CONST = (37, 121, 200)
SPECIALS = ("black", "constant", "white", "blue", "one_white")


def bits(a):
    return bsc.bits(a)


def same_bits(got, want, what=""):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def host_twin(img, boxes, window, sums=True):
    """phd_debug_window_stats_host over a uint8 image at any base: ([n, 7] values,
    [n][264] sums as Python integers or None), or the error text."""
    from photohive_dsp_amd import lib as L
    assert img.dtype == np.uint8 and img.flags.c_contiguous
    cb = boundaries(boxes)
    n = len(boxes)
    vals = np.full((max(n, 1), 7), np.nan)
    rec = np.full((max(n, 1), REC), 0xDEADBEEF, np.uint64)
    rc = L.lib.phd_debug_window_stats_host(img.ctypes.data, img.shape[0], img.shape[1], ctypes.byref(cb), window,
                                           vals.ctypes.data, rec.ctypes.data if sums else None)
    if rc != 0:
        assert rc == -1
        return L.last_error()
    return vals[:n], ([[int(v) for v in row] for row in rec[:n]] if sums else None)


def reference_values(img, boxes):
    """[n, 7]: oracle.stats (the reference's get_rgb_statistics restated in C) on
    each window's crop, and expected_doubles' S-bar on the crop's k / 255.0."""
    from oracle import oracle as orc
    img = np.asarray(img)
    out = bsc.expected_doubles(img.astype(np.float64) / 255.0, boxes)
    for k, (t, b, l, r) in enumerate(boxes):
        out[k, :6] = orc.stats(np.ascontiguousarray(img[t:b, l:r]))
    return out


def contrast_rule(got, want, what=""):
    """The three contrasts against the twin's.  Bit for bit: the argument of sqrt
    comes from the shared rows and fp64 sqrt without fast-math flags is correctly
    rounded on gfx950 (observed on the MI355X)."""
    same_bits(np.asarray(got)[..., 3:6], np.asarray(want)[..., 3:6], f"{what}: contrast bits")


def assert_device(img, boxes, got, what, oracle=True):
    """The bar of every GPU test: brightness and S-bar bit for bit the twin's, the
    contrasts by contrast_rule, all seven against the reference's restatement."""
    twin = host_twin(np.ascontiguousarray(img), boxes, boxes[0][1] - boxes[0][0], sums=False)
    assert not isinstance(twin, str), twin
    want = twin[0]
    got = np.asarray(got).reshape(len(boxes), 7)
    same_bits(got[:, :3], want[:, :3], f"{what}: brightness bits")
    same_bits(got[:, 6], want[:, 6], f"{what}: S-bar bits")
    contrast_rule(got, want, what)
    if oracle:
        bsc.assert_close(got, reference_values(img, boxes), boxes, what)
    return want


# ---- special windows ----------------------------------------------------------------------
def special_window(name, T):
    w = np.zeros((T, T, 3), np.uint8)
    if name == "black":
        pass
    elif name == "constant":
        w[...] = CONST
    elif name == "white":
        w[...] = 255
    elif name == "blue":
        w[..., 2] = 255
    elif name == "one_white":                        # one white pixel, not at a corner
        w[T // 3, T // 2] = 255
    else:
        raise KeyError(name)
    return w


def special_image(T):
    """The special windows side by side inside an image of 255s, and their boxes."""
    img = np.full((T + 9, len(SPECIALS) * (T + 3) + 4, 3), 255, np.uint8)
    boxes = []
    for k, name in enumerate(SPECIALS):
        l = 3 + k * (T + 3)
        img[4:4 + T, l:l + T] = special_window(name, T)
        boxes.append((4, 4 + T, l, l + T))
    return img, boxes


def assert_special_values(vals, T):
    """The hand values of the special windows, from the header's formulas."""
    by = dict(zip(SPECIALS, np.asarray(vals).reshape(len(SPECIALS), 7)))
    n = T * T
    fn = float(n)
    assert not by["black"].any() and not np.signbit(by["black"]).any()
    c = by["constant"]
    assert (c[3:6] == 0.0).all()
    assert [float(v) for v in c[:3]] == [float(k * n) / 255.0 / fn for k in CONST]
    assert float(c[6]) == (float(163 * n) / 200.0) / fn             # max 200, d 163, no zero channel
    wh = by["white"]
    assert (wh[:3] == 1.0).all() and (wh[3:6] == 0.0).all() and wh[6] == 0.0
    bl = by["blue"]
    assert float(bl[6]) == (fn - (1.0 - 0.999999) * fn) / fn         # D[255] = 255 n: S = n; n1 = n
    assert list(bl[:6]) == [0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    # one white pixel: M = 255, sum k^2 = 65025 per channel; d = 0
    ow = by["one_white"]
    assert [float(v) for v in ow[:3]] == [255.0 / 255.0 / fn] * 3 == [1.0 / fn] * 3
    want_c = math.sqrt(float(n * 65025 - 255 * 255) / 65025.0 / (fn * fn))
    assert [float(v) for v in ow[3:6]] == [want_c] * 3
    assert abs(want_c - math.sqrt(n - 1.0) / n) <= 2.0 ** -52 * want_c
    assert ow[6] == 0.0
