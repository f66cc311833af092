"""Windows, images and references shared by the window sharpness tests (CPU and
GPU): the Python big-integer restatement of the header's definition, the host
twin's call, and the window lists.

Bars against oracle.sharpness: FLOAT_RTOL and TIGHT_RTOL of tests/sharp_boxes.py
on every compared window, none left out; every compared window has S1 > 0
(asserted on the twin's sums), so the oracle's own average is away from 0."""
import ctypes
import functools

import numpy as np

from tests.sharp_boxes import KINDS, assert_sharp

SIZES = (16, 32, 64, 128)
H, W = 353, 350                       # the kinds' image size
ODD_H, ODD_W = 131, 197               # 3 * W = 591: every row at another byte phase


def boxes_as_dicts(boxes):
    return [dict(top=int(t), bottom=int(b), left=int(l), right=int(r)) for t, b, l, r in boxes]


def grid4(h, w, T):
    """A 4 x 4 grid of T x T windows spread over h x w (overlapping where they
    must), then the flush bottom-right window once more."""
    tops = np.linspace(0, h - T, 4).astype(int)
    lefts = np.linspace(0, w - T, 4).astype(int)
    return [(int(t), int(t) + T, int(l), int(l) + T) for t in tops for l in lefts] + [(h - T, h, w - T, w)]


def odd_windows(T, h=ODD_H, w=ODD_W):
    """Windows of the 131 x 197 image: left = 0, 1, 2, 3 (mod 4), touching the right
    and the bottom edge, overlapping, one duplicated (the last two)."""
    wins = [(0, T, l, l + T) for l in (0, 1, 2, 3) if l + T <= w]
    wins += [(1, 1 + T, l, l + T) for l in (4, 5, 6, 7) if l + T <= w and 1 + T <= h]
    wins += [(h - T, h, w - T, w), (h - T, h, 0, T), (0, T, w - T, w), ((h - T) // 2, (h - T) // 2 + T, w - T - 1, w - 1)]
    wins += [wins[1], wins[1]]
    assert {l % 4 for _, _, l, _ in wins} == {0, 1, 2, 3}
    return wins


@functools.lru_cache(maxsize=None)
def kind_image(kind, h=H, w=W, seed=11):
    from photohive_dsp_amd import synth
    img = np.ascontiguousarray(synth.make(kind, h, w, seed))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def odd_image():
    return kind_image("uniform", ODD_H, ODD_W, 23)


def bigint_window(img, box):
    """The header's definition in Python integers and the finish's three rows in
    Python floats (IEEE doubles): (sharpness, variance, S1, S2, D)."""
    t, b, l, r = box
    T = b - t
    c = img[t:b, l:r].astype(np.int64)
    lum = 299 * c[..., 0] + 587 * c[..., 1] + 114 * c[..., 2]
    pad = np.zeros((T + 2, T + 2), np.int64)
    pad[1:-1, 1:-1] = lum
    box9 = sum(pad[dy:dy + T, dx:dx + T] for dy in range(3) for dx in range(3))
    f = 9 * lum - box9
    assert int(np.abs(f).max()) <= 2_040_000
    n, S1, S2 = T * T, int(f.sum()), int((f * f).sum())     # f * f < 2^42: the int64 sums are exact
    assert S1 >= 0
    D = n * S2 - S1 * S1
    assert D >= 0
    hi, lo = D >> 64, D & (2 ** 64 - 1)
    num = float(hi) * 18446744073709551616.0 + float(lo)
    with np.errstate(divide="ignore", invalid="ignore"):
        sharp = float(np.float64(num) / np.float64((float(n) * float(S1)) * 255000.0))
    var = num / ((float(n) * float(n)) * 65025000000.0)
    return sharp, var, S1, S2, D


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def boundaries(boxes):
    from photohive_dsp_amd.core import window_boundaries
    return window_boundaries(boxes)


def host_twin(img, boxes, window, variance=True, sums=True):
    """phd_debug_window_sharpness_host: (sharpness, variance, sums [n, 2]) or the
    error text."""
    from photohive_dsp_amd import lib as L
    img = np.ascontiguousarray(img, np.uint8)
    cb = boundaries(boxes)
    n = len(boxes)
    s = np.full(n, -1.0)
    v = np.full(n, -1.0) if variance else None
    u = np.zeros((n, 2), np.uint64) if sums else None
    rc = L.lib.phd_debug_window_sharpness_host(img.ctypes.data, img.shape[0], img.shape[1], ctypes.byref(cb), window,
                                               s.ctypes.data, v.ctypes.data if variance else None,
                                               u.ctypes.data if sums else None)
    if rc != 0:
        assert rc == -1
        return L.last_error()
    return s, v, u


def assert_against_oracle(img, boxes, got, sums):
    """Both bars on every window; the border ring of each is not black."""
    from oracle import oracle as orc
    assert np.all(np.asarray(sums)[:, 0] > 0), "a compared window has S1 == 0"
    assert_sharp(got, orc.sharpness(np.asarray(img), boxes_as_dicts(boxes)))


# ---- special windows ----------------------------------------------------------------------
def special_window(name, T):
    w = np.zeros((T, T, 3), np.uint8)
    if name == "black":
        pass
    elif name == "black_ring":                       # content inside a black border ring
        w[1:-1, 1:-1] = np.arange((T - 2) * (T - 2) * 3, dtype=np.int64).reshape(T - 2, T - 2, 3) * 37 % 251
    elif name == "grey":
        w[...] = 128
    elif name == "white":
        w[...] = 255
    elif name == "corner":                           # one white pixel at (0, 0)
        w[0, 0] = 255
    else:
        raise KeyError(name)
    return w


SPECIALS = ("black", "black_ring", "grey", "white", "corner")
