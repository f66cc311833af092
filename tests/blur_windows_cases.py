"""Shared by the window blur tests and the fixture maker: the cases, their images
and windows, the special-pattern image, the C oracle on a window's crop, the
bars (all from tests/test_gpu_parity.py) and the calls into the library."""
import ctypes
import functools
import json
import os

import numpy as np

from tests.test_gpu_parity import BINS_NORMWISE, BINS_TIGHT_RTOL, TIGHT_RTOL

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
MAX_BINS = 2880            # blur_window.h: kWinMaxBins
BLUR_KW = dict(fft_streak_thresh=1.20, magnitude_thresh=0.3, blur_cutoff_ratio_denom=2)   # the report's defaults

# (name, synth kind, height, width, seed, window, radius_partitions, angle_partitions, windows)
TILE = 128


def _spread(T, h=300, w=333):
    """Eight windows over an h x w image: corners, edges, odd offsets."""
    return [(t, t + T, l, l + T) for t, l in ((0, 0), (3, 7), (h - T, w - T), (100, 101), (50, 2), (h - T, 0),
                                               (120, 200 - T // 2), (17, 150))]


CASES = [
    ("hblur_128_16x36", "hblur", 300, 333, 31, 128, 16, 36,
     [(0, 128, 0, 128), (3, 131, 7, 135), (172, 300, 205, 333), (100, 228, 101, 229), (50, 178, 2, 130),
      (172, 300, 0, 128)]),
    ("special_128_16x36", "special", 256, 512, 0, 128, 16, 36,
     [(TILE * (k // 4), TILE * (k // 4) + 128, TILE * (k % 4), TILE * (k % 4) + 128) for k in range(8)]),
    ("uniform_128_8x18", "uniform", 200, 261, 32, 128, 8, 18, [(0, 128, 0, 128), (72, 200, 133, 261), (31, 159, 66, 194)]),
    ("vblur_128_40x72", "vblur", 300, 333, 33, 128, 40, 72, [(5, 133, 9, 137), (172, 300, 205, 333)]),
    ("dominant_64_16x36", "dominant", 200, 231, 34, 64, 16, 36,
     [(0, 64, 0, 64), (78, 142, 13, 77), (90, 154, 167, 231), (136, 200, 167, 231), (100, 164, 50, 114),
      (136, 200, 0, 64)]),
    ("special_64_8x18", "special", 256, 512, 0, 64, 8, 18,
     [(TILE * (k // 4), TILE * (k // 4) + 64, TILE * (k % 4), TILE * (k % 4) + 64) for k in range(8)]),
    ("hblur_64_16x36", "hblur", 300, 333, 35, 64, 16, 36,
     [(0, 64, 0, 64), (3, 67, 7, 71), (236, 300, 269, 333), (100, 164, 101, 165)]),
    ("vblur_64_8x18", "vblur", 300, 333, 36, 64, 8, 18,
     [(0, 64, 0, 64), (236, 300, 269, 333), (100, 164, 101, 165), (50, 114, 2, 66), (120, 184, 200, 264),
      (17, 81, 150, 214)]),
    ("motion_128_16x36", "motion", 300, 333, 41, 128, 16, 36, _spread(128)),
    ("motion_128_8x18", "motion", 300, 333, 42, 128, 8, 18, _spread(128)),
    ("motion_64_8x18", "motion", 300, 333, 43, 64, 8, 18, _spread(64)),
]

# the special image's 128 x 128 tiles, row-major over 2 x 4
# (a constant grey is not among them: its every p is rounding noise, 8e-25 at most from the exact channel sums
# and 9e-18 from the reference's sequential fp64 means, so its fft_max has no relative bar; its all-zero bins are
# checked without a fixture)
SPECIAL_TILES = ("colour", "black", "white", "one_pixel", "h_stripes", "v_stripes", "checkerboard", "noise")


def special_tile(name, T=TILE):
    """One T x T x 3 pattern: a constant colour, a constant grey, black and white
    (the last three: every p < 1, all-zero bins), one bright pixel on black, horizontal and vertical 1-px
    stripes and a checkerboard (energy in the Nyquist row, the Nyquist column
    and the corner), and noise."""
    yy, xx = np.mgrid[0:T, 0:T]
    if name == "colour":                              # constant: luma - avg is a constant, only the DC term is left
        return np.ascontiguousarray(np.broadcast_to(np.array([200, 50, 50], np.uint8), (T, T, 3)))
    if name == "grey":
        g = np.full((T, T), 119)
    elif name == "black":
        g = np.zeros((T, T), np.int64)
    elif name == "white":
        g = np.full((T, T), 255)
    elif name in ("one_pixel", "one_pixel_255"):
        # one pixel of luma v on black: |X| = v everywhere but at DC.  254 keeps every p below 1; 255 puts
        # every p on the p >= 1 threshold itself, where rounding decides (bins of 1e-16 at most)
        g = np.zeros((T, T), np.int64)
        g[40, 50] = 254 if name == "one_pixel" else 255
    elif name == "h_stripes":
        g = (yy & 1) * 255
    elif name == "v_stripes":
        g = (xx & 1) * 255
    elif name == "checkerboard":
        g = ((xx + yy) & 1) * 255
    else:
        from photohive_dsp_amd import synth
        return synth.uniform(T, T, 77)
    return np.repeat(g.astype(np.uint8)[..., None], 3, axis=2)


def special_image():
    rows = [np.concatenate([special_tile(n) for n in SPECIAL_TILES[4 * r:4 * r + 4]], axis=1) for r in range(2)]
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def manifest():
    with open(os.path.join(GOLDEN, "blur_windows_manifest.json")) as f:
        return json.load(f)["cases"]


def fixture(name):
    with np.load(os.path.join(GOLDEN, f"blur_windows_{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _image(kind, h, w, seed):
    if kind == "special":
        img = special_image()
        assert img.shape == (h, w, 3)
        return img
    from photohive_dsp_amd import synth
    return np.ascontiguousarray(synth.make(kind, h, w, seed))


def case_image(case):
    return _image(case["kind"], case["height"], case["width"], case["seed"])


def case_kw(case):
    return dict(radius_partitions=case["radius_partitions"], angle_partitions=case["angle_partitions"])


# ---- the C oracle on a window's crop ----------------------------------------------------
def oracle_window(img, box, nr, na, kw=BLUR_KW):
    """bins [na, nr], angles [10], mags [10], fft_max, angle and radius bin size."""
    from oracle import oracle as orc
    t, b, l, r = box
    crop = np.ascontiguousarray(img[t:b, l:r])
    st = orc.stats(crop)
    avg = (st[0] + st[1] + st[2]) / 3.0
    power = orc.power_spectrum(orc.pgm_dc(crop, avg))
    bins, _counts, fmax, abs_, rbs = orc.blur_profile(power, nr, na)
    ang, mag = orc.vectorize(bins, kw["fft_streak_thresh"], kw["magnitude_thresh"], kw["blur_cutoff_ratio_denom"])
    return bins, ang, mag, fmax, abs_, rbs


def oracle_windows(img, boxes, nr, na):
    res = [oracle_window(img, b, nr, na) for b in boxes]
    return (np.array([r[0] for r in res]).reshape(len(boxes), na, nr), np.array([r[1] for r in res], np.int32),
            np.array([r[2] for r in res], np.float32), np.array([r[3] for r in res]))


def vectorize(bins, kw=BLUR_KW):
    from oracle import oracle as orc
    return orc.vectorize(bins, kw["fft_streak_thresh"], kw["magnitude_thresh"], kw["blur_cutoff_ratio_denom"])


# ---- the bars ----------------------------------------------------------------------------
def bins_errors(got, want):
    """(normwise, largest relative difference over the bins outside atol)."""
    got, want = np.asarray(got), np.asarray(want)
    scale = max(float(np.max(np.abs(want))), 1e-300)
    d = np.abs(got - want)
    rel = np.where(d > 1e-13, d / np.maximum(np.abs(want), 1e-300), 0.0)
    return float(np.max(d)) / scale, float(np.max(rel)) if rel.size else 0.0


def assert_bins(got, want, what=""):
    """One window's bins: BINS_TIGHT_RTOL with atol 1e-13, and BINS_NORMWISE."""
    normwise, _ = bins_errors(got, want)
    assert normwise <= BINS_NORMWISE, (what, normwise)
    np.testing.assert_allclose(got, want, rtol=BINS_TIGHT_RTOL, atol=1e-13, err_msg=str(what))


def assert_windows(got, want, what=""):
    """got, want: (bins [n, na, nr], angles [n, 10], mags [n, 10], fft_max [n]).
    Bins at the bins bars per window, vectors exact, fft_max at TIGHT_RTOL."""
    assert got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    for k in range(want[0].shape[0]):
        assert_bins(got[0][k], want[0][k], (what, "window", k))
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what} angles")
    np.testing.assert_array_equal(np.asarray(got[2], np.float32), np.asarray(want[2], np.float32),
                                  err_msg=f"{what} magnitudes")
    np.testing.assert_allclose(got[3], want[3], rtol=TIGHT_RTOL, atol=0, err_msg=f"{what} fft_max")


def assert_vectors_follow_bins(res, what="", kw=BLUR_KW):
    """The vectors of every window are the C oracle's vectorize of its own bins."""
    bins, ang, mag, _ = res
    for k in range(bins.shape[0]):
        a, m = vectorize(bins[k], kw)
        np.testing.assert_array_equal(ang[k], a, err_msg=f"{what} window {k} angles")
        np.testing.assert_array_equal(mag[k], m, err_msg=f"{what} window {k} magnitudes")


# ---- the library ---------------------------------------------------------------------------
def boundaries(boxes):
    from photohive_dsp_amd.core import window_boundaries
    return window_boundaries(boxes)


def host_twin(img, boxes, window, **kw):
    """phd_debug_window_blur_host: (bins, angles, mags, fft_max), or the error text."""
    from photohive_dsp_amd import lib as L
    from photohive_dsp_amd.core import WINDOW_DEFAULTS, make_config
    cfg = make_config(**{**WINDOW_DEFAULTS, **kw})
    img = np.ascontiguousarray(img)
    n, na, nr = len(boxes), cfg.angle_partitions, cfg.radius_partitions
    bins = np.zeros((n, na, nr))
    vec = np.zeros((n, 10, 2), np.int32)
    fmax = np.zeros(n)
    cb = boundaries(boxes)
    rc = L.lib.phd_debug_window_blur_host(img.ctypes.data, img.shape[0], img.shape[1], ctypes.byref(cb), window,
                                          ctypes.byref(cfg), bins.ctypes.data, vec.ctypes.data, fmax.ctypes.data)
    if rc != 0:
        return L.last_error()
    return bins, vec[..., 0].copy(), vec[..., 1].copy().view(np.float32), fmax
