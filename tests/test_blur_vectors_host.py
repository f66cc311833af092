"""Blur vectors without a device: the symbols and documents, every refusal of the
two device entries that comes before any HIP call, the shared finish
(blur_window.h through phd_debug_window_finish_host) against the C oracle's
vectorize on bin sums made in numpy, and the kernel's twin
(phd_debug_window_vectors_host) on every fixture window of the compiled reference.

Bars: vectors exact everywhere.  The finish's bins against the formula
flat[b] = sums[b] == 0 ? 0 : (double)sums[b] / scale * gs / counts[b], evaluated with
math.sqrt, math.log and numpy float64 division, at rtol 4 * 2^-53: one last place
for a log that may not be the same binary's, through one reciprocal and one
product.  The counts are the C oracle's (the reference's own counting over a
T x (T/2+1) spectrum), because phd_blur_counts needs a device;
tests/test_gpu_blur_vectors.py checks on the device that phd_blur_counts(T, T, nr,
na) gives the same numbers.  The twin's fft_max is bit-identical to
phd_debug_window_blur_host's."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest

from tests import blur_windows_cases as bwc

CASES = bwc.manifest()
ENTRIES = ("phd_blur_vectors_device", "phd_blur_vector_maps_device", "phd_debug_window_vectors_host",
           "phd_debug_window_finish_host")
GRIDS = [(64, 8, 18), (64, 16, 36), (128, 8, 18), (128, 16, 36)]          # (window, nr, na)
BINS_RTOL = 4 * 2.0 ** -53


def _lib():
    from photohive_dsp_amd import lib as L
    return L


def _cfg(**kw):
    from photohive_dsp_amd.core import WINDOW_DEFAULTS, make_config
    return make_config(**{**WINDOW_DEFAULTS, **bwc.BLUR_KW, **kw})


def test_symbols_documents_and_python_names():
    L = _lib()
    for name in ENTRIES:
        assert getattr(L.lib, name).argtypes is not None, name
    assert L.WINDOW_VECTORS_KERNEL == 15 and L.WINDOW_BLUR_KERNEL == 14
    from tests.conftest import ROOT
    with open(os.path.join(ROOT, "include", "photohive_dsp.h")) as f:
        h = f.read()
    for s in ("15 window_vectors", "14 window_blur") + tuple(e + "(" for e in ENTRIES):
        assert s in h, s
    import photohive_dsp_amd as phd
    assert callable(phd.blur_vectors_device) and callable(phd.blur_vector_maps_device)
    assert callable(phd.blur_windows_device) and callable(phd.blur_map_device)


# ---- refusals ----------------------------------------------------------------------------
def _lists(L, imgs, hs, ws, boxes, window, cfg, vec, fmax, n=None):
    from photohive_dsp_amd.structures import Crop_Boundaries
    k = len(imgs)
    cbs = None if boxes is None else \
        (ctypes.POINTER(Crop_Boundaries) * k)(*[ctypes.pointer(b) if b is not None else None for b in boxes])
    return L.lib.phd_blur_vectors_device((ctypes.c_void_p * k)(*imgs), (ctypes.c_int * k)(*hs), (ctypes.c_int * k)(*ws),
                                         k if n is None else n, cbs, window,
                                         ctypes.byref(cfg) if cfg is not None else None,
                                         (ctypes.c_void_p * k)(*vec) if vec is not None else None,
                                         (ctypes.c_void_p * k)(*fmax) if fmax is not None else None, None)


def _maps(L, imgs, hs, ws, window, stride, cfg, vec, fmax, n=None):
    k = len(imgs)
    return L.lib.phd_blur_vector_maps_device((ctypes.c_void_p * k)(*imgs), (ctypes.c_int * k)(*hs),
                                             (ctypes.c_int * k)(*ws), k if n is None else n, window, stride,
                                             ctypes.byref(cfg) if cfg is not None else None,
                                             (ctypes.c_void_p * k)(*vec) if vec is not None else None,
                                             (ctypes.c_void_p * k)(*fmax) if fmax is not None else None, None)


def test_list_entry_rejects_bad_arguments_before_touching_hip():
    """With or without a device: the pointers below are never dereferenced."""
    L = _lib()
    good = bwc.boundaries([(0, 64, 0, 64), (36, 100, 136, 200)])

    def call(imgs=(4096, 8192), hs=(100, 100), ws=(200, 200), boxes=(good, good), window=64, nr=16, na=36, cfg=True,
             vec=(1 << 20, 2 << 20), fmax=(3 << 20, None), n=None):
        c = _cfg(radius_partitions=nr, angle_partitions=na) if cfg else None
        rc = _lists(L, list(imgs), hs, ws, None if boxes is None else list(boxes), window, c,
                    None if vec is None else list(vec), None if fmax is None else list(fmax), n)
        assert rc == -1
        msg = L.last_error()
        assert msg.startswith("phd_blur_vectors_device: "), msg
        return msg

    assert "NULL argument" in call(cfg=False)
    assert "NULL argument" in call(boxes=None)
    assert "NULL argument" in call(vec=None)
    assert "n_images" in call(n=0) and "n_images" in call(n=-3)
    assert "image 1: NULL image" in call(imgs=(4096, None))
    for w in (0, 32, 96, 256):
        assert "window must be 64 or 128" in call(window=w), w
    assert "outside the polar bin table" in call(window=64, nr=40, na=72)
    assert "radius bin size 0" in call(window=64, nr=46, na=36)
    assert "exceeds 2880 bins" in call(nr=41, na=72)
    msg = call(na=1)
    assert "angle_partitions must be at least 2" in msg and "not 1" in msg, msg
    msg = call(boxes=(good, bwc.boundaries([(0, 64, 0, 65)])))
    assert "image 1: window 0 " in msg and "is not 64 x 64" in msg, msg
    msg = call(boxes=(bwc.boundaries([(1, 65, 1, 65), (37, 101, 0, 64)]), good))
    assert "image 0: window 1 " in msg and "leaves the 100 x 200 image" in msg, msg
    assert "image 1: 63 x 200 is smaller than the window 64" in call(hs=(100, 63))
    msg = call(vec=(1 << 20, None))
    assert "image 1: NULL d_vectors for 2 windows" in msg, msg
    # an image without windows needs no d_vectors; its neighbour's refusal still comes
    msg = call(boxes=(None, bwc.boundaries([(0, 64, 0, 63)])), vec=(None, 1 << 20))
    assert "image 1: window 0 " in msg, msg


def test_grid_entry_rejects_bad_arguments_before_touching_hip():
    L = _lib()

    def call(imgs=(4096, 8192), hs=(100, 100), ws=(200, 200), window=64, stride=64, nr=16, na=36, cfg=True,
             vec=(1 << 20, 2 << 20), fmax=None, n=None):
        c = _cfg(radius_partitions=nr, angle_partitions=na) if cfg else None
        rc = _maps(L, list(imgs), hs, ws, window, stride, c, None if vec is None else list(vec),
                   None if fmax is None else list(fmax), n)
        assert rc == -1
        msg = L.last_error()
        assert msg.startswith("phd_blur_vector_maps_device: "), msg
        return msg

    assert "NULL argument" in call(cfg=False)
    assert "NULL argument" in call(vec=None)
    assert "n_images" in call(n=0)
    assert "image 0: NULL image" in call(imgs=(None, 8192))
    assert "window must be 64 or 128" in call(window=32)
    assert "outside the polar bin table" in call(window=64, nr=40, na=72)
    assert "radius bin size 0" in call(window=64, nr=46, na=36)
    assert "exceeds 2880 bins" in call(nr=41, na=72)
    assert "angle_partitions must be at least 2" in call(na=1)
    for s in (0, -1):
        msg = call(stride=s)
        assert "stride must be positive" in msg and f"not {s}" in msg, msg
    assert "image 1: 100 x 50 is smaller than the window 64" in call(ws=(200, 50))
    assert "image 0: 100 x 200 is smaller than the window 128" in call(window=128)
    msg = call(vec=(None, 2 << 20))
    assert "image 0: NULL d_vectors for 3 windows" in msg, msg          # 100 x 200 at 64 / 64: 1 x 3
    # more than 2^31 - 1 windows: 46341^2 windows of 64 x 64 at stride 1
    big = 46340 + 64
    msg = call(imgs=(4096,), hs=(big,), ws=(big,), stride=1, vec=(1 << 20,))
    assert "too many windows" in msg, msg
    # three grids of (2^31 - 64)^2 windows: their sum does not fit a long long; refused at the first
    top = 2147483647
    msg = call(imgs=(4096, 8192, 12288), hs=(top,) * 3, ws=(top,) * 3, stride=1, vec=(1 << 20, 2 << 20, 3 << 20))
    assert "too many windows" in msg, msg
    # the running count is checked image by image: image 1's own defect is never reached
    msg = call(imgs=(4096, None), hs=(big, 100), ws=(big, 200), stride=1)
    assert "too many windows" in msg and "image 1" not in msg, msg


def test_python_wrappers_without_images_return_nothing():
    """No image: [] before any tensor or device is touched."""
    import photohive_dsp_amd as phd
    assert phd.blur_vectors_device([], []) == [] and phd.blur_vectors_device([], None) == []
    assert phd.blur_vector_maps_device([]) == [] and phd.blur_vector_maps_device([], stride=0) == []
    with pytest.raises(ValueError, match="windows has 1 entries for 0 images"):
        phd.blur_vectors_device([], [None])


def test_twin_and_finish_reject_bad_arguments():
    L = _lib()
    img = np.zeros((100, 200, 3), np.uint8)
    for boxes, window, kw, what in (([(0, 64, 0, 65)], 64, {}, "window 0 "), ([(0, 64, 0, 64)], 32, {}, "64 or 128"),
                                    ([(0, 128, 0, 128)], 128, {}, "smaller than"),
                                    ([(0, 64, 0, 64)], 64, dict(angle_partitions=1), "at least 2"),
                                    ([(0, 64, 0, 64)], 64, dict(radius_partitions=46), "radius bin size 0")):
        msg = _twin(img, boxes, window, **kw)
        assert isinstance(msg, str) and "phd_debug_window_vectors_host" in msg and what in msg, (what, msg)
    sums = np.zeros(16 * 36, np.uint64)
    vec = np.zeros((10, 2), np.int32)
    for window, kw, what in ((32, {}, "64 or 128"), (64, dict(angle_partitions=1), "at least 2"),
                             (64, dict(radius_partitions=41, angle_partitions=72), "2880")):
        assert L.lib.phd_debug_window_finish_host(sums.ctypes.data, 2.0, window, ctypes.byref(_cfg(**kw)), None,
                                                  vec.ctypes.data) == -1
        assert "phd_debug_window_finish_host" in L.last_error() and what in L.last_error()
    assert L.lib.phd_debug_window_finish_host(None, 2.0, 64, ctypes.byref(_cfg()), None, vec.ctypes.data) == -1


# ---- the finish against the oracle ----------------------------------------------------------
def _scale(T):
    """bin_scale(T, T/2+1) (phd_internal.h)."""
    wf = T // 2 + 1
    n = T * 2.0 * wf
    return 2.0 ** (62 - math.ceil(math.log2(T * wf * 2.0 * math.log(n) + 1.0)))


@functools.lru_cache(maxsize=None)
def _counts(T, nr, na):
    from oracle import oracle as orc
    _bins, counts, _fmax, _a, _r = orc.blur_profile(np.zeros((T, T // 2 + 1)), nr, na)
    counts = np.asarray(counts, np.int64).reshape(na, nr).copy()
    assert counts.sum() == T * (T // 2 + 1) and counts.max() <= 65535
    counts.setflags(write=False)
    return counts


def _gs(fmax):
    return 1 / (2 * math.log(math.sqrt(fmax) + 1))


def _finish(sums, fmax, T, nr, na, want_bins=True, **kw):
    """phd_debug_window_finish_host: (bins [na, nr] or None, angles, mags)."""
    L = _lib()
    sums = np.ascontiguousarray(sums, np.uint64).reshape(-1)
    assert sums.size == na * nr
    bins = np.full((na, nr), np.nan) if want_bins else None
    vec = np.full((10, 2), -1, np.int32)
    rc = L.lib.phd_debug_window_finish_host(sums.ctypes.data, float(fmax), T,
                                            ctypes.byref(_cfg(radius_partitions=nr, angle_partitions=na, **kw)),
                                            bins.ctypes.data if want_bins else None, vec.ctypes.data)
    assert rc == 0, L.last_error()
    return bins, vec[:, 0].copy(), vec[:, 1].copy().view(np.float32)


def _sums_for(target, T, nr, na, fmax):
    """Bin sums whose flat bins come out near `target` [na, nr] (0 stays exactly 0)."""
    c = _counts(T, nr, na).astype(np.float64)
    return np.rint(np.asarray(target, np.float64) * c * _scale(T) / _gs(fmax)).astype(np.uint64)


def _smoothed(bins, denom=2):
    """tot, avg and the smoothed totals in the reference's order (numpy float64 scalars are IEEE)."""
    na, nr = bins.shape
    rc = nr // denom
    tot = []
    for i in range(na):
        t = np.float64(0.0)
        for j in range(rc):
            t = t + bins[i, j]
        tot.append(t)
    avg = np.float64(0.0)
    for t in tot:
        avg = avg + t
    avg = avg / na
    sm = []
    for i in range(na):
        s = np.float64(0.0)
        for j in range(5):
            s = s + tot[(i - j) % na]
        sm.append(s / 5)
    return tot, avg, sm


def _maxima(bins, streak=1.20, denom=2):
    """Every strict local maximum above the threshold (not cut at ten)."""
    _tot, avg, sm = _smoothed(bins, denom)
    na = len(sm)
    return [i for i in range(na) if sm[i] > sm[i - 1] and sm[i] > sm[(i + 1) % na] and sm[i] > avg * streak]


def _check(sums, fmax, T, nr, na, what, **kw):
    """The finish of these sums: bins at the formula, vectors the oracle's of those bins; returns them."""
    bins, ang, mag = _finish(sums, fmax, T, nr, na, **kw)
    c = _counts(T, nr, na)
    s = np.asarray(sums, np.uint64).reshape(na, nr)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(s == 0, 0.0, s.astype(np.float64) / _scale(T) * (_gs(fmax) if fmax > 0 else np.inf))
        want = np.where(c != 0, want / c, 0.0)
    np.testing.assert_allclose(bins, want, rtol=BINS_RTOL, atol=0, err_msg=f"{what}: bins")
    assert ((s == 0) <= (bins == 0)).all(), f"{what}: a zero sum is a zero bin"
    a, m = bwc.vectorize(bins, {**bwc.BLUR_KW, **kw})
    np.testing.assert_array_equal(ang, a, err_msg=f"{what}: angles")
    np.testing.assert_array_equal(mag, m, err_msg=f"{what}: magnitudes")
    # without the bins: the same vectors
    _none, ang2, mag2 = _finish(sums, fmax, T, nr, na, want_bins=False, **kw)
    np.testing.assert_array_equal(ang2, ang)
    np.testing.assert_array_equal(mag2, mag)
    return bins, ang, mag


def _bump(na, nr, at, base=0.05, top=3.0):
    """A triangular bump of five angle rows whose smoothed totals have their one maximum at `at`;
    the perpendicular row stays above magnitude_thresh for three radii."""
    t = np.full((na, nr), base)
    for d, v in zip(range(-2, 3), (0.3, 0.6, 1.0, 0.6, 0.3)):
        t[(at - 2 + d) % na, :] = base + (top - base) * v
    perp = (at + na // 2) % na
    t[perp, :3] = 0.31
    return t


@pytest.mark.parametrize("T,nr,na", GRIDS, ids=[f"{g[0]}_{g[1]}x{g[2]}" for g in GRIDS])
def test_finish_against_the_oracle(T, nr, na):
    rng = np.random.default_rng(1000 + T + na)
    fmax = 2672.0508363325334 if T == 64 else 43649.3071442577
    full = _counts(T, nr, na) > 0
    some = 0
    for rep in range(12):                                     # random sums: flat bins over [0, 1.2)
        _b, _a, m = _check(_sums_for(rng.random((na, nr)) * (0.2 + rng.random((na, 1))), T, nr, na, fmax), fmax, T, nr,
                           na, f"random {rep}", fft_streak_thresh=1.0 + 0.02 * rep)
        some += int(np.count_nonzero(m))
    assert some > 0, "the random sums give vectors"
    for f in (0.0, 0.25, fmax):                               # all zero (fft_max < 1: gs is never used)
        bins, ang, mag = _check(np.zeros(na * nr, np.uint64), f, T, nr, na, f"zero sums, fft_max {f}")
        assert not bins.any() and not ang.any() and not mag.any()
    bins, ang, mag = _check(np.full(na * nr, 1 << 40, np.uint64), fmax, T, nr, na, "equal sums")
    bins, ang, mag = _check(_sums_for(np.full((na, nr), 0.5), T, nr, na, fmax), fmax, T, nr, na, "equal bins")
    for at in (0, na - 1, na // 3):                           # one raised angle: a maximum first, last, inside
        bins, ang, mag = _check(_sums_for(_bump(na, nr, at), T, nr, na, fmax), fmax, T, nr, na, f"bump at {at}")
        if full.all():
            assert _maxima(bins) == [at], (at, _maxima(bins))
            perp = (at + na // 2) % na
            assert mag[0] == np.float32(3) / np.float32(nr) and not mag[1:].any()
            assert ang[0] == int(np.float32(180) * (np.float32(perp) / np.float32(na)) - np.float32(90))
    # more maxima than ten: every third angle at 36 (twelve), every second at 18 (nine: all that fit)
    period = 3 if na == 36 else 2
    t = np.empty((na, nr))
    for i in range(na):
        t[i, :] = (0.9, 0.2, 0.02)[i % period] if period == 3 else (0.9, 0.02)[i % 2]
    for a in range(na):                                       # perpendicular rows that are not rejected differ
        t[a, :1 + a % 5] = np.maximum(t[a, :1 + a % 5], 0.31)
    bins, ang, mag = _check(_sums_for(t, T, nr, na, fmax), fmax, T, nr, na, "many maxima", fft_streak_thresh=0.5)
    if full.all():
        assert len(_maxima(bins, streak=0.5)) == (12 if na == 36 else 9)
    # a plateau of two equal neighbours: four raised angles, every other sum zero
    p = na // 2
    t = np.zeros((na, nr))
    for k, v in zip(range(p - 3, p + 1), (0.4, 0.7, 0.9, 0.6)):
        t[k, :] = v
    bins, ang, mag = _check(_sums_for(t, T, nr, na, fmax), fmax, T, nr, na, "plateau")
    _tot, avg, sm = _smoothed(bins)
    assert sm[p] == sm[p + 1] and sm[p] > sm[p - 1] and sm[p + 1] > sm[p + 2] and sm[p] > avg * 1.2
    assert _maxima(bins) == [] and not ang.any() and not mag.any()
    # denom larger than nr: no radius is summed, nothing is a maximum
    bins, ang, mag = _check(_sums_for(_bump(na, nr, 5), T, nr, na, fmax), fmax, T, nr, na, "denom > nr",
                            blur_cutoff_ratio_denom=nr + 1)
    assert bins.any() and not ang.any() and not mag.any()
    bins, ang, mag = _check(_sums_for(_bump(na, nr, 5), T, nr, na, fmax), fmax, T, nr, na, "denom = nr",
                            blur_cutoff_ratio_denom=nr)


@pytest.mark.parametrize("T,nr", [(64, 8), (64, 16), (128, 8), (128, 16)])
def test_finish_at_two_angle_partitions(T, nr):
    rng = np.random.default_rng(2000 + T + nr)
    fmax = 1234.5
    for rep in range(8):
        t = rng.random((2, nr)) * np.array([[1.0], [0.2 + 0.2 * rep]])
        _check(_sums_for(t, T, nr, 2, fmax), fmax, T, nr, 2, f"two angles {rep}", fft_streak_thresh=1.0 + 0.05 * rep)
    bins, ang, mag = _check(np.zeros(2 * nr, np.uint64), fmax, T, nr, 2, "two angles, zero sums")
    assert not ang.any() and not mag.any()


# ---- the twin on every fixture window ---------------------------------------------------------
def _twin(img, boxes, window, **kw):
    """phd_debug_window_vectors_host: (angles, mags, fft_max), or the error text."""
    L = _lib()
    cfg = _cfg(**kw)
    img = np.ascontiguousarray(img)
    n = len(boxes)
    vec = np.full((n, 10, 2), -1, np.int32)
    fmax = np.full(n, np.nan)
    cb = bwc.boundaries(boxes)
    rc = L.lib.phd_debug_window_vectors_host(img.ctypes.data, img.shape[0], img.shape[1], ctypes.byref(cb), window,
                                             ctypes.byref(cfg), vec.ctypes.data, fmax.ctypes.data)
    if rc != 0:
        return L.last_error()
    return vec[..., 0].copy(), vec[..., 1].copy().view(np.float32), fmax


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_on_reference_fixtures(case):
    fx = bwc.fixture(case["name"])
    boxes = [tuple(int(v) for v in b) for b in fx["windows"]]
    img = bwc.case_image(case)
    got = _twin(img, boxes, case["window"], **bwc.case_kw(case))
    assert not isinstance(got, str), got
    np.testing.assert_array_equal(got[0], fx["angles"], err_msg="angles")
    np.testing.assert_array_equal(got[1], np.asarray(fx["mags"], np.float32), err_msg="magnitudes")
    old = bwc.host_twin(img, boxes, case["window"], **bwc.case_kw(case))
    assert not isinstance(old, str), old
    np.testing.assert_array_equal(got[2].view(np.uint64), old[3].view(np.uint64), err_msg="fft_max bits")
    np.testing.assert_array_equal(got[0], old[1])
    np.testing.assert_array_equal(got[1], old[2])


def test_twin_without_windows_and_on_constant_windows():
    img = np.zeros((100, 200, 3), np.uint8)
    assert _twin(img, [], 64)[0].shape == (0, 10)
    for name in ("grey", "black", "white", "colour"):
        got = _twin(bwc.special_tile(name), [(0, 64, 0, 64), (64, 128, 64, 128)], 64)
        assert not isinstance(got, str), got
        assert not got[0].any() and not got[1].any(), name
