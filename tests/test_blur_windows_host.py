"""Window blur without a device: the symbols and the struct, the free, every
refusal that comes before any HIP call, and the host twin
(phd_debug_window_blur_host: the kernel's own plan, passes and index maps,
blur_window.h) against every fixture of the compiled reference and on the
special patterns."""
import ctypes

import numpy as np
import pytest

from tests import blur_windows_cases as bwc

CASES = bwc.manifest()
ENTRIES = ("phd_blur_windows_device", "phd_free_window_blur", "phd_debug_window_blur_host")


def _lib():
    from photohive_dsp_amd import lib as L
    return L


def test_symbols_types_and_struct_layout():
    L = _lib()
    from photohive_dsp_amd.structures import PhdWindowBlur
    for name in ENTRIES:
        assert getattr(L.lib, name).argtypes is not None, name
    assert L.WINDOW_BLUR_KERNEL == 14
    assert ctypes.sizeof(PhdWindowBlur) == 48
    assert [getattr(PhdWindowBlur, f).offset for f, _ in PhdWindowBlur._fields_] == [0, 4, 8, 12, 16, 24, 32, 40]
    import os
    from tests.conftest import ROOT
    with open(os.path.join(ROOT, "include", "photohive_dsp.h")) as f:
        h = f.read()
    for s in ("typedef struct phd_window_blur {", "14 window_blur", "PHD_WINDOW_BLUR_BUDGET") + \
            tuple(e + "(" for e in ENTRIES):
        assert s in h, s
    import photohive_dsp_amd as phd
    assert callable(phd.blur_windows_device) and callable(phd.blur_map_device) and callable(phd.window_grid)


def test_all_fixture_cases_are_present():
    assert [c["name"] for c in CASES] == [c[0] for c in bwc.CASES]
    got = {(c["window"], c["radius_partitions"], c["angle_partitions"]) for c in CASES}
    assert {(128, 16, 36), (128, 8, 18), (128, 40, 72), (64, 16, 36), (64, 8, 18)} <= got
    total = moving = 0
    for c in CASES:
        fx = bwc.fixture(c["name"])
        assert sorted(fx) == ["angle_bin_size", "angles", "bins", "fft_max", "mags", "radius_bin_size", "windows"]
        total += len(fx["windows"])
        moving += int(np.count_nonzero(fx["mags"].max(axis=1) > 0))
    assert 3 * moving >= total, (moving, total)


def _stage(L, imgs, hs, ws, boxes, window, cfg, out, n=None):
    from photohive_dsp_amd.structures import Crop_Boundaries
    n = len(imgs) if n is None else n
    cbs = (ctypes.POINTER(Crop_Boundaries) * len(imgs))(*[ctypes.pointer(b) if b is not None else None for b in boxes])
    return L.lib.phd_blur_windows_device((ctypes.c_void_p * len(imgs))(*imgs), (ctypes.c_int * len(imgs))(*hs),
                                         (ctypes.c_int * len(imgs))(*ws), n, cbs, window,
                                         ctypes.byref(cfg) if cfg is not None else None, out, None)


def test_stage_rejects_bad_arguments_before_touching_hip():
    """With or without a device: the image pointers below are never dereferenced."""
    L = _lib()
    from photohive_dsp_amd.core import make_config
    from photohive_dsp_amd.structures import PhdWindowBlur
    good = bwc.boundaries([(0, 64, 0, 64), (36, 100, 136, 200)])
    junk = (ctypes.c_double * 2)()

    def call(imgs=(4096, 8192), hs=(100, 100), ws=(200, 200), boxes=(good, good), window=64, nr=16, na=36, cfg=True):
        out = (PhdWindowBlur * 2)()
        for o in out:
            o.n_windows = 7
            o.bins = ctypes.cast(junk, type(o.bins))
            o.fft_max = ctypes.cast(junk, type(o.fft_max))
        c = make_config(radius_partitions=nr, angle_partitions=na) if cfg else None
        rc = _stage(L, list(imgs), hs, ws, list(boxes), window, c, out)
        assert rc == -1
        assert all(o.n_windows == 0 and not o.bins and not o.vectors and not o.fft_max and o.num_angle_bins == 0
                   for o in out), "out is left zeroed"
        return L.last_error()

    assert "phd_blur_windows_device: image 1: NULL image" in call(imgs=(4096, None))
    assert "image 1: 63 x 200 is smaller than the window 64" in call(hs=(100, 63))
    assert "image 0: 100 x 10 is smaller than the window 64" in call(ws=(10, 200))
    for w in (0, 32, 65, 96, 256, -64):
        assert "window must be 64 or 128" in call(window=w), w
    # sides that are not T: a 128 box in a 64 call, a 64 x 65 box, an inverted box
    for box, k in (((0, 128, 0, 128), 0), ((0, 64, 0, 65), 0), ((64, 0, 0, 64), 0)):
        msg = call(boxes=(good, bwc.boundaries([box])))
        assert "image 1: window 0 " in msg and "is not 64 x 64" in msg, msg
    msg = call(boxes=(bwc.boundaries([(0, 64, 0, 64), (0, 64, 0, 63)]), good))
    assert "image 0: window 1 " in msg and "is not 64 x 64" in msg, msg
    # boxes that leave the image
    for box in ((37, 101, 0, 64), (0, 64, 137, 201), (-1, 63, 0, 64), (0, 64, -3, 61)):
        msg = call(boxes=(good, bwc.boundaries([(1, 65, 1, 65), box])))
        assert "image 1: window 1 " in msg and "leaves the 100 x 200 image" in msg, msg
    assert "exceeds 2880 bins" in call(nr=41, na=72)
    assert "exceeds 2880 bins" in call(window=128, nr=40, na=73,
                                       boxes=(bwc.boundaries([(0, 100, 0, 100)]),) * 2)
    # the two grids build_blur_table refuses, with its own messages
    assert "radius bin size 0" in call(window=64, nr=46, na=36)
    assert "outside the polar bin table" in call(window=64, nr=40, na=72)
    big = bwc.boundaries([(0, 128, 0, 128)])
    assert "outside the polar bin table" in call(window=128, nr=35, na=36, hs=(128, 128), ws=(128, 128),
                                                 boxes=(big, big))
    # (128 at 46 x 72 has such elements too; its 3312 bins are refused first)
    assert "exceeds 2880 bins" in call(window=128, nr=46, na=72, hs=(128, 128), ws=(128, 128), boxes=(big, big))
    assert "NULL argument" in call(cfg=False)
    out = (PhdWindowBlur * 2)()
    cfg = make_config(radius_partitions=16, angle_partitions=36)
    assert L.lib.phd_blur_windows_device(None, None, None, 2, None, 64, ctypes.byref(cfg), out, None) == -1
    assert "phd_blur_windows_device: NULL argument" in L.last_error()
    assert _stage(L, [4096, 8192], (100, 100), (200, 200), [good, good], 64, cfg, out, n=0) == -1
    assert "n_images" in L.last_error()
    bad = make_config(radius_partitions=0, angle_partitions=36)
    assert _stage(L, [4096, 8192], (100, 100), (200, 200), [good, good], 64, bad, out) == -1
    assert "radius/angle_partitions must be positive" in L.last_error()


def test_images_without_windows_need_no_device():
    L = _lib()
    from photohive_dsp_amd.core import make_config
    from photohive_dsp_amd.structures import PhdWindowBlur
    none = bwc.boundaries([])
    out = (PhdWindowBlur * 2)()
    out[0].n_windows = 5
    cfg = make_config(radius_partitions=16, angle_partitions=36)
    assert _stage(L, [4096, 8192], (150, 128), (200, 128), [None, none], 128, cfg, out) == 0, L.last_error()
    for o in out:
        assert (o.n_windows, bool(o.bins), bool(o.vectors), bool(o.fft_max)) == (0, False, False, False)
        assert (o.num_angle_bins, o.num_radius_bins) == (36, 16)
        # calculate_blur_profile's integers for a 128 x 65 spectrum (src/blur_profile.c:56-61)
        assert (o.angle_bin_size, o.radius_bin_size) == (180 // 36, int(np.sqrt(65 * 65 + 128 * 128 // 4) / 16))
    L.lib.phd_free_window_blur(out, 2)
    assert all(o.num_angle_bins == 0 for o in out)


def test_free_on_zeroed_and_null_input():
    L = _lib()
    from photohive_dsp_amd.structures import PhdWindowBlur
    out = (PhdWindowBlur * 3)()
    L.lib.phd_free_window_blur(out, 3)
    L.lib.phd_free_window_blur(out, 3)
    L.lib.phd_free_window_blur(None, 3)
    L.lib.phd_free_window_blur(out, 0)
    assert all(o.n_windows == 0 and not o.bins and not o.vectors and not o.fft_max for o in out)


def test_twin_rejects_bad_arguments():
    img = np.zeros((100, 200, 3), np.uint8)
    for boxes, window, kw, what in (([(0, 64, 0, 65)], 64, {}, "window 0 "), ([(0, 64, 0, 64), (37, 101, 0, 64)], 64, {}, "window 1 "),
                                    ([(0, 64, 0, 64)], 32, {}, "64 or 128"), ([(0, 128, 0, 128)], 128, {}, "smaller than"),
                                    ([(0, 64, 0, 64)], 64, dict(radius_partitions=46), "radius bin size 0"),
                                    ([(0, 64, 0, 64)], 64, dict(radius_partitions=40, angle_partitions=72), "outside"),
                                    ([(0, 64, 0, 64)], 64, dict(radius_partitions=41, angle_partitions=72), "2880")):
        msg = bwc.host_twin(img, boxes, window, **kw)
        assert isinstance(msg, str) and "phd_debug_window_blur_host" in msg and what in msg, (what, msg)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_on_reference_fixtures(case):
    fx = bwc.fixture(case["name"])
    boxes = [tuple(int(v) for v in b) for b in fx["windows"]]
    assert len(boxes) == case["windows"]
    got = bwc.host_twin(bwc.case_image(case), boxes, case["window"], **bwc.case_kw(case))
    assert not isinstance(got, str), got
    want = (fx["bins"], fx["angles"], fx["mags"], fx["fft_max"])
    worst = max(bwc.bins_errors(got[0][k], want[0][k])[0] for k in range(len(boxes)))
    print(f"{case['name']}: twin against the reference, bins normwise at worst {worst:.3e}")
    bwc.assert_windows(got, want, case["name"])
    bwc.assert_vectors_follow_bins(got, case["name"])
    # the bin sizes of the struct are the table's: checked where the struct is filled (no device needed)
    L = _lib()
    from photohive_dsp_amd.core import make_config
    from photohive_dsp_amd.structures import PhdWindowBlur
    out = (PhdWindowBlur * 1)()
    assert _stage(L, [4096], (case["height"],), (case["width"],), [None], case["window"],
                  make_config(**bwc.case_kw(case)), out) == 0, L.last_error()
    assert (out[0].angle_bin_size, out[0].radius_bin_size) == (int(fx["angle_bin_size"]), int(fx["radius_bin_size"]))


@pytest.mark.parametrize("window", [64, 128])
def test_twin_on_special_patterns(window):
    """Constant grey, black and white windows: all-zero bins and vectors.  One
    bright pixel, 1-px stripes and a checkerboard against the C oracle, at a
    base that is not 4-byte aligned and at odd window positions."""
    T = window
    for name in ("grey", "black", "white"):
        got = bwc.host_twin(bwc.special_tile(name), [(0, T, 0, T), (128 - T, 128, 128 - T, 128)], T)
        assert not isinstance(got, str), got
        assert not got[0].any() and not got[1].any() and not got[2].any(), name
        assert (got[3] < 1).all(), (name, got[3])
    rows = []
    for name in ("one_pixel", "h_stripes", "v_stripes", "checkerboard"):
        rows.append(np.concatenate([bwc.special_tile("noise"), bwc.special_tile(name), bwc.special_tile("black")], axis=1))
    img = np.concatenate(rows, axis=0)                      # 512 x 384
    boxes = [(128 * r + dy, 128 * r + dy + T, 128 + dx, 128 + dx + T) for r in range(4) for dy, dx in ((0, 0), (1, 1))
             if 128 + dx + T <= 256 or T == 64]
    dy = 3 if T == 64 else 0
    boxes += [(128 * r + dy, 128 * r + dy + T, 128 - 5, 128 - 5 + T) for r in range(4)]   # straddling two tiles
    raw = np.zeros(img.size + 1, np.uint8)
    raw[1:] = img.ravel()
    odd = raw[1:].reshape(img.shape)                        # base + 1
    assert odd.ctypes.data % 4 != img.ctypes.data % 4
    want = bwc.oracle_windows(img, boxes, 16, 36)
    for im in (img, odd):
        got = bwc.host_twin(im, boxes, T)
        assert not isinstance(got, str), got
        bwc.assert_windows(got, want, f"special {T}")
        bwc.assert_vectors_follow_bins(got, f"special {T}")
    # the stripes and the checkerboard put their energy where the packed column and the Nyquist row are
    assert want[3][2:len(boxes) - 4].min() > 1.0 and want[0][2:len(boxes) - 4].max() > 0.0
    # one pixel of luma 1: every p but DC's is 1 up to rounding, so every log is rounding noise
    got = bwc.host_twin(bwc.special_tile("one_pixel_255"), [(0, T, 0, T)], T)
    assert got[0].max() <= 1e-13 and got[0].min() >= 0.0
    np.testing.assert_allclose(got[3], 1.0, rtol=bwc.TIGHT_RTOL)
    bwc.assert_vectors_follow_bins(got, "one pixel on the threshold")
