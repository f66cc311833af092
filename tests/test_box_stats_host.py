"""Box statistics without a device: the symbols and the struct, the free, the
argument checks that come before any HIP call, and the host twin
(phd_debug_box_stats_host: the kernel's own item plan and row walk,
box_stat_tiles.h) against Python integers on synthetic images at every base
phase and against every fixture of the compiled reference."""
import ctypes

import numpy as np
import pytest

from tests import box_stats_cases as bsc

CASES = bsc.manifest()


def _lib():
    from photohive_dsp_amd import lib as L
    return L


ENTRIES = ("phd_box_stats_device", "phd_free_box_stats", "phd_debug_box_stats_host",
           "phd_report_batch_device_mixed_box_stats", "phd_report_batch_device_views_box_stats",
           "phd_report_batch_device_typed_views_box_stats", "phd_report_batch_device_yuv_box_stats")


def test_symbols_types_and_struct_layout():
    L = _lib()
    from photohive_dsp_amd.structures import PhdBoxStats
    for name in ENTRIES:
        assert getattr(L.lib, name).argtypes is not None, name
    assert (L.BOX_STATS_KERNEL, L.PLANAR_BOX_STATS_KERNEL) == (12, 13)
    assert ctypes.sizeof(PhdBoxStats) == 24
    assert (PhdBoxStats.n_boxes.offset, PhdBoxStats.stats.offset, PhdBoxStats.average_saturation.offset) == (0, 8, 16)
    import os
    from tests.conftest import ROOT
    with open(os.path.join(ROOT, "include", "photohive_dsp.h")) as f:
        h = f.read()
    for s in ("typedef struct phd_box_stats {", "12 box_stats") + tuple(e + "(" for e in ENTRIES):
        assert s in h, s
    import photohive_dsp_amd as phd
    assert callable(phd.box_stats_device)


def _stage(L, imgs, hs, ws, boxes, out, n=None):
    n = len(imgs) if n is None else n
    from photohive_dsp_amd.structures import Crop_Boundaries
    cbs = (ctypes.POINTER(Crop_Boundaries) * len(imgs))(*[ctypes.pointer(b) if b is not None else None for b in boxes])
    return L.lib.phd_box_stats_device((ctypes.c_void_p * len(imgs))(*imgs), (ctypes.c_int * len(imgs))(*hs),
                                      (ctypes.c_int * len(imgs))(*ws), n, cbs, out, None)


def test_stage_rejects_bad_arguments_before_touching_hip():
    """With or without a device: the image pointers below are never dereferenced."""
    L = _lib()
    from photohive_dsp_amd.structures import PhdBoxStats
    good, keep0 = bsc.crop_boundaries([(0, 4, 0, 5)])
    inverted, keep1 = bsc.crop_boundaries([(0, 4, 0, 5), (3, 2, 0, 5)])
    past, keep2 = bsc.crop_boundaries([(0, 4, 0, 5), (0, 4, 0, 5), (0, 4, 1, 8)])
    negative, keep3 = bsc.crop_boundaries([(-1, 4, 0, 5)])
    empty, keep4 = bsc.crop_boundaries([(2, 2, 0, 5)])
    junk = (ctypes.c_double * 2)()

    def call(imgs=(4096, 8192), hs=(4, 4), ws=(5, 7), boxes=(good, good)):
        out = (PhdBoxStats * 2)()
        for o in out:
            o.n_boxes = 7
            o.stats = ctypes.cast(junk, type(o.stats))
            o.average_saturation = ctypes.cast(junk, type(o.average_saturation))
        rc = _stage(L, list(imgs), hs, ws, list(boxes), out)
        assert rc == -1
        assert all(o.n_boxes == 0 and not o.stats and not o.average_saturation for o in out), "out is left zeroed"
        return L.last_error()

    assert "phd_box_stats_device: image 1: NULL image" in call(imgs=(4096, None))
    assert "image 1: height and width must be positive" in call(hs=(4, 0))
    assert "image 0: height and width must be positive" in call(ws=(-5, 7))
    for boxes, img, crop in (((good, inverted), 1, 1), ((good, past), 1, 2), ((negative, good), 0, 0),
                             ((empty, good), 0, 0)):
        msg = call(boxes=boxes)
        assert f"image {img}: " in msg and f"(crop {crop})" in msg, msg
    out = (PhdBoxStats * 2)()
    assert L.lib.phd_box_stats_device(None, None, None, 2, None, out, None) == -1
    assert "phd_box_stats_device: NULL argument" in L.last_error()
    assert _stage(L, [4096, 8192], (4, 4), (5, 7), [good, good], out, n=0) == -1
    assert "n_images" in L.last_error()
    del keep0, keep1, keep2, keep3, keep4


def test_images_without_boxes_need_no_device():
    L = _lib()
    from photohive_dsp_amd.structures import PhdBoxStats
    none, keep = bsc.crop_boundaries([])
    out = (PhdBoxStats * 2)()
    out[0].n_boxes = 5
    assert _stage(L, [4096, 8192], (4, 4), (5, 7), [None, none], out) == 0, L.last_error()
    assert [(o.n_boxes, bool(o.stats), bool(o.average_saturation)) for o in out] == [(0, False, False)] * 2
    L.lib.phd_free_box_stats(out, 2)
    del keep


def test_free_on_zeroed_and_null_input():
    L = _lib()
    from photohive_dsp_amd.structures import PhdBoxStats
    out = (PhdBoxStats * 3)()
    L.lib.phd_free_box_stats(out, 3)
    L.lib.phd_free_box_stats(out, 3)
    L.lib.phd_free_box_stats(None, 3)
    L.lib.phd_free_box_stats(out, 0)
    assert all(o.n_boxes == 0 and not o.stats and not o.average_saturation for o in out)


def test_twin_rejects_bad_arguments():
    L = _lib()
    img = np.zeros((4, 5, 3), np.uint8)
    st, sb = np.zeros((2, 6)), np.zeros(2)
    for boxes, what in (([(0, 5, 0, 5)], "(crop 0)"), ([(0, 4, 0, 5), (0, 4, 3, 2)], "(crop 1)")):
        cb, keep = bsc.crop_boundaries(boxes)
        assert L.lib.phd_debug_box_stats_host(img.ctypes.data, 4, 5, ctypes.byref(cb), st.ctypes.data, sb.ctypes.data,
                                              None) == -1
        assert what in L.last_error()
    cb, keep = bsc.crop_boundaries([(0, 4, 0, 5)])
    assert L.lib.phd_debug_box_stats_host(None, 4, 5, ctypes.byref(cb), st.ctypes.data, sb.ctypes.data, None) == -1
    assert L.lib.phd_debug_box_stats_host(img.ctypes.data, 4, 5, ctypes.byref(cb), None, sb.ctypes.data, None) == -1
    assert L.lib.phd_debug_box_stats_host(img.ctypes.data, 0, 5, ctypes.byref(cb), st.ctypes.data, sb.ctypes.data,
                                          None) == -1


# the smallest shapes where the plan can go wrong: one pixel; a few; a row longer
# than one pass of a block; an odd width (3 W is odd, so the rows sit at every
# 4-byte phase) with more than one band
SHAPES = [(1, 1), (3, 5), (7, 4099), (257, 1031)]


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_twin_sums_equal_python_integers_at_every_base_phase(h, w):
    img = bsc.random_image(h, w, 5 * h + w)
    boxes = bsc.box_list(h, w, h + w)
    want = bsc.expected_sums(img, boxes)
    vals = bsc.expected_u8(img, boxes)
    for off in range(4):
        got_vals, got = bsc.host_twin(bsc.at_offset(img, off), boxes)
        assert got == want, f"base + {off}"
        # stats bitwise stats_from_sums' formula, S-bar the defined finish
        np.testing.assert_array_equal(bsc.bits(got_vals), bsc.bits(vals), err_msg=f"base + {off}")
    for rec, (t, bo, l, r) in zip(want, boxes):
        assert rec[7] == (bo - t) * (r - l) and sum(rec[8:]) <= 255 * rec[7]


def test_twin_without_sums_and_single_colour_boxes():
    """A constant box: contrast exactly 0; black: S-bar 0; white: d = 0;
    a primary: every pixel on the 0.999999 path."""
    img, boxes = bsc.special_image()
    got, _ = bsc.host_twin(img, boxes, want_sums=False)
    np.testing.assert_array_equal(bsc.bits(got), bsc.bits(bsc.expected_u8(img, boxes)))
    np.testing.assert_array_equal(got[0, 3:6], 0.0)
    np.testing.assert_array_equal(got[0, :3], np.array([37, 121, 200]) / 255.0)
    assert got[1, 6] == 0.0 and not got[1, :6].any()
    assert got[2, 6] == 0.0 and (got[2, :3] == 1.0).all() and not got[2, 3:6].any()
    assert got[3, 6] == (float(133 * 63) - (1.0 - 0.999999) * float(133 * 63)) / float(133 * 63)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_on_reference_fixtures(case):
    """The twin on the 8-bit image of every fixture against the compiled
    reference's values (a deep case: on the 8-bit image its doubles came from is
    no comparison, so its numpy restatement on the doubles is checked instead)."""
    fx = bsc.fixture(case["name"])
    boxes = [tuple(int(v) for v in b) for b in fx["boxes"]]
    assert boxes == bsc.case_boxes(case) and len(boxes) == case["boxes"]
    assert sorted(fx) == ["average_saturation", "boxes", "stats"]
    img = bsc.case_image(case)
    want = bsc.fixture_values(fx)
    if case["deep"]:
        bsc.assert_close(bsc.expected_doubles(img, boxes), want, boxes, case["name"])
        return
    got, _ = bsc.host_twin(img, boxes, want_sums=False)
    bsc.assert_close(got, want, boxes, case["name"])
