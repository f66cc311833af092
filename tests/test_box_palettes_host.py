"""Box palettes without a device: the symbols and the struct, the argument
checks that come before any HIP call, the free, and the host twin
(phd_debug_box_counts_host: the counting kernel's own item plan and row code,
box_tiles.h) against plain numpy on synthetic maps and on every committed
label fixture."""
import ctypes

import numpy as np
import pytest

from tests import box_palette_cases as bc
from tests import deep_label_cases as dc
from tests import label_cases as lc

CASES = lc.manifest()
DEEP = dc.manifest()


def _lib():
    from photohive_dsp_amd import lib as L
    return L


def test_symbols_types_and_struct_layout():
    L = _lib()
    from photohive_dsp_amd.structures import PhdBoxPalette
    for name in ("phd_box_palettes_device", "phd_free_box_palettes", "phd_debug_box_counts_host"):
        assert getattr(L.lib, name).argtypes is not None, name
    assert L.BOX_PALETTES_KERNEL == 11
    assert ctypes.sizeof(PhdBoxPalette) == 16
    assert (PhdBoxPalette.n_boxes.offset, PhdBoxPalette.n_slots.offset, PhdBoxPalette.counts.offset) == (0, 4, 8)
    import os
    from tests.conftest import ROOT
    with open(os.path.join(ROOT, "include", "photohive_dsp.h")) as f:
        h = f.read()
    for s in ("typedef struct phd_box_palette {", "int phd_box_palettes_device(", "void phd_free_box_palettes(",
              "int phd_debug_box_counts_host(", "11 box_palettes"):
        assert s in h, s


def _stage(L, maps, hs, ws, ns, boxes, out, n=None):
    n = len(maps) if n is None else n
    from photohive_dsp_amd.structures import Crop_Boundaries
    cbs = (ctypes.POINTER(Crop_Boundaries) * len(maps))(*[ctypes.pointer(b) if b is not None else None for b in boxes])
    return L.lib.phd_box_palettes_device((ctypes.c_void_p * len(maps))(*maps), (ctypes.c_int * len(maps))(*hs),
                                         (ctypes.c_int * len(maps))(*ws), n, (ctypes.c_int * len(maps))(*ns), cbs,
                                         out, None)


def test_stage_rejects_bad_arguments_before_touching_hip():
    """With or without a device: the map pointers below are never dereferenced."""
    L = _lib()
    from photohive_dsp_amd.structures import PhdBoxPalette
    good, keep0 = bc.crop_boundaries([(0, 4, 0, 5)])
    inverted, keep1 = bc.crop_boundaries([(0, 4, 0, 5), (3, 2, 0, 5)])
    past, keep2 = bc.crop_boundaries([(0, 4, 0, 5), (0, 4, 0, 5), (0, 4, 1, 8)])
    negative, keep3 = bc.crop_boundaries([(-1, 4, 0, 5)])

    def call(maps=(4096, 8192), hs=(4, 4), ws=(5, 7), ns=(3, 3), boxes=(good, good)):
        out = (PhdBoxPalette * 2)()
        for o in out:
            o.n_boxes, o.n_slots = 7, 7
        rc = _stage(L, list(maps), hs, ws, ns, list(boxes), out)
        assert rc == -1
        assert all(o.n_boxes == 0 and o.n_slots == 0 and not o.counts for o in out), "out is left zeroed"
        return L.last_error()

    assert "phd_box_palettes_device: map 1: NULL map" in call(maps=(4096, None))
    assert "map 1: height and width must be positive" in call(hs=(4, 0))
    assert "map 0: height and width must be positive" in call(ws=(-5, 7))
    assert "map 1: n_slots must be in 0..4096" in call(ns=(4096, 4097))
    assert "map 0: n_slots" in call(ns=(-1, 3))
    msg = call(boxes=(good, inverted))
    assert "map 1: box 1 " in msg and "inverted or outside" in msg
    msg = call(boxes=(good, past))
    assert "map 1: box 2 " in msg and "4 x 7 map" in msg
    msg = call(boxes=(negative, good))
    assert "map 0: box 0 " in msg
    out = (PhdBoxPalette * 2)()
    assert L.lib.phd_box_palettes_device(None, None, None, 2, None, None, out, None) == -1
    assert "phd_box_palettes_device: NULL argument" in L.last_error()
    assert _stage(L, [4096, 8192], (4, 4), (5, 7), (3, 3), [good, good], out, n=0) == -1
    assert "n_maps" in L.last_error()
    del keep0, keep1, keep2, keep3


def test_maps_without_boxes_need_no_device():
    L = _lib()
    from photohive_dsp_amd.structures import PhdBoxPalette
    none, keep = bc.crop_boundaries([])
    out = (PhdBoxPalette * 2)()
    assert _stage(L, [4096, 8192], (4, 4), (5, 7), (3, 9), [None, none], out) == 0, L.last_error()
    assert [(o.n_boxes, o.n_slots, bool(o.counts)) for o in out] == [(0, 3, False), (0, 9, False)]
    L.lib.phd_free_box_palettes(out, 2)
    del keep


def test_free_on_zeroed_and_null_input():
    L = _lib()
    from photohive_dsp_amd.structures import PhdBoxPalette
    out = (PhdBoxPalette * 3)()
    L.lib.phd_free_box_palettes(out, 3)
    L.lib.phd_free_box_palettes(out, 3)
    L.lib.phd_free_box_palettes(None, 3)
    L.lib.phd_free_box_palettes(out, 0)
    assert all(o.n_boxes == 0 and o.n_slots == 0 and not o.counts for o in out)


def test_twin_rejects_bad_boxes():
    L = _lib()
    lab = np.zeros((4, 5), np.uint16)
    out = np.zeros((2, 4), np.uint32)
    for boxes, what in (([(0, 5, 0, 5)], "box 0 "), ([(0, 4, 0, 5), (0, 4, 3, 2)], "box 1 ")):
        cb, keep = bc.crop_boundaries(boxes)
        assert L.lib.phd_debug_box_counts_host(lab.ctypes.data, 4, 5, 3, ctypes.byref(cb), out.ctypes.data) == -1
        assert what in L.last_error()
    cb, keep = bc.crop_boundaries([(0, 4, 0, 5)])
    assert L.lib.phd_debug_box_counts_host(lab.ctypes.data, 4, 5, 4097, ctypes.byref(cb), out.ctypes.data) == -1
    assert L.lib.phd_debug_box_counts_host(None, 4, 5, 3, ctypes.byref(cb), out.ctypes.data) == -1


SYN = bc.synthetic_maps()


@pytest.mark.parametrize("k", range(len(SYN)), ids=[s[0] for s in SYN])
def test_twin_on_synthetic_maps(k):
    _, lab, ns, boxes = SYN[k]
    got = bc.host_counts(lab, boxes, ns)
    want = bc.expected_counts(lab, boxes, ns)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got.sum(axis=1, dtype=np.int64), [(b - t) * (r - l) for t, b, l, r in boxes])


def test_twin_at_every_base_phase():
    """The same map at each of the four 2-byte phases of an 8-byte word."""
    lab = bc.random_map(37, 131, 17, 5)
    boxes = bc.box_list(37, 131, 6)
    want = bc.expected_counts(lab, boxes, 17)
    for e in range(4):
        np.testing.assert_array_equal(bc.host_counts(bc.at_offset(lab, e), boxes, 17), want)


def _check_fixture(lab, ds, height, width, counts, n_none, pct):
    mh, mw = lab.shape
    ns = len(counts)
    img_boxes = bc.box_list(height, width, 17, empty=False)
    boxes = [bc.image_to_map_box(b, ds, mh, mw) for b in img_boxes]
    assert boxes[0] == (0, mh, 0, mw)
    got = bc.host_counts(lab, boxes, ns)
    np.testing.assert_array_equal(got, bc.expected_counts(lab, boxes, ns))
    np.testing.assert_array_equal(got[0, :ns], counts)
    assert int(got[0, ns]) == n_none
    if pct is not None:
        mine = got[0, :ns].astype(np.float64) * (1.0 / float(mh * mw))
        np.testing.assert_array_equal(mine.view(np.int64), np.asarray(pct, np.float64).view(np.int64))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_twin_on_label_fixtures(case):
    from tests.conftest import golden_case
    fx = lc.fixture(case["name"])
    lab = np.ascontiguousarray(lc.expected_map(case, fx))
    pct = golden_case(case["base"])["palette_pct"] if case["base"] else None
    _check_fixture(lab, case["config"].get("downsample_rate", 1), case["height"], case["width"], fx["counts"],
                   len(fx["dropped"]), pct)


@pytest.mark.parametrize("case", DEEP, ids=[c["name"] for c in DEEP])
def test_twin_on_deep_label_fixtures(case):
    fx = dc.fixture(case["name"])
    lab = np.ascontiguousarray(fx["map"].astype(np.uint16))
    _check_fixture(lab, case["config"].get("downsample_rate", 1), case["height"], case["width"], fx["counts"],
                   int(np.count_nonzero(lab == lc.NONE)), fx["percentages"])


def test_image_to_map_box_rule():
    """rows ceil(top / r) .. min(ceil(bottom / r), mh): the elements whose
    nominal position (y * r, x * r) lies inside the box."""
    for r, h, w in ((2, 720, 1280), (3, 700, 900), (3, 701, 902)):
        mh, mw = h // r, w // r
        for box in bc.box_list(h, w, 9, empty=False):
            t, bo, l, rt = bc.image_to_map_box(box, r, mh, mw)
            ys = [y for y in range(mh) if box[0] <= y * r < box[1]]
            xs = [x for x in range(mw) if box[2] <= x * r < box[3]]
            assert (bo - t, rt - l) == (len(ys), len(xs))
            assert (not ys or (t, bo) == (ys[0], ys[-1] + 1)) and (not xs or (l, rt) == (xs[0], xs[-1] + 1))
    assert bc.image_to_map_box((3, 9, 4, 8), 1, 10, 10) == (3, 9, 4, 8)
