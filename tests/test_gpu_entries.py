"""The device batch entries share one driver (phd_entries.cpp,
run_device_batch): the same images through phd_report_batch_device, _crops,
_mixed, _mixed_crops, _views and _typed_views, on two lanes and on one, give
the same reports.  17 images of 401x577 (no compile-time FFT plan; enough
images for the lane split, 9 + 8) and 3 of 512x512 (a compile-time plan).
A size the reference rejects fails its own group of a views, typed or YUV
call and no other.  A typed call that asks for label maps, box palettes and box
statistics at once gives every image what a call with that image alone gives."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_parity import _phd
from tests.test_gpu_views import _assert_same

pytestmark = pytest.mark.gpu

SIZES = [((401, 577), 17), ((512, 512), 3)]
_cache = {}


def _images():
    """per size one [N, H, W, 3] device tensor, and the reports of
    phd_report_batch_device on one lane (made once, never changed)"""
    if not _cache:
        phd, L, torch = _phd()
        import numpy as np
        from photohive_dsp_amd import synth
        kinds = ("structured", "uniform", "hblur", "dominant")
        batches, k = [], 0
        for (h, w), n in SIZES:
            batches.append(torch.from_numpy(np.stack([synth.make(kinds[(k + i) % 4], h, w, 700 + k + i)
                                                      for i in range(n)])).cuda())
            k += n
        torch.cuda.synchronize()
        prev = L.lib.phd_set_lanes(1)
        try:
            want = [r for b in batches for r in phd.report_device(b)]
        finally:
            L.lib.phd_set_lanes(prev)
        _cache["batches"], _cache["want"] = batches, want
    return _cache["batches"], _cache["want"]


@pytest.mark.parametrize("lanes", [2, 1])
def test_every_device_entry_gives_the_same_reports(lanes):
    phd, L, torch = _phd()
    batches, want = _images()
    singles = [im for b in batches for im in b.unbind(0)]
    n = len(singles)
    none = [None] * n
    prev = L.lib.phd_set_lanes(lanes)
    try:
        got = {
            "device": [r for b in batches for r in phd.report_device(b)],
            "crops": [r for b in batches for r in phd.report_device(b, salient_characters=[None] * len(b))],
            "mixed": phd.reports_device_mixed(singles),
            "mixed_crops": phd.reports_device_mixed(singles, salient_characters=none),
            "views": phd.reports_device_views(singles),
            # U8 typed views, packed: read in place, they join the RGB8 run
            "typed": phd.reports_device_typed(singles),
        }
    finally:
        L.lib.phd_set_lanes(prev)
    for entry, reports in got.items():
        assert len(reports) == n == 20, entry
        for i, (g, w) in enumerate(zip(reports, want)):
            _assert_same(g, w, (entry, lanes, i))


# precheck's message for the 300 x 400 image (src/utilities.c:64-87, no ": " after Width)
_TOO_SMALL = "Error: Image height and width must be greater than 350. Height: 300\tWidth400"
# entry -> (C function, phd_last_error after the call below)
_REJECTED = {
    "views": ("phd_report_batch_device_views", _TOO_SMALL),
    "typed": ("phd_report_batch_device_typed_views", "image 1: " + _TOO_SMALL),
    "yuv": ("phd_report_batch_device_yuv", _TOO_SMALL),
}


def _three_descriptors(entry, torch):
    """352x350, 300x400 (a size precheck rejects: a group of its own) and
    352x350 again as the entry's descriptors: (array, objects to keep alive)"""
    from photohive_dsp_amd import make_typed_views, make_views, make_yuv_views, synth
    imgs = [synth.make(kind, h, w, 760 + i)
            for i, (kind, h, w) in enumerate((("structured", 352, 350), ("uniform", 300, 400), ("hblur", 352, 350)))]
    if entry == "yuv":
        from tests.test_gpu_yuv_views import _ycc_planes
        return make_yuv_views([tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in _ycc_planes(im))
                               for im in imgs])
    tensors = [torch.from_numpy(im).cuda() for im in imgs]
    return make_typed_views(tensors) if entry == "typed" else make_views(tensors)


def _c_call(L, fn, views, n):
    """The C entry itself: (rc, statuses, the out pointers, phd_last_error)."""
    from photohive_dsp_amd.core import make_config
    from photohive_dsp_amd.structures import Full_Report_Data
    cfg = make_config()
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    rc = getattr(L.lib, fn)(views, n, ctypes.byref(cfg), None, outs, st, None)
    return rc, list(st), outs, L.last_error()


@pytest.mark.parametrize("entry", sorted(_REJECTED))
def test_rejected_size_fails_its_group_alone(entry):
    """Three images, the middle one of a size the reference rejects: the call
    returns 1, that image has no report and a negative status, the other two
    the reports of a call without it, and phd_last_error is precheck's message
    -- bare from the views and YUV entries, behind the image's number from the
    typed entry."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import _finish
    fn, message = _REJECTED[entry]
    views, keep = _three_descriptors(entry, torch)
    torch.cuda.synchronize()
    good = (type(views[0]) * 2)(views[0], views[2])
    rc, st, outs, err = _c_call(L, fn, good, 2)
    assert rc == 0 and st == [0, 0], err
    want = [_finish(outs[i], good[i].height, good[i].width, {}) for i in range(2)]
    rc, st, outs, err = _c_call(L, fn, views, 3)
    got = {i: _finish(outs[i], views[i].height, views[i].width, {}) for i in range(3) if st[i] == 0}
    assert rc == 1, err
    assert st[0] == 0 and st[1] < 0 and st[2] == 0
    assert not outs[1]
    _assert_same(got[0], want[0], (entry, 0))
    _assert_same(got[2], want[1], (entry, 2))
    assert err == message
    assert "greater than 350" in err
    assert ("image 1" in err) == (entry == "typed")
    del keep


def test_caller_stream_takes_one_lane():
    """A call on the caller's stream is not split over the lanes."""
    phd, L, torch = _phd()
    batches, want = _images()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    prev = L.lib.phd_set_lanes(2)
    try:
        got = phd.report_device(batches[0], stream=side)
    finally:
        L.lib.phd_set_lanes(prev)
    side.synchronize()
    for i, g in enumerate(got):
        _assert_same(g, want[i], ("stream", i))


# ---- all three per-image outputs at once ---------------------------------------------------------

_BAD, _NO_BOXES, _NO_MAP, _FP64, _U16, _ODD = 4, 2, 3, (0, 1), 5, 16
_KW = dict(linked_list_size=64)


def _outputs_call(views, box_lists, maps, stream=None):
    """phd_report_batch_device_typed_views_box_stats with every output asked
    for; maps: a device tensor or None per image.  (rc, statuses, reports, the
    structs' fields as the call left them, box palettes, box statistics)"""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import _finish, make_config
    from photohive_dsp_amd.structures import Full_Report_Data, PhdBoxPalette, PhdBoxStats, PhdTypedView
    from tests.test_gpu_box_palettes import _take as take_palettes
    from tests.test_gpu_box_stats import _crops
    from tests.test_gpu_box_stats import _take as take_stats
    n = len(views)
    cfg = make_config(**_KW)
    crops, keep = _crops(box_lists)
    lab = (ctypes.c_void_p * n)(*[m.data_ptr() if m is not None else None for m in maps])
    outs, st = (ctypes.POINTER(Full_Report_Data) * n)(), (ctypes.c_int * n)()
    bp, bs = (PhdBoxPalette * n)(), (PhdBoxStats * n)()
    for i in range(n):                                           # the call zeroes them first
        bp[i].n_boxes = bp[i].n_slots = bs[i].n_boxes = 5
    rc = L.lib.phd_report_batch_device_typed_views_box_stats(
        (PhdTypedView * n)(*views), n, ctypes.byref(cfg), crops, lab, bp, bs, outs, st,
        stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    reps = [_finish(outs[i], views[i].height, views[i].width, _KW) if st[i] == 0 else None for i in range(n)]
    raw = [(bp[i].n_boxes, bp[i].n_slots, bool(bp[i].counts), bs[i].n_boxes, bool(bs[i].stats),
            bool(bs[i].average_saturation)) for i in range(n)]
    del keep
    return rc, list(st), reps, raw, take_palettes(L, bp, n), take_stats(L, bs, n)


def _outputs_inputs():
    """The 17 typed views (sixteen 352 x 352, one 360 x 352), their boxes and the
    results of the same entry over each image alone (made once, never changed)."""
    if "outputs" not in _cache:
        phd, L, torch = _phd()
        from photohive_dsp_amd import make_typed_views, synth
        from tests import box_stats_cases as bsc
        from tests.test_gpu_labels_inputs import _u16_dev
        kinds = ("structured", "uniform", "hblur", "dominant")
        u8 = [synth.make(kinds[i % 4], 360 if i == _ODD else 352, 352, 900 + i) for i in range(17)]
        tensors = []
        for i, im in enumerate(u8):
            if i in _FP64:                                       # doubles that are no multiple of 1 / 255
                f = im.astype(np.float64) / 255.0 * 0.999
                assert not np.array_equal(np.rint(f * 255.0) / 255.0, f)
                tensors.append(torch.from_numpy(f).cuda())
            elif i == _U16:                                      # k * 257 / 65535 = k / 255: the 8-bit route, staged
                tensors.append(_u16_dev(torch, im.astype(np.uint16) * 257))
            else:
                tensors.append(torch.from_numpy(im).cuda())
        views, keep = make_typed_views(tensors)
        views = [views[i] for i in range(17)]
        boxes = [bsc.box_list(im.shape[0], im.shape[1], 50 + i) for i, im in enumerate(u8)]
        boxes[_NO_BOXES] = None
        boxes[_BAD] = [(0, 10, 0, 10), (5, 4, 0, 10)]
        torch.cuda.synchronize()
        alone = []
        for i in range(17):
            m = torch.full(u8[i].shape[:2], -2, dtype=torch.int16, device="cuda")
            rc, st, reps, raw, pals, stats = _outputs_call(views[i:i + 1], boxes[i:i + 1], [m])
            assert (rc, st) == ((1, [-1]) if i == _BAD else (0, [0])), (i, L.last_error())
            alone.append((reps[0], m, pals[0], stats[0]))
        _cache["outputs"] = (u8, keep, views, boxes, alone)
    return _cache["outputs"]


def test_all_outputs_follow_their_image_through_groups_and_lanes():
    """Label maps, box palettes and box statistics asked for at once from a typed
    call of two size groups (one per lane on the library's streams; one lane on
    a caller's stream), with fp64-route images, an image without boxes, one
    without a map of the caller's and one with a bad box: every image's outputs
    are those of a call with that image alone, an 8-bit image's also those of
    the stage-only entries on its bytes and map; the failed image keeps zeroed
    structs.  All comparisons are exact."""
    for where in ("two lanes", "caller's stream"):
        _check_all_outputs(where)


def _check_all_outputs(where):
    phd, L, torch = _phd()
    from tests import box_stats_cases as bsc
    from tests.test_gpu_box_palettes import _same_report
    u8, keep, views, boxes, alone = _outputs_inputs()
    n = len(views)
    maps = [None if i == _NO_MAP else torch.full(u8[i].shape[:2], -2, dtype=torch.int16, device="cuda")
            for i in range(n)]
    stream = None
    if where == "caller's stream":
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    prev = L.lib.phd_set_lanes(2)
    try:
        rc, st, reps, raw, pals, stats = _outputs_call(views, boxes, maps, stream)
    finally:
        L.lib.phd_set_lanes(prev)
    assert rc == 1 and st == [-1 if i == _BAD else 0 for i in range(n)], (st, L.last_error())
    assert raw[_BAD] == (0, 0, False, 0, False, False) and reps[_BAD] is None
    packed, packed_boxes, packed_maps, packed_slots, packed_at = [], [], [], [], []
    for i in range(n):
        if i == _BAD:
            continue
        rep1, map1, pal1, stat1 = alone[i]
        if i in _FP64:
            # (the fp64 route's sharpness pass adds its block partials atomically: the bar of
            # tests/test_gpu_typed_views.py; the report is not what this test is about)
            np.testing.assert_allclose(reps[i].sharpnesses, rep1.sharpnesses, rtol=1e-12, atol=0, equal_nan=True)
            reps[i].sharpnesses = rep1.sharpnesses
        _same_report(reps[i], rep1, (where, i))
        if maps[i] is not None:
            assert torch.equal(maps[i], map1), (where, i)
        assert pals[i].shape == pal1.shape == (len(boxes[i] or []), len(rep1.color_palette.colors) + 1)
        np.testing.assert_array_equal(pals[i], pal1, err_msg=f"{where}, image {i}: box palette")
        assert stats[i].shape == stat1.shape == (len(boxes[i] or []), 7)
        np.testing.assert_array_equal(bsc.bits(stats[i]), bsc.bits(stat1), err_msg=f"{where}, image {i}: box stats")
        if i not in _FP64:
            packed.append(torch.from_numpy(u8[i]).cuda())
            packed_boxes.append(boxes[i])
            packed_maps.append(maps[i] if maps[i] is not None else map1)
            packed_slots.append(len(rep1.color_palette.colors))
            packed_at.append(i)
    # the stage-only entries over the 8-bit images' bytes and maps
    sal = [b and [dict(top=t, bottom=bo, left=le, right=ri) for t, bo, le, ri in b] for b in packed_boxes]
    for i, s, p in zip(packed_at, phd.box_stats_device(packed, sal),
                       phd.box_palettes_device(packed_maps, packed_slots, sal)):
        np.testing.assert_array_equal(bsc.bits(stats[i]), bsc.bits(s), err_msg=f"{where}, image {i}: stage stats")
        np.testing.assert_array_equal(pals[i], p, err_msg=f"{where}, image {i}: stage palette")
    del keep
