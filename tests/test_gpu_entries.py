"""The device batch entries share one driver (phd_entries.cpp,
run_device_batch): the same images through phd_report_batch_device, _crops,
_mixed, _mixed_crops, _views and _typed_views, on two lanes and on one, give
the same reports.  17 images of 401x577 (no compile-time FFT plan; enough
images for the lane split, 9 + 8) and 3 of 512x512 (a compile-time plan).
A size the reference rejects fails its own group of a views, typed or YUV
call and no other."""
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
