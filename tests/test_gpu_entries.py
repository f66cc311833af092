"""The device batch entries share one driver (phd_entries.cpp,
run_device_batch): the same images through phd_report_batch_device, _crops,
_mixed, _mixed_crops and _views, on two lanes and on one, give the same
reports.  17 images of 401x577 (no compile-time FFT plan; enough images for
the lane split, 9 + 8) and 3 of 512x512 (a compile-time plan)."""
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
        }
    finally:
        L.lib.phd_set_lanes(prev)
    for entry, reports in got.items():
        assert len(reports) == n == 20, entry
        for i, (g, w) in enumerate(zip(reports, want)):
            _assert_same(g, w, (entry, lanes, i))


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
