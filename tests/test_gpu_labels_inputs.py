"""Palette label maps of views, typed views and YUV frames on the device
(phd_report_batch_device_views_labels, _typed_views_labels, _yuv_labels).

8-bit route (views, YUV frames, typed views found 8-bit): the map is the one
phd_report_batch_device_mixed_labels gives for the same packed bytes, and the
8-bit fixtures' (tests/label_cases.py).  fp64 route (typed views that are not
8-bit; k_planar_labels, planar.hip): the reference's own maps on the doubles
(tests/golden/labels_deep_*.npz, tests/deep_label_cases.py), element for
element and by SHA-256, and per slot percentages[i] == (double)count(label ==
i) * (1.0 / (double)(mh*mw)) bit for bit.

Reports are compared as tests/test_gpu_labels.py compares a report with a map
to one without (_assert_same_report): palette order, percentages, RGB
statistics, bins, blur vectors and sharpness bit for bit; palette h / s / v
and S-bar at 1e-12 relative, because both calls add those fp64 sums with
atomics that land in any order (two runs of one call differ there too)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import deep_label_cases as dc
from tests import label_cases as lc
from tests.test_gpu_labels import (CASES, FILL, GUARD, Guarded, _assert_count_identity, _assert_same_report, _call,
                                   _dev, _expected, _image, _single)
from tests.test_gpu_parity import _phd

pytestmark = pytest.mark.gpu

DEEP = {c["name"]: c for c in dc.manifest()}
assert GUARD == 64


def _entry(kind, views, kw, maps, crops=None, labels_entry=True):
    """phd_report_batch_device_<kind>[_labels] over a list of descriptors; maps:
    a label pointer or None per image, or None for d_labels == NULL.
    (rc, reports or None per image, statuses)"""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import _finish, make_config
    from photohive_dsp_amd.structures import Full_Report_Data
    n = len(views)
    arr = (type(views[0]) * n)(*views)
    cfg = make_config(**kw)
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    if labels_entry:
        lab = (ctypes.c_void_p * n)(*maps) if maps is not None else None
        rc = getattr(L.lib, f"phd_report_batch_device_{kind}_labels")(arr, n, ctypes.byref(cfg), crops, lab, outs, st,
                                                                      None)
    else:
        assert maps is None
        rc = getattr(L.lib, f"phd_report_batch_device_{kind}")(arr, n, ctypes.byref(cfg), crops, outs, st, None)
    reps = [_finish(outs[i], arr[i].height, arr[i].width, kw) if st[i] == 0 else None for i in range(n)]
    return rc, reps, list(st)


def _map_shape(view, kw):
    return lc.map_shape(view.height, view.width, kw.get("downsample_rate", 1))


def _guards(torch, views, kw, off=0):
    return [Guarded(torch, int(np.prod(_map_shape(v, kw))), off=off) for v in views]


# ---- 1. views ---------------------------------------------------------------------------

def _three_layouts(torch, img):
    """(views, tensors) of one [H, W, 3] device image as planar CHW, as pitched
    BGRA read through channel_stride = -1, and as a region of a larger frame."""
    from photohive_dsp_amd import make_views
    h, w = int(img.shape[0]), int(img.shape[1])
    chw = img.permute(2, 0, 1).contiguous()
    bgra = torch.full((h, w + 5, 4), 201, dtype=torch.uint8, device=img.device)
    bgra[:, :w, :3] = img[..., [2, 1, 0]]
    frame = torch.full((h + 8, w + 9, 3), 33, dtype=torch.uint8, device=img.device)
    frame[5:-3, 7:-2] = img
    v0, _ = make_views([chw], "CHW")
    v1, _ = make_views([bgra[:, :w]], "HWC", bgr=True)
    v2, _ = make_views([frame[5:-3, 7:-2]], "HWC")
    assert v1[0].channel_stride == -1 and v1[0].pixel_stride == 4 and v1[0].row_stride == 4 * (w + 5)
    assert v2[0].row_stride == 3 * (w + 9)
    return [v0[0], v1[0], v2[0]], [chw, bgra, frame]


@pytest.mark.parametrize("name", ["uniform_401x577_L64", "structured_720x1280_ds2"])
def test_views_get_the_packed_images_map(name):
    phd, L, torch = _phd()
    kw = CASES[name]["config"]
    want = _expected(name)
    views, keep = _three_layouts(torch, _dev(torch, _image(name)))
    bufs = _guards(torch, views, kw)
    rc, reps, st = _entry("views", views, kw, [b.ptr for b in bufs])
    assert rc == 0 and st == [0, 0, 0], L.last_error()
    one, rep1 = _single(name)                                  # the mixed-labels call on the packed bytes
    np.testing.assert_array_equal(one, want)
    for k, (b, rep) in enumerate(zip(bufs, reps)):
        b.assert_guards((name, k))
        got = b.map(want.shape)
        np.testing.assert_array_equal(got, want, err_msg=f"{name}, layout {k}")
        assert lc.map_sha256(got) == lc.fixture(name)["sha256"].tobytes()
        _assert_same_report(rep, rep1, (name, k))
        _assert_count_identity(got, rep, (name, k))


def test_views_wrapper_returns_int16_maps():
    phd, L, torch = _phd()
    name = "structured_720x1280_ds2"
    chw = _dev(torch, _image(name)).permute(2, 0, 1).contiguous()
    reps, maps = phd.reports_device_views([chw], layout="CHW", labels=True, **CASES[name]["config"])
    assert len(reps) == len(maps) == 1
    assert maps[0].dtype == torch.int16 and tuple(maps[0].shape) == (360, 640) and maps[0].device == chw.device
    np.testing.assert_array_equal(maps[0].cpu().numpy().view(np.uint16), _expected(name))
    img = phd.quantize_device(maps, reps)[0]                   # quantize_device works on these maps unchanged
    assert tuple(img.shape) == (360, 640, 3) and img.dtype == torch.uint8


# ---- 2. YUV frames ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _yuv_frames():
    """A 401 x 577 NV12 surface (odd sizes, pitch > width, triangle chroma) and a
    401 x 577 YUY2 frame: (views, tensors)."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    from tests.test_gpu_yuv_views import Frames, _ycc_planes
    nv12, t0, _, _ = Frames._nv12_pitched(torch, *_ycc_planes(synth.make("uniform", 401, 577, 21)), (0, 0, 1))
    yuy2, t1, _, _ = Frames._yuy2(torch, *_ycc_planes(synth.make("structured", 401, 577, 22)), (1, 1, 0))
    assert nv12.y_row_stride > nv12.width and nv12.chroma == 1 and nv12.height % 2 == 1 and nv12.width % 2 == 1
    torch.cuda.synchronize()
    return [nv12, yuy2], [t0, t1]


@pytest.mark.parametrize("kw", [dict(linked_list_size=64), dict(linked_list_size=64, downsample_rate=2)],
                         ids=["ds1", "ds2"])
def test_yuv_frames_get_the_converted_images_map(kw):
    phd, L, torch = _phd()
    views, keep = _yuv_frames()
    rgb = phd.convert_yuv_device(views)
    want_bufs = _guards(torch, views, kw)
    rc, want_reps, st = _call(rgb, kw, [b.ptr for b in want_bufs])
    assert rc == 0 and st == [0, 0], L.last_error()
    bufs = _guards(torch, views, kw)
    rc, reps, st = _entry("yuv", views, kw, [b.ptr for b in bufs])
    assert rc == 0 and st == [0, 0], L.last_error()
    for k, (b, wb) in enumerate(zip(bufs, want_bufs)):
        b.assert_guards(k)
        assert np.array_equal(b.host(), wb.host()), f"frame {k}: map differs from the packed call's"
        _assert_same_report(reps[k], want_reps[k], k)
        _assert_count_identity(b.map(_map_shape(views[k], kw)), reps[k], k)
    assert int((bufs[0].map(_map_shape(views[0], kw)) == lc.NONE).sum()) > 0       # noise at L = 64 drops pixels
    # the wrapper on the NV12 surface's tensors (a YUY2 frame is a descriptor: no tensor to allocate beside)
    reps2, maps = phd.reports_device_yuv([phd.nv12_planes(keep[0], 401, 577)], chroma="triangle", labels=True, **kw)
    m = maps[0]
    assert m.dtype == torch.int16 and tuple(m.shape) == _map_shape(views[0], kw) and m.device == keep[0].device
    np.testing.assert_array_equal(m.cpu().numpy().view(np.uint16), bufs[0].map(tuple(m.shape)))
    _assert_same_report(reps2[0], reps[0], "wrapper")


# ---- 3. typed views, 8-bit route -----------------------------------------------------------

def _typed(tensors, layout="HWC", **kw):
    from photohive_dsp_amd import make_typed_views
    v, keep = make_typed_views(tensors, layout, **kw)
    return [v[i] for i in range(len(keep))]


def _u16_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


@pytest.mark.parametrize("name", ["uniform_401x577_L64", "structured_720x1280_ds2"])
def test_typed_view_found_eight_bit_gets_the_eight_bit_map(name):
    """uint16 k * 257 is k / 255 exactly: the classifier routes it to the RGB8
    run, whose label launch writes the fixture's map."""
    phd, L, torch = _phd()
    kw = CASES[name]["config"]
    want = _expected(name)
    t = _u16_dev(torch, _image(name).astype(np.uint16) * 257)
    views = _typed([t])
    b = _guards(torch, views, kw)[0]
    rc, reps, st = _entry("typed_views", views, kw, [b.ptr])
    assert rc == 0 and st == [0], L.last_error()
    b.assert_guards(name)
    np.testing.assert_array_equal(b.map(want.shape), want)
    one, rep1 = _single(name)
    np.testing.assert_array_equal(b.map(want.shape), one)
    _assert_same_report(reps[0], rep1, name)


# ---- 4. typed views, fp64 route --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _deep(name):
    img = dc.image(DEEP[name])
    img.setflags(write=False)
    return img


def _deep_tensor(torch, name, form):
    img = _deep(name)
    if form == "u16_hwc":
        return _u16_dev(torch, dc.u16_of(img)), "HWC"
    return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda(), "CHW"


def _assert_deep(lab, rep, name, what=""):
    fx = dc.fixture(name)
    bad = np.flatnonzero(lab.reshape(-1) != fx["map"].reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} labels differ, first at {bad[:5]}: {lab.reshape(-1)[bad[:5]]} for "
                           f"{fx['map'].reshape(-1)[bad[:5]]}")
    assert lc.map_sha256(lab) == fx["sha256"].tobytes(), what
    q = np.array(rep.color_palette.quantities)
    assert len(q) == len(fx["counts"]), what
    got = lc.percentages(lc.slot_counts(lab, len(q)), lab.size)
    assert np.array_equal(got.view(np.int64), q.view(np.int64)), what
    assert np.array_equal(q.view(np.int64), fx["percentages"].view(np.int64)), what


@pytest.mark.parametrize("form,off", [("u16_hwc", 0), ("f64_chw", 1)])
@pytest.mark.parametrize("name", list(DEEP))
def test_fp64_route_against_the_reference(name, form, off):
    """The reference's map on the doubles, with the destination 8-byte aligned
    (one 8-byte store per 4 pixels) and at base + 2 bytes (four u16 stores).
    141553 pixels: 35388 groups of four and one pixel for the tail lane; odd,
    so the green plane is not 16-byte aligned (its elementwise loads) while
    red and blue are."""
    phd, L, torch = _phd()
    kw = DEEP[name]["config"]
    t, layout = _deep_tensor(torch, name, form)
    views = _typed([t], layout)
    b = _guards(torch, views, kw, off=off)[0]
    assert b.ptr % 8 == 2 * off
    prev = L.lib.phd_set_lanes(1)
    assert L.lib.phd_profile_kernels(1 << L.PALETTE_LABELS_KERNEL) == 0
    try:
        rc, reps, st = _entry("typed_views", views, kw, [b.ptr])
        tot, cnt = ctypes.c_double(), ctypes.c_long()
        assert L.lib.phd_profile_read(L.PALETTE_LABELS_KERNEL, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    finally:
        L.lib.phd_profile_kernels(0)
        L.lib.phd_set_lanes(prev)
    assert rc == 0 and st == [0], L.last_error()
    assert cnt.value == 1 and tot.value > 0, "one label launch of the fp64 pipeline, in profile slot 10"
    b.assert_guards((name, form))
    _assert_deep(b.map(tuple(DEEP[name]["shape"])), reps[0], name, (name, form))
    plain = phd.reports_device_typed([t], layout=layout, **kw)[0]
    _assert_same_report(reps[0], plain, (name, form))


def test_typed_wrapper_returns_int16_maps():
    phd, L, torch = _phd()
    name = "structured_706x802_ds2_L40"
    t, layout = _deep_tensor(torch, name, "u16_hwc")
    reps, maps = phd.reports_device_typed([t], layout=layout, labels=True, **DEEP[name]["config"])
    assert maps[0].dtype == torch.int16 and tuple(maps[0].shape) == (353, 401) and maps[0].device == t.device
    got = maps[0].cpu().numpy()
    _assert_deep(got.view(np.uint16), reps[0], name)
    assert int((got == -1).sum()) == DEEP[name]["dropped"]
    assert tuple(phd.quantize_device(maps, reps)[0].shape) == (353, 401, 3)


# ---- 5. one mixed batch ------------------------------------------------------------------------

def test_mixed_batch_routes_null_destination_and_a_nan_image():
    """One call, linked_list_size = 50: 401 x 577 images on the 8-bit route (a
    uint8 view, a uint16 k * 257 view, a uint8 view with a NULL destination)
    and 353 x 401 images on the fp64 route (uint16 HWC, float64 CHW) with a
    float32 image holding a NaN.  The NaN image fails alone; every buffer's 64
    canary elements on both sides stay intact, the failed image's included;
    the other maps are right; one lane and two give the same."""
    phd, L, torch = _phd()
    kw = dict(linked_list_size=50)
    n8 = ("uniform_401x577_L64", "motion_401x577_L64", "structured_577x401_L64")
    nd = ("structured_353x401_L50", "dominant_353x401_L50")
    img8 = [_image(n8[0]), _image(n8[1]), np.ascontiguousarray(_image(n8[2]).transpose(1, 0, 2))]
    assert all(a.shape == (401, 577, 3) for a in img8)
    nan = _deep(nd[0]).astype(np.float32)
    nan[200, 123, 1] = np.nan
    d0, l0 = _deep_tensor(torch, nd[0], "u16_hwc")
    d1, l1 = _deep_tensor(torch, nd[1], "f64_chw")
    tensors = [_dev(torch, img8[0]), d0, _u16_dev(torch, img8[1].astype(np.uint16) * 257), torch.from_numpy(nan).cuda(),
               _dev(torch, img8[2]), d1]
    views = (_typed([tensors[0]]) + _typed([d0], l0) + _typed([tensors[2]]) + _typed([tensors[3]]) +
             _typed([tensors[4]]) + _typed([d1], l1))
    null, bad = 4, 3
    # the 8-bit route's yardstick: the packed call on the same bytes with this configuration
    want8 = _guards(torch, [views[0], views[2]], kw)
    rc, reps8, st8 = _call([_dev(torch, img8[0]), _dev(torch, img8[1])], kw, [b.ptr for b in want8])
    assert rc == 0 and st8 == [0, 0], L.last_error()
    results = []
    prev = L.lib.phd_set_lanes(1)
    try:
        for lanes in (1, 2):
            L.lib.phd_set_lanes(lanes)
            bufs = [None if i == null else g for i, g in enumerate(_guards(torch, views, kw, off=0))]
            rc, reps, st = _entry("typed_views", views, kw, [b.ptr if b else None for b in bufs])
            err = L.last_error()
            assert rc == 1 and [s == 0 for s in st] == [i != bad for i in range(6)], (lanes, st, err)
            assert reps[bad] is None
            if lanes == 1:                                     # (two lanes: the last failing lane's message stays)
                assert f"image {bad}" in err and "finite" in err, err
            for i, b in enumerate(bufs):
                if b is not None:
                    b.assert_guards((lanes, i))
            shape8, shaped = (401, 577), (353, 401)
            np.testing.assert_array_equal(bufs[0].map(shape8), want8[0].map(shape8), err_msg=f"lanes {lanes}, image 0")
            np.testing.assert_array_equal(bufs[2].map(shape8), want8[1].map(shape8), err_msg=f"lanes {lanes}, image 2")
            _assert_same_report(reps[0], reps8[0], (lanes, 0))
            _assert_same_report(reps[2], reps8[1], (lanes, 2))
            _assert_deep(bufs[1].map(shaped), reps[1], nd[0], (lanes, 1))
            _assert_deep(bufs[5].map(shaped), reps[5], nd[1], (lanes, 5))
            assert reps[null] is not None
            results.append((st, [None if b is None else b.host() for b in bufs], reps))
    finally:
        L.lib.phd_set_lanes(prev)
    (st1, h1, r1), (st2, h2, r2) = results
    assert st1 == st2
    for i, (a, b) in enumerate(zip(h1, h2)):
        assert (a is None and b is None) or np.array_equal(a, b), f"image {i}: one lane and two differ"
    for i in range(6):
        if i != bad:
            _assert_same_report(r1[i], r2[i], i)


# ---- 6. no maps ------------------------------------------------------------------------------------

def test_null_labels_is_the_call_without_maps():
    """d_labels == NULL through each _labels entry, and labels=False through
    each wrapper, against the existing entries on the same inputs."""
    phd, L, torch = _phd()
    kw = dict(linked_list_size=64)
    u8 = "uniform_401x577_L64"
    chw = _dev(torch, _image(u8)).permute(2, 0, 1).contiguous()
    from photohive_dsp_amd import make_views
    vv, _ = make_views([chw], "CHW")
    d0, l0 = _deep_tensor(torch, "structured_353x401_L50", "u16_hwc")
    tv = _typed([_u16_dev(torch, _image(u8).astype(np.uint16) * 257)]) + _typed([d0], l0)
    yv, _keep = _yuv_frames()
    for kind, views, wrapper in (("views", [vv[0]], lambda: phd.reports_device_views([chw], layout="CHW", **kw)),
                                 ("typed_views", tv, None), ("yuv", yv, lambda: phd.reports_device_yuv(yv, **kw))):
        rc0, want, st0 = _entry(kind, views, kw, None, labels_entry=False)
        rc1, got, st1 = _entry(kind, views, kw, None)
        assert rc0 == rc1 == 0 and st0 == st1 == [0] * len(views), (kind, L.last_error())
        for k, (g, w) in enumerate(zip(got, want)):
            _assert_same_report(g, w, (kind, k))
        if wrapper:
            res = wrapper()
            assert isinstance(res, list) and len(res) == len(views)
            for k, (g, w) in enumerate(zip(res, want)):
                _assert_same_report(g, w, (kind, "wrapper", k))
    res = phd.reports_device_typed([d0], layout=l0, labels=False, **kw)
    assert isinstance(res, list) and len(res) == 1
    _assert_same_report(res[0], _entry("typed_views", _typed([d0], l0), kw, None, labels_entry=False)[1][0], "typed")
