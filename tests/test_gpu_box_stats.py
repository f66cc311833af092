"""Box statistics on the device (box_stats.hip: k_box_stats; planar.hip:
k_planar_box_stats) against the host twin, the fixtures of the compiled
reference (tests/golden/box_stats_*.npz) and numpy.

Bars: the 8-bit results equal the host twin bit for bit and a second run is
identical (integer atomics); a whole-image box equals the report's rgb_stats bit
for bit; against the reference means and contrasts rtol 1e-9 (contrasts atol
max(1e-12, N 2^-53)), S-bar rtol max(1e-12, N 2^-53)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import box_stats_cases as bsc
from tests.test_gpu_parity import _phd

pytestmark = pytest.mark.gpu

KW = dict(linked_list_size=64)
CASES = {c["name"]: c for c in bsc.manifest()}
GUARD = 0xA5


def _take(L, bs, n):
    """numpy [n_boxes, 7] copies of n filled phd_box_stats structs; the C blocks are freed."""
    out = []
    for i in range(n):
        nb = bs[i].n_boxes
        a = np.zeros((nb, 7))
        if nb:
            st = np.ctypeslib.as_array(ctypes.cast(bs[i].stats, ctypes.POINTER(ctypes.c_double)), shape=(nb, 6))
            a[:, :6] = st
            a[:, 6] = np.ctypeslib.as_array(bs[i].average_saturation, shape=(nb,))
            # one block: the saturations follow the statistics
            assert ctypes.addressof(bs[i].average_saturation.contents) == \
                ctypes.addressof(bs[i].stats.contents) + 48 * nb
        else:
            assert not bs[i].stats and not bs[i].average_saturation
        out.append(a)
    L.lib.phd_free_box_stats(bs, n)
    assert all(not bs[i].stats and bs[i].n_boxes == 0 for i in range(n))
    return out


def _crops(box_lists):
    from photohive_dsp_amd.structures import Crop_Boundaries
    made = [bsc.crop_boundaries(b) if b is not None else None for b in box_lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * len(box_lists))(*[ctypes.pointer(m[0]) if m else None for m in made])
    return arr, made


def _upload(torch, img, off):
    """The image on the device `off` bytes past a 256-byte boundary inside a larger
    tensor whose other bytes are GUARD: (tensor, pointer)."""
    buf = torch.full((img.size + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    o = 16 + off
    buf[o:o + img.size] = torch.tensor(np.ascontiguousarray(img).reshape(-1), device="cuda")
    return buf, buf.data_ptr() + o


def _stage(ptrs, shapes, box_lists):
    phd, L, torch = _phd()
    from photohive_dsp_amd.structures import PhdBoxStats
    n = len(ptrs)
    crops, keep = _crops(box_lists)
    bs = (PhdBoxStats * n)()
    rc = L.lib.phd_box_stats_device((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*[s[0] for s in shapes]),
                                    (ctypes.c_int * n)(*[s[1] for s in shapes]), n, crops, bs, None)
    assert rc == 0, L.last_error()
    del keep
    return _take(L, bs, n)


def _launches(L, kernel):
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert L.lib.phd_profile_read(kernel, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    return cnt.value


@functools.lru_cache(maxsize=None)
def _twin(name):
    """(image, boxes, the host twin's [n, 7]) of a fixture case (8-bit)."""
    case = CASES[name]
    img, boxes = bsc.case_image(case), bsc.case_boxes(case)
    img.setflags(write=False)
    return img, boxes, bsc.host_twin(np.ascontiguousarray(img), boxes, want_sums=False)[0]


def test_stage_alone_sizes_bases_and_one_launch():
    """One call over images of different sizes at device bases + 0 .. + 3, one
    boxes[i] NULL; guard bytes around every image; one launch in slot 12."""
    phd, L, torch = _phd()
    imgs = [bsc.random_image(h, w, 9 * h + w) for h, w in ((1, 1), (3, 5), (7, 4099), (257, 1031))]
    imgs += [np.ascontiguousarray(_twin(n)[0]) for n in ("structured_353x350", "special_350x351")]
    boxes = [bsc.box_list(im.shape[0], im.shape[1], 11 + k) for k, im in enumerate(imgs)]
    boxes[5] = _twin("special_350x351")[1]
    boxes[1] = None
    ups = [_upload(torch, im, (k + 1) % 4) for k, im in enumerate(imgs)]
    assert {p % 4 for _, p in ups} == {0, 1, 2, 3}
    ptrs, shapes = [p for _, p in ups], [im.shape[:2] for im in imgs]
    assert L.lib.phd_profile_kernels(1 << L.BOX_STATS_KERNEL) == 0
    try:
        got = _stage(ptrs, shapes, boxes)
        assert _launches(L, L.BOX_STATS_KERNEL) == 1, "every box of every image in one launch"
    finally:
        L.lib.phd_profile_kernels(0)
    again = _stage(ptrs, shapes, boxes)
    for k, (im, b, g, g2) in enumerate(zip(imgs, boxes, got, again)):
        if b is None:
            assert g.shape == (0, 7)
            continue
        want = bsc.host_twin(im, b, want_sums=False)[0]
        np.testing.assert_array_equal(bsc.bits(g), bsc.bits(want), err_msg=f"image {k}: differs from the host twin")
        np.testing.assert_array_equal(bsc.bits(g2), bsc.bits(g), err_msg=f"image {k}: second run")
    bsc.assert_close(got[5], bsc.fixture_values(bsc.fixture("special_350x351")), boxes[5], "special")
    for buf, _ in ups:                                           # the guards are as they were
        h = buf.cpu().numpy()
        assert (h[:16] == GUARD).all() and (h[-44:] == GUARD).all()


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c["deep"]])
def test_stage_alone_against_the_reference_fixtures(name):
    phd, L, torch = _phd()
    img, boxes, twin = _twin(name)
    buf, p = _upload(torch, img, 3)
    got = _stage([p], [img.shape[:2]], [boxes])[0]
    np.testing.assert_array_equal(bsc.bits(got), bsc.bits(twin))
    bsc.assert_close(got, bsc.fixture_values(bsc.fixture(name)), boxes, name)


def test_four_thousand_small_boxes():
    """More items than resident blocks, and runs of items that cross boxes."""
    phd, L, torch = _phd()
    img = bsc.random_image(350, 350, 3)
    rng = np.random.default_rng(4)
    boxes = [(int(t), int(t) + 8, int(l), int(l) + 8)
             for t, l in zip(rng.integers(0, 343, 4000), rng.integers(0, 343, 4000))]
    buf, p = _upload(torch, img, 1)
    got = _stage([p], [(350, 350)], [boxes])[0]
    want = bsc.host_twin(img, boxes, want_sums=False)[0]
    np.testing.assert_array_equal(bsc.bits(got), bsc.bits(want))


# ---- the report entries ------------------------------------------------------------------------

def _run(kind, srcs, kw, box_lists, maps=None, palettes=False, stats=True):
    """phd_report_batch_device_<kind>_box_stats; srcs: device tensors [H, W, 3]
    (kind "mixed") or descriptors.  (rc, reports, statuses, palettes or None,
    statistics or None)"""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import _finish, make_config
    from photohive_dsp_amd.structures import Full_Report_Data, PhdBoxPalette, PhdBoxStats
    from tests.test_gpu_box_palettes import _take as take_palettes
    n = len(srcs)
    cfg = make_config(**kw)
    crops, keep = _crops(box_lists) if box_lists is not None else (None, None)
    lab = (ctypes.c_void_p * n)(*maps) if maps is not None else None
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    bp = (PhdBoxPalette * n)() if palettes else None
    bs = (PhdBoxStats * n)() if stats else None
    if stats:
        for o in bs:                                             # the call zeroes them first
            o.n_boxes = 5
    if kind == "mixed":
        ptrs = (ctypes.c_void_p * n)(*[im.data_ptr() for im in srcs])
        hs = (ctypes.c_int * n)(*[int(im.shape[0]) for im in srcs])
        ws = (ctypes.c_int * n)(*[int(im.shape[1]) for im in srcs])
        rc = L.lib.phd_report_batch_device_mixed_box_stats(ptrs, hs, ws, n, ctypes.byref(cfg), crops, lab, bp, bs,
                                                           outs, st, None)
        sizes = list(zip(hs, ws))
    else:
        arr = (type(srcs[0]) * n)(*srcs)
        rc = getattr(L.lib, f"phd_report_batch_device_{kind}_box_stats")(arr, n, ctypes.byref(cfg), crops, lab, bp, bs,
                                                                         outs, st, None)
        sizes = [(v.height, v.width) for v in srcs]
    reps = [_finish(outs[i], *sizes[i], kw) if st[i] == 0 else None for i in range(n)]
    del keep
    return rc, reps, list(st), (take_palettes(L, bp, n) if palettes else None), (_take(L, bs, n) if stats else None)


def _report_stats(rep):
    s = rep.rgb_stats
    return np.array([s.Br, s.Bg, s.Bb, s.Cr, s.Cg, s.Cb])


def test_packed_entry_whole_image_box_rate_two_and_no_label_work():
    phd, L, torch = _phd()
    name = "structured_353x350"
    img, boxes, twin = _twin(name)
    assert boxes[0] == (0, 353, 0, 350)
    t = torch.tensor(img, device="cuda")
    mask = (1 << L.PALETTE_LABELS_KERNEL) | (1 << L.BOX_PALETTES_KERNEL) | (1 << L.BOX_STATS_KERNEL)
    assert L.lib.phd_profile_kernels(mask) == 0
    try:
        rc, reps, st, _, stats = _run("mixed", [t], KW, [boxes])    # d_labels and box_palettes NULL
        assert rc == 0 and st == [0], L.last_error()
        assert _launches(L, L.PALETTE_LABELS_KERNEL) == 0 and _launches(L, L.BOX_PALETTES_KERNEL) == 0
        assert _launches(L, L.BOX_STATS_KERNEL) == 1
    finally:
        L.lib.phd_profile_kernels(0)
    np.testing.assert_array_equal(bsc.bits(stats[0]), bsc.bits(twin))
    np.testing.assert_array_equal(bsc.bits(stats[0][0, :6]), bsc.bits(_report_stats(reps[0])),
                                  err_msg="a whole-image box is the report's rgb_stats bit for bit")
    n = 353 * 350
    np.testing.assert_allclose(stats[0][0, 6], reps[0].average_saturation, rtol=max(1e-12, n * 2.0 ** -53), atol=0)
    # downsample_rate plays no part
    rc, reps2, st, _, stats2 = _run("mixed", [t], dict(KW, downsample_rate=2), [boxes])
    assert rc == 0 and st == [0], L.last_error()
    np.testing.assert_array_equal(bsc.bits(stats2[0]), bsc.bits(twin))
    np.testing.assert_array_equal(bsc.bits(_report_stats(reps2[0])), bsc.bits(_report_stats(reps[0])))


def test_null_box_stats_is_the_box_palettes_call():
    phd, L, torch = _phd()
    from tests.test_gpu_box_palettes import _run as run_palettes
    from tests.test_gpu_box_palettes import _same_report
    img, boxes, twin = _twin("dominant_400x357")
    t = torch.tensor(img, device="cuda")
    rc0, reps0, st0, pals0 = run_palettes("mixed", [t], KW, None, [boxes])
    rc1, reps1, st1, pals1, none = _run("mixed", [t], KW, [boxes], palettes=True, stats=False)
    rc2, reps2, st2, pals2, stats = _run("mixed", [t], KW, [boxes], palettes=True)
    assert rc0 == rc1 == rc2 == 0 and st0 == st1 == st2 == [0] and none is None, L.last_error()
    for reps, pals in ((reps1, pals1), (reps2, pals2)):
        _same_report(reps[0], reps0[0])
        np.testing.assert_array_equal(pals[0], pals0[0])
    np.testing.assert_array_equal(bsc.bits(stats[0]), bsc.bits(twin))


def test_one_mixed_call_on_one_lane_and_two():
    """Two sizes; images with boxes, without boxes (NULL and N == 0) and with a
    bad box: it fails alone and keeps {0, NULL, NULL}."""
    phd, L, torch = _phd()
    names = ["uniform_350x351", "structured_353x350", "grayish_350x351", "posterized_353x350", "uniform_350x351",
             "structured_353x350"]
    imgs = [torch.tensor(_twin(n)[0], device="cuda") for n in names]
    box_lists = [_twin(names[0])[1], _twin(names[1])[1], None, [], [(0, 10, 0, 10), (5, 4, 0, 10)], _twin(names[5])[1]]
    bad = 4
    results = []
    prev = L.lib.phd_set_lanes(1)
    try:
        for lanes in (1, 2):
            L.lib.phd_set_lanes(lanes)
            rc, reps, st, _, stats = _run("mixed", imgs, KW, box_lists)
            assert rc == 1 and [s == 0 for s in st] == [i != bad for i in range(len(names))], (st, L.last_error())
            assert stats[bad].shape == (0, 7) and reps[bad] is None
            for i, n in enumerate(names):
                if i == bad:
                    continue
                if not box_lists[i]:
                    assert stats[i].shape == (0, 7)
                    continue
                np.testing.assert_array_equal(bsc.bits(stats[i]), bsc.bits(_twin(n)[2]), err_msg=f"{lanes} lanes, {i}")
            results.append(stats)
    finally:
        L.lib.phd_set_lanes(prev)
    for a, b in zip(*results):
        np.testing.assert_array_equal(bsc.bits(a), bsc.bits(b))


def test_views_yuv_and_typed_eight_bit_equal_the_packed_entry():
    """A pitched BGRA view and a region of a larger frame; an NV12 surface with
    triangle chroma against the packed entry over phd_convert_yuv_device's bytes;
    uint16 k * 257 (the 8-bit route)."""
    phd, L, torch = _phd()
    from tests.test_gpu_labels_inputs import _three_layouts, _typed, _u16_dev, _yuv_frames
    name = "uniform_350x351"
    img, boxes, twin = _twin(name)
    t = torch.tensor(img, device="cuda")
    rc, reps, st, _, packed = _run("mixed", [t], KW, [boxes])
    assert rc == 0 and st == [0], L.last_error()
    np.testing.assert_array_equal(bsc.bits(packed[0]), bsc.bits(twin))
    views, keep = _three_layouts(torch, t)
    rc, reps, st, _, stats = _run("views", views[1:], KW, [boxes, boxes])
    assert rc == 0 and st == [0, 0], L.last_error()
    for k in range(2):
        np.testing.assert_array_equal(bsc.bits(stats[k]), bsc.bits(packed[0]), err_msg=f"view {k}")
    tv = _typed([_u16_dev(torch, np.ascontiguousarray(img).astype(np.uint16) * 257)])
    rc, reps, st, _, stats = _run("typed_views", tv, KW, [boxes])
    assert rc == 0 and st == [0], L.last_error()
    np.testing.assert_array_equal(bsc.bits(stats[0]), bsc.bits(packed[0]), err_msg="u16 k * 257")
    yv, keep2 = _yuv_frames()
    ybox = bsc.box_list(401, 577, 41)
    rgb = phd.convert_yuv_device(yv[:1])
    rc, reps_p, st, _, stats_p = _run("mixed", rgb, KW, [ybox])
    assert rc == 0 and st == [0], L.last_error()
    rc, reps_y, st, _, stats_y = _run("yuv", yv[:1], KW, [ybox])
    assert rc == 0 and st == [0], L.last_error()
    np.testing.assert_array_equal(bsc.bits(stats_y[0]), bsc.bits(stats_p[0]))
    np.testing.assert_array_equal(bsc.bits(stats_p[0]),
                                  bsc.bits(bsc.host_twin(np.ascontiguousarray(rgb[0].cpu().numpy()), ybox, False)[0]))


# ---- the fp64 route ------------------------------------------------------------------------------

def _deep_views(torch, img, form):
    from tests.test_gpu_labels_inputs import _typed, _u16_dev
    if form == "u16_hwc":
        u = np.rint(img * 65535.0).astype(np.uint16)
        assert np.array_equal(u.astype(np.float64) / 65535.0, img)
        return _typed([_u16_dev(torch, u)])
    return _typed([torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).cuda()], "CHW")


@pytest.mark.parametrize("form", ["u16_hwc", "f64_chw"])
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["deep"]])
def test_fp64_route_against_the_reference(name, form):
    phd, L, torch = _phd()
    case = CASES[name]
    img, boxes = bsc.case_image(case), bsc.case_boxes(case)
    want = bsc.fixture_values(bsc.fixture(name))
    views = _deep_views(torch, img, form)
    assert L.lib.phd_profile_kernels(1 << L.PLANAR_BOX_STATS_KERNEL | 1 << L.BOX_STATS_KERNEL) == 0
    try:
        rc, reps, st, _, stats = _run("typed_views", views, KW, [boxes])
        assert rc == 0 and st == [0], L.last_error()
        assert _launches(L, L.PLANAR_BOX_STATS_KERNEL) == 1 and _launches(L, L.BOX_STATS_KERNEL) == 0
    finally:
        L.lib.phd_profile_kernels(0)
    bsc.assert_close(stats[0], want, boxes, (name, form))
    bsc.assert_close(stats[0], bsc.expected_doubles(img, boxes), boxes, (name, form, "numpy"))
    # the whole-image box against the report's own statistics
    np.testing.assert_allclose(stats[0][0, :6], _report_stats(reps[0]), rtol=bsc.TIGHT_RTOL, atol=1e-12)
    rc, reps2, st, _, again = _run("typed_views", views, KW, [boxes])
    assert rc == 0 and st == [0], L.last_error()
    np.testing.assert_array_equal(bsc.bits(again[0]), bsc.bits(stats[0]), err_msg="a repeat run is bit-identical")


def test_a_nan_image_fails_alone():
    phd, L, torch = _phd()
    from tests.test_gpu_labels_inputs import _typed
    name = "deep_structured_353x350"
    case = CASES[name]
    img, boxes = bsc.case_image(case), bsc.case_boxes(case)
    nan = img.astype(np.float32)
    nan[200, 123, 1] = np.nan
    views = _typed([torch.from_numpy(nan).cuda()]) + _deep_views(torch, img, "u16_hwc")
    rc, reps, st, _, stats = _run("typed_views", views, KW, [boxes, boxes])
    assert rc == 1 and st[0] != 0 and st[1] == 0, L.last_error()
    assert stats[0].shape == (0, 7)
    bsc.assert_close(stats[1], bsc.fixture_values(bsc.fixture(name)), boxes, name)


# ---- Python -------------------------------------------------------------------------------------

def test_python_entry_points():
    """box_stats_device and box_stats=True on the four report wrappers."""
    phd, L, torch = _phd()
    name = "uniform_350x351"
    img, boxes, twin = _twin(name)
    t = torch.tensor(img, device="cuda")
    sal = [[dict(top=b[0], bottom=b[1], left=b[2], right=b[3]) for b in boxes]]

    def same(stats, want=twin):
        assert len(stats) == 1 and stats[0].dtype == np.float64 and stats[0].shape == want.shape
        np.testing.assert_array_equal(bsc.bits(stats[0]), bsc.bits(want))

    got = phd.box_stats_device([t, t], [sal[0], None])
    same(got[:1])
    assert got[1].shape == (0, 7)
    reps, maps, stats = phd.reports_device_labels([t], salient_characters=sal, box_stats=True, **KW)
    same(stats)
    reps, maps, pals, stats = phd.reports_device_labels([t], salient_characters=sal, box_palettes=True,
                                                        box_stats=True, **KW)
    assert pals[0].shape[0] == len(boxes)
    same(stats)
    chw = t.permute(2, 0, 1).contiguous()
    reps, stats = phd.reports_device_views([chw], layout="CHW", salient_characters=sal, box_stats=True, **KW)
    same(stats)
    reps, maps, pals, stats = phd.reports_device_views([chw], layout="CHW", salient_characters=sal, labels=True,
                                                       box_palettes=True, box_stats=True, **KW)
    assert maps[0].dtype == torch.int16 and pals[0].shape[0] == len(boxes)
    same(stats)
    reps, stats = phd.reports_device_views([chw], layout="CHW", box_stats=True, **KW)          # no boxes
    assert stats[0].shape == (0, 7)
    u16 = torch.from_numpy((np.ascontiguousarray(img).astype(np.uint16) * 257).view(np.int16)).cuda().view(torch.uint16)
    reps, stats = phd.reports_device_typed([u16], salient_characters=sal, box_stats=True, **KW)
    same(stats)
    from tests.test_gpu_labels_inputs import _yuv_frames
    yv, keep = _yuv_frames()
    ybox = bsc.box_list(401, 577, 41)
    ysal = [[dict(top=b[0], bottom=b[1], left=b[2], right=b[3]) for b in ybox]]
    frame = [phd.nv12_planes(keep[0], 401, 577)]
    reps, stats = phd.reports_device_yuv(frame, chroma="triangle", salient_characters=ysal, box_stats=True, **KW)
    rgb = phd.convert_yuv_device(yv[:1])
    same(stats, bsc.host_twin(np.ascontiguousarray(rgb[0].cpu().numpy()), ybox, False)[0])
