"""Typed image views on the MI355X: the decode kernel (decode_views.hip) bit
for bit against numpy over every element type and layout of
tests/typed_cases.py with guard doubles around every destination, and
phd_report_batch_device_typed_views against the reference's fixtures, against
get_full_report_data on the same doubles (the fp64 route) and against
reports_device_views on the same 8-bit image (the RGB8 route).

Equality of two reports: bins, blur vectors, statistics, palette group ids and
quantities are compared exactly.  The fields either route sums with fp64
atomics move in their last bits between runs and are held to 1e-12, the bar of
tests/test_gpu_views.py: the average saturation on the RGB8 route (exact on the
fp64 route, whose sums have a fixed order) and the sharpnesses on the fp64
route (exact on the RGB8 route, whose batched kernel merges in a fixed order)."""
import ctypes

import numpy as np
import pytest

from tests.conftest import golden_case, golden_manifest
from tests.sharp_boxes import box, three
from tests.test_gpu_parity import _phd
from tests.typed_cases import ELEMS, F16, F32, F64, LAYOUTS, SNAP, U8, U16, decode, same_doubles, typed_case

pytestmark = pytest.mark.gpu

DECODE_SHAPES = [(1, 1), (3, 5), (37, 61), (350, 352)]
GUARD = -777.0
PLANAR = {c["name"]: c for c in golden_manifest().get("planar_cases", [])}


# ---- 1. the decode kernel against numpy ------------------------------------------

@pytest.mark.parametrize("elem", sorted(ELEMS), ids=[ELEMS[e][0] for e in sorted(ELEMS)])
def test_decode_kernel_bit_for_bit(elem):
    """One phd_decode_views_device call holds every layout at every shape with
    base offsets of 0..3 elements (head, body and tail of a row are all taken)
    and the three max_values; the destinations sit at offsets of 0 and 1
    doubles inside one tensor prefilled with a guard value.  The planes equal
    numpy's decode bit for bit (NaNs by position); every guard is untouched."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.structures import PhdTypedView
    es = np.dtype(ELEMS[elem][1]).itemsize
    cases, src_parts, src_at, dst_at, k = [], [], 0, 8, 0
    for layout in sorted(LAYOUTS):
        for h, w in DECODE_SHAPES:
            for off in ((0, 3) if h > 100 else (0, 1, 2, 3)):
                buf, data_off, strides, raw = typed_case(elem, layout, h, w, off, off % 2 * 4 + off // 2, seed=1)
                mv = (0.0, 1023.0, 255.0)[k % 3]
                doff = (k // 3) % 2
                cases.append((h, w, (src_at + data_off) * es, strides, decode(elem, raw, mv)[0], dst_at + doff, mv))
                pad = (-len(buf)) % (16 // es)
                src_parts += [buf, np.zeros(pad, buf.dtype)]
                src_at += len(buf) + pad
                dst_at += (3 * h * w + doff + 6 + 1) // 2 * 2               # >= 6 guard doubles between images
                k += 1
    src = torch.from_numpy(np.concatenate(src_parts).view(np.uint8)).cuda()
    dst = torch.full((dst_at + 8,), GUARD, dtype=torch.float64, device="cuda")
    assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    n = len(cases)
    views = (PhdTypedView * n)(*[PhdTypedView(src.data_ptr() + s, h, w, *st, elem, 0, mv)
                                 for h, w, s, st, _, _, mv in cases])
    dsts = (ctypes.c_void_p * n)(*[dst.data_ptr() + 8 * d for *_, d, _ in cases])
    torch.cuda.synchronize()
    assert L.lib.phd_decode_views_device(views, n, dsts, None) == 0, L.last_error()
    got = dst.cpu().numpy()
    written = np.zeros(len(got), bool)
    for h, w, _, st, want, d, mv in cases:
        assert same_doubles(got[d:d + 3 * h * w].reshape(3, h, w), want), (ELEMS[elem][0], h, w, st, d % 2, mv)
        written[d:d + 3 * h * w] = True
    assert (got[~written] == GUARD).all(), "a double outside the destinations was written"


def test_decode_views_device_wrapper():
    """The Python wrapper on torch tensors: [N, 3, H, W] halves, BGRA floats and
    10-bit data in 16-bit storage give the planes torch itself makes."""
    phd, L, torch = _phd()
    g = torch.Generator().manual_seed(3)
    chw = torch.rand((2, 3, 37, 53), generator=g).half().cuda()
    for got, t in zip(phd.decode_views_device(chw, "CHW"), chw):
        assert torch.equal(got, t.double())
    bgra = torch.rand((2, 40, 61, 4), generator=g).mul(255).cuda()
    for got, t in zip(phd.decode_views_device(bgra, bgr=True, max_value=255), bgra):
        want = (t.cpu().numpy()[..., [2, 1, 0]].astype(np.float64) / 255.0).transpose(2, 0, 1)   # IEEE division
        assert np.array_equal(got.cpu().numpy(), want)
    ten = np.random.default_rng(4).integers(0, 1024, (29, 31, 3)).astype(np.uint16)
    got = phd.decode_views_device([torch.from_numpy(ten.view(np.int16)).cuda().view(torch.uint16)], max_value=1023)[0]
    assert np.array_equal(got.cpu().numpy(), (ten / 1023.0).transpose(2, 0, 1))


# ---- helpers -----------------------------------------------------------------------

def _legacy(img, cfg=None, crops=None):
    """get_full_report_data on float64 HxWx3 host doubles (tests/test_gpu_planar.py)."""
    from tests.test_gpu_planar import _call
    return _call(np.ascontiguousarray(img), cfg, crops)


def _dev(arr, layout="hwc"):
    """(device tensor, make_typed_views layout) of a numpy HxWx3 array in one of
    the test's layouts; 16-bit unsigned data goes up as int16 storage."""
    import torch

    def up(a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint16:
            return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
        return torch.from_numpy(a).cuda()

    h, w = arr.shape[:2]
    if layout == "hwc":
        return up(arr), "HWC"
    if layout == "chw":
        return up(arr.transpose(2, 0, 1)), "CHW"
    if layout == "chw_roi":                                  # a pitched CHW region of a larger tensor
        frame = np.zeros((3, h + 8, w + 9), arr.dtype)
        frame[:, 5:-3, 7:-2] = arr.transpose(2, 0, 1)
        return up(frame)[:, 5:-3, 7:-2], "CHW"
    if layout == "rgba":
        frame = np.zeros((h, w, 4), arr.dtype)
        frame[..., :3] = arr
        return up(frame), "HWC"
    raise KeyError(layout)


def _stats(r):
    s = r.rgb_stats
    return [s.Br, s.Bg, s.Bb, s.Cr, s.Cg, s.Cb]


def _vectors(r):
    return [(v.angle, v.magnitude) for v in r.blur_vectors]


def _assert_identical(got, want, what="", exact_s=True, hsv_rtol=None):
    assert np.array_equal(np.array(got.blur_profile.bins), np.array(want.blur_profile.bins)), what
    assert _vectors(got) == _vectors(want), what
    assert _stats(got) == _stats(want), what
    assert got.color_palette.group_ids == want.color_palette.group_ids, what
    assert got.color_palette.quantities == want.color_palette.quantities, what
    if exact_s and want.sharpnesses:
        # the fp64 route's sharpness pass (k_sharp_pass) adds its block partials atomically
        assert list(got.sharpnesses) == pytest.approx(list(want.sharpnesses), rel=1e-12), what
    else:
        assert got.sharpnesses == want.sharpnesses, what
    if exact_s:
        assert got.average_saturation == want.average_saturation, what
    else:
        assert got.average_saturation == pytest.approx(want.average_saturation, rel=1e-12), what
    if hsv_rtol is not None:
        np.testing.assert_allclose(np.array(got.color_palette.hsv), np.array(want.color_palette.hsv), rtol=hsv_rtol)


def _u16_of(img):
    """The 16-bit image whose values / 65535.0 are exactly the doubles of synth.deep."""
    u16 = np.rint(img * 65535.0).astype(np.uint16)
    assert np.array_equal(u16 / 65535.0, img)
    return u16


def _typed_c_call(L, views, n, crops=None, **kw):
    """The C call itself: (rc, statuses, reports or None per image)."""
    from photohive_dsp_amd.core import _finish, make_config, normalize_salient
    from photohive_dsp_amd.structures import Full_Report_Data
    cfg = make_config(**kw)
    cr = normalize_salient(crops, n)
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    rc = L.lib.phd_report_batch_device_typed_views(views, n, ctypes.byref(cfg), cr[0] if cr else None, outs, st, None)
    err = L.last_error()
    reps = [_finish(outs[i], views[i].height, views[i].width, kw) if st[i] == 0 else None for i in range(n)]
    return rc, list(st), reps, err


# ---- 2. the reference's fixtures through the new entry -------------------------------

FIXTURES = ["deep_structured_600x800_crops", "deep_uniform_700x900_ds2_L50", "deep_motion_1201x1009_hsv36",
            "deep_dominant_1024x1536"]


@pytest.mark.parametrize("name,layout", [(FIXTURES[0], "hwc"), (FIXTURES[0], "chw_roi")] +
                         [(f, "hwc") for f in FIXTURES[1:]])
def test_reference_fixtures_as_u16(name, layout):
    """The 16-bit device image rint(synth.deep * 65535) decodes to exactly the
    doubles the fixture was made from: the report meets the fixture at the
    bars of tests/test_gpu_planar.py."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    from tests.test_gpu_parity import assert_report_matches
    case = PLANAR[name]
    g = golden_case(name)
    u16 = _u16_of(synth.deep(case["kind"], case["height"], case["width"], case["seed"]))
    t, lay = _dev(u16, layout)
    rep = phd.reports_device_typed([t], lay, salient_characters=[case["crops"]] if case["crops"] else None,
                                   **case["config"])[0]
    assert_report_matches(rep, g)
    np.testing.assert_allclose(_stats(rep), g["stats"], rtol=1e-9)
    np.testing.assert_allclose(rep.average_saturation, float(g["average_saturation"]), rtol=1e-9)
    np.testing.assert_allclose(np.array(rep.color_palette.hsv).reshape(-1, 3), g["palette_hsv"], rtol=1e-9)


# ---- 3. the same doubles by both routes ---------------------------------------------

def test_same_doubles_both_routes():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    img = synth.deep("structured", 400, 400, 3)
    boxes = three(400, 400)
    t, lay = _dev(_u16_of(img))
    got = phd.reports_device_typed([t], lay, salient_characters=[boxes])[0]
    want = _legacy(img, crops=boxes)
    _assert_identical(got, want, hsv_rtol=1e-9)


# ---- 4. 8-bit promotion -----------------------------------------------------------------

def test_eight_bit_images_take_the_rgb8_run():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    u8 = synth.make("structured", 352, 350, 21)
    boxes = [[box(340, 352, 300, 350)]]
    want = phd.reports_device_views([torch.from_numpy(u8).cuda()], salient_characters=boxes)[0]
    f32 = torch.from_numpy(u8).float().div(255)                   # ToTensor()'s values
    for what, arr, layout, kw in (("u16 * 257", u8.astype(np.uint16) * 257, "chw_roi", {}),
                                  ("f64 / 255", u8 / 255.0, "hwc", {}),
                                  ("f32 snap", f32.numpy(), "chw", {"snap_u8": True}),
                                  ("f16 snap", f32.half().numpy(), "rgba", {"snap_u8": True}),
                                  ("u8 * 1, max 255", u8, "chw", {"max_value": 255}),
                                  ("f32 0..255", u8.astype(np.float32), "hwc", {"max_value": 255.0})):
        t, lay = _dev(arr, layout)
        got = phd.reports_device_typed([t], lay, salient_characters=boxes, **kw)[0]
        _assert_identical(got, want, what, exact_s=False)
    # without snap the float image is the doubles its floats widen to: the fp64 route
    t, lay = _dev(f32.numpy(), "chw")
    got = phd.reports_device_typed([t], lay, salient_characters=boxes)[0]
    _assert_identical(got, _legacy(f32.numpy().astype(np.float64), crops=boxes[0]), "f32 no snap", hsv_rtol=1e-9)
    assert got.rgb_stats.Cr != want.rgb_stats.Cr
    # halves that are no table entries: the fp64 route, snap or not
    halves = np.random.default_rng(8).random((352, 350, 3)).astype(np.float16)
    t, lay = _dev(halves, "hwc")
    got = phd.reports_device_typed([t], lay, snap_u8=True)[0]
    _assert_identical(got, _legacy(halves.astype(np.float64)), "random f16", hsv_rtol=1e-9)


# ---- 5. mixed batches, lanes --------------------------------------------------------------

def _mixed_batch():
    """(tensors, layouts, per-image kwargs, boxes): a u16 deep image, a u16 * 257
    image, a float32 snap image and a U8 view; two sizes; boxes on two."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import make_typed_views, synth
    a = _dev(_u16_of(synth.deep("uniform", 352, 350, 5)), "chw")
    b = _dev(synth.make("structured", 352, 350, 6).astype(np.uint16) * 257, "hwc")
    c = _dev(torch.from_numpy(synth.make("hblur", 360, 400, 7)).float().div(255).numpy(), "chw_roi")
    d = _dev(synth.make("dominant", 352, 350, 8), "chw")
    views, keep = [], []
    for (t, lay), snap in ((a, False), (b, False), (c, True), (d, False)):
        v, k = make_typed_views([t], lay, snap_u8=snap)
        views.append(v[0])
        keep += k
    boxes = [three(352, 350), None, [box(351, 360, 389, 400)], None]
    return views, keep, boxes


@pytest.mark.parametrize("lanes", [1, 2])
def test_mixed_batch_equals_images_alone(lanes):
    phd, L, torch = _phd()
    views, keep, boxes = _mixed_batch()
    prev = L.lib.phd_set_lanes(lanes)
    try:
        together = phd.reports_device_typed(views, salient_characters=boxes)
        alone = [phd.reports_device_typed([v], salient_characters=[b])[0] for v, b in zip(views, boxes)]
    finally:
        L.lib.phd_set_lanes(prev)
    for i, (g, w) in enumerate(zip(together, alone)):
        _assert_identical(g, w, i, exact_s=(i == 0), hsv_rtol=1e-9)
    assert together[0].rgb_stats.Cr != together[1].rgb_stats.Cr


def test_single_size_batch_on_two_lanes():
    """Sixteen typed views of one size (fp64 and 8-bit ones alternating): one
    size group, split in two so that both lanes work."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    imgs = []
    for i in range(16):
        if i % 2:
            imgs.append(_dev(synth.make("structured", 352, 350, 40 + i).astype(np.uint16) * 257)[0])
        else:
            imgs.append(_dev(_u16_of(synth.deep("uniform", 352, 350, 40 + i)))[0])
    prev = L.lib.phd_set_lanes(1)
    try:
        want = phd.reports_device_typed(imgs[:4]) + phd.reports_device_typed(imgs[4:])
        L.lib.phd_set_lanes(2)
        assert L.lib.phd_profile_kernels(1 << L.CLASSIFY_VIEWS_KERNEL | 1 << L.DECODE_VIEWS_KERNEL) == 0
        got = phd.reports_device_typed(imgs)
        assert _launches(L, L.CLASSIFY_VIEWS_KERNEL) == 2 and _launches(L, L.DECODE_VIEWS_KERNEL) == 8
    finally:
        L.lib.phd_profile_kernels(0)
        L.lib.phd_set_lanes(prev)
    for i, (g, w) in enumerate(zip(got, want)):
        _assert_identical(g, w, i, exact_s=(i % 2 == 0), hsv_rtol=1e-9)


# ---- 6. failures stay alone ------------------------------------------------------------------

def test_failures_stay_alone():
    phd, L, torch = _phd()
    from photohive_dsp_amd import make_typed_views, synth
    from photohive_dsp_amd.structures import PhdTypedView
    good_a = _dev(_u16_of(synth.deep("uniform", 352, 350, 60)))
    good_b = _dev(synth.make("structured", 352, 350, 61).astype(np.uint16) * 257)
    va, ka = make_typed_views([good_a[0]], good_a[1])
    vb, kb = make_typed_views([good_b[0]], good_b[1])
    want = phd.reports_device_typed([va[0], vb[0]])

    def batch_with(bad_view):
        views = (PhdTypedView * 3)(va[0], bad_view, vb[0])
        rc, st, reps, err = _typed_c_call(L, views, 3)
        assert rc == 1 and st[0] == 0 and st[1] < 0 and st[2] == 0, (rc, st, err)
        assert reps[1] is None
        _assert_identical(reps[0], want[0], "first")
        _assert_identical(reps[2], want[1], "third", exact_s=False)
        assert "image 1" in err, err
        return err

    nan = synth.deep("uniform", 352, 350, 62).astype(np.float32)
    nan[100, 17, 1] = np.nan
    t, lay = _dev(nan, "chw")
    assert "finite" in batch_with(make_typed_views([t], lay)[0][0])
    inf = nan.copy()
    inf[100, 17, 1] = np.inf
    t, lay = _dev(inf, "hwc")
    assert "finite" in batch_with(make_typed_views([t], lay, snap_u8=True)[0][0])
    ten = np.random.default_rng(63).integers(0, 1024, (352, 350, 3)).astype(np.uint16)
    ten[200, 100] = 65535                                      # 64.06: outside the octree
    t, lay = _dev(ten)
    assert "octree" in batch_with(make_typed_views([t], lay, max_value=1023)[0][0])
    t, lay = _dev(_u16_of(synth.deep("uniform", 300, 400, 64)))
    assert "greater than 350" in batch_with(make_typed_views([t], lay)[0][0])
    bad_elem = PhdTypedView(*[getattr(va[0], f) for f, _ in PhdTypedView._fields_])
    bad_elem.elem = 7
    assert "elem" in batch_with(bad_elem)
    with pytest.raises(RuntimeError, match="image 1"):
        phd.reports_device_typed([va[0], bad_elem, vb[0]])


# ---- 7. repeat, teardown, launch counts ----------------------------------------------------------

def _launches(L, kernel):
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert L.lib.phd_profile_read(kernel, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    return cnt.value


def test_repeat_teardown_and_launch_counts():
    """The same mixed call twice, then after phd_shutdown(): statistics, bins
    and vectors bit-identical each time.  Profile bits 7 and 8: one classify
    launch per size group that holds a non-U8 view, one decode launch per
    fp64 image."""
    phd, L, torch = _phd()
    views, keep, boxes = _mixed_batch()
    prev = L.lib.phd_set_lanes(1)
    try:
        assert L.lib.phd_profile_kernels(1 << L.CLASSIFY_VIEWS_KERNEL | 1 << L.DECODE_VIEWS_KERNEL) == 0
        first = phd.reports_device_typed(views, salient_characters=boxes)
        assert _launches(L, L.CLASSIFY_VIEWS_KERNEL) == 2 and _launches(L, L.DECODE_VIEWS_KERNEL) == 1
        L.lib.phd_profile_kernels(0)
        second = phd.reports_device_typed(views, salient_characters=boxes)
        torch.cuda.synchronize()
        L.lib.phd_shutdown()
        third = phd.reports_device_typed(views, salient_characters=boxes)
        # a call of U8 views only launches neither kernel
        assert L.lib.phd_profile_kernels(1 << L.CLASSIFY_VIEWS_KERNEL | 1 << L.DECODE_VIEWS_KERNEL) == 0
        only_u8 = phd.reports_device_typed([views[3]])
        assert _launches(L, L.CLASSIFY_VIEWS_KERNEL) == 0 and _launches(L, L.DECODE_VIEWS_KERNEL) == 0
    finally:
        L.lib.phd_profile_kernels(0)
        L.lib.phd_set_lanes(prev)
    for other in (second, third):
        for i, (g, w) in enumerate(zip(other, first)):
            assert _stats(g) == _stats(w), i
            assert np.array_equal(np.array(g.blur_profile.bins), np.array(w.blur_profile.bins)), i
            assert _vectors(g) == _vectors(w), i
    _assert_identical(only_u8[0], first[3], exact_s=False)
