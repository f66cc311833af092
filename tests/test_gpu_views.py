"""Image views on the MI355X: the pack kernel (pack_views.hip) byte for byte
against numpy over every layout, offset and pitch of tests/view_cases.py with
guard bytes around every destination, and phd_report_batch_device_views
against phd_report_batch_device_mixed over packed copies of the same pixels
(the arithmetic behind the gather is unchanged, so the comparison is exact but
for the atomically summed fields)."""
import ctypes

import numpy as np
import pytest

from tests.sharp_boxes import box, three, twelve
from tests.test_gpu_parity import _phd
from tests.view_cases import LAYOUTS, OFFSETS, PITCH_EXTRA, view_case

pytestmark = pytest.mark.gpu

PACK_SHAPES = [(1, 1), (5, 7), (17, 67), (33, 129), (352, 401), (9, 515)]      # (the last: a whole-block row)
GUARD = 0xA5


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_pack_kernel_byte_for_byte(name):
    """One phd_pack_views_device call (one launch) per layout holds the views
    of every shape, base offset 0..3 and pitch minimum + {0, 1, 4}; the
    destinations sit at byte offsets 0..3 inside one tensor prefilled with
    0xA5.  Packed bytes equal numpy's; every guard byte is still 0xA5."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.structures import PhdImageView
    cases, src_parts, src_at, dst_at = [], [], 0, 64
    for h, w in PACK_SHAPES:
        for off in OFFSETS:
            for extra in PITCH_EXTRA:
                buf, data_off, strides, want = view_case(name, h, w, off, extra)
                doff = (off + extra + h) % 4
                cases.append((h, w, src_at + data_off, strides, want, dst_at + doff))
                pad = (-len(buf)) % 16
                src_parts += [buf, np.zeros(pad, np.uint8)]
                src_at += len(buf) + pad
                dst_at += (3 * h * w + doff + 48 + 15) // 16 * 16          # >= 48 guard bytes between images
    src = torch.from_numpy(np.concatenate(src_parts)).cuda()
    dst = torch.full((dst_at + 64,), GUARD, dtype=torch.uint8, device="cuda")
    n = len(cases)
    views = (PhdImageView * n)(*[PhdImageView(src.data_ptr() + s, h, w, *st) for h, w, s, st, _, _ in cases])
    dsts = (ctypes.c_void_p * n)(*[dst.data_ptr() + d for *_, d in cases])
    torch.cuda.synchronize()
    assert L.lib.phd_pack_views_device(views, n, dsts, None) == 0, L.last_error()
    got = dst.cpu().numpy()
    written = np.zeros(len(got), bool)
    for h, w, _, st, want, d in cases:
        assert np.array_equal(got[d:d + 3 * h * w].reshape(h, w, 3), want), (name, h, w, st, d % 4)
        written[d:d + 3 * h * w] = True
    assert (got[~written] == GUARD).all(), "a byte outside the destinations was written"


def test_pack_views_device_wrapper():
    """The Python wrapper on torch tensors: a [N, 3, H, W] batch, BGRA frames
    and an expanded grey plane give the packed tensors torch itself makes."""
    phd, L, torch = _phd()
    g = torch.Generator().manual_seed(3)
    chw = torch.randint(0, 256, (3, 3, 37, 53), dtype=torch.uint8, generator=g).cuda()
    for got, t in zip(phd.pack_views_device(chw, "CHW"), chw):
        assert torch.equal(got, t.permute(1, 2, 0).contiguous())
    bgra = torch.randint(0, 256, (2, 40, 61, 4), dtype=torch.uint8, generator=g).cuda()
    for got, t in zip(phd.pack_views_device(bgra, bgr=True), bgra):
        assert torch.equal(got, t[..., [2, 1, 0]].contiguous())
    gray = torch.randint(0, 256, (29, 31), dtype=torch.uint8, generator=g).cuda()
    got = phd.pack_views_device([gray[..., None].expand(29, 31, 3)])[0]
    assert torch.equal(got, gray[..., None].expand(29, 31, 3).contiguous())


# ---- reports from views --------------------------------------------------------

SIZES = [(352, 400), (401, 577), (480, 640)]


class Mixed:
    """Images of several sizes on the GPU, each in another layout, as views
    (with the tensors that own the memory) and as packed copies."""

    def __init__(self, sizes, per_size=2, seed0=900):
        phd, L, torch = _phd()
        from photohive_dsp_amd import make_views, synth
        self.views, self.keep, self.packed, self.layouts = [], [], [], []
        kinds = ("structured", "uniform", "hblur", "dominant")
        makers = [self._chw, self._rgba, self._bgr, self._pitched, self._roi, self._packed]
        k = 0
        for h, w in sizes:
            for _ in range(per_size):
                img = torch.from_numpy(synth.make(kinds[k % len(kinds)], h, w, seed0 + k)).cuda()
                tensor, layout, bgr = makers[k % len(makers)](torch, img, h, w)
                v, keep = make_views([tensor], layout, bgr)
                self.views.append(v[0])
                self.keep += keep
                self.packed.append(img.contiguous())
                self.layouts.append(makers[k % len(makers)].__name__)
                k += 1
        torch.cuda.synchronize()

    @staticmethod
    def _chw(torch, img, h, w):
        return img.permute(2, 0, 1).contiguous(), "CHW", False

    @staticmethod
    def _rgba(torch, img, h, w):
        alpha = torch.full((h, w, 1), 200, dtype=torch.uint8, device=img.device)
        return torch.cat([img, alpha], dim=2).contiguous(), "HWC", False

    @staticmethod
    def _bgr(torch, img, h, w):
        return img[..., [2, 1, 0]].contiguous(), "HWC", True

    @staticmethod
    def _pitched(torch, img, h, w):
        frame = torch.full((h, w + 5, 3), 77, dtype=torch.uint8, device=img.device)
        frame[:, :w] = img
        return frame[:, :w], "HWC", False

    @staticmethod
    def _roi(torch, img, h, w):
        frame = torch.full((h + 8, w + 9, 3), 33, dtype=torch.uint8, device=img.device)
        frame[5:-3, 7:-2] = img
        return frame[5:-3, 7:-2], "HWC", False

    @staticmethod
    def _packed(torch, img, h, w):
        return img.contiguous(), "HWC", False

    def boxes(self):
        """per image: boxes flush with the last row and column among them"""
        out = []
        for i, v in enumerate(self.views):
            h, w = v.height, v.width
            out.append([twelve(h, w), three(h, w), None, [box(h - 9, h, w - 11, w)]][i % 4])
        return out


_cache = {}


def _mixed():
    if "mixed" not in _cache:
        _cache["mixed"] = Mixed(SIZES)
    return _cache["mixed"]


def _reference(key, mixed, **kw):
    """reports_device_mixed over the packed copies, once per configuration"""
    if key not in _cache:
        phd, L, torch = _phd()
        _cache[key] = phd.reports_device_mixed(mixed.packed, **kw)
    return _cache[key]


def _assert_same(got, want, what=""):
    assert got.color_palette.group_ids == want.color_palette.group_ids, what
    assert got.color_palette.quantities == want.color_palette.quantities, what
    assert np.array_equal(np.array(got.blur_profile.bins), np.array(want.blur_profile.bins)), what
    assert [(v.angle, v.magnitude) for v in got.blur_vectors] == [(v.angle, v.magnitude) for v in want.blur_vectors]
    assert got.sharpnesses == want.sharpnesses, what
    # fp64 sums from atomics: order-dependent in the last bits (tests/test_gpu_round2.py)
    assert got.average_saturation == pytest.approx(want.average_saturation, rel=1e-12), what
    for f in ("Br", "Bg", "Bb", "Cr", "Cg", "Cb"):
        assert getattr(got.rgb_stats, f) == pytest.approx(getattr(want.rgb_stats, f), rel=1e-12), (what, f)


@pytest.mark.parametrize("ds", [1, 2])
def test_reports_from_views_equal_reports_from_packed_copies(ds):
    """One call: 352x400, 401x577 and 480x640, two of each, as CHW, RGBA, BGR,
    pitched, a region of interest of a larger frame and an already packed
    image, with per-image boxes; downsample_rate 1 and 2."""
    phd, L, torch = _phd()
    m = _mixed()
    assert sorted(set(m.layouts)) == ["_bgr", "_chw", "_packed", "_pitched", "_rgba", "_roi"]
    kw = dict(salient_characters=m.boxes(), downsample_rate=ds)
    want = _reference(("boxes", ds), m, **kw)
    got = phd.reports_device_views(m.views, **kw)
    assert len(got) == len(want) == 6
    for i, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, (i, m.layouts[i]))


def _pack_launches(L):
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert L.lib.phd_profile_read(L.PACK_VIEWS_KERNEL, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    return cnt.value


def test_packed_view_is_not_copied():
    """Profile bit 6 (pack_views): no launch when every view is packed, one
    launch when one CHW view sits among packed ones."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import make_views, synth
    imgs = [torch.from_numpy(synth.make("structured", 352, 400, 950 + i)).cuda() for i in range(3)]
    chw = imgs[1].permute(2, 0, 1).contiguous()
    v_chw, _ = make_views([chw], "CHW")
    try:
        assert L.lib.phd_profile_kernels(1 << L.PACK_VIEWS_KERNEL) == 0
        all_packed = phd.reports_device_views(imgs)
        assert _pack_launches(L) == 0
        assert L.lib.phd_profile_kernels(1 << L.PACK_VIEWS_KERNEL) == 0
        one_chw = phd.reports_device_views([imgs[0], v_chw[0], imgs[2]])
        assert _pack_launches(L) == 1
    finally:
        L.lib.phd_profile_kernels(0)
    for a, b in zip(all_packed, one_chw):
        _assert_same(a, b)


def test_bad_view_fails_alone():
    """pixel_stride = 0 in one view of three: the C call returns 1, that image
    has no report and a negative status, the others their reports; the Python
    wrapper raises RuntimeError naming the image."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import _finish, make_config
    from photohive_dsp_amd.structures import Full_Report_Data, PhdImageView
    m = _mixed()
    want = _reference(("plain", 1), m)
    views = (PhdImageView * 3)(m.views[0], m.views[1], m.views[2])
    views[1].pixel_stride = 0
    cfg = make_config()
    outs = (ctypes.POINTER(Full_Report_Data) * 3)()
    st = (ctypes.c_int * 3)()
    rc = L.lib.phd_report_batch_device_views(views, 3, ctypes.byref(cfg), None, outs, st, None)
    assert rc == 1, L.last_error()
    assert st[0] == 0 and st[1] < 0 and st[2] == 0
    assert not outs[1]
    assert "image 1" in L.last_error() and "pixel_stride" in L.last_error()
    for i in (0, 2):
        _assert_same(_finish(outs[i], views[i].height, views[i].width, {}), want[i], i)
    with pytest.raises(RuntimeError, match="image 1"):
        phd.reports_device_views(list(views))


def test_lanes_one_and_two():
    """Four size groups under phd_set_lanes(1) and (2): the groups go to the
    lanes in turn, each lane with its own staging images."""
    phd, L, torch = _phd()
    if "four" not in _cache:
        _cache["four"] = Mixed(SIZES + [(384, 512)], per_size=2, seed0=930)
    m = _cache["four"]
    want = _reference(("four", 1), m, salient_characters=m.boxes())
    prev = L.lib.phd_set_lanes(1)
    try:
        one = phd.reports_device_views(m.views, salient_characters=m.boxes())
        L.lib.phd_set_lanes(2)
        two = phd.reports_device_views(m.views, salient_characters=m.boxes())
    finally:
        L.lib.phd_set_lanes(prev)
    for i, w in enumerate(want):
        _assert_same(one[i], w, ("one lane", i, m.layouts[i]))
        _assert_same(two[i], w, ("two lanes", i, m.layouts[i]))


def test_view_still_being_produced_on_a_side_stream():
    """The call is made on a non-default torch stream while a producer on that
    stream is still writing the CHW tensor (tests/test_gpu_round2.py:
    test_device_input_produced_by_async_torch_op): the gather is enqueued
    behind it, and the reports are the finished tensor's."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    src = torch.from_numpy(synth.structured(600, 800, 5)).cuda().permute(2, 0, 1).contiguous()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = torch.randn(6144, 6144, device="cuda")
        for _ in range(4):
            a = a @ a                                   # keeps the stream busy for milliseconds
            a = a / a.abs().max()
        t = (src.to(torch.int16) + (a[0, 0] * 0).to(torch.int16)).to(torch.uint8)
        got = phd.reports_device_views([t], "CHW")[0]
    side.synchronize()
    assert torch.equal(t, src)
    want = phd.reports_device_mixed([src.permute(1, 2, 0).contiguous()])[0]
    _assert_same(got, want)


def test_repeat_and_teardown():
    """The same mixed call twice (the staging images are reused across groups
    of different sizes), then once more after phd_shutdown()."""
    phd, L, torch = _phd()
    m = _mixed()
    want = _reference(("plain", 1), m)
    for round_ in ("first", "second"):
        for i, g in enumerate(phd.reports_device_views(m.views)):
            _assert_same(g, want[i], (round_, i, m.layouts[i]))
    torch.cuda.synchronize()
    L.lib.phd_shutdown()
    for i, g in enumerate(phd.reports_device_views(m.views)):
        _assert_same(g, want[i], ("after shutdown", i, m.layouts[i]))


def test_single_size_batch_on_two_lanes():
    """Sixteen views of one size: one size group, split in two so that both
    lanes work (as phd_report_batch_device splits its batch); each half packs
    its own views into its lane's staging images."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    imgs = [torch.from_numpy(synth.make(("uniform", "structured")[i % 2], 352, 400, 970 + i)).cuda() for i in range(16)]
    chw = torch.stack(imgs).permute(0, 3, 1, 2).contiguous()
    want = phd.reports_device_mixed(imgs)
    prev = L.lib.phd_set_lanes(2)
    try:
        assert L.lib.phd_profile_kernels(1 << L.PACK_VIEWS_KERNEL) == 0
        got = phd.reports_device_views(chw, "CHW")
        assert _pack_launches(L) == 2
    finally:
        L.lib.phd_profile_kernels(0)
        L.lib.phd_set_lanes(prev)
    for i, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, i)
