"""YCbCr views on the MI355X: the conversion kernel (yuv_views.hip) byte for
byte against the numpy restatement of the definition (tests/yuv_cases.py) over
every layout, offset, pitch and mode with guard bytes around every
destination, over all 256^3 triples, and phd_report_batch_device_yuv against
phd_report_batch_device_mixed over the RGB8 images numpy converts the same
frames to (the pipeline behind the conversion is unchanged, so the comparison
is exact but for the atomically summed fields)."""
import ctypes

import numpy as np
import pytest

from tests.sharp_boxes import box, three, twelve
from tests.test_gpu_parity import _phd
from tests.test_gpu_views import _assert_same
from tests.yuv_cases import (LAYOUTS, MODES, OFFSETS, PITCH_EXTRA, SHAPES, TABLE, convert, cube_planes, make_view,
                             yuv_case)

pytestmark = pytest.mark.gpu

BIG = (352, 401)                # many bands of whole rows; its modes go round the cases
GUARD = 0xA5


def _yuv_launches(L):
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert L.lib.phd_profile_read(L.YUV_VIEWS_KERNEL, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    return cnt.value


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_convert_kernel_byte_for_byte(name):
    """One phd_convert_yuv_device call (one launch, profile bit 9) per layout
    holds the views of every shape, base offset 0..3, pitch minimum + {0, 1, 4}
    and mode; the destinations sit at byte offsets 0..3 inside one tensor
    prefilled with 0xA5.  Converted bytes equal numpy's; every guard byte is
    still 0xA5."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.structures import PhdYuvView
    cases, src_parts, src_at, dst_at, k = [], [], 0, 64, 0
    for h, w in SHAPES + [BIG]:
        for off in OFFSETS:
            for extra in PITCH_EXTRA:
                buf, lay, (Y, Cb, Cr) = yuv_case(name, h, w, off, extra)
                k += 1
                for mode in (MODES if (h, w) != BIG else [MODES[k % len(MODES)]]):
                    doff = (off + extra + h + len(cases)) % 4
                    cases.append((h, w, src_at, lay, mode, convert(Y, Cb, Cr, lay["sx"], lay["sy"], *mode),
                                  dst_at + doff))
                    dst_at += (3 * h * w + doff + 48 + 15) // 16 * 16        # >= 48 guard bytes between images
                pad = (-len(buf)) % 16
                src_parts += [buf, np.zeros(pad, np.uint8)]
                src_at += len(buf) + pad
    src = torch.from_numpy(np.concatenate(src_parts)).cuda()
    dst = torch.full((dst_at + 64,), GUARD, dtype=torch.uint8, device="cuda")
    n = len(cases)
    views = (PhdYuvView * n)(*[make_view(src.data_ptr() + s, lay, h, w, mode) for h, w, s, lay, mode, _, _ in cases])
    dsts = (ctypes.c_void_p * n)(*[dst.data_ptr() + d for *_, d in cases])
    torch.cuda.synchronize()
    try:
        assert L.lib.phd_profile_kernels(1 << L.YUV_VIEWS_KERNEL) == 0
        assert L.lib.phd_convert_yuv_device(views, n, dsts, None) == 0, L.last_error()
        assert _yuv_launches(L) == 1
    finally:
        L.lib.phd_profile_kernels(0)
    got = dst.cpu().numpy()
    written = np.zeros(len(got), bool)
    for h, w, _, lay, mode, want, d in cases:
        assert np.array_equal(got[d:d + 3 * h * w].reshape(h, w, 3), want), (name, h, w, mode, d % 4)
        written[d:d + 3 * h * w] = True
    assert (got[~written] == GUARD).all(), "a byte outside the destinations was written"


@pytest.mark.parametrize("matrix,rng", sorted(TABLE))
def test_all_triples_on_device(matrix, rng):
    """All 256^3 (Y, Cb, Cr) triples as one 4096 x 4096 4:4:4 view: the
    kernel's bytes equal the definition's, computed on the GPU with torch
    integer ops."""
    phd, L, torch = _phd()
    Y, Cb, Cr = (torch.from_numpy(p).cuda() for p in cube_planes())
    got = phd.convert_yuv_device([(Y, Cb, Cr)], matrix=("bt601", "bt709")[matrix], full_range=not rng)[0]
    cy, crv, cgu, cgv, cbu, yoff = TABLE[(matrix, rng)]
    u, v = Cb.to(torch.int32) - 128, Cr.to(torch.int32) - 128
    yy = cy * (Y.to(torch.int32) - yoff)
    want = torch.stack([(yy + crv * v + 32768) >> 16, (yy - cgu * u - cgv * v + 32768) >> 16,
                        (yy + cbu * u + 32768) >> 16], dim=-1).clamp_(0, 255).to(torch.uint8)
    assert got.shape == want.shape == (4096, 4096, 3)
    assert torch.equal(got, want)


# ---- reports from YUV frames --------------------------------------------------------

SIZES = [(352, 400), (401, 577), (480, 640)]


def _ycc_planes(img):
    """Full-resolution Y, Cb, Cr planes (uint8) of an RGB8 image: any fixed map will do."""
    r, g, b = (img[..., c].astype(np.float64) for c in range(3))
    y = 0.299 * r + 0.587 * g + 0.114 * b
    to8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)            # noqa: E731
    return to8(y), to8(128 + 0.564 * (b - y)), to8(128 + 0.713 * (r - y))


class Frames:
    """YCbCr frames of several sizes on the GPU, each in another layout and
    mode, as views (with the tensors that own the memory) and as the packed
    RGB8 images numpy converts them to."""

    def __init__(self, sizes, per_size=2, seed0=1200):
        phd, L, torch = _phd()
        from photohive_dsp_amd import synth
        self.views, self.keep, self.rgb, self.layouts = [], [], [], []
        kinds = ("structured", "uniform", "hblur", "dominant")
        makers = [self._nv12_pitched, self._i420, self._yuy2, self._i444, self._nv21, self._i422]
        k = 0
        for h, w in sizes:
            for _ in range(per_size):
                Y, Cb, Cr = _ycc_planes(synth.make(kinds[k % len(kinds)], h, w, seed0 + k))
                mode = MODES[(3 * k + 1) % len(MODES)]
                maker = makers[k % len(makers)]
                view, keep, (sx, sy), (cb, cr) = maker(torch, Y, Cb, Cr, mode)
                self.views.append(view)
                self.keep.append(keep)
                self.rgb.append(torch.from_numpy(convert(Y, cb, cr, sx, sy, *mode)).cuda())
                self.layouts.append((maker.__name__, mode))
                k += 1
        torch.cuda.synchronize()

    @staticmethod
    def _kw(mode):
        m, r, c = mode
        return dict(matrix=("bt601", "bt709")[m], full_range=not r, chroma=("replicate", "triangle")[c])

    @classmethod
    def _planar(cls, torch, Y, cb, cr, mode):
        from photohive_dsp_amd import make_yuv_views
        t = tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in (Y, cb, cr))
        v, _ = make_yuv_views([t], **cls._kw(mode))
        return v[0], t

    @classmethod
    def _i420(cls, torch, Y, Cb, Cr, mode):
        cb, cr = Cb[::2, ::2], Cr[::2, ::2]
        return (*cls._planar(torch, Y, cb, cr, mode), (1, 1), (cb, cr))

    @classmethod
    def _i422(cls, torch, Y, Cb, Cr, mode):
        cb, cr = Cb[:, ::2], Cr[:, ::2]
        return (*cls._planar(torch, Y, cb, cr, mode), (1, 0), (cb, cr))

    @classmethod
    def _i444(cls, torch, Y, Cb, Cr, mode):
        return (*cls._planar(torch, Y, Cb, Cr, mode), (0, 0), (Cb, Cr))

    @classmethod
    def _semi(cls, torch, Y, Cb, Cr, mode, swap, extra):
        from photohive_dsp_amd import make_yuv_views, nv12_planes
        h, w = Y.shape
        cb, cr = Cb[::2, ::2], Cr[::2, ::2]
        ch, cw = cb.shape
        surface = np.full((h + ch + 2, 2 * cw + extra), 91, np.uint8)       # a decoder surface with a pitch
        surface[:h, :w] = Y
        surface[h:h + ch, 0:2 * cw:2] = cr if swap else cb
        surface[h:h + ch, 1:2 * cw:2] = cb if swap else cr
        t = torch.from_numpy(surface).cuda()
        v, _ = make_yuv_views([nv12_planes(t, h, w)], swap_uv=swap, **cls._kw(mode))
        return v[0], t, (1, 1), (cb, cr)

    @classmethod
    def _nv12_pitched(cls, torch, Y, Cb, Cr, mode):
        return cls._semi(torch, Y, Cb, Cr, mode, False, 37)

    @classmethod
    def _nv21(cls, torch, Y, Cb, Cr, mode):
        return cls._semi(torch, Y, Cb, Cr, mode, True, 0)

    @classmethod
    def _yuy2(cls, torch, Y, Cb, Cr, mode):
        from photohive_dsp_amd.structures import PhdYuvView
        h, w = Y.shape
        cb, cr = Cb[:, ::2], Cr[:, ::2]
        cw = cb.shape[1]
        quads = np.full((h, cw, 4), 55, np.uint8)
        quads[:, :, 0] = Y[:, 0::2]
        quads[:, :w // 2, 2] = Y[:, 1::2]
        quads[:, :, 1], quads[:, :, 3] = cb, cr
        t = torch.from_numpy(quads).cuda()
        p, (m, r, c) = t.data_ptr(), mode
        return PhdYuvView(p, p + 1, p + 3, h, w, 4 * cw, 2, 4 * cw, 4, 1, 0, m, r, c), t, (1, 0), (cb, cr)

    def boxes(self):
        """per image: boxes flush with the last row and column among them"""
        out = []
        for i, v in enumerate(self.views):
            h, w = v.height, v.width
            out.append([twelve(h, w), three(h, w), None, [box(h - 9, h, w - 11, w)]][i % 4])
        return out


_cache = {}


def _frames():
    if "frames" not in _cache:
        _cache["frames"] = Frames(SIZES)
    return _cache["frames"]


def _reference(key, frames, **kw):
    """reports_device_mixed over the numpy-converted RGB8 images, once per configuration"""
    if key not in _cache:
        phd, L, torch = _phd()
        _cache[key] = phd.reports_device_mixed(frames.rgb, **kw)
    return _cache[key]


@pytest.mark.parametrize("ds", [1, 2])
def test_reports_from_yuv_equal_reports_from_converted_rgb(ds):
    """One call: 352x400, 401x577 and 480x640, two of each, as pitched NV12,
    I420, YUY2, I444, NV21 and I422 with the matrix, range and chroma mode
    mixed across the images and per-image boxes; downsample_rate 1 and 2."""
    phd, L, torch = _phd()
    f = _frames()
    assert sorted({name for name, _ in f.layouts}) == ["_i420", "_i422", "_i444", "_nv12_pitched", "_nv21", "_yuy2"]
    assert len({m for _, m in f.layouts}) >= 4
    kw = dict(salient_characters=f.boxes(), downsample_rate=ds)
    want = _reference(("boxes", ds), f, **kw)
    got = phd.reports_device_yuv(f.views, **kw)
    assert len(got) == len(want) == 6
    for i, (g, w) in enumerate(zip(got, want)):
        _assert_same(g, w, (i, f.layouts[i]))


def test_convert_wrapper_equals_numpy():
    """convert_yuv_device on the report frames: the RGB8 tensors the yardstick is made of."""
    phd, L, torch = _phd()
    f = _frames()
    for i, (got, want) in enumerate(zip(phd.convert_yuv_device(f.views), f.rgb)):
        assert torch.equal(got, want), (i, f.layouts[i])


def test_bad_view_fails_alone():
    """c_pixel_stride = 0 in one view of three: the C call returns 1, that
    image has no report and a negative status, the others their reports; the
    Python wrapper raises RuntimeError naming the image."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import _finish, make_config
    from photohive_dsp_amd.structures import Full_Report_Data, PhdYuvView
    f = _frames()
    want = _reference(("plain", 1), f)
    views = (PhdYuvView * 3)(f.views[0], f.views[1], f.views[2])
    views[1].c_pixel_stride = 0
    cfg = make_config()
    outs = (ctypes.POINTER(Full_Report_Data) * 3)()
    st = (ctypes.c_int * 3)()
    rc = L.lib.phd_report_batch_device_yuv(views, 3, ctypes.byref(cfg), None, outs, st, None)
    assert rc == 1, L.last_error()
    assert st[0] == 0 and st[1] < 0 and st[2] == 0
    assert not outs[1]
    assert "image 1" in L.last_error() and "c_pixel_stride" in L.last_error()
    for i in (0, 2):
        _assert_same(_finish(outs[i], views[i].height, views[i].width, {}), want[i], i)
    with pytest.raises(RuntimeError, match="image 1"):
        phd.reports_device_yuv(list(views))


def test_lanes_one_and_two():
    """Four size groups under phd_set_lanes(1) and (2): the groups go to the
    lanes in turn, each lane with its own staging images."""
    phd, L, torch = _phd()
    if "four" not in _cache:
        _cache["four"] = Frames(SIZES + [(384, 512)], per_size=2, seed0=1230)
    f = _cache["four"]
    want = _reference(("four", 1), f, salient_characters=f.boxes())
    prev = L.lib.phd_set_lanes(1)
    try:
        one = phd.reports_device_yuv(f.views, salient_characters=f.boxes())
        L.lib.phd_set_lanes(2)
        two = phd.reports_device_yuv(f.views, salient_characters=f.boxes())
    finally:
        L.lib.phd_set_lanes(prev)
    for i, w in enumerate(want):
        _assert_same(one[i], w, ("one lane", i, f.layouts[i]))
        _assert_same(two[i], w, ("two lanes", i, f.layouts[i]))


def test_surface_still_being_produced_on_a_side_stream():
    """The call is made on a non-default torch stream while a producer on that
    stream is still writing the NV12 surface: the conversion is enqueued behind
    it, and the report is the finished surface's."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import nv12_planes, synth
    h, w = 600, 800
    Y, Cb, Cr = _ycc_planes(synth.structured(h, w, 5))
    cb, cr = Cb[::2, ::2], Cr[::2, ::2]
    surface = np.zeros((h + h // 2, w + 32), np.uint8)
    surface[:h, :w] = Y
    surface[h:, 0:w:2], surface[h:, 1:w:2] = cb, cr
    src = torch.from_numpy(surface).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = torch.randn(6144, 6144, device="cuda")
        for _ in range(4):
            a = a @ a                                   # keeps the stream busy for milliseconds
            a = a / a.abs().max()
        t = (src.to(torch.int16) + (a[0, 0] * 0).to(torch.int16)).to(torch.uint8)
        got = phd.reports_device_yuv([nv12_planes(t, h, w)], matrix="bt709", chroma="triangle")[0]
    side.synchronize()
    assert torch.equal(t, src)
    rgb = torch.from_numpy(convert(Y, cb, cr, 1, 1, 1, 0, 1)).cuda()
    _assert_same(got, phd.reports_device_mixed([rgb])[0])


def test_repeat_and_teardown():
    """The same mixed call twice (the staging images are reused across groups
    of different sizes), then once more after phd_shutdown()."""
    phd, L, torch = _phd()
    f = _frames()
    want = _reference(("plain", 1), f)
    for round_ in ("first", "second"):
        for i, g in enumerate(phd.reports_device_yuv(f.views)):
            _assert_same(g, want[i], (round_, i, f.layouts[i]))
    torch.cuda.synchronize()
    L.lib.phd_shutdown()
    for i, g in enumerate(phd.reports_device_yuv(f.views)):
        _assert_same(g, want[i], ("after shutdown", i, f.layouts[i]))
