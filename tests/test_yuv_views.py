"""YCbCr views (CPU): the C-ABI surface of the YUV entry points, the
conversion kernel's host twin (phd_debug_yuv_view_host: the kernel's own row
code, yuv_view.h) against the numpy restatement of the definition
(tests/yuv_cases.py) over every layout of the descriptor's table and over all
256^3 (Y, Cb, Cr) triples, the JFIF row against libjpeg, the descriptor's
validation, make_yuv_views' and nv12_planes' stride arithmetic on CPU tensors,
and the twin under ASan + UBSan on exactly-sized buffers (the span rule)."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.yuv_cases import (LAYOUTS, MODES, OFFSETS, PITCH_EXTRA, SHAPES, TABLE, convert, cube_planes, make_view,
                             matrix_rgb, real_rgb, yuv_case)


def test_surface():
    from photohive_dsp_amd import lib as L
    from photohive_dsp_amd.structures import PhdYuvView
    for name in ("phd_report_batch_device_yuv", "phd_convert_yuv_device", "phd_debug_yuv_view_host"):
        assert getattr(L.lib, name).argtypes is not None, name
    assert L.YUV_VIEWS_KERNEL == 9
    assert ctypes.sizeof(PhdYuvView) == 88
    assert [f for f, _ in PhdYuvView._fields_] == ["y", "cb", "cr", "height", "width", "y_row_stride",
                                                   "y_pixel_stride", "c_row_stride", "c_pixel_stride",
                                                   "chroma_shift_x", "chroma_shift_y", "matrix", "range", "chroma"]
    assert [getattr(PhdYuvView, f).offset for f, _ in PhdYuvView._fields_] == [0, 8, 16, 24, 28, 32, 40, 48, 56,
                                                                               64, 68, 72, 76, 80]


def _host_convert(view, h, w, doff):
    """phd_debug_yuv_view_host into a guarded destination at byte offset doff."""
    from photohive_dsp_amd.lib import last_error, lib
    dst = np.full(3 * h * w + 40, 0xA5, np.uint8)
    lo = 16 + (-dst.ctypes.data) % 16 + doff
    assert lib.phd_debug_yuv_view_host(ctypes.byref(view), dst.ctypes.data + lo) == 0, last_error()
    assert (dst[:lo] == 0xA5).all() and (dst[lo + 3 * h * w:] == 0xA5).all(), "guard bytes written"
    return dst[lo:lo + 3 * h * w].reshape(h, w, 3)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_host_twin_equals_numpy(name):
    """Every layout at every shape, base offset 0..3, pitch minimum + {0, 1, 4},
    both chroma modes over all four matrix rows and destination offset 0..3:
    bytes-equal, guards intact."""
    for h, w in SHAPES:
        for off in OFFSETS:
            for extra in PITCH_EXTRA:
                buf, lay, (Y, Cb, Cr) = yuv_case(name, h, w, off, extra)
                for mode in MODES:
                    want = convert(Y, Cb, Cr, lay["sx"], lay["sy"], *mode)
                    view = make_view(buf.ctypes.data, lay, h, w, mode)
                    for doff in OFFSETS:
                        got = _host_convert(view, h, w, doff)
                        assert np.array_equal(got, want), (name, h, w, off, extra, mode, doff)


@pytest.fixture(scope="module")
def cube():
    return cube_planes()


@pytest.mark.parametrize("matrix,rng", sorted(TABLE))
def test_all_triples(cube, matrix, rng):
    """All 256^3 (Y, Cb, Cr) triples as one 4096 x 4096 4:4:4 view per table
    row: the twin equals numpy, and stays within 0.504 of the clamped
    real-valued matrix (0.5 + 511 * 0.5 / 65536)."""
    from photohive_dsp_amd.lib import last_error, lib
    from photohive_dsp_amd.structures import PhdYuvView
    Y, Cb, Cr = cube
    n = 4096
    view = PhdYuvView(Y.ctypes.data, Cb.ctypes.data, Cr.ctypes.data, n, n, n, 1, n, 1, 0, 0, matrix, rng, 0)
    got = np.empty((n, n, 3), np.uint8)
    assert lib.phd_debug_yuv_view_host(ctypes.byref(view), got.ctypes.data) == 0, last_error()
    worst = 0.0
    for r0 in range(0, n, 512):                      # in slabs: the float64 image is 400 MB whole
        s = slice(r0, r0 + 512)
        assert np.array_equal(got[s], matrix_rgb(Y[s], Cb[s], Cr[s], matrix, rng)), (matrix, rng, r0)
        worst = max(worst, float(np.abs(got[s].astype(np.float64) - real_rgb(Y[s], Cb[s], Cr[s], matrix, rng)).max()))
    print(f"matrix {matrix} range {rng}: max |integer - real| = {worst:.4f}")
    assert worst <= 0.504, worst


def test_jfif_row_equals_libjpeg():
    """A 4:4:4 JPEG decoded by libjpeg to RGB, and to YCbCr (draft mode) with
    the twin's BT601 FULL row applied: the same bytes."""
    Image = pytest.importorskip("PIL.Image")
    from photohive_dsp_amd import synth
    from photohive_dsp_amd.lib import last_error, lib
    from photohive_dsp_amd.structures import PhdYuvView
    h, w = 61, 83
    src = synth.make("structured", 352, 400, 5)[:h, :w]
    f = io.BytesIO()
    Image.fromarray(src).save(f, "JPEG", quality=92, subsampling=0)
    rgb = np.asarray(Image.open(io.BytesIO(f.getvalue())).convert("RGB"))
    im = Image.open(io.BytesIO(f.getvalue()))
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr"
    ycc = np.ascontiguousarray(np.asarray(im))
    assert ycc.shape == (h, w, 3)
    p = ycc.ctypes.data
    view = PhdYuvView(p, p + 1, p + 2, h, w, 3 * w, 3, 3 * w, 3, 0, 0, 0, 0, 0)
    got = np.empty((h, w, 3), np.uint8)
    assert lib.phd_debug_yuv_view_host(ctypes.byref(view), got.ctypes.data) == 0, last_error()
    assert np.array_equal(got, rgb)


def test_validation_names_the_field():
    """The host-side checks of the descriptor, before any launch (so without a
    GPU): phd_convert_yuv_device fails the whole call with the image and the
    field in phd_last_error; the host twin returns -1 with the field."""
    from photohive_dsp_amd.lib import last_error, lib
    from photohive_dsp_amd.structures import PhdYuvView
    buf = np.zeros(4096, np.uint8)
    dst = np.zeros(4096, np.uint8)
    p = buf.ctypes.data

    def view(**kw):
        f = dict(y=p, cb=p + 1024, cr=p + 2048, height=4, width=6, y_row_stride=6, y_pixel_stride=1,
                 c_row_stride=3, c_pixel_stride=1, chroma_shift_x=1, chroma_shift_y=1, matrix=0, range=0, chroma=0)
        f.update(kw)
        return PhdYuvView(**f)

    good = view()
    assert lib.phd_debug_yuv_view_host(ctypes.byref(good), dst.ctypes.data) == 0, last_error()
    for kw, word in ((dict(y=None), "y is NULL"), (dict(cb=None), "cb is NULL"), (dict(cr=None), "cr is NULL"),
                     (dict(height=0), "height"), (dict(width=-1), "width"),
                     (dict(chroma_shift_x=0), "chroma_shift"), (dict(chroma_shift_x=2), "chroma_shift"),
                     (dict(chroma_shift_y=-1), "chroma_shift"),
                     (dict(matrix=2), "matrix"), (dict(range=-1), "range"), (dict(chroma=2), "chroma"),
                     (dict(y_pixel_stride=0), "y_pixel_stride"), (dict(y_row_stride=0), "y_row_stride"),
                     (dict(c_pixel_stride=0), "c_pixel_stride"), (dict(c_row_stride=0), "c_row_stride")):
        bad = view(**kw)
        views = (PhdYuvView * 2)(good, bad)
        dsts = (ctypes.c_void_p * 2)(dst.ctypes.data, dst.ctypes.data + 1024)
        assert lib.phd_convert_yuv_device(views, 2, dsts, None) == -1, kw
        assert "image 1" in last_error() and word in last_error(), (kw, last_error())
        assert lib.phd_debug_yuv_view_host(ctypes.byref(bad), dst.ctypes.data) == -1, kw
        assert word in last_error(), (kw, last_error())
    # the strides that may be 0: a single column, a single row, a single chroma sample or row
    for kw in (dict(width=1, y_pixel_stride=0, c_pixel_stride=0), dict(height=1, y_row_stride=0, c_row_stride=0),
               dict(width=2, c_pixel_stride=0), dict(height=2, c_row_stride=0)):
        assert lib.phd_debug_yuv_view_host(ctypes.byref(view(**kw)), dst.ctypes.data) == 0, (kw, last_error())
    # a NULL destination fails the call too
    views = (PhdYuvView * 1)(good)
    assert lib.phd_convert_yuv_device(views, 1, (ctypes.c_void_p * 1)(None), None) == -1
    assert "image 0" in last_error() and "destination" in last_error()


def _fields(v):
    return tuple(getattr(v, f) for f, _ in type(v)._fields_)


def test_make_yuv_views_and_nv12_planes_on_cpu_tensors():
    import torch
    from photohive_dsp_amd import make_yuv_views, nv12_planes
    from photohive_dsp_amd.structures import PhdYuvView
    H, W = 20, 30
    y = torch.zeros((H, W), dtype=torch.uint8)
    c420 = [torch.zeros((H // 2, W // 2), dtype=torch.uint8) for _ in range(2)]
    v, keep = make_yuv_views([(y, *c420)])
    assert _fields(v[0]) == (y.data_ptr(), c420[0].data_ptr(), c420[1].data_ptr(), H, W, W, 1, W // 2, 1,
                             1, 1, 0, 0, 0)
    assert keep[0][0] is y
    # YV12, and the mode arguments
    v, _ = make_yuv_views([(y, *c420)], matrix="bt709", full_range=False, chroma="triangle", swap_uv=True)
    assert _fields(v[0]) == (y.data_ptr(), c420[1].data_ptr(), c420[0].data_ptr(), H, W, W, 1, W // 2, 1,
                             1, 1, 1, 1, 1)
    c422 = [torch.zeros((H, W // 2), dtype=torch.uint8) for _ in range(2)]
    v, _ = make_yuv_views([(y, *c422)])
    assert _fields(v[0])[9:11] == (1, 0)
    c444 = [torch.zeros((H, W), dtype=torch.uint8) for _ in range(2)]
    v, _ = make_yuv_views([(y, *c444)])
    assert _fields(v[0])[9:11] == (0, 0)
    # odd sizes round the chroma planes up
    yo = torch.zeros((21, 31), dtype=torch.uint8)
    co = [torch.zeros((11, 16), dtype=torch.uint8) for _ in range(2)]
    v, _ = make_yuv_views([(yo, *co)])
    assert _fields(v[0])[3:5] == (21, 31) and _fields(v[0])[9:11] == (1, 1)
    # a pitched NV12 surface, split without a copy; NV21 by swap_uv
    pitch = 48
    surface = torch.zeros((H + H // 2 + 3, pitch), dtype=torch.uint8)
    ys, uv = nv12_planes(surface, H, W)
    assert ys.data_ptr() == surface.data_ptr() and ys.shape == (H, W) and ys.stride() == (pitch, 1)
    assert uv.data_ptr() == surface.data_ptr() + H * pitch and uv.shape == (H // 2, W // 2, 2)
    assert uv.stride() == (pitch, 2, 1)
    v, _ = make_yuv_views([(ys, uv)])
    base = surface.data_ptr()
    assert _fields(v[0]) == (base, base + H * pitch, base + H * pitch + 1, H, W, pitch, 1, pitch, 2, 1, 1, 0, 0, 0)
    v, _ = make_yuv_views([(ys, uv)], swap_uv=True)
    assert _fields(v[0])[:3] == (base, base + H * pitch + 1, base + H * pitch)
    # an even-origin region of the surface
    v, _ = make_yuv_views([(ys[4:12, 6:20], uv[2:6, 3:10])])
    assert _fields(v[0]) == (base + 4 * pitch + 6, base + (H + 2) * pitch + 6, base + (H + 2) * pitch + 7, 8, 14,
                             pitch, 1, pitch, 2, 1, 1, 0, 0, 0)
    # odd sizes: (height + 1) // 2 chroma rows of (width + 1) // 2 pairs
    so = torch.zeros((21 + 11, 32), dtype=torch.uint8)
    yo2, uvo = nv12_planes(so, 21, 31)
    assert yo2.shape == (21, 31) and uvo.shape == (11, 16, 2)
    # a ready-made view passes through
    ready = PhdYuvView(1, 2, 4, 5, 6, 12, 2, 12, 4, 1, 0, 0, 0, 0)
    v2, _ = make_yuv_views([ready, (y, *c420)])
    assert _fields(v2[0]) == _fields(ready) and _fields(v2[1])[0] == y.data_ptr()
    for bad, kw in (([(y, c420[0])], {}),                                              # uv not [ch, cw, 2]
                    ([(y, torch.zeros((H // 2, W // 2, 3), dtype=torch.uint8))], {}),
                    ([(y, torch.zeros((H // 2, W // 2 + 1), dtype=torch.uint8),
                       torch.zeros((H // 2, W // 2 + 1), dtype=torch.uint8))], {}),    # no subsampling fits
                    ([(y, c420[0], c422[0])], {}),                                     # cb and cr differ
                    ([(y.float(), *c420)], {}),                                        # dtype
                    ([(y[None], *c420)], {}),                                          # rank
                    ([(y, *c420, c420[0])], {}),                                       # four planes
                    ([y], {}),                                                         # not a frame
                    ([(y, *c420)], dict(matrix="bt2020")),
                    ([(y, *c420)], dict(chroma="bicubic"))):
        with pytest.raises(ValueError):
            make_yuv_views(bad, **kw)
    with pytest.raises(ValueError, match="image 1"):
        make_yuv_views([(y, *c420), (y, c420[0], c422[0])])
    for bad_surface, hh, ww in ((torch.zeros((H + H // 2 - 1, pitch), dtype=torch.uint8), H, W),   # too few rows
                                (torch.zeros((H + H // 2, W - 2), dtype=torch.uint8), H, W),       # too narrow
                                (torch.zeros((H, W, 2), dtype=torch.uint8), H, W)):
        with pytest.raises(ValueError):
            nv12_planes(bad_surface, hh, ww)


def test_host_twin_under_asan_ubsan(tmp_path):
    """phd_yuv.cpp (with yuv_view.h, the kernel's row code) and a C++ driver
    built with ASan + UBSan, run as their own process: every case of
    test_host_twin_equals_numpy, each plane in a malloc of exactly its span,
    planes whose spans interleave (NV12, YUY2) in one malloc of their joint
    span, each destination in a malloc of exactly 3*H*W bytes."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "yuv_view_asan"
    src = [os.path.join(ROOT, "tests", "native", "yuv_view_asan.cpp"),
           os.path.join(ROOT, "photohive_dsp_amd", "csrc", "phd_yuv.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + src,
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "yuv view host OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
