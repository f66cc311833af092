"""Typed image views (CPU): the C-ABI surface, make_typed_views' stride
arithmetic on CPU tensors, the decode kernels' host twin
(phd_debug_decode_view_host: the kernels' own row code, decode_view.h) against
numpy bit for bit over every element type and layout, the snap tables, the
descriptor's validation, and the twin under ASan + UBSan on exactly sized
buffers (the span rule: no byte read outside a view's lowest to highest
addressed byte, none written outside the 3*H*W doubles and bytes)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.typed_cases import (ELEMS, F16, F32, F64, LAYOUTS, MAX_VALUES, OFFSETS, SHAPES, SNAP, U8, U16, decode,
                               same_doubles, snap_table, typed_case)


class _TypedViewABI(ctypes.Structure):
    """include/photohive_dsp.h: phd_typed_view, written out."""
    _fields_ = [("data", ctypes.c_void_p), ("height", ctypes.c_int), ("width", ctypes.c_int),
                ("row_stride", ctypes.c_int64), ("pixel_stride", ctypes.c_int64), ("channel_stride", ctypes.c_int64),
                ("elem", ctypes.c_int), ("flags", ctypes.c_int), ("max_value", ctypes.c_double)]


def test_surface_and_abi():
    from photohive_dsp_amd import lib as L
    from photohive_dsp_amd import structures as S
    for name in ("phd_report_batch_device_typed_views", "phd_decode_views_device", "phd_debug_decode_view_host"):
        assert getattr(L.lib, name).argtypes is not None, name
    T = S.PhdTypedView
    assert ctypes.sizeof(T) == ctypes.sizeof(_TypedViewABI) == 56
    assert [f for f, _ in T._fields_] == [f for f, _ in _TypedViewABI._fields_]
    assert [getattr(T, f).offset for f, _ in T._fields_] == [0, 8, 12, 16, 24, 32, 40, 44, 48]
    assert [getattr(T, f).offset for f, _ in T._fields_] == [getattr(_TypedViewABI, f).offset
                                                             for f, _ in _TypedViewABI._fields_]
    assert (S.PHD_ELEM_U8, S.PHD_ELEM_U16, S.PHD_ELEM_F16, S.PHD_ELEM_F32, S.PHD_ELEM_F64) == (0, 1, 2, 3, 4)
    assert S.PHD_VIEW_SNAP_U8 == 1
    assert (L.CLASSIFY_VIEWS_KERNEL, L.DECODE_VIEWS_KERNEL) == (7, 8)
    header = open(os.path.join(ROOT, "include", "photohive_dsp.h")).read()
    assert "PHD_ELEM_U8 = 0, PHD_ELEM_U16 = 1, PHD_ELEM_F16 = 2, PHD_ELEM_F32 = 3, PHD_ELEM_F64 = 4" in header
    assert "7 classify_views, 8 decode_views" in header


def _fields(v):
    return (v.data, v.height, v.width, v.row_stride, v.pixel_stride, v.channel_stride, v.elem, v.flags, v.max_value)


def test_make_typed_views_on_cpu_tensors():
    import torch
    from photohive_dsp_amd import make_typed_views
    from photohive_dsp_amd.structures import PhdTypedView
    H, W = 20, 30
    dtypes = [(torch.uint8, 0, 1), (torch.float16, 2, 2), (torch.float32, 3, 4), (torch.float64, 4, 8)]
    if hasattr(torch, "uint16"):
        dtypes.append((torch.uint16, 1, 2))
    for dt, elem, es in dtypes:
        t = torch.zeros((H, W, 3), dtype=dt)
        v, keep = make_typed_views([t])
        assert _fields(v[0]) == (t.data_ptr(), H, W, 3 * W * es, 3 * es, es, elem, 0, 0.0) and keep[0] is t
        c = torch.zeros((3, H, W), dtype=dt)
        v, _ = make_typed_views([c], "CHW")
        assert _fields(v[0]) == (c.data_ptr(), H, W, W * es, es, H * W * es, elem, 0, 0.0)
        a = torch.zeros((H, W, 4), dtype=dt)
        v, _ = make_typed_views([t, a], bgr=True, max_value=[None, 255], snap_u8=[True, False])
        assert _fields(v[0]) == (t.data_ptr() + 2 * es, H, W, 3 * W * es, 3 * es, -es, elem, 1, 0.0)
        assert _fields(v[1]) == (a.data_ptr() + 2 * es, H, W, 4 * W * es, 4 * es, -es, elem, 0, 255.0)
        v, _ = make_typed_views([c], "CHW", bgr=True, max_value=1023)
        assert _fields(v[0]) == (c.data_ptr() + 2 * H * W * es, H, W, W * es, es, -H * W * es, elem, 0, 1023.0)
        roi = c[:, 5:-3, 7:-2]
        v, _ = make_typed_views([roi], "CHW")
        assert _fields(v[0]) == (c.data_ptr() + (5 * W + 7) * es, H - 8, W - 9, W * es, es, H * W * es, elem, 0, 0.0)
        gray = torch.zeros((H, W), dtype=dt)
        v, _ = make_typed_views([gray[..., None].expand(H, W, 3)], snap_u8=True)
        assert _fields(v[0]) == (gray.data_ptr(), H, W, W * es, es, 0, elem, 1, 0.0)
        batch = torch.zeros((4, 3, H, W), dtype=dt)
        v, keep = make_typed_views(batch, "CHW")
        assert len(keep) == 4
        for i in range(4):
            assert _fields(v[i])[:6] == (batch.data_ptr() + i * 3 * H * W * es, H, W, W * es, es, H * W * es)
    if hasattr(torch, "uint16"):
        s16 = torch.zeros((H, W, 3), dtype=torch.int16)
        v, _ = make_typed_views([s16.view(torch.uint16)])
        assert _fields(v[0]) == (s16.data_ptr(), H, W, 6 * W, 6, 2, 1, 0, 0.0)
    # a ready-made view passes through
    ready = PhdTypedView(1024, 4, 5, 60, 12, 4, 3, 1, 0.0)
    v, _ = make_typed_views([ready, torch.zeros((H, W, 3), dtype=torch.float32)])
    assert _fields(v[0]) == _fields(ready) and v[1].elem == 3
    t8 = torch.zeros((H, W, 3), dtype=torch.uint8)
    for bad, layout, kw in (([torch.zeros((H, W, 3), dtype=torch.int16)], "HWC", {}),          # dtype
                            ([torch.zeros((H, W, 3), dtype=torch.bfloat16)], "HWC", {}),
                            ([torch.zeros((H, W, 3), dtype=torch.int32)], "HWC", {}),
                            ([np.zeros((H, W, 3), np.uint16)], "HWC", {}),                      # not a tensor
                            ([torch.zeros((H, W), dtype=torch.float32)], "HWC", {}),            # rank
                            (torch.zeros((H, W, 3), dtype=torch.float32), "HWC", {}),           # a lone 3-D tensor
                            ([torch.zeros((H, W, 2), dtype=torch.float32)], "HWC", {}),         # channel count
                            ([torch.zeros((5, H, W), dtype=torch.float16)], "CHW", {}),
                            ([t8], "NHWC", {}),
                            ([t8], "HWC", {"max_value": -1.0}),
                            ([t8], "HWC", {"max_value": float("nan")}),
                            ([t8, t8], "HWC", {"max_value": [1.0]})):
        with pytest.raises(ValueError):
            make_typed_views(bad, layout, **kw)
    with pytest.raises(ValueError, match="image 1"):
        make_typed_views([t8, torch.zeros((H, W, 3), dtype=torch.int16)])


def _host_decode(buf, data_off, strides, h, w, elem, flags, max_value, doff, want_rgb8=True):
    """phd_debug_decode_view_host into guarded planes at an offset of doff doubles."""
    from photohive_dsp_amd.lib import last_error, lib
    from photohive_dsp_amd.structures import PhdTypedView
    n = 3 * h * w
    planes = np.full(n + 8, -777.0, np.float64)
    lo = 2 + (planes.ctypes.data // 8) % 2 + doff           # doff 0: 16-byte aligned
    rgb8 = np.full(n + 32, 0xA5, np.uint8)
    is_u8 = ctypes.c_int(-1)
    view = PhdTypedView(buf.ctypes.data + data_off * buf.itemsize, h, w, *strides, elem, flags, max_value)
    rc = lib.phd_debug_decode_view_host(ctypes.byref(view), planes.ctypes.data + 8 * lo,
                                        rgb8.ctypes.data + 16 if want_rgb8 else None, ctypes.byref(is_u8))
    assert rc == 0, last_error()
    assert (planes[:lo] == -777.0).all() and (planes[lo + n:] == -777.0).all(), "guard doubles written"
    assert (rgb8[:16] == 0xA5).all() and (rgb8[16 + n:] == 0xA5).all(), "guard bytes written"
    return planes[lo:lo + n].reshape(3, h, w), rgb8[16:16 + n].reshape(h, w, 3), is_u8.value


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("elem", sorted(ELEMS), ids=[ELEMS[e][0] for e in sorted(ELEMS)])
def test_host_twin_equals_numpy(elem, layout):
    """Every element type and layout at every shape, base offset 0..3 elements,
    destination offset 0 / 1 doubles and max_value 0 / 1023 / 255: the planes,
    the RGB8 bytes and the 8-bit verdict, bit for bit."""
    for h, w in SHAPES:
        for off in OFFSETS:
            extra = off % 2 * 4 + off // 2
            buf, data_off, strides, raw = typed_case(elem, layout, h, w, off, extra)
            for mv in MAX_VALUES:
                for snap in (0, SNAP):
                    want_p, want_k, want_u8 = decode(elem, raw, mv, bool(snap))
                    for doff in (0, 1):
                        got_p, got_k, got_u8 = _host_decode(buf, data_off, strides, h, w, elem, snap, mv, doff)
                        what = (ELEMS[elem][0], layout, h, w, off, mv, snap, doff)
                        assert same_doubles(got_p, want_p), what
                        assert np.array_equal(got_k, want_k), what
                        assert got_u8 == int(want_u8), what


@pytest.mark.parametrize("elem", (U16, F16), ids=("u16", "f16"))
def test_host_twin_all_16_bit_patterns(elem):
    """All 65536 16-bit values in each channel (halves: subnormals, +-0,
    infinities and NaNs, compared by position), planar and interleaved."""
    every = np.arange(65536, dtype=np.uint16)
    for layout, h, w in (("chw", 128, 512), ("hwc", 256, 256), ("rgba", 128, 512)):
        bits = np.concatenate([np.roll(every, 7 * c) for c in range(3)])
        buf, data_off, strides, raw = typed_case(elem, layout, h, w, 0, 0, bits=bits)
        if layout == "chw":
            assert all(np.array_equal(np.sort(raw[..., c].ravel()), every) for c in range(3))
        for mv in MAX_VALUES:
            want_p, want_k, want_u8 = decode(elem, raw, mv, True)
            got_p, got_k, got_u8 = _host_decode(buf, data_off, strides, h, w, elem, SNAP, mv, 0)
            assert same_doubles(got_p, want_p) and np.array_equal(got_k, want_k) and got_u8 == int(want_u8)


def test_u16_multiples_of_257_and_k255_doubles_are_8_bit():
    j = np.arange(256)
    assert np.array_equal((j * 257) / 65535.0, j / 255.0)
    img = np.random.default_rng(5).integers(0, 256, (9, 11, 3))
    for elem, arr in ((U16, (img * 257).astype(np.uint16)), (F64, (img / 255.0).view(np.uint64)),
                      (U8, img.astype(np.uint8))):
        buf = np.ascontiguousarray(arr).ravel()
        es = buf.itemsize
        _, k, u8 = _host_decode(buf, 0, (33 * es, 3 * es, es), 9, 11, elem, 0, 0.0, 0)
        assert u8 == 1 and np.array_equal(k, img)
    # only the verdict (no RGB8 buffer)
    buf = (img * 257).astype(np.uint16).ravel()
    assert _host_decode(buf, 0, (66, 6, 2), 9, 11, U16, 0, 0.0, 0, want_rgb8=False)[2] == 1
    buf[5] += 1
    assert _host_decode(buf, 0, (66, 6, 2), 9, 11, U16, 0, 0.0, 0, want_rgb8=False)[2] == 0


@pytest.mark.parametrize("elem", (F16, F32), ids=("f16", "f32"))
def test_snap(elem):
    """The tables: 256 distinct entries equal to what uint8 / 255 in that type
    holds; an image of table entries is 8-bit with the flag and its bytes are
    j; one element one ulp off is not; without the flag the float32 image takes
    the fp64 path (2 of its 256 entries widen to j / 255.0)."""
    import torch
    tab = snap_table(elem)
    store = ELEMS[elem][1]
    assert len(np.unique(tab)) == 256
    t8 = torch.arange(256, dtype=torch.uint8)
    tt = t8.float().div(255)
    assert np.array_equal((tt.half() if elem == F16 else tt).numpy(), tab)
    if elem == F32:
        assert int((tab.astype(np.float64) == np.arange(256) / 255.0).sum()) == 2
    j = np.random.default_rng(3).integers(0, 256, (16, 16, 3))
    j.reshape(-1)[:256] = np.arange(256)
    buf = tab[j].view(store).ravel().copy()
    es = buf.itemsize
    strides = (48 * es, 3 * es, es)
    planes, k, u8 = _host_decode(buf, 0, strides, 16, 16, elem, SNAP, 0.0, 0)
    assert u8 == 1 and np.array_equal(k, j)
    assert same_doubles(planes, tab[j].astype(np.float64).transpose(2, 0, 1))
    assert _host_decode(buf, 0, strides, 16, 16, elem, 0, 0.0, 0)[2] == 0
    # an explicit maximum of 1.0 is the default maximum
    assert _host_decode(buf, 0, strides, 16, 16, elem, SNAP, 1.0, 0)[2] == 1
    assert _host_decode(buf, 0, strides, 16, 16, elem, SNAP, 255.0, 0)[2] == 0
    for at in (0, 300, 767):
        for step in (1, -1):
            off = buf.copy()
            off[at] = (int(off[at]) + step) % (1 << (8 * es))     # the neighbouring bit pattern
            assert _host_decode(off, 0, strides, 16, 16, elem, SNAP, 0.0, 0)[2] == 0, (at, step)


def test_snap_flag_is_ignored_for_other_types():
    rng = np.random.default_rng(11)
    for elem in (U8, U16, F64):
        buf, data_off, strides, raw = typed_case(elem, "hwc", 5, 7, 0)
        a = _host_decode(buf, data_off, strides, 5, 7, elem, 0, 0.0, 0)
        b = _host_decode(buf, data_off, strides, 5, 7, elem, SNAP, 0.0, 0)
        assert same_doubles(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # float64 holding the float32 table: not 8-bit, flag or no flag
    buf = snap_table(F32)[rng.integers(1, 255, 105)].astype(np.float64).view(np.uint64)
    assert _host_decode(buf, 0, (168, 24, 8), 5, 7, F64, SNAP, 0.0, 0)[2] == 0


def test_validation_names_the_field():
    """The host-side checks of the descriptor, before any launch (so without a
    GPU): the twin returns -1 with the field in phd_last_error, and
    phd_decode_views_device fails the whole call naming the image."""
    from photohive_dsp_amd.lib import last_error, lib
    from photohive_dsp_amd.structures import PhdTypedView as V
    buf = np.zeros(4096, np.float64)
    planes = np.zeros(4096, np.float64)
    p = buf.ctypes.data
    good = V(p, 4, 5, 60, 12, 4, F32, 0, 0.0)
    for bad, word in ((V(None, 4, 5, 60, 12, 4, F32, 0, 0.0), "data"),
                      (V(p, 4, 5, 60, 12, 4, 5, 0, 0.0), "elem"),
                      (V(p, 4, 5, 60, 12, 4, -1, 0, 0.0), "elem"),
                      (V(p, 4, 5, 60, 12, 4, F32, 2, 0.0), "flags"),
                      (V(p, 4, 5, 60, 12, 4, F32, 1 | 4, 0.0), "flags"),
                      (V(p, 4, 5, 62, 12, 4, F32, 0, 0.0), "row_stride"),
                      (V(p, 4, 5, 60, 6, 4, F32, 0, 0.0), "pixel_stride"),
                      (V(p, 4, 5, 60, 12, 2, F32, 0, 0.0), "channel_stride"),
                      (V(p, 4, 5, 30, 6, 1, U16, 0, 0.0), "channel_stride"),
                      (V(p, 4, 5, 120, 24, 4, F64, 0, 0.0), "channel_stride"),
                      (V(p + 2, 4, 5, 60, 12, 4, F32, 0, 0.0), "data"),
                      (V(p + 1, 4, 5, 30, 6, 2, F16, 0, 0.0), "data"),
                      (V(p + 4, 4, 5, 120, 24, 8, F64, 0, 0.0), "data"),
                      (V(p, 4, 5, 60, 12, 4, F32, 0, -1.0), "max_value"),
                      (V(p, 4, 5, 60, 12, 4, F32, 0, float("nan")), "max_value"),
                      (V(p, 4, 5, 60, 12, 4, F32, 0, float("inf")), "max_value"),
                      (V(p, 0, 5, 60, 12, 4, F32, 0, 0.0), "height"),
                      (V(p, 4, -1, 60, 12, 4, F32, 0, 0.0), "width"),
                      (V(p, 4, 5, 60, 0, 4, F32, 0, 0.0), "pixel_stride"),
                      (V(p, 4, 5, 0, 12, 4, F32, 0, 0.0), "row_stride")):
        assert lib.phd_debug_decode_view_host(ctypes.byref(bad), planes.ctypes.data, None, None) == -1, word
        assert word in last_error(), (word, last_error())
        views = (V * 2)(good, bad)
        dsts = (ctypes.c_void_p * 2)(planes.ctypes.data, planes.ctypes.data + 1024)
        assert lib.phd_decode_views_device(views, 2, dsts, None) == -1
        assert "image 1" in last_error() and word in last_error(), (word, last_error())
    # the strides that may be 0: a single column, a single row, any channel stride
    for ok in (V(p, 4, 1, 60, 0, 4, F32, 0, 0.0), V(p, 1, 5, 0, 12, 4, F32, 0, 0.0), V(p, 4, 5, 60, 12, 0, F32, 1, 0.0),
               V(p + 1, 4, 5, 15, 3, 1, U8, 0, 100.0), V(p, 4, 5, -60, -12, -4, F32, 0, 1e-300)):
        base = V(ok.data + (2048 if ok.row_stride < 0 else 0), *_fields(ok)[1:])
        assert lib.phd_debug_decode_view_host(ctypes.byref(base), planes.ctypes.data, None, None) == 0, last_error()
        assert last_error() == ""


def test_host_twin_under_asan_ubsan(tmp_path):
    """phd_views.cpp (with decode_view.h, the kernels' row code) and a C++
    driver built with ASan + UBSan, run as their own process: every element
    type, layout and shape of test_host_twin_equals_numpy, each view in a
    malloc of exactly its span and the planes in a malloc of exactly 3*H*W
    doubles (the RGB8 bytes in exactly 3*H*W bytes)."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "decode_view_asan"
    src = [os.path.join(ROOT, "tests", "native", "decode_view_asan.cpp"),
           os.path.join(ROOT, "photohive_dsp_amd", "csrc", "phd_views.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + src,
                   check=True, timeout=300)
    env = {k: v for k, v in os.environ.items() if k in ("PATH", "HOME", "LANG", "TMPDIR")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "decode view host OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
