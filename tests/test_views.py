"""Image views (CPU): the C-ABI surface of the view entry points, make_views'
stride arithmetic on CPU tensors, the pack kernel's host twin
(phd_debug_pack_view_host: the kernel's own row code, pack_view.h) against
numpy over every layout of the descriptor's table, the descriptor's
validation, and the twin under ASan + UBSan on exactly-sized buffers (the
check of the span rule: no byte read outside a view's lowest to highest
addressed byte, none written outside the 3*H*W destination bytes)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.view_cases import LAYOUTS, OFFSETS, PITCH_EXTRA, SHAPES, view_case


def test_surface():
    from photohive_dsp_amd.lib import lib
    from photohive_dsp_amd.structures import PhdImageView
    for name in ("phd_report_batch_device_views", "phd_pack_views_device", "phd_debug_pack_view_host"):
        assert getattr(lib, name).argtypes is not None, name
    assert ctypes.sizeof(PhdImageView) == 40
    offs = [getattr(PhdImageView, f).offset for f, _ in PhdImageView._fields_]
    assert offs == [0, 8, 12, 16, 24, 32]
    assert [f for f, _ in PhdImageView._fields_] == ["data", "height", "width", "row_stride", "pixel_stride",
                                                      "channel_stride"]


def _fields(v):
    return (v.data, v.height, v.width, v.row_stride, v.pixel_stride, v.channel_stride)


def test_make_views_on_cpu_tensors():
    import torch
    from photohive_dsp_amd import make_views
    H, W = 20, 30
    t = torch.zeros((H, W, 3), dtype=torch.uint8)
    v, keep = make_views([t])
    assert _fields(v[0]) == (t.data_ptr(), H, W, 3 * W, 3, 1) and keep[0] is t
    c = torch.zeros((3, H, W), dtype=torch.uint8)
    v, _ = make_views([c], "CHW")
    assert _fields(v[0]) == (c.data_ptr(), H, W, W, 1, H * W)
    a = torch.zeros((H, W, 4), dtype=torch.uint8)
    v, _ = make_views([a])
    assert _fields(v[0]) == (a.data_ptr(), H, W, 4 * W, 4, 1)
    v, _ = make_views([t, a], bgr=True)
    assert _fields(v[0]) == (t.data_ptr() + 2, H, W, 3 * W, 3, -1)
    assert _fields(v[1]) == (a.data_ptr() + 2, H, W, 4 * W, 4, -1)
    v, _ = make_views([c], "CHW", bgr=True)
    assert _fields(v[0]) == (c.data_ptr() + 2 * H * W, H, W, W, 1, -H * W)
    roi = t[5:-3, 7:-2]
    v, _ = make_views([roi])
    assert _fields(v[0]) == (t.data_ptr() + 5 * 3 * W + 7 * 3, H - 8, W - 9, 3 * W, 3, 1)
    flat = torch.zeros(H * W * 3 + 1, dtype=torch.uint8)
    odd = flat[1:].view(H, W, 3)                                   # one byte off
    v, _ = make_views([odd])
    assert _fields(v[0]) == (flat.data_ptr() + 1, H, W, 3 * W, 3, 1)
    gray = torch.zeros((H, W), dtype=torch.uint8)
    v, _ = make_views([gray[..., None].expand(H, W, 3)])
    assert _fields(v[0]) == (gray.data_ptr(), H, W, W, 1, 0)
    batch = torch.zeros((4, 3, H, W), dtype=torch.uint8)
    v, keep = make_views(batch, "CHW")
    assert len(keep) == 4
    for i in range(4):
        assert _fields(v[i]) == (batch.data_ptr() + i * 3 * H * W, H, W, W, 1, H * W)
    # a ready-made view passes through
    v2, _ = make_views([v[1], t])
    assert _fields(v2[0]) == _fields(v[1]) and _fields(v2[1]) == (t.data_ptr(), H, W, 3 * W, 3, 1)
    for bad, layout in (([torch.zeros((H, W, 3), dtype=torch.float32)], "HWC"),      # dtype
                        ([np.zeros((H, W, 3), np.uint8)], "HWC"),                    # not a tensor
                        ([torch.zeros((H, W), dtype=torch.uint8)], "HWC"),           # rank
                        (torch.zeros((H, W, 3), dtype=torch.uint8), "HWC"),          # a lone 3-D tensor
                        ([torch.zeros((H, W, 2), dtype=torch.uint8)], "HWC"),        # channel count
                        ([torch.zeros((5, H, W), dtype=torch.uint8)], "CHW"),
                        ([torch.zeros((H, W, 3), dtype=torch.uint8)], "CHW"),        # H read as channels
                        ([t], "NHWC")):
        with pytest.raises(ValueError):
            make_views(bad, layout)


def _host_pack(buf, data_off, strides, h, w, doff):
    """phd_debug_pack_view_host into a guarded destination at byte offset doff."""
    from photohive_dsp_amd.lib import lib
    from photohive_dsp_amd.structures import PhdImageView
    dst = np.full(3 * h * w + 40, 0xA5, np.uint8)
    lo = 16 + (-dst.ctypes.data) % 16 + doff
    view = PhdImageView(buf.ctypes.data + data_off, h, w, *strides)
    assert lib.phd_debug_pack_view_host(ctypes.byref(view), dst.ctypes.data + lo) == 0
    assert (dst[:lo] == 0xA5).all() and (dst[lo + 3 * h * w:] == 0xA5).all(), "guard bytes written"
    return dst[lo:lo + 3 * h * w].reshape(h, w, 3)


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_host_twin_equals_numpy(name):
    """Every layout at every shape, base offset 0..3, pitch minimum + {0, 1, 4}
    and destination offset 0..3: bytes-equal."""
    for h, w in SHAPES:
        for off in OFFSETS:
            for extra in PITCH_EXTRA:
                buf, data_off, strides, want = view_case(name, h, w, off, extra)
                for doff in OFFSETS:
                    got = _host_pack(buf, data_off, strides, h, w, doff)
                    assert np.array_equal(got, want), (name, h, w, off, extra, doff)


def test_validation_names_the_field():
    """The host-side checks of the descriptor, before any launch (so without a
    GPU): phd_pack_views_device fails the whole call with the image and the
    field in phd_last_error; the host twin returns -1."""
    from photohive_dsp_amd.lib import last_error, lib
    from photohive_dsp_amd.structures import PhdImageView
    buf = np.zeros(4096, np.uint8)
    dst = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    good = PhdImageView(p, 4, 5, 15, 3, 1)
    for bad, word in ((PhdImageView(None, 4, 5, 15, 3, 1), "data"),
                      (PhdImageView(p, 0, 5, 15, 3, 1), "height"),
                      (PhdImageView(p, 4, -1, 15, 3, 1), "width"),
                      (PhdImageView(p, 4, 5, 15, 0, 1), "pixel_stride"),
                      (PhdImageView(p, 4, 5, 0, 3, 1), "row_stride")):
        views = (PhdImageView * 2)(good, bad)
        dsts = (ctypes.c_void_p * 2)(dst.ctypes.data, dst.ctypes.data + 1024)
        assert lib.phd_pack_views_device(views, 2, dsts, None) == -1
        assert "image 1" in last_error() and word in last_error(), (word, last_error())
        assert lib.phd_debug_pack_view_host(ctypes.byref(bad), dst.ctypes.data) == -1
    # the strides that may be 0: a single column, a single row, any channel stride
    for ok in (PhdImageView(p, 4, 1, 15, 0, 1), PhdImageView(p, 1, 5, 0, 3, 1), PhdImageView(p, 4, 5, 15, 3, 0)):
        assert lib.phd_debug_pack_view_host(ctypes.byref(ok), dst.ctypes.data) == 0


def test_host_twin_under_asan_ubsan(tmp_path):
    """phd_views.cpp (with pack_view.h, the kernel's row code) and a C++ driver
    built with ASan + UBSan, run as their own process: every layout and shape
    of test_host_twin_equals_numpy, each view in a malloc of exactly its span
    (the last row flush with the end of the buffer) and each destination in a
    malloc of exactly 3*H*W bytes."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "pack_view_asan"
    src = [os.path.join(ROOT, "tests", "native", "pack_view_asan.cpp"),
           os.path.join(ROOT, "photohive_dsp_amd", "csrc", "phd_views.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + src,
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "pack view host OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
