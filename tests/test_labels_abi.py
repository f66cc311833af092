"""The label map entries' surface without a device: the symbols, the argument
checks that come before any HIP call, and the Python wrappers' input checks."""
import ctypes

import numpy as np
import pytest


def _lib():
    from photohive_dsp_amd import lib as L
    return L


def test_symbols_and_constants():
    L = _lib()
    assert hasattr(L.lib, "phd_report_batch_device_mixed_labels")
    assert hasattr(L.lib, "phd_labels_to_rgb_device")
    assert L.LABEL_NONE == 0xFFFF and np.array([L.LABEL_NONE], np.uint16).view(np.int16)[0] == -1
    assert L.PALETTE_LABELS_KERNEL == 10
    import photohive_dsp_amd as phd
    assert callable(phd.reports_device_labels) and callable(phd.quantize_device)


def test_header_declares_the_entries():
    import os
    from tests.conftest import ROOT
    with open(os.path.join(ROOT, "include", "photohive_dsp.h")) as f:
        h = f.read()
    for s in ("enum { PHD_LABEL_NONE = 0xFFFF };", "int phd_report_batch_device_mixed_labels(",
              "int phd_labels_to_rgb_device(", "10 palette_labels"):
        assert s in h, s


def test_labels_entry_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = _lib()
    from photohive_dsp_amd.core import make_config
    cfg = make_config()
    n = 1
    ptrs = (ctypes.c_void_p * n)(4096)
    hs, ws = (ctypes.c_int * n)(400), (ctypes.c_int * n)(400)
    maps = (ctypes.c_void_p * n)(8192)
    from photohive_dsp_amd.structures import Full_Report_Data
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    assert L.lib.phd_report_batch_device_mixed_labels(ptrs, hs, ws, n, ctypes.byref(cfg), None, maps, outs, st,
                                                      None) == -1
    assert "no HIP device" in L.last_error()
    # bad arguments come first
    assert L.lib.phd_report_batch_device_mixed_labels(None, hs, ws, n, ctypes.byref(cfg), None, maps, outs, st,
                                                      None) == -1
    assert "phd_report_batch_device_mixed_labels: bad arguments" in L.last_error()


def _to_rgb(L, maps, hs, ws, n, luts, ns, none, dst):
    return L.lib.phd_labels_to_rgb_device(maps, hs, ws, n, luts, ns, none, dst, None)


def test_labels_to_rgb_rejects_before_touching_hip():
    """NULL arguments and non-positive sizes: a message naming the call, with
    or without a device (the pointers below are never dereferenced)."""
    L = _lib()
    n = 2
    maps = (ctypes.c_void_p * n)(4096, 8192)
    dst = (ctypes.c_void_p * n)(12288, 16384)
    hs, ws = (ctypes.c_int * n)(4, 5), (ctypes.c_int * n)(6, 7)
    lut = np.zeros((3, 3), np.uint8)
    luts = (ctypes.c_void_p * n)(lut.ctypes.data, lut.ctypes.data)
    ns = (ctypes.c_int * n)(3, 3)
    none = (ctypes.c_uint8 * 3)(1, 2, 3)
    args = [maps, hs, ws, n, luts, ns, none, dst]
    for k in (0, 1, 2, 4, 5, 6, 7):
        bad = list(args)
        bad[k] = None
        assert _to_rgb(L, *bad) == -1
        assert "phd_labels_to_rgb_device: NULL argument" in L.last_error(), k
    for bad_n in (0, -1, 65536):
        assert _to_rgb(L, maps, hs, ws, bad_n, luts, ns, none, dst) == -1
        assert "n_maps" in L.last_error()
    for field, arr in (("height", (ctypes.c_int * n)(4, 0)), ("width", (ctypes.c_int * n)(4, -3))):
        a = list(args)
        a[1 if field == "height" else 2] = arr
        assert _to_rgb(L, *a) == -1
        assert "map 1" in L.last_error() and "positive" in L.last_error()
    assert _to_rgb(L, (ctypes.c_void_p * n)(4096, None), hs, ws, n, luts, ns, none, dst) == -1
    assert "map 1: NULL map or destination" in L.last_error()
    assert _to_rgb(L, maps, hs, ws, n, luts, ns, none, (ctypes.c_void_p * n)(None, 16384)) == -1
    assert "map 0: NULL map or destination" in L.last_error()
    assert _to_rgb(L, maps, hs, ws, n, (ctypes.c_void_p * n)(lut.ctypes.data, None), ns, none, dst) == -1
    assert "map 1: NULL lut" in L.last_error()
    assert _to_rgb(L, maps, hs, ws, n, luts, (ctypes.c_int * n)(3, -1), none, dst) == -1
    assert "n_slots" in L.last_error()


def test_python_wrappers_reject_wrong_inputs():
    import torch
    import photohive_dsp_amd as phd
    ok = torch.zeros((400, 400, 3), dtype=torch.uint8)
    for bad in ([ok.float()], [ok.to(torch.int8)], [ok[:, :, :2]], [ok[:, ::2]], [ok.permute(2, 0, 1)],
                ok, ok.unsqueeze(0).float(), [ok.numpy()]):
        with pytest.raises(ValueError):
            phd.reports_device_labels(bad)
    with pytest.raises(TypeError):
        phd.reports_device_labels([ok], no_such_parameter=1)
    with pytest.raises(ValueError):
        phd.reports_device_labels([ok, ok], salient_characters=[None])
    assert phd.reports_device_labels([]) == ([], [])
    lab = torch.zeros((4, 5), dtype=torch.int16)
    for bad in ([lab.to(torch.int32)], [lab.to(torch.uint8)], [lab[0]], [lab[:, ::2]], [lab[:0]]):
        with pytest.raises(ValueError):
            phd.quantize_device(bad, [None])
    with pytest.raises(ValueError):
        phd.quantize_device([lab], [])
    for none in ((0, 0), (0, 0, 256), (-1, 0, 0)):
        with pytest.raises(ValueError):
            phd.quantize_device([lab], [None], none_rgb=none)
    assert phd.quantize_device([], []) == []
