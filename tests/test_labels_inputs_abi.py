"""The label map entries of views, typed views and YUV frames without a device:
the symbols and their declared argument types, the argument checks that come
before any HIP call, and the Python wrappers' input checks (the packed
entry's: tests/test_labels_abi.py)."""
import ctypes

import pytest

ENTRIES = ("views", "typed_views", "yuv")


def _lib():
    from photohive_dsp_amd import lib as L
    return L


def _view_types():
    from photohive_dsp_amd.structures import PhdImageView, PhdTypedView, PhdYuvView
    return dict(views=PhdImageView, typed_views=PhdTypedView, yuv=PhdYuvView)


def _args(n=1):
    from photohive_dsp_amd.structures import Full_Report_Data
    return (ctypes.POINTER(Full_Report_Data) * n)(), (ctypes.c_int * n)()


def test_symbols_and_argument_types():
    """Each entry is the existing call plus d_labels, in the packed labels
    entry's order: (views, n, cfg, crops, d_labels, out, status, stream)."""
    L = _lib()
    from photohive_dsp_amd.structures import Crop_Boundaries, Full_Report_Data, PhdConfig
    P = ctypes.POINTER
    for name, view in _view_types().items():
        f = getattr(L.lib, f"phd_report_batch_device_{name}_labels")
        assert f.restype is ctypes.c_int
        assert list(f.argtypes) == [P(view), ctypes.c_int, P(PhdConfig), P(P(Crop_Boundaries)), ctypes.c_void_p,
                                    P(P(Full_Report_Data)), P(ctypes.c_int), ctypes.c_void_p], name
        plain = getattr(L.lib, f"phd_report_batch_device_{name}")
        assert list(plain.argtypes) == list(f.argtypes[:4]) + list(f.argtypes[5:]), name


def test_header_declares_the_entries():
    import os
    from tests.conftest import ROOT
    with open(os.path.join(ROOT, "include", "photohive_dsp.h")) as f:
        h = f.read()
    for s in ("int phd_report_batch_device_views_labels(const phd_image_view* views,",
              "int phd_report_batch_device_typed_views_labels(const phd_typed_view* views,",
              "int phd_report_batch_device_yuv_labels(const phd_yuv_view* views,"):
        assert s in h, s
        decl = h[h.index(s):]
        decl = " ".join(decl[:decl.index(";")].split())
        assert decl.endswith("const Crop_Boundaries* const* crops, uint16_t* const* d_labels, Full_Report_Data** out, "
                             "int* status, void* stream)"), decl


@pytest.mark.parametrize("name", ENTRIES)
def test_bad_arguments_come_first(name):
    """-1 and a message that names the entry, before any HIP call (the
    pointers are never dereferenced); with d_labels NULL the call is the plain
    entry and says so."""
    L = _lib()
    from photohive_dsp_amd.core import make_config
    cfg = make_config()
    views = (_view_types()[name] * 1)()
    maps = (ctypes.c_void_p * 1)(8192)
    outs, st = _args()
    f = getattr(L.lib, f"phd_report_batch_device_{name}_labels")
    entry = f"phd_report_batch_device_{name}_labels"
    for bad in (dict(views=None), dict(cfg=None), dict(outs=None), dict(st=None), dict(n=0), dict(n=-3)):
        a = dict(views=views, n=1, cfg=ctypes.byref(cfg), outs=outs, st=st)
        a.update(bad)
        assert f(a["views"], a["n"], a["cfg"], None, maps, a["outs"], a["st"], None) == -1, bad
        assert f"{entry}: bad arguments" in L.last_error(), (bad, L.last_error())
    assert f(None, 1, ctypes.byref(cfg), None, None, outs, st, None) == -1
    assert f"phd_report_batch_device_{name}: bad arguments" in L.last_error()
    # 64 * 32 * 16 + 17 octree groups: a slot could reach PHD_LABEL_NONE's sign bit
    big = make_config(h_partitions=64, s_partitions=32, v_partitions=16)
    assert f(views, 1, ctypes.byref(big), None, maps, outs, st, None) == -1
    assert f"{entry}: label maps need fewer than 32768 octree groups" in L.last_error()


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_without_a_device(name):
    import torch
    L = _lib()
    from photohive_dsp_amd.core import make_config
    cfg = make_config()
    views = (_view_types()[name] * 1)()                      # a zeroed descriptor: invalid
    maps = (ctypes.c_void_p * 1)(8192)
    outs, st = _args()
    f = getattr(L.lib, f"phd_report_batch_device_{name}_labels")
    rc = f(views, 1, ctypes.byref(cfg), None, maps, outs, st, None)
    if torch.cuda.is_available():
        assert rc == 1 and st[0] != 0 and "image 0" in L.last_error()      # the bad view fails alone
    else:
        assert rc == -1 and "no HIP device" in L.last_error()
    assert not outs[0]


def test_python_wrappers_reject_non_tensor_inputs_with_labels():
    """labels=True allocates each map on its image's device: a descriptor
    that is no tensor is refused before anything is called."""
    import torch
    import photohive_dsp_amd as phd
    from photohive_dsp_amd.structures import PhdImageView, PhdTypedView, PhdYuvView
    ok = torch.zeros((400, 400, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="labels=True needs torch tensors"):
        phd.reports_device_views([ok, PhdImageView()], labels=True)
    with pytest.raises(ValueError, match="labels=True needs torch tensors"):
        phd.reports_device_typed([PhdTypedView()], labels=True)
    y = torch.zeros((400, 400), dtype=torch.uint8)
    with pytest.raises(ValueError, match="labels=True needs torch tensors"):
        phd.reports_device_yuv([(y, y, y), PhdYuvView()], labels=True)
    # the inputs' own checks still come first
    with pytest.raises(ValueError):
        phd.reports_device_views([ok.numpy()], labels=True)
    with pytest.raises(ValueError):
        phd.reports_device_typed([ok.to(torch.int32)], labels=True)
    with pytest.raises(ValueError):
        phd.reports_device_yuv([(y,)], labels=True)
    with pytest.raises(ValueError):
        phd.reports_device_views([ok, ok], labels=True, salient_characters=[None])
    with pytest.raises(TypeError):
        phd.reports_device_views([ok], labels=True, no_such_parameter=1)
    for fn in (phd.reports_device_views, phd.reports_device_typed, phd.reports_device_yuv):
        assert fn([], labels=True) == ([], [])
