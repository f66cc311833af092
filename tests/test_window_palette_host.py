"""Window palettes without a device: the host twin of k_window_palette
(phd_debug_window_palette_host: pal_window.h's unit, clamp and dominant key)
against numpy and the box palettes' twin, integer for integer; the slot-count
edges on either side of every threshold of the copies rule; the special windows;
every base phase; counts-only and dominant-only calls; every refusal of the two
device entries, which come before any HIP call, and of the twin; the ABI; the
host-only build; and the twin under ASan + UBSan as a stand-alone program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import box_palette_cases as bpc
from tests import window_palette_cases as wpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("phd_palette_windows_device", "phd_palette_maps_device", "phd_debug_window_palette_host")
CSRC = os.path.join(ROOT, "photohive_dsp_amd", "csrc")


def _lib():
    from photohive_dsp_amd import lib as L
    return L


def _twin(lab, boxes, n_slots, T, **kw):
    got = wpc.host_twin(lab, boxes, n_slots, T, **kw)
    assert not isinstance(got, str), got
    return got


def _check(lab, boxes, n_slots, T, what=""):
    """The twin on every window against numpy and the box twin; returns its values."""
    counts, dom = _twin(lab, boxes, n_slots, T)
    want_c, want_d = wpc.expected(lab, boxes, n_slots)
    assert np.array_equal(counts, want_c), what
    assert np.array_equal(counts, bpc.host_counts(lab, boxes, n_slots)), what
    assert np.array_equal(dom, want_d), what
    assert (counts.sum(axis=1, dtype=np.int64) == T * T).all(), what
    return counts, dom


# ---- the twin against numpy and the box twin ---------------------------------------------------
@pytest.mark.parametrize("T", wpc.SIZES)
def test_twin_against_numpy_and_the_box_twin(T):
    lab = wpc.odd_map()
    boxes = wpc.odd_windows(T)
    assert {l % 4 for _, _, l, _ in boxes} == {0, 1, 2, 3}
    assert any(t == 0 for t, _, _, _ in boxes) and any(b == wpc.ODD_H for _, b, _, _ in boxes)
    assert any(l == 0 for _, _, l, _ in boxes) and any(r == wpc.ODD_W for _, _, _, r in boxes)
    assert (wpc.ODD_H - T, wpc.ODD_H, wpc.ODD_W - T, wpc.ODD_W) in boxes
    counts, dom = _check(lab, boxes, 17, T)
    assert counts[-1].tobytes() == counts[-2].tobytes() == counts[1].tobytes() and dom[-1] == dom[-2] == dom[1]
    for elems in (1, 2, 3):                                   # base + 2, + 4, + 6 bytes
        moved = bpc.at_offset(lab, elems)
        c2, d2 = _check(moved, boxes, 17, T, f"base + {2 * elems}")
        assert np.array_equal(c2, counts) and np.array_equal(d2, dom), f"base + {2 * elems}"


# ---- slot-count edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (16, 128))
@pytest.mark.parametrize("n_slots", wpc.SLOT_EDGES)
def test_slot_count_edges(n_slots, T):
    lab = bpc.random_map(140, 150, n_slots, 900 + n_slots)
    _check(lab, wpc.edge_windows(T, 140, 150), n_slots, T)


def test_slot_edges_sit_on_either_side_of_every_copies_threshold(tmp_path):
    """pal_window.h's own pw_copies, compiled (tests/native/pal_window_rule.cpp): wherever the number
    of copies changes, SLOT_EDGES has the n_slots on either side; the rule's invariants hold for
    every counter count; the launch's LDS at 4096 slots is the one copy's."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "pal_window_rule"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "pal_window_rule.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    rule = {int(ln[1]): (int(ln[3]), [int(x) for x in ln[5:]]) for ln in lines if ln[0] == "T"}
    lds = {int(ln[1]): (int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "lds"}
    assert set(rule) == set(lds) == set(wpc.SIZES)
    seen = set()
    for T in wpc.SIZES:
        most, changes = rule[T]
        assert most > 1 and changes, (T, rule[T])             # small palettes get several copies
        for nc in changes:                                    # counters nc - 1 and nc: n_slots nc - 2 and nc - 1
            assert nc - 2 in wpc.SLOT_EDGES and nc - 1 in wpc.SLOT_EDGES, (T, nc)
            seen.add(nc - 1)
        assert lds[T] == (4100, 4100)                         # one copy of 4097 counters, rounded up to four
    assert seen == set(wpc.COPY_THRESHOLDS)                   # and the edges list no threshold the rule lacks


# ---- special windows -------------------------------------------------------------------------------
@pytest.mark.parametrize("T", wpc.SIZES)
def test_special_windows(T):
    lab, boxes, ns, doms = wpc.special_map(T)
    counts, dom = _check(lab, boxes, ns, T)
    assert np.array_equal(dom, doms)
    by = dict(zip(wpc.SPECIALS, counts))
    n = T * T
    assert by["single"][9] == n
    assert by["alternating"][4] == by["alternating"][11] == n // 2
    assert by["all_none"][17] == n and by["over"][17] == n
    assert by["half_2_5"][2] == by["half_2_5"][5] == n // 2
    assert by["half_none_3"][3] == by["half_none_3"][17] == n // 2
    assert by["none_majority"][17] == n // 2 + 1 and by["none_majority"][3] == n // 2 - 1
    # no slots at all: every element is "none"
    c0, d0 = _check(lab, boxes, 0, T)
    assert (c0 == n).all() and (d0 == wpc.NONE).all()


# ---- counts-only and dominant-only ---------------------------------------------------------------
@pytest.mark.parametrize("T", wpc.SIZES)
def test_counts_only_and_dominant_only(T):
    lab = wpc.odd_map()
    boxes = wpc.odd_windows(T)
    both_c, both_d = _twin(lab, boxes, 17, T)
    c, d = _twin(lab, boxes, 17, T, dominant=False, fill=0xA5A5A5A5)
    assert np.array_equal(c, both_c) and (d == 0xA5A5).all()
    c, d = _twin(lab, boxes, 17, T, counts=False, fill=0xA5A5A5A5)
    assert np.array_equal(d, both_d) and (c == 0xA5A5A5A5).all()


# ---- refusals ---------------------------------------------------------------------------------------
def _arr(ctype, vals, k):
    return None if vals is None else (ctype * k)(*vals)


def _lists(L, maps, hs, ws, ns, boxes, window, counts, dominant, n=None):
    from photohive_dsp_amd.structures import Crop_Boundaries
    k = len(hs)
    cbs = None if boxes is None else \
        (ctypes.POINTER(Crop_Boundaries) * k)(*[ctypes.pointer(b) if b is not None else None for b in boxes])
    return L.lib.phd_palette_windows_device(
        _arr(ctypes.c_void_p, maps, k), (ctypes.c_int * k)(*hs), (ctypes.c_int * k)(*ws), k if n is None else n,
        _arr(ctypes.c_int, ns, k), cbs, window, _arr(ctypes.c_void_p, counts, k), _arr(ctypes.c_void_p, dominant, k),
        None)


def _maps(L, maps, hs, ws, ns, window, stride, counts, dominant, n=None):
    k = len(hs)
    return L.lib.phd_palette_maps_device(
        _arr(ctypes.c_void_p, maps, k), (ctypes.c_int * k)(*hs), (ctypes.c_int * k)(*ws), k if n is None else n,
        _arr(ctypes.c_int, ns, k), window, stride, _arr(ctypes.c_void_p, counts, k),
        _arr(ctypes.c_void_p, dominant, k), None)


def test_list_entry_rejects_bad_arguments_before_touching_hip():
    """With or without a device: the pointers below are never dereferenced."""
    L = _lib()
    good = wpc.boundaries([(0, 64, 0, 64), (36, 100, 136, 200)])

    def call(maps=(4096, 8192), hs=(100, 100), ws=(200, 200), ns=(17, 17), boxes=(good, good), window=64,
             counts=(1 << 20, 2 << 20), dominant=(3 << 20, 4 << 20), n=None):
        rc = _lists(L, maps, hs, ws, ns, None if boxes is None else list(boxes), window, counts, dominant, n)
        assert rc == -1
        msg = L.last_error()
        assert msg.startswith("phd_palette_windows_device: "), msg
        return msg

    assert call(maps=None).endswith(": NULL argument")
    assert call(ns=None).endswith(": NULL argument")
    assert call(boxes=None).endswith(": NULL argument")
    assert call(counts=None, dominant=None).endswith(": NULL argument")
    assert call(n=0).endswith("n_maps must be positive") and call(n=-3).endswith("n_maps must be positive")
    assert call(maps=(4096, None)).endswith("map 1: NULL map")
    for w in (0, 8, 24, 48, 96, 256, -64):
        assert call(window=w).endswith(f"window must be 16, 32, 64 or 128, not {w}")
    msg = call(boxes=(good, wpc.boundaries([(0, 64, 0, 65)])))
    assert "map 1: window 0 (top 0, bottom 64, left 0, right 65)" in msg and msg.endswith("is not 64 x 64"), msg
    msg = call(boxes=(good, wpc.boundaries([(0, 32, 0, 32)])))
    assert "map 1: window 0 " in msg and msg.endswith("is not 64 x 64"), msg
    msg = call(boxes=(wpc.boundaries([(1, 65, 1, 65), (37, 101, 0, 64)]), good))
    assert "map 0: window 1 " in msg and msg.endswith("leaves the 100 x 200 map"), msg
    msg = call(boxes=(wpc.boundaries([(-1, 63, 0, 64)]), good))
    assert "map 0: window 0 " in msg and msg.endswith("leaves the 100 x 200 map"), msg
    assert call(hs=(100, 63)).endswith("map 1: 63 x 200 is smaller than the window 64")
    assert call(ws=(15, 200), window=16).endswith("map 0: 100 x 15 is smaller than the window 16")
    assert call(ns=(17, -1)).endswith("map 1: n_slots must be in 0..4096, not -1")
    assert call(ns=(4097, 17)).endswith("map 0: n_slots must be in 0..4096, not 4097")
    assert call(counts=(1 << 20, None), dominant=(None, None)).endswith(
        "map 1: neither d_counts nor d_dominant for 2 windows")
    assert call(counts=None, dominant=(None, 4 << 20)).endswith("map 0: neither d_counts nor d_dominant for 2 windows")
    assert call(maps=(4096, 8193)).endswith("map 1: the map is not 2-byte aligned")
    assert call(counts=((1 << 20) + 2, 2 << 20)).endswith("map 0: d_counts is not 4-byte aligned")
    assert call(dominant=(3 << 20, (4 << 20) + 1)).endswith("map 1: d_dominant is not 2-byte aligned")
    # a map without windows needs no output; its neighbour's refusal still comes
    msg = call(boxes=(None, wpc.boundaries([(0, 64, 0, 63)])), counts=(None, 1 << 20), dominant=None)
    assert "map 1: window 0 " in msg, msg


def test_grid_entry_rejects_bad_arguments_before_touching_hip():
    L = _lib()

    def call(maps=(4096, 8192), hs=(100, 100), ws=(200, 200), ns=(17, 17), window=64, stride=64,
             counts=(1 << 20, 2 << 20), dominant=(3 << 20, 4 << 20), n=None):
        rc = _maps(L, maps, hs, ws, ns, window, stride, counts, dominant, n)
        assert rc == -1
        msg = L.last_error()
        assert msg.startswith("phd_palette_maps_device: "), msg
        return msg

    assert call(maps=None).endswith(": NULL argument")
    assert call(ns=None).endswith(": NULL argument")
    assert call(counts=None, dominant=None).endswith(": NULL argument")
    assert call(n=0).endswith("n_maps must be positive")
    assert call(maps=(None, 8192)).endswith("map 0: NULL map")
    for w in (0, 48, 256):
        assert call(window=w).endswith(f"window must be 16, 32, 64 or 128, not {w}")
    for s in (0, -1):
        assert call(stride=s).endswith(f"stride must be positive, not {s}")
    assert call(ws=(200, 50)).endswith("map 1: 100 x 50 is smaller than the window 64")
    assert call(window=128).endswith("map 0: 100 x 200 is smaller than the window 128")
    assert call(ns=(-1, 17)).endswith("map 0: n_slots must be in 0..4096, not -1")
    assert call(ns=(17, 4097)).endswith("map 1: n_slots must be in 0..4096, not 4097")
    # 100 x 200 at 64 / 64: 1 x 3 windows
    assert call(counts=(None, 2 << 20), dominant=None).endswith("map 0: neither d_counts nor d_dominant for 3 windows")
    assert call(maps=(4097, 8192)).endswith("map 0: the map is not 2-byte aligned")
    assert call(counts=(1 << 20, (2 << 20) + 1)).endswith("map 1: d_counts is not 4-byte aligned")
    assert call(dominant=((3 << 20) + 1, 4 << 20)).endswith("map 0: d_dominant is not 2-byte aligned")
    # three maps of 2147483647^2 labels at stride 1: refused at the first, before any pointer is read
    top = 2147483647
    for T in wpc.SIZES:
        msg = call(maps=(4096, 8192, 12288), hs=(top,) * 3, ws=(top,) * 3, ns=(17,) * 3, window=T, stride=1,
                   counts=(1 << 20, 2 << 20, 3 << 20), dominant=None)
        assert msg.endswith("too many windows"), msg


def test_a_call_without_windows_does_nothing_and_succeeds():
    """No window at all: 0 before any device work, so also without a device."""
    L = _lib()
    none = wpc.boundaries([])
    for T in wpc.SIZES:
        assert _lists(L, (4096, 8192), (200, 200), (200, 200), (17, 0), [None, none], T, (None, None), None) == 0
    import photohive_dsp_amd as phd
    assert phd.palette_windows_device([], [], []) == [] and phd.palette_maps_device([], [], stride=0) == []
    with pytest.raises(ValueError, match="windows has 1 entries for 0 maps"):
        phd.palette_windows_device([], [], [None])
    with pytest.raises(ValueError, match="counts or dominant"):
        phd.palette_maps_device([], [], counts=False)


def test_twin_rejects_bad_arguments():
    lab = np.zeros((100, 200), np.uint16)
    for boxes, window, ns, what in (([(0, 64, 0, 65)], 64, 17,
                                     "window 0 (top 0, bottom 64, left 0, right 65) is not 64 x 64"),
                                    ([(0, 48, 0, 48)], 48, 17, "window must be 16, 32, 64 or 128, not 48"),
                                    ([(0, 128, 0, 128)], 128, 17, "100 x 200 is smaller than the window 128"),
                                    ([(40, 104, 0, 64)], 64, 17, "leaves the 100 x 200 map"),
                                    ([(0, 64, 0, 64)], 64, -1, "n_slots must be in 0..4096, not -1"),
                                    ([(0, 64, 0, 64)], 64, 4097, "n_slots must be in 0..4096, not 4097")):
        msg = wpc.host_twin(lab, boxes, ns, window)
        assert isinstance(msg, str) and msg.startswith("phd_debug_window_palette_host: ") and msg.endswith(what), msg
    L = _lib()
    cb = wpc.boundaries([(0, 16, 0, 16)])
    assert L.lib.phd_debug_window_palette_host(None, 100, 200, 17, ctypes.byref(cb), 16, None, None) == -1
    assert L.last_error() == "phd_debug_window_palette_host: NULL map"
    assert L.lib.phd_debug_window_palette_host(lab.ctypes.data, 100, 200, 17, ctypes.byref(cb), 16, None, None) == -1
    assert L.last_error() == "phd_debug_window_palette_host: NULL counts and dominant"
    assert L.lib.phd_debug_window_palette_host(lab.ctypes.data, 100, 200, 17, None, 16, None, None) == 0


# ---- the ABI ------------------------------------------------------------------------------------------
def test_symbols_documents_and_python_names():
    L = _lib()
    so = ctypes.CDLL(os.path.join(ROOT, "photohive_dsp_amd", "PhotoHive_DSP_lib", "libreport_data.so"))
    for name in ENTRIES:
        assert hasattr(so, name), name
        assert getattr(L.lib, name).argtypes is not None and getattr(L.lib, name).restype is ctypes.c_int, name
    assert len(L.lib.phd_palette_windows_device.argtypes) == 10 and len(L.lib.phd_palette_maps_device.argtypes) == 10
    assert len(L.lib.phd_debug_window_palette_host.argtypes) == 8
    assert L.WINDOW_PALETTE_KERNEL == 18
    with open(os.path.join(ROOT, "include", "photohive_dsp.h")) as f:
        h = f.read()
    for s in ("18 window_palette", "src/color_quantization.c:342-479", ":510-576", "src/image_processing.c:213-232") + \
            tuple(e + "(" for e in ENTRIES):
        assert s in h, s
    import photohive_dsp_amd as phd
    assert callable(phd.palette_windows_device) and callable(phd.palette_maps_device)


def test_twin_compiles_host_only(tmp_path):
    """phd_palwin.cpp -DPHD_PALWIN_HOST_ONLY needs no HIP header and defines the twin alone."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    obj = tmp_path / "phd_palwin.o"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-DPHD_PALWIN_HOST_ONLY", "-c", "-o",
                    str(obj), os.path.join(CSRC, "phd_palwin.cpp")], check=True, timeout=300)
    nm = subprocess.run(["nm", "--defined-only", str(obj)], capture_output=True, text=True, check=True).stdout
    assert " T phd_debug_window_palette_host" in nm
    assert "phd_palette_windows_device" not in nm and "phd_palette_maps_device" not in nm


# ---- the sanitizer build -------------------------------------------------------------------------------
def test_host_twin_under_asan(tmp_path):
    """phd_palwin.cpp's host half and a C++ driver built with ASan + UBSan, run as
    their own process: heap maps of exactly 2 mh mw bytes at each of the four sizes,
    windows flush with every edge, n_slots 0, 17 and 4096."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "window_palette_asan"
    src = [os.path.join(ROOT, "tests", "native", "window_palette_asan.cpp"), os.path.join(CSRC, "phd_palwin.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-DPHD_PALWIN_HOST_ONLY",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + src,
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "window palette host OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
