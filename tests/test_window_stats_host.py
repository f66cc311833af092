"""Window statistics without a device: the host twin of k_window_stats
(phd_debug_window_stats_host: stat_unit.h's plain unit and stat_window.h's finish)
against exact Python integers, the definition's restatement with math.sqrt and the
box statistics' twin, bit for bit; against the reference's restatement at the box
statistics' bars; the special windows; every byte phase; every refusal of the two
device entries, which come before any HIP call; the ABI; and the twin under
ASan + UBSan as a stand-alone program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import box_stats_cases as bsc
from tests import window_stats_cases as wtc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("phd_stats_windows_device", "phd_stats_maps_device", "phd_debug_window_stats_host")
CSRC = os.path.join(ROOT, "photohive_dsp_amd", "csrc")


def _lib():
    from photohive_dsp_amd import lib as L
    return L


def _twin(img, boxes, T, sums=True):
    got = wtc.host_twin(img, boxes, T, sums)
    assert not isinstance(got, str), got
    return got


@pytest.fixture(scope="module")
def random_image():
    img = bsc.random_image(wtc.H, wtc.W, 41)
    img.setflags(write=False)
    return img


# ---- 1, 2: the twin against exact integers, the box twin and the reference -----------------
@pytest.mark.parametrize("T", wtc.SIZES)
def test_twin_against_exact_integers_and_the_box_twin(T, random_image):
    img = random_image
    boxes = wtc.grid4(wtc.H, wtc.W, T)
    vals, sums = _twin(img, boxes, T)
    assert sums == bsc.expected_sums(img, boxes)
    assert all(rec[7] == T * T for rec in sums)
    wtc.same_bits(vals, bsc.expected_u8(img, boxes), "the definition in Python doubles")
    box_vals, box_sums = bsc.host_twin(np.ascontiguousarray(img), boxes)
    assert box_sums == sums
    wtc.same_bits(vals, box_vals, "phd_debug_box_stats_host on the same boxes")
    assert vals[-1].tobytes() == vals[-2].tobytes()          # the flush window twice
    wtc.same_bits(_twin(img, boxes, T, sums=False)[0], vals, "without sums")
    assert np.isfinite(vals).all()


@pytest.mark.parametrize("T", wtc.SIZES)
def test_twin_against_the_reference_restatement(T, random_image):
    """oracle.stats of every window's crop and expected_doubles' S-bar, at
    assert_close's bars; no window left out."""
    boxes = wtc.grid4(wtc.H, wtc.W, T)
    vals, _ = _twin(random_image, boxes, T, sums=False)
    bsc.assert_close(vals, wtc.reference_values(random_image, boxes), boxes, f"T = {T}")


# ---- 3: special windows ------------------------------------------------------------------------
@pytest.mark.parametrize("T", wtc.SIZES)
def test_special_windows(T):
    img, boxes = wtc.special_image(T)
    vals, sums = _twin(img, boxes, T)
    assert sums == bsc.expected_sums(img, boxes)
    wtc.same_bits(vals, bsc.expected_u8(img, boxes))
    wtc.assert_special_values(vals, T)
    by = dict(zip(wtc.SPECIALS, sums))
    n = T * T
    assert by["blue"][6] == n and by["blue"][8 + 255] == 255 * n and sum(by["blue"][8:]) == 255 * n
    assert by["one_white"][:8] == [255] * 3 + [65025] * 3 + [0, n] and not any(by["one_white"][8:])
    assert by["constant"][8 + 200] == 163 * n and by["constant"][6] == 0


# ---- 4: odd phases --------------------------------------------------------------------------------
@pytest.mark.parametrize("T", wtc.SIZES)
def test_every_byte_phase_edges_overlaps_and_duplicates(T):
    img = wtc.odd_image()
    boxes = wtc.odd_windows(T)
    vals, sums = _twin(img, boxes, T)
    assert sums == bsc.expected_sums(img, boxes)
    wtc.same_bits(vals, bsc.expected_u8(img, boxes))
    bsc.assert_close(vals, wtc.reference_values(img, boxes), boxes, f"131x197 at {T}")
    assert vals[-1].tobytes() == vals[-2].tobytes() == vals[1].tobytes()
    raw = np.zeros(img.size + 8, np.uint8)
    base = next(j for j in range(4) if (raw.ctypes.data + j) % 4 == 0)
    for off in (1, 2, 3):
        moved = raw[base + off:base + off + img.size].reshape(img.shape)
        moved[...] = img
        assert moved.ctypes.data % 4 == off
        v2, s2 = _twin(moved, boxes, T)
        assert s2 == sums, f"base + {off}"
        wtc.same_bits(v2, vals, f"base + {off}")


# ---- 5: refusals ---------------------------------------------------------------------------------
def _lists(L, imgs, hs, ws, boxes, window, stats, n=None):
    from photohive_dsp_amd.structures import Crop_Boundaries
    k = len(hs)
    cbs = None if boxes is None else \
        (ctypes.POINTER(Crop_Boundaries) * k)(*[ctypes.pointer(b) if b is not None else None for b in boxes])
    return L.lib.phd_stats_windows_device(
        (ctypes.c_void_p * k)(*imgs) if imgs is not None else None, (ctypes.c_int * k)(*hs), (ctypes.c_int * k)(*ws),
        k if n is None else n, cbs, window, (ctypes.c_void_p * k)(*stats) if stats is not None else None, None)


def _maps(L, imgs, hs, ws, window, stride, stats, n=None):
    k = len(hs)
    return L.lib.phd_stats_maps_device(
        (ctypes.c_void_p * k)(*imgs) if imgs is not None else None, (ctypes.c_int * k)(*hs), (ctypes.c_int * k)(*ws),
        k if n is None else n, window, stride, (ctypes.c_void_p * k)(*stats) if stats is not None else None, None)


def test_list_entry_rejects_bad_arguments_before_touching_hip():
    """With or without a device: the pointers below are never dereferenced."""
    L = _lib()
    good = wtc.boundaries([(0, 64, 0, 64), (36, 100, 136, 200)])

    def call(imgs=(4096, 8192), hs=(100, 100), ws=(200, 200), boxes=(good, good), window=64,
             stats=(1 << 20, 2 << 20), n=None):
        rc = _lists(L, None if imgs is None else list(imgs), hs, ws, None if boxes is None else list(boxes), window,
                    None if stats is None else list(stats), n)
        assert rc == -1
        msg = L.last_error()
        assert msg.startswith("phd_stats_windows_device: "), msg
        return msg

    assert "NULL argument" in call(imgs=None)
    assert "NULL argument" in call(boxes=None)
    assert "NULL argument" in call(stats=None)
    assert "n_images must be positive" in call(n=0) and "n_images must be positive" in call(n=-3)
    assert "image 1: NULL image" in call(imgs=(4096, None))
    for w in (0, 8, 24, 48, 96, 256, -64):
        msg = call(window=w)
        assert msg.endswith(f"window must be 16, 32, 64 or 128, not {w}"), msg
    msg = call(boxes=(good, wtc.boundaries([(0, 64, 0, 65)])))
    assert "image 1: window 0 " in msg and msg.endswith("is not 64 x 64"), msg
    msg = call(boxes=(good, wtc.boundaries([(0, 32, 0, 32)])))
    assert "image 1: window 0 " in msg and msg.endswith("is not 64 x 64"), msg
    msg = call(boxes=(wtc.boundaries([(1, 65, 1, 65), (37, 101, 0, 64)]), good))
    assert "image 0: window 1 " in msg and msg.endswith("leaves the 100 x 200 image"), msg
    msg = call(boxes=(wtc.boundaries([(-1, 63, 0, 64)]), good))
    assert "image 0: window 0 " in msg and msg.endswith("leaves the 100 x 200 image"), msg
    assert call(hs=(100, 63)).endswith("image 1: 63 x 200 is smaller than the window 64")
    assert call(ws=(15, 200), window=16).endswith("image 0: 100 x 15 is smaller than the window 16")
    assert call(stats=(1 << 20, None)).endswith("image 1: NULL d_stats for 2 windows")
    # an image without windows needs no d_stats; its neighbour's refusal still comes
    msg = call(boxes=(None, wtc.boundaries([(0, 64, 0, 63)])), stats=(None, 1 << 20))
    assert "image 1: window 0 " in msg, msg


def test_grid_entry_rejects_bad_arguments_before_touching_hip():
    L = _lib()

    def call(imgs=(4096, 8192), hs=(100, 100), ws=(200, 200), window=64, stride=64, stats=(1 << 20, 2 << 20),
             n=None):
        rc = _maps(L, None if imgs is None else list(imgs), hs, ws, window, stride,
                   None if stats is None else list(stats), n)
        assert rc == -1
        msg = L.last_error()
        assert msg.startswith("phd_stats_maps_device: "), msg
        return msg

    assert "NULL argument" in call(imgs=None)
    assert "NULL argument" in call(stats=None)
    assert "n_images must be positive" in call(n=0)
    assert "image 0: NULL image" in call(imgs=(None, 8192))
    for w in (0, 48, 256):
        assert call(window=w).endswith(f"window must be 16, 32, 64 or 128, not {w}")
    for s in (0, -1):
        assert call(stride=s).endswith(f"stride must be positive, not {s}")
    assert call(ws=(200, 50)).endswith("image 1: 100 x 50 is smaller than the window 64")
    assert call(window=128).endswith("image 0: 100 x 200 is smaller than the window 128")
    assert call(stats=(None, 2 << 20)).endswith("image 0: NULL d_stats for 3 windows")   # 100 x 200 at 64 / 64: 1 x 3
    # three images of 2147483647^2 pixels at stride 1: refused at the first, before any pointer is read
    top = 2147483647
    for T in wtc.SIZES:
        msg = call(imgs=(4096, 8192, 12288), hs=(top,) * 3, ws=(top,) * 3, window=T, stride=1,
                   stats=(1 << 20, 2 << 20, 3 << 20))
        assert msg.endswith("too many windows"), msg
    # 46341^2 windows of 16 at stride 1 is one too many; image 1's own defect is never reached
    big = 46340 + 16
    msg = call(imgs=(4096, None), hs=(big, 100), ws=(big, 200), window=16, stride=1)
    assert msg.endswith("too many windows") and "image 1" not in msg, msg


def test_a_call_without_windows_does_nothing_and_succeeds():
    """No window at all: 0 before any device work, so also without a device."""
    L = _lib()
    none = wtc.boundaries([])
    for T in wtc.SIZES:
        assert _lists(L, [4096, 8192], (200, 200), (200, 200), [None, none], T, [None, None]) == 0
    import photohive_dsp_amd as phd
    assert phd.stats_windows_device([], []) == [] and phd.stats_maps_device([], stride=0) == []
    with pytest.raises(ValueError, match="windows has 1 entries for 0 images"):
        phd.stats_windows_device([], [None])


def test_twin_rejects_bad_arguments():
    img = np.zeros((100, 200, 3), np.uint8)
    for boxes, window, what in (([(0, 64, 0, 65)], 64, "window 0 "), ([(0, 48, 0, 48)], 48, "16, 32, 64 or 128, not 48"),
                                ([(0, 128, 0, 128)], 128, "smaller than"), ([(40, 104, 0, 64)], 64, "leaves the")):
        msg = wtc.host_twin(img, boxes, window)
        assert isinstance(msg, str) and msg.startswith("phd_debug_window_stats_host: ") and what in msg, (what, msg)
    L = _lib()
    cb = wtc.boundaries([(0, 16, 0, 16)])
    assert L.lib.phd_debug_window_stats_host(None, 100, 200, ctypes.byref(cb), 16, None, None) == -1
    assert "NULL image" in L.last_error()
    assert L.lib.phd_debug_window_stats_host(img.ctypes.data, 100, 200, ctypes.byref(cb), 16, None, None) == -1
    assert "NULL stats" in L.last_error()
    assert L.lib.phd_debug_window_stats_host(img.ctypes.data, 100, 200, None, 16, None, None) == 0


# ---- 6: the ABI -------------------------------------------------------------------------------------
def test_symbols_documents_and_python_names():
    L = _lib()
    so = ctypes.CDLL(os.path.join(ROOT, "photohive_dsp_amd", "PhotoHive_DSP_lib", "libreport_data.so"))
    for name in ENTRIES:
        assert hasattr(so, name), name
        assert getattr(L.lib, name).argtypes is not None and getattr(L.lib, name).restype is ctypes.c_int, name
    assert len(L.lib.phd_stats_windows_device.argtypes) == 8 and len(L.lib.phd_stats_maps_device.argtypes) == 8
    assert len(L.lib.phd_debug_window_stats_host.argtypes) == 7
    assert L.WINDOW_STATS_KERNEL == 17 and L.WINDOW_SHARP_KERNEL == 16
    with open(os.path.join(ROOT, "include", "photohive_dsp.h")) as f:
        h = f.read()
    for s in ("16 window_sharp", "17 window_stats", "src/image_processing.c:543-553", "src/filtering.c:125-148") + \
            tuple(e + "(" for e in ENTRIES):
        assert s in h, s
    import photohive_dsp_amd as phd
    assert callable(phd.stats_windows_device) and callable(phd.stats_maps_device)


def test_twin_compiles_host_only(tmp_path):
    """phd_statwin.cpp -DPHD_STATWIN_HOST_ONLY needs no HIP header and defines the twin alone."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    obj = tmp_path / "phd_statwin.o"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                    "-DPHD_STATWIN_HOST_ONLY", "-c", "-o", str(obj), os.path.join(CSRC, "phd_statwin.cpp")],
                   check=True, timeout=300)
    nm = subprocess.run(["nm", "--defined-only", str(obj)], capture_output=True, text=True, check=True).stdout
    assert " T phd_debug_window_stats_host" in nm
    assert "phd_stats_windows_device" not in nm and "phd_stats_maps_device" not in nm


# ---- 7: the sanitizer build --------------------------------------------------------------------------
def test_host_twin_under_asan(tmp_path):
    """phd_statwin.cpp's host half and a C++ driver built with ASan + UBSan, run as
    their own process: heap images of exactly 3 H W bytes at each of the four sizes,
    windows flush with every edge."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "window_stats_asan"
    src = [os.path.join(ROOT, "tests", "native", "window_stats_asan.cpp"), os.path.join(CSRC, "phd_statwin.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-DPHD_STATWIN_HOST_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe)] + src, check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "window statistics host OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
