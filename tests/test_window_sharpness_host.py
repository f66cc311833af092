"""Window sharpness without a device: the host twin of k_window_sharp
(phd_debug_window_sharpness_host: sharp_window.h's row code and finish) against
oracle.sharpness at both bars of tests/sharp_boxes.py, and bit for bit against a
Python big-integer restatement of the header's definition; the special windows;
every refusal of the two device entries, which come before any HIP call; the ABI;
and the twin, and the plan of a window call (window_call.h), under ASan + UBSan as
stand-alone programs."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import window_sharp_cases as wsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("phd_sharpness_windows_device", "phd_sharpness_maps_device", "phd_debug_window_sharpness_host")


def _lib():
    from photohive_dsp_amd import lib as L
    return L


def _check_bigint(img, boxes, s, v, u):
    want = [wsc.bigint_window(img, b) for b in boxes]
    assert wsc.same_bits(s, [x[0] for x in want])
    assert wsc.same_bits(v, [x[1] for x in want])
    assert [int(a) for a in u[:, 0]] == [x[2] for x in want]
    assert [int(a) for a in u[:, 1]] == [x[3] for x in want]
    return want


def test_symbols_documents_and_python_names():
    L = _lib()
    so = ctypes.CDLL(os.path.join(ROOT, "photohive_dsp_amd", "PhotoHive_DSP_lib", "libreport_data.so"))
    for name in ENTRIES:
        assert hasattr(so, name), name
        assert getattr(L.lib, name).argtypes is not None, name
    assert L.WINDOW_SHARP_KERNEL == 16
    with open(os.path.join(ROOT, "include", "photohive_dsp.h")) as f:
        h = f.read()
    for s in ("16 window_sharp", "15 window_vectors") + tuple(e + "(" for e in ENTRIES):
        assert s in h, s
    import photohive_dsp_amd as phd
    assert callable(phd.sharpness_windows_device) and callable(phd.sharpness_maps_device)


@pytest.mark.parametrize("T", wsc.SIZES)
def test_twin_against_oracle_and_big_integers(T):
    """The five kinds at 353 x 350: a 4 x 4 grid and the flush bottom-right window."""
    boxes = wsc.grid4(wsc.H, wsc.W, T)
    for kind in wsc.KINDS:
        img = wsc.kind_image(kind)
        s, v, u = wsc.host_twin(img, boxes, T)
        wsc.assert_against_oracle(img, boxes, s, u)
        _check_bigint(img, boxes, s, v, u)
        assert s[-1].tobytes() == s[-2].tobytes()            # the flush window twice: the same bits
        # without the optional outputs: the same sharpness
        assert wsc.same_bits(wsc.host_twin(img, boxes, T, variance=False, sums=False)[0], s)


def test_d_needs_more_than_64_bits_on_noise_at_128():
    img = wsc.kind_image("uniform")
    boxes = wsc.grid4(wsc.H, wsc.W, 128)
    s, v, u = wsc.host_twin(img, boxes, 128)
    want = _check_bigint(img, boxes, s, v, u)
    top = max(x[4] for x in want)
    print("largest D:", top.bit_length(), "bits")
    assert top >= 2 ** 64


@pytest.mark.parametrize("T", wsc.SIZES)
def test_special_windows(T):
    # each special window in the middle of a 255-filled frame: nothing outside the window counts
    def run(name):
        img = np.full((T + 9, T + 7, 3), 255, np.uint8)
        img[4:4 + T, 3:3 + T] = wsc.special_window(name, T)
        box = [(4, 4 + T, 3, 3 + T)]
        s, v, u = wsc.host_twin(img, box, T)
        _check_bigint(img, box, s, v, u)
        return img, box, float(s[0]), float(v[0]), int(u[0, 0]), int(u[0, 1])

    _, _, s, v, s1, s2 = run("black")
    assert math.isnan(s) and v == 0.0 and s1 == 0 and s2 == 0
    _, _, s, v, s1, s2 = run("black_ring")
    assert s == math.inf and v > 0 and s1 == 0 and s2 > 0
    L = 255000
    for name, lum in (("grey", 128 * 1000), ("white", L)):
        img, box, s, v, s1, s2 = run(name)
        # f is 3 l on the 4 (T - 2) edge pixels, 5 l at the corners and 0 inside
        assert s1 == (12 * (T - 2) + 20) * lum and s2 == (36 * (T - 2) + 100) * lum * lum
        wsc.assert_against_oracle(img, box, [s], np.array([[s1, s2]]))
    # by hand: one white pixel at the corner has f = 8 L there and -L at its three neighbours
    img, box, s, v, s1, s2 = run("corner")
    n = T * T
    assert s1 == 5 * L and s2 == 67 * L * L
    d = n * 67 - 25                                          # D / L^2
    assert v == d / (n * n)                                  # a dyadic quotient: exact
    assert s == float(d * L * L) / ((float(n) * float(5 * L)) * 255000.0)
    assert abs(s - d / (5 * n)) <= 3e-16 * s                 # one rounding on either side, 2^-53 each
    if T == 16:
        assert (s1, s2, d) == (1275000, 67 * 65025000000, 17127) and v == 17127 / 65536
    wsc.assert_against_oracle(img, box, [s], np.array([[s1, s2]]))


@pytest.mark.parametrize("T", wsc.SIZES)
def test_every_byte_phase_edges_overlaps_and_duplicates(T):
    img = wsc.odd_image()
    boxes = wsc.odd_windows(T)
    s, v, u = wsc.host_twin(img, boxes, T)
    _check_bigint(img, boxes, s, v, u)
    wsc.assert_against_oracle(img, boxes, s, u)
    assert s[-1].tobytes() == s[-2].tobytes() == s[1].tobytes() and v[-1].tobytes() == v[1].tobytes()
    # the image at every alignment of host memory: the same bits
    raw = np.zeros(img.size + 8, np.uint8)
    for off in (1, 2, 3):
        moved = raw[off:off + img.size].reshape(img.shape)
        moved[...] = img
        s2, v2, u2 = wsc.host_twin(moved, boxes, T)
        assert wsc.same_bits(s2, s) and wsc.same_bits(v2, v) and np.array_equal(u2, u)


# ---- refusals ----------------------------------------------------------------------------
def _lists(L, imgs, hs, ws, boxes, window, sharp, var, n=None):
    from photohive_dsp_amd.structures import Crop_Boundaries
    k = len(imgs)
    cbs = None if boxes is None else \
        (ctypes.POINTER(Crop_Boundaries) * k)(*[ctypes.pointer(b) if b is not None else None for b in boxes])
    return L.lib.phd_sharpness_windows_device(
        (ctypes.c_void_p * k)(*imgs) if imgs is not None else None, (ctypes.c_int * k)(*hs), (ctypes.c_int * k)(*ws),
        k if n is None else n, cbs, window, (ctypes.c_void_p * k)(*sharp) if sharp is not None else None,
        (ctypes.c_void_p * k)(*var) if var is not None else None, None)


def _maps(L, imgs, hs, ws, window, stride, sharp, var, n=None):
    k = len(imgs)
    return L.lib.phd_sharpness_maps_device(
        (ctypes.c_void_p * k)(*imgs), (ctypes.c_int * k)(*hs), (ctypes.c_int * k)(*ws), k if n is None else n, window,
        stride, (ctypes.c_void_p * k)(*sharp) if sharp is not None else None,
        (ctypes.c_void_p * k)(*var) if var is not None else None, None)


def test_list_entry_rejects_bad_arguments_before_touching_hip():
    """With or without a device: the pointers below are never dereferenced."""
    L = _lib()
    good = wsc.boundaries([(0, 64, 0, 64), (36, 100, 136, 200)])

    def call(imgs=(4096, 8192), hs=(100, 100), ws=(200, 200), boxes=(good, good), window=64,
             sharp=(1 << 20, 2 << 20), var=(3 << 20, None), n=None):
        rc = _lists(L, list(imgs), hs, ws, None if boxes is None else list(boxes), window,
                    None if sharp is None else list(sharp), None if var is None else list(var), n)
        assert rc == -1
        msg = L.last_error()
        assert msg.startswith("phd_sharpness_windows_device: "), msg
        return msg

    assert "NULL argument" in call(boxes=None)
    assert "NULL argument" in call(sharp=None)
    assert "n_images" in call(n=0) and "n_images" in call(n=-3)
    assert "image 1: NULL image" in call(imgs=(4096, None))
    for w in (0, 8, 24, 96, 256, -64):
        msg = call(window=w)
        assert "window must be 16, 32, 64 or 128" in msg and f"not {w}" in msg, msg
    msg = call(boxes=(good, wsc.boundaries([(0, 64, 0, 65)])))
    assert "image 1: window 0 " in msg and "is not 64 x 64" in msg, msg
    msg = call(boxes=(good, wsc.boundaries([(0, 32, 0, 32)])))
    assert "image 1: window 0 " in msg and "is not 64 x 64" in msg, msg
    msg = call(boxes=(wsc.boundaries([(1, 65, 1, 65), (37, 101, 0, 64)]), good))
    assert "image 0: window 1 " in msg and "leaves the 100 x 200 image" in msg, msg
    msg = call(boxes=(wsc.boundaries([(-1, 63, 0, 64)]), good))
    assert "image 0: window 0 " in msg and "leaves the 100 x 200 image" in msg, msg
    assert "image 1: 63 x 200 is smaller than the window 64" in call(hs=(100, 63))
    assert "image 0: 100 x 15 is smaller than the window 16" in call(ws=(15, 200), window=16)
    msg = call(sharp=(1 << 20, None))
    assert "image 1: NULL d_sharpness for 2 windows" in msg, msg
    # an image without windows needs no d_sharpness; its neighbour's refusal still comes
    msg = call(boxes=(None, wsc.boundaries([(0, 64, 0, 63)])), sharp=(None, 1 << 20))
    assert "image 1: window 0 " in msg, msg


def test_grid_entry_rejects_bad_arguments_before_touching_hip():
    L = _lib()

    def call(imgs=(4096, 8192), hs=(100, 100), ws=(200, 200), window=64, stride=64, sharp=(1 << 20, 2 << 20),
             var=None, n=None):
        rc = _maps(L, list(imgs), hs, ws, window, stride, None if sharp is None else list(sharp),
                   None if var is None else list(var), n)
        assert rc == -1
        msg = L.last_error()
        assert msg.startswith("phd_sharpness_maps_device: "), msg
        return msg

    assert "NULL argument" in call(sharp=None)
    assert "n_images" in call(n=0)
    assert "image 0: NULL image" in call(imgs=(None, 8192))
    for w in (0, 48, 256):
        assert "window must be 16, 32, 64 or 128" in call(window=w)
    for s in (0, -1):
        msg = call(stride=s)
        assert "stride must be positive" in msg and f"not {s}" in msg, msg
    assert "image 1: 100 x 50 is smaller than the window 64" in call(ws=(200, 50))
    assert "image 0: 100 x 200 is smaller than the window 128" in call(window=128)
    msg = call(sharp=(None, 2 << 20))
    assert "image 0: NULL d_sharpness for 3 windows" in msg, msg         # 100 x 200 at 64 / 64: 1 x 3
    # more than 2^31 - 1 windows: 46341^2 windows of 16 x 16 at stride 1
    big = 46340 + 16
    msg = call(imgs=(4096,), hs=(big,), ws=(big,), window=16, stride=1, sharp=(1 << 20,))
    assert "too many windows" in msg, msg
    # three grids of (2^31 - 16)^2 windows: their sum does not fit a long long; refused at the first
    top = 2147483647
    msg = call(imgs=(4096, 8192, 12288), hs=(top,) * 3, ws=(top,) * 3, window=16, stride=1,
               sharp=(1 << 20, 2 << 20, 3 << 20))
    assert "too many windows" in msg, msg
    # the running count is checked image by image: image 1's own defect is never reached
    msg = call(imgs=(4096, None), hs=(big, 100), ws=(big, 200), window=16, stride=1)
    assert "too many windows" in msg and "image 1" not in msg, msg


def test_python_wrappers_without_images_return_nothing():
    """No image: [] before any tensor or device is touched."""
    import photohive_dsp_amd as phd
    assert phd.sharpness_windows_device([], []) == [] and phd.sharpness_windows_device([], None, variance=True) == []
    assert phd.sharpness_maps_device([]) == [] and phd.sharpness_maps_device([], stride=0, variance=True) == []
    with pytest.raises(ValueError, match="windows has 1 entries for 0 images"):
        phd.sharpness_windows_device([], [None])


def test_a_call_without_windows_does_nothing_and_succeeds():
    """No window at all: 0 before any device work, so also without a device."""
    L = _lib()
    none = wsc.boundaries([])
    assert _lists(L, [4096, 8192], (100, 100), (200, 200), [None, none], 32, [None, None], None) == 0


def test_twin_rejects_bad_arguments():
    img = np.zeros((100, 200, 3), np.uint8)
    for boxes, window, what in (([(0, 64, 0, 65)], 64, "window 0 "), ([(0, 48, 0, 48)], 48, "16, 32, 64 or 128"),
                                ([(0, 128, 0, 128)], 128, "smaller than"), ([(40, 104, 0, 64)], 64, "leaves the")):
        msg = wsc.host_twin(img, boxes, window)
        assert isinstance(msg, str) and "phd_debug_window_sharpness_host" in msg and what in msg, (what, msg)
    L = _lib()
    cb = wsc.boundaries([(0, 16, 0, 16)])
    assert L.lib.phd_debug_window_sharpness_host(None, 100, 200, ctypes.byref(cb), 16, None, None, None) == -1
    assert L.lib.phd_debug_window_sharpness_host(img.ctypes.data, 100, 200, ctypes.byref(cb), 16, None, None,
                                                 None) == -1
    assert "NULL sharpness" in L.last_error()
    assert L.lib.phd_debug_window_sharpness_host(img.ctypes.data, 100, 200, None, 16, None, None, None) == 0


def test_host_twin_under_asan(tmp_path):
    """phd_sharpwin.cpp's host half and a C++ driver built with ASan + UBSan, run
    as their own process: heap images of exactly 3 H W bytes at each of the four
    sizes, windows flush with every edge."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "window_sharp_asan"
    src = [os.path.join(ROOT, "tests", "native", "window_sharp_asan.cpp"),
           os.path.join(ROOT, "photohive_dsp_amd", "csrc", "phd_sharpwin.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-DPHD_SHARPWIN_HOST_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", str(exe)] + src, check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "window sharpness host OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_window_call_plan_under_asan(tmp_path):
    """window_call.h alone and a C++ driver built with ASan + UBSan, run as their own
    process: the walk against window_grid's boxes for lists and grids, every refusal
    of the plan word for word, the counts at and far past 2^31 - 1 with no overflow
    report, and the twins' ladder."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "window_call_asan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "window_call_asan.cpp")], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "window call OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
