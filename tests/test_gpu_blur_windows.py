"""Window blur on the MI355X (blur_windows.hip: k_window_blur<64>, <128>): every
fixture of the compiled reference, exact-size images at every base phase inside
guarded tensors, a 131 x 197 image (3 W no multiple of 4) with windows at every
column phase, touching the edges, overlapping and duplicated, one call over four
images with a NULL list, one launch in profile slot 14, bit-identical repeats,
2000 windows against the C oracle, the device against the host twin, and the
three Python entry points.

Bars: bins BINS_TIGHT_RTOL with atol 1e-13 and BINS_NORMWISE per window, vectors,
bin sizes and n_windows exact, fft_max TIGHT_RTOL (tests/test_gpu_parity.py); for
every device result the C oracle's vectorize of the device's bins equals the
device's vectors exactly."""
import ctypes
import functools

import numpy as np
import pytest

from tests import blur_windows_cases as bwc
from tests.test_gpu_parity import _phd

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in bwc.manifest()}
GUARD = 0xA5


def _upload(torch, img, off):
    """The image on the device `off` bytes past a 256-byte boundary inside a larger
    tensor whose other bytes are GUARD: (tensor, pointer)."""
    buf = torch.full((img.size + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    o = 16 + off
    buf[o:o + img.size] = torch.tensor(np.ascontiguousarray(img).reshape(-1), device="cuda")
    return buf, buf.data_ptr() + o


def _guards_intact(ups):
    for buf, _ in ups:
        h = buf.cpu().numpy()
        assert (h[:16] == GUARD).all() and (h[-44:] == GUARD).all()


def _stage(ptrs, shapes, box_lists, window, **kw):
    """phd_blur_windows_device through ctypes: per image (bins, angles, mags, fft_max) and the struct's
    (n_windows, na, nr, angle_bin_size, radius_bin_size)."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import WINDOW_DEFAULTS, make_config
    from photohive_dsp_amd.structures import Crop_Boundaries, PhdWindowBlur
    cfg = make_config(**{**WINDOW_DEFAULTS, **kw})
    n = len(ptrs)
    keep = [bwc.boundaries(b) if b is not None else None for b in box_lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * n)(*[ctypes.pointer(k) if k is not None else None for k in keep])
    wb = (PhdWindowBlur * n)()
    rc = L.lib.phd_blur_windows_device((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*[s[0] for s in shapes]),
                                       (ctypes.c_int * n)(*[s[1] for s in shapes]), n, arr, window, ctypes.byref(cfg),
                                       wb, None)
    assert rc == 0, L.last_error()
    na, nr = cfg.angle_partitions, cfg.radius_partitions
    meta = [(wb[i].n_windows, wb[i].num_angle_bins, wb[i].num_radius_bins, wb[i].angle_bin_size,
             wb[i].radius_bin_size) for i in range(n)]
    for i in range(n):                                        # one block: bins | fft_max | vectors
        if wb[i].n_windows:
            m = wb[i].n_windows
            base = ctypes.addressof(wb[i].bins.contents)
            assert ctypes.addressof(wb[i].fft_max.contents) == base + 8 * m * na * nr
            assert ctypes.addressof(wb[i].vectors.contents) == base + 8 * m * na * nr + 8 * m
        else:
            assert not wb[i].bins and not wb[i].vectors and not wb[i].fft_max
    from photohive_dsp_amd.core import _take_window_blur
    res = _take_window_blur(wb, n, na, nr)
    assert all(wb[i].n_windows == 0 and not wb[i].bins for i in range(n))
    return res, meta


def _launches(L, kernel):
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert L.lib.phd_profile_read(kernel, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    return cnt.value


def _bits(res):
    return np.concatenate([res[0].ravel().view(np.uint64), res[3].view(np.uint64)])


@functools.lru_cache(maxsize=None)
def _twin(name):
    case = CASES[name]
    fx = bwc.fixture(name)
    boxes = [tuple(int(v) for v in b) for b in fx["windows"]]
    img = bwc.case_image(case)
    got = bwc.host_twin(img, boxes, case["window"], **bwc.case_kw(case))
    assert not isinstance(got, str), got
    return img, boxes, got, fx


def _worst(got, want):
    return max([bwc.bins_errors(got[0][k], want[0][k])[0] for k in range(want[0].shape[0])] or [0.0])


@pytest.mark.parametrize("name", list(CASES))
def test_every_fixture_of_the_reference(name):
    phd, L, torch = _phd()
    case = CASES[name]
    img, boxes, twin, fx = _twin(name)
    buf, p = _upload(torch, img, 3)
    (got,), (meta,) = _stage([p], [img.shape[:2]], [boxes], case["window"], **bwc.case_kw(case))
    want = (fx["bins"], fx["angles"], fx["mags"], fx["fft_max"])
    print(f"{name}: device against the reference, bins normwise at worst {_worst(got, want):.3e}; "
          f"against the host twin {_worst(got, twin):.3e}")
    assert meta == (len(boxes), case["angle_partitions"], case["radius_partitions"], int(fx["angle_bin_size"]),
                    int(fx["radius_bin_size"]))
    bwc.assert_windows(got, want, name)
    bwc.assert_windows(got, twin, (name, "twin"))
    bwc.assert_vectors_follow_bins(got, name)


@pytest.mark.parametrize("window", [64, 128])
def test_exact_size_images_at_every_base_phase(window):
    """An image that is exactly one window, at device bases + 0 .. + 3 inside guarded
    tensors: the same bits at every phase, the twin's values, the guards untouched."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    T = window
    img = np.ascontiguousarray(synth.make("motion", T, T, 50 + T))
    boxes = [(0, T, 0, T)]
    ups = [_upload(torch, img, off) for off in range(4)]
    assert [p % 4 for _, p in ups] == [0, 1, 2, 3]
    res, _ = _stage([p for _, p in ups], [(T, T)] * 4, [boxes] * 4, T)
    twin = bwc.host_twin(img, boxes, T)
    for off, r in enumerate(res):
        np.testing.assert_array_equal(_bits(r), _bits(res[0]), err_msg=f"base + {off}")
        bwc.assert_windows(r, twin, f"base + {off}")
        bwc.assert_vectors_follow_bins(r, f"base + {off}")
    bwc.assert_windows(res[0], bwc.oracle_windows(img, boxes, 16, 36), "oracle")
    _guards_intact(ups)


@pytest.mark.parametrize("window", [64, 128])
def test_odd_width_every_column_phase_edges_overlaps_duplicates(window):
    """131 x 197: 3 W = 591 is no multiple of 4, so rows start at every phase."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    T, H, W = window, 131, 197
    img = np.ascontiguousarray(synth.make("hblur", H, W, 61))
    lefts = [0, 1, 2, 3, W - T, W - T - 1, 5, 5]                  # left = 0 1 2 3 (mod 4) among them; a duplicate
    tops = [0, 1, 2, H - T, H - T, 0, 3, 3]
    boxes = [(t, t + T, l, l + T) for t, l in zip(tops, lefts)]
    assert {b[2] % 4 for b in boxes} == {0, 1, 2, 3} and boxes[6] == boxes[7]
    assert any(b[1] == H for b in boxes) and any(b[3] == W for b in boxes)
    ups = [_upload(torch, img, 1)]
    (got,), _ = _stage([ups[0][1]], [(H, W)], [boxes], T)
    np.testing.assert_array_equal(got[0][6], got[0][7], err_msg="a duplicated window")
    bwc.assert_windows(got, bwc.oracle_windows(img, boxes, 16, 36), f"131x197 T={T}")
    bwc.assert_windows(got, bwc.host_twin(img, boxes, T), f"131x197 T={T} twin")
    bwc.assert_vectors_follow_bins(got, f"131x197 T={T}")
    _guards_intact(ups)


def test_four_images_one_null_list_one_launch_and_repeats():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    T = 64
    shapes = [(64, 64), (131, 197), (200, 90), (77, 300)]
    imgs = [np.ascontiguousarray(synth.make(k, h, w, 70 + i))
            for i, (k, (h, w)) in enumerate(zip(("motion", "hblur", "uniform", "vblur"), shapes))]
    boxes = [[(0, 64, 0, 64)], [(1, 65, 2, 66), (67, 131, 133, 197), (30, 94, 64, 128)], None,
             [(13, 77, 236, 300), (0, 64, 0, 64)]]
    ups = [_upload(torch, im, (k + 1) % 4) for k, im in enumerate(imgs)]
    ptrs = [p for _, p in ups]
    assert L.lib.phd_profile_kernels(1 << L.WINDOW_BLUR_KERNEL) == 0
    try:
        got, meta = _stage(ptrs, shapes, boxes, T)
        assert _launches(L, L.WINDOW_BLUR_KERNEL) == 1, "every window of every image in one launch"
    finally:
        L.lib.phd_profile_kernels(0)
    again, _ = _stage(ptrs, shapes, boxes, T)
    assert [m[0] for m in meta] == [1, 3, 0, 2]
    for k, (im, b, g, g2) in enumerate(zip(imgs, boxes, got, again)):
        if b is None:
            assert g[0].shape == (0, 36, 16) and g[1].shape == (0, 10) and g[3].shape == (0,)
            continue
        np.testing.assert_array_equal(_bits(g2), _bits(g), err_msg=f"image {k}: second run")
        np.testing.assert_array_equal(g2[1], g[1])
        np.testing.assert_array_equal(g2[2], g[2])
        bwc.assert_windows(g, bwc.oracle_windows(im, b, 16, 36), f"image {k}")
        bwc.assert_windows(g, bwc.host_twin(im, b, T), f"image {k} twin")
        bwc.assert_vectors_follow_bins(g, f"image {k}")
    _guards_intact(ups)


@functools.lru_cache(maxsize=None)
def _many():
    """2000 windows of 64 on one 353 x 350 image and the C oracle's values (computed once)."""
    from photohive_dsp_amd import synth
    img = np.ascontiguousarray(synth.make("motion", 353, 350, 81))
    rng = np.random.default_rng(82)
    tops, lefts = rng.integers(0, 353 - 64 + 1, 2000), rng.integers(0, 350 - 64 + 1, 2000)
    boxes = [(int(t), int(t) + 64, int(l), int(l) + 64) for t, l in zip(tops, lefts)]
    img.setflags(write=False)
    return img, boxes, bwc.oracle_windows(img, boxes, 8, 18)


def test_two_thousand_windows_against_the_c_oracle():
    phd, L, torch = _phd()
    img, boxes, want = _many()
    buf, p = _upload(torch, img, 2)
    assert L.lib.phd_profile_kernels(1 << L.WINDOW_BLUR_KERNEL) == 0
    try:
        (got,), _ = _stage([p], [img.shape[:2]], [boxes], 64, radius_partitions=8, angle_partitions=18)
        assert _launches(L, L.WINDOW_BLUR_KERNEL) == 1
    finally:
        L.lib.phd_profile_kernels(0)
    print(f"2000 windows: bins normwise at worst {_worst(got, want):.3e}, "
          f"{int(np.count_nonzero(want[2].max(axis=1) > 0))} with a non-zero magnitude")
    bwc.assert_windows(got, want, "2000 windows")
    bwc.assert_vectors_follow_bins(got, "2000 windows")


@pytest.mark.parametrize("window", [64, 128])
def test_special_patterns_on_the_device(window):
    phd, L, torch = _phd()
    T = window
    names = ("grey", "black", "white", "one_pixel", "one_pixel_255", "h_stripes", "v_stripes", "checkerboard")
    imgs = [np.ascontiguousarray(bwc.special_tile(n)) for n in names]
    boxes = [(0, T, 0, T), (128 - T, 128, 128 - T, 128)]
    ups = [_upload(torch, im, k % 4) for k, im in enumerate(imgs)]
    res, _ = _stage([p for _, p in ups], [(128, 128)] * len(imgs), [boxes] * len(imgs), T)
    for name, im, r in zip(names, imgs, res):
        bwc.assert_vectors_follow_bins(r, name)
        if name in ("grey", "black", "white", "one_pixel"):
            assert not r[0].any() and not r[1].any() and not r[2].any() and (r[3] < 1).all(), name
        elif name == "one_pixel_255":
            assert r[0].max() <= 1e-13 and r[0].min() >= 0.0
            np.testing.assert_allclose(r[3][0], 1.0, rtol=bwc.TIGHT_RTOL)
        else:
            bwc.assert_windows(r, bwc.oracle_windows(im, boxes, 16, 36), name)
            assert r[0].max() > 0.0


def test_python_entry_points():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    img = np.ascontiguousarray(synth.make("motion", 300, 400, 91))
    t = torch.from_numpy(img).cuda()
    boxes, (gh, gw) = phd.window_grid(300, 400, 128, 64)
    assert (gh, gw) == (3, 5) and len(boxes) == 15 and boxes[0] == (0, 128, 0, 128) and boxes[-1] == (128, 256, 256, 384)
    assert phd.window_grid(300, 400, 64) == ([(64 * y, 64 * y + 64, 64 * x, 64 * x + 64) for y in range(4)
                                               for x in range(6)], (4, 6))
    assert phd.window_grid(100, 400, 128) == ([], (0, 3))
    (flat,) = phd.blur_windows_device([t], [boxes], window=128)
    (grid,) = phd.blur_map_device(t[None], window=128, stride=64)
    assert grid[0].shape == (3, 5, 36, 16) and grid[1].shape == (3, 5, 10) and grid[2].shape == (3, 5, 10)
    assert grid[3].shape == (3, 5) and grid[0].dtype == np.float64 and grid[1].dtype == np.int32
    assert grid[2].dtype == np.float32
    for a, b in zip(flat, grid):
        np.testing.assert_array_equal(a, b.reshape(a.shape))
    bwc.assert_windows(flat, bwc.oracle_windows(img, boxes, 16, 36), "python")
    bwc.assert_vectors_follow_bins(flat, "python")
    # dict boxes, a Crop_Boundaries, None; another grid through kw
    d = [dict(top=b[0], bottom=b[1], left=b[2], right=b[3]) for b in boxes[:2]]
    r = phd.blur_windows_device([t, t, t], [d, phd.set_bounding_boxes(d), None], window=128, radius_partitions=8,
                                angle_partitions=18)
    assert r[0][0].shape == (2, 18, 8) and r[2][0].shape == (0, 18, 8)
    np.testing.assert_array_equal(r[0][0], r[1][0])
    bwc.assert_windows(r[0], bwc.oracle_windows(img, boxes[:2], 8, 18), "python 8x18")
    with pytest.raises(RuntimeError, match="window 0 "):
        phd.blur_windows_device([t], [[(0, 64, 0, 64)]], window=128)
    with pytest.raises(RuntimeError, match="outside the polar bin table"):
        phd.blur_map_device([t], window=64, radius_partitions=40, angle_partitions=72)
