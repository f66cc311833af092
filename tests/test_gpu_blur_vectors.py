"""Blur vectors on the MI355X (blur_windows.hip: k_window_vectors<64>, <128>): the
window blur finished in the window's own block, ten Blur_Vectors and fft_max per
window left in device memory.

Bars: the vectors equal the compiled reference's fixtures exactly, and
phd_blur_windows_device's on the same windows exactly; fft_max is bit-identical to
that entry's; the host twin's vectors exactly; outputs and images sit inside
guarded tensors, the vectors at a base that is 4-byte but not 8-byte aligned, and
no byte outside 80 n and 8 n changes.  Upload helpers and guards are
tests/test_gpu_blur_windows.py's."""
import ctypes

import numpy as np
import pytest

from tests import blur_windows_cases as bwc
from tests.test_gpu_blur_windows import GUARD, _guards_intact, _launches, _stage, _upload
from tests.test_gpu_parity import _phd

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in bwc.manifest()}
VEC_OFF, MAX_OFF = 20, 24          # vectors: 4 (mod 8) past a 256-byte boundary; maxima: 8-byte aligned


class _Out:
    """The device outputs of one call, each inside a guarded tensor."""

    def __init__(self, torch, counts, no_vectors=(), no_maxima=()):
        self.counts = list(counts)
        self.vec, self.fmax = [], []
        for i, n in enumerate(self.counts):
            v = None if i in no_vectors else torch.full((80 * n + 64,), GUARD, dtype=torch.uint8, device="cuda")
            f = None if i in no_maxima else torch.full((8 * n + 64,), GUARD, dtype=torch.uint8, device="cuda")
            assert all(t is None or t.data_ptr() % 256 == 0 for t in (v, f))
            self.vec.append(v)
            self.fmax.append(f)

    def pointers(self):
        n = len(self.counts)
        pv = (ctypes.c_void_p * n)(*[None if v is None else v.data_ptr() + VEC_OFF for v in self.vec])
        pf = (ctypes.c_void_p * n)(*[None if f is None else f.data_ptr() + MAX_OFF for f in self.fmax])
        return pv, pf

    def results(self):
        """Per image (angles [n, 10], mags [n, 10], fft_max [n] or None); the guards are checked."""
        out = []
        for n, v, f in zip(self.counts, self.vec, self.fmax):
            ang, mag, fm = np.zeros((n, 10), np.int32), np.zeros((n, 10), np.float32), None
            if v is not None:
                h = v.cpu().numpy()
                assert (h[:VEC_OFF] == GUARD).all() and (h[VEC_OFF + 80 * n:] == GUARD).all(), "vector guards"
                w = h[VEC_OFF:VEC_OFF + 80 * n].copy().view(np.int32).reshape(n, 10, 2)
                ang, mag = w[..., 0].copy(), w[..., 1].copy().view(np.float32)
            if f is not None:
                h = f.cpu().numpy()
                assert (h[:MAX_OFF] == GUARD).all() and (h[MAX_OFF + 8 * n:] == GUARD).all(), "maxima guards"
                fm = h[MAX_OFF:MAX_OFF + 8 * n].copy().view(np.float64)
            out.append((ang, mag, fm))
        return out


def _cfg(**kw):
    from photohive_dsp_amd.core import WINDOW_DEFAULTS, make_config
    return make_config(**{**WINDOW_DEFAULTS, **kw})


def _enqueue(ptrs, shapes, box_lists, window, out, stream=None, **kw):
    """phd_blur_vectors_device through ctypes into out's tensors."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.structures import Crop_Boundaries
    n = len(ptrs)
    keep = [bwc.boundaries(b) if b is not None else None for b in box_lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * n)(*[ctypes.pointer(k) if k is not None else None for k in keep])
    pv, pf = out.pointers()
    rc = L.lib.phd_blur_vectors_device((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*[s[0] for s in shapes]),
                                       (ctypes.c_int * n)(*[s[1] for s in shapes]), n, arr, window,
                                       ctypes.byref(_cfg(**kw)), pv, pf, stream)
    assert rc == 0, L.last_error()


def _vectors(ptrs, shapes, box_lists, window, no_vectors=(), no_maxima=(), **kw):
    """One call on the library's stream: per image (angles, mags, fft_max)."""
    phd, L, torch = _phd()
    out = _Out(torch, [len(b) if b is not None else 0 for b in box_lists], no_vectors, no_maxima)
    _enqueue(ptrs, shapes, box_lists, window, out, **kw)
    return out.results()


def _same(got, old, what):
    """got: (angles, mags, fft_max) of the new entry; old: phd_blur_windows_device's (bins, angles, mags, fft_max)."""
    np.testing.assert_array_equal(got[0], old[1], err_msg=f"{what}: angles")
    np.testing.assert_array_equal(got[1].view(np.uint32), np.asarray(old[2], np.float32).view(np.uint32),
                                  err_msg=f"{what}: magnitudes")
    if got[2] is not None:
        np.testing.assert_array_equal(got[2].view(np.uint64), old[3].view(np.uint64), err_msg=f"{what}: fft_max bits")


def _bits(r):
    return np.concatenate([r[0].ravel().view(np.uint32), r[1].ravel().view(np.uint32)]), r[2].view(np.uint64)


def _raw(x):
    """The bytes of one window's row of an output (fft_max: a scalar)."""
    return np.atleast_1d(x).view(np.uint8)


def _twin(img, boxes, window, **kw):
    from tests.test_blur_vectors_host import _twin as twin
    got = twin(img, boxes, window, **kw)
    assert not isinstance(got, str), got
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_every_fixture_of_the_reference(name):
    phd, L, torch = _phd()
    case = CASES[name]
    fx = bwc.fixture(name)
    boxes = [tuple(int(v) for v in b) for b in fx["windows"]]
    img = bwc.case_image(case)
    ups = [_upload(torch, img, 3)]
    p = ups[0][1]
    (got,) = _vectors([p], [img.shape[:2]], [boxes], case["window"], **bwc.case_kw(case))
    (old,), _ = _stage([p], [img.shape[:2]], [boxes], case["window"], **bwc.case_kw(case))
    np.testing.assert_array_equal(got[0], fx["angles"], err_msg="angles against the reference")
    np.testing.assert_array_equal(got[1], np.asarray(fx["mags"], np.float32), err_msg="magnitudes against the reference")
    _same(got, old, name)
    np.testing.assert_allclose(got[2], fx["fft_max"], rtol=bwc.TIGHT_RTOL, atol=0)
    _guards_intact(ups)


@pytest.mark.parametrize("window", [64, 128])
def test_exact_size_images_at_every_base_phase(window):
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    T = window
    img = np.ascontiguousarray(synth.make("motion", T, T, 50 + T))
    boxes = [(0, T, 0, T)]
    ups = [_upload(torch, img, off) for off in range(4)]
    assert [p % 4 for _, p in ups] == [0, 1, 2, 3]
    res = _vectors([p for _, p in ups], [(T, T)] * 4, [boxes] * 4, T)
    twin = _twin(img, boxes, T)
    for off, r in enumerate(res):
        for a, b in zip(_bits(r), _bits(res[0])):
            np.testing.assert_array_equal(a, b, err_msg=f"base + {off}")
        np.testing.assert_array_equal(r[0], twin[0], err_msg=f"base + {off}: twin angles")
        np.testing.assert_array_equal(r[1], twin[1], err_msg=f"base + {off}: twin magnitudes")
        np.testing.assert_allclose(r[2], twin[2], rtol=bwc.TIGHT_RTOL, atol=0)
    (old,), _ = _stage([ups[0][1]], [(T, T)], [boxes], T)
    _same(res[0], old, "exact size")
    _guards_intact(ups)


def test_odd_width_every_column_phase_edges_overlaps_duplicates():
    """131 x 197: 3 W = 591 is no multiple of 4, so rows start at every phase."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    T, H, W = 64, 131, 197
    img = np.ascontiguousarray(synth.make("hblur", H, W, 61))
    lefts = [0, 1, 2, 3, W - T, W - T - 1, 5, 5, 20]               # every phase, the right edge, a duplicate, overlaps
    tops = [0, 1, 2, H - T, H - T, 0, 3, 3, 10]
    boxes = [(t, t + T, l, l + T) for t, l in zip(tops, lefts)]
    assert {b[2] % 4 for b in boxes} == {0, 1, 2, 3} and boxes[6] == boxes[7]
    assert any(b[0] == 0 for b in boxes) and any(b[2] == 0 for b in boxes)
    assert any(b[1] == H for b in boxes) and any(b[3] == W for b in boxes)
    ups = [_upload(torch, img, 1)]
    (got,) = _vectors([ups[0][1]], [(H, W)], [boxes], T)
    (old,), _ = _stage([ups[0][1]], [(H, W)], [boxes], T)
    _same(got, old, "131x197")
    for k in range(3):
        np.testing.assert_array_equal(_raw(got[k][6]), _raw(got[k][7]), err_msg="a duplicated window")
    _guards_intact(ups)


def test_one_call_over_images_of_different_sizes_null_list_null_outputs():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    T = 64
    shapes = [(64, 64), (131, 197), (200, 90), (77, 300), (90, 90)]
    imgs = [np.ascontiguousarray(synth.make(k, h, w, 70 + i))
            for i, (k, (h, w)) in enumerate(zip(("motion", "hblur", "uniform", "vblur", "motion"), shapes))]
    boxes = [[(0, 64, 0, 64)], [(1, 65, 2, 66), (67, 131, 133, 197), (30, 94, 64, 128)], None,
             [(13, 77, 236, 300), (0, 64, 0, 64)], []]
    ups = [_upload(torch, im, (k + 1) % 4) for k, im in enumerate(imgs)]
    ptrs = [p for _, p in ups]
    assert L.lib.phd_profile_kernels((1 << L.WINDOW_VECTORS_KERNEL) | (1 << L.WINDOW_BLUR_KERNEL)) == 0
    try:
        # image 2: a NULL list; image 4: N == 0 and a NULL d_vectors entry; image 1: no maxima wanted
        got = _vectors(ptrs, shapes, boxes, T, no_vectors=(4,), no_maxima=(1, 4))
        assert _launches(L, L.WINDOW_VECTORS_KERNEL) == 1, "every window of every image in one launch"
        assert _launches(L, L.WINDOW_BLUR_KERNEL) == 0
    finally:
        L.lib.phd_profile_kernels(0)
    assert got[1][2] is None and got[2][0].shape == (0, 10) and got[4][0].shape == (0, 10)
    for k, (b, g) in enumerate(zip(boxes, got)):
        if not b:
            continue
        (one,) = _vectors([ptrs[k]], [shapes[k]], [b], T)
        np.testing.assert_array_equal(g[0], one[0], err_msg=f"image {k}: angles")
        np.testing.assert_array_equal(g[1].view(np.uint32), one[1].view(np.uint32), err_msg=f"image {k}: magnitudes")
        if g[2] is not None:
            np.testing.assert_array_equal(g[2].view(np.uint64), one[2].view(np.uint64), err_msg=f"image {k}: fft_max")
        (old,), _ = _stage([ptrs[k]], [shapes[k]], [b], T)
        _same(one, old, f"image {k}")
    _guards_intact(ups)


@pytest.mark.parametrize("window", [64, 128])
def test_special_windows(window):
    phd, L, torch = _phd()
    T = window
    img = bwc.special_image()
    names = bwc.SPECIAL_TILES
    boxes = [(bwc.TILE * (k // 4), bwc.TILE * (k // 4) + T, bwc.TILE * (k % 4), bwc.TILE * (k % 4) + T)
             for k in range(8)]
    ups = [_upload(torch, img, 2)]
    (got,) = _vectors([ups[0][1]], [img.shape[:2]], [boxes], T)
    (old,), _ = _stage([ups[0][1]], [img.shape[:2]], [boxes], T)
    _same(got, old, f"special {T}")
    for k, name in enumerate(names):
        if name in ("black", "white", "colour"):
            assert not got[0][k].any() and not got[1][k].any(), name
    _guards_intact(ups)


def _explain(img, boxes, window, got, old, kw, mag_thresh=0.3):
    """The windows whose vectors differ, with the bin nearest to magnitude_thresh."""
    lines = []
    for k in range(len(boxes)):
        if (got[0][k] != old[1][k]).any() or (got[1][k].view(np.uint32) != old[2][k].view(np.uint32)).any():
            d = np.abs(old[0][k] - mag_thresh)
            a, r = np.unravel_index(int(np.argmin(d)), d.shape)
            lines.append(f"window {k} {boxes[k]}: new {got[0][k].tolist()} {got[1][k].tolist()} old "
                         f"{old[1][k].tolist()} {old[2][k].tolist()}; nearest bin [{a}][{r}] = {old[0][k][a, r]!r}, "
                         f"{d[a, r] / mag_thresh:.3e} relative from magnitude_thresh")
    return "\n".join(lines)


@pytest.mark.parametrize("window,count,seed,nr,na", [(64, 2000, 101, 16, 36), (128, 500, 102, 16, 36),
                                                      (64, 2000, 103, 8, 18)])
def test_many_windows_against_the_existing_entry(window, count, seed, nr, na):
    """(the count of windows with a non-zero magnitude is printed: at 16 x 36 only 3 of the 2000
    64-windows of this image have one, hence the 8 x 18 case, where 1083 do)"""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    T, H, W = window, 300, 333
    img = np.ascontiguousarray(synth.make("motion", H, W, 81))
    rng = np.random.default_rng(seed)
    tops, lefts = rng.integers(0, H - T + 1, count), rng.integers(0, W - T + 1, count)
    boxes = [(int(t), int(t) + T, int(l), int(l) + T) for t, l in zip(tops, lefts)]
    ups = [_upload(torch, img, 2)]
    p = ups[0][1]
    kw = dict(radius_partitions=nr, angle_partitions=na)
    (got,) = _vectors([p], [(H, W)], [boxes], T, **kw)
    (old,), _ = _stage([p], [(H, W)], [boxes], T, **kw)
    assert got[0].shape == (count, 10) and (got[2] > 0).all(), "no window is left out"
    why = _explain(img, boxes, T, got, old, kw)
    if why:
        print(why)
    print(f"{count} windows of {T} at {nr} x {na}: {int(np.count_nonzero(got[1].max(axis=1) > 0))} with a non-zero magnitude")
    _same(got, old, f"{count} windows of {T}")
    _guards_intact(ups)


@pytest.mark.parametrize("window,na", [(64, 2172), (64, 2173), (64, 2880), (128, 2880)])
def test_thousands_of_angle_bins(window, na):
    """One radius bin and more angle bins than threads: the per-angle phases take several rounds, and at
    T = 64 the totals and smoothed totals (16 na + 64 bytes) stop fitting the dead spectrum above 2172
    angle bins, where the launcher places them behind the bins."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    T, H, W = window, 140, 150
    img = np.ascontiguousarray(synth.make("motion", H, W, 5))
    boxes = [(0, T, 0, T), (5, 5 + T, 9, 9 + T), (H - T, H, W - T, W)]
    kw = dict(radius_partitions=1, angle_partitions=na, blur_cutoff_ratio_denom=1, magnitude_thresh=0.05)
    ups = [_upload(torch, img, 1)]
    p = ups[0][1]
    (got,) = _vectors([p], [(H, W)], [boxes], T, **kw)
    (old,), _ = _stage([p], [(H, W)], [boxes], T, **kw)
    twin = _twin(img, boxes, T, **kw)
    assert got[0].any(), "the grid gives vectors"
    np.testing.assert_array_equal(got[0], twin[0], err_msg="twin angles")
    np.testing.assert_array_equal(got[1], twin[1], err_msg="twin magnitudes")
    _same(got, old, f"{T} at 1 x {na}")
    _guards_intact(ups)


def _maps(ptrs, shapes, window, stride, grids, **kw):
    phd, L, torch = _phd()
    n = len(ptrs)
    out = _Out(torch, [g[0] * g[1] for g in grids])
    pv, pf = out.pointers()
    rc = L.lib.phd_blur_vector_maps_device((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*[s[0] for s in shapes]),
                                           (ctypes.c_int * n)(*[s[1] for s in shapes]), n, window, stride,
                                           ctypes.byref(_cfg(**kw)), pv, pf, None)
    assert rc == 0, L.last_error()
    return out.results()


@pytest.mark.parametrize("window,stride", [(128, 128), (128, 64), (64, 96), (64, 64)])
def test_grid_entry(window, stride):
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    H, W = 256, 390
    img = np.ascontiguousarray(synth.make("motion", H, W, 93))
    boxes, (gh, gw) = phd.window_grid(H, W, window, stride)
    assert (gh, gw) == ((H - window) // stride + 1, (W - window) // stride + 1) and len(boxes) == gh * gw > 1
    ups = [_upload(torch, img, 1)]
    p = ups[0][1]
    (grid,) = _maps([p], [(H, W)], window, stride, [(gh, gw)])
    (flat,) = _vectors([p], [(H, W)], [boxes], window)
    for a, b in zip(_bits(grid), _bits(flat)):
        np.testing.assert_array_equal(a, b, err_msg=f"grid {window} / {stride}")
    _guards_intact(ups)


def test_repeats_and_positions_give_identical_bits():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    T, H, W = 64, 200, 231
    img = np.ascontiguousarray(synth.make("dominant", H, W, 34))
    rng = np.random.default_rng(7)
    boxes = [(int(t), int(t) + T, int(l), int(l) + T)
             for t, l in zip(rng.integers(0, H - T + 1, 40), rng.integers(0, W - T + 1, 40))]
    probe = (78, 142, 13, 77)
    boxes[0] = boxes[20] = boxes[39] = probe
    ups = [_upload(torch, img, 3)]
    p = ups[0][1]
    runs = [_vectors([p], [(H, W)], [boxes], T)[0] for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(_bits(r), _bits(runs[0])):
            np.testing.assert_array_equal(a, b, err_msg="a repeated call")
    for k in (20, 39):
        for j in range(3):
            np.testing.assert_array_equal(_raw(runs[0][j][k]), _raw(runs[0][j][0]),
                                          err_msg=f"the same window at place {k}")
    (alone,) = _vectors([p], [(H, W)], [[probe]], T)
    for j in range(3):
        np.testing.assert_array_equal(_raw(alone[j][0]), _raw(runs[0][j][0]), err_msg="alone")


def test_two_calls_back_to_back_on_a_callers_stream():
    """No synchronisation between the calls: the second call's table (another window size, grid and
    window count) must not reach the pinned block while the first one's copy is still pending."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    H, W = 300, 333
    img = np.ascontiguousarray(synth.make("motion", H, W, 95))
    rng = np.random.default_rng(9)
    b1 = [(int(t), int(t) + 64, int(l), int(l) + 64)
          for t, l in zip(rng.integers(0, H - 63, 700), rng.integers(0, W - 63, 700))]
    b2 = [(int(t), int(t) + 128, int(l), int(l) + 128)
          for t, l in zip(rng.integers(0, H - 127, 90), rng.integers(0, W - 127, 90))]
    kw1, kw2 = dict(radius_partitions=16, angle_partitions=36), dict(radius_partitions=8, angle_partitions=18)
    ups = [_upload(torch, img, 0)]
    p = ups[0][1]
    want1 = _vectors([p], [(H, W)], [b1], 64, **kw1)
    want2 = _vectors([p], [(H, W)], [b2], 128, **kw2)
    o1, o2 = _Out(torch, [len(b1)]), _Out(torch, [len(b2)])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())                  # the image and the guard fills are done first
    _enqueue([p], [(H, W)], [b1], 64, o1, stream=s.cuda_stream, **kw1)
    _enqueue([p], [(H, W)], [b2], 128, o2, stream=s.cuda_stream, **kw2)
    s.synchronize()
    for got, want, what in ((o1.results(), want1, "first call"), (o2.results(), want2, "second call")):
        for a, b in zip(_bits(got[0]), _bits(want[0])):
            np.testing.assert_array_equal(a, b, err_msg=what)
    _guards_intact(ups)


def test_two_grid_calls_back_to_back_on_a_callers_stream():
    """The grid entry twice through the shared table call with no synchronisation between: 70 x 133
    (3 x 24 windows at 64 / 3) and 64 x 64 (its single window), then other images in the other order.
    Vectors: the host twin's exactly; fft_max: the bits of the same call on the library's stream."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    shapes, T, stride = [(70, 133), (64, 64)], 64, 3
    imgs = [[np.ascontiguousarray(synth.make(kind, h, w, seed)) for (h, w), seed in zip(shapes, seeds)]
            for kind, seeds in (("motion", (96, 97)), ("dominant", (98, 99)))]
    imgs[1].reverse()
    ups = [[_upload(torch, im, 1 + i) for i, im in enumerate(call)] for call in imgs]
    grids = [[phd.window_grid(*im.shape[:2], T, stride) for im in call] for call in imgs]
    assert [g[1] for g in grids[0]] == [(3, 24), (1, 1)]
    want = [_maps([u[1] for u in up], [im.shape[:2] for im in call], T, stride, [g[1] for g in gs])
            for call, up, gs in zip(imgs, ups, grids)]
    outs = [_Out(torch, [len(g[0]) for g in gs]) for gs in grids]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())                  # the images and the guard fills are done first
    for call, up, out in zip(imgs, ups, outs):
        pv, pf = out.pointers()
        rc = L.lib.phd_blur_vector_maps_device((ctypes.c_void_p * 2)(*[u[1] for u in up]),
                                               (ctypes.c_int * 2)(*[im.shape[0] for im in call]),
                                               (ctypes.c_int * 2)(*[im.shape[1] for im in call]), 2, T, stride,
                                               ctypes.byref(_cfg()), pv, pf, s.cuda_stream)
        assert rc == 0, L.last_error()
    s.synchronize()
    for c, (call, out) in enumerate(zip(imgs, outs)):
        for i, (im, got) in enumerate(zip(call, out.results())):
            twin = _twin(im, grids[c][i][0], T)
            np.testing.assert_array_equal(got[0], twin[0], err_msg=f"call {c} image {i}: twin angles")
            np.testing.assert_array_equal(got[1].view(np.uint32), twin[1].view(np.uint32),
                                          err_msg=f"call {c} image {i}: twin magnitudes")
            for a, b in zip(_bits(got), _bits(want[c][i])):
                np.testing.assert_array_equal(a, b, err_msg=f"call {c} image {i}")
    _guards_intact(ups[0] + ups[1])


def test_python_wrappers():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    img = np.ascontiguousarray(synth.make("motion", 300, 333, 91))
    t = torch.from_numpy(img).cuda()
    for window, stride in ((128, 64), (64, None)):
        (m,) = phd.blur_vector_maps_device([t], window=window, stride=stride)
        (old,) = phd.blur_map_device([t], window=window, stride=stride)
        gh, gw = old[3].shape
        assert tuple(m[0].shape) == (gh, gw, 10) and tuple(m[1].shape) == (gh, gw, 10) and tuple(m[2].shape) == (gh, gw)
        assert (m[0].dtype, m[1].dtype, m[2].dtype) == (torch.int32, torch.float32, torch.float64)
        assert all(x.is_cuda for x in m)
        assert m[1].data_ptr() == m[0].data_ptr() + 4 and m[0].stride() == m[1].stride() == (gw * 20, 20, 2)
        np.testing.assert_array_equal(m[0].cpu().numpy(), old[1])
        np.testing.assert_array_equal(m[1].cpu().numpy().view(np.uint32), old[2].view(np.uint32))
        np.testing.assert_array_equal(m[2].cpu().numpy().view(np.uint64), old[3].view(np.uint64))
        boxes, _ = phd.window_grid(300, 333, window, stride)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        r = phd.blur_vectors_device([t, t], [boxes, None], window=window, stream=s)
        s.synchronize()
        assert tuple(r[0][0].shape) == (len(boxes), 10) and tuple(r[0][2].shape) == (len(boxes),)
        assert tuple(r[1][0].shape) == (0, 10) and tuple(r[1][1].shape) == (0, 10) and tuple(r[1][2].shape) == (0,)
        assert torch.equal(r[0][0], m[0].reshape(-1, 10)) and torch.equal(r[0][2], m[2].reshape(-1))
        assert torch.equal(r[0][1].view(torch.int32), m[1].reshape(-1, 10).view(torch.int32))
    with pytest.raises(RuntimeError, match="at least 2"):
        phd.blur_vectors_device([t], [[(0, 64, 0, 64)]], window=64, angle_partitions=1)
    with pytest.raises(RuntimeError, match="stride must be positive"):
        phd.blur_vector_maps_device([t], window=64, stride=0)


def test_bin_counts_are_the_oracles():
    """tests/test_blur_vectors_host.py takes the bins' element counts from the C oracle, since
    phd_blur_counts needs a device: here they are shown to be phd_blur_counts(T, T, nr, na)."""
    phd, L, torch = _phd()
    from tests.test_blur_vectors_host import GRIDS, _counts
    for T, nr, na in GRIDS + [(64, 8, 2), (128, 16, 2)]:
        c = (ctypes.c_longlong * (na * nr))()
        assert L.lib.phd_blur_counts(T, T, nr, na, c) == 0, L.last_error()
        np.testing.assert_array_equal(np.array(c[:]).reshape(na, nr), _counts(T, nr, na), err_msg=str((T, nr, na)))
