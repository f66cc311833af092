"""Window sharpness on the MI355X (window_sharp.hip: k_window_sharp<16>, <32>, <64>,
<128>): the Laplacian sharpness, and optionally the Laplacian's variance, of
every window left in device memory by one launch.

Bars: both outputs bit for bit the host twin's (phd_debug_window_sharpness_host,
itself bit for bit a Python big-integer restatement, tests/
test_window_sharpness_host.py), and the sharpness against oracle.sharpness at
FLOAT_RTOL and TIGHT_RTOL on every window (each has S1 > 0, asserted).  Images
sit inside tensors whose other bytes are 255, outputs inside guarded tensors, and
no byte outside 8 n changes."""
import ctypes
import math

import numpy as np
import pytest

from tests import window_sharp_cases as wsc
from tests.test_gpu_parity import _phd

pytestmark = pytest.mark.gpu

IMG_GUARD, OUT_GUARD = 255, 0xA5
OUT_OFF = 24                           # outputs: 8-byte aligned, 24 past a 256-byte boundary


def _upload(torch, img, off):
    """The image `off` bytes past a 256-byte boundary inside a tensor of 255s."""
    buf = torch.full((img.size + 64,), IMG_GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    o = 16 + off
    buf[o:o + img.size] = torch.tensor(np.ascontiguousarray(img).reshape(-1), device="cuda")
    return buf, buf.data_ptr() + o


def _guards_intact(ups):
    for buf, _ in ups:
        h = buf.cpu().numpy()
        assert (h[:16] == IMG_GUARD).all() and (h[-44:] == IMG_GUARD).all()


class _Out:
    """The device outputs of one call, each inside a guarded tensor.  variance:
    None (d_variance NULL), or the images that get one."""

    def __init__(self, torch, counts, variance=None, no_sharpness=()):
        self.counts = list(counts)
        self.want_var = variance is not None
        mk = lambda n: torch.full((8 * n + 64,), OUT_GUARD, dtype=torch.uint8, device="cuda")
        self.sharp = [None if i in no_sharpness else mk(n) for i, n in enumerate(self.counts)]
        self.var = [mk(n) if variance is not None and i in variance else None for i, n in enumerate(self.counts)]
        assert all(t is None or t.data_ptr() % 256 == 0 for t in self.sharp + self.var)

    def pointers(self):
        n = len(self.counts)
        ps = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() + OUT_OFF for t in self.sharp])
        pv = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() + OUT_OFF for t in self.var]) \
            if self.want_var else None
        return ps, pv

    @staticmethod
    def _take(t, n):
        if t is None:
            return None
        h = t.cpu().numpy()
        assert (h[:OUT_OFF] == OUT_GUARD).all() and (h[OUT_OFF + 8 * n:] == OUT_GUARD).all(), "output guards"
        return h[OUT_OFF:OUT_OFF + 8 * n].copy().view(np.float64)

    def results(self):
        """Per image (sharpness [n] or None, variance [n] or None); the guards are checked."""
        return [(self._take(s, n), self._take(v, n)) for n, s, v in zip(self.counts, self.sharp, self.var)]


def _enqueue(ptrs, shapes, box_lists, window, out, stream=None):
    phd, L, torch = _phd()
    from photohive_dsp_amd.structures import Crop_Boundaries
    n = len(ptrs)
    keep = [wsc.boundaries(b) if b is not None else None for b in box_lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * n)(*[ctypes.pointer(k) if k is not None else None for k in keep])
    ps, pv = out.pointers()
    rc = L.lib.phd_sharpness_windows_device((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*[s[0] for s in shapes]),
                                            (ctypes.c_int * n)(*[s[1] for s in shapes]), n, arr, window, ps, pv, stream)
    assert rc == 0, L.last_error()


def _windows(ptrs, shapes, box_lists, window, variance="all", no_sharpness=()):
    """One call on the library's stream: per image (sharpness, variance)."""
    phd, L, torch = _phd()
    if variance == "all":
        variance = range(len(ptrs))
    out = _Out(torch, [len(b) if b is not None else 0 for b in box_lists], variance, no_sharpness)
    _enqueue(ptrs, shapes, box_lists, window, out)
    return out.results()


def _maps(ptrs, shapes, window, stride, grids):
    phd, L, torch = _phd()
    n = len(ptrs)
    out = _Out(torch, [g[0] * g[1] for g in grids], range(n))
    ps, pv = out.pointers()
    rc = L.lib.phd_sharpness_maps_device((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*[s[0] for s in shapes]),
                                         (ctypes.c_int * n)(*[s[1] for s in shapes]), n, window, stride, ps, pv, None)
    assert rc == 0, L.last_error()
    return out.results()


def _twin(img, boxes, T):
    got = wsc.host_twin(img, boxes, T)
    assert not isinstance(got, str), got
    return got


def _same(got, want, what):
    np.testing.assert_array_equal(wsc.bits(got), wsc.bits(want), err_msg=what)


def _check(img, boxes, T, got, what, oracle=True):
    """got: (sharpness, variance) of the device against the twin (bits) and the oracle (both bars)."""
    s, v, u = _twin(img, boxes, T)
    _same(got[0], s, f"{what}: sharpness bits")
    if got[1] is not None:
        _same(got[1], v, f"{what}: variance bits")
    if oracle:
        wsc.assert_against_oracle(img, boxes, got[0], u)


@pytest.mark.parametrize("T", wsc.SIZES)
def test_odd_width_every_byte_phase_edges_overlaps_duplicates(T):
    """131 x 197: 3 W = 591 is no multiple of 4, so rows start at every phase."""
    phd, L, torch = _phd()
    img, boxes = wsc.odd_image(), wsc.odd_windows(T)
    ups = [_upload(torch, img, 1)]
    (got,) = _windows([ups[0][1]], [img.shape[:2]], [boxes], T)
    _check(img, boxes, T, got, f"131x197 at {T}")
    assert got[0][-1].tobytes() == got[0][-2].tobytes() == got[0][1].tobytes(), "a duplicated window"
    _guards_intact(ups)


def test_every_window_of_a_20_by_21_image_at_16():
    phd, L, torch = _phd()
    T, H, W = 16, 20, 21
    img = wsc.kind_image("structured", H, W, 31)
    boxes, (gh, gw) = phd.window_grid(H, W, T, 1)
    assert (gh, gw) == (5, 6)
    ups = [_upload(torch, img, 3)]
    (got,) = _windows([ups[0][1]], [(H, W)], [boxes], T)
    _check(img, boxes, T, got, "20x21")
    (grid,) = _maps([ups[0][1]], [(H, W)], T, 1, [(gh, gw)])
    _same(grid[0], got[0], "the grid entry at stride 1")
    _same(grid[1], got[1], "the grid entry at stride 1: variance")
    _guards_intact(ups)


@pytest.mark.parametrize("T", wsc.SIZES)
def test_exact_size_images_at_every_base_phase_and_the_optional_variance(T):
    """The image is the window: its first and last dwords reach into the 255s around
    it at bases + 1, + 2 and + 3.  d_variance NULL, all set and mixed."""
    phd, L, torch = _phd()
    img = wsc.kind_image("dominant", T, T, 50 + T)
    boxes = [(0, T, 0, T)]
    ups = [_upload(torch, img, off) for off in range(4)]
    assert [p % 4 for _, p in ups] == [0, 1, 2, 3]
    ptrs = [p for _, p in ups]
    res = _windows(ptrs, [(T, T)] * 4, [boxes] * 4, T)
    for off, r in enumerate(res):
        _check(img, boxes, T, r, f"base + {off}", oracle=off == 0)
    none = _windows(ptrs, [(T, T)] * 4, [boxes] * 4, T, variance=None)
    mixed = _windows(ptrs, [(T, T)] * 4, [boxes] * 4, T, variance=(1, 3))
    for off in range(4):
        assert none[off][1] is None and (mixed[off][1] is None) == (off in (0, 2))
        _same(none[off][0], res[0][0], f"no variance, base + {off}")
        _same(mixed[off][0], res[0][0], f"mixed variance, base + {off}")
        if mixed[off][1] is not None:
            _same(mixed[off][1], res[0][1], f"mixed variance, base + {off}: variance")
    _guards_intact(ups)


def test_one_call_over_four_images_null_list_null_variance_one_launch():
    phd, L, torch = _phd()
    T = 32
    shapes = [(32, 32), (131, 197), (77, 300), (90, 41)]
    kinds = ("uniform", "hblur", "grayish", "structured")
    imgs = [wsc.kind_image(k, h, w, 70 + i) for i, (k, (h, w)) in enumerate(zip(kinds, shapes))]
    boxes = [[(0, 32, 0, 32)], [(1, 33, 2, 34), (99, 131, 165, 197), (30, 62, 64, 96), (30, 62, 65, 97)], None,
             [(58, 90, 9, 41), (0, 32, 0, 32), (7, 39, 3, 35), (7, 39, 3, 35), (29, 61, 5, 37)]]
    ups = [_upload(torch, im, (k + 1) % 4) for k, im in enumerate(imgs)]
    ptrs = [p for _, p in ups]
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert L.lib.phd_profile_kernels(1 << L.WINDOW_SHARP_KERNEL) == 0
    try:
        # image 2: a NULL list and NULL outputs; image 1: a NULL d_variance entry
        got = _windows(ptrs, shapes, boxes, T, variance=(0, 3), no_sharpness=(2,))
        assert L.lib.phd_profile_read(L.WINDOW_SHARP_KERNEL, ctypes.byref(tot), ctypes.byref(cnt)) == 0
        assert cnt.value == 1 and tot.value > 0, "every window of every image in one launch"
    finally:
        L.lib.phd_profile_kernels(0)
    assert got[1][1] is None and got[2] == (None, None)
    again = _windows(ptrs, shapes, boxes, T, variance=(0, 3), no_sharpness=(2,))
    for k, (b, g, a) in enumerate(zip(boxes, got, again)):
        if not b:
            continue
        _check(imgs[k], b, T, g, f"image {k}")
        _same(a[0], g[0], f"image {k}: a second call")
        if g[1] is not None:
            _same(a[1], g[1], f"image {k}: a second call, variance")
    # the same window alone in its own call
    (alone,) = _windows([ptrs[3]], [shapes[3]], [[boxes[3][2]]], T)
    assert alone[0][0].tobytes() == got[3][0][2].tobytes() == got[3][0][3].tobytes()
    assert alone[1][0].tobytes() == got[3][1][2].tobytes()
    _guards_intact(ups)


@pytest.mark.parametrize("T", wsc.SIZES)
def test_grid_entry_is_the_list_entry_on_window_grid(T):
    phd, L, torch = _phd()
    H, W = 2 * T + 9, 3 * T + 2
    img = wsc.kind_image("structured", H, W, 93)
    ups = [_upload(torch, img, 2)]
    p = ups[0][1]
    for stride in (7, T):
        boxes, (gh, gw) = phd.window_grid(H, W, T, stride)
        assert len(boxes) == gh * gw > 1
        (grid,) = _maps([p], [(H, W)], T, stride, [(gh, gw)])
        (flat,) = _windows([p], [(H, W)], [boxes], T)
        _same(grid[0], flat[0], f"grid {T} / {stride}")
        _same(grid[1], flat[1], f"grid {T} / {stride}: variance")
        if stride == T:
            _check(img, boxes, T, grid, f"grid {T} / {T}")
    _guards_intact(ups)


def test_two_calls_back_to_back_on_a_callers_stream():
    """No synchronisation between the calls: the second call's table (another window size and count)
    must not reach the pinned block while the first one's copy is still pending."""
    phd, L, torch = _phd()
    H, W = 150, 171
    img = wsc.kind_image("uniform", H, W, 95)
    rng = np.random.default_rng(9)
    b1 = [(int(t), int(t) + 16, int(l), int(l) + 16)
          for t, l in zip(rng.integers(0, H - 15, 900), rng.integers(0, W - 15, 900))]
    b2 = [(int(t), int(t) + 128, int(l), int(l) + 128)
          for t, l in zip(rng.integers(0, H - 127, 70), rng.integers(0, W - 127, 70))]
    ups = [_upload(torch, img, 1)]
    p = ups[0][1]
    o1, o2 = _Out(torch, [len(b1)], (0,)), _Out(torch, [len(b2)], (0,))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())                  # the image and the guard fills are done first
    _enqueue([p], [(H, W)], [b1], 16, o1, stream=s.cuda_stream)
    _enqueue([p], [(H, W)], [b2], 128, o2, stream=s.cuda_stream)
    s.synchronize()
    _check(img, b1, 16, o1.results()[0], "first call", oracle=False)
    _check(img, b2, 128, o2.results()[0], "second call", oracle=False)
    _guards_intact(ups)


def test_two_grid_calls_back_to_back_on_a_callers_stream():
    """The grid entry twice through the shared table call with no synchronisation between: 70 x 133
    (3 x 24 windows at 64 / 3) and 64 x 64 (its single window), then other images in the other order."""
    phd, L, torch = _phd()
    shapes, T, stride = [(70, 133), (64, 64)], 64, 3
    imgs = [[wsc.kind_image(kind, h, w, seed) for (h, w), seed in zip(shapes, seeds)]
            for kind, seeds in (("uniform", (96, 97)), ("structured", (98, 99)))]
    imgs[1].reverse()
    ups = [[_upload(torch, im, 1 + i) for i, im in enumerate(call)] for call in imgs]
    grids = [[phd.window_grid(*im.shape[:2], T, stride) for im in call] for call in imgs]
    assert [g[1] for g in grids[0]] == [(3, 24), (1, 1)]
    outs = [_Out(torch, [len(g[0]) for g in call], range(2)) for call in grids]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())                  # the images and the guard fills are done first
    for call, up, out in zip(imgs, ups, outs):
        ps, pv = out.pointers()
        rc = L.lib.phd_sharpness_maps_device((ctypes.c_void_p * 2)(*[u[1] for u in up]),
                                             (ctypes.c_int * 2)(*[im.shape[0] for im in call]),
                                             (ctypes.c_int * 2)(*[im.shape[1] for im in call]), 2, T, stride, ps, pv,
                                             s.cuda_stream)
        assert rc == 0, L.last_error()
    s.synchronize()
    for c, (call, out) in enumerate(zip(imgs, outs)):
        for i, (im, got) in enumerate(zip(call, out.results())):
            _check(im, grids[c][i][0], T, got, f"call {c} image {i}", oracle=False)
    _guards_intact(ups[0] + ups[1])


@pytest.mark.parametrize("T", wsc.SIZES)
def test_special_windows(T):
    phd, L, torch = _phd()
    img = np.full((T + 9, len(wsc.SPECIALS) * (T + 3) + 4, 3), 255, np.uint8)
    boxes = []
    for k, name in enumerate(wsc.SPECIALS):
        l = 3 + k * (T + 3)
        img[4:4 + T, l:l + T] = wsc.special_window(name, T)
        boxes.append((4, 4 + T, l, l + T))
    ups = [_upload(torch, img, 3)]
    (got,) = _windows([ups[0][1]], [img.shape[:2]], [boxes], T)
    _check(img, boxes, T, got, f"special {T}", oracle=False)
    by = dict(zip(wsc.SPECIALS, zip(*got)))
    assert math.isnan(by["black"][0]) and by["black"][1] == 0.0
    assert by["black_ring"][0] == math.inf and by["black_ring"][1] > 0
    finite = [k for k, name in enumerate(wsc.SPECIALS) if name in ("grey", "white", "corner")]
    s, v, u = _twin(img, [boxes[k] for k in finite], T)
    wsc.assert_against_oracle(img, [boxes[k] for k in finite], got[0][finite], u)
    _guards_intact(ups)


def test_python_wrappers():
    phd, L, torch = _phd()
    H, W = 150, 171
    img = wsc.kind_image("structured", H, W, 91)
    t = torch.from_numpy(np.array(img)).cuda()
    for window, stride in ((16, None), (32, 20), (64, None), (128, 11)):
        boxes, (gh, gw) = phd.window_grid(H, W, window, stride)
        s_ref, v_ref, _ = _twin(img, boxes, window)
        (m,) = phd.sharpness_maps_device([t], window=window, stride=stride)
        assert tuple(m.shape) == (gh, gw) and m.dtype == torch.float64 and m.is_cuda
        _same(m.cpu().numpy().reshape(-1), s_ref, f"map {window}")
        ((ms, mv),) = phd.sharpness_maps_device([t], window=window, stride=stride, variance=True)
        assert tuple(ms.shape) == tuple(mv.shape) == (gh, gw) and mv.dtype == torch.float64 and mv.is_cuda
        assert torch.equal(ms, m)
        _same(mv.cpu().numpy().reshape(-1), v_ref, f"map {window}: variance")
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        r = phd.sharpness_windows_device([t, t], [boxes, None], window=window, variance=True, stream=st)
        st.synchronize()
        assert tuple(r[0][0].shape) == tuple(r[0][1].shape) == (len(boxes),)
        assert tuple(r[1][0].shape) == tuple(r[1][1].shape) == (0,) and r[1][0].dtype == torch.float64
        assert torch.equal(r[0][0], m.reshape(-1)) and torch.equal(r[0][1], mv.reshape(-1))
        (plain,) = phd.sharpness_windows_device([t], [boxes[:3]], window=window)
        assert isinstance(plain, torch.Tensor) and torch.equal(plain, m.reshape(-1)[:3])
    assert tuple(phd.sharpness_maps_device([t])[0].shape) == ((H - 64) // 64 + 1, (W - 64) // 64 + 1)   # window 64
    with pytest.raises(RuntimeError, match="16, 32, 64 or 128"):
        phd.sharpness_windows_device([t], [[(0, 48, 0, 48)]], window=48)
    with pytest.raises(RuntimeError, match="stride must be positive"):
        phd.sharpness_maps_device([t], window=64, stride=0)
