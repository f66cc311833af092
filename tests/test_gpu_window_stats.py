"""Window statistics on the MI355X (window_stats.hip: k_window_stats<16>, <32>,
<64>, <128>): brightness, contrast and average saturation of every window, seven
doubles each, left in device memory by one launch.

Bars (tests/window_stats_cases.py: assert_device): brightness and S-bar bit for
bit the host twin's (phd_debug_window_stats_host, itself bit for bit the
definition in Python integers and doubles, tests/test_window_stats_host.py), the
contrasts by contrast_rule, and all seven against the reference's restatement at
the box statistics' bars on every window.  Images sit inside tensors whose other
bytes are 255, outputs inside 0xA5-guarded tensors, and no byte outside 56 n
changes."""
import ctypes

import numpy as np
import pytest

from tests import box_stats_cases as bsc
from tests import window_stats_cases as wtc
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
    """The device outputs of one call, each inside a guarded tensor; `null`: the
    images whose d_stats entry is NULL."""

    def __init__(self, torch, counts, null=()):
        self.counts = list(counts)
        self.bufs = [None if i in null else torch.full((56 * n + 64,), OUT_GUARD, dtype=torch.uint8, device="cuda")
                     for i, n in enumerate(self.counts)]
        assert all(t is None or t.data_ptr() % 256 == 0 for t in self.bufs)

    def pointers(self):
        return (ctypes.c_void_p * len(self.counts))(*[None if t is None else t.data_ptr() + OUT_OFF
                                                      for t in self.bufs])

    def results(self):
        """Per image [n, 7] or None; the guards are checked."""
        out = []
        for t, n in zip(self.bufs, self.counts):
            if t is None:
                out.append(None)
                continue
            h = t.cpu().numpy()
            assert (h[:OUT_OFF] == OUT_GUARD).all() and (h[OUT_OFF + 56 * n:] == OUT_GUARD).all(), "output guards"
            out.append(h[OUT_OFF:OUT_OFF + 56 * n].copy().view(np.float64).reshape(n, 7))
        return out


def _arrays(ptrs, shapes):
    n = len(ptrs)
    return ((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*[s[0] for s in shapes]),
            (ctypes.c_int * n)(*[s[1] for s in shapes]), n)


def _enqueue(ptrs, shapes, box_lists, window, out, stream=None):
    phd, L, torch = _phd()
    from photohive_dsp_amd.structures import Crop_Boundaries
    keep = [wtc.boundaries(b) if b is not None else None for b in box_lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * len(ptrs))(*[ctypes.pointer(k) if k is not None else None for k in keep])
    p, hs, ws, n = _arrays(ptrs, shapes)
    rc = L.lib.phd_stats_windows_device(p, hs, ws, n, arr, window, out.pointers(), stream)
    assert rc == 0, L.last_error()


def _enqueue_maps(ptrs, shapes, window, stride, out, stream=None):
    phd, L, torch = _phd()
    p, hs, ws, n = _arrays(ptrs, shapes)
    rc = L.lib.phd_stats_maps_device(p, hs, ws, n, window, stride, out.pointers(), stream)
    assert rc == 0, L.last_error()


def _windows(ptrs, shapes, box_lists, window, null=()):
    """One call on the library's stream: per image [n, 7]."""
    phd, L, torch = _phd()
    out = _Out(torch, [len(b) if b is not None else 0 for b in box_lists], null)
    _enqueue(ptrs, shapes, box_lists, window, out)
    return out.results()


def _maps(ptrs, shapes, window, stride, grids):
    phd, L, torch = _phd()
    out = _Out(torch, [g[0] * g[1] for g in grids])
    _enqueue_maps(ptrs, shapes, window, stride, out)
    return out.results()


# ---- 1 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", wtc.SIZES)
def test_odd_width_every_byte_phase_edges_overlaps_duplicates(T):
    """131 x 197: 3 W = 591 is no multiple of 4, so rows start at every phase."""
    phd, L, torch = _phd()
    img, boxes = wtc.odd_image(), wtc.odd_windows(T)
    ups = [_upload(torch, img, 1)]
    (got,) = _windows([ups[0][1]], [img.shape[:2]], [boxes], T)
    wtc.assert_device(img, boxes, got, f"131x197 at {T}")
    assert got[-1].tobytes() == got[-2].tobytes() == got[1].tobytes(), "a duplicated window"
    _guards_intact(ups)


# ---- 2 ---------------------------------------------------------------------------------------
def test_every_window_of_a_20_by_21_image_at_16():
    phd, L, torch = _phd()
    T, H, W = 16, 20, 21
    img = bsc.random_image(H, W, 31)
    boxes, (gh, gw) = phd.window_grid(H, W, T, 1)
    assert (gh, gw) == (5, 6)
    ups = [_upload(torch, img, 3)]
    (got,) = _windows([ups[0][1]], [(H, W)], [boxes], T)
    wtc.assert_device(img, boxes, got, "20x21")
    (grid,) = _maps([ups[0][1]], [(H, W)], T, 1, [(gh, gw)])
    wtc.same_bits(grid, got, "the grid entry at stride 1")
    _guards_intact(ups)


# ---- 3 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", wtc.SIZES)
def test_exact_size_images_at_every_base_phase(T):
    """The image is the window, at bases + 0, + 1, + 2 and + 3: a unit straddles every dword phase."""
    phd, L, torch = _phd()
    img = bsc.random_image(T, T, 50 + T)
    boxes = [(0, T, 0, T)]
    ups = [_upload(torch, img, off) for off in range(4)]
    assert [p % 4 for _, p in ups] == [0, 1, 2, 3]
    res = _windows([p for _, p in ups], [(T, T)] * 4, [boxes] * 4, T)
    for off, r in enumerate(res):
        wtc.assert_device(img, boxes, r, f"base + {off}", oracle=off == 0)
        wtc.same_bits(r, res[0], f"base + {off} against base + 0")
    _guards_intact(ups)


# ---- 4 ---------------------------------------------------------------------------------------
def test_one_call_over_four_images_null_list_one_launch():
    phd, L, torch = _phd()
    T = 32
    shapes = [(32, 32), (131, 197), (77, 300), (90, 41)]
    imgs = [bsc.random_image(h, w, 70 + i) for i, (h, w) in enumerate(shapes)]
    boxes = [[(0, 32, 0, 32)], [(1, 33, 2, 34), (99, 131, 165, 197), (30, 62, 64, 96), (30, 62, 65, 97)], None,
             [(58, 90, 9, 41), (0, 32, 0, 32), (7, 39, 3, 35), (7, 39, 3, 35), (29, 61, 5, 37)]]
    ups = [_upload(torch, im, (k + 1) % 4) for k, im in enumerate(imgs)]
    ptrs = [p for _, p in ups]
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert L.lib.phd_profile_kernels(1 << L.WINDOW_STATS_KERNEL) == 0
    try:
        got = _windows(ptrs, shapes, boxes, T, null=(2,))         # image 2: a NULL list and a NULL d_stats
        assert L.lib.phd_profile_read(L.WINDOW_STATS_KERNEL, ctypes.byref(tot), ctypes.byref(cnt)) == 0
        assert cnt.value == 1 and tot.value > 0, "every window of every image in one launch"
    finally:
        L.lib.phd_profile_kernels(0)
    assert got[2] is None
    again = _windows(ptrs, shapes, boxes, T, null=(2,))
    for k, (b, g, a) in enumerate(zip(boxes, got, again)):
        if not b:
            continue
        wtc.assert_device(imgs[k], b, g, f"image {k}")
        wtc.same_bits(a, g, f"image {k}: a second call")
    # the same window alone in its own call: the same 56 bytes
    (alone,) = _windows([ptrs[3]], [shapes[3]], [[boxes[3][2]]], T)
    assert alone[0].tobytes() == got[3][2].tobytes() == got[3][3].tobytes() and len(alone[0].tobytes()) == 56
    _guards_intact(ups)


# ---- 5 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", wtc.SIZES)
def test_grid_entry_is_the_list_entry_on_window_grid(T):
    phd, L, torch = _phd()
    H, W = 2 * T + 9, 3 * T + 2
    img = bsc.random_image(H, W, 93)
    ups = [_upload(torch, img, 2)]
    p = ups[0][1]
    for stride in (7, T):
        boxes, (gh, gw) = phd.window_grid(H, W, T, stride)
        assert len(boxes) == gh * gw > 1
        (grid,) = _maps([p], [(H, W)], T, stride, [(gh, gw)])
        (flat,) = _windows([p], [(H, W)], [boxes], T)
        wtc.same_bits(grid, flat, f"grid {T} / {stride}")
        if stride == T:
            wtc.assert_device(img, boxes, grid, f"grid {T} / {T}")
    _guards_intact(ups)


# ---- 6 ---------------------------------------------------------------------------------------
def test_calls_back_to_back_on_a_callers_stream():
    """No synchronisation between the calls: a later call's table (another window size and count)
    must not reach the pinned block while an earlier one's copy is still pending.  Two list calls,
    then two grid calls."""
    phd, L, torch = _phd()
    H, W = 150, 171
    img = bsc.random_image(H, W, 95)
    rng = np.random.default_rng(9)
    b1 = [(int(t), int(t) + 16, int(l), int(l) + 16)
          for t, l in zip(rng.integers(0, H - 15, 900), rng.integers(0, W - 15, 900))]
    b2 = [(int(t), int(t) + 128, int(l), int(l) + 128)
          for t, l in zip(rng.integers(0, H - 127, 70), rng.integers(0, W - 127, 70))]
    g3, s3 = phd.window_grid(H, W, 32, 5)
    g4, s4 = phd.window_grid(H, W, 64, 64)
    ups = [_upload(torch, img, 1)]
    p = ups[0][1]
    o1, o2, o3, o4 = (_Out(torch, [len(b)]) for b in (b1, b2, g3, g4))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())                  # the image and the guard fills are done first
    _enqueue([p], [(H, W)], [b1], 16, o1, stream=s.cuda_stream)
    _enqueue([p], [(H, W)], [b2], 128, o2, stream=s.cuda_stream)
    _enqueue_maps([p], [(H, W)], 32, 5, o3, stream=s.cuda_stream)
    _enqueue_maps([p], [(H, W)], 64, 64, o4, stream=s.cuda_stream)
    s.synchronize()
    for what, b, o in (("first list call", b1, o1), ("second list call", b2, o2), ("first grid call", g3, o3),
                       ("second grid call", g4, o4)):
        wtc.assert_device(img, b, o.results()[0], what, oracle=False)
    _guards_intact(ups)


# ---- 7 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", wtc.SIZES)
def test_special_windows(T):
    phd, L, torch = _phd()
    img, boxes = wtc.special_image(T)
    ups = [_upload(torch, img, 3)]
    (got,) = _windows([ups[0][1]], [img.shape[:2]], [boxes], T)
    wtc.assert_device(img, boxes, got, f"special {T}")
    wtc.assert_special_values(got, T)
    _guards_intact(ups)


# ---- 8 ---------------------------------------------------------------------------------------
def test_agreement_with_the_box_statistics_entry():
    """phd_box_stats_device on the same boxes: the same brightness and S-bar bit for
    bit, the contrasts by contrast_rule."""
    phd, L, torch = _phd()
    H, W = 150, 171
    img = bsc.random_image(H, W, 97)
    t = torch.from_numpy(np.array(img)).cuda()
    for T in wtc.SIZES:
        boxes = wtc.grid4(H, W, T)
        (box,) = phd.box_stats_device([t], [[dict(top=b[0], bottom=b[1], left=b[2], right=b[3]) for b in boxes]])
        (win,) = phd.stats_windows_device([t], [boxes], window=T)
        win = win.cpu().numpy()
        assert box.shape == win.shape == (len(boxes), 7)
        wtc.same_bits(win[:, :3], box[:, :3], f"brightness at {T}")
        wtc.same_bits(win[:, 6], box[:, 6], f"S-bar at {T}")
        wtc.contrast_rule(win, box, f"against box_stats_device at {T}")


# ---- 9 ---------------------------------------------------------------------------------------
def test_python_wrappers():
    phd, L, torch = _phd()
    H, W = 150, 171
    img = bsc.random_image(H, W, 91)
    t = torch.from_numpy(np.array(img)).cuda()
    for window, stride in ((16, None), (32, 20), (64, None), (128, 11)):
        boxes, (gh, gw) = phd.window_grid(H, W, window, stride)
        (m,) = phd.stats_maps_device([t], window=window, stride=stride)
        assert tuple(m.shape) == (gh, gw, 7) and m.dtype == torch.float64 and m.is_cuda
        wtc.assert_device(img, boxes, m.cpu().numpy(), f"map {window}", oracle=False)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        r = phd.stats_windows_device([t, t], [boxes, None], window=window, stream=st)
        st.synchronize()
        assert tuple(r[0].shape) == (len(boxes), 7) and tuple(r[1].shape) == (0, 7)
        assert r[1].dtype == torch.float64 and r[1].is_cuda
        assert torch.equal(r[0], m.reshape(-1, 7))
        (first,) = phd.stats_windows_device([t], [boxes[:3]], window=window)
        assert isinstance(first, torch.Tensor) and torch.equal(first, m.reshape(-1, 7)[:3])
    assert tuple(phd.stats_maps_device([t])[0].shape) == ((H - 64) // 64 + 1, (W - 64) // 64 + 1, 7)   # window 64
    (d,) = phd.stats_windows_device([t], [[(0, 64, 0, 64)]])                                            # window 64
    assert tuple(d.shape) == (1, 7)
    with pytest.raises(RuntimeError, match="16, 32, 64 or 128, not 48"):
        phd.stats_windows_device([t], [[(0, 48, 0, 48)]], window=48)
    with pytest.raises(RuntimeError, match="stride must be positive, not 0"):
        phd.stats_maps_device([t], window=64, stride=0)
