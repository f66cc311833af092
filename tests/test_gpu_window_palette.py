"""Window palettes on the MI355X (window_palette.hip: k_window_palette<16>, <32>,
<64>, <128>): the palette slot counts and the dominant slot of every window of a
label map, left in device memory by one launch.

Bar: counts and dominant equal the host twin's (phd_debug_window_palette_host,
itself numpy's and the box twin's, tests/test_window_palette_host.py) and numpy's
(tests/box_palette_cases.expected_counts, window_palette_cases.expected_dominant),
integer for integer, on every window.  Maps sit inside tensors of 0xFFFF at bases
+ 0, 2, 4 and 6 bytes, the counts inside 0xA5-guarded tensors at a 4-byte-odd
offset and the dominant labels at a 2-byte-odd one; the guards are checked after
every call."""
import ctypes

import numpy as np
import pytest

from tests import box_palette_cases as bpc
from tests import window_palette_cases as wpc
from tests.test_gpu_parity import _phd

pytestmark = pytest.mark.gpu

OUT_GUARD = 0xA5
C_OFF, D_OFF = 20, 18                  # counts: 4 mod 8 bytes past a 256-byte boundary; dominant: 2 mod 4
LEAD = 8                               # guard labels in front of a map


def _upload(torch, lab, elems):
    """The map 2 * elems bytes past an 8-byte boundary inside a tensor of 0xFFFF."""
    buf = torch.full((lab.size + 32,), -1, dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 256 == 0
    o = LEAD + elems
    buf[o:o + lab.size] = torch.from_numpy(np.ascontiguousarray(lab).view(np.int16).reshape(-1)).cuda()
    return buf, buf.data_ptr() + 2 * o, o, lab.size


def _guards_intact(ups):
    for buf, _, o, size in ups:
        h = buf.cpu().numpy()
        assert (h[:o] == -1).all() and (h[o + size:] == -1).all(), "the bytes around a map"


class _Out:
    """The device outputs of one call, each inside a guarded tensor.  want[i]: which
    of "c" (counts) and "d" (dominant) map i gets -- "" for NULL entries."""

    def __init__(self, torch, n_windows, ns, want=None):
        self.n, self.ns = list(n_windows), list(ns)
        self.want = list(want) if want is not None else ["cd"] * len(self.n)
        self.cb = [torch.full((4 * n * (s + 1) + 64,), OUT_GUARD, dtype=torch.uint8, device="cuda")
                   if "c" in w else None for n, s, w in zip(self.n, self.ns, self.want)]
        self.db = [torch.full((2 * n + 64,), OUT_GUARD, dtype=torch.uint8, device="cuda") if "d" in w else None
                   for n, w in zip(self.n, self.want)]
        assert all(t is None or t.data_ptr() % 256 == 0 for t in self.cb + self.db)

    def pointers(self):
        k = len(self.n)
        pc = (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() + C_OFF for t in self.cb])
        pd = (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() + D_OFF for t in self.db])
        return (pc if any(t is not None for t in self.cb) else None,
                pd if any(t is not None for t in self.db) else None)

    def results(self):
        """Per map (counts [n, n_slots + 1] or None, dominant [n] or None); the guards are checked."""
        out = []
        for n, s, tc, td in zip(self.n, self.ns, self.cb, self.db):
            c = d = None
            if tc is not None:
                h, nb = tc.cpu().numpy(), 4 * n * (s + 1)
                assert (h[:C_OFF] == OUT_GUARD).all() and (h[C_OFF + nb:] == OUT_GUARD).all(), "counts guards"
                c = h[C_OFF:C_OFF + nb].copy().view(np.uint32).reshape(n, s + 1)
            if td is not None:
                h, nb = td.cpu().numpy(), 2 * n
                assert (h[:D_OFF] == OUT_GUARD).all() and (h[D_OFF + nb:] == OUT_GUARD).all(), "dominant guards"
                d = h[D_OFF:D_OFF + nb].copy().view(np.uint16)
            out.append((c, d))
        return out


def _arrays(ptrs, shapes, ns):
    n = len(ptrs)
    return ((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*[s[0] for s in shapes]),
            (ctypes.c_int * n)(*[s[1] for s in shapes]), n, (ctypes.c_int * n)(*ns))


def _enqueue(ptrs, shapes, ns, box_lists, T, out, stream=None):
    phd, L, torch = _phd()
    from photohive_dsp_amd.structures import Crop_Boundaries
    keep = [wpc.boundaries(b) if b is not None else None for b in box_lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * len(ptrs))(*[ctypes.pointer(k) if k is not None else None for k in keep])
    p, hs, ws, n, nsa = _arrays(ptrs, shapes, ns)
    pc, pd = out.pointers()
    rc = L.lib.phd_palette_windows_device(p, hs, ws, n, nsa, arr, T, pc, pd, stream)
    assert rc == 0, L.last_error()


def _enqueue_maps(ptrs, shapes, ns, T, stride, out, stream=None):
    phd, L, torch = _phd()
    p, hs, ws, n, nsa = _arrays(ptrs, shapes, ns)
    pc, pd = out.pointers()
    rc = L.lib.phd_palette_maps_device(p, hs, ws, n, nsa, T, stride, pc, pd, stream)
    assert rc == 0, L.last_error()


def _windows(ptrs, shapes, ns, box_lists, T, want=None):
    """One list call on the library's stream: per map (counts, dominant)."""
    phd, L, torch = _phd()
    out = _Out(torch, [len(b) if b is not None else 0 for b in box_lists], ns, want)
    _enqueue(ptrs, shapes, ns, box_lists, T, out)
    return out.results()


def _maps(ptrs, shapes, ns, T, stride, grids, want=None):
    phd, L, torch = _phd()
    out = _Out(torch, [g[0] * g[1] for g in grids], ns, want)
    _enqueue_maps(ptrs, shapes, ns, T, stride, out)
    return out.results()


def _assert_device(lab, boxes, n_slots, T, got, what=""):
    """Counts and dominant (where present) against the host twin and numpy, every window."""
    c, d = got
    want_c, want_d = wpc.expected(lab, boxes, n_slots)
    twin = wpc.host_twin(np.ascontiguousarray(lab), boxes, n_slots, T)
    assert not isinstance(twin, str), twin
    assert np.array_equal(twin[0], want_c) and np.array_equal(twin[1], want_d), what
    if c is not None:
        assert c.shape == want_c.shape and np.array_equal(c, want_c), what
        assert (c.sum(axis=1, dtype=np.int64) == T * T).all(), what
    if d is not None:
        assert d.shape == want_d.shape and np.array_equal(d, want_d), what


# ---- the 131 x 197 map ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", wpc.SIZES)
def test_odd_width_every_phase_edges_overlaps_duplicates(T):
    phd, L, torch = _phd()
    lab, boxes = wpc.odd_map(), wpc.odd_windows(T)
    ups = [_upload(torch, lab, 1)]
    (got,) = _windows([ups[0][1]], [lab.shape], [17], [boxes], T)
    _assert_device(lab, boxes, 17, T, got, f"131x197 at {T}")
    assert got[0][-1].tobytes() == got[0][-2].tobytes() == got[0][1].tobytes(), "a duplicated window"
    _guards_intact(ups)


# ---- every window of a small map, both entries ------------------------------------------------------
def test_every_window_of_a_20_by_21_map_at_16():
    phd, L, torch = _phd()
    T, H, W = 16, 20, 21
    lab = bpc.random_map(H, W, 17, 31)
    boxes, (gh, gw) = phd.window_grid(H, W, T, 1)
    assert (gh, gw) == (5, 6) and boxes == wpc.all_windows(T, H, W)
    ups = [_upload(torch, lab, 3)]
    (got,) = _windows([ups[0][1]], [(H, W)], [17], [boxes], T)
    _assert_device(lab, boxes, 17, T, got, "20x21")
    (grid,) = _maps([ups[0][1]], [(H, W)], [17], T, 1, [(gh, gw)])
    assert np.array_equal(grid[0], got[0]) and np.array_equal(grid[1], got[1]), "the grid entry at stride 1"
    _guards_intact(ups)


# ---- T x T maps at the four bases ---------------------------------------------------------------------
@pytest.mark.parametrize("T", wpc.SIZES)
def test_exact_size_maps_at_every_base_phase(T):
    phd, L, torch = _phd()
    lab = bpc.random_map(T, T, 17, 50 + T)
    boxes = [(0, T, 0, T)]
    ups = [_upload(torch, lab, e) for e in range(4)]
    assert [p % 8 for _, p, _, _ in ups] == [0, 2, 4, 6]
    res = _windows([p for _, p, _, _ in ups], [(T, T)] * 4, [17] * 4, [boxes] * 4, T)
    for e, r in enumerate(res):
        _assert_device(lab, boxes, 17, T, r, f"base + {2 * e}")
    _guards_intact(ups)


# ---- slot-count edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots", wpc.SLOT_EDGES)
def test_slot_count_edges(n_slots):
    phd, L, torch = _phd()
    lab = bpc.random_map(140, 150, n_slots, 900 + n_slots)
    ups = [_upload(torch, lab, 1)]
    for T in (16, 128):
        boxes = wpc.edge_windows(T, 140, 150)
        (got,) = _windows([ups[0][1]], [lab.shape], [n_slots], [boxes], T)
        _assert_device(lab, boxes, n_slots, T, got, f"{n_slots} slots at {T}")
    _guards_intact(ups)


# ---- special windows --------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", wpc.SIZES)
def test_special_windows(T):
    phd, L, torch = _phd()
    lab, boxes, ns, doms = wpc.special_map(T)
    ups = [_upload(torch, lab, 2)]
    (got,) = _windows([ups[0][1]], [lab.shape], [ns], [boxes], T)
    _assert_device(lab, boxes, ns, T, got, f"special {T}")
    assert np.array_equal(got[1], doms)
    (zero,) = _windows([ups[0][1]], [lab.shape], [0], [boxes], T)
    _assert_device(lab, boxes, 0, T, zero, f"special {T}, no slots")
    assert (zero[0] == T * T).all() and (zero[1] == wpc.NONE).all()
    _guards_intact(ups)


# ---- a block's last waves without a window --------------------------------------------------------------
@pytest.mark.parametrize("T", (16, 32))
@pytest.mark.parametrize("count", (1, 5))
def test_window_counts_that_leave_waves_idle(T, count):
    phd, L, torch = _phd()
    lab = bpc.random_map(70, 81, 17, 60 + count)
    boxes = wpc.edge_windows(T, 70, 81)[3:3 + count]
    assert len(boxes) == count
    ups = [_upload(torch, lab, 3)]
    (got,) = _windows([ups[0][1]], [lab.shape], [17], [boxes], T)
    _assert_device(lab, boxes, 17, T, got, f"{count} windows of {T}")
    _guards_intact(ups)


# ---- one call over four maps -----------------------------------------------------------------------------
@pytest.mark.parametrize("T", (32, 64))
def test_one_call_over_four_maps_mixed_palettes_one_launch(T):
    phd, L, torch = _phd()
    shapes = [(T, T), (131, 197), (77, 300), (90, 141)]
    ns = [0, 3, 17, 4096]
    labs = [bpc.random_map(h, w, s, 70 + i) for i, ((h, w), s) in enumerate(zip(shapes, ns))]
    boxes = [[(0, T, 0, T)], None, wpc.edge_windows(T, 77, 300)[:6], wpc.edge_windows(T, 90, 141)]
    want = ["c", "", "d", "cd"]                               # map 1: a NULL list and NULL outputs
    ups = [_upload(torch, lab, (k + 1) % 4) for k, lab in enumerate(labs)]
    ptrs = [p for _, p, _, _ in ups]
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert L.lib.phd_profile_kernels(1 << L.WINDOW_PALETTE_KERNEL) == 0
    try:
        got = _windows(ptrs, shapes, ns, boxes, T, want)
        assert L.lib.phd_profile_read(L.WINDOW_PALETTE_KERNEL, ctypes.byref(tot), ctypes.byref(cnt)) == 0
        assert cnt.value == 1 and tot.value > 0, "every window of every map in one launch"
    finally:
        L.lib.phd_profile_kernels(0)
    assert got[1] == (None, None) and got[0][1] is None and got[2][0] is None
    again = _windows(ptrs, shapes, ns, boxes, T, want)
    for k, (b, g, a) in enumerate(zip(boxes, got, again)):
        if not b:
            continue
        _assert_device(labs[k], b, ns[k], T, g, f"map {k}")
        for x, y in zip(g, a):
            assert (x is None and y is None) or x.tobytes() == y.tobytes(), f"map {k}: a second call"
    # the same window alone in its own call: the same bytes
    (alone,) = _windows([ptrs[3]], [shapes[3]], [4096], [[boxes[3][2]]], T)
    assert alone[0][0].tobytes() == got[3][0][2].tobytes() and alone[1][0] == got[3][1][2]
    assert len(alone[0][0].tobytes()) == 4 * 4097
    _guards_intact(ups)


# ---- the grid entry against the list entry ------------------------------------------------------------------
@pytest.mark.parametrize("T", wpc.SIZES)
def test_grid_entry_is_the_list_entry_on_window_grid(T):
    phd, L, torch = _phd()
    H, W = 2 * T + 9, 3 * T + 2
    lab = bpc.random_map(H, W, 17, 93)
    ups = [_upload(torch, lab, 2)]
    p = ups[0][1]
    for stride in (7, T):
        boxes, (gh, gw) = phd.window_grid(H, W, T, stride)
        assert len(boxes) == gh * gw > 1
        (grid,) = _maps([p], [(H, W)], [17], T, stride, [(gh, gw)])
        (flat,) = _windows([p], [(H, W)], [17], [boxes], T)
        assert np.array_equal(grid[0], flat[0]) and np.array_equal(grid[1], flat[1]), f"grid {T} / {stride}"
        _assert_device(lab, boxes, 17, T, grid, f"grid {T} / {stride}")
    _guards_intact(ups)


# ---- calls back to back ---------------------------------------------------------------------------------------
def test_calls_back_to_back_on_a_callers_stream():
    """No synchronisation between the calls: a later call's table (another window size, count and
    palette) must not reach the pinned block while an earlier one's copy is still pending.  Two
    list calls, then two grid calls."""
    phd, L, torch = _phd()
    H, W = 150, 171
    lab = bpc.random_map(H, W, 127, 95)
    rng = np.random.default_rng(9)
    b1 = [(int(t), int(t) + 16, int(l), int(l) + 16)
          for t, l in zip(rng.integers(0, H - 15, 900), rng.integers(0, W - 15, 900))]
    b2 = [(int(t), int(t) + 128, int(l), int(l) + 128)
          for t, l in zip(rng.integers(0, H - 127, 70), rng.integers(0, W - 127, 70))]
    g3, s3 = phd.window_grid(H, W, 32, 5)
    g4, s4 = phd.window_grid(H, W, 64, 64)
    ups = [_upload(torch, lab, 1)]
    p = ups[0][1]
    slots = (127, 4096, 17, 127)                              # (labels >= 17 count as none in the third call)
    o1, o2, o3, o4 = (_Out(torch, [len(b)], [s]) for b, s in zip((b1, b2, g3, g4), slots))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())                # the map and the guard fills are done first
    _enqueue([p], [(H, W)], [slots[0]], [b1], 16, o1, stream=s.cuda_stream)
    _enqueue([p], [(H, W)], [slots[1]], [b2], 128, o2, stream=s.cuda_stream)
    _enqueue_maps([p], [(H, W)], [slots[2]], 32, 5, o3, stream=s.cuda_stream)
    _enqueue_maps([p], [(H, W)], [slots[3]], 64, 64, o4, stream=s.cuda_stream)
    s.synchronize()
    for what, b, T, ns, o in (("first list call", b1, 16, slots[0], o1), ("second list call", b2, 128, slots[1], o2),
                              ("first grid call", g3, 32, slots[2], o3), ("second grid call", g4, 64, slots[3], o4)):
        _assert_device(lab, b, ns, T, o.results()[0], what)
    _guards_intact(ups)


# ---- the box entry on the same boxes ---------------------------------------------------------------------------
def test_agreement_with_the_box_palettes_entry():
    phd, L, torch = _phd()
    H, W = 150, 171
    lab = bpc.random_map(H, W, 17, 97)
    t = torch.from_numpy(lab.view(np.int16)).cuda()
    for T in wpc.SIZES:
        boxes = wpc.edge_windows(T, H, W)
        dicts = [dict(top=b[0], bottom=b[1], left=b[2], right=b[3]) for b in boxes]
        (box,) = phd.box_palettes_device([t], [17], [dicts])
        (win,) = phd.palette_windows_device([t], [17], [boxes], window=T)
        assert win.dtype == torch.int32 and tuple(win.shape) == box.shape == (len(boxes), 18)
        assert np.array_equal(win.cpu().numpy().view(np.uint32), box), f"against box_palettes_device at {T}"


# ---- end to end -------------------------------------------------------------------------------------------------
def test_report_labels_to_palette_maps_to_quantised_image():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    H, W, T = 352, 368, 16
    img = np.ascontiguousarray(synth.make("structured", H, W, 11))
    reps, labels = phd.reports_device_labels([torch.from_numpy(img).cuda()])
    rep, lab = reps[0], labels[0]
    mh, mw = int(lab.shape[0]), int(lab.shape[1])
    assert (mh, mw) == (H, W) and mh % T == 0 and mw % T == 0          # the grid tiles the map exactly
    q = np.array(rep.color_palette.quantities)
    ns = len(q)
    (counts, dom), = phd.palette_maps_device([lab], [rep], window=T, stride=T, counts=True, dominant=True)
    assert tuple(counts.shape) == (22, 23, ns + 1) and tuple(dom.shape) == (22, 23)
    assert counts.dtype == torch.int32 and dom.dtype == torch.int16
    c = counts.cpu().numpy().view(np.uint32).reshape(-1, ns + 1)
    host = lab.cpu().numpy().view(np.uint16)
    boxes, _ = phd.window_grid(mh, mw, T, T)
    _assert_device(host, boxes, ns, T, (c, dom.cpu().numpy().view(np.uint16).reshape(-1)), "end to end")
    mine = c[:, :ns].sum(axis=0, dtype=np.int64).astype(np.float64) * (1.0 / float(mh * mw))
    assert np.array_equal(mine.view(np.int64), q.view(np.int64)), "the counts of a tiling add up to the report's"
    (painted,) = phd.quantize_device([dom], [rep])
    assert tuple(painted.shape) == (22, 23, 3) and painted.dtype == torch.uint8
    colours = {tuple(int(v) for v in col) for col in rep.color_palette.colors} | {(0, 0, 0)}
    assert {tuple(px) for px in painted.cpu().numpy().reshape(-1, 3).tolist()} <= colours


# ---- the wrappers ---------------------------------------------------------------------------------------------------
def test_python_wrappers():
    phd, L, torch = _phd()
    H, W = 150, 171
    labs = [bpc.random_map(H, W, 17, 91), bpc.random_map(H, W, 3, 92)]
    ts = [torch.from_numpy(a.view(np.int16)).cuda() for a in labs]
    for window, stride in ((16, None), (32, 20), (64, None), (128, 11)):
        boxes, (gh, gw) = phd.window_grid(H, W, window, stride)
        res = phd.palette_maps_device(ts, [17, 3], window=window, stride=stride, dominant=True)
        for (c, d), lab, ns in zip(res, labs, (17, 3)):
            assert tuple(c.shape) == (gh, gw, ns + 1) and c.dtype == torch.int32 and c.is_cuda
            assert tuple(d.shape) == (gh, gw) and d.dtype == torch.int16 and d.is_cuda
            _assert_device(lab, boxes, ns, window, (c.cpu().numpy().view(np.uint32).reshape(-1, ns + 1),
                                                    d.cpu().numpy().view(np.uint16).reshape(-1)), f"map {window}")
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        r = phd.palette_windows_device(ts, [17, 3], [boxes, None], window=window, stream=st)
        st.synchronize()
        assert tuple(r[0].shape) == (len(boxes), 18) and tuple(r[1].shape) == (0, 4) and r[1].dtype == torch.int32
        assert torch.equal(r[0], res[0][0].reshape(-1, 18))
        (only_d,) = phd.palette_windows_device(ts[:1], [17], [boxes[:3]], window=window, counts=False, dominant=True)
        assert isinstance(only_d, torch.Tensor) and only_d.dtype == torch.int16
        assert torch.equal(only_d, res[0][1].reshape(-1)[:3])
    assert tuple(phd.palette_maps_device(ts[:1], [17])[0].shape) == ((H - 64) // 64 + 1, (W - 64) // 64 + 1, 18)
    with pytest.raises(RuntimeError, match="16, 32, 64 or 128, not 48"):
        phd.palette_windows_device(ts[:1], [17], [[(0, 48, 0, 48)]], window=48)
    with pytest.raises(RuntimeError, match="stride must be positive, not 0"):
        phd.palette_maps_device(ts[:1], [17], window=64, stride=0)
    with pytest.raises(RuntimeError, match="n_slots must be in 0..4096, not 4097"):
        phd.palette_maps_device(ts[:1], [4097])
    with pytest.raises(ValueError, match="counts or dominant"):
        phd.palette_maps_device(ts[:1], [17], counts=False)
