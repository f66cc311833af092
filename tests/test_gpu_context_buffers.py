"""The context's grow-only blocks on the MI355X (grow_buf.h: GrowBuf, Staged):
each stage that owns a device / pinned pair runs alone on a fresh context with
a small job, a larger one whose byte need passes the first job's capacity
(need + need / 4 + 4096, derived at each case from the stage's own layout) and
the small one again.  phd_debug_context_bytes shows the growth between calls 1
and 2 and none between 2 and 3; every call's results meet what the stage's own
GPU test compares them with, at that test's bars (the host twin bit for bit
where that test says so), and calls 1 and 3 are identical.  Then the teardown:
phd_shutdown leaves 0, 0 and the next call gives the same values."""
import ctypes

import numpy as np
import pytest

from tests import blur_windows_cases as bwc
from tests import box_palette_cases as bc
from tests import box_stats_cases as bsc
from tests.sharp_boxes import assert_sharp, box
from tests.test_gpu_parity import _phd

pytestmark = pytest.mark.gpu


def cap(need):
    """GrowBuf's growth rule."""
    return need + need // 4 + 4096


def _bytes(L):
    d, h = ctypes.c_ulonglong(1), ctypes.c_ulonglong(1)
    assert L.lib.phd_debug_context_bytes(ctypes.byref(d), ctypes.byref(h)) == 0
    return d.value, h.value


def _fresh(L):
    """No context: the case's first call makes one whose blocks are all empty."""
    L.lib.phd_shutdown()
    assert _bytes(L) == (0, 0)


def _three_calls(L, run, small, large):
    """run(job) for small, large, small on a fresh context: the three results;
    both totals rise between calls 1 and 2 and stay between 2 and 3."""
    _fresh(L)
    r1, b1 = run(small), _bytes(L)
    r2, b2 = run(large), _bytes(L)
    r3, b3 = run(small), _bytes(L)
    print("context bytes (device, pinned) after calls 1, 2, 3:", b1, b2, b3)
    assert b1[0] > 0 and b1[1] > 0
    assert b2[0] > b1[0] and b2[1] > b1[1], (b1, b2)
    assert b3 == b2, (b2, b3)
    return r1, r2, r3, (b1, b2, b3)


# ---- box statistics ---------------------------------------------------------------------------
# Device (phd_boxstats.cpp, BoxStatLayout): records al(24 nb) | items 16 ni -> al | sums al(8 * 264 nb) |
# finish al(64 nb); pinned max(records | items, 64 nb).  One box (one item): 256 + 256 + 2304 + 256 = 3072
# -> capacity 7936; pinned 272 -> 4436.  Eight boxes: 256 + 256 + 16896 + 512 = 17920 > 7936, but pinned
# max(384, 512) <= 4436: only the device block regrows.  72 boxes: pinned 64 * 72 = 4608 > 4436, device
# 1792 + 1280 + 152064 + 4608 = 159744 > 17920 + 17920 / 4 + 4096 = 26496: both regrow.
EIGHT = [(3, 40, 5, 30),                   # 25 columns: one pixel past the 4-pixel units, left = 1 (mod 4)
         (0, 64, 0, 64), (10, 11, 0, 64), (0, 64, 63, 64), (7, 9, 2, 9), (20, 50, 3, 6), (63, 64, 61, 64),
         (31, 33, 30, 47)]


def _box_stat_jobs():
    rng = np.random.default_rng(5)
    many = list(EIGHT)
    while len(many) < 72:
        t, l = int(rng.integers(0, 64)), int(rng.integers(0, 64))
        many.append((t, int(rng.integers(t + 1, 65)), l, int(rng.integers(l + 1, 65))))
    assert any((r - l) % 4 for _, _, l, r in EIGHT)
    return EIGHT[:1], EIGHT, many


def _box_stat_run(torch):
    """(run(boxes) -> [n, 7], the image, its device tensor): one 64 x 64 image whose
    origin is an odd device address."""
    from tests.test_gpu_box_stats import _stage, _upload
    img = bsc.random_image(64, 64, 31)
    buf, p = _upload(torch, img, 1)
    assert p % 2 == 1
    return (lambda boxes: _stage([p], [(64, 64)], [boxes])[0]), img, buf


def test_box_statistics_regrow():
    phd, L, torch = _phd()
    one, eight, many = _box_stat_jobs()
    run, img, keep = _box_stat_run(torch)
    _fresh(L)
    r1, b1 = run(one), _bytes(L)
    assert b1 == (cap(3072), cap(272)) == (7936, 4436)
    r8, b8 = run(eight), _bytes(L)
    assert b8 == (cap(17920), b1[1]), "eight boxes: the device block regrows, the pinned one holds them"
    r2, b2 = run(many), _bytes(L)
    r3, b3 = run(one), _bytes(L)
    assert b2 == (cap(159744), cap(4608)) and b2[0] > b8[0] and b2[1] > b8[1] and b3 == b2, (b8, b2, b3)
    for got, boxes in ((r1, one), (r8, eight), (r2, many), (r3, one)):
        want = bsc.host_twin(img, boxes, want_sums=False)[0]
        np.testing.assert_array_equal(bsc.bits(got), bsc.bits(want), err_msg=f"{len(boxes)} boxes: the host twin")
        bsc.assert_close(got, bsc.expected_u8(img, boxes), boxes, f"{len(boxes)} boxes")
    np.testing.assert_array_equal(bsc.bits(r3), bsc.bits(r1))


# ---- box palettes -----------------------------------------------------------------------------
# Counters (phd_boxpal.cpp): 4 (n_slots + 1) bytes per box, device and pinned alike; the launch table:
# al(32 boxes) + 16 items.  One box of 17 slots: 72 -> capacity 4186 (table 272 -> 4436).  Two boxes of
# 4095 slots: 2 * 4096 * 4 = 32768 > 4186.
def test_box_palettes_regrow():
    phd, L, torch = _phd()
    from tests.test_gpu_box_palettes import _stage, _upload
    maps = {ns: bc.random_map(64, 64, ns, 40 + ns) for ns in (17, 4095)}
    ups = {ns: _upload(torch, lab) for ns, lab in maps.items()}
    small = (17, [(3, 40, 5, 30)])
    large = (4095, [(0, 64, 0, 64), (1, 63, 3, 62)])

    def run(job):
        ns, boxes = job
        return _stage([ups[ns][1]], [(64, 64)], [ns], [boxes])[0]

    r1, r2, r3, (b1, b2, b3) = _three_calls(L, run, small, large)
    assert b1 == (cap(72) + cap(272), cap(72) + cap(272))
    assert b2 == (cap(32768) + cap(272), cap(32768) + cap(272))
    for got, (ns, boxes) in ((r1, small), (r2, large), (r3, small)):
        np.testing.assert_array_equal(got, bc.expected_counts(maps[ns], boxes, ns))
        np.testing.assert_array_equal(got.sum(axis=1, dtype=np.int64), [(bo - t) * (r - l) for t, bo, l, r in boxes])
    np.testing.assert_array_equal(r3, r1)


# ---- batched sharpness ------------------------------------------------------------------------
# (phd_report.cpp, enqueue_sharpness) uploaded: pointers al(8 n) | boxes al(24 nb) | prefix al(4 (nb + 1));
# device only: partials al(24 slices) | flat sums al(16 nb).  Two images, one box of three tiles: uploaded 768
# -> pinned capacity 5056; device 768 + 256 + 256 = 1280 -> 5696.  200 boxes: uploaded 256 + 4864 + 1024 =
# 6144 > 5056, device > 6144 > 5696.
def _sharp_jobs():
    rng = np.random.default_rng(9)
    small = [None, [box(7, 40, 3, 36)]]                                   # 33 x 33: three tiles
    lists = [[], []]
    for k in range(200):
        t, l = int(rng.integers(0, 52)), int(rng.integers(0, 52))
        lists[k % 2].append(box(t, int(rng.integers(t + 12, 65)), l, int(rng.integers(l + 12, 65))))
    return small, lists


def test_batched_sharpness_regrow():
    phd, L, torch = _phd()
    from oracle import oracle as orc
    from photohive_dsp_amd import synth
    from photohive_dsp_amd.core import sharpness_device
    imgs = [synth.make(k, 64, 64, 50 + i) for i, k in enumerate(("structured", "hblur"))]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    small, large = _sharp_jobs()
    r1, r2, r3, (b1, b2, b3) = _three_calls(L, lambda lists: sharpness_device(t, lists), small, large)
    assert b1[1] >= cap(768) and b2[1] >= cap(6144)
    for got, lists in ((r1, small), (r2, large), (r3, small)):
        for img, g, boxes in zip(imgs, got, lists):
            if boxes:
                assert_sharp(g, orc.sharpness(img, boxes))
            else:
                assert g == []
    assert r3 == r1


# ---- window blur ------------------------------------------------------------------------------
# (phd_blurwin.cpp, 64-px windows, 36 x 16 = 576 bins) device: twiddles al(16 * 64) | records 16 nw -> al |
# bin sums al(8 * 576 nw) | maxima al(8 nw); pinned max(twiddles | records, 8 * 576 nw + 8 nw).  One window:
# 1024 + 256 + 4608 + 256 = 6144 -> 11776, pinned 4616 -> 9866.  Six windows: 1280 + 27648 + 256 = 29184 >
# 11776, pinned 27696 > 9866.
def test_window_blur_regrow():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    from tests.test_gpu_blur_windows import _bits, _stage, _upload
    img = np.ascontiguousarray(synth.make("motion", 128, 128, 57))
    buf, p = _upload(torch, img, 1)
    small = [(1, 65, 3, 67)]
    large = [(0, 64, 0, 64), (0, 64, 64, 128), (64, 128, 0, 64), (64, 128, 64, 128), (33, 97, 31, 95), (1, 65, 3, 67)]
    r1, r2, r3, (b1, b2, b3) = _three_calls(L, lambda boxes: _stage([p], [(128, 128)], [boxes], 64)[0][0],
                                            small, large)
    assert b1 == (cap(6144), cap(4616)) and b2 == (cap(29184), cap(27696))
    for got, boxes in ((r1, small), (r2, large), (r3, small)):
        bwc.assert_windows(got, bwc.oracle_windows(img, boxes, 16, 36), f"{len(boxes)} windows")
        bwc.assert_windows(got, bwc.host_twin(img, boxes, 64), f"{len(boxes)} windows, twin")
        bwc.assert_vectors_follow_bins(got, f"{len(boxes)} windows")
    np.testing.assert_array_equal(_bits(r3), _bits(r1))
    np.testing.assert_array_equal(r3[1], r1[1])
    np.testing.assert_array_equal(r3[2], r1[2])
    assert buf[:16].eq(0xA5).all() and buf[-44:].eq(0xA5).all()


# ---- launch tables ----------------------------------------------------------------------------
# (phd_inputs.cpp, pack_view.h) one 64-byte PackRec per view, device and pinned alike: one view 64 ->
# capacity 4176; 128 views 8192 > 4176.
@pytest.mark.parametrize("own_stream", [False, True], ids=["library_stream", "caller_stream"])
def test_launch_tables_regrow(own_stream):
    """On a caller's stream the call does not wait for its launch: ev_views alone
    keeps the next call from regrowing or rewriting the table under it."""
    phd, L, torch = _phd()
    g = torch.Generator().manual_seed(7)
    chw = torch.randint(0, 256, (128, 3, 8, 8), dtype=torch.uint8, generator=g).cuda()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if own_stream else None

    def run(n):
        return phd.pack_views_device(chw[:n], "CHW", stream=stream)

    r1, r2, r3, (b1, b2, b3) = _three_calls(L, run, 1, 128)
    assert b1 == (cap(64), cap(64)) and b2 == (cap(8192), cap(8192))
    if own_stream:
        stream.synchronize()
    for got in (r1, r2, r3):
        assert len(got) in (1, 128)
        for out, src in zip(got, chw):
            assert torch.equal(out, src.permute(1, 2, 0).contiguous())
    assert torch.equal(r3[0], r1[0])


# ---- teardown ---------------------------------------------------------------------------------
def test_teardown_leaves_nothing_and_the_next_call_starts_afresh():
    phd, L, torch = _phd()
    jobs = _box_stat_jobs()
    run, img, keep = _box_stat_run(torch)
    first = [run(boxes) for boxes in jobs]
    assert _bytes(L)[0] >= cap(159744)                        # (whatever the cases before left, and these)
    L.lib.phd_shutdown()
    assert _bytes(L) == (0, 0)
    L.lib.phd_shutdown()                                      # twice
    assert _bytes(L) == (0, 0)
    again = [run(jobs[0])]
    assert _bytes(L) == (cap(3072), cap(272)), "a fresh context: the first job's capacities"
    again += [run(boxes) for boxes in jobs[1:]]
    for a, b, boxes in zip(first, again, jobs):
        np.testing.assert_array_equal(bsc.bits(b), bsc.bits(a), err_msg=f"{len(boxes)} boxes after the teardown")
        np.testing.assert_array_equal(bsc.bits(b), bsc.bits(bsc.host_twin(img, boxes, want_sums=False)[0]))
