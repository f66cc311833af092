"""Palette label maps on the device (palette_labels.hip) against the reference's
own label maps (tests/golden/labels_*.npz, tests/label_cases.py) and the C
oracle's per-pixel groups.

Bars: maps element for element and by SHA-256; the report returned with a map
against reports_device_mixed on the same image -- palette order, percentages,
RGB statistics, bins and blur vectors bit for bit, palette h / s / v at 1e-12
relative (fp64 atomics land in any order), S-bar at 1e-12 relative for the
same reason (tests/test_gpu_views.py's bar); per slot, percentages[i] ==
(double)count(label == i) * (1.0 / (double)(mh*mw)) bit for bit."""
import ctypes
import functools

import numpy as np
import pytest

from tests import label_cases as lc
from tests import palette_grids as pg
from tests.test_gpu_parity import _phd, _trace

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in lc.manifest()}
GUARD, FILL = 64, 0xABCD
L64 = ("uniform_401x577_L64", "motion_401x577_L64", "structured_577x401_L64")   # one configuration, r = 1


class Guarded:
    """A label buffer of n elements between two GUARD-element bands of FILL;
    off: elements past 8-byte alignment."""

    def __init__(self, torch, n, off=0):
        self.n, self.off = n, off
        self.buf = torch.full((GUARD + off + n + GUARD,), int(np.array([FILL], np.uint16).view(np.int16)[0]),
                              dtype=torch.int16, device="cuda")
        assert self.buf.data_ptr() % 8 == 0
        self.ptr = self.buf.data_ptr() + 2 * (GUARD + off)
        assert self.ptr % 8 == (2 * off) % 8

    def host(self):
        return self.buf.cpu().numpy().view(np.uint16)

    def map(self, shape):
        return self.host()[GUARD + self.off:GUARD + self.off + self.n].reshape(shape)

    def assert_guards(self, what=""):
        h = self.host()
        assert (h[:GUARD + self.off] == FILL).all() and (h[GUARD + self.off + self.n:] == FILL).all(), what

    def untouched(self):
        return bool((self.host() == FILL).all())


def _call(imgs, kw, maps, crops=None):
    """phd_report_batch_device_mixed_labels over device tensors [H, W, 3];
    maps: a label pointer or None per image.  (rc, reports or None, statuses)"""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import _finish, make_config
    from photohive_dsp_amd.structures import Full_Report_Data
    n = len(imgs)
    cfg = make_config(**kw)
    ptrs = (ctypes.c_void_p * n)(*[im.data_ptr() for im in imgs])
    hs = (ctypes.c_int * n)(*[int(im.shape[0]) for im in imgs])
    ws = (ctypes.c_int * n)(*[int(im.shape[1]) for im in imgs])
    lab = (ctypes.c_void_p * n)(*maps)
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    rc = L.lib.phd_report_batch_device_mixed_labels(ptrs, hs, ws, n, ctypes.byref(cfg), crops, lab, outs, st, None)
    reps = [_finish(outs[i], hs[i], ws[i], kw) if st[i] == 0 else None for i in range(n)]
    return rc, reps, list(st)


def _dev(torch, a):
    """A device copy of a (read-only) host array."""
    return torch.tensor(a, device="cuda")


@functools.lru_cache(maxsize=None)
def _image(name):
    img = np.ascontiguousarray(lc.image(CASES[name]))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _expected(name):
    fx = lc.fixture(name)
    lab = lc.expected_map(CASES[name], fx, _image(name))
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def _single(name):
    """(map, report) of one fixture image alone in a call, its map guarded."""
    phd, L, torch = _phd()
    case = CASES[name]
    want = _expected(name)
    t = _dev(torch, _image(name))
    g = Guarded(torch, want.size)
    rc, reps, st = _call([t], case["config"], [g.ptr])
    assert rc == 0 and st == [0], L.last_error()
    g.assert_guards(name)
    lab = g.map(want.shape).copy()
    lab.setflags(write=False)
    return lab, reps[0]


def _assert_count_identity(lab, rep, what=""):
    q = np.array(rep.color_palette.quantities)
    got = lc.percentages(lc.slot_counts(lab, len(q)), lab.size)
    assert np.array_equal(got.view(np.int64), q.view(np.int64)), what
    assert lab[lab != lc.NONE].max(initial=0) < len(q), what


def _assert_same_report(got, want, what=""):
    assert got.color_palette.group_ids == want.color_palette.group_ids, what
    assert got.color_palette.quantities == want.color_palette.quantities, what
    for f in ("Br", "Bg", "Bb", "Cr", "Cg", "Cb"):
        assert getattr(got.rgb_stats, f) == getattr(want.rgb_stats, f), (what, f)
    assert np.array_equal(np.array(got.blur_profile.bins), np.array(want.blur_profile.bins)), what
    assert [(v.angle, v.magnitude) for v in got.blur_vectors] == [(v.angle, v.magnitude) for v in want.blur_vectors]
    assert got.sharpnesses == want.sharpnesses, what
    np.testing.assert_allclose(np.array(got.color_palette.hsv), np.array(want.color_palette.hsv), rtol=1e-12, atol=0)
    assert got.average_saturation == pytest.approx(want.average_saturation, rel=1e-12), what


# ---- 1. fixture parity (6.: the downsampled maps are two of the cases) ----------

@pytest.mark.parametrize("name", list(CASES))
def test_fixture_parity(name):
    phd, L, torch = _phd()
    case, fx, want = CASES[name], lc.fixture(name), _expected(name)
    lab, rep = _single(name)
    assert lab.shape == want.shape == lc.map_shape(case["height"], case["width"],
                                                   case["config"].get("downsample_rate", 1))
    bad = np.flatnonzero(lab.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (f"{bad.size} labels differ, first at {bad[:5]}: "
                           f"{lab.reshape(-1)[bad[:5]]} for {want.reshape(-1)[bad[:5]]}")
    assert lc.map_sha256(lab) == fx["sha256"].tobytes()
    plain = phd.reports_device_mixed([_dev(torch, _image(name))], **case["config"])[0]
    _assert_same_report(rep, plain, name)
    _assert_count_identity(lab, rep, name)
    np.testing.assert_array_equal(lc.slot_counts(lab, len(fx["counts"])), fx["counts"])


def test_downsampled_maps_through_the_wrapper():
    """reports_device_labels: int16 maps of 360 x 640 (ds 2) and 233 x 300 (ds 3)
    holding the C map's bits, NONE as -1."""
    phd, L, torch = _phd()
    for name, shape in (("structured_720x1280_ds2", (360, 640)), ("uniform_700x900_ds3_L50", (233, 300))):
        reps, labs = phd.reports_device_labels([_dev(torch, _image(name))], **CASES[name]["config"])
        assert labs[0].dtype == torch.int16 and tuple(labs[0].shape) == shape and labs[0].is_cuda
        got = labs[0].cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint16), _expected(name))
        assert int((got == -1).sum()) == len(lc.fixture(name)["dropped"])
        _assert_count_identity(got.view(np.uint16), reps[0], name)


# ---- 2. one mixed call: two sizes, one size group of three, a NULL destination ---

def test_mixed_call_with_null_entries_and_guard_bands():
    phd, L, torch = _phd()
    names = list(L64) + [L64[0], L64[2]]              # 401x577: uniform, motion, uniform; 577x401: two
    null = {3}
    imgs = [_dev(torch, _image(n)) for n in names]
    bufs = [None if i in null else Guarded(torch, _expected(n).size) for i, n in enumerate(names)]
    # (one lane, so both size groups run on the context whose profiler mask is set here)
    prev = L.lib.phd_set_lanes(1)
    assert L.lib.phd_profile_kernels(1 << L.PALETTE_LABELS_KERNEL) == 0
    try:
        rc, reps, st = _call(imgs, CASES[L64[0]]["config"], [b.ptr if b else None for b in bufs])
        tot, cnt = ctypes.c_double(), ctypes.c_long()
        assert L.lib.phd_profile_read(L.PALETTE_LABELS_KERNEL, ctypes.byref(tot), ctypes.byref(cnt)) == 0
        assert cnt.value == 2 and tot.value > 0, "one label launch per size group"
        # and none when no image asks for a map
        phd.reports_device_mixed(imgs, **CASES[L64[0]]["config"])
        assert L.lib.phd_profile_read(L.PALETTE_LABELS_KERNEL, ctypes.byref(tot), ctypes.byref(cnt)) == 0
        assert cnt.value == 2
    finally:
        L.lib.phd_profile_kernels(0)
        L.lib.phd_set_lanes(prev)
    assert rc == 0 and st == [0] * len(names), L.last_error()
    # the same call on two lanes, one size group each
    bufs2 = [None if i in null else Guarded(torch, _expected(n).size) for i, n in enumerate(names)]
    rc2, reps2, st2 = _call(imgs, CASES[L64[0]]["config"], [b.ptr if b else None for b in bufs2])
    assert rc2 == 0 and st2 == st, L.last_error()
    for b, b2 in zip(bufs, bufs2):
        assert (b is None and b2 is None) or np.array_equal(b.host(), b2.host())
    for i, n in enumerate(names):
        one, rep1 = _single(n)
        _assert_same_report(reps[i], rep1, (i, n))
        if bufs[i] is None:
            continue
        bufs[i].assert_guards((i, n))
        np.testing.assert_array_equal(bufs[i].map(one.shape), one, err_msg=f"image {i} ({n})")


# ---- 3. unaligned image and map bases ----------------------------------------------

@pytest.mark.parametrize("img_off", [1, 2])
def test_unaligned_image_and_map_bases(img_off):
    """Images 1 or 2 bytes into larger allocations (byte loads, kAligned =
    false), maps 2 bytes past 8-byte alignment (u16 stores)."""
    phd, L, torch = _phd()
    imgs, keep = [], []
    for n in L64:
        a = _image(n)
        big = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
        big[img_off:img_off + a.size] = _dev(torch, a.reshape(-1))
        v = big[img_off:img_off + a.size].view(*a.shape)
        assert v.data_ptr() % 4 == img_off and v.is_contiguous()
        imgs.append(v)
        keep.append(big)
    bufs = [Guarded(torch, _expected(n).size, off=1) for n in L64]
    assert all(b.ptr % 8 == 2 for b in bufs)
    rc, reps, st = _call(imgs, CASES[L64[0]]["config"], [b.ptr for b in bufs])
    assert rc == 0 and st == [0, 0, 0], L.last_error()
    for n, b, rep in zip(L64, bufs, reps):
        one, rep1 = _single(n)
        b.assert_guards(n)
        np.testing.assert_array_equal(b.map(one.shape), one, err_msg=n)
        _assert_same_report(rep, rep1, n)


# ---- 4. lanes ------------------------------------------------------------------------

def test_lanes_two_and_one_give_identical_maps():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    h, w, n = 401, 577, 16
    t = torch.from_numpy(np.stack([synth.make("uniform", h, w, 100 + i) for i in range(n)])).cuda()
    kw = dict(linked_list_size=64)
    prev = L.lib.phd_set_lanes(2)
    try:
        reps2, labs2 = phd.reports_device_labels(t, **kw)
        assert L.lib.phd_set_lanes(1) == 2
        reps1, labs1 = phd.reports_device_labels(t, **kw)
    finally:
        L.lib.phd_set_lanes(prev)
    assert len(labs1) == len(labs2) == n
    for i in range(n):
        a, b = labs2[i].cpu().numpy().view(np.uint16), labs1[i].cpu().numpy().view(np.uint16)
        assert a.shape == (h, w)
        np.testing.assert_array_equal(a, b, err_msg=f"image {i}")
        _assert_count_identity(a, reps2[i], i)
        _assert_count_identity(b, reps1[i], i)
        assert int((a == lc.NONE).sum()) > 0                     # L = 64 on noise: every image drops pixels


# ---- 5. kernel paths -------------------------------------------------------------------

# case -> (grid of tests/palette_grids.py, further parameters per image kind, fused, batched tail).  L = 64.
PATH_CASES = {
    "fused_thr": ("18_2_3", {}, True, True),                     # table K1; batched label kernel, kThr = true
    "fused_si8": ("s8_table", {}, True, True),                   # ... kThr = false
    "k3_batched_thr": ("h360_s4", {}, False, True),              # K1 histogram + Kcut + batched K3
    "k3_batched_si8": ("s10_twopass", {}, False, True),
    # the per-image Kcut / K3 and the one-image label kernel: slot counts the batched K3's LDS does not hold
    "k3_per_image": ("max_grid", dict(dominant=dict(coverage_thresh=0.9)), False, False),
}


@pytest.mark.parametrize("kind,seed", [("uniform", 1), ("dominant", 2)])
@pytest.mark.parametrize("case", list(PATH_CASES))
def test_kernel_paths(case, kind, seed):
    phd, L, torch = _phd()
    from oracle import oracle as orc
    from photohive_dsp_amd import synth
    name, extra, fused, batched = PATH_CASES[case]
    base = pg.LEGACY[name][0] if name in pg.LEGACY else pg.GRIDS[name][0]
    cfg = dict(base, linked_list_size=64, **extra.get(kind, {}))
    img = np.ascontiguousarray(synth.make(kind, 384, 512, seed))
    hist, parents, kept = _trace(img, **cfg)
    m = pg.path(cfg, len(parents))
    print(f"{case}/{kind}: {len(parents)} slots, path {pg.describe(m)}, {img.shape[0] * img.shape[1] - kept.sum()} "
          "pixels dropped")
    assert m >= 0 and bool(m & pg.FUSED) == fused and bool(m & pg.BATCHED) == batched, pg.describe(m)
    g = Guarded(torch, img.shape[0] * img.shape[1])
    rc, reps, st = _call([torch.from_numpy(img).cuda()], cfg, [g.ptr])
    assert rc == 0 and st == [0], L.last_error()
    g.assert_guards()
    lab = g.map(img.shape[:2]).reshape(-1)
    _assert_count_identity(lab, reps[0])
    np.testing.assert_array_equal(lc.slot_counts(lab, len(parents)), kept)
    gid = orc.group_ids(img, **cfg)
    on = lab != lc.NONE
    pairs = np.unique(np.stack([gid[on].astype(np.int64), lab[on].astype(np.int64)]), axis=1)
    assert pairs.shape[1] == len(np.unique(gid[on])), "the kept pixels of one group carry two labels"
    slot_of_group = dict(zip(pairs[0].tolist(), pairs[1].tolist()))
    for i, p in enumerate(parents.tolist()):
        if hist[p]:
            assert slot_of_group.get(p) == i, f"parent group {p} is slot {i}, its pixels are labelled {slot_of_group.get(p)}"
            assert on[gid == p].all(), f"parent group {p} lost pixels of its own"


# ---- 7. the quantised image --------------------------------------------------------------

def _lut_image(lab, lut, none):
    out = np.empty(lab.shape + (3,), np.uint8)
    out[...] = np.array(none, np.uint8)
    ok = lab < len(lut)
    out[ok] = lut[lab[ok]]
    return out


def test_labels_to_rgb_against_numpy():
    """One launch over a 1x1 map, a 7x5 map at odd bases and a 401x577 map:
    lut[label], none_rgb for NONE and for labels >= n_slots."""
    phd, L, torch = _phd()
    rng = np.random.default_rng(7)
    none = (9, 200, 31)
    shapes, n_slots, offs = [(1, 1), (7, 5), (401, 577)], [1, 6, 300], [(0, 0), (1, 1), (0, 0)]
    labs, luts, keep, maps, dsts = [], [], [], [], []
    for (h, w), ns, (mo, do) in zip(shapes, n_slots, offs):
        lab = rng.integers(0, ns + 3, size=(h, w)).astype(np.uint16)
        lab[rng.random((h, w)) < 0.1] = lc.NONE
        if lab.size > 4:
            lab.reshape(-1)[:4] = [0, ns - 1, ns, lc.NONE]
        lut = rng.integers(0, 256, size=(ns, 3)).astype(np.uint8)
        m = torch.zeros(lab.size + 8, dtype=torch.int16, device="cuda")
        m[mo:mo + lab.size] = torch.from_numpy(lab.view(np.int16).reshape(-1)).cuda()
        d = torch.full((3 * lab.size + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        labs.append(lab)
        luts.append(lut)
        keep += [m, d]
        maps.append(m.data_ptr() + 2 * mo)
        dsts.append((d, do))
    n = len(shapes)
    rc = L.lib.phd_labels_to_rgb_device((ctypes.c_void_p * n)(*maps), (ctypes.c_int * n)(*[s[0] for s in shapes]),
                                        (ctypes.c_int * n)(*[s[1] for s in shapes]), n,
                                        (ctypes.c_void_p * n)(*[a.ctypes.data for a in luts]),
                                        (ctypes.c_int * n)(*n_slots), (ctypes.c_uint8 * 3)(*none),
                                        (ctypes.c_void_p * n)(*[d.data_ptr() + do for d, do in dsts]), None)
    assert rc == 0, L.last_error()
    for lab, lut, (d, do) in zip(labs, luts, dsts):
        got = d.cpu().numpy()
        np.testing.assert_array_equal(got[do:do + 3 * lab.size].reshape(lab.shape + (3,)), _lut_image(lab, lut, none))
        assert (got[:do] == 0x5A).all() and (got[do + 3 * lab.size:] == 0x5A).all(), "written outside the image"


def test_quantize_device_paints_the_palette_colours():
    phd, L, torch = _phd()
    names = ("uniform_401x577_L64", "uniform_700x900_ds3_L50")            # two sizes in one call
    labs, reps = [], []
    for n in names:
        lab, rep = _single(n)
        labs.append(torch.from_numpy(lab.view(np.int16).copy()).cuda())
        reps.append(rep)
    none = (255, 0, 255)
    out = phd.quantize_device(labs, reps, none_rgb=none)
    for n, o, rep in zip(names, out, reps):
        lab = _single(n)[0]
        assert o.dtype == torch.uint8 and tuple(o.shape) == lab.shape + (3,)
        lut = np.array([[int(c) for c in col] for col in rep.color_palette.colors], np.uint8)
        np.testing.assert_array_equal(o.cpu().numpy(), _lut_image(lab, lut, none), err_msg=n)


# ---- 8. an image that fails ----------------------------------------------------------------

def test_failing_image_fails_alone():
    """349 x 400 fails the reference's size check (src/utilities.c:64-87): no
    report, its buffer's guard bands intact, the other images' maps right."""
    phd, L, torch = _phd()
    names = (L64[0], L64[2])
    small = torch.zeros((349, 400, 3), dtype=torch.uint8, device="cuda")
    imgs = [_dev(torch, _image(names[0])), small, _dev(torch, _image(names[1]))]
    bufs = [Guarded(torch, _expected(names[0]).size), Guarded(torch, 349 * 400), Guarded(torch, _expected(names[1]).size)]
    rc, reps, st = _call(imgs, CASES[names[0]]["config"], [b.ptr for b in bufs])
    assert rc == 1 and st[0] == 0 and st[1] != 0 and st[2] == 0 and reps[1] is None
    for b in bufs:
        b.assert_guards()
    assert bufs[1].untouched()                                    # (the size check comes before any launch)
    for n, b in zip(names, (bufs[0], bufs[2])):
        one, _ = _single(n)
        np.testing.assert_array_equal(b.map(one.shape), one, err_msg=n)
