"""Box palettes on the device (box_palette.hip: k_box_counts) against plain
numpy over the same label maps (tests/box_palette_cases.py: expected_counts).

Bars: counts integer for integer; every row sums to its box's element count;
for the box that is the whole map, (double)count * (1.0 / (double)(mh*mw)) ==
the report's percentages bit for bit; a second run of a call gives identical
counts (integer atomics)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import box_palette_cases as bc
from tests import deep_label_cases as dc
from tests.test_gpu_labels import CASES, _dev, _expected, _image
from tests.test_gpu_parity import _phd

pytestmark = pytest.mark.gpu


def _take(L, bp, n):
    """numpy copies of n filled phd_box_palette structs; the C blocks are freed."""
    out = []
    for i in range(n):
        nb, ns = bp[i].n_boxes, bp[i].n_slots
        a = np.zeros((nb, ns + 1), np.uint32)
        if nb:
            ctypes.memmove(a.ctypes.data, bp[i].counts, a.nbytes)
        else:
            assert not bp[i].counts
        out.append(a)
    L.lib.phd_free_box_palettes(bp, n)
    assert all(not bp[i].counts and bp[i].n_boxes == 0 for i in range(n))
    return out


def _stage(ptrs, shapes, slots, boxes):
    """phd_box_palettes_device over device maps at ptrs; boxes[i]: a list of
    boxes or None for boxes[i] == NULL."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.structures import Crop_Boundaries, PhdBoxPalette
    n = len(ptrs)
    made = [bc.crop_boundaries(b) if b is not None else None for b in boxes]
    cbs = (ctypes.POINTER(Crop_Boundaries) * n)(*[ctypes.pointer(m[0]) if m else None for m in made])
    bp = (PhdBoxPalette * n)()
    rc = L.lib.phd_box_palettes_device((ctypes.c_void_p * n)(*ptrs), (ctypes.c_int * n)(*[s[0] for s in shapes]),
                                       (ctypes.c_int * n)(*[s[1] for s in shapes]), n, (ctypes.c_int * n)(*slots),
                                       cbs, bp, None)
    assert rc == 0, L.last_error()
    return _take(L, bp, n)


@functools.lru_cache(maxsize=None)
def _synthetic():
    return bc.synthetic_maps()


def _upload(torch, lab):
    """The map on the device at the host copy's 8-byte phase: (tensor, pointer)."""
    off = (lab.ctypes.data % 8) // 2
    buf = torch.zeros(lab.size + 4, dtype=torch.int16, device="cuda")
    assert buf.data_ptr() % 8 == 0
    buf[off:off + lab.size] = torch.tensor(np.ascontiguousarray(lab).view(np.int16).reshape(-1), device="cuda")
    return buf, buf.data_ptr() + 2 * off


def test_stage_alone_on_synthetic_maps():
    """One call over maps of different sizes and palettes, a NULL boxes[i] among
    them and one map at base + 2 bytes; the profiler sees one launch."""
    phd, L, torch = _phd()
    syn = _synthetic()
    ups = [_upload(torch, lab) for _, lab, _, _ in syn]
    assert any(p % 8 == 2 for _, p in ups)
    boxes = [b for _, _, _, b in syn]
    boxes[1] = None
    assert L.lib.phd_profile_kernels(1 << L.BOX_PALETTES_KERNEL) == 0
    try:
        got = _stage([p for _, p in ups], [lab.shape for _, lab, _, _ in syn], [ns for _, _, ns, _ in syn], boxes)
        tot, cnt = ctypes.c_double(), ctypes.c_long()
        assert L.lib.phd_profile_read(L.BOX_PALETTES_KERNEL, ctypes.byref(tot), ctypes.byref(cnt)) == 0
        assert cnt.value == 1 and tot.value > 0, "every box of every map in one launch"
    finally:
        L.lib.phd_profile_kernels(0)
    again = _stage([p for _, p in ups], [lab.shape for _, lab, _, _ in syn], [ns for _, _, ns, _ in syn], boxes)
    for (name, lab, ns, _), b, g, g2 in zip(syn, boxes, got, again):
        if b is None:
            assert g.shape == (0, ns + 1), name
            continue
        np.testing.assert_array_equal(g, bc.expected_counts(lab, b, ns), err_msg=name)
        np.testing.assert_array_equal(g.sum(axis=1, dtype=np.int64), [(bo - t) * (r - l) for t, bo, l, r in b])
        np.testing.assert_array_equal(g, g2, err_msg=f"{name}: second run")


def test_stage_alone_through_python():
    phd, L, torch = _phd()
    name, lab, ns, boxes = _synthetic()[3]
    t = torch.tensor(np.ascontiguousarray(lab).view(np.int16), device="cuda")
    dicts = [dict(top=b[0], bottom=b[1], left=b[2], right=b[3]) for b in boxes]
    got = phd.box_palettes_device([t, t], [ns, 5], [dicts, None])
    assert got[0].dtype == np.uint32 and got[1].shape == (0, 6)
    np.testing.assert_array_equal(got[0], bc.expected_counts(lab, boxes, ns))


# ---- the report entries ------------------------------------------------------------------

def _crops(box_lists):
    """(array of n POINTER(Crop_Boundaries), keep-alive): box_lists[i] a list of
    boxes of image coordinates, or None for crops[i] == NULL."""
    from photohive_dsp_amd.structures import Crop_Boundaries
    made = [bc.crop_boundaries(b) if b is not None else None for b in box_lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * len(box_lists))(*[ctypes.pointer(m[0]) if m else None for m in made])
    return arr, made


def _run(kind, srcs, kw, maps, box_lists, palettes=True):
    """phd_report_batch_device_<kind>_box_palettes; srcs: device tensors [H, W, 3]
    (kind "mixed") or descriptors; maps: None (d_labels == NULL) or a pointer or
    None per image; palettes=False: box_palettes == NULL.
    (rc, reports or None, statuses, palettes or None)"""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import _finish, make_config
    from photohive_dsp_amd.structures import Full_Report_Data, PhdBoxPalette
    n = len(srcs)
    cfg = make_config(**kw)
    crops, keep = _crops(box_lists) if box_lists is not None else (None, None)
    lab = (ctypes.c_void_p * n)(*maps) if maps is not None else None
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    bp = (PhdBoxPalette * n)() if palettes else None
    if palettes:
        for o in bp:                                             # the call zeroes them first
            o.n_boxes, o.n_slots = 5, 5
    if kind == "mixed":
        ptrs = (ctypes.c_void_p * n)(*[im.data_ptr() for im in srcs])
        hs = (ctypes.c_int * n)(*[int(im.shape[0]) for im in srcs])
        ws = (ctypes.c_int * n)(*[int(im.shape[1]) for im in srcs])
        rc = L.lib.phd_report_batch_device_mixed_box_palettes(ptrs, hs, ws, n, ctypes.byref(cfg), crops, lab, bp, outs,
                                                              st, None)
        sizes = list(zip(hs, ws))
    else:
        arr = (type(srcs[0]) * n)(*srcs)
        rc = getattr(L.lib, f"phd_report_batch_device_{kind}_box_palettes")(arr, n, ctypes.byref(cfg), crops, lab, bp,
                                                                            outs, st, None)
        sizes = [(v.height, v.width) for v in srcs]
    reps = [_finish(outs[i], *sizes[i], kw) if st[i] == 0 else None for i in range(n)]
    del keep
    return rc, reps, list(st), (_take(L, bp, n) if palettes else None)


def _check_image(pal, lab, img_boxes, ds, rep, what=""):
    """An image's box palette against numpy over its map `lab`; with the whole
    image as box 0, the count identity against the report's percentages."""
    mh, mw = lab.shape
    q = np.array(rep.color_palette.quantities)
    ns = len(q)
    if not img_boxes:
        assert pal.shape == (0, ns + 1), what
        return
    boxes = [bc.image_to_map_box(b, ds, mh, mw) for b in img_boxes]
    assert pal.shape == (len(boxes), ns + 1), what
    np.testing.assert_array_equal(pal, bc.expected_counts(lab, boxes, ns), err_msg=str(what))
    np.testing.assert_array_equal(pal.sum(axis=1, dtype=np.int64), [(b - t) * (r - l) for t, b, l, r in boxes])
    if boxes[0] == (0, mh, 0, mw):
        mine = pal[0, :ns].astype(np.float64) * (1.0 / float(mh * mw))
        assert np.array_equal(mine.view(np.int64), q.view(np.int64)), what
        assert int(pal[0, ns]) == int(np.count_nonzero(lab >= ns)), what


def _same_report(got, want, what=""):
    """tests/test_gpu_labels.py's _assert_same_report, with the sharpnesses
    compared as numbers that may be NaN (a 1 x 1 box, a black image: 0 / 0)."""
    from tests.test_gpu_labels import _assert_same_report
    g, w = (np.array(r.sharpnesses if r.sharpnesses is not None else [], np.float64) for r in (got, want))
    assert np.array_equal(g, w, equal_nan=True), what
    saved = got.sharpnesses, want.sharpnesses
    got.sharpnesses = want.sharpnesses = None
    try:
        _assert_same_report(got, want, what)
    finally:
        got.sharpnesses, want.sharpnesses = saved


def _img_boxes(name, seed=17):
    c = CASES[name]
    return bc.box_list(c["height"], c["width"], seed, empty=False)


@pytest.mark.parametrize("name", list(CASES))
def test_packed_route_with_a_caller_map_and_with_scratch(name):
    phd, L, torch = _phd()
    from tests.test_gpu_labels import Guarded
    kw = CASES[name]["config"]
    ds = kw.get("downsample_rate", 1)
    want = _expected(name)
    t = _dev(torch, _image(name))
    boxes = _img_boxes(name)
    g = Guarded(torch, want.size)
    rc, reps, st, pals = _run("mixed", [t], kw, [g.ptr], [boxes])
    assert rc == 0 and st == [0], L.last_error()
    g.assert_guards(name)
    np.testing.assert_array_equal(g.map(want.shape), want)
    _check_image(pals[0], want, boxes, ds, reps[0], (name, "caller map"))
    rc, reps2, st, pals2 = _run("mixed", [t], kw, None, [boxes])           # d_labels == NULL: the scratch map
    assert rc == 0 and st == [0], L.last_error()
    _check_image(pals2[0], want, boxes, ds, reps2[0], (name, "scratch"))
    np.testing.assert_array_equal(pals[0], pals2[0])
    _same_report(reps2[0], reps[0], name)
    # box_palettes == NULL is the _labels call
    from tests.test_gpu_labels import _call
    crops, keep = _crops([boxes])
    g3 = Guarded(torch, want.size)
    rc3, reps3, st3 = _call([t], kw, [g3.ptr], crops)
    rc4, reps4, st4, none = _run("mixed", [t], kw, [g.ptr], [boxes], palettes=False)
    assert rc3 == rc4 == 0 and none is None
    _same_report(reps4[0], reps3[0], (name, "NULL palettes"))
    _same_report(reps[0], reps3[0], (name, "with palettes"))
    assert np.array_equal(g3.host(), g.host())


def test_one_mixed_call_on_one_lane_and_two():
    """Two sizes; images with a map and boxes, boxes only, a map only, neither,
    a NULL destination, an image with a bad box: it fails alone."""
    phd, L, torch = _phd()
    from tests.test_gpu_labels import L64, Guarded
    names = [L64[0], L64[1], L64[2], L64[0], L64[2], L64[1], L64[0]]
    kw = CASES[L64[0]]["config"]
    imgs = [_dev(torch, _image(n)) for n in names]
    box_lists = [_img_boxes(names[0], 1), _img_boxes(names[1], 2), None, [], _img_boxes(names[4], 3),
                 [(0, 10, 0, 10), (5, 4, 0, 10)], _img_boxes(names[6], 4)]
    with_map = {0, 2, 4}
    bad = 5
    results = []
    prev = L.lib.phd_set_lanes(1)
    try:
        for lanes in (1, 2):
            L.lib.phd_set_lanes(lanes)
            bufs = [Guarded(torch, _expected(n).size) if i in with_map else None for i, n in enumerate(names)]
            rc, reps, st, pals = _run("mixed", imgs, kw, [b.ptr if b else None for b in bufs], box_lists)
            assert rc == 1 and [s == 0 for s in st] == [i != bad for i in range(len(names))], (st, L.last_error())
            assert pals[bad].shape == (0, 1) and reps[bad] is None          # {0, 0, NULL}
            for i, n in enumerate(names):
                if i == bad:
                    continue
                if bufs[i]:
                    bufs[i].assert_guards((lanes, i))
                    np.testing.assert_array_equal(bufs[i].map(_expected(n).shape), _expected(n))
                _check_image(pals[i], _expected(n), box_lists[i], 1, reps[i], (lanes, i))
            results.append(pals)
    finally:
        L.lib.phd_set_lanes(prev)
    for a, b in zip(*results):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("case", ["fused_thr", "k3_batched_thr", "k3_per_image"])
def test_palette_paths(case):
    """The fused palette, the batched K3 and the per-image K3 (the one-image
    label kernel writes the scratch map): counts against the map the same call
    returns, and against a scratch-map call."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    from tests import palette_grids as pg
    from tests.test_gpu_labels import PATH_CASES, Guarded
    name, extra, fused, batched = PATH_CASES[case]
    base = pg.LEGACY[name][0] if name in pg.LEGACY else pg.GRIDS[name][0]
    kind = "dominant"
    cfg = dict(base, linked_list_size=64, **extra.get(kind, {}))
    img = np.ascontiguousarray(synth.make(kind, 384, 512, 2))
    t = torch.from_numpy(img).cuda()
    boxes = bc.box_list(384, 512, 23, empty=False)
    g = Guarded(torch, 384 * 512)
    rc, reps, st, pals = _run("mixed", [t], cfg, [g.ptr], [boxes])
    assert rc == 0 and st == [0], L.last_error()
    m = pg.path(cfg, len(reps[0].color_palette.quantities))
    assert bool(m & pg.FUSED) == fused and bool(m & pg.BATCHED) == batched, pg.describe(m)
    lab = g.map((384, 512)).copy()
    _check_image(pals[0], lab, boxes, 1, reps[0], case)
    rc, reps2, st, pals2 = _run("mixed", [t], cfg, None, [boxes])
    assert rc == 0 and st == [0], L.last_error()
    np.testing.assert_array_equal(pals2[0], pals[0])


def test_views_yuv_and_typed_eight_bit():
    """A pitched BGRA view and a region of a larger frame; a 401 x 577 NV12
    surface with triangle chroma against the packed call over
    phd_convert_yuv_device's bytes; uint16 k * 257 (the 8-bit route)."""
    phd, L, torch = _phd()
    from tests.test_gpu_labels_inputs import _three_layouts, _typed, _u16_dev, _yuv_frames
    name = "uniform_401x577_L64"
    kw = CASES[name]["config"]
    want = _expected(name)
    boxes = _img_boxes(name)
    views, keep = _three_layouts(torch, _dev(torch, _image(name)))
    rc, reps, st, pals = _run("views", views[1:], kw, None, [boxes, boxes])
    assert rc == 0 and st == [0, 0], L.last_error()
    for k in range(2):
        _check_image(pals[k], want, boxes, 1, reps[k], ("views", k))
    tv = _typed([_u16_dev(torch, _image(name).astype(np.uint16) * 257)])
    rc, reps, st, pals = _run("typed_views", tv, kw, None, [boxes])
    assert rc == 0 and st == [0], L.last_error()
    _check_image(pals[0], want, boxes, 1, reps[0], "u16 k * 257")
    yv, keep2 = _yuv_frames()
    rgb = phd.convert_yuv_device(yv[:1])
    rc, reps_p, st, pals_p = _run("mixed", rgb, kw, None, [boxes])
    assert rc == 0 and st == [0], L.last_error()
    rc, reps_y, st, pals_y = _run("yuv", yv[:1], kw, None, [boxes])
    assert rc == 0 and st == [0], L.last_error()
    np.testing.assert_array_equal(pals_y[0], pals_p[0])
    assert pals_y[0][0].sum() == 401 * 577


@pytest.mark.parametrize("form", ["u16_hwc", "f64_chw"])
@pytest.mark.parametrize("name", [c["name"] for c in dc.manifest()])
def test_fp64_route(name, form):
    """Every deep fixture on the fp64 route (k_planar_labels, then the same
    counting kernel), with a caller map and with the scratch map."""
    phd, L, torch = _phd()
    from tests import deep_label_cases as dc
    from tests.test_gpu_labels import Guarded
    from tests.test_gpu_labels_inputs import DEEP, _deep_tensor, _typed
    kw = DEEP[name]["config"]
    ds = kw.get("downsample_rate", 1)
    fx = dc.fixture(name)
    want = fx["map"].astype(np.uint16)
    t, layout = _deep_tensor(torch, name, form)
    views = _typed([t], layout)
    boxes = bc.box_list(DEEP[name]["height"], DEEP[name]["width"], 29, empty=False)
    g = Guarded(torch, want.size)
    rc, reps, st, pals = _run("typed_views", views, kw, [g.ptr], [boxes])
    assert rc == 0 and st == [0], L.last_error()
    g.assert_guards(name)
    np.testing.assert_array_equal(g.map(want.shape), want)
    _check_image(pals[0], want, boxes, ds, reps[0], (name, form))
    assert np.array_equal(np.array(reps[0].color_palette.quantities).view(np.int64),
                          fx["percentages"].view(np.int64))
    rc, reps2, st, pals2 = _run("typed_views", views, kw, None, [boxes])
    assert rc == 0 and st == [0], L.last_error()
    np.testing.assert_array_equal(pals2[0], pals[0])


def test_a_nan_image_fails_alone():
    phd, L, torch = _phd()
    from tests.test_gpu_labels_inputs import _deep, _deep_tensor, _typed
    nd = "structured_353x401_L50"
    kw = dict(linked_list_size=50)
    nan = _deep(nd).astype(np.float32)
    nan[200, 123, 1] = np.nan
    d0, l0 = _deep_tensor(torch, nd, "u16_hwc")
    views = _typed([torch.from_numpy(nan).cuda()]) + _typed([d0], l0)
    boxes = bc.box_list(353, 401, 31, empty=False)
    rc, reps, st, pals = _run("typed_views", views, kw, None, [boxes, boxes])
    assert rc == 1 and st[0] != 0 and st[1] == 0, L.last_error()
    assert pals[0].shape == (0, 1)
    from tests import deep_label_cases as dc
    _check_image(pals[1], dc.fixture(nd)["map"].astype(np.uint16), boxes, 1, reps[1], nd)


def test_python_wrappers():
    """box_palettes=True with and without labels=True on the four wrappers."""
    phd, L, torch = _phd()
    from tests.test_gpu_labels_inputs import _deep_tensor, _yuv_frames
    name = "structured_720x1280_ds2"
    kw = CASES[name]["config"]
    want = _expected(name)
    t = _dev(torch, _image(name))
    boxes = _img_boxes(name)
    sal = [[dict(top=b[0], bottom=b[1], left=b[2], right=b[3]) for b in boxes]]

    def check(pals, reps, lab=want, ds=2, bx=boxes):
        assert len(pals) == 1 and pals[0].dtype == np.uint32
        _check_image(pals[0], lab, bx, ds, reps[0])

    reps, maps, pals = phd.reports_device_labels([t], salient_characters=sal, box_palettes=True, **kw)
    np.testing.assert_array_equal(maps[0].cpu().numpy().view(np.uint16), want)
    check(pals, reps)
    chw = t.permute(2, 0, 1).contiguous()
    reps, pals = phd.reports_device_views([chw], layout="CHW", salient_characters=sal, box_palettes=True, **kw)
    check(pals, reps)
    reps, maps, pals = phd.reports_device_views([chw], layout="CHW", salient_characters=sal, labels=True,
                                                box_palettes=True, **kw)
    assert maps[0].dtype == torch.int16
    check(pals, reps)
    reps, pals = phd.reports_device_views([chw], layout="CHW", box_palettes=True, **kw)       # no boxes
    assert pals[0].shape == (0, len(reps[0].color_palette.quantities) + 1)
    dn = "structured_706x802_ds2_L40"
    from tests import deep_label_cases as dc
    from tests.test_gpu_labels_inputs import DEEP
    d, layout = _deep_tensor(torch, dn, "u16_hwc")
    dbox = bc.box_list(706, 802, 37, empty=False)
    dsal = [[dict(top=b[0], bottom=b[1], left=b[2], right=b[3]) for b in dbox]]
    dlab = dc.fixture(dn)["map"].astype(np.uint16)
    reps, pals = phd.reports_device_typed([d], layout=layout, salient_characters=dsal, box_palettes=True,
                                          **DEEP[dn]["config"])
    check(pals, reps, dlab, 2, dbox)
    reps, maps, pals = phd.reports_device_typed([d], layout=layout, salient_characters=dsal, labels=True,
                                                box_palettes=True, **DEEP[dn]["config"])
    np.testing.assert_array_equal(maps[0].cpu().numpy().view(np.uint16), dlab)
    check(pals, reps, dlab, 2, dbox)
    yv, keep = _yuv_frames()
    ybox = bc.box_list(401, 577, 41, empty=False)
    ysal = [[dict(top=b[0], bottom=b[1], left=b[2], right=b[3]) for b in ybox]]
    frame = [phd.nv12_planes(keep[0], 401, 577)]
    ykw = dict(linked_list_size=64)
    reps, maps, pals = phd.reports_device_yuv(frame, chroma="triangle", salient_characters=ysal, labels=True,
                                              box_palettes=True, **ykw)
    check(pals, reps, maps[0].cpu().numpy().view(np.uint16), 1, ybox)
    reps2, pals2 = phd.reports_device_yuv(frame, chroma="triangle", salient_characters=ysal, box_palettes=True, **ykw)
    np.testing.assert_array_equal(pals2[0], pals[0])
    # the stage alone over the returned maps, boxes in map coordinates
    again = phd.box_palettes_device(maps, reps, ysal)
    np.testing.assert_array_equal(again[0], pals[0])
