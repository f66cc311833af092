"""The report entries' per-image outputs (label maps, box palettes, box
statistics) without a device: which entry a message names and which of the
caller's structs a call resets, the 32768-groups rule, the ctypes prototypes
and the Python wrappers' input checks.  Every expectation here was recorded
from the library as it stood before the outputs became one record
(ImageOutputs, phd_host.h): the tests pass unchanged on both sides."""
import ctypes
import itertools

import pytest

V, I, SZ, P = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER

STEM = "phd_report_batch_device_"
FAMILIES = ("mixed", "views", "typed_views", "yuv")
# entry -> (family, the outputs it takes, in argument order)
ENTRIES = {STEM + "mixed": ("mixed", ()), STEM + "mixed_crops": ("mixed", ())}
for _f in FAMILIES:
    if _f != "mixed":
        ENTRIES[STEM + _f] = (_f, ())
    ENTRIES[STEM + _f + "_labels"] = (_f, ("labels",))
    ENTRIES[STEM + _f + "_box_palettes"] = (_f, ("labels", "box_pal"))
    ENTRIES[STEM + _f + "_box_stats"] = (_f, ("labels", "box_pal", "box_stats"))


def _L():
    from photohive_dsp_amd import lib as L
    return L


def expected_name(entry, present, crops):
    """The entry a message names: the most derived output present picks the
    suffix; with none, the views families name the plain entry, the mixed
    family _mixed_labels from _mixed_labels on, and the two plain mixed
    entries themselves (_mixed_crops without crops: _mixed)."""
    family, takes = ENTRIES[entry]
    for out, suffix in (("box_stats", "_box_stats"), ("box_pal", "_box_palettes"), ("labels", "_labels")):
        if out in present:
            return STEM + family + suffix
    if family != "mixed":
        return STEM + family
    if takes:
        return STEM + "mixed_labels"
    return STEM + ("mixed_crops" if entry.endswith("_crops") and crops else "mixed")


def _garbage(n):
    from photohive_dsp_amd.structures import PhdBoxPalette, PhdBoxStats, RGB_Statistics
    bp, bs = (PhdBoxPalette * n)(), (PhdBoxStats * n)()
    for i in range(n):
        bp[i].n_boxes, bp[i].n_slots = 7 + i, 9 + i
        bp[i].counts = ctypes.cast(V(0x1000), P(ctypes.c_uint32))
        bs[i].n_boxes = 5 + i
        bs[i].stats = ctypes.cast(V(0x2000), P(RGB_Statistics))
        bs[i].average_saturation = ctypes.cast(V(0x3000), P(ctypes.c_double))
    return bp, bs


def _addr(p):
    return ctypes.cast(p, V).value


def _bp_state(bp):
    return [(b.n_boxes, b.n_slots, _addr(b.counts)) for b in bp]


def _bs_state(bs):
    return [(b.n_boxes, _addr(b.stats), _addr(b.average_saturation)) for b in bs]


def _call(entry, head, cfg, crops, present, bp, bs, outs, st):
    """The C entry with the outputs in `present` non-NULL (a fake map array)."""
    family, takes = ENTRIES[entry]
    maps = (V * 2)(0x4000, 0x8000)
    given = {"labels": maps, "box_pal": bp, "box_stats": bs}
    args = list(head) + [ctypes.byref(cfg)]
    if entry != STEM + "mixed":
        args.append(crops)
    args += [given[o] if o in present else None for o in takes]
    return getattr(_L().lib, entry)(*args, outs, st, None)


def _cases():
    for entry, (family, takes) in ENTRIES.items():
        for k in range(len(takes) + 1):
            for present in itertools.combinations(takes, k):
                for crops in ((False, True) if entry == STEM + "mixed_crops" else (False,)):
                    yield pytest.param(entry, present, crops, id="-".join(
                        [entry[len(STEM):], "+".join(present) or "none"] + ["crops"] * crops))


def test_the_table_covers_every_report_entry():
    import os
    import re
    from tests.conftest import ROOT
    with open(os.path.join(ROOT, "include", "photohive_dsp.h")) as f:
        declared = set(re.findall(r"\bint (phd_report_batch_device_(?:mixed|views|typed_views|yuv)\w*)\(", f.read()))
    assert declared == set(ENTRIES) and len(ENTRIES) == 17      # sixteen with crops, and the plain _mixed


@pytest.mark.parametrize("entry,present,crops", list(_cases()))
def test_name_and_reset(entry, present, crops):
    """A NULL first argument with n_images = 2: -1, "<name>: bad arguments",
    the structs that were passed zeroed, the others untouched."""
    from photohive_dsp_amd.core import make_config
    from photohive_dsp_amd.structures import Crop_Boundaries, Full_Report_Data
    L = _L()
    family = ENTRIES[entry][0]
    n = 2
    hs, ws = (I * n)(400, 400), (I * n)(400, 400)
    head = (None, hs, ws, n) if family == "mixed" else (None, n)
    bp, bs = _garbage(n)
    bp0, bs0 = _bp_state(bp), _bs_state(bs)
    outs, st = (P(Full_Report_Data) * n)(), (I * n)()
    boxes = (P(Crop_Boundaries) * n)() if crops else None
    assert _call(entry, head, make_config(), boxes, present, bp, bs, outs, st) == -1
    assert L.last_error() == expected_name(entry, present, crops) + ": bad arguments"
    assert _bp_state(bp) == ([(0, 0, None)] * n if "box_pal" in present else bp0)
    assert _bs_state(bs) == ([(0, None, None)] * n if "box_stats" in present else bs0)


def _descriptors(family, n):
    """Valid descriptors of 400 x 400 images at fake device addresses."""
    from photohive_dsp_amd.structures import (PHD_ELEM_U8, PHD_YUV_BT601, PHD_YUV_CHROMA_REPLICATE, PHD_YUV_FULL,
                                              PhdImageView, PhdTypedView, PhdYuvView)
    if family == "mixed":
        return ((V * n)(*[0x100000 * (i + 1) for i in range(n)]), (I * n)(*[400] * n), (I * n)(*[400] * n), n), None
    if family == "views":
        views = (PhdImageView * n)(*[PhdImageView(0x100000 * (i + 1), 400, 400, 1200, 3, 1) for i in range(n)])
    elif family == "typed_views":
        views = (PhdTypedView * n)(*[PhdTypedView(0x100000 * (i + 1), 400, 400, 1200, 3, 1, PHD_ELEM_U8, 0, 0.0)
                                     for i in range(n)])
    else:
        views = (PhdYuvView * n)(*[PhdYuvView(0x100000 * (i + 1), 0x100000 * (i + 1) + 160000,
                                              0x100000 * (i + 1) + 320000, 400, 400, 400, 1, 400, 1, 0, 0,
                                              PHD_YUV_BT601, PHD_YUV_FULL, PHD_YUV_CHROMA_REPLICATE)
                                   for i in range(n)])
    return (views, n), views


# make_grid (phd_palette.cpp): tl = h_partitions * s_partitions * v_partitions +
# v_partitions + 1 octree groups.  32 * 32 * 32 + 32 + 1 = 32801 >= 32768, and the
# rule is checked before validate_config looks at anything else.
_BIG_GRID = dict(h_partitions=32, s_partitions=32, v_partitions=32)
_RULE = ": label maps need fewer than 32768 octree groups (palette slots)"


@pytest.mark.parametrize("entry", [e for e, (_, takes) in ENTRIES.items() if takes])
def test_label_slots_rule(entry):
    """>= 32768 octree groups: a call given labels or box palettes fails on the
    rule before any HIP call; box statistics alone pass it."""
    import torch
    from photohive_dsp_amd.core import make_config
    from photohive_dsp_amd.structures import Full_Report_Data
    L = _L()
    family, takes = ENTRIES[entry]
    n = 2
    cfg = make_config(**_BIG_GRID)
    assert cfg.h_partitions * cfg.s_partitions * cfg.v_partitions + cfg.v_partitions + 1 >= 32768
    head, keep = _descriptors(family, n)
    for k in range(1, len(takes) + 1):
        for present in itertools.combinations(takes, k):
            bp, bs = _garbage(n)
            outs, st = (P(Full_Report_Data) * n)(), (I * n)()
            if present == ("box_stats",):
                if torch.cuda.is_available():
                    continue                                  # (with a device the call would go on to read the images)
                assert _call(entry, head, cfg, None, present, bp, bs, outs, st) == -1
                assert "no HIP device" in L.last_error()
                continue
            assert _call(entry, head, cfg, None, present, bp, bs, outs, st) == -1
            assert L.last_error() == expected_name(entry, present, False) + _RULE
    del keep


def _prototypes():
    from photohive_dsp_amd.structures import (Crop_Boundaries, Full_Report_Data, PhdBoxPalette, PhdBoxStats, PhdConfig,
                                              PhdImageView, PhdTypedView, PhdYuvView)
    C, CB, BP, BS, O, S = P(PhdConfig), P(P(Crop_Boundaries)), P(PhdBoxPalette), P(PhdBoxStats), \
        P(P(Full_Report_Data)), P(I)
    IV, TV, YV = P(PhdImageView), P(PhdTypedView), P(PhdYuvView)
    return {
        STEM + "mixed": [V, V, V, I, C, V, V, V],
        STEM + "mixed_crops": [V, V, V, I, C, CB, V, V, V],
        STEM + "mixed_labels": [V, V, V, I, C, CB, V, V, V, V],
        STEM + "mixed_box_palettes": [V, V, V, I, C, CB, V, BP, V, V, V],
        STEM + "mixed_box_stats": [V, V, V, I, C, CB, V, BP, BS, V, V, V],
        STEM + "views": [IV, I, C, CB, O, S, V],
        STEM + "views_labels": [IV, I, C, CB, V, O, S, V],
        STEM + "views_box_palettes": [IV, I, C, CB, V, BP, O, S, V],
        STEM + "views_box_stats": [IV, I, C, CB, V, BP, BS, O, S, V],
        STEM + "typed_views": [TV, I, C, CB, O, S, V],
        STEM + "typed_views_labels": [TV, I, C, CB, V, O, S, V],
        STEM + "typed_views_box_palettes": [TV, I, C, CB, V, BP, O, S, V],
        STEM + "typed_views_box_stats": [TV, I, C, CB, V, BP, BS, O, S, V],
        STEM + "yuv": [YV, I, C, CB, O, S, V],
        STEM + "yuv_labels": [YV, I, C, CB, V, O, S, V],
        STEM + "yuv_box_palettes": [YV, I, C, CB, V, BP, O, S, V],
        STEM + "yuv_box_stats": [YV, I, C, CB, V, BP, BS, O, S, V],
    }


def test_prototypes():
    lib = _L().lib
    table = _prototypes()
    assert set(table) == set(ENTRIES)
    for name, argtypes in table.items():
        f = getattr(lib, name)
        assert f.restype is I, name
        assert list(f.argtypes) == argtypes, name


# ---- the Python wrappers' input checks ---------------------------------------------
_PLAIN = "expected contiguous uint8 [H, W, 3] device tensors"
_NONEMPTY = "expected contiguous, non-empty uint8 [H, W, 3] device tensors"
_BATCH = "expected a uint8 [N, H, W, 3] device tensor or a list of [H, W, 3] tensors"


def _raises(text, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert str(e.value) == text


def _bad_images(torch):
    """(what, images) that every packed-image validator refuses."""
    good = torch.zeros((8, 8, 3), dtype=torch.uint8)
    return [("dtype", [good, torch.zeros((8, 8, 3), dtype=torch.float32)]),
            ("int8", [torch.zeros((8, 8, 3), dtype=torch.int8)]),
            ("non-contiguous", [torch.zeros((8, 3, 8), dtype=torch.uint8).permute(0, 2, 1)]),
            ("2-D in a list", [torch.zeros((8, 8), dtype=torch.uint8)]),
            ("4 channels", [torch.zeros((8, 8, 4), dtype=torch.uint8)]),
            ("no tensor", [good.numpy()])]


def test_reports_device_labels_validation():
    import torch
    import photohive_dsp_amd as phd
    for what, images in _bad_images(torch):
        _raises(_PLAIN, phd.reports_device_labels, images)
    # one tensor must be a batch; a 4-D one is taken as its images
    _raises(_BATCH, phd.reports_device_labels, torch.zeros((8, 8), dtype=torch.uint8))
    _raises(_BATCH, phd.reports_device_labels, torch.zeros((8, 8, 3), dtype=torch.uint8))
    _raises(_PLAIN, phd.reports_device_labels, torch.zeros((2, 8, 8, 4), dtype=torch.uint8))
    good = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    _raises("salient_characters has 1 entries for 2 images", phd.reports_device_labels, good,
            salient_characters=[None])
    with pytest.raises(TypeError, match="unknown parameters"):
        phd.reports_device_labels(good, no_such_parameter=1)
    # no images: empty results before anything touches a device
    assert phd.reports_device_labels([]) == ([], [])
    assert phd.reports_device_labels([], box_palettes=True) == ([], [], [])
    assert phd.reports_device_labels([], box_palettes=True, box_stats=True) == ([], [], [], [])
    assert phd.reports_device_labels([], box_stats=True) == ([], [], [])


@pytest.mark.parametrize("fn", ["box_stats_device", "blur_windows_device"])
def test_host_result_wrappers_validation(fn):
    """box_stats_device and blur_windows_device: empty tensors are refused, CPU
    tensors are not (the library would say)."""
    import torch
    import photohive_dsp_amd as phd
    f = getattr(phd, fn)
    for what, images in _bad_images(torch):
        _raises(_NONEMPTY, f, images, None)
    _raises(_NONEMPTY, f, [torch.zeros((0, 8, 3), dtype=torch.uint8)], None)
    _raises(_NONEMPTY, f, torch.zeros((2, 8, 8, 4), dtype=torch.uint8), None)
    # (a tensor that is no batch is iterated: its rows are 2-D)
    _raises(_NONEMPTY, f, torch.zeros((8, 8, 3), dtype=torch.uint8), None)
    good = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    _raises("salient_characters has 1 entries for 2 images" if fn == "box_stats_device"
            else "windows has 1 entries for 2 images", f, good, [None])
    assert f([], None) == []


@pytest.mark.parametrize("fn", ["blur_vectors_device", "blur_vector_maps_device"])
def test_device_result_wrappers_validation(fn):
    """The blur vector wrappers allocate their results on the images' device: a
    CPU tensor is refused with the others."""
    import torch
    import photohive_dsp_amd as phd
    f = getattr(phd, fn)
    rest = (None,) if fn == "blur_vectors_device" else ()
    for what, images in _bad_images(torch):
        _raises(_NONEMPTY, f, images, *rest)
    _raises(_NONEMPTY, f, [torch.zeros((0, 8, 3), dtype=torch.uint8)], *rest)
    _raises(_NONEMPTY, f, [torch.zeros((8, 8, 3), dtype=torch.uint8)], *rest)              # a CPU tensor
    _raises(_NONEMPTY, f, torch.zeros((2, 8, 8, 3), dtype=torch.uint8), *rest)
    if fn == "blur_vectors_device":
        _raises("windows has 1 entries for 0 images", f, [], [None])
    assert f([], *rest) == []
