"""Palette label map fixtures from the reference's own C (oracle/_ref, this
container only): tests/golden/labels_<name>.npz and labels_manifest.json.

    python -m tests.golden.make_label_golden

The reference's list nodes hold copies of Pixel_HSV, whose parent_id rgb2hsv
leaves zero (calloc) and nothing reads.  So the raster index of every pixel is
written there after rgb2hsv, the reference runs initialize_octree, arm_octree,
find_valid_octree_parents and group_irregular_pixels
(src/color_quantization.c:22-479), and each valid parent's list is walked: the
indices read back are the reference's label map, with no restatement.

Asserted before anything is written: every pixel is in at most one list; per
slot percentages[i] == (double)count * (1.0 / (double)n) bit for bit; the kept
pixels of one arm_octree group carry one label; a group's drops are its pixels
after the first `keep` in raster order, except possibly its last pixel;
oracle.group_ids equals the reference's grouping per pixel; and
tests/label_cases.py's hsv_image equals downsample_rgb's image.  The fixtures
are compact (tests/label_cases.py) and the rebuilt map's SHA-256 is checked."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as orc  # noqa: E402
from oracle import ref_pipeline as rp  # noqa: E402
from photohive_dsp_amd import synth  # noqa: E402
from tests import label_cases as lc  # noqa: E402

PIXEL = np.dtype([("parent_id", "<i4"), ("pad", "<i4"), ("h", "<f8"), ("s", "<f8"), ("v", "<f8")])
assert PIXEL.itemsize == C.sizeof(rp.Pixel_HSV)


def _pixels(ptr, n):
    """n Pixel_HSV at ptr as a structured array over the reference's memory."""
    buf = C.cast(ptr, C.POINTER(C.c_char * (PIXEL.itemsize * n))).contents
    return np.frombuffer(buf, dtype=PIXEL, count=n)


def _walk(group):
    """The raster indices (parent_id) of the pixels in a group's list."""
    out = []
    node = group.head
    while node:
        k = node.contents.num_pixels
        if k:
            out.append(_pixels(node.contents.pixels, k)["parent_id"].copy())
        node = node.contents.next
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int32)


def reference_labels(img, cfg):
    """(label map uint16 [mh, mw], reference group per pixel, percentages,
    the image rgb2hsv saw as uint8) of one image."""
    L = rp.lib()
    im, _keep = rp._image_rgb(img)
    pim = C.pointer(im)
    assert not L.pre_compute_error_checks(pim)
    ds = L.downsample_rgb(pim, cfg.downsample_rate) if cfg.downsample_rate > 1 else pim
    mh, mw = ds.contents.height, ds.contents.width
    n = mh * mw
    small = np.stack([np.rint(np.ctypeslib.as_array(getattr(ds.contents, c), shape=(n,)) * 255.0)
                      for c in "rgb"], axis=-1).astype(np.uint8).reshape(mh, mw, 3)
    hsv = L.rgb2hsv(ds)
    px = _pixels(hsv.contents.pixels, n)
    assert not px["parent_id"].any()                        # calloc'd, unused
    px["parent_id"] = np.arange(n, dtype=np.int32)
    C.c_float.in_dll(L, "QUANTITY_WEIGHT").value = cfg.quantity_weight
    C.c_float.in_dll(L, "SATURATION_VALUE_WEIGHT").value = cfg.saturation_value_weight
    oc = L.initialize_octree(cfg.h_partitions, cfg.s_partitions, cfg.v_partitions, cfg.black_thresh,
                             cfg.gray_thresh)
    L.arm_octree(hsv, oc, cfg.linked_list_size)
    tl = oc.contents.total_length
    ref_gid = np.full(n, -1, dtype=np.int32)
    for g in range(tl):
        idx = _walk(oc.contents.groups[g])
        assert (ref_gid[idx] == -1).all()
        ref_gid[idx] = g
    assert (ref_gid >= 0).all()
    L.find_valid_octree_parents(oc, n, cfg.coverage_thresh)
    nvp = oc.contents.len_valid_parents
    vp = [oc.contents.valid_parents[i] for i in range(nvp)]
    L.group_irregular_pixels(oc)
    lab = np.full(n, lc.NONE, dtype=np.uint16)
    for i, p in enumerate(vp):
        idx = _walk(oc.contents.groups[int(p)])
        assert (lab[idx] == lc.NONE).all() and len(np.unique(idx)) == len(idx), "a pixel is in two lists"
        lab[idx] = i
    cp = L.calculate_avg_hsv(oc, hsv)
    pct = np.array([cp.contents.percentages[i] for i in range(cp.contents.N)])
    L.free_color_palette(cp)
    L.free_octree(oc)
    L.free_image_hsv(hsv)
    if cfg.downsample_rate > 1:
        L.free_image_rgb(ds)
    return lab.reshape(mh, mw), ref_gid, pct, small


def compact(name, kind, h, w, seed, kw):
    img = synth.make(kind, h, w, seed)
    cfg = rp.Config(**kw)
    lab, ref_gid, pct, small = reference_labels(img, cfg)
    n = lab.size
    flat = lab.reshape(-1)
    assert lab.shape == lc.map_shape(h, w, cfg.downsample_rate)
    assert np.array_equal(small, lc.hsv_image(img, cfg.downsample_rate)), "hsv_image differs from downsample_rgb"
    gid = orc.group_ids(np.ascontiguousarray(small), **{k: v for k, v in kw.items() if k != "downsample_rate"})
    assert np.array_equal(gid, ref_gid), "oracle.group_ids differs from the reference's grouping"
    counts = lc.slot_counts(flat, len(pct))
    assert np.array_equal(lc.percentages(counts, n).view(np.int64), pct.view(np.int64)), "count identity"
    tl = cfg.h_partitions * cfg.s_partitions * cfg.v_partitions + cfg.v_partitions + 1   # initialize_octree, :27-29
    assert int(ref_gid.max()) < tl
    group_slot = np.full(tl, -1, dtype=np.int16)
    dangling = 0
    for g in np.unique(ref_gid):
        idx = np.flatnonzero(ref_gid == g)                   # raster order
        kept = flat[idx] != lc.NONE
        if not kept.any():
            continue
        slots = np.unique(flat[idx][kept])
        assert len(slots) == 1, f"group {g} kept under {len(slots)} labels"
        group_slot[g] = slots[0]
        if kept.all():
            continue
        keep = int(np.argmin(kept))                          # the first dropped pixel's rank
        tail = kept[keep:]
        assert not tail[:-1].any(), f"group {g}: a pixel after the first {keep} is kept that is not the last"
        dangling += int(tail[-1])
    dropped = np.flatnonzero(flat == lc.NONE).astype(np.uint32)
    fx = dict(group_slot=group_slot, dropped=dropped, shape=np.array(lab.shape, dtype=np.int32),
              counts=counts.astype(np.int64), sha256=np.frombuffer(lc.map_sha256(lab), dtype=np.uint8))
    case = dict(name=name, kind=kind, height=h, width=w, seed=seed, config=kw)
    rebuilt = lc.expected_map(case, fx, img)
    assert np.array_equal(rebuilt, lab) and lc.map_sha256(rebuilt) == lc.map_sha256(lab)
    print(f"{name}: map {lab.shape}, {len(pct)} slots, {len(dropped)} dropped, {dangling} dangling kept", flush=True)
    return fx


def main():
    cases = []
    for name, kind, h, w, seed, kw, base in lc.CASES:
        fx = compact(name, kind, h, w, seed, kw)
        np.savez_compressed(os.path.join(HERE, f"labels_{name}.npz"), **fx)
        cases.append(dict(name=name, kind=kind, height=h, width=w, seed=seed, config=kw, base=base))
    with open(os.path.join(HERE, "labels_manifest.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
