"""Box palettes: the expected counts in plain numpy, the image-to-map box rule
and the box lists and synthetic maps shared by tests/test_box_palettes_host.py
(no GPU) and tests/test_gpu_box_palettes.py."""
import ctypes

import numpy as np

NONE = 0xFFFF
BAND = 65536          # box_tiles.h: kBoxBandElems, the elements of one item


def expected_counts(lab, boxes, n_slots):
    """uint32 [n_boxes, n_slots + 1]: per box (top, bottom, left, right) of map
    coordinates, rows top <= y < bottom and columns left <= x < right, the
    elements of every slot; labels >= n_slots (NONE included) in the last column."""
    lab = np.asarray(lab)
    out = np.zeros((len(boxes), n_slots + 1), np.uint32)
    for b, (t, bo, l, r) in enumerate(boxes):
        part = np.minimum(lab[t:bo, l:r].astype(np.int64).reshape(-1), n_slots)
        out[b] = np.bincount(part, minlength=n_slots + 1)
    return out


def image_to_map_box(box, r, mh, mw):
    """A box of image coordinates on the map of downsample_rate r: the elements
    whose nominal position (y * r, x * r) lies inside it."""
    t, bo, l, rt = box
    if r <= 1:
        return (t, bo, l, rt)
    ceil = lambda v: -(-v // r)                                            # noqa: E731
    t2, l2 = min(ceil(t), mh), min(ceil(l), mw)
    return (t2, max(t2, min(ceil(bo), mh)), l2, max(l2, min(ceil(rt), mw)))


def box_list(h, w, seed, empty=True, extra=6):
    """Boxes of an h x w map (or image): always the whole of it, a 1 x 1 box, a
    one-row and a one-column box, an empty box (stage alone only), odd and even
    `left` and width, two overlapping boxes, a box touching the bottom-right
    corner and, where the map has more than one band of elements, a box cut into
    several bands; then `extra` random ones."""
    rng = np.random.default_rng(seed)
    boxes = [(0, h, 0, w), (h // 2, h // 2 + 1, w // 3, w // 3 + 1), (h // 3, h // 3 + 1, 0, w),
             (0, h, w // 2, w // 2 + 1)]
    if empty:
        boxes += [(h // 2, h // 2, 1 % w, w), (0, h, w, w)]
    if w >= 6 and h >= 4:
        boxes += [(1, h - 1, 1, min(w, 1 + 5)), (1, h - 1, 2, min(w, 2 + 5)), (0, 3, 1, min(w, 1 + 4)),
                  (0, 3, 2, min(w, 2 + 4)),
                  (h // 4, 3 * h // 4, w // 4, 3 * w // 4), (h // 2, h, w // 2, w),     # overlap; the corner
                  (h - 1, h, w - 1, w)]
    for _ in range(extra):
        t, l = int(rng.integers(0, h)), int(rng.integers(0, w))
        boxes.append((t, int(rng.integers(t + 1, h + 1)), l, int(rng.integers(l + 1, w + 1))))
    assert h * w <= BAND or any((bo - t) * (r - l) > BAND for t, bo, l, r in boxes)   # two bands or more
    return boxes


def crop_boundaries(boxes):
    """A Crop_Boundaries of the boxes and the arrays that keep it alive."""
    from photohive_dsp_amd.structures import Crop_Boundaries
    n = len(boxes)
    arrs = [(ctypes.c_int * max(n, 1))(*[b[k] for b in boxes]) for k in range(4)]
    cb = Crop_Boundaries()
    cb.N = n
    cb.top, cb.bottom, cb.left, cb.right = (ctypes.cast(a, ctypes.POINTER(ctypes.c_int)) for a in arrs)
    return cb, arrs


def host_counts(lab, boxes, n_slots):
    """phd_debug_box_counts_host over a uint16 map (any 2-byte aligned base)."""
    from photohive_dsp_amd import lib as L
    assert lab.dtype == np.uint16 and lab.flags.c_contiguous
    cb, keep = crop_boundaries(boxes)
    out = np.full((len(boxes), n_slots + 1), 0xDEADBEEF, np.uint32)
    rc = L.lib.phd_debug_box_counts_host(lab.ctypes.data, lab.shape[0], lab.shape[1], n_slots, ctypes.byref(cb),
                                         out.ctypes.data)
    assert rc == 0, L.last_error()
    del keep
    return out


def at_offset(lab, elems=1):
    """A copy of the map whose base is `elems` uint16 past an 8-byte boundary."""
    buf = np.zeros(lab.size + 8, np.uint16)
    k = next(j for j in range(4) if (buf.ctypes.data // 2 + j) % 4 == elems % 4)
    v = buf[k:k + lab.size].reshape(lab.shape)
    v[...] = lab
    assert (v.ctypes.data % 8) == 2 * (elems % 4)
    return v


def random_map(h, w, n_slots, seed, none=0.05, over=0.05):
    """Random labels in runs (as label maps have them): slots 0 .. n_slots-1,
    some NONE, some labels >= n_slots that are not NONE."""
    rng = np.random.default_rng(seed)
    n = h * w
    lens = rng.integers(1, 12, size=n)
    vals = rng.integers(0, max(n_slots, 1), size=n).astype(np.int64)
    u = rng.random(n)
    vals[u < none] = NONE
    vals[(u >= none) & (u < none + over)] = min(n_slots + int(rng.integers(0, 5)), NONE - 1)
    if n_slots == 0:
        vals[u >= none + over] = 7
    return np.repeat(vals, lens)[:n].astype(np.uint16).reshape(h, w)


# (name, height, width, n_slots): the smallest shapes where the plan can go
# wrong -- one element; a few; a row longer than one pass of a block (7 x 4099);
# an odd width, so every row starts at another 8-byte phase, and more than one
# band (257 x 1031) -- at the slot-count edges
SYNTHETIC = [("1x1", 1, 1, 17), ("3x5", 3, 5, 1), ("7x4099", 7, 4099, 17), ("257x1031", 257, 1031, 17),
             ("257x1031_s4096", 257, 1031, 4096), ("129x1031_s0", 129, 1031, 0), ("64x2050_s1", 64, 2050, 1)]


def synthetic_maps():
    """[(name, map, n_slots, boxes)]: the random maps of SYNTHETIC, one of them
    at base + 2 bytes, a single-label map (every element on one counter) and a
    map that alternates labels every element (no runs to merge)."""
    out = []
    for i, (name, h, w, ns) in enumerate(SYNTHETIC):
        out.append((name, random_map(h, w, ns, 100 + i), ns, box_list(h, w, 200 + i)))
    name, lab, ns, boxes = out[3]
    out.append((name + "_base2", at_offset(lab, 1), ns, boxes))
    h, w = 300, 1030
    out.append(("single_label", np.full((h, w), 3, np.uint16), 17, box_list(h, w, 300)))
    alt = (np.arange(h * w, dtype=np.int64) % 2 * 16).astype(np.uint16).reshape(h, w)
    out.append(("alternating", alt, 17, box_list(h, w, 301)))
    return out
