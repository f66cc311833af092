"""Typed-view cases shared by tests/test_typed_views.py (host twin) and
tests/test_gpu_typed_views.py (kernels): every element type of the descriptor
(include/photohive_dsp.h: phd_typed_view) in the layouts of its table, as
element strides over an exactly sized buffer, and the decode numpy takes from
the same strides: value = (double)element / max_value, the 8-bit rule of
k_planar_to_u8 (value == j / 255.0) and the snap tables."""
import numpy as np

U8, U16, F16, F32, F64 = range(5)
SNAP = 1
# elem -> (name, storage dtype, value dtype, the type's own maximum)
ELEMS = {
    U8: ("u8", np.uint8, np.uint8, 255.0),
    U16: ("u16", np.uint16, np.uint16, 65535.0),
    F16: ("f16", np.uint16, np.float16, 1.0),
    F32: ("f32", np.uint32, np.float32, 1.0),
    F64: ("f64", np.uint64, np.float64, 1.0),
}

# name -> f(H, W, extra) = (row, pixel, channel) strides in ELEMENTS; extra widens the pitch
LAYOUTS = {
    "hwc": lambda h, w, e: (3 * w, 3, 1),                           # packed
    "hwc_pitched": lambda h, w, e: (3 * w + 1 + e, 3, 1),
    "rgba": lambda h, w, e: (4 * w + e, 4, 1),
    "bgr": lambda h, w, e: (3 * w + e, 3, -1),                      # data at the R element (+2)
    "bgra": lambda h, w, e: (4 * w + e, 4, -1),
    "chw": lambda h, w, e: (w, 1, w * h),                           # packed planes
    "chw_pitched": lambda h, w, e: (w + 3 + e, 1, (w + 3 + e) * h + e),
    "roi_hwc": lambda h, w, e: (3 * (w + 9) + e, 3, 1),             # t[5:-3, 7:-2] of a larger frame
    "roi_chw": lambda h, w, e: (w + 9 + e, 1, (w + 9 + e) * (h + 8)),
    "gray": lambda h, w, e: (w + e, 1, 0),                          # an expanded grey plane
    "chw_flipped": lambda h, w, e: (-(w + e), 1, (w + e) * h),      # negative row stride
    "hwc_mirrored": lambda h, w, e: (3 * w + e, -3, 1),             # the generic kind
}

SHAPES = [(1, 1), (1, 7), (5, 1), (3, 5), (37, 61), (64, 64)]
OFFSETS = (0, 1, 2, 3)
MAX_VALUES = (0.0, 1023.0, 255.0)


def snap_table(elem):
    """(T)((double)j / 255.0) for j in 0..255 as values of the element type."""
    return (np.arange(256, dtype=np.float64) / 255.0).astype(ELEMS[elem][2])


def fill(elem, count, rng):
    """count storage words: random bit patterns of the whole type, with runs of
    table entries, exact 8-bit values and values in [0, 1] among them."""
    _, store, val, _ = ELEMS[elem]
    bits = rng.integers(0, np.iinfo(store).max, count, dtype=store, endpoint=True)
    if elem in (F16, F32, F64):
        pick = rng.random(count)
        tab = snap_table(elem).view(store)
        j = rng.integers(0, 256, count)
        bits = np.where(pick < 0.3, tab[j], bits)
        unit = rng.random(count).astype(val).view(store)
        bits = np.where((pick >= 0.3) & (pick < 0.5), unit, bits)
    elif elem == U16:
        pick = rng.random(count)
        bits = np.where(pick < 0.3, (rng.integers(0, 256, count) * 257).astype(store), bits)
        bits = np.where((pick >= 0.3) & (pick < 0.5), rng.integers(0, 1024, count).astype(store), bits)
    return bits.astype(store)


def typed_case(elem, layout, h, w, off, extra=0, seed=0, bits=None):
    """(buf, data_off, (rs, ps, cs), raw): buf holds off + span storage words,
    the view's lowest addressed element at buf[off] and its highest at buf[-1];
    data (element R of pixel (0, 0)) is buf[data_off]; strides in BYTES; raw is
    the gathered [h, w, 3] array of storage words.  bits: a fill to use instead
    of the random one (cycled over the span)."""
    _, store, _, _ = ELEMS[elem]
    rs, ps, cs = LAYOUTS[layout](h, w, extra)
    corners = [y * rs + x * ps + c * cs for y in (0, h - 1) for x in (0, w - 1) for c in (0, 2)]
    lo, hi = min(corners), max(corners)
    span = hi - lo + 1
    rng = np.random.default_rng(seed * 1000003 + elem * 977 + h * 131 + w * 7 + off * 3 + extra)
    buf = fill(elem, off + span, rng) if bits is None else np.resize(bits, off + span).astype(store)
    data_off = off - lo
    es = buf.itemsize
    strides = (rs * es, ps * es, cs * es)
    raw = np.lib.stride_tricks.as_strided(buf[data_off:], shape=(h, w, 3), strides=strides, writeable=False)
    return buf, data_off, strides, np.ascontiguousarray(raw)


def decode(elem, raw, max_value=0.0, snap=False):
    """The decode of a gathered [h, w, 3] array of storage words: (planes
    [3, h, w] float64, rgb8 [h, w, 3] uint8, is_u8)."""
    _, _, val, own = ELEMS[elem]
    mv = max_value if max_value else own
    x = raw.view(val)
    with np.errstate(all="ignore"):
        v = x.astype(np.float64) / mv
        inside = (v >= 0.0) & (v <= 1.0)
        k = np.where(inside, np.rint(np.where(inside, v, 0.0) * 255.0), 0.0).astype(np.int64)
        is8 = inside & (k / 255.0 == v)
        if snap and elem in (F16, F32) and mv == 1.0:
            is8 |= inside & (snap_table(elem)[k] == x)
    return np.ascontiguousarray(v.transpose(2, 0, 1)), k.astype(np.uint8), bool(is8.all())


def same_doubles(got, want):
    """Bit for bit, NaNs by position."""
    g, w = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
    return bool(((g == w) | (np.isnan(got) & np.isnan(want))).all())
