"""Box statistics: the exact expectations for 8-bit images in Python integers,
a numpy restatement for doubles, the seeded box lists, the fixtures of
tests/golden/make_box_stats_golden.py and the tolerances, shared by
tests/test_box_stats_host.py (no GPU) and tests/test_gpu_box_stats.py."""
import ctypes
import json
import math
import os

import numpy as np

from tests.box_palette_cases import crop_boundaries  # noqa: F401  (re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
BAND = 65536          # box_tiles.h: kBoxBandElems, the pixels of one item
REC = 264             # box_stat_tiles.h: kBoxStatRec = M[6], n1, N, D[256]
TIGHT_RTOL = 1e-9     # tests/test_gpu_parity.py's


# ---- 8-bit images: exact integers ---------------------------------------------------
def expected_sums(img, boxes):
    """Per box (top, bottom, left, right) the record of the definition as Python
    integers: M[6] (sum k, sum k^2 per channel), n1 = #(min == 0 < max), N,
    D[256] (sum of max - min over the pixels whose max is m)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    out = []
    for t, bo, l, r in boxes:
        c = img[t:bo, l:r].reshape(-1, 3).astype(np.int64)
        mx, mn = c.max(axis=1), c.min(axis=1)
        d = np.zeros(256, np.int64)
        np.add.at(d, mx, mx - mn)
        rec = [int(v) for v in c.sum(axis=0)] + [int(v) for v in (c * c).sum(axis=0)]
        rec += [int(np.count_nonzero((mn == 0) & (mx > 0))), int(c.shape[0])] + [int(v) for v in d]
        assert len(rec) == REC
        out.append(rec)
    return out


def finish(rec):
    """The definition's finish of one record: (Br Bg Bb Cr Cg Cb, S-bar).  The
    moments as stats_from_sums (phd_assemble.cpp) forms them, S ascending and
    sequential."""
    m, n1, n, d = rec[:6], rec[6], rec[7], rec[8:]
    st = [float(m[c]) / 255.0 / float(n) for c in range(3)]
    for c in range(3):
        num = n * m[3 + c] - m[c] * m[c]                     # exact (128 bits in C)
        st.append(math.sqrt(float(num) / 65025.0 / (float(n) * float(n))))
    s = 0.0
    for k in range(1, 256):
        s += float(d[k]) / float(k)
    return st, (s - (1.0 - 0.999999) * float(n1)) / float(n)


def expected_u8(img, boxes):
    """float64 [n_boxes, 7]: Br Bg Bb Cr Cg Cb S-bar of the definition."""
    out = np.zeros((len(boxes), 7))
    for k, rec in enumerate(expected_sums(img, boxes)):
        st, sbar = finish(rec)
        out[k, :6], out[k, 6] = st, sbar
    return out


# ---- doubles: a numpy restatement ------------------------------------------------------
def saturation(x):
    """rgb2hsv's s (src/image_processing.c:408-414) of float64 [..., 3]."""
    mx, mn = x.max(axis=-1), x.min(axis=-1)
    d = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(mx == 0, 0.0, np.where(d == mx, 0.999999, d / np.where(mx == 0, 1.0, mx)))
    return s


def expected_doubles(img, boxes):
    """get_rgb_statistics and get_hsv_average on the crop of float64 [H, W, 3]
    (mean sum / N, the variance's second pass, s per pixel), in numpy's own
    summation order."""
    out = np.zeros((len(boxes), 7))
    for k, (t, bo, l, r) in enumerate(boxes):
        c = np.asarray(img, np.float64)[t:bo, l:r].reshape(-1, 3)
        n = float(c.shape[0])
        mean = c.sum(axis=0) / n
        out[k, :3] = mean
        out[k, 3:6] = np.sqrt(((c - mean) ** 2).sum(axis=0) / n)
        out[k, 6] = saturation(c).sum() / n
    return out


# ---- tolerances (the issue's, all taken from the project) ----------------------------------
def assert_close(got, want, boxes, what=""):
    """got, want: [n_boxes, 7].  Means and contrasts rtol TIGHT_RTOL, the contrasts
    also atol max(1e-12, N 2^-53); S-bar rtol max(1e-12, N 2^-53)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == (len(boxes), 7), (got.shape, want.shape)
    for k, (t, bo, l, r) in enumerate(boxes):
        n = (bo - t) * (r - l)
        tol = max(1e-12, n * 2.0 ** -53)
        np.testing.assert_allclose(got[k, :3], want[k, :3], rtol=TIGHT_RTOL, atol=0, err_msg=f"{what} box {k} mean")
        np.testing.assert_allclose(got[k, 3:6], want[k, 3:6], rtol=TIGHT_RTOL, atol=tol,
                                   err_msg=f"{what} box {k} contrast")
        np.testing.assert_allclose(got[k, 6], want[k, 6], rtol=tol, atol=0, err_msg=f"{what} box {k} S-bar")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- boxes -----------------------------------------------------------------------------------
def box_list(h, w, seed, extra=4):
    """Boxes (top, bottom, left, right) of an h x w image: always the whole image,
    a 1 x 1 box, a one-row and a one-column box, `left` = 0, 1, 2, 3 (mod 4),
    widths 1..9, two overlapping boxes, the bottom-right corner and, where the
    image has more than BAND pixels, one box above BAND pixels (several bands);
    then `extra` random ones.  No box is empty (the rule of the report's crops)."""
    rng = np.random.default_rng(seed)
    boxes = [(0, h, 0, w), (h // 2, h // 2 + 1, w // 3, w // 3 + 1), (h // 3, h // 3 + 1, 0, w),
             (0, h, w // 2, w // 2 + 1)]
    for ph in range(4):                                       # every phase of left
        l = min(4 * ((w // 5) // 4) + ph, w - 1)
        boxes.append((0, min(h, 3), l, min(w, l + 6)))
    for wd in range(1, 10):                                   # widths 1..9: 0..2 units and every tail
        if wd <= w:
            l = min(w - wd, 1 + wd)
            boxes.append((max(0, h - 5), h, l, l + wd))
    if h >= 4 and w >= 4:
        boxes += [(h // 4, 3 * h // 4, w // 4, 3 * w // 4), (h // 2, h, w // 2, w)]   # overlap; the corner
    boxes.append((h - 1, h, w - 1, w))
    if h * w > BAND:
        boxes.append((1, h, 1, w))                            # several bands
        assert (h - 1) * (w - 1) > BAND
    for _ in range(extra):
        t, l = int(rng.integers(0, h)), int(rng.integers(0, w))
        boxes.append((t, int(rng.integers(t + 1, h + 1)), l, int(rng.integers(l + 1, w + 1))))
    assert all(0 <= t < bo <= h and 0 <= l < r <= w for t, bo, l, r in boxes)
    return boxes


def random_image(h, w, seed):
    """uint8 [h, w, 3] with every case of the saturation formula: random colours,
    greys (d == 0), black (max == 0) and pixels with a zero channel (min == 0 <
    max, the 0.999999 path), in runs."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    u = rng.random((h, w))
    img[u < 0.1] = img[u < 0.1][:, :1]                        # grey
    img[(u >= 0.1) & (u < 0.15)] = 0                          # black
    z = (u >= 0.15) & (u < 0.3)
    ch = rng.integers(0, 3, size=int(z.sum()))
    px = img[z]
    px[np.arange(len(ch)), ch] = 0
    img[z] = px
    img[(u >= 0.3) & (u < 0.33)] = 255
    return img


def at_offset(img, off):
    """A copy of the image whose base is `off` bytes past a 4-byte boundary."""
    buf = np.zeros(img.size + 8, np.uint8)
    k = next(j for j in range(4) if (buf.ctypes.data + j) % 4 == off % 4)
    v = buf[k:k + img.size].reshape(img.shape)
    v[...] = img
    assert v.ctypes.data % 4 == off % 4
    return v


# ---- the host twin ----------------------------------------------------------------------------
def host_twin(img, boxes, want_sums=True):
    """phd_debug_box_stats_host over a uint8 image at any base: ([n, 7] values,
    [n][264] sums as Python integers or None)."""
    from photohive_dsp_amd import lib as L
    assert img.dtype == np.uint8 and img.flags.c_contiguous
    cb, keep = crop_boundaries(boxes)
    n = len(boxes)
    st = np.full((max(n, 1), 6), np.nan)
    sb = np.full(max(n, 1), np.nan)
    sums = np.full((max(n, 1), REC), 0xDEADBEEF, np.uint64)
    rc = L.lib.phd_debug_box_stats_host(img.ctypes.data, img.shape[0], img.shape[1], ctypes.byref(cb), st.ctypes.data,
                                        sb.ctypes.data, sums.ctypes.data if want_sums else None)
    assert rc == 0, L.last_error()
    del keep
    out = np.concatenate([st[:n], sb[:n, None]], axis=1)
    return out, ([[int(v) for v in row] for row in sums[:n]] if want_sums else None)


# ---- fixtures from the compiled reference --------------------------------------------------------
def manifest():
    with open(os.path.join(GOLDEN, "box_stats_manifest.json")) as f:
        return json.load(f)["cases"]


def fixture(name):
    """boxes int32 [n, 4] (top, bottom, left, right), stats [n, 6], average_saturation [n]."""
    with np.load(os.path.join(GOLDEN, f"box_stats_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture_values(fx):
    return np.concatenate([fx["stats"], fx["average_saturation"][:, None]], axis=1)


def special_image(h=350, w=351):
    """The special-pattern image and its boxes: a constant box (the contrast
    floor), an all-black box (S-bar 0), an all-white box (max 255, d 0), a
    pure-primary box (d == max: the 0.999999 path), on a random ground."""
    img = random_image(h, w, 77)
    boxes = [(10, 74, 10, 74), (100, 140, 33, 98), (150, 181, 201, 263), (200, 333, 7, 70), (0, h, 0, w),
             (5, 120, 5, 120)]
    img[10:74, 10:74] = (37, 121, 200)
    img[100:140, 33:98] = 0
    img[150:181, 201:263] = 255
    img[200:333, 7:70] = (0, 0, 255)
    img[200:266, 7:40] = (255, 0, 0)
    return img, boxes


def case_image(case):
    """The image of a manifest case: uint8 [H, W, 3], or float64 for a deep one."""
    from photohive_dsp_amd import synth
    if case["kind"] == "special":
        return special_image(case["height"], case["width"])[0]
    if case["deep"]:
        return synth.deep(case["kind"], case["height"], case["width"], case["seed"])
    return synth.make(case["kind"], case["height"], case["width"], case["seed"])


def case_boxes(case):
    if case["kind"] == "special":
        return special_image(case["height"], case["width"])[1]
    return box_list(case["height"], case["width"], case["seed"] + 1000)
