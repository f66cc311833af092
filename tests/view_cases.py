"""Image-view layouts shared by tests/test_views.py (host twin) and
tests/test_gpu_views.py (pack kernel): every layout of the descriptor's table
(include/photohive_dsp.h: phd_image_view) as byte strides over an exactly
sized buffer, and the packed image numpy takes from the same strides."""
import numpy as np

# name -> f(H, W, extra) = (row_stride, pixel_stride, channel_stride); extra
# widens the pitch beyond its minimum
LAYOUTS = {
    "hwc": lambda h, w, e: (3 * w + e, 3, 1),                       # packed at e == 0, else pitched
    "rgba": lambda h, w, e: (4 * w + e, 4, 1),
    "bgr": lambda h, w, e: (3 * w + e, 3, -1),                      # data at the R byte (+2)
    "bgra": lambda h, w, e: (4 * w + e, 4, -1),                     # data at +2
    "argb": lambda h, w, e: (4 * w + e, 4, 1),                      # data at +1 (same strides as rgba)
    "chw": lambda h, w, e: (w + e, 1, (w + e) * h + e),
    "gray": lambda h, w, e: (w + e, 1, 0),                          # an expanded grey plane
    "roi_hwc": lambda h, w, e: (3 * (w + 9) + e, 3, 1),             # t[5:-3, 7:-2] of a larger frame
    "roi_rgba": lambda h, w, e: (4 * (w + 9) + e, 4, 1),
    "roi_chw": lambda h, w, e: (w + 9 + e, 1, (w + 9 + e) * (h + 8)),
    "chw_flipped": lambda h, w, e: (-(w + e), 1, (w + e) * h),      # rows bottom-up
    "hwc_mirrored": lambda h, w, e: (3 * w + e, -3, 1),             # pixels right to left: the generic kind
    "chw_bgr": lambda h, w, e: (w + e, 1, -(w + e) * h),            # planes in B, G, R order
}

SHAPES = [(1, 1), (1, 5), (3, 4), (5, 7), (17, 67), (16, 64), (33, 129)]
OFFSETS = (0, 1, 2, 3)
PITCH_EXTRA = (0, 1, 4)


def view_case(name, h, w, off, extra, seed=0):
    """(buf, data_off, (rs, ps, cs), want): buf is off + span random bytes, the
    view's lowest addressed byte at buf[off] and its highest at buf[-1]; data
    (the R byte of pixel (0, 0)) is buf[data_off]; want is the packed [h, w, 3]
    image (np.ascontiguousarray of the strided array)."""
    rs, ps, cs = LAYOUTS[name](h, w, extra)
    corners = [y * rs + x * ps + c * cs for y in (0, h - 1) for x in (0, w - 1) for c in (0, 2)]
    lo, hi = min(corners), max(corners)
    span = hi - lo + 1
    rng = np.random.default_rng(seed * 1000003 + h * 131 + w * 7 + off * 3 + extra)
    buf = rng.integers(0, 256, off + span, dtype=np.uint8)
    data_off = off - lo
    strided = np.lib.stride_tricks.as_strided(buf[data_off:], shape=(h, w, 3), strides=(rs, ps, cs), writeable=False)
    return buf, data_off, (rs, ps, cs), np.ascontiguousarray(strided)
