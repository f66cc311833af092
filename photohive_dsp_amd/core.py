"""Python API: get_report / Report / set_bounding_boxes (as /root/reference/core.py).

Same call signature, defaults, fields and error behaviour as the reference
(core.py:23-119, 388-515); the image goes to the MI355X library as raw RGB8
(phd_report_u8) instead of three planar double arrays.  New: get_reports()
for a list of images and report_device() for RGB8 batches already on the GPU.
GUI display methods (tkinter / matplotlib) are out of scope.
"""
from __future__ import annotations

import ctypes
import json
import os
import time
from ctypes import POINTER
from types import SimpleNamespace

import numpy as np

from .lib import last_error, lib
from .structures import (PHD_ELEM_F16, PHD_ELEM_F32, PHD_ELEM_F64, PHD_ELEM_U8, PHD_ELEM_U16, PHD_VIEW_SNAP_U8,
                         PHD_YUV_BT601, PHD_YUV_BT709, PHD_YUV_CHROMA_REPLICATE, PHD_YUV_CHROMA_TRIANGLE,
                         PHD_YUV_FULL, PHD_YUV_LIMITED, Crop_Boundaries, Full_Report_Data, PhdBoxPalette, PhdBoxStats,
                         PhdConfig, PhdImageView, PhdTypedView, PhdWindowBlur, PhdYuvView, Pixel_HSV, RGB_Statistics)
from .utils import hsv_to_rgb, image_pgm_to_pillow, to_rgb8

DEFAULTS = dict(h_partitions=18, s_partitions=2, v_partitions=3, black_thresh=0.1, gray_thresh=0.1,
                coverage_thresh=0.95, linked_list_size=1000, downsample_rate=1, radius_partitions=40,
                angle_partitions=72, quantity_weight=0.1, saturation_value_weight=0.9,
                fft_streak_thresh=1.20, magnitude_thresh=0.3, blur_cutoff_ratio_denom=2)


def _stream_handle(stream):
    """The hipStream_t a device call runs on: the given torch stream, else
    torch's current stream (its handle 0, the null stream, makes the library
    order its own stream after the null stream's prior work)."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream or None


def make_config(**kw) -> PhdConfig:
    c = dict(DEFAULTS)
    unknown = set(kw) - set(c)
    if unknown:
        raise TypeError(f"unknown parameters {sorted(unknown)}")
    c.update(kw)
    return PhdConfig(**c)


class Report:
    """Report of one image; fields as the reference's Report (core.py:24-119)."""

    def __init__(self, report_ptr, height, width):
        report_data = report_ptr.contents          # NULL -> ValueError, as in the reference
        self.data_ptr = report_ptr
        self.rgb_stats = report_data.rgb_stats.contents
        self.rgb_stats.height = height
        self.rgb_stats.width = width
        self.color_palette = self._convert_color_palette(report_data.color_palette)
        self.blur_profile = self._convert_blur_profile(report_data.blur_profile)
        self.blur_vectors = self._convert_blur_vectors(report_data.blur_vectors)
        self.average_saturation = report_data.average_saturation
        self.sharpnesses = self._convert_sharpnesses(report_data.sharpness)

    @staticmethod
    def _convert_sharpnesses(ptr):
        if not ptr:
            return []
        s = ptr.contents
        return [s.sharpness[i] for i in range(s.N)]

    @staticmethod
    def _convert_blur_vectors(ptr):
        g = ptr.contents
        out = []
        for i in range(g.len_vectors):
            v = SimpleNamespace()
            v.angle = g.blur_vectors[i].angle
            v.magnitude = g.blur_vectors[i].magnitude
            out.append(v)
        return out

    @staticmethod
    def _convert_color_palette(ptr):
        cp = ptr.contents
        averages = ctypes.cast(cp.averages, POINTER(Pixel_HSV * cp.N)).contents if cp.N else []
        cp.colors = [hsv_to_rgb(p.h, p.s, p.v) for p in averages]
        cp.quantities = [cp.percentages[i] for i in range(cp.N)]
        cp.hsv = [(p.h, p.s, p.v) for p in averages]          # new: raw palette HSV
        cp.group_ids = [p.parent_id for p in averages]        # new: octree group of each colour
        return cp

    def _convert_blur_profile(self, ptr):
        c = ptr.contents
        self.bp_ptr = c
        bp = SimpleNamespace()
        bins = [list(ctypes.cast(c.bins[i], POINTER(ctypes.c_double * c.num_radius_bins)).contents)
                for i in range(c.num_angle_bins)]
        for a, row in enumerate(bins):            # core.py:109-117, same message
            for r, val in enumerate(row):
                if np.isnan(val):
                    print(f"NaN found at angle {a}, radius {r}. Correcting to 0.")
                    bins[a][r] = 0.0
        bp.bins = bins
        return bp

    def generate_blur_profile_image(self):
        """core.py:219-228 via get_blur_profile_visual (freed here, unlike the reference)."""
        h, w = self.rgb_stats.height, self.rgb_stats.width
        ptr = lib.get_blur_profile_visual(ctypes.byref(self.bp_ptr), h, w)
        img = image_pgm_to_pillow(ptr, w, h)
        lib.phd_free_pgm(ptr)
        self.blur_profile_image = img.crop((0, 0, w // 2, h))

    def generate_color_palette_image(self):
        """core.py:182-216 (falls back to PIL's default font when DejaVuSans is absent)."""
        from PIL import Image, ImageDraw, ImageFont
        n = len(self.color_palette.colors)
        block = 50
        per_row = int(np.ceil(np.sqrt(n))) if n else 1
        img = Image.new("RGB", (per_row * block, max(1, (n + per_row - 1) // per_row) * block), "black")
        draw = ImageDraw.Draw(img)
        try:
            font = ImageFont.truetype("DejaVuSans.ttf", 12)
        except OSError:
            font = ImageFont.load_default()
        for i, (color, q) in enumerate(zip(self.color_palette.colors, self.color_palette.quantities)):
            x1, y1 = (i % per_row) * block, (i // per_row) * block
            draw.rectangle([x1, y1, x1 + block, y1 + block], fill=tuple(int(c) for c in color))
            text = f"{q:.1%}"
            tw, th = draw.textbbox((0, 0), text, font=font)[2:]
            draw.text((x1 + (block - tw) / 2, y1 + (block - th) / 2), text, fill="black", font=font)
        self.color_palette_image = img

    def to_json(self):
        """core.py:388-436, same keys and padding."""
        d = {
            "Height": self.rgb_stats.height, "Width": self.rgb_stats.width,
            "Average Saturation": self.average_saturation,
            "Red Brightness": self.rgb_stats.Br, "Green Brightness": self.rgb_stats.Bg,
            "Blue Brightness": self.rgb_stats.Bb, "Red Contrast": self.rgb_stats.Cr,
            "Green Contrast": self.rgb_stats.Cg, "Blue Contrast": self.rgb_stats.Cb,
        }
        for i in range(10):
            d[f"Blur Vector {i+1} Angle"] = self.blur_vectors[i].angle
            d[f"Blur Vector {i+1} Magnitude"] = self.blur_vectors[i].magnitude
        for i in range(100):
            if i < len(self.color_palette.colors):
                h, s, v = self.color_palette.colors[i]
                pct = self.color_palette.quantities[i]
            else:
                h, s, v, pct = 0, 0, 0, 0
            d[f"Color {i+1} H"], d[f"Color {i+1} S"], d[f"Color {i+1} V"] = h, s, v
            d[f"Color {i+1} Percentage"] = pct
        for i in range(10):
            d[f"Sharpness {i+1}:"] = self.sharpnesses[i] if i < len(self.sharpnesses) else 0.0
        return json.dumps(d, indent=4)

    def __del__(self):
        ptr = getattr(self, "data_ptr", None)
        if ptr:
            lib.free_full_report(ctypes.byref(ptr))


def _finish(ptr, height, width, kw):
    report = Report(ptr, height, width)
    report.magnitude_threshold = kw.get("magnitude_thresh", DEFAULTS["magnitude_thresh"])
    report.fft_streak_threshold = kw.get("fft_streak_thresh", DEFAULTS["fft_streak_thresh"])
    report.blur_cutoff_ratio_denom = kw.get("blur_cutoff_ratio_denom", DEFAULTS["blur_cutoff_ratio_denom"])
    return report


def get_report(pil_image, salient_characters=None, h_partitions=18, s_partitions=2, v_partitions=3,
               black_thresh=0.1, gray_thresh=0.1, coverage_thresh=0.95, linked_list_size=1000,
               downsample_rate=1, radius_partitions=40, angle_partitions=72, quantity_weight=0.1,
               saturation_value_weight=0.9, fft_streak_thresh=1.20, magnitude_thresh=0.3,
               blur_cutoff_ratio_denom=2):
    """core.py:442-486.  `pil_image` may be a PIL image or an H x W x 3 uint8 array.
    An image the reference rejects (src/utilities.c:64-87) raises ValueError
    ("NULL pointer access"), exactly like the reference binding does."""
    kw = dict(h_partitions=h_partitions, s_partitions=s_partitions, v_partitions=v_partitions,
              black_thresh=black_thresh, gray_thresh=gray_thresh, coverage_thresh=coverage_thresh,
              linked_list_size=linked_list_size, downsample_rate=downsample_rate,
              radius_partitions=radius_partitions, angle_partitions=angle_partitions,
              quantity_weight=quantity_weight, saturation_value_weight=saturation_value_weight,
              fft_streak_thresh=fft_streak_thresh, magnitude_thresh=magnitude_thresh,
              blur_cutoff_ratio_denom=blur_cutoff_ratio_denom)
    rgb = to_rgb8(pil_image)
    height, width = rgb.shape[:2]
    cfg = make_config(**kw)
    crops = ctypes.byref(salient_characters) if isinstance(salient_characters, Crop_Boundaries) \
        else salient_characters
    start = time.time()
    ptr = lib.phd_report_u8(rgb.ctypes.data, height, width, 0, ctypes.byref(cfg), crops)
    if os.environ.get("PHD_VERBOSE"):
        print(f"Elapsed time: {time.time() - start} seconds")
    return _finish(ptr, height, width, kw)


def normalize_salient(salient_characters, n):
    """The per-image crop boxes of a batch call as the C argument: `None`, or
    (array of n POINTER(Crop_Boundaries), objects to keep alive for the call).
    salient_characters: a sequence of length n whose entries are None (no
    sharpnesses for that image), a Crop_Boundaries, or a list of
    {"top", "bottom", "left", "right"} dicts (set_bounding_boxes' input; an
    empty list gives N == 0).  Needs no GPU."""
    if salient_characters is None:
        return None
    entries = list(salient_characters)
    if len(entries) != n:
        raise ValueError(f"salient_characters has {len(entries)} entries for {n} images")
    keep = []
    arr = (POINTER(Crop_Boundaries) * n)()
    for i, e in enumerate(entries):
        if e is None:
            continue
        cb = e if isinstance(e, Crop_Boundaries) else set_bounding_boxes(list(e))
        keep.append(cb)
        arr[i] = ctypes.pointer(cb)
    return arr, keep


def _packed_images(images, nonempty=True, cuda=False, batch_error=None):
    """The packed uint8 [H, W, 3] tensors of a call as a list: a 4-D tensor is
    taken as its images (batch_error: what any other single tensor raises).
    nonempty / cuda: whether empty tensors and tensors off the GPU are refused."""
    import torch
    if isinstance(images, torch.Tensor):
        if images.dim() == 4:
            images = images.unbind(0)
        elif batch_error:
            raise ValueError(batch_error)
    images = list(images)
    for im in images:
        if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 \
                or not im.is_contiguous() or (nonempty and im.numel() == 0) or (cuda and not im.is_cuda):
            raise ValueError(f"expected contiguous{', non-empty' if nonempty else ''} uint8 [H, W, 3] device tensors")
    return images


def _image_arrays(images, ptr=lambda im: im.data_ptr()):
    """(pointers, heights, widths) of 2-D or [H, W, ...] images as C arrays."""
    n = len(images)
    return ((ctypes.c_void_p * n)(*[ptr(im) for im in images]),
            (ctypes.c_int * n)(*[int(im.shape[0]) for im in images]),
            (ctypes.c_int * n)(*[int(im.shape[1]) for im in images]))


def _window_entries(windows, n, noun="images"):
    """The per-image window lists of a call over n images (None: none for any)."""
    entries = list(windows) if windows is not None else [None] * n
    if len(entries) != n:
        raise ValueError(f"windows has {len(entries)} entries for {n} {noun}")
    return entries


def _window_array(entries):
    """The window lists of a call as the C argument: (array of
    POINTER(Crop_Boundaries), the Crop_Boundaries to keep alive, None entries
    for images without windows)."""
    keep = [None if e is None else window_boundaries(e) for e in entries]
    arr = (POINTER(Crop_Boundaries) * len(keep))()
    for i, cb in enumerate(keep):
        if cb is not None:
            arr[i] = ctypes.pointer(cb)
    return arr, keep


def get_reports(images, salient_characters=None, **kw):
    """Reports for a list of images (any sizes).  Failed images give None.
    salient_characters: per-image crop boxes (normalize_salient)."""
    cfg = make_config(**kw)
    arrs = [to_rgb8(im) for im in images]
    n = len(arrs)
    crops = normalize_salient(salient_characters, n)
    ptrs, hs, ws = _image_arrays(arrs, lambda a: a.ctypes.data)
    outs = (POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    if crops is None:
        lib.phd_report_batch_u8(ptrs, hs, ws, n, ctypes.byref(cfg), outs, st)
    else:
        lib.phd_report_batch_u8_crops(ptrs, hs, ws, n, ctypes.byref(cfg), crops[0], outs, st)
    return [(_finish(outs[i], hs[i], ws[i], kw) if st[i] == 0 else None) for i in range(n)]


def _run_reports(call, name, n, sizes, kw):
    """The result tail of the report*_device* wrappers: call(outs, status) makes
    the C call over n images, sizes[i] is image i's (height, width).  The
    reports, or RuntimeError with the library's message when one is missing."""
    outs = (POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    call(outs, st)
    res = [(_finish(outs[i], *sizes[i], kw) if st[i] == 0 else None) for i in range(n)]
    if any(r is None for r in res):
        err = last_error()
        del res                     # (the reports that did come back are freed)
        raise RuntimeError(f"{name} failed: {err}")
    return res


def _view_sizes(views, n):
    return [(views[i].height, views[i].width) for i in range(n)]


def _convert(call, name, views, n, shape, dtype, devices):
    """The conversion-only wrappers: one new tensor of shape(height, width) per
    view on devices[i], filled by call(array of their data pointers)."""
    import torch
    if n == 0:
        return []
    out = [torch.empty(shape(views[i].height, views[i].width), dtype=dtype, device=devices[i]) for i in range(n)]
    dst = (ctypes.c_void_p * n)(*[o.data_ptr() for o in out])
    if call(dst) != 0:
        raise RuntimeError(f"{name} failed: {last_error()}")
    return out


def _tensor_devices(keep):
    import torch
    return [t.device if isinstance(t, torch.Tensor) else "cuda" for t in keep]


def report_device(images, stream=None, salient_characters=None, **kw):
    """Reports for a uint8 torch tensor [N, H, W, 3] resident on the current GPU.
    salient_characters: per-image crop boxes (normalize_salient)."""
    if images.dtype.itemsize != 1 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError("expected a contiguous uint8 [N, H, W, 3] device tensor")
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    cfg = make_config(**kw)
    crops = normalize_salient(salient_characters, n)
    s = _stream_handle(stream)

    def call(outs, st):
        if crops is None:
            lib.phd_report_batch_device(images.data_ptr(), n, h, w, 0, ctypes.byref(cfg), outs, st, s)
        else:
            lib.phd_report_batch_device_crops(images.data_ptr(), n, h, w, 0, ctypes.byref(cfg), crops[0], outs, st, s)

    return _run_reports(call, "report_device", n, [(h, w)] * n, kw)


def reports_device_mixed(images, stream=None, salient_characters=None, **kw):
    """Reports for a list of uint8 torch tensors [H, W, 3] of any sizes resident
    on the current GPU (BASELINE config 5): one batched run per group of
    same-size images (phd_report_batch_device_mixed).  salient_characters:
    per-image crop boxes (normalize_salient)."""
    for im in images:
        if im.dtype.itemsize != 1 or im.dim() != 3 or im.shape[2] != 3 or not im.is_contiguous():
            raise ValueError("expected contiguous uint8 [H, W, 3] device tensors")
    n = len(images)
    cfg = make_config(**kw)
    crops = normalize_salient(salient_characters, n)
    ptrs, hs, ws = _image_arrays(images)
    s = _stream_handle(stream)

    def call(outs, st):
        if crops is None:
            lib.phd_report_batch_device_mixed(ptrs, hs, ws, n, ctypes.byref(cfg), outs, st, s)
        else:
            lib.phd_report_batch_device_mixed_crops(ptrs, hs, ws, n, ctypes.byref(cfg), crops[0], outs, st, s)

    return _run_reports(call, "reports_device_mixed", n, list(zip(hs, ws)), kw)


def reports_device_labels(images, stream=None, salient_characters=None, box_palettes=False, box_stats=False, **kw):
    """reports_device_mixed plus each image's palette label map
    (phd_report_batch_device_mixed_labels).  images: a list of uint8 [H, W, 3]
    device tensors of any sizes, or one [N, H, W, 3] tensor.  Returns (reports,
    labels): labels[i] is a torch.int16 [H // r, W // r] device tensor (r =
    downsample_rate; [H, W] for r <= 1) with the bits of the C map: the palette
    slot whose colour pixel k went into (an index into
    Report.color_palette.colors), or -1 (PHD_LABEL_NONE) for a pixel no slot
    kept.  box_palettes=True: returns (reports, labels, palettes), palettes[i]
    the image's box palette for its salient_characters boxes (image
    coordinates) as box_palettes_device returns it
    (phd_report_batch_device_mixed_box_palettes).  box_stats=True: the images'
    box statistics are appended last to the result, per image a float64
    [n_boxes, 7] array (Br Bg Bb Cr Cg Cb and the average saturation of each
    salient_characters box at full resolution) as box_stats_device returns it
    (phd_report_batch_device_mixed_box_stats)."""
    images = _packed_images(images, nonempty=False,
                            batch_error="expected a uint8 [N, H, W, 3] device tensor or a list of [H, W, 3] tensors")
    ptrs, hs, ws = _image_arrays(images)
    return _report_views("mixed", "reports_device_labels", (ptrs, hs, ws, len(images)), list(zip(hs, ws)), stream,
                         salient_characters, kw, [im.device for im in images], box_palettes, box_stats)


def quantize_device(labels, reports, none_rgb=(0, 0, 0), stream=None):
    """The quantised images of label maps (phd_labels_to_rgb_device): per map a
    uint8 [mh, mw, 3] device tensor whose pixel k is the palette colour of
    labels[i][k] -- the integer triple Report.color_palette.colors[label], what
    generate_color_palette_image draws -- or none_rgb where the label is -1.
    labels: int16 [mh, mw] device tensors (reports_device_labels); reports: the
    Report of each."""
    import torch
    labels, reports = list(labels), list(reports)
    if len(labels) != len(reports):
        raise ValueError(f"{len(labels)} label maps for {len(reports)} reports")
    for m in labels:
        if not isinstance(m, torch.Tensor) or m.dtype != torch.int16 or m.dim() != 2 or not m.is_contiguous() \
                or m.numel() == 0:
            raise ValueError("expected contiguous, non-empty int16 [mh, mw] device tensors")
    none = [int(c) for c in none_rgb]
    if len(none) != 3 or any(c < 0 or c > 255 for c in none):
        raise ValueError("none_rgb must be three values in 0..255")
    n = len(labels)
    if n == 0:
        return []
    luts = [np.array([[int(c) for c in col] for col in rep.color_palette.colors], dtype=np.uint8).reshape(-1, 3)
            for rep in reports]
    out = [torch.empty((m.shape[0], m.shape[1], 3), dtype=torch.uint8, device=m.device) for m in labels]
    maps, hs, ws = _image_arrays(labels)
    lut_ptrs = (ctypes.c_void_p * n)(*[(a.ctypes.data if a.size else None) for a in luts])
    ns = (ctypes.c_int * n)(*[a.shape[0] for a in luts])
    dst = (ctypes.c_void_p * n)(*[o.data_ptr() for o in out])
    if lib.phd_labels_to_rgb_device(maps, hs, ws, n, lut_ptrs, ns, (ctypes.c_uint8 * 3)(*none), dst,
                                    _stream_handle(stream)) != 0:
        raise RuntimeError(f"quantize_device failed: {last_error()}")
    return out


def _take_box_palettes(bp, n):
    """The numpy copies of n filled phd_box_palette structs (uint32 [n_boxes,
    n_slots + 1] each); the C blocks are freed."""
    try:
        out = []
        for i in range(n):
            nb, ns = int(bp[i].n_boxes), int(bp[i].n_slots)
            a = np.zeros((nb, ns + 1), dtype=np.uint32)
            if nb:
                ctypes.memmove(a.ctypes.data, bp[i].counts, a.nbytes)
            out.append(a)
        return out
    finally:
        lib.phd_free_box_palettes(bp, n)


def _free_boxes(bp, bs, n):
    if bp is not None:
        lib.phd_free_box_palettes(bp, n)
    if bs is not None:
        lib.phd_free_box_stats(bs, n)


def _take_box_stats(bs, n):
    """The numpy copies of n filled phd_box_stats structs (float64 [n_boxes, 7]
    each: Br Bg Bb Cr Cg Cb, average saturation); the C blocks are freed."""
    try:
        out = []
        for i in range(n):
            nb = int(bs[i].n_boxes)
            a = np.zeros((nb, 7), dtype=np.float64)
            if nb:
                st = np.ctypeslib.as_array(ctypes.cast(bs[i].stats, ctypes.POINTER(ctypes.c_double)), shape=(nb, 6))
                a[:, :6] = st
                a[:, 6] = np.ctypeslib.as_array(bs[i].average_saturation, shape=(nb,))
            out.append(a)
        return out
    finally:
        lib.phd_free_box_stats(bs, n)


def box_stats_device(images, boxes, stream=None):
    """The box statistics of packed uint8 [H, W, 3] device tensors of any sizes
    (phd_box_stats_device): per image a numpy.float64 [n_boxes, 7] array, row b
    the brightness Br Bg Bb, the contrast Cr Cg Cb and the average saturation
    of the pixels of box b at full resolution -- what get_rgb_statistics and
    get_hsv_average give on the cropped image.  boxes: what normalize_salient
    accepts, in image coordinates (rows top <= y < bottom, columns left <= x <
    right; None or an empty list: no boxes, an array of shape (0, 7)).  One
    launch sums every box of every image."""
    images = _packed_images(images)
    n = len(images)
    crops = normalize_salient(boxes if boxes is not None else [None] * n, n)
    if n == 0:
        return []
    ptrs, hs, ws = _image_arrays(images)
    bs = (PhdBoxStats * n)()
    if lib.phd_box_stats_device(ptrs, hs, ws, n, crops[0], bs, _stream_handle(stream)) != 0:
        raise RuntimeError(f"box_stats_device failed: {last_error()}")
    return _take_box_stats(bs, n)


def box_palettes_device(labels, reports_or_n_slots, boxes, stream=None):
    """The box palettes of label maps (phd_box_palettes_device): per map a
    numpy.uint32 [n_boxes, n_slots + 1] array; row b, column s is the number of
    map elements inside box b whose label is slot s, the last column those in no
    slot (-1, and any label >= n_slots).  labels: int16 [mh, mw] device tensors
    (reports_device_labels); reports_or_n_slots: the Report of each map, or its
    number of palette slots; boxes: what normalize_salient accepts, in MAP
    coordinates (rows top <= y < bottom, columns left <= x < right; None or an
    empty list: no boxes, an array of shape (0, n_slots + 1))."""
    import torch
    labels, slots = list(labels), list(reports_or_n_slots)
    if len(labels) != len(slots):
        raise ValueError(f"{len(labels)} label maps for {len(slots)} reports")
    for m in labels:
        if not isinstance(m, torch.Tensor) or m.dtype != torch.int16 or m.dim() != 2 or not m.is_contiguous() \
                or m.numel() == 0:
            raise ValueError("expected contiguous, non-empty int16 [mh, mw] device tensors")
    n = len(labels)
    crops = normalize_salient(boxes if boxes is not None else [None] * n, n)
    if n == 0:
        return []
    ns = (ctypes.c_int * n)(*[(int(s) if isinstance(s, (int, np.integer)) else len(s.color_palette.colors))
                              for s in slots])
    maps, hs, ws = _image_arrays(labels)
    bp = (PhdBoxPalette * n)()
    if lib.phd_box_palettes_device(maps, hs, ws, n, ns, crops[0], bp, _stream_handle(stream)) != 0:
        raise RuntimeError(f"box_palettes_device failed: {last_error()}")
    return _take_box_palettes(bp, n)


def _report_views(family, name, head, sizes, stream, salient_characters, kw, devices=None, box_palettes=False,
                  box_stats=False):
    """The four reports_device_* wrappers after their inputs are made: the C
    call of `family` ("mixed", "views", "typed_views", "yuv") whose leading
    arguments are `head` -- (pointers, heights, widths, n) or (descriptors, n)
    -- over images of sizes[i] = (height, width).  devices (labels=True): image
    i's label map is allocated here on devices[i].  The entry called is the
    least that takes what was asked for: the plain one, _labels, _box_palettes
    (with or without maps) or _box_stats (with or without either).  Returns
    the reports, or a tuple of them and, in this order, the maps, the box
    palettes and the box statistics that were asked for."""
    n = len(sizes)
    cfg = make_config(**kw)
    crops = normalize_salient(salient_characters, n)
    want_maps = devices is not None
    extras = want_maps + bool(box_palettes) + bool(box_stats)
    if n == 0 and extras:
        return ([],) * (1 + extras)
    s = _stream_handle(stream)
    labels = maps = None
    if want_maps:
        import torch
        r = max(1, int(cfg.downsample_rate))
        labels = [torch.empty((h // r, w // r) if r > 1 else (h, w), dtype=torch.int16, device=dev)
                  for (h, w), dev in zip(sizes, devices)]
        maps = (ctypes.c_void_p * n)(*[m.data_ptr() for m in labels])
    bp = (PhdBoxPalette * n)() if box_palettes else None
    bs = (PhdBoxStats * n)() if box_stats else None
    suffix, tail = ("_box_stats", (maps, bp, bs)) if box_stats else ("_box_palettes", (maps, bp)) if box_palettes \
        else ("_labels", (maps,)) if want_maps else ("", ())
    entry = getattr(lib, f"phd_report_batch_device_{family}{suffix}")
    try:
        reps = _run_reports(lambda outs, st: entry(*head, ctypes.byref(cfg), crops[0] if crops else None, *tail, outs,
                                                   st, s), name, n, sizes, kw)
    except RuntimeError:
        _free_boxes(bp, bs, n)
        raise
    if not extras:
        return reps
    return (reps,) + ((labels,) if want_maps else ()) + ((_take_box_palettes(bp, n),) if bp is not None else ()) + \
        ((_take_box_stats(bs, n),) if bs is not None else ())


def _label_devices(keep, tensor_of):
    """The device of each image's label map (labels=True): its tensor's.  A
    descriptor that is no tensor names no device to allocate on."""
    import torch
    devs = []
    for i, k in enumerate(keep):
        t = tensor_of(k)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"image {i}: labels=True needs torch tensors (the map is allocated on the image's "
                             "device); call the C entry with maps of your own for descriptors")
        devs.append(t.device)
    return devs


def _image_list(tensors, layout):
    """make_views' and make_typed_views' input as a list of images."""
    import torch
    if layout not in ("HWC", "CHW"):
        raise ValueError(f"layout must be 'HWC' or 'CHW', not {layout!r}")
    if isinstance(tensors, torch.Tensor):
        if tensors.dim() != 4:
            raise ValueError("a single tensor must be 4-D (a batch of images)")
        tensors = list(tensors.unbind(0))
    return list(tensors)


def _tensor_view_fields(t, layout, bgr, i):
    """(data, height, width, row stride, pixel stride, channel stride), the
    strides in bytes, of image i's tensor ([H, W, C] or [C, H, W], C = 3 or 4);
    bgr: data at channel 2, the channel stride negated."""
    if t.dim() != 3:
        raise ValueError(f"image {i}: expected 3 dimensions ({layout}), got {t.dim()}")
    if layout == "HWC":
        (h, w, ch), (rs, ps, cs) = t.shape, t.stride()
    else:
        (ch, h, w), (cs, rs, ps) = t.shape, t.stride()
    if ch not in (3, 4):
        raise ValueError(f"image {i}: expected 3 or 4 channels, got {ch}")
    es = t.element_size()
    rs, ps, cs = rs * es, ps * es, cs * es
    data = t.data_ptr()
    if bgr:
        data, cs = data + 2 * cs, -cs
    return data, int(h), int(w), int(rs), int(ps), int(cs)


def make_views(tensors, layout="HWC", bgr=False):
    """The PhdImageView descriptors of uint8 torch tensors, with no copy: a
    sequence of [H, W, C] (C = 3 or 4; layout "HWC") or [C, H, W] ("CHW")
    tensors of any strides, or one 4-D tensor taken as its images.  Channels
    0..2 are R, G, B; bgr=True reverses them (data at channel 2, the channel
    stride negated).  An entry that is a PhdImageView already is taken as it
    is (a call that mixes layouts, or memory that is no tensor).  Pure stride
    arithmetic on data_ptr() and stride(): needs no GPU (CPU tensors work).
    Returns (array of PhdImageView, objects to keep alive while the views are
    in use)."""
    import torch
    tensors = _image_list(tensors, layout)
    views = (PhdImageView * max(1, len(tensors)))()
    for i, t in enumerate(tensors):
        if isinstance(t, PhdImageView):
            views[i] = t
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError(f"image {i}: expected a uint8 torch tensor")
        views[i] = PhdImageView(*_tensor_view_fields(t, layout, bgr, i))
    return views, tensors


def reports_device_views(images, layout="HWC", bgr=False, stream=None, salient_characters=None, labels=False,
                         box_palettes=False, box_stats=False, **kw):
    """Reports for uint8 device tensors in any byte-strided layout (make_views:
    planar CHW, pitched rows, RGBA / BGRA, BGR, regions of interest, expanded
    grey planes; any sizes), without a repacked copy on the caller's side:
    views that are not packed RGB8 already are gathered into a library-owned
    staging image by one launch per run (phd_report_batch_device_views).
    salient_characters: per-image crop boxes in each view's own coordinates
    (normalize_salient).  labels=True: returns (reports, maps), maps[i] the
    image's palette label map as reports_device_labels returns it (int16
    [mh, mw] on the image's device, in the view's own coordinates;
    phd_report_batch_device_views_labels); the images must be tensors.
    box_palettes=True (independent of labels; no map tensor is allocated for
    it): the images' box palettes are appended to the result, (reports,
    palettes) or (reports, maps, palettes) -- per image a numpy.uint32
    [n_boxes, n_slots + 1] array as box_palettes_device returns it, for its
    salient_characters boxes (image coordinates); shape (0, n_slots + 1) for an
    image without boxes (phd_report_batch_device_views_box_palettes).
    box_stats=True (independent of both): the images' box statistics are
    appended last -- per image a float64 [n_boxes, 7] array (Br Bg Bb Cr Cg Cb
    and the average saturation of each box at full resolution) as
    box_stats_device returns it (phd_report_batch_device_views_box_stats)."""
    views, keep = make_views(images, layout, bgr)
    n = len(keep)
    return _report_views("views", "reports_device_views", (views, n), _view_sizes(views, n), stream, salient_characters,
                         kw, _label_devices(keep, lambda t: t) if labels else None, box_palettes, box_stats)


def pack_views_device(images, layout="HWC", bgr=False, stream=None):
    """The gather alone (phd_pack_views_device): packed [H, W, 3] uint8 device
    tensors of the given views (make_views), for the stage-only calls
    (sharpness_device, hsv_stats_device, blur_profiles_device)."""
    import torch
    views, keep = make_views(images, layout, bgr)
    n = len(keep)
    return _convert(lambda dst: lib.phd_pack_views_device(views, n, dst, _stream_handle(stream)),
                    "pack_views_device", views, n, lambda h, w: (h, w, 3), torch.uint8, _tensor_devices(keep))


def _typed_elems():
    import torch
    elems = {torch.uint8: PHD_ELEM_U8, torch.float16: PHD_ELEM_F16, torch.float32: PHD_ELEM_F32,
             torch.float64: PHD_ELEM_F64}
    if hasattr(torch, "uint16"):
        elems[torch.uint16] = PHD_ELEM_U16
    return elems


def make_typed_views(tensors, layout="HWC", bgr=False, max_value=None, snap_u8=False):
    """The PhdTypedView descriptors of uint8, uint16, float16, float32 or
    float64 torch tensors, with no copy: make_views' layouts ([H, W, C] with
    C = 3 or 4, or [C, H, W]; any strides; one 4-D tensor as its images;
    bgr=True reverses the channels), byte strides = element strides *
    element_size().  16-bit images held as int16 go in as
    t.view(torch.uint16).  An element's value is element / max_value
    (None: the type's own 255, 65535 or 1.0; a number, or one per image:
    1023 for 10-bit data in 16-bit storage, 255 for floats in 0..255).
    snap_u8 (a bool, or one per image): float16 / float32 elements that are
    uint8 / 255 rounded to that type count as that 8-bit value, so a
    ToTensor() image gets the report of the 8-bit image it came from.  An entry
    that is a PhdTypedView already is taken as it is.  Needs no GPU (CPU tensors
    work).  Returns (array of PhdTypedView, objects to keep alive)."""
    import torch
    tensors = _image_list(tensors, layout)
    n = len(tensors)
    maxes = list(max_value) if isinstance(max_value, (list, tuple)) else [max_value] * n
    snaps = list(snap_u8) if isinstance(snap_u8, (list, tuple)) else [snap_u8] * n
    if len(maxes) != n or len(snaps) != n:
        raise ValueError(f"max_value / snap_u8 must be one value or one per image ({n} images)")
    elems = _typed_elems()
    views = (PhdTypedView * max(1, n))()
    for i, t in enumerate(tensors):
        if isinstance(t, PhdTypedView):
            views[i] = t
            continue
        if not isinstance(t, torch.Tensor) or t.dtype not in elems:
            raise ValueError(f"image {i}: expected a uint8, uint16, float16, float32 or float64 torch tensor")
        fields = _tensor_view_fields(t, layout, bgr, i)
        mv = 0.0 if maxes[i] is None else float(maxes[i])
        if not (mv >= 0.0 and mv != float("inf")) or (maxes[i] is not None and mv == 0.0):
            raise ValueError(f"image {i}: max_value must be finite and positive")
        views[i] = PhdTypedView(*fields, elems[t.dtype], PHD_VIEW_SNAP_U8 if snaps[i] else 0, mv)
    return views, tensors


def reports_device_typed(images, layout="HWC", bgr=False, max_value=None, snap_u8=False, stream=None,
                         salient_characters=None, labels=False, box_palettes=False, box_stats=False, **kw):
    """Reports for device tensors of any element type in any byte-strided layout
    (make_typed_views; any sizes): a 16-bit decode, a float CHW tensor in 0..1,
    double planes already on the GPU.  Images whose values are exactly 8-bit
    (j / 255; with snap_u8 also floats that are uint8 / 255 in their own type)
    join the RGB8 batch of their size and get its report bit for bit; every
    other image is decoded to doubles on the device and reported by the fp64
    pipeline of get_full_report_data on those doubles, with no host round trip
    of pixels (phd_report_batch_device_typed_views).  salient_characters:
    per-image crop boxes in each view's own coordinates (normalize_salient).
    labels=True: returns (reports, maps) as reports_device_views does
    (phd_report_batch_device_typed_views_labels): an 8-bit image's map is that
    of its bytes, an fp64-route image's the reference's lists on its doubles.
    box_palettes=True: the box palettes are appended as reports_device_views
    appends them (phd_report_batch_device_typed_views_box_palettes).
    box_stats=True: the box statistics are appended last as
    reports_device_views appends them; an fp64-route image's are the fp64
    functions on its doubles (phd_report_batch_device_typed_views_box_stats)."""
    views, keep = make_typed_views(images, layout, bgr, max_value, snap_u8)
    n = len(keep)
    return _report_views("typed_views", "reports_device_typed", (views, n), _view_sizes(views, n), stream,
                         salient_characters, kw, _label_devices(keep, lambda t: t) if labels else None, box_palettes,
                         box_stats)


def decode_views_device(images, layout="HWC", bgr=False, max_value=None, stream=None):
    """The decode alone (phd_decode_views_device): float64 [3, H, W] device
    tensors holding element / max_value of the given views (make_typed_views),
    the planes get_full_report_data takes."""
    import torch
    views, keep = make_typed_views(images, layout, bgr, max_value)
    n = len(keep)
    return _convert(lambda dst: lib.phd_decode_views_device(views, n, dst, _stream_handle(stream)),
                    "decode_views_device", views, n, lambda h, w: (3, h, w), torch.float64, _tensor_devices(keep))


def nv12_planes(surface, height, width):
    """The (y, uv) planes of an NV12 decoder surface, with no copy: `surface`
    is a 2-D uint8 tensor [>= height + ch, pitch] (pitch >= width rounded up to
    even) holding height luma rows and then ch = (height + 1) // 2 rows of
    interleaved Cb Cr pairs.  Returns y [height, width] and uv [ch, cw, 2]
    views of it (cw = (width + 1) // 2), make_yuv_views' (y, uv) frame."""
    ch, cw = (height + 1) // 2, (width + 1) // 2
    if surface.dim() != 2 or surface.shape[0] < height + ch or surface.shape[1] < max(width, 2 * cw):
        raise ValueError(f"expected a 2-D surface of at least {height + ch} rows of {max(width, 2 * cw)} bytes, "
                         f"got {tuple(surface.shape)}")
    y = surface[:height, :width]
    uv = surface[height:height + ch, :2 * cw].unflatten(1, (cw, 2))
    return y, uv


_YUV_MATRICES = {"bt601": PHD_YUV_BT601, "bt709": PHD_YUV_BT709}
_YUV_CHROMA = {"replicate": PHD_YUV_CHROMA_REPLICATE, "triangle": PHD_YUV_CHROMA_TRIANGLE}


def make_yuv_views(frames, matrix="bt601", full_range=True, chroma="replicate", swap_uv=False):
    """The PhdYuvView descriptors of 8-bit YCbCr frames held in uint8 torch
    tensors, with no copy.  Each frame is (y, cb, cr), three 2-D tensors (I420,
    I422, I444 and their pitched or cropped views); (y, uv) with uv of shape
    [ch, cw, 2], interleaved Cb Cr (NV12; nv12_planes splits a decoder
    surface); or a PhdYuvView, taken as it is (YUY2, memory that is no
    tensor).  swap_uv=True reads the chroma as Cr Cb (NV21; YV12 for three
    planes).  The subsampling is inferred from the shapes: chroma of
    (H, W) is 4:4:4, (H, (W + 1) // 2) 4:2:2, ((H + 1) // 2, (W + 1) // 2)
    4:2:0.  matrix: "bt601" or "bt709"; full_range: JFIF's 0..255, else
    16..235 / 16..240; chroma: "replicate" or "triangle" (libjpeg's fancy
    upsampling).  Pure stride arithmetic on data_ptr() and stride(): needs no
    GPU (CPU tensors work).  Returns (array of PhdYuvView, objects to keep
    alive while the views are in use)."""
    import torch
    if matrix not in _YUV_MATRICES:
        raise ValueError(f"matrix must be 'bt601' or 'bt709', not {matrix!r}")
    if chroma not in _YUV_CHROMA:
        raise ValueError(f"chroma must be 'replicate' or 'triangle', not {chroma!r}")
    frames = list(frames)
    views = (PhdYuvView * max(1, len(frames)))()

    def plane(i, t, dims, what):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != dims:
            raise ValueError(f"image {i}: {what} must be a {dims}-D uint8 torch tensor")
        return t

    for i, f in enumerate(frames):
        if isinstance(f, PhdYuvView):
            views[i] = f
            continue
        if not isinstance(f, (tuple, list)) or len(f) not in (2, 3):
            raise ValueError(f"image {i}: expected (y, cb, cr), (y, uv) or a PhdYuvView")
        y = plane(i, f[0], 2, "y")
        h, w = int(y.shape[0]), int(y.shape[1])
        if h < 1 or w < 1:
            raise ValueError(f"image {i}: empty luma plane {tuple(y.shape)}")
        if len(f) == 2:
            uv = plane(i, f[1], 3, "uv")
            if uv.shape[2] != 2:
                raise ValueError(f"image {i}: uv must have shape [ch, cw, 2], got {tuple(uv.shape)}")
            cshape, (crs, cps, pair) = tuple(uv.shape[:2]), uv.stride()
            cb, cr = uv.data_ptr(), uv.data_ptr() + pair
        else:
            pb, pr = plane(i, f[1], 2, "cb"), plane(i, f[2], 2, "cr")
            if pb.shape != pr.shape or pb.stride() != pr.stride():
                raise ValueError(f"image {i}: cb and cr differ in shape or strides "
                                 f"({tuple(pb.shape)} {pb.stride()} and {tuple(pr.shape)} {pr.stride()})")
            cshape, (crs, cps) = tuple(pb.shape), pb.stride()
            cb, cr = pb.data_ptr(), pr.data_ptr()
        # (a single row or column fits several: the least subsampled reading)
        fits = [s for s in ((0, 0), (1, 0), (1, 1)) if cshape == ((h + s[1]) >> s[1], (w + s[0]) >> s[0])]
        if not fits:
            raise ValueError(f"image {i}: chroma of shape {cshape} fits no subsampling of a {h} x {w} luma plane")
        sx, sy = fits[0]
        if swap_uv:
            cb, cr = cr, cb
        yrs, yps = y.stride()
        views[i] = PhdYuvView(y.data_ptr(), cb, cr, h, w, int(yrs), int(yps), int(crs), int(cps), sx, sy,
                              _YUV_MATRICES[matrix], PHD_YUV_FULL if full_range else PHD_YUV_LIMITED,
                              _YUV_CHROMA[chroma])
    return views, frames


def reports_device_yuv(frames, matrix="bt601", full_range=True, chroma="replicate", swap_uv=False, stream=None,
                       salient_characters=None, labels=False, box_palettes=False, box_stats=False, **kw):
    """Reports for 8-bit YCbCr frames on the current GPU (make_yuv_views: NV12
    surfaces, planar 4:2:0 / 4:2:2 / 4:4:4, YUY2 descriptors; any sizes): each
    frame is converted to RGB8 by the library's integer conversion
    (include/photohive_dsp.h), one launch per run, and reported as that image
    (phd_report_batch_device_yuv).  salient_characters: per-image crop boxes
    in luma coordinates (normalize_salient).  labels=True: returns (reports,
    maps), maps[i] the label map of frame i's RGB8 conversion in luma
    coordinates, on the luma plane's device (phd_report_batch_device_yuv_labels;
    the frames must be tensors).  box_palettes=True: the box palettes are
    appended as reports_device_views appends them
    (phd_report_batch_device_yuv_box_palettes).  box_stats=True: the box
    statistics of the RGB8 conversion are appended last as reports_device_views
    appends them (phd_report_batch_device_yuv_box_stats)."""
    views, keep = make_yuv_views(frames, matrix, full_range, chroma, swap_uv)
    n = len(keep)
    return _report_views("yuv", "reports_device_yuv", (views, n), _view_sizes(views, n), stream, salient_characters, kw,
                         _label_devices(keep, lambda f: f[0] if isinstance(f, (tuple, list)) else f) if labels
                         else None, box_palettes, box_stats)


def convert_yuv_device(frames, matrix="bt601", full_range=True, chroma="replicate", swap_uv=False, stream=None):
    """The conversion alone (phd_convert_yuv_device): packed [H, W, 3] uint8
    device tensors of the given frames (make_yuv_views), for the stage-only
    calls and for callers that want the library's RGB8 bytes."""
    import torch
    views, keep = make_yuv_views(frames, matrix, full_range, chroma, swap_uv)
    n = len(keep)
    return _convert(lambda dst: lib.phd_convert_yuv_device(views, n, dst, _stream_handle(stream)),
                    "convert_yuv_device", views, n, lambda h, w: (h, w, 3), torch.uint8,
                    [f[0].device if isinstance(f, (tuple, list)) else "cuda" for f in keep])


def sharpness_device(images, salient_characters, stream=None):
    """The sharpness stage alone (get_variance_sharpness, src/filtering.c:151-183)
    for a uint8 torch tensor [N, H, W, 3] on the current GPU and per-image crop
    boxes (normalize_salient): a list of N lists, the full report's values
    ([] for an image without boxes)."""
    if images.dtype.itemsize != 1 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError("expected a contiguous uint8 [N, H, W, 3] device tensor")
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    crops = normalize_salient(salient_characters, n)
    if crops is None:
        raise ValueError("sharpness_device needs salient_characters")
    counts = [crops[0][i].contents.N if crops[0][i] else 0 for i in range(n)]
    out = (ctypes.c_double * max(1, sum(counts)))()
    s = _stream_handle(stream)
    if lib.phd_sharpness_batch_device(images.data_ptr(), n, h, w, 0, crops[0], out, s) != 0:
        raise RuntimeError(f"sharpness_device failed: {last_error()}")
    res, k = [], 0
    for m in counts:
        res.append([out[k + j] for j in range(m)])
        k += m
    return res


def hsv_stats_device(images, stream=None):
    """rgb2hsv + get_hsv_average + get_rgb_statistics (src/image_processing.c:372-417, 533-553)
    for a uint8 torch tensor [N, H, W, 3] on the current GPU: returns
    ([RGB_Statistics] * N, [average saturation] * N)."""
    if images.dtype.itemsize != 1 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError("expected a contiguous uint8 [N, H, W, 3] device tensor")
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    stats = (RGB_Statistics * n)()
    sat = (ctypes.c_double * n)()
    s = _stream_handle(stream)
    if lib.phd_hsv_stats_batch_device(images.data_ptr(), n, h, w, 0, stats, sat, s) != 0:
        raise RuntimeError(f"hsv_stats_device failed: {last_error()}")
    return list(stats), list(sat)


def blur_profiles_device(images, stream=None, **kw):
    """The FFT + blur-profile path alone (BASELINE config 4; rgb2pgm, pgm_fft,
    calculate_blur_profile, vectorize_blur_profile) for a uint8 torch tensor
    [N, H, W, 3] on the current GPU: returns (bins [N, angle, radius] float64,
    [[(angle, magnitude)] * 10] * N) -- the full report's values."""
    from .structures import Blur_Vector
    if images.dtype.itemsize != 1 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError("expected a contiguous uint8 [N, H, W, 3] device tensor")
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    cfg = make_config(**kw)
    na, nr = cfg.angle_partitions, cfg.radius_partitions
    bins = np.zeros((n, na, nr), dtype=np.float64)
    vecs = (Blur_Vector * (10 * n))()
    s = _stream_handle(stream)
    if lib.phd_blur_batch_device(images.data_ptr(), n, h, w, 0, ctypes.byref(cfg),
                                 bins.ctypes.data_as(POINTER(ctypes.c_double)), vecs, s) != 0:
        raise RuntimeError(f"blur_profiles_device failed: {last_error()}")
    return bins, [[(vecs[10 * i + k].angle, vecs[10 * i + k].magnitude) for k in range(10)] for i in range(n)]


WINDOW_DEFAULTS = dict(radius_partitions=16, angle_partitions=36)


def window_grid(height, width, window=128, stride=None):
    """The row-major list of window x window boxes (top, bottom, left, right) at
    steps of `stride` (default: window) that lie inside a height x width image,
    and its shape (gh, gw).  Needs no GPU."""
    stride = window if stride is None else int(stride)
    if window <= 0 or stride <= 0:
        raise ValueError("window and stride must be positive")
    gh = (height - window) // stride + 1 if height >= window else 0
    gw = (width - window) // stride + 1 if width >= window else 0
    boxes = [(y * stride, y * stride + window, x * stride, x * stride + window) for y in range(gh) for x in range(gw)]
    return boxes, (gh, gw)


def window_boundaries(boxes):
    """A Crop_Boundaries of window boxes: a Crop_Boundaries as is, else a sequence
    of (top, bottom, left, right) tuples or set_bounding_boxes' dicts."""
    if isinstance(boxes, Crop_Boundaries):
        return boxes
    rows = [(b["top"], b["bottom"], b["left"], b["right"]) if isinstance(b, dict) else tuple(b) for b in boxes]
    a = np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(-1, 4).T)
    n = a.shape[1]
    cols = [(ctypes.c_int * n).from_buffer_copy(a[k].tobytes()) if n else (ctypes.c_int * 0)() for k in range(4)]
    return Crop_Boundaries(N=n, top=cols[0], bottom=cols[1], left=cols[2], right=cols[3])


def blur_windows_device(images, windows, window=128, stream=None, **kw):
    """The window blur of packed uint8 [H, W, 3] device tensors of any sizes from
    window x window (phd_blur_windows_device): per image a tuple (bins [n, na, nr]
    float64, angles [n, 10] int32, magnitudes [n, 10] float32, fft_max [n]
    float64) -- the reference's Blur_Profile bins, its ten Blur_Vectors and the
    spectrum maximum on each window's crop of the full-resolution image.
    windows: per image None, a Crop_Boundaries or a sequence of (top, bottom, left,
    right) boxes whose sides are `window` (64 or 128).  kw: the report's
    parameters; radius_partitions and angle_partitions default to 16 and 36 here
    (the report's 40 x 72 leaves most bins of a small spectrum empty and has no
    table at 64).  One launch takes every window of every image."""
    images = _packed_images(images)
    n = len(images)
    entries = _window_entries(windows, n)
    cfg = make_config(**{**WINDOW_DEFAULTS, **kw})
    if n == 0:
        return []
    arr, keep = _window_array(entries)
    ptrs, hs, ws = _image_arrays(images)
    wb = (PhdWindowBlur * n)()
    if lib.phd_blur_windows_device(ptrs, hs, ws, n, arr, int(window), ctypes.byref(cfg), wb,
                                   _stream_handle(stream)) != 0:
        raise RuntimeError(f"blur_windows_device failed: {last_error()}")
    return _take_window_blur(wb, n, cfg.angle_partitions, cfg.radius_partitions)


def _take_window_blur(wb, n, na, nr):
    """The numpy copies of n filled phd_window_blur structs; the C blocks are freed."""
    try:
        out = []
        for i in range(n):
            m = int(wb[i].n_windows)
            bins = np.zeros((m, na, nr), dtype=np.float64)
            ang = np.zeros((m, 10), dtype=np.int32)
            mag = np.zeros((m, 10), dtype=np.float32)
            fmax = np.zeros(m, dtype=np.float64)
            if m:
                bins[...] = np.ctypeslib.as_array(wb[i].bins, shape=(m, na, nr))
                v = np.ctypeslib.as_array(ctypes.cast(wb[i].vectors, POINTER(ctypes.c_int32)), shape=(m, 10, 2))
                ang[...] = v[..., 0]
                mag[...] = v[..., 1].copy().view(np.float32)
                fmax[...] = np.ctypeslib.as_array(wb[i].fft_max, shape=(m,))
            out.append((bins, ang, mag, fmax))
        return out
    finally:
        lib.phd_free_window_blur(wb, n)


def blur_map_device(images, window=128, stride=None, stream=None, **kw):
    """blur_windows_device over window_grid of every image: per image the same
    four arrays shaped [gh, gw, ...] (bins [gh, gw, na, nr], angles and
    magnitudes [gh, gw, 10], fft_max [gh, gw]).  Other inputs -- strided, planar
    or 4-byte views, YCbCr frames -- go through pack_views_device or
    convert_yuv_device first."""
    import torch
    if isinstance(images, torch.Tensor) and images.dim() == 4:
        images = list(images.unbind(0))
    images = list(images)
    grids = [window_grid(int(im.shape[0]), int(im.shape[1]), window, stride) for im in images]
    res = blur_windows_device(images, [g[0] for g in grids], window=window, stream=stream, **kw)
    return [tuple(a.reshape(g[1] + a.shape[1:]) for a in r) for r, g in zip(res, grids)]


def _window_lists(images, windows, kw=None):
    """The list preamble of a window call: (images, the C array of their window
    lists, what keeps it alive, windows per image, cfg from kw -- None without)."""
    images = _packed_images(images, cuda=True)
    entries = _window_entries(windows, len(images))
    cfg = None if kw is None else make_config(**{**WINDOW_DEFAULTS, **kw})
    arr, keep = _window_array(entries)
    return images, arr, keep, [0 if cb is None else int(cb.N) for cb in keep], cfg


def _window_grids(images, window, stride, kw=None):
    """The grid preamble of a window call: (images, the stride, window_grid's
    shape per image -- (0, 0) where the library refuses the window or the stride
    --, cfg from kw -- None without)."""
    images = _packed_images(images, cuda=True)
    stride = window if stride is None else int(stride)
    cfg = None if kw is None else make_config(**{**WINDOW_DEFAULTS, **kw})
    grids = [window_grid(int(im.shape[0]), int(im.shape[1]), window, stride)[1] if stride > 0 and window > 0
             else (0, 0) for im in images]
    return images, stride, grids, cfg


def _window_call(name, images, counts, shapes, outputs, stream, call):
    """The device tensors of a window call and the call itself.  outputs: (per
    output array of the C entry its (dtype, trailing shape), or None for one not
    asked for -- a NULL array; form); a trailing shape given as a function is
    called with the image's index (the palette maps' n_slots + 1 counters); call(pointers,
    heights, widths, n, *output arrays, stream handle) is the entry; form(*an
    image's tensors, each shaped shapes[i] + its trailing shape) is the image's
    result."""
    import torch
    n = len(images)
    if n == 0:
        return []
    specs, form = outputs
    trail = lambda s, i: tuple(s[1](i) if callable(s[1]) else s[1])         # noqa: E731
    outs = [None if s is None else [torch.empty((c,) + trail(s, i), dtype=s[0], device=im.device)
                                    for i, (im, c) in enumerate(zip(images, counts))] for s in specs]
    live = [ts for ts in outs if ts is not None]
    if stream is not None:
        for t in sum(live, []):
            t.record_stream(stream)
    ptrs, hs, ws = _image_arrays(images)
    arrays = [None if ts is None else (ctypes.c_void_p * n)(*[t.data_ptr() if c else None for t, c in zip(ts, counts)])
              for ts in outs]
    if call(ptrs, hs, ws, n, *arrays, _stream_handle(stream)) != 0:
        raise RuntimeError(f"{name} failed: {last_error()}")
    return [form(*[t.reshape(tuple(shp) + tuple(t.shape[1:])) for t in ts]) for ts, shp in zip(zip(*live), shapes)]


def _vector_outputs():
    """_window_call's outputs of the blur vector entries: per image (angles,
    magnitudes, fft_max) shaped shapes[i] + (10,), (10,), ()."""
    import torch
    return ([(torch.int32, (10, 2)), (torch.float64, ())],
            lambda v, f: (v[..., 0], v[..., 1].view(torch.float32), f))


def _sharpness_outputs(variance):
    """_window_call's outputs of the window sharpness entries: per image the
    sharpness shaped shapes[i], or (sharpness, variance)."""
    import torch
    spec = (torch.float64, ())
    return [spec, spec if variance else None], (lambda s, v: (s, v)) if variance else (lambda s: s)


def blur_vectors_device(images, windows, window=128, stream=None, **kw):
    """The ten Blur_Vectors and the spectrum maximum of every window, finished on
    the device (phd_blur_vectors_device): per image a tuple of device tensors
    (angles [n, 10] int32, magnitudes [n, 10] float32, fft_max [n] float64);
    angles and magnitudes are views of one interleaved [n, 10, 2] int32 tensor.
    Inputs and kw as blur_windows_device; angle_partitions must be at least 2.
    Nothing is copied to the host; with stream= the call is enqueued on that
    stream and the tensors are valid in its order."""
    images, arr, keep, counts, cfg = _window_lists(images, windows, kw)
    return _window_call("blur_vectors_device", images, counts, [(c,) for c in counts], _vector_outputs(), stream,
                        lambda ptrs, hs, ws, n, pv, pf, s: lib.phd_blur_vectors_device(
                            ptrs, hs, ws, n, arr, int(window), ctypes.byref(cfg), pv, pf, s))


def blur_vector_maps_device(images, window=128, stride=None, stream=None, **kw):
    """blur_vectors_device over window_grid of every image, the grid formed by the
    library (phd_blur_vector_maps_device): per image device tensors (angles
    [gh, gw, 10] int32, magnitudes [gh, gw, 10] float32, fft_max [gh, gw]
    float64) -- blur_map_device's vectors and maxima without its bins, and
    without a copy to the host."""
    images, stride, grids, cfg = _window_grids(images, window, stride, kw)
    return _window_call("blur_vector_maps_device", images, [g[0] * g[1] for g in grids], grids, _vector_outputs(),
                        stream, lambda ptrs, hs, ws, n, pv, pf, s: lib.phd_blur_vector_maps_device(
                            ptrs, hs, ws, n, int(window), stride, ctypes.byref(cfg), pv, pf, s))


def sharpness_windows_device(images, windows, window=64, variance=False, stream=None):
    """The Laplacian sharpness of every window, left on the device
    (phd_sharpness_windows_device): per image a float64 device tensor [n] -- the
    reference's get_variance_sharpness on each window's crop of the
    full-resolution luma -- or with variance=True a pair (sharpness, variance of
    the Laplacian).  images: packed uint8 [H, W, 3] device tensors of any sizes
    from window x window; windows: per image None, a Crop_Boundaries or a sequence
    of (top, bottom, left, right) boxes whose sides are `window` (16, 32, 64 or
    128).  A window with a black border ring gives +inf (NaN when it is black
    throughout).  One launch takes every window of every image; nothing is copied
    to the host; with stream= the call is enqueued on that stream and the tensors
    are valid in its order."""
    images, arr, keep, counts, _ = _window_lists(images, windows)
    return _window_call("sharpness_windows_device", images, counts, [(c,) for c in counts],
                        _sharpness_outputs(variance), stream,
                        lambda ptrs, hs, ws, n, ps, pv, s: lib.phd_sharpness_windows_device(
                            ptrs, hs, ws, n, arr, int(window), ps, pv, s))


def sharpness_maps_device(images, window=64, stride=None, variance=False, stream=None):
    """sharpness_windows_device over window_grid of every image, the grid formed by
    the library (phd_sharpness_maps_device): per image a float64 device tensor
    [gh, gw], or with variance=True a pair of them.  At window 64 and 128 the grid
    is blur_vector_maps_device's."""
    images, stride, grids, _ = _window_grids(images, window, stride)
    return _window_call("sharpness_maps_device", images, [g[0] * g[1] for g in grids], grids,
                        _sharpness_outputs(variance), stream,
                        lambda ptrs, hs, ws, n, ps, pv, s: lib.phd_sharpness_maps_device(
                            ptrs, hs, ws, n, int(window), stride, ps, pv, s))


def _stats_outputs():
    """_window_call's output of the window statistics entries: per image one tensor
    shaped shapes[i] + (7,)."""
    import torch
    return [(torch.float64, (7,))], lambda s: s


def stats_windows_device(images, windows, window=64, stream=None):
    """Brightness, contrast and average saturation of every window, left on the
    device (phd_stats_windows_device): per image a float64 device tensor [n, 7] --
    Br Bg Bb Cr Cg Cb S-bar, the reference's get_rgb_statistics and
    get_hsv_average on each window's crop.  images and windows as
    sharpness_windows_device takes them (`window` is 16, 32, 64 or 128).  One
    launch takes every window of every image; nothing is copied to the host; with
    stream= the call is enqueued on that stream and the tensors are valid in its
    order."""
    images, arr, keep, counts, _ = _window_lists(images, windows)
    return _window_call("stats_windows_device", images, counts, [(c,) for c in counts], _stats_outputs(), stream,
                        lambda ptrs, hs, ws, n, ps, s: lib.phd_stats_windows_device(
                            ptrs, hs, ws, n, arr, int(window), ps, s))


def stats_maps_device(images, window=64, stride=None, stream=None):
    """stats_windows_device over window_grid of every image, the grid formed by the
    library (phd_stats_maps_device): per image a float64 device tensor
    [gh, gw, 7].  The grid is sharpness_maps_device's."""
    images, stride, grids, _ = _window_grids(images, window, stride)
    return _window_call("stats_maps_device", images, [g[0] * g[1] for g in grids], grids, _stats_outputs(), stream,
                        lambda ptrs, hs, ws, n, ps, s: lib.phd_stats_maps_device(
                            ptrs, hs, ws, n, int(window), stride, ps, s))


def _label_maps(labels, reports_or_n_slots):
    """The label preamble of a palette window call: (the int16 [mh, mw] device
    tensors as a list, the C array of their palette slot counts and its values)."""
    import torch
    labels, slots = list(labels), list(reports_or_n_slots)
    if len(labels) != len(slots):
        raise ValueError(f"{len(labels)} label maps for {len(slots)} reports")
    for m in labels:
        if not isinstance(m, torch.Tensor) or m.dtype != torch.int16 or m.dim() != 2 or not m.is_contiguous() \
                or m.numel() == 0 or not m.is_cuda:
            raise ValueError("expected contiguous, non-empty int16 [mh, mw] device tensors")
    ns = [(int(s) if isinstance(s, (int, np.integer)) else len(s.color_palette.colors)) for s in slots]
    return labels, (ctypes.c_int * len(ns))(*ns), ns


def _palette_outputs(ns, counts, dominant):
    """_window_call's outputs of the palette window entries: per map the counts
    shaped shapes[i] + (n_slots + 1,), the dominant labels shaped shapes[i], or the
    pair (counts, dominant)."""
    import torch
    if not counts and not dominant:
        raise ValueError("counts or dominant (or both) must be asked for")
    # a slot count outside 0..4096 is the library's to refuse; its tensor only has to exist
    return ([(torch.int32, lambda i: (min(max(ns[i], 0), 4096) + 1,)) if counts else None,
             (torch.int16, ()) if dominant else None],
            (lambda c, d: (c, d)) if counts and dominant else (lambda t: t))


def palette_windows_device(labels, reports_or_n_slots, windows, window=64, counts=True, dominant=False, stream=None):
    """The palette slot counts of every window of label maps, left on the device
    (phd_palette_windows_device): per map a torch.int32 device tensor
    [n, n_slots + 1] -- row k, column s the number of elements of window k whose
    label is slot s, the last column those in no slot (-1, and any label >=
    n_slots): box_palettes_device's integers on the same boxes -- and / or, with
    dominant=True, a torch.int16 tensor [n]: the slot with the largest count, the
    lowest on a tie, -1 where "no slot" is strictly the largest.  With both the
    result is the pair (counts, dominant).  labels and reports_or_n_slots as
    box_palettes_device takes them; windows: per map None, a Crop_Boundaries or a
    sequence of (top, bottom, left, right) boxes of MAP coordinates whose sides are
    `window` (16, 32, 64 or 128).  One launch takes every window of every map;
    nothing is copied to the host; with stream= the call is enqueued on that stream
    and the tensors are valid in its order."""
    labels, ns_arr, ns = _label_maps(labels, reports_or_n_slots)
    arr, keep = _window_array(_window_entries(windows, len(labels), "maps"))
    n_win = [0 if cb is None else int(cb.N) for cb in keep]
    return _window_call("palette_windows_device", labels, n_win, [(c,) for c in n_win],
                        _palette_outputs(ns, counts, dominant), stream,
                        lambda ptrs, hs, ws, n, pc, pd, s: lib.phd_palette_windows_device(
                            ptrs, hs, ws, n, ns_arr, arr, int(window), pc, pd, s))


def palette_maps_device(labels, reports_or_n_slots, window=64, stride=None, counts=True, dominant=False, stream=None):
    """palette_windows_device over window_grid of every map, the grid formed by the
    library (phd_palette_maps_device): per map a torch.int32 device tensor
    [gh, gw, n_slots + 1] and / or a torch.int16 tensor [gh, gw].  The dominant
    tensor is itself a label map of the same palette: quantize_device paints it."""
    labels, ns_arr, ns = _label_maps(labels, reports_or_n_slots)
    stride = window if stride is None else int(stride)
    grids = [window_grid(int(m.shape[0]), int(m.shape[1]), window, stride)[1] if stride > 0 and window > 0
             else (0, 0) for m in labels]
    return _window_call("palette_maps_device", labels, [g[0] * g[1] for g in grids], grids,
                        _palette_outputs(ns, counts, dominant), stream,
                        lambda ptrs, hs, ws, n, pc, pd, s: lib.phd_palette_maps_device(
                            ptrs, hs, ws, n, ns_arr, int(window), stride, pc, pd, s))


def set_bounding_boxes(bounding_boxes):
    """core.py:489-515."""
    n = len(bounding_boxes)
    arrs = {k: (ctypes.c_int * n)(*[b[k] for b in bounding_boxes]) for k in ("top", "bottom", "left", "right")}
    return Crop_Boundaries(N=n, **arrs)
