"""Palette label map fixtures, shared by tests/golden/make_label_golden.py (the
generator: the reference's own C), tests/test_label_golden.py (no GPU) and
tests/test_gpu_labels.py.

A fixture (tests/golden/labels_<name>.npz) holds a map in compact form:
group_slot[TL] (the palette slot of each arm_octree group's kept pixels, -1
when it keeps none), dropped (sorted raster indices of the pixels in no list),
shape (mh, mw), counts (pixels per slot) and sha256 (of the little-endian
uint16 map bytes).  The expected map is group_slot[oracle.group_ids(image)]
with the dropped pixels set to NONE."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = 0xFFFF

# (name, synth kind, height, width, seed, configuration, the same-named case of manifest.json or None)
CASES = [
    ("uniform_401x577_L64", "uniform", 401, 577, 6, dict(linked_list_size=64), "uniform_401x577_L64"),
    ("motion_401x577_L64", "motion", 401, 577, 5, dict(linked_list_size=64), None),
    ("structured_577x401_L64", "structured", 577, 401, 7, dict(linked_list_size=64), "structured_577x401_L64"),
    ("dominant_512x768", "dominant", 512, 768, 9, {}, "dominant_512x768"),
    ("black_400", "black", 400, 400, 0, {}, "black_400"),
    ("uniform_512_hsv36_4_5", "uniform", 512, 512, 10, dict(h_partitions=36, s_partitions=4, v_partitions=5),
     "uniform_512_hsv36_4_5"),
    ("structured_600x800_hsv36_L200", "structured", 600, 800, 11,
     dict(h_partitions=36, s_partitions=4, v_partitions=5, linked_list_size=200), "structured_600x800_hsv36_L200"),
    ("structured_720x1280_ds2", "structured", 720, 1280, 12, dict(downsample_rate=2), "structured_720x1280_ds2"),
    ("uniform_700x900_ds3_L50", "uniform", 700, 900, 13, dict(downsample_rate=3, linked_list_size=50),
     "uniform_700x900_ds3_L50"),
]


def manifest():
    with open(os.path.join(GOLDEN, "labels_manifest.json")) as f:
        return json.load(f)["cases"]


def fixture(name):
    with np.load(os.path.join(GOLDEN, f"labels_{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def image(case):
    from photohive_dsp_amd import synth
    return synth.make(case["kind"], case["height"], case["width"], case["seed"])


def map_shape(height, width, ds):
    return (height // ds, width // ds) if ds > 1 else (height, width)


def hsv_image(img, ds):
    """The image rgb2hsv sees (src/interface.c:46): img, or for downsample_rate
    ds > 1 downsample_rgb's image with its row quirk (src/image_processing.c:
    344-366): new pixel (y, x) is old flat pixel y * (ds - 1) * W + x * ds."""
    if ds <= 1:
        return img
    h, w = img.shape[:2]
    mh, mw = h // ds, w // ds
    y, x = np.divmod(np.arange(mh * mw, dtype=np.int64), mw)
    return img.reshape(-1, 3)[y * (ds - 1) * w + x * ds].reshape(mh, mw, 3)


def expected_map(case, fx, img=None):
    """The fixture's label map, uint16 [mh, mw], rebuilt through the C oracle's
    per-pixel groups."""
    from oracle import oracle as orc
    cfg = case["config"]
    img = image(case) if img is None else img
    small = hsv_image(img, cfg.get("downsample_rate", 1))
    gid = orc.group_ids(np.ascontiguousarray(small), **{k: v for k, v in cfg.items() if k != "downsample_rate"})
    lab = fx["group_slot"].astype(np.int32)[gid].astype(np.uint16)        # -1 -> NONE
    lab[fx["dropped"]] = NONE
    return lab.reshape(tuple(int(v) for v in fx["shape"]))


def map_sha256(lab):
    return hashlib.sha256(np.ascontiguousarray(lab, dtype="<u2").tobytes()).digest()


def slot_counts(lab, n_slots):
    lab = np.asarray(lab).reshape(-1).astype(np.uint16)
    return np.bincount(lab[lab != NONE], minlength=n_slots)[:n_slots]


def percentages(counts, n_pixels):
    """calculate_avg_hsv's percentages (src/color_quantization.c:572):
    (double)count * (1.0 / (double)n)."""
    return np.asarray(counts, dtype=np.float64) * (1.0 / float(n_pixels))
