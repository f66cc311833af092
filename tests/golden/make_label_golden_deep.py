"""Palette label map fixtures for images that are not 8-bit, from the
reference's own C (oracle/_ref): tests/golden/labels_deep_<name>.npz and
labels_deep_manifest.json.

    python -m tests.golden.make_label_golden_deep

The images are synth.deep's doubles (a 16-bit image / 65535: rint(x * 65535)
reproduces the uint16 it came from), which oracle/ref_pipeline.py hands to the
reference as the doubles themselves -- what a C caller of get_full_report_data
(src/interface.c:20-94) passes.  make_label_golden.reference_labels runs the
reference on them and reads its lists back (see that module).
oracle.group_ids restates arm_octree for 8-bit images only, so the compact
fixture form of tests/label_cases.py cannot be rebuilt for doubles: a fixture
here stores the full map (`map`, uint16 [mh, mw], compressed), `counts`
(pixels per slot), `percentages` (the reference's own), `shape` and `sha256`
(of the little-endian uint16 map bytes).

Asserted before anything is written, as make_label_golden.py asserts what
needs no group_ids: every pixel is in at most one list (reference_labels); per
slot percentages[i] == (double)count * (1.0 / (double)n) bit for bit; and
tests/label_cases.py's hsv_image equals downsample_rgb's image on the doubles
(src/image_processing.c:344-366)."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_pipeline as rp  # noqa: E402
from photohive_dsp_amd import synth  # noqa: E402
from tests import label_cases as lc  # noqa: E402
from tests.golden.make_label_golden import reference_labels  # noqa: E402

MAX_BYTES = 150 * 1024

# (name, synth.deep kind, height, width, seed, configuration)
CASES = [
    ("structured_353x401_L50", "structured", 353, 401, 3, dict(linked_list_size=50)),
    ("dominant_353x401_L50", "dominant", 353, 401, 4, dict(linked_list_size=50)),
    ("structured_706x802_ds2_L40", "structured", 706, 802, 5, dict(downsample_rate=2, linked_list_size=40)),
]


def downsampled_doubles(img, ds):
    """downsample_rgb's image of the doubles (float64 [mh, mw, 3]); img for ds <= 1."""
    if ds <= 1:
        return img
    L = rp.lib()
    im, _keep = rp._image_rgb(img)
    out = L.downsample_rgb(C.pointer(im), ds)
    mh, mw = out.contents.height, out.contents.width
    small = np.stack([np.ctypeslib.as_array(getattr(out.contents, c), shape=(mh * mw,)).copy() for c in "rgb"],
                     axis=-1).reshape(mh, mw, 3)
    L.free_image_rgb(out)
    return small


def fixture(name, kind, h, w, seed, kw):
    img = synth.deep(kind, h, w, seed)
    assert img.dtype == np.float64 and np.array_equal(np.rint(img * 65535.0) / 65535.0, img)
    cfg = rp.Config(**kw)
    lab, _ref_gid, pct, _small = reference_labels(img, cfg)
    n = lab.size
    assert lab.shape == lc.map_shape(h, w, cfg.downsample_rate)
    small = downsampled_doubles(img, cfg.downsample_rate)
    assert np.array_equal(small.view(np.int64), lc.hsv_image(img, cfg.downsample_rate).view(np.int64)), \
        "hsv_image differs from downsample_rgb"
    counts = lc.slot_counts(lab, len(pct))
    assert np.array_equal(lc.percentages(counts, n).view(np.int64), pct.view(np.int64)), "count identity"
    dropped = int((lab == lc.NONE).sum())
    assert int(counts.sum()) + dropped == n
    print(f"{name}: map {lab.shape}, {len(pct)} slots, {dropped} dropped", flush=True)
    return dict(map=np.ascontiguousarray(lab, dtype="<u2"), counts=counts.astype(np.int64),
                percentages=pct.astype(np.float64), shape=np.array(lab.shape, dtype=np.int32),
                sha256=np.frombuffer(lc.map_sha256(lab), dtype=np.uint8))


def main():
    cases = []
    for name, kind, h, w, seed, kw in CASES:
        fx = fixture(name, kind, h, w, seed, kw)
        path = os.path.join(HERE, f"labels_deep_{name}.npz")
        np.savez_compressed(path, **fx)
        size = os.path.getsize(path)
        assert size < MAX_BYTES, f"{path}: {size} bytes"
        print(f"  {os.path.basename(path)}: {size} bytes", flush=True)
        cases.append(dict(name=name, kind=kind, height=h, width=w, seed=seed, config=kw,
                          shape=[int(v) for v in fx["shape"]], slots=int(len(fx["counts"])),
                          dropped=int(fx["map"].size - fx["counts"].sum())))
    with open(os.path.join(HERE, "labels_deep_manifest.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
