"""The fp64 label map fixtures (tests/golden/labels_deep_<name>.npz, made by
tests/golden/make_label_golden_deep.py), shared by tests/test_label_golden_deep.py
(no GPU) and tests/test_gpu_labels_inputs.py.

A fixture holds the reference's full map: map (uint16 [mh, mw]), counts
(pixels per slot), percentages (the reference's), shape and sha256 (of the
little-endian uint16 map bytes).  The image is synth.deep's doubles."""
import json
import os

import numpy as np

from tests.label_cases import GOLDEN


def manifest():
    with open(os.path.join(GOLDEN, "labels_deep_manifest.json")) as f:
        return json.load(f)["cases"]


def path(name):
    return os.path.join(GOLDEN, f"labels_deep_{name}.npz")


def fixture(name):
    with np.load(path(name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def image(case):
    """float64 [H, W, 3]: a 16-bit image / 65535."""
    from photohive_dsp_amd import synth
    return synth.deep(case["kind"], case["height"], case["width"], case["seed"])


def u16_of(img):
    """The 16-bit image whose values / 65535.0 are exactly the doubles of synth.deep."""
    u16 = np.rint(img * 65535.0).astype(np.uint16)
    assert np.array_equal(u16 / 65535.0, img)
    return u16
