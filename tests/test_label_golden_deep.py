"""The fp64 label map fixtures (tests/golden/labels_deep_*.npz, made by
tests/golden/make_label_golden_deep.py from the reference's own C) are whole:
each loads, its map has the stored SHA-256 and the manifest's shape, and its
stored percentages are calculate_avg_hsv's (double)count * (1.0 / (double)n)
of its counts, bit for bit."""
import os

import numpy as np
import pytest

from tests import deep_label_cases as dc
from tests import label_cases as lc

CASES = dc.manifest()


def test_manifest_lists_the_cases():
    assert [c["name"] for c in CASES] == ["structured_353x401_L50", "dominant_353x401_L50",
                                          "structured_706x802_ds2_L40"]
    for c in CASES:
        assert os.path.getsize(dc.path(c["name"])) < 150 * 1024, c["name"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_is_whole(case):
    fx = dc.fixture(case["name"])
    lab = fx["map"]
    ds = case["config"].get("downsample_rate", 1)
    assert lab.dtype == np.uint16 and lab.shape == tuple(fx["shape"]) == tuple(case["shape"])
    assert lab.shape == lc.map_shape(case["height"], case["width"], ds) == (353, 401)
    assert lc.map_sha256(lab) == fx["sha256"].tobytes()
    n_slots = len(fx["counts"])
    assert n_slots == case["slots"] == len(fx["percentages"])
    np.testing.assert_array_equal(lc.slot_counts(lab, n_slots), fx["counts"])
    assert int((lab == lc.NONE).sum()) == case["dropped"] > 0             # every case has tie-overflow drops
    assert int(lab[lab != lc.NONE].max()) == n_slots - 1
    got = lc.percentages(fx["counts"], lab.size)
    assert np.array_equal(got.view(np.int64), fx["percentages"].view(np.int64))


def test_images_are_sixteen_bit_and_not_eight_bit():
    """rint(x * 65535) reproduces the doubles, and they are no 8-bit image
    (so the typed entry takes the fp64 route)."""
    for case in CASES:
        img = dc.image(case)
        u16 = dc.u16_of(img)
        assert u16.dtype == np.uint16 and img.shape == (case["height"], case["width"], 3)
        assert not np.array_equal(np.rint(img * 255.0) / 255.0, img)
