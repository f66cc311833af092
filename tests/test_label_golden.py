"""The palette label map fixtures (tests/golden/labels_*.npz, written from the
reference's own C by tests/golden/make_label_golden.py) against themselves and
against the report fixtures of the same images: no GPU."""
import numpy as np
import pytest

from tests import label_cases as lc
from tests.conftest import golden_case

CASES = lc.manifest()


def test_manifest_lists_every_case():
    assert [(c["name"], c["kind"], c["height"], c["width"], c["seed"], c["config"], c["base"]) for c in CASES] == \
        [tuple(c) for c in lc.CASES]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_is_consistent(case):
    fx = lc.fixture(case["name"])
    mh, mw = (int(v) for v in fx["shape"])
    assert (mh, mw) == lc.map_shape(case["height"], case["width"], case["config"].get("downsample_rate", 1))
    n = mh * mw
    dropped = fx["dropped"].astype(np.int64)
    assert np.all(np.diff(dropped) > 0), "dropped indices are sorted and distinct"
    assert len(dropped) == 0 or (dropped[0] >= 0 and dropped[-1] < n)
    assert int(fx["counts"].sum()) + len(dropped) == n
    slots = fx["group_slot"]
    assert slots.min() >= -1 and slots.max() == len(fx["counts"]) - 1
    if case["base"]:
        g = golden_case(case["base"])
        np.testing.assert_array_equal(fx["counts"], g["kept"])
        # percentages[i] == (double)count * (1.0 / (double)n), bit for bit
        np.testing.assert_array_equal(lc.percentages(fx["counts"], n).view(np.int64), g["palette_pct"].view(np.int64))
        # the slot of a parent's own group is its place in valid_parents
        np.testing.assert_array_equal(slots[g["valid_parents"]], np.arange(len(g["valid_parents"])))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_rebuilt_map_has_the_recorded_hash(case):
    fx = lc.fixture(case["name"])
    lab = lc.expected_map(case, fx)
    assert lab.dtype == np.uint16 and lab.shape == tuple(int(v) for v in fx["shape"])
    assert lc.map_sha256(lab) == fx["sha256"].tobytes()
    np.testing.assert_array_equal(lc.slot_counts(lab, len(fx["counts"])), fx["counts"])
    assert int(np.count_nonzero(lab == lc.NONE)) == len(fx["dropped"])
