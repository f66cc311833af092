"""The palette on colour grids outside the fused K1's range and past the
threshold form of the saturation class (tests/palette_grids.py), against the C
oracle's per-pixel arm_octree / group_irregular_pixels / calculate_avg_hsv
(oracle/phd_oracle.c: one loop for any grid).

Reached here and nowhere else in the suite: the kThr = false instantiations of
palette.hip (si_of reads ClassTables::si8 from global memory), the
histogram-only K1 with k_cutoffs_b and the batched K3 k_palette_sums_b at full
resolution, the per-image k_cutoffs / k_palette_sums at downsample_rate 1, the
table K1 with a code table built for s_partitions > 6, grids without a code
table, and the kAligned = false forms of all of them.

Bars: group ids, palette order, quantities, hist and kept bit-exact; palette
HSV and S-bar at TIGHT_RTOL (atol 1e-12 on HSV).  Every test first asserts,
from phd_debug_palette_path and the oracle's slot count, the path it was
written for, and prints it with the largest HSV error it saw."""
import functools

import numpy as np
import pytest

from tests import palette_grids as pg
from tests.test_gpu_parity import TIGHT_RTOL, _phd, _trace, check_hsv_groups_rgb_cube

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _image(kind, h, w, seed):
    from photohive_dsp_amd import synth
    img = np.ascontiguousarray(synth.make(kind, h, w, seed))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _cube_image():
    k = np.arange(1 << 24, dtype=np.uint32)
    cube = np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)
    cube.setflags(write=False)
    return cube


def _oracle(img, cfg):
    from oracle import oracle as orc
    return orc.palette(img, **cfg)


def _assert_path(label, cfg, name, slots, batched):
    """The grid bits of the table's row and the tail of this slot count."""
    m = pg.path(cfg, slots)
    print(f"{label}: {slots} slots, path {pg.describe(m)}")
    assert m >= 0
    assert m & pg.GRID_BITS == pg.GRIDS[name][1], pg.describe(m)
    assert batched is None or bool(m & pg.BATCHED) == batched, f"{slots} slots: {pg.describe(m)}"
    return m


def _hsv_rel_err(got, want):
    d = np.abs(got - want)
    nz = want != 0
    return float(np.max(d[nz] / np.abs(want[nz]))) if nz.any() else 0.0


def _check_palette(label, rep, o, hsv=True):
    cp = rep.color_palette
    np.testing.assert_array_equal(np.array(cp.group_ids), o["valid_parents"])
    np.testing.assert_array_equal(np.array(cp.quantities), o["palette_pct"])
    np.testing.assert_allclose(rep.average_saturation, o["average_saturation"], rtol=TIGHT_RTOL)
    if hsv:
        got = np.array(cp.hsv).reshape(-1, 3)
        print(f"{label}: max rel HSV err {_hsv_rel_err(got, o['palette_hsv']):.3e}")
        np.testing.assert_allclose(got, o["palette_hsv"], rtol=TIGHT_RTOL, atol=1e-12)


# ---- a. per-pixel classification over every RGB8 triple -----------------------

CUBE_PIXEL_CFGS = {
    "s8_table": pg.grid("s8_table"),
    "s10_twopass": pg.grid("s10_twopass"),
    "max_grid": pg.grid("max_grid"),
    # no black and no grey pixels: a colour group (si >= 0) for every triple
    "max_grid_no_gray": pg.grid("max_grid", black_thresh=0.0, gray_thresh=0.0),
}


@pytest.mark.parametrize("case", list(CUBE_PIXEL_CFGS))
def test_hsv_group_rgb_cube_si8_table(case):
    """k_debug_hsv<false>: group id and h, s, v of all 2^24 triples bit-equal
    to the oracle's, with Si from the table in global memory."""
    cfg = CUBE_PIXEL_CFGS[case]
    m = pg.path(cfg)
    print(f"{case}: path {pg.describe(m)}")
    assert m >= 0 and not m & pg.THR
    check_hsv_groups_rgb_cube(cfg)


# ---- b. single reports ----------------------------------------------------------

@pytest.mark.parametrize("kind", pg.REPORT_KINDS)
@pytest.mark.parametrize("case", list(pg.REPORT_CASES))
def test_report_and_trace_against_oracle(case, kind):
    phd, L, _ = _phd()
    name, extra = pg.REPORT_CASES[case]
    cfg = pg.grid(name, **extra)
    img = _image(kind, *pg.REPORT_SHAPE, 11)
    o = _oracle(img, cfg)
    label = f"{case}/{kind}"
    _assert_path(label, cfg, name, len(o["valid_parents"]), (case, kind) not in pg.PER_IMAGE_TAIL)
    moved = int(np.count_nonzero(o["kept"] != o["hist"][o["valid_parents"]]))
    if extra.get("coverage_thresh") != 1.0:
        assert moved >= 1, "no parent took pixels of other groups: the keep rules have no work"
    _check_palette(label, phd.get_report(img, **cfg), o)
    # the two-pass kernels' intermediates (the trace runs K1 histogram + Kcut + K3 on every grid)
    hist, parents, kept = _trace(img, **cfg)
    np.testing.assert_array_equal(hist, o["hist"])
    np.testing.assert_array_equal(parents, o["valid_parents"])
    np.testing.assert_array_equal(kept, o["kept"])


# ---- c. whole-group sums over every colour --------------------------------------

@pytest.mark.parametrize("case", list(pg.CUBE_CASES))
def test_rgb_cube_palette_two_pass(case):
    """The 4096 x 4096 image of all 256^3 triples through the two-pass
    palette.  With coverage 1.0 every non-empty group is a slot kept whole, so
    each group's count and h / s / v sums over all its colours are compared."""
    phd, L, _ = _phd()
    name, extra, slots, batched = pg.CUBE_CASES[case]
    cfg = pg.grid(name, **extra)
    o = _oracle(_cube_image(), cfg)
    assert len(o["valid_parents"]) == slots
    m = _assert_path(case, cfg, name, slots, batched)
    assert not m & pg.FUSED
    if extra.get("coverage_thresh") == 1.0:
        assert slots == np.count_nonzero(o["hist"])
        np.testing.assert_array_equal(o["kept"], o["hist"][o["valid_parents"]])
    _check_palette(case, phd.get_report(_cube_image(), **cfg), o)


# ---- d. batches ------------------------------------------------------------------

@pytest.mark.parametrize("name,batched", [("s8_table", True), ("h360_s4", True), ("s10_twopass", True),
                                          ("max_grid", False)])
def test_unaligned_batch_against_oracle(name, batched):
    """Three 401 x 577 images in one tensor: 694131 bytes each, so images 1 and
    2 are not word-aligned and the batch takes the kAligned = false kernels
    (s8_table: the fused k_hsv_stats instead of the table K1; max_grid: the
    noise image has more slots than the batched K3 holds, so every image takes
    the per-image K3's byte loads, and 401 * 577 is odd: its partial final
    group).  Every image against the oracle, and the batch against three
    single calls."""
    phd, L, torch = _phd()
    h, w = 401, 577
    assert (h * w * 3) % 4 != 0 and (2 * h * w * 3) % 4 != 0 and (h * w) % 4 != 0
    cfg = pg.grid(name)
    imgs = [_image(k, h, w, 30 + i) for i, k in enumerate(("uniform", "structured", "posterized"))]
    os_ = [_oracle(img, cfg) for img in imgs]
    fused = bool(pg.GRIDS[name][1] & pg.FUSED)
    # the batch's tail is chosen by its largest slot count (the noise image's)
    for i, o in enumerate(os_):
        _assert_path(f"{name}/single {i}", cfg, name, len(o["valid_parents"]), True if batched else None)
    m = _assert_path(f"{name}/batch", cfg, name, max(len(o["valid_parents"]) for o in os_), batched)
    assert bool(m & pg.FUSED) == fused
    t = torch.from_numpy(np.stack(imgs)).cuda()
    assert t.data_ptr() % 4 == 0 and t[1].data_ptr() % 4 != 0 and t[2].data_ptr() % 4 != 0
    batch = phd.report_device(t, **cfg)
    for i, (img, rb, o) in enumerate(zip(imgs, batch, os_)):
        _check_palette(f"{name}/batch image {i}", rb, o)
        one = phd.report_device(t[i:i + 1].clone(), **cfg)[0]          # (a tensor of its own: word-aligned)
        assert one.color_palette.group_ids == rb.color_palette.group_ids
        assert one.color_palette.quantities == rb.color_palette.quantities


def test_batched_k3_runs_cross_images():
    """Forty 600 x 800 images, s10_twopass: 1200 chunk items against one K3
    block per CU, so a block's run of items walks from one image into the next
    (its rules and slot offsets reloaded, its sums flushed per image)."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    h, w, n = 600, 800, 40
    cfg = pg.grid("s10_twopass")
    nchunks = -(-h * w // 16384)
    assert n * nchunks == 1200 and nchunks == 30
    t = torch.empty(n * h * w * 3, dtype=torch.uint8, device="cuda")
    for i in range(n):
        assert L.lib.phd_fill_uniform_device(t[i * h * w * 3:].data_ptr(), h * w * 3, 200 + i, None) == 0
    os_ = [_oracle(synth.uniform(h, w, 200 + i), cfg) for i in range(n)]
    for o in os_:
        assert pg.path(cfg, len(o["valid_parents"])) & pg.BATCHED
    _assert_path("s10_twopass/40 images", cfg, "s10_twopass", max(len(o["valid_parents"]) for o in os_), True)
    reps = phd.report_device(t.view(n, h, w, 3), **cfg)
    for i, (r, o) in enumerate(zip(reps, os_)):
        _check_palette(f"s10_twopass/image {i} of 40", r, o, hsv=i in (0, 19, 39))
