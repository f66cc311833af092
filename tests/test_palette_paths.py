"""Which palette kernels a configuration runs (phd_debug_palette_path, host
only): the grids of tests/palette_grids.py sit where their rows say, on both
sides of the fused K1's LDS limit (fused_palette_ok) and of the threshold form
of the saturation class (kSiThresholds), so tests/test_gpu_palette_grids.py
reaches the kernels it names.  A later change of an LDS budget that moves a
grid to another path fails here, without a GPU."""
import functools

import numpy as np
import pytest

from tests import palette_grids as pg


@pytest.mark.parametrize("name", list(pg.GRIDS))
def test_grid_takes_the_path_of_its_row(name):
    cfg, bits = pg.GRIDS[name]
    m = pg.path(cfg)
    assert m >= 0
    assert m & pg.GRID_BITS == bits, f"{name}: {pg.describe(m)}, expected {pg.describe(bits)}"


def test_grids_cover_both_sides_of_both_thresholds():
    masks = {name: pg.path(cfg) for name, (cfg, _) in pg.GRIDS.items()}
    for fused in (0, pg.FUSED):
        for thr in (0, pg.THR):
            if fused and thr:
                continue                                   # the grids of the rest of the suite (below)
            assert any(m & (pg.FUSED | pg.THR) == fused | thr for m in masks.values()), (fused, thr, masks)
    assert any(m & pg.TABLE and not m & pg.THR for m in masks.values())      # a code table built for s > 6
    assert any(not m & pg.CODES for m in masks.values())
    assert all(pg.groups(cfg) > 2164 for name, (cfg, _) in pg.GRIDS.items() if not masks[name] & pg.FUSED)


@pytest.mark.parametrize("name", list(pg.LEGACY))
def test_grids_of_the_rest_of_the_suite_keep_their_path(name):
    cfg, on, off = pg.LEGACY[name]
    m = pg.path(cfg)
    assert m >= 0 and m & on == on and m & off == 0, f"{name}: {pg.describe(m)}"


def test_batched_tail_depends_on_the_slot_count():
    for name in ("h180_fine", "max_grid"):
        cfg = pg.grid(name)
        assert pg.path(cfg, 1) & pg.BATCHED, name
        assert not pg.path(cfg, pg.groups(cfg)) & pg.BATCHED, name
        assert pg.path(cfg, 1) & pg.GRID_BITS == pg.path(cfg, pg.groups(cfg)) & pg.GRID_BITS
    cfg = pg.grid("h360_s4")
    assert pg.path(cfg, 1) & pg.BATCHED and pg.path(cfg, pg.groups(cfg)) & pg.BATCHED
    # a fused palette's second pass (the partial groups alone) is always the batched one
    for name in ("s8_table", "s12_fused"):
        cfg = pg.grid(name)
        assert all(pg.path(cfg, s) & pg.BATCHED for s in (1, pg.groups(cfg) // 2, pg.groups(cfg)))


def test_largest_grid_is_accepted_and_the_next_rejected():
    from photohive_dsp_amd.lib import last_error
    assert pg.groups(pg.grid("max_grid")) == 4096
    assert pg.path(pg.grid("max_grid")) >= 0
    over = dict(h_partitions=9, s_partitions=65, v_partitions=7)
    assert pg.groups(over) == 4103
    assert pg.path(over) == -1 and "4096" in last_error()
    assert pg.path(dict(h_partitions=1, s_partitions=128, v_partitions=1)) == -1 and "127" in last_error()
    assert pg.path(dict(h_partitions=1, s_partitions=127, v_partitions=1)) >= 0
    assert pg.path(dict(h_partitions=7)) == -1 and "divide 360" in last_error()


@functools.lru_cache(maxsize=None)
def _image(kind):
    from photohive_dsp_amd import synth
    img = synth.make(kind, *pg.REPORT_SHAPE, 11)
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("case", list(pg.REPORT_CASES))
def test_report_cases_reach_their_tail_and_keep_cutoffs(case):
    """The oracle's side of the GPU cases: its slot count puts each
    (case, image) on the tail pg.PER_IMAGE_TAIL says, and every case but the
    coverage 1.0 one has parents whose kept count differs from their histogram
    count, so the keep-cutoff kernels have work."""
    from oracle import oracle as orc
    name, extra = pg.REPORT_CASES[case]
    cfg = pg.grid(name, **extra)
    for kind in pg.REPORT_KINDS:
        o = orc.palette(_image(kind), **cfg)
        ns = len(o["valid_parents"])
        batched = bool(pg.path(cfg, ns) & pg.BATCHED)
        assert batched == ((case, kind) not in pg.PER_IMAGE_TAIL), (case, kind, ns)
        moved = int(np.count_nonzero(o["kept"] != o["hist"][o["valid_parents"]]))
        if extra.get("coverage_thresh") == 1.0:
            assert moved == 0 and ns == np.count_nonzero(o["hist"])
        else:
            assert moved >= 1, (case, kind)
    tails = {(case, kind) in pg.PER_IMAGE_TAIL for kind in pg.REPORT_KINDS}
    if case in ("max_grid", "h180_fine_cov1"):
        assert tails == {True, False}                      # both tails on one grid
