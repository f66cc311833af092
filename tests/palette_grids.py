"""Colour grids on every side of the two thresholds that decide which palette
kernels a report runs, shared by tests/test_palette_paths.py (the path hook, no
GPU) and tests/test_gpu_palette_grids.py (the kernels against the C oracle).

The path of a configuration is a mask from phd_debug_palette_path
(include/photohive_dsp.h), which asks the functions run_reports asks:
FUSED the one-pass palette (fused_palette_ok: K1's sums and hue cells fit its
LDS), else K1 histogram + Kcut + K3; TABLE / TABLE2 the table K1 of k1.hip and
its two-block form; THR the saturation class from per-value thresholds
(s_partitions <= 6), else from ClassTables::si8 in global memory (the kernels'
kThr = false instantiations); CODES the grid has a K1 code table; BATCHED the
second pass of an image with that many palette slots is one Kcut and one K3
launch per batch, else a pair of launches per image."""
import ctypes

FUSED, TABLE, TABLE2, THR, CODES, BATCHED = 1, 2, 4, 8, 16, 32
GRID_BITS = FUSED | TABLE | TABLE2 | THR | CODES     # decided by the grid alone (BATCHED: also by the slot count)

# name -> (config, expected GRID_BITS); what each row is here for:
GRIDS = {
    # table K1 (one block per CU) with a code table of 8 * 3 colour codes; unaligned batches take the fused
    # k_hsv_stats, kThr = false
    "s8_table": (dict(h_partitions=18, s_partitions=8, v_partitions=3), FUSED | TABLE | CODES),
    # palette.hip's fused K1, kThr = false
    "s12_fused": (dict(h_partitions=12, s_partitions=12, v_partitions=12), FUSED | CODES),
    # two-pass path, kThr = true
    "h360_s4": (dict(h_partitions=360, s_partitions=4, v_partitions=2), THR | CODES),
    # two-pass path, kThr = false
    "s10_twopass": (dict(h_partitions=36, s_partitions=10, v_partitions=10), CODES),
    # two-pass path; with coverage 1.0 on noise more slots than the batched K3 holds
    "h180_fine": (dict(h_partitions=180, s_partitions=4, v_partitions=5), THR | CODES),
    # the largest grid the library accepts (4096 groups): no code table
    "max_grid": (dict(h_partitions=8, s_partitions=73, v_partitions=7), 0),
}

# the grids the rest of the suite leans on: (config, bits set, bits clear)
LEGACY = {
    "18_2_3": (dict(), FUSED | TABLE | TABLE2 | THR, 0),
    "36_4_5": (dict(h_partitions=36, s_partitions=4, v_partitions=5), FUSED | TABLE, TABLE2),
    "360_2_3": (dict(h_partitions=360), FUSED, TABLE),
}


# single 600 x 800 reports (tests/test_gpu_palette_grids.py): case -> (grid, further parameters), each on every
# kind of REPORT_KINDS (seed 11): exact hues on bin edges, many slots, flat regions, grey groups
REPORT_CASES = dict({name: (name, {}) for name in GRIDS},
                    h180_fine_cov1=("h180_fine", dict(coverage_thresh=1.0)),
                    s10_twopass_l50=("s10_twopass", dict(linked_list_size=50)),
                    h360_s4_l50=("h360_s4", dict(linked_list_size=50)))
REPORT_KINDS = ("posterized", "uniform", "structured", "grayish")
REPORT_SHAPE = (600, 800)
# ... whose oracle slot count takes the per-image Kcut / K3 (every other one: the batched tail).  The batched
# K3's LDS is not monotonic in the slot count (fewer slots get more lane-private copies), so 102 slots of
# max_grid and 862 of h180_fine do not fit where 479 and 2429 do.
PER_IMAGE_TAIL = {("max_grid", "posterized"), ("max_grid", "uniform"),
                  ("h180_fine_cov1", "uniform"), ("h180_fine_cov1", "structured")}

# the 4096 x 4096 image of every RGB8 triple: case -> (grid, further parameters, oracle slots, batched tail)
CUBE_CASES = {
    "h360_s4_cov1": ("h360_s4", dict(coverage_thresh=1.0), 2876, True),
    "s10_twopass": ("s10_twopass", {}, 2410, True),
    "max_grid_cov1": ("max_grid", dict(coverage_thresh=1.0), 4090, False),
}


def grid(name, **extra):
    """The configuration of a grid of the table, with further report parameters."""
    return dict(GRIDS[name][0], **extra)


def groups(cfg):
    """h s v + v + 1: colour groups, the grey groups and the black group."""
    h, s, v = (cfg.get(k, d) for k, d in (("h_partitions", 18), ("s_partitions", 2), ("v_partitions", 3)))
    return h * s * v + v + 1


def path(cfg, max_slots=1):
    """phd_debug_palette_path of a configuration (a dict of report parameters)."""
    from photohive_dsp_amd.core import make_config
    from photohive_dsp_amd.lib import lib
    c = make_config(**cfg)
    return lib.phd_debug_palette_path(ctypes.byref(c), max_slots)


def describe(mask):
    names = ("fused", "table", "table2", "thr", "codes", "batched")
    return f"{mask:#04x} [" + " ".join(n for i, n in enumerate(names) if mask >> i & 1) + "]"
