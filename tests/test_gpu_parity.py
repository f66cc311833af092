"""GPU parity: the HIP path through the C-ABI against the reference's golden
vectors (tests/golden, produced by the reference's own C) and the CPU oracle.

Bars (BASELINE.json north_star): histogram counts, palette group ids/order,
kept-pixel counts, blur bin counts and percentages bit-exact; float fields
within 1e-4 relative (observed ~1e-12: fp64 everywhere, only summation order
and libm ulps differ).
"""
import ctypes
import os

import numpy as np
import pytest

from tests.conftest import golden_case, golden_image, golden_manifest

pytestmark = pytest.mark.gpu

FLOAT_RTOL = 1e-4          # north_star tolerance for float fields
TIGHT_RTOL = 1e-9          # what fp64 actually delivers; tracked, not the contract
# the column passes sum log(p) in fp64 (fft_ct.hip: e ln2 + fp64 log of each
# run's mantissa product) in bin_scale fixed point; what remains is the FFT
# (ours vs pocketfft standing in for FFTW) and the fixed-point rounding:
# tracked, not the contract
BINS_TIGHT_RTOL = 1e-10
# and normwise, |bins - fixture| <= BINS_NORMWISE * max|fixture|: 7e-12 or less
# on every fixture but one (tools/bins_err.py).  On dominant_3000x4000_intmin
# the spectrum's max is the DC term, N (mean luma - avg): a cancellation that
# turns the fixture's own rounding of the channel means (the reference sums
# 12 M values of one dominant colour sequentially in fp64, so the errors add
# up instead of averaging out) into 1.37e-9 on fft_max; ours, from exact
# integer sums, is within 6e-14 of a numpy restatement (tools/fmax_probe.py
# run, round 3).  G_s = 1 / (2 log(sqrt(max) + 1)) carries that to every bin.
BINS_NORMWISE = 1e-11
BINS_NORMWISE_EXCEPT = {"dominant_3000x4000_intmin": 1e-10}

CASES = golden_manifest()["cases"]


def _phd():
    import photohive_dsp_amd as phd
    from photohive_dsp_amd import lib as L
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return phd, L, torch


def _crops(case):
    from photohive_dsp_amd import set_bounding_boxes
    return set_bounding_boxes(case["crops"]) if case["crops"] else None


def _trace(img, **kw):
    """palette intermediates (hist, parents, kept) of the device path."""
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import make_config
    cfg = make_config(**kw)
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    tl = cfg.h_partitions * cfg.s_partitions * cfg.v_partitions + cfg.v_partitions + 1
    hist = (ctypes.c_int * tl)()
    parents = (ctypes.c_int * tl)()
    kept = (ctypes.c_int * tl)()
    npar = ctypes.c_int()
    rc = L.lib.phd_palette_trace_device(t.data_ptr(), img.shape[0], img.shape[1], ctypes.byref(cfg),
                                        hist, parents, kept, ctypes.byref(npar))
    assert rc == tl, L.last_error()
    n = npar.value
    return np.array(hist[:]), np.array(parents[:n]), np.array(kept[:n])


def assert_report_matches(rep, g, rtol=FLOAT_RTOL):
    st = rep.rgb_stats
    np.testing.assert_allclose([st.Br, st.Bg, st.Bb, st.Cr, st.Cg, st.Cb], g["stats"], rtol=rtol, atol=1e-15)
    np.testing.assert_allclose(rep.average_saturation, float(g["average_saturation"]), rtol=rtol, atol=1e-15)
    cp = rep.color_palette
    # palette indices and order: bit-exact
    np.testing.assert_array_equal(np.array(cp.group_ids), g["valid_parents"])
    # percentages = kept/N: bit-exact
    np.testing.assert_array_equal(np.array(cp.quantities), g["palette_pct"])
    np.testing.assert_allclose(np.array(cp.hsv).reshape(-1, 3), g["palette_hsv"], rtol=rtol, atol=1e-12)
    bins = np.array(rep.blur_profile.bins)
    np.testing.assert_allclose(bins, g["bins"], rtol=rtol, atol=1e-12)
    np.testing.assert_array_equal([v.angle for v in rep.blur_vectors], g["blur_angles"])
    np.testing.assert_array_equal(np.array([v.magnitude for v in rep.blur_vectors], np.float32), g["blur_mags"])
    assert rep.bp_ptr.angle_bin_size == int(g["angle_bin_size"])
    assert rep.bp_ptr.radius_bin_size == int(g["radius_bin_size"])
    if "sharpness" in g:
        np.testing.assert_allclose(rep.sharpnesses, g["sharpness"], rtol=rtol)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_report_matches_reference_fixture(case):
    phd, L, _ = _phd()
    g = golden_case(case["name"])
    img = golden_image(case)
    rep = phd.get_report(img, salient_characters=_crops(case), **case["config"])
    assert_report_matches(rep, g)
    # and the tighter bar fp64 actually reaches (reported separately for the record)
    st = rep.rgb_stats
    np.testing.assert_allclose([st.Br, st.Bg, st.Bb, st.Cr, st.Cg, st.Cb], g["stats"], rtol=TIGHT_RTOL)
    np.testing.assert_allclose(np.array(rep.blur_profile.bins), g["bins"], rtol=BINS_TIGHT_RTOL, atol=1e-13)
    bins = np.array(rep.blur_profile.bins)
    normwise = np.max(np.abs(bins - g["bins"])) / max(np.max(np.abs(g["bins"])), 1e-300)   # (all-zero bins: exact)
    assert normwise <= BINS_NORMWISE_EXCEPT.get(case["name"], BINS_NORMWISE), normwise


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_palette_intermediates_bit_exact(case):
    g = golden_case(case["name"])
    img = golden_image(case)
    hist, parents, kept = _trace(img, **case["config"])
    np.testing.assert_array_equal(hist, g["hist"])
    np.testing.assert_array_equal(parents, g["valid_parents"])
    np.testing.assert_array_equal(kept, g["kept"])


@pytest.mark.parametrize("case", [c for c in CASES if not c["config"].get("downsample_rate")][:6],
                         ids=lambda c: c["name"])
def test_blur_counts_bit_exact(case):
    phd, L, _ = _phd()
    g = golden_case(case["name"])
    na = case["config"].get("angle_partitions", 72)
    nr = case["config"].get("radius_partitions", 40)
    counts = (ctypes.c_longlong * (na * nr))()
    assert L.lib.phd_blur_counts(case["height"], case["width"], nr, na, counts) == 0
    np.testing.assert_array_equal(np.array(counts[:]).reshape(na, nr), g["bin_counts"])


def test_legacy_planar_double_entry_point():
    """get_full_report_data with the reference binding's planar doubles (utils.py:30-46)."""
    phd, L, _ = _phd()
    from photohive_dsp_amd.utils import pil_image_to_image_rgb
    from PIL import Image
    case = [c for c in CASES if c["name"] == "structured_384x512"][0]
    g = golden_case(case["name"])
    pil = Image.fromarray(golden_image(case))
    im = pil_image_to_image_rgb(pil)
    ptr = L.lib.get_full_report_data(ctypes.byref(im), None, 18, 2, 3, 0.1, 0.1, 0.95, 1000, 1, 40, 72,
                                     0.1, 0.9, 1.20, 0.3, 2)
    rep = phd.Report(ptr, case["height"], case["width"])
    assert_report_matches(rep, g)


def test_batch_device_matches_single_reports():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    imgs = [synth.make(k, 480, 640, s) for k, s in [("uniform", 1), ("structured", 2), ("hblur", 3)]]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    batch = phd.report_device(t)
    for img, rb in zip(imgs, batch):
        rs = phd.get_report(img)
        assert rs.color_palette.group_ids == rb.color_palette.group_ids
        assert rs.color_palette.quantities == rb.color_palette.quantities
        np.testing.assert_allclose(np.array(rb.blur_profile.bins), np.array(rs.blur_profile.bins), rtol=1e-12,
                                   atol=1e-14)


def test_batched_k1_runs_cross_images():
    """One K1 launch over 12 images (576 chunk items > one item per block, so block runs
    cross image boundaries): every image's palette and statistics equal the oracle's."""
    phd, L, torch = _phd()
    from oracle import oracle as orc
    from photohive_dsp_amd import synth
    h, w, n = 768, 1024, 12
    t = torch.empty(n * h * w * 3, dtype=torch.uint8, device="cuda")
    for i in range(n):
        assert L.lib.phd_fill_uniform_device(t[i * h * w * 3:].data_ptr(), h * w * 3, 100 + i, None) == 0
    reps = phd.report_device(t.view(n, h, w, 3))
    for i, r in enumerate(reps):
        img = synth.uniform(h, w, 100 + i)
        o = orc.palette(img)
        np.testing.assert_array_equal(np.array(r.color_palette.group_ids), o["valid_parents"])
        np.testing.assert_array_equal(np.array(r.color_palette.quantities), o["palette_pct"])
        st = r.rgb_stats
        np.testing.assert_allclose([st.Br, st.Bg, st.Bb, st.Cr, st.Cg, st.Cb], orc.stats(img), rtol=TIGHT_RTOL)
        np.testing.assert_allclose(r.average_saturation, o["average_saturation"], rtol=TIGHT_RTOL)


def test_hsv_stats_batch_config3_shape():
    """BASELINE config 3 pass (rgb2hsv + get_hsv_average + get_rgb_statistics) over a batch of
    1080p device images against the oracle."""
    phd, L, torch = _phd()
    from oracle import oracle as orc
    from photohive_dsp_amd import synth
    from photohive_dsp_amd.core import hsv_stats_device
    h, w, n = 1080, 1920, 20
    t = torch.empty(n * h * w * 3, dtype=torch.uint8, device="cuda")
    for i in range(n):
        assert L.lib.phd_fill_uniform_device(t[i * h * w * 3:].data_ptr(), h * w * 3, i, None) == 0
    stats, sat = hsv_stats_device(t.view(n, h, w, 3))
    for i in (0, 1, 9, 19):
        img = synth.uniform(h, w, i)
        st = stats[i]
        np.testing.assert_allclose([st.Br, st.Bg, st.Bb, st.Cr, st.Cg, st.Cb], orc.stats(img), rtol=TIGHT_RTOL)
        np.testing.assert_allclose(sat[i], orc.palette(img)["average_saturation"], rtol=STATS_SAT_RTOL)
    # a structured image (flat regions) in a batch of one
    img = synth.make("structured", h, w, 5)
    stats, sat = hsv_stats_device(torch.from_numpy(img[None]).cuda())
    st = stats[0]
    np.testing.assert_allclose([st.Br, st.Bg, st.Bb, st.Cr, st.Cg, st.Cb], orc.stats(img), rtol=TIGHT_RTOL)
    np.testing.assert_allclose(sat[0], orc.palette(img)["average_saturation"], rtol=STATS_SAT_RTOL)


# The statistics-only pass (stats.hip): exact integer sums of d per max value,
# finished on the host in fp64 -- the reference's width, within 1e-12 of its
# sequential fp64 sum.  The moments are exact.
STATS_SAT_RTOL = 1e-12


def stats_sat_rtol(npix):
    """The pass is bounded by the reference's own rounding: its S-bar is a
    sequential fp64 sum of npix per-pixel doubles (src/image_processing.c:533-540),
    whose error bound is npix * 2^-53 relative (reached on images where every
    pixel adds the same 0.999999)."""
    return max(STATS_SAT_RTOL, npix * 2.0 ** -53)


@pytest.mark.parametrize("kind,h,w", [("uniform", 401, 577), ("black", 400, 400), ("saturated", 360, 1200),
                                      ("grayish", 720, 1280), ("posterized", 600, 800)])
def test_hsv_stats_pass_edge_images(kind, h, w):
    """Odd pixel counts (partial final group, unaligned images of a batch), black
    (max == 0), fully saturated (min == 0: the 0.999999 case) and flat images."""
    phd, L, torch = _phd()
    from oracle import oracle as orc
    from photohive_dsp_amd import synth
    from photohive_dsp_amd.core import hsv_stats_device
    rng = np.random.default_rng(h * w)
    imgs = []
    for i in range(3):
        if kind == "black":
            img = np.zeros((h, w, 3), np.uint8)
            img[::7, ::5] = rng.integers(0, 3, (len(range(0, h, 7)), len(range(0, w, 5)), 3), dtype=np.uint8) * i
        elif kind == "saturated":
            img = synth.uniform(h, w, 40 + i).copy()
            img[..., i % 3] = 0
        elif kind == "posterized":
            img = (synth.make("structured", h, w, 60 + i) // 51 * 51).astype(np.uint8)
        else:
            img = synth.make(kind, h, w, 50 + i)
        imgs.append(np.ascontiguousarray(img))
    stats, sat = hsv_stats_device(torch.from_numpy(np.stack(imgs)).cuda())
    for i, img in enumerate(imgs):
        ref_st, ref_sat = orc.stats(img), orc.palette(img)["average_saturation"]
        # in the batch (odd sizes: unaligned images take K1's statistics form) and
        # alone (aligned: stats.hip, with the partial final group when h*w % 4 != 0)
        s1, a1 = hsv_stats_device(torch.from_numpy(img[None]).cuda())
        for st, sv in ((stats[i], sat[i]), (s1[0], a1[0])):
            np.testing.assert_allclose([st.Br, st.Bg, st.Bb, st.Cr, st.Cg, st.Cb], ref_st, rtol=TIGHT_RTOL)
            np.testing.assert_allclose(sv, ref_sat, rtol=stats_sat_rtol(h * w), atol=1e-15)


def test_hsv_stats_pass_batch_512_1080p_consistency():
    """BASELINE config 3 at full size (512 x 1080p, 3.2 GB resident): every image of
    the batch agrees with the same image run alone (runs cross image boundaries
    differently), and a sample agrees with the oracle."""
    phd, L, torch = _phd()
    from oracle import oracle as orc
    from photohive_dsp_amd import synth
    from photohive_dsp_amd.core import hsv_stats_device
    h, w, n = 1080, 1920, 512
    t = torch.empty(n * h * w * 3, dtype=torch.uint8, device="cuda")
    for i in range(n):
        assert L.lib.phd_fill_uniform_device(t[i * h * w * 3:].data_ptr(), h * w * 3, i, None) == 0
    v = t.view(n, h, w, 3)
    stats, sat = hsv_stats_device(v)
    for i in (0, 255, 511):
        s1, a1 = hsv_stats_device(v[i:i + 1])
        assert [getattr(stats[i], f) for f in ("Br", "Bg", "Bb", "Cr", "Cg", "Cb")] == \
            [getattr(s1[0], f) for f in ("Br", "Bg", "Bb", "Cr", "Cg", "Cb")]
        np.testing.assert_allclose(sat[i], a1[0], rtol=1e-14)
    img = synth.uniform(h, w, 511)
    np.testing.assert_allclose(sat[511], orc.palette(img)["average_saturation"], rtol=STATS_SAT_RTOL)
    del t, v


@pytest.mark.parametrize("kind,h,w", [("hblur", 3000, 4000), ("structured", 600, 800), ("motion", 401, 577)])
def test_blur_batch_matches_full_report(kind, h, w):
    """The FFT + blur-profile path alone (phd_blur_batch_device, config 4) gives
    the full report's bins and vectors: the compile-time path takes the DC sums
    from its own row pass, the runtime-plan path from the statistics pass, the
    full report from K1 -- the same integers.  Bins agree to the last bits the
    order of the column pass's fp64 atomics leaves free (1e-12)."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    from photohive_dsp_amd.core import blur_profiles_device, report_device
    imgs = np.stack([synth.make(kind, h, w, 70 + i) for i in range(2)])
    t = torch.from_numpy(imgs).cuda()
    bins, vecs = blur_profiles_device(t)
    reps = report_device(t)
    for i, r in enumerate(reps):
        np.testing.assert_allclose(bins[i], np.array(r.blur_profile.bins), rtol=1e-12, atol=1e-15)
        assert vecs[i] == [(v.angle, v.magnitude) for v in r.blur_vectors]


def test_mixed_size_host_batch():
    phd, L, _ = _phd()
    from photohive_dsp_amd import synth
    from oracle import oracle as orc
    imgs = [synth.make("structured", h, w, s) for (h, w, s) in [(512, 512, 1), (480, 640, 2), (720, 1280, 3)]]
    reps = phd.get_reports(imgs, h_partitions=36, s_partitions=4, v_partitions=5)
    for img, r in zip(imgs, reps):
        o = orc.report(img, h_partitions=36, s_partitions=4, v_partitions=5)
        np.testing.assert_array_equal(np.array(r.color_palette.group_ids), o.valid_parents)
        np.testing.assert_array_equal(np.array(r.color_palette.quantities), o.palette_pct)
        np.testing.assert_allclose(np.array(r.blur_profile.bins), o.bins, rtol=FLOAT_RTOL, atol=1e-12)


def test_mixed_size_device_batch_groups():
    """phd_report_batch_device_mixed (config 5): interleaved sizes, grouped into
    batches per size, each report equal to the single-image device report."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    from photohive_dsp_amd.core import report_device, reports_device_mixed
    shapes = [(512, 512), (480, 640), (512, 512), (720, 1280), (480, 640), (512, 512)]
    imgs = [synth.make(("structured", "uniform", "dominant")[i % 3], h, w, 40 + i) for i, (h, w) in enumerate(shapes)]
    ts = [torch.from_numpy(im).cuda() for im in imgs]
    kw = dict(h_partitions=36, s_partitions=4, v_partitions=5)
    reps = reports_device_mixed(ts, **kw)
    for t, r in zip(ts, reps):
        one = report_device(t[None].contiguous(), **kw)[0]
        assert r.color_palette.group_ids == one.color_palette.group_ids
        assert r.color_palette.quantities == one.color_palette.quantities
        np.testing.assert_allclose(np.array(r.blur_profile.bins), np.array(one.blur_profile.bins), rtol=1e-12,
                                   atol=1e-15)
        assert r.sharpnesses == one.sharpnesses
        assert r.blur_vectors == one.blur_vectors


@pytest.mark.parametrize("shape", [(720, 1280), (513, 700)])
def test_runtime_plan_batch_against_oracle(shape):
    """Runtime-plan sizes in a batch: the row and column passes of the batch are
    one launch each (grid.y = image); every image's report against the CPU
    oracle."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    from photohive_dsp_amd.core import report_device
    from oracle import oracle as orc
    h, w = shape
    imgs = np.stack([synth.make(("structured", "uniform", "dominant")[i % 3], h, w, 60 + i) for i in range(5)])
    reps = report_device(torch.from_numpy(imgs).cuda())
    for img, rep in zip(imgs, reps):
        o = orc.report(img)
        g = dict(stats=o.stats, average_saturation=np.array(o.average_saturation), valid_parents=o.valid_parents,
                 palette_pct=o.palette_pct, palette_hsv=o.palette_hsv, bins=o.bins, blur_angles=o.blur_angles,
                 blur_mags=o.blur_mags, angle_bin_size=np.array(o.angle_bin_size),
                 radius_bin_size=np.array(o.radius_bin_size))
        assert_report_matches(rep, g)


def test_host_batch_rejected_image_keeps_the_others():
    """phd_report_batch_u8 groups images by size: a rejected size (349x350,
    pre_compute_error_checks) fails alone, every other image of the batch is
    reported and matches its single-image report."""
    phd, L, _ = _phd()
    from photohive_dsp_amd import synth
    imgs = [synth.make("structured", 512, 512, 81), np.zeros((349, 350, 3), np.uint8),
            synth.make("uniform", 480, 640, 82), synth.make("dominant", 512, 512, 83)]
    reps = phd.get_reports(imgs)
    assert reps[1] is None
    for i in (0, 2, 3):
        one = phd.get_report(imgs[i])
        assert reps[i].color_palette.group_ids == one.color_palette.group_ids
        assert reps[i].color_palette.quantities == one.color_palette.quantities
        np.testing.assert_allclose(np.array(reps[i].blur_profile.bins), np.array(one.blur_profile.bins),
                                   rtol=1e-12, atol=1e-15)


def test_rejections_return_null():
    phd, L, _ = _phd()
    for h, w in [(349, 350), (2001, 400), (400, 2001)]:
        with pytest.raises(ValueError):
            phd.get_report(np.zeros((h, w, 3), np.uint8))


def test_device_synthetic_fill_matches_numpy():
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    n = 3 * 401 * 577
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert L.lib.phd_fill_uniform_device(t.data_ptr(), n, 7, None) == 0
    np.testing.assert_array_equal(t.cpu().numpy(), synth.uniform(401, 577, 7).ravel())


@pytest.mark.parametrize("kind,seed", [("uniform", 1), ("structured", 2), ("dominant", 3),
                                       # gradient + disks + 15-px horizontal box blur
                                       ("hblur", 2)])
def test_full_size_4000x3000_against_oracle(kind, seed):
    """BASELINE config 2 size: the whole report against the CPU oracle."""
    phd, L, _ = _phd()
    from photohive_dsp_amd import synth
    from oracle import oracle as orc
    img = synth.make(kind, 3000, 4000, seed)
    rep = phd.get_report(img)
    o = orc.report(img, fft_workers=8)
    hist, parents, kept = _trace(img)
    np.testing.assert_array_equal(hist, o.hist)
    np.testing.assert_array_equal(parents, o.valid_parents)
    np.testing.assert_array_equal(kept, o.kept)
    g = dict(stats=o.stats, average_saturation=np.array(o.average_saturation), valid_parents=o.valid_parents,
             palette_pct=o.palette_pct, palette_hsv=o.palette_hsv, bins=o.bins, blur_angles=o.blur_angles,
             blur_mags=o.blur_mags, angle_bin_size=np.array(o.angle_bin_size),
             radius_bin_size=np.array(o.radius_bin_size))
    assert_report_matches(rep, g)


@pytest.mark.parametrize("shape,kind", [((2000, 3000), "structured"), ((3000, 2000), "dominant"),
                                        ((4000, 6000), "structured"), ((6000, 4000), "uniform")])
def test_config5_large_sizes_against_oracle(shape, kind):
    """The large config-5 sizes (compile-time row plans 2000 / 3000 / 6000,
    column plans 2000 / 4000 / 6000) at h/s/v 36/4/5: the whole report
    against the CPU oracle."""
    phd, L, _ = _phd()
    from photohive_dsp_amd import synth
    from oracle import oracle as orc
    kw = dict(h_partitions=36, s_partitions=4, v_partitions=5)
    img = synth.make(kind, shape[0], shape[1], 11)
    rep = phd.get_report(img, **kw)
    o = orc.report(img, fft_workers=8, **kw)
    g = dict(stats=o.stats, average_saturation=np.array(o.average_saturation), valid_parents=o.valid_parents,
             palette_pct=o.palette_pct, palette_hsv=o.palette_hsv, bins=o.bins, blur_angles=o.blur_angles,
             blur_mags=o.blur_mags, angle_bin_size=np.array(o.angle_bin_size),
             radius_bin_size=np.array(o.radius_bin_size))
    assert_report_matches(rep, g)


@pytest.mark.parametrize("cfg", [{}, {"h_partitions": 36, "s_partitions": 4, "v_partitions": 5},
                                 {"black_thresh": 0.25, "gray_thresh": 0.2, "h_partitions": 12}],
                         ids=["default", "36_4_5", "thresholds"])
def test_hsv_group_exhaustive_rgb_cube(cfg):
    """Device rgb2hsv + arm_octree group id == the C oracle for all 2^24 RGB8 triples."""
    check_hsv_groups_rgb_cube(cfg)


def check_hsv_groups_rgb_cube(cfg):
    """(also run by tests/test_gpu_palette_grids.py on the grids past s_partitions = 6)"""
    phd, L, torch = _phd()
    from oracle import oracle as orc
    from photohive_dsp_amd.core import make_config
    k = np.arange(1 << 24, dtype=np.uint32)
    cube = np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], axis=1).astype(np.uint8)
    want, want_hsv = orc.group_ids(cube, with_hsv=True, **cfg)
    d_rgb = torch.from_numpy(cube).cuda()
    d_gid = torch.empty(1 << 24, dtype=torch.int32, device="cuda")
    d_hsv = torch.empty((1 << 24, 3), dtype=torch.float64, device="cuda")
    c = make_config(**cfg)
    assert L.lib.phd_debug_hsv_groups_device(d_rgb.data_ptr(), 1 << 24, ctypes.byref(c), d_gid.data_ptr(),
                                             d_hsv.data_ptr()) == 0
    got_hsv = d_hsv.cpu().numpy()
    bad = np.nonzero(np.any(got_hsv != want_hsv, axis=1))[0]
    assert bad.size == 0, f"{bad.size} hsv mismatches, e.g. rgb={cube[bad[:5]].tolist()} " \
                          f"gpu={got_hsv[bad[:3]].tolist()} cpu={want_hsv[bad[:3]].tolist()}"
    np.testing.assert_array_equal(d_gid.cpu().numpy(), want)


@pytest.mark.parametrize("cfg", [{"coverage_thresh": 1.0}, {},
                                 {"h_partitions": 36, "s_partitions": 4, "v_partitions": 5, "coverage_thresh": 1.0},
                                 {"h_partitions": 15, "s_partitions": 3, "v_partitions": 2}])
def test_table_k1_exhaustive_rgb_cube_palette(cfg):
    """The production K1 (k1.hip: table classification, packed counts, one-pass
    palette sums) over every RGB8 triple once: a 4096 x 4096 image holding the
    whole 256^3 cube, full report against the oracle.  With coverage 1.0 every
    non-empty group is a palette slot kept whole, so each group's count and
    h / s / v sums over all its colours are compared directly."""
    phd, L, _ = _phd()
    from oracle import oracle as orc
    k = np.arange(1 << 24, dtype=np.uint32)
    cube = np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], axis=1).astype(np.uint8).reshape(4096, 4096, 3)
    rep = phd.get_report(cube, **cfg)
    o = orc.palette(cube, **cfg)
    cp = rep.color_palette
    np.testing.assert_array_equal(np.array(cp.group_ids), o["valid_parents"])
    np.testing.assert_array_equal(np.array(cp.quantities), o["palette_pct"])
    np.testing.assert_allclose(np.array(cp.hsv).reshape(-1, 3), o["palette_hsv"], rtol=TIGHT_RTOL, atol=1e-12)
    np.testing.assert_allclose(rep.average_saturation, o["average_saturation"], rtol=TIGHT_RTOL)


FUSED_CFGS = [{}, {"h_partitions": 9}, {"h_partitions": 15, "s_partitions": 3, "v_partitions": 2},
              {"h_partitions": 5, "linked_list_size": 50}, {"h_partitions": 1, "s_partitions": 3},
              {"h_partitions": 72, "s_partitions": 2, "v_partitions": 2, "linked_list_size": 64},
              {"h_partitions": 36, "s_partitions": 4, "v_partitions": 5}, {"h_partitions": 360}]


@pytest.mark.parametrize("kind", ["posterized", "uniform", "structured", "grayish"])
@pytest.mark.parametrize("cfg", FUSED_CFGS, ids=lambda c: "_".join(f"{k[0]}{v}" for k, v in c.items()) or "default")
def test_fused_palette_sums_against_oracle(cfg, kind):
    """The one-pass palette (per-group sums + hue-cell wrap counts in K1, partial
    groups on the device) against the oracle's per-pixel calculate_avg_hsv:
    odd and even hue partitions put the wrap thresholds on bin centres or bin
    edges; posterized images put many exact hues on them; small linked lists
    make tie-overflow (partial) groups."""
    phd, L, _ = _phd()
    from photohive_dsp_amd import synth
    from oracle import oracle as orc
    img = synth.make(kind, 600, 800, 11)
    rep = phd.get_report(img, **cfg)
    o = orc.palette(img, **cfg)
    cp = rep.color_palette
    np.testing.assert_array_equal(np.array(cp.group_ids), o["valid_parents"])
    np.testing.assert_array_equal(np.array(cp.quantities), o["palette_pct"])
    np.testing.assert_allclose(np.array(cp.hsv).reshape(-1, 3), o["palette_hsv"], rtol=TIGHT_RTOL, atol=1e-12)


@pytest.mark.parametrize("kind,seed,H,W", [("uniform", 5, 3000, 4000), ("structured", 6, 3000, 4000),
                                            # config 5's sub-3-MP sizes (compile-time plans, round 3)
                                            ("structured", 7, 1080, 1920),
                                            ("structured", 9, 1536, 2048), ("uniform", 10, 720, 1280),
                                            ("structured", 11, 1280, 720), ("uniform", 12, 640, 480),
                                            ("structured", 13, 480, 640), ("structured", 14, 512, 512)])
def test_power_spectrum_compile_time_fft(kind, seed, H, W):
    """The production FFT kernels' |X|^2 against numpy's rfft2 (pocketfft, fp64)
    of the reference's luma - DC bias (src/image_processing.c:505-512,
    src/blur_profile.c:233-238, src/fft_processing.c:34-50)."""
    phd, L, torch = _phd()
    from photohive_dsp_amd import synth
    img = synth.make(kind, H, W, seed)
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    wf = W // 2 + 1
    out = torch.empty(wf * H, dtype=torch.float64, device="cuda")
    rc = L.lib.phd_debug_power_spectrum(t.data_ptr(), H, W, out.data_ptr())
    if rc == -2:
        pytest.skip("no compile-time FFT plan for this size")
    assert rc == 0, L.last_error()
    got = out.cpu().numpy().reshape(wf, H).T
    k255 = np.arange(256, dtype=np.float64) / 255.0
    f = img.astype(np.int64)
    pgm = 0.299 * k255[f[..., 0]] + 0.587 * k255[f[..., 1]] + 0.114 * k255[f[..., 2]]
    n = float(H * W)
    avg = (f[..., 0].sum() / 255.0 / n + f[..., 1].sum() / 255.0 / n + f[..., 2].sum() / 255.0 / n) / 3.0
    X = np.fft.rfft2(pgm - avg)
    want = X.real * X.real + X.imag * X.imag
    scale = want.max()
    err = np.abs(got - want)
    assert err.max() <= 1e-11 * scale, f"max abs err {err.max() / scale:.3e} of max"
    big = want > 1e-6 * scale
    assert np.max(err[big] / want[big]) < 1e-8
