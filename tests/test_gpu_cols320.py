"""The 3000-row column pass with the prime-factor butterflies every compile-time
plan inherits, at its smallest sizes and both prefetch forms.  The 320-thread
plan (radices 15, 10 and a radix-20 last pass split over lane pairs; measured
slower and kept as a build variant) is covered by this
file when the library is built with it, and in every build by
test_split_pass_plan_against_numpy_fft, which runs its passes on the device
through a hook of their own.

The smallest images that reach k_cols_ct<3000, ...> through the library are
3000 rows of 640 and 720 columns: the narrowest widths with a compile-time row
plan that the reference's aspect-ratio check (at most 5 : 1, src/utilities.c,
precheck in phd_report.cpp) lets through -- 3000 x 480 and 3000 x 512 are
rejected before any kernel runs.  wf = 321 and 361, both odd, so the phantom
column of the last column pair runs, and 81 / 91 tile pairs against a grid of
128 logical blocks (512 resident blocks / 4), so blocks without units run too
(asserted below against the size of the grid).  Both prefetch
forms (phd_debug_column_form), one image and a batch of three in one launch (a
block's range of units then spans two images)."""
import functools

import numpy as np
import pytest

from tests.test_gpu_parity import BINS_NORMWISE, BINS_TIGHT_RTOL, _phd, assert_report_matches

pytestmark = pytest.mark.gpu

SIZES_3000 = [(3000, 640), (3000, 720)]
# one case each at 2000 and 480 rows: plans that only inherit the butterflies
SIZES_OTHER = [(2000, 480), (480, 512)]


@functools.lru_cache(maxsize=None)
def _image(h, w, seed=0):
    from photohive_dsp_amd import synth
    img = synth.make("structured", h, w, 40 + seed)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _rfft2_power(h, w):
    """|rfft2(luma - DC bias)|^2 as test_power_spectrum_compile_time_fft forms it."""
    img = _image(h, w)
    k255 = np.arange(256, dtype=np.float64) / 255.0
    f = img.astype(np.int64)
    pgm = 0.299 * k255[f[..., 0]] + 0.587 * k255[f[..., 1]] + 0.114 * k255[f[..., 2]]
    n = float(h * w)
    avg = (f[..., 0].sum() / 255.0 / n + f[..., 1].sum() / 255.0 / n + f[..., 2].sum() / 255.0 / n) / 3.0
    X = np.fft.rfft2(pgm - avg)
    want = X.real * X.real + X.imag * X.imag
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _oracle(h, w):
    from oracle import oracle as orc
    o = orc.report(_image(h, w), fft_workers=8)
    return dict(stats=o.stats, average_saturation=np.array(o.average_saturation), valid_parents=o.valid_parents,
                palette_pct=o.palette_pct, palette_hsv=o.palette_hsv, bins=o.bins, blur_angles=o.blur_angles,
                blur_mags=o.blur_mags, angle_bin_size=np.array(o.angle_bin_size),
                radius_bin_size=np.array(o.radius_bin_size))


class _form:
    """phd_debug_column_form(form) for the block, the previous setting after it."""

    def __init__(self, L, form):
        self.L, self.form = L, form

    def __enter__(self):
        self.prev = self.L.lib.phd_debug_column_form(self.form)

    def __exit__(self, *exc):
        self.L.lib.phd_debug_column_form(self.prev)


def _check_power(h, w, form):
    phd, L, torch = _phd()
    img = _image(h, w)
    t = torch.from_numpy(np.array(img)).cuda()
    wf = w // 2 + 1
    out = torch.empty(wf * h, dtype=torch.float64, device="cuda")
    with _form(L, form):
        rc = L.lib.phd_debug_power_spectrum(t.data_ptr(), h, w, out.data_ptr())
    assert rc == 0, L.last_error()                 # (-2, no compile-time plan, is a failure here)
    got = out.cpu().numpy().reshape(wf, h).T
    want = _rfft2_power(h, w)
    scale = want.max()
    err = np.abs(got - want)
    big = want > 1e-6 * scale
    print(f"{h}x{w} form {form}: max abs err {err.max() / scale:.3e} of max, "
          f"max rel err of the large terms {np.max(err[big] / want[big]):.3e}")
    # the bars of test_power_spectrum_compile_time_fft
    assert err.max() <= 1e-11 * scale, f"max abs err {err.max() / scale:.3e} of max"
    assert np.max(err[big] / want[big]) < 1e-8


@pytest.mark.parametrize("form", [0, 1], ids=["half", "full"])
@pytest.mark.parametrize("h,w", SIZES_3000)
def test_power_spectrum_3000_rows(h, w, form):
    """|X|^2 of the 3000-row column plan (debug hook) against numpy's rfft2, both
    prefetch forms, odd wf (phantom column) and more blocks than tile pairs."""
    _check_power(h, w, form)


@pytest.mark.parametrize("h,w", SIZES_OTHER)
def test_power_spectrum_inherited_butterflies(h, w):
    """2000 rows (10 10 20) and 480 rows (5 6 16): unchanged plans whose radix
    6, 10 and 20 butterflies are now the prime-factor form."""
    _check_power(h, w, -1)


@pytest.mark.parametrize("form", [0, 1], ids=["half", "full"])
@pytest.mark.parametrize("h,w", SIZES_3000)
def test_report_bins_against_oracle(h, w, form):
    """The whole report against the CPU oracle; the bins at the bars of
    tests/test_gpu_parity.py (1e-11 normwise, 1e-10 element-wise)."""
    phd, L, _ = _phd()
    g = _oracle(h, w)
    with _form(L, form):
        rep = phd.get_report(_image(h, w))
    assert_report_matches(rep, g)
    bins = np.array(rep.blur_profile.bins)
    normwise = np.max(np.abs(bins - g["bins"])) / max(np.max(np.abs(g["bins"])), 1e-300)
    print(f"{h}x{w} form {form}: bins normwise {normwise:.3e}")
    assert normwise <= BINS_NORMWISE, normwise
    np.testing.assert_allclose(bins, g["bins"], rtol=BINS_TIGHT_RTOL, atol=1e-13)


@pytest.mark.parametrize("h,w", SIZES_3000)
def test_sizes_exercise_phantom_column_and_idle_blocks(h, w):
    """The properties the sizes above were chosen for: an odd wf, fewer tile
    pairs than logical blocks (a quarter of the column kernel's grid, the
    number of its max partials), and the compile-time plans (the power
    spectrum hook returns -2 without them; checked in the tests above)."""
    phd, L, torch = _phd()
    wf = w // 2 + 1
    assert wf % 2 == 1
    tile_pairs = ((wf + 1) // 2 + 1) // 2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert tile_pairs < 2 * cus // 32 * 32 // 4, (tile_pairs, cus)


def test_split_pass_plan_against_numpy_fft():
    """fe::SplitPass on the device in every build (phd_debug_fft_split_pass): five
    3000-point transforms, one block each, through the 320-thread plan 15, 10,
    split 20 -- SplitPass's loads, twiddles and DPP exchange and the indexing
    of its outputs (active, row0, OUT, NB) as k_cols_ct's epilogue uses them --
    against numpy's fft.  Inputs: random, one impulse per residue class that
    the last pass separates (input 1, and input 150 + 1) and a pure tone, so a
    permuted output row cannot hide.

    Bound: 1e-13 of the largest output of each transform.  An fp64
    Cooley-Tukey transform's error is at most about c eps log2(N) ||X||_2 with
    c a small constant (three passes, twiddles from chains of at most five
    products); here eps = 1.1e-16, log2 N = 11.6 and, for the random input,
    ||X||_2 = sqrt(3000) rms ~ 20 max|X|, which gives 2.6e-14 c: c = 4."""
    phd, L, torch = _phd()
    rng = np.random.default_rng(7)
    n, N = 5, 3000
    x = np.zeros((n, N), dtype=np.complex128)
    x[0] = rng.uniform(-1, 1, N) + 1j * rng.uniform(-1, 1, N)
    x[1] = rng.uniform(-1, 1, N) + 1j * rng.uniform(-1, 1, N)
    x[2, 1] = 1.0
    x[3, 151] = 1.0 - 0.5j
    x[4] = np.exp(2j * np.pi * 1637 * np.arange(N) / N)          # X = N at row 1637 (an odd lane's output)
    dx = torch.from_numpy(x.view(np.float64).reshape(n, 2 * N)).cuda()
    dX = torch.full((n, 2 * N), float("nan"), dtype=torch.float64, device="cuda")
    assert L.lib.phd_debug_fft_split_pass(dx.data_ptr(), dX.data_ptr(), n) == 0, L.last_error()
    got = dX.cpu().numpy().view(np.complex128).reshape(n, N)
    want = np.fft.fft(x, axis=1)
    for i in range(n):
        scale = np.abs(want[i]).max()
        err = np.abs(got[i] - want[i]).max()               # (NaN, a row never written, fails the comparison)
        print(f"split-pass plan, transform {i}: max err {err / scale:.3e} of max")
        assert err <= 1e-13 * scale, (i, err / scale, int(np.nanargmax(np.abs(got[i] - want[i]))))


def _blur(rep):
    return (np.array(rep.blur_profile.bins), [(v.angle, v.magnitude) for v in rep.blur_vectors])


@pytest.mark.parametrize("form", [0, 1], ids=["half", "full"])
@pytest.mark.parametrize("h,w", SIZES_3000)
def test_batch_of_three_bit_identical_to_single_calls(h, w, form):
    """Three images in one call take the batched column launch, where a block's
    range of units runs from one image into the next: bins and blur vectors
    bit-identical to three one-image calls (fixed-point bin sums, whatever the
    order) and over a repeat."""
    phd, L, torch = _phd()
    t = torch.from_numpy(np.stack([_image(h, w, i) for i in range(3)])).cuda()
    with _form(L, form):
        batch = [_blur(r) for r in phd.report_device(t)]
        again = [_blur(r) for r in phd.report_device(t)]
        single = [_blur(phd.report_device(t[i:i + 1])[0]) for i in range(3)]
    for i in range(3):
        assert np.array_equal(batch[i][0], single[i][0]), f"image {i}: batch bins differ from the single call's"
        assert batch[i][1] == single[i][1]
        assert np.array_equal(batch[i][0], again[i][0]), f"image {i}: bins differ over a repeat"
        assert batch[i][1] == again[i][1]
    # (the three images differ, so a block that read the wrong image would show)
    assert not np.array_equal(batch[0][0], batch[1][0])
