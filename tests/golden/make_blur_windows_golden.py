"""Window blur fixtures from the reference's own C (oracle/_ref):
tests/golden/blur_windows_<case>.npz and blur_windows_manifest.json.

    python -m tests.golden.make_blur_windows_golden

Per case an image from photohive_dsp_amd.synth by seed (or the special-pattern
image of tests/blur_windows_cases.py), a window size, a polar grid and a window
list; per window the reference's get_blur_profile on the crop in
oracle/ref_pipeline.py's manner -- numpy slicing is crop_image's copy
(src/image_processing.c:244-266); get_rgb_statistics, rgb2pgm and remove_dc_bias
(:543-553, :505-512, src/blur_profile.c:233-238) are the reference's own;
numpy.fft.rfft2 and normalize_power stand in for FFTW and pgm_normalize_fft
(src/fft_processing.c:18-63, 173-213); cartesian_to_polar_conversion,
calculate_blur_profile and vectorize_blur_profile (src/blur_profile.c:427-458,
34-126, 324-416) are the reference's own.  A file holds windows, bins, angles,
mags, fft_max and the two bin sizes; the images are rebuilt from the manifest.

Asserted before anything is written: the C restatement (oracle.stats / pgm_dc /
power_spectrum / blur_profile / vectorize) agrees with the reference within the
tests' own bars; every window's vectors are unchanged when its bins are
perturbed by +-1e-10 relative (8 draws); at least a third of the windows have a
non-zero magnitude."""
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
from tests import blur_windows_cases as bwc  # noqa: E402

MAX_BYTES = 64 * 1024


def reference_window(img, box, nr, na, kw=bwc.BLUR_KW):
    """bins [na, nr], angles [10], mags [10], fft_max, bin sizes of the reference on the crop."""
    L = rp.lib()
    t, b, l, r = box
    crop = np.ascontiguousarray(img[t:b, l:r])
    T = crop.shape[0]
    im, _keep = rp._image_rgb(crop)
    pim = C.pointer(im)
    pgm = L.rgb2pgm(pim)
    stp = L.get_rgb_statistics(pim)
    st = stp.contents
    avg = (st.Br + st.Bg + st.Bb) / 3.0                          # src/interface.c:78
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(stp, C.c_void_p))
    L.remove_dc_bias(pgm, avg)
    data = np.ctypeslib.as_array(pgm.contents.data, shape=(T * T,)).reshape(T, T)
    X = np.fft.rfft2(data)
    power = X.real * X.real + X.imag * X.imag
    norm, fmax = rp.normalize_power(power)
    wf = T // 2 + 1
    fft_img = L.create_pgm_image(wf, T)
    np.ctypeslib.as_array(fft_img.contents.data, shape=(T * wf,))[:] = norm.ravel()
    conv = L.cartesian_to_polar_conversion(wf, T)
    bp = L.calculate_blur_profile(conv, fft_img, nr, na)
    bins = np.array([[bp.contents.bins[a][q] for q in range(nr)] for a in range(na)])
    bv = L.vectorize_blur_profile(bp, kw["fft_streak_thresh"], kw["magnitude_thresh"], kw["blur_cutoff_ratio_denom"])
    ang = np.array([bv.contents.blur_vectors[i].angle for i in range(10)], np.int32)
    mag = np.array([bv.contents.blur_vectors[i].magnitude for i in range(10)], np.float32)
    sizes = (bp.contents.angle_bin_size, bp.contents.radius_bin_size)
    L.free_blur_vector_group(bv)
    L.free_blur_profile(bp)
    L.free_cartesian_to_polar(conv)
    L.free_image_pgm(fft_img)
    L.free_image_pgm(pgm)
    return bins, ang, mag, fmax, sizes


def stable(bins, ang, mag, seed):
    rng = np.random.default_rng(seed)
    for _ in range(8):
        a, m = bwc.vectorize(bins * (1.0 + 1e-10 * rng.choice([-1.0, 1.0], size=bins.shape)))
        if not (np.array_equal(a, ang) and np.array_equal(m, mag)):
            return False
    return True


def main():
    cases, total, moving = [], 0, 0
    for name, kind, h, w, seed, T, nr, na, windows in bwc.CASES:
        case = dict(name=name, kind=kind, height=h, width=w, seed=seed, window=T, radius_partitions=nr,
                    angle_partitions=na, windows=len(windows))
        img = bwc.case_image(case)
        ref = [reference_window(img, b, nr, na) for b in windows]
        sizes = ref[0][4]
        want = (np.array([r[0] for r in ref]), np.array([r[1] for r in ref], np.int32),
                np.array([r[2] for r in ref], np.float32), np.array([r[3] for r in ref]))
        bwc.assert_windows(bwc.oracle_windows(img, windows, nr, na), want, name)
        for k, b in enumerate(windows):
            o = bwc.oracle_window(img, b, nr, na)
            assert (o[4], o[5]) == sizes == ref[k][4], (name, k)
            assert stable(want[0][k], want[1][k], want[2][k], 1000 * seed + k), f"{name} window {k}: unstable vectors"
        nz = int(np.count_nonzero(want[2].max(axis=1) > 0))
        total += len(windows)
        moving += nz
        path = os.path.join(HERE, f"blur_windows_{name}.npz")
        np.savez_compressed(path, windows=np.array(windows, dtype=np.int32), bins=want[0], angles=want[1],
                            mags=want[2], fft_max=want[3], angle_bin_size=np.int32(sizes[0]),
                            radius_bin_size=np.int32(sizes[1]))
        size = os.path.getsize(path)
        assert size < MAX_BYTES, f"{path}: {size} bytes"
        print(f"{name}: {len(windows)} windows, {nz} with a non-zero magnitude, {size} bytes", flush=True)
        cases.append(case)
    assert 3 * moving >= total, f"{moving} of {total} windows have a non-zero magnitude"
    with open(os.path.join(HERE, "blur_windows_manifest.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=1)
        f.write("\n")
    print(f"{moving} of {total} windows have a non-zero magnitude")


if __name__ == "__main__":
    main()
