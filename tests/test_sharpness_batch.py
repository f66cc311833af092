"""Batched sharpness, CPU side: the host twin of the batched kernel
(phd_debug_sharpness_host: the kernel's tile plan and merge order,
sharp_tiles.h) against the oracle, the Python normalisation of per-image crop
boxes, and the twin under ASan + UBSan as a stand-alone program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.sharp_boxes import KINDS, TIGHT_RTOL, assert_sharp, box, three, twelve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_twin(img, boxes):
    from photohive_dsp_amd import set_bounding_boxes
    from photohive_dsp_amd.lib import lib
    img = np.ascontiguousarray(img, dtype=np.uint8)
    cb = set_bounding_boxes(boxes)
    out = (ctypes.c_double * max(1, len(boxes)))()
    rc = lib.phd_debug_sharpness_host(img.ctypes.data, img.shape[0], img.shape[1], ctypes.byref(cb), out)
    return rc, [out[k] for k in range(len(boxes))]


@pytest.mark.parametrize("h,w", [(480, 640), (401, 577)])
def test_host_twin_matches_oracle(h, w):
    from photohive_dsp_amd import synth
    from oracle import oracle as orc
    for seed in (1, 2):
        for kind in KINDS:
            img = synth.make(kind, h, w, seed)
            boxes = twelve(h, w) + three(h, w)
            rc, got = host_twin(img, boxes)
            assert rc == 0
            want = orc.sharpness(img, boxes)
            assert_sharp(got, want)
            assert got[6] == got[7]                      # the duplicate box: the same bits


def test_host_twin_rejects_bad_boxes():
    from photohive_dsp_amd import synth
    img = synth.make("uniform", 400, 400, 3)
    for bad in (box(0, 401, 0, 10), box(0, 10, 0, 401), box(5, 5, 0, 10), box(0, 10, 9, 3), box(-1, 4, 0, 4)):
        rc, _ = host_twin(img, [box(0, 4, 0, 4), bad])
        assert rc == -1, bad
    assert host_twin(img, [])[0] == 0


def test_normalize_salient():
    from photohive_dsp_amd import set_bounding_boxes
    from photohive_dsp_amd.core import normalize_salient
    from photohive_dsp_amd.structures import Crop_Boundaries
    assert normalize_salient(None, 4) is None
    cb = set_bounding_boxes([box(1, 2, 3, 4)])
    arr, keep = normalize_salient([[box(0, 10, 5, 9), box(2, 3, 4, 6)], None, cb, []], 4)
    assert len(arr) == 4
    a0 = arr[0].contents
    assert a0.N == 2
    assert [a0.top[1], a0.bottom[1], a0.left[1], a0.right[1]] == [2, 3, 4, 6]
    assert [a0.top[0], a0.bottom[0], a0.left[0], a0.right[0]] == [0, 10, 5, 9]
    assert not arr[1]                                    # None: a NULL pointer
    assert ctypes.addressof(arr[2].contents) == ctypes.addressof(cb)   # passed through, not copied
    assert arr[3] and arr[3].contents.N == 0             # []: a Crop_Boundaries with N == 0
    assert all(isinstance(k, Crop_Boundaries) for k in keep) and len(keep) == 3
    with pytest.raises(ValueError):
        normalize_salient([None, None], 3)
    with pytest.raises(ValueError):
        normalize_salient([], 1)


def test_length_mismatch_raises_before_any_library_call():
    """get_reports checks salient_characters against the images first (no GPU
    here: a library call would fail differently)."""
    import photohive_dsp_amd as phd
    from photohive_dsp_amd import synth
    imgs = [synth.make("uniform", 400, 400, 1)] * 2
    with pytest.raises(ValueError, match="salient_characters"):
        phd.get_reports(imgs, salient_characters=[None])


def test_host_twin_under_asan(tmp_path):
    """phd_sharp_host.cpp and a C++ driver built with ASan + UBSan, run as
    their own process: edge boxes (single pixels, boxes flush with the last
    row and column of an exactly-sized buffer, one more than a tile)."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "sharp_asan"
    src = [os.path.join(ROOT, "tests", "native", "sharpness_host_asan.cpp"),
           os.path.join(ROOT, "photohive_dsp_amd", "csrc", "phd_sharp_host.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + src,
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "sharpness host OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
