"""blur_window.h on the host (no GPU): tests/native/blur_window_fft.cpp, built
from the header's host half with ASan + UBSan and run as its own process -- for
T = 64 and 128 the window plan's passes, the row pairs' separation and the
packed DC + i Nyquist column through the shared index maps against a direct
2-D DFT in long double (random, constant, one pixel, 1-px stripes both ways, a
checkerboard), to 1e-13 of the largest output; the index maps as permutations;
the box rule."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


def test_window_transform_against_direct_dft(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    exe = tmp_path / "blur_window_fft"
    src = os.path.join(ROOT, "tests", "native", "blur_window_fft.cpp")
    # the header's host half only: no device pass, no code object
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", str(exe)], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "blur window fft OK" in r.stdout and "FAIL" not in r.stdout
    assert r.stdout.count("err ") == 12, r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
