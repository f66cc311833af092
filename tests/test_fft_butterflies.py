"""fft_engine.h's butterflies on the host (no GPU): tests/native/
fft_butterflies.cpp, built from the header's host half with ASan + UBSan and
run as its own process -- dft<R> for R in 6 10 12 15 20 30 (the prime-factor
form) and 8 9 16 25 against a direct fp64 DFT, the prime-factor index maps as
permutations, and a two-lane emulation of the split radix-20 last pass; all to
1e-14 of the largest output."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


def test_butterflies_against_direct_dft(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    exe = tmp_path / "fft_butterflies"
    src = os.path.join(ROOT, "tests", "native", "fft_butterflies.cpp")
    # the header's host half only: no device pass, no code object
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-std=c++17", "-O1", "-g",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", str(exe)], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "fft butterflies OK" in r.stdout and "FAIL" not in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
