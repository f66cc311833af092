"""grow_buf.h on the host (no GPU): tests/native/grow_buf_asan.cpp, built with
ASan + UBSan (leak check on, ASan's default) and run as its own process --
GrowBuf and the staged pair's reserve over a malloc-backed memory kind that
counts and orders its alloc, free and idle calls and can fail an allocation:
kept blocks, the growth rule and its idle-free-alloc order, failures, release
twice and release-then-ensure, ensure(0), nothing alive at the end."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    return shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc") or None


def test_grow_buf_under_sanitizers(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    exe = tmp_path / "grow_buf_asan"
    src = os.path.join(ROOT, "tests", "native", "grow_buf_asan.cpp")
    # plain C++ (the header is host only and includes no HIP): hipcc as the compiler driver
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", str(exe)],
                   check=True, timeout=600)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "LSAN_OPTIONS")}   # ASan's defaults
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "grow_buf OK" in r.stdout and "FAIL" not in r.stdout, r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "ERROR: LeakSanitizer" not in r.stderr
    assert "runtime error" not in r.stderr
