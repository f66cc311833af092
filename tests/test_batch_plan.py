"""The batch entries' grouping (CPU): batch_plan.h -- size_groups and
lane_split -- through a C++ program of its own built with ASan + UBSan
(tests/native/batch_plan.cpp)."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


def test_batch_plan_under_asan_ubsan(tmp_path):
    """The 35 + 3 + 35 images of test_mixed_batch_groups_past_64_images make a
    70-image and a 3-image group; a full group opens a second one; cap wins
    over a small pixel budget; kMixedGroupMax holds for 1,100 small images;
    lane_split gives 262 of 512, 8 of 16 and two non-empty parts for 16..1024."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "batch_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "batch_plan.cpp")], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "batch plan OK" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
