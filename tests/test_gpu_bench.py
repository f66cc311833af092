"""bench.py's plain run on the GPU: `--steps` timed steps of the headline and
nothing else in the line, and `--dump-outputs` writes the reports of the last
timed step -- the same values report_device gives for the same seeded images
in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_parity import _phd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, B = 600, 800, 5


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("bench") / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", str(B), "--height", str(H), "--width", str(W), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {p[:-4]: np.load(out / p) for p in os.listdir(out)}


def test_plain_line_holds_the_headline_alone(plain_run):
    d, _ = plain_run
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0
    # value and ms_per_step are the same timed region, B images per step (ms_per_step is
    # rounded to 1e-3 ms, a step of this small batch takes a few tenths of a ms at the least)
    assert d["value"] == pytest.approx(1000.0 * B / d["ms_per_step"], rel=1e-2)
    moved = {"cpu_baseline", "vs_cpu_baseline", "one_lane", "per_kernel", "warmup_kernels_us_per_launch",
             "config1", "config2_single", "config2_structured", "config3", "config4", "config5", "host_buffer",
             "legacy_entry"}
    assert not moved & set(d), sorted(moved & set(d))


def test_dumped_outputs_are_the_reports_of_the_same_images(plain_run):
    """Image i of the batch is uniform noise of seed i (rank 0).  Integer-sum
    fields are exact; S-bar and the palette's h / s / v are fp64 sums whose
    atomics land in any order (1e-12, as tests/test_gpu_round5.py)."""
    d, got = plain_run
    phd, L, torch = _phd()
    from photohive_dsp_amd.core import report_device
    assert set(got) == set(d["dumped_outputs"]["arrays"]) and all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    t = torch.empty((B, H, W, 3), dtype=torch.uint8, device="cuda")
    for i in range(B):
        assert L.lib.phd_fill_uniform_device(t[i].data_ptr(), t[i].numel(), i, None) == 0, L.last_error()
    torch.cuda.synchronize()
    reps = report_device(t)
    assert got["blur_bins"].shape == (B, 72, 40) and got["palette_n"].shape == (B,)
    for i, rep in enumerate(reps):
        st, cp = rep.rgb_stats, rep.color_palette
        assert got["rgb_stats"][i].tolist() == [st.Br, st.Bg, st.Bb, st.Cr, st.Cg, st.Cb]
        np.testing.assert_allclose(got["average_saturation"][i], rep.average_saturation, rtol=1e-12)
        n = int(got["palette_n"][i])
        assert n == cp.N > 0
        assert got["palette_group_ids"][i, :n].tolist() == cp.group_ids
        assert (got["palette_group_ids"][i, n:] == -1).all()
        assert got["palette_percentages"][i, :n].tolist() == cp.quantities
        np.testing.assert_allclose(got["palette_hsv"][i, :n], np.array(cp.hsv), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(got["blur_bins"][i], np.array(rep.blur_profile.bins), rtol=1e-12)
        assert int(got["blur_vectors_n"][i]) == len(rep.blur_vectors)
        assert got["blur_vectors"][i, :len(rep.blur_vectors)].tolist() == \
            [[v.angle, v.magnitude] for v in rep.blur_vectors]
    # the images differ, so do their reports
    assert not np.array_equal(got["blur_bins"][0], got["blur_bins"][1])
