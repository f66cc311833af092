"""bench.py's multi-rank path on the CPU: `python bench.py --gpus 2` with no
torchrun environment starts the ranks itself (a torch.distributed.run child),
every rank takes its shard of configs 2, 4 and 5 and one gloo all_reduce
(shard.merge_counters) merges the counters; rank 0 prints one JSON line with
both ranks' images."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus2_spawns_ranks_and_merges_counters():
    env = dict(os.environ, PHD_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--plan-only",
                        "--batch", "8", "--config4-images", "64", "--config5-images", "96"],
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks"] == 2
    assert d["config2"]["images"] == 2 * 8                      # weak: batch 8 per rank
    assert d["config4"]["images"] == 64 and d["config5"]["images"] == 96   # strong: totals split
    from photohive_dsp_amd import shard
    sizes = shard.mixed_sizes(96, 5)
    assert d["config5"]["pixels"] == sum(h * w for h, w in sizes)
    assert d["config2"]["elapsed_max"] == 2.0                   # max over ranks (1 + rank)


def test_every_roofline_prices_algorithmic_bytes():
    """Every roofline object bench.py builds takes its bytes from
    algorithmic_bytes, never from a literal byte formula."""
    import ast
    import re
    src = open(os.path.join(ROOT, "bench.py")).read()
    tree = ast.parse(src)
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "ab" for t in node.targets):
            seg = ast.get_source_segment(src, node.value)
            assert "algorithmic_bytes(" in seg, f"bench.py:{node.lineno}: ab = {seg}"
    # no per-element byte constants left in the byte counts (the removed 18 H Wf bin map)
    assert not re.search(r"\b18(\.0)? \* h", src)
    sys.path.insert(0, ROOT)
    import bench
    h, w = 3000, 4000
    assert bench.algorithmic_bytes("fft_cols", h, w) == 16 * h * (w // 2 + 1)
    assert bench.algorithmic_bytes("blur_path", h, w) == 3 * h * w + 32 * h * (w // 2 + 1)
    assert bench.algorithmic_bytes("report", h, w) == 9 * h * w + 32 * h * (w // 2 + 1)


def test_plain_run_is_the_default_and_dump_writes_every_report_field(tmp_path):
    """A plain run (no --full) takes none of the extra legs; dump_reports
    (--dump-outputs) writes every field of each Full_Report_Data as float64,
    image index first, padded past an image's own palette."""
    import ctypes
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from photohive_dsp_amd.core import make_config
    from photohive_dsp_amd.structures import Full_Report_Data
    from tests.test_report_host import _report_struct
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    assert bench.parse(["--full", "--dump-outputs", "x"]).full is True
    made = [_report_struct(7, 3), _report_struct(120, 0)]
    outs = (ctypes.POINTER(Full_Report_Data) * 2)(*[ctypes.pointer(m[0]) for m in made])
    shapes = bench.dump_reports(outs, 2, make_config(angle_partitions=8, radius_partitions=5), str(tmp_path))
    got = {p[:-4]: np.load(tmp_path / p) for p in os.listdir(tmp_path)}
    assert set(got) == set(shapes) and all(v.dtype == np.float64 for v in got.values())
    assert got["palette_n"].tolist() == [7, 120] and got["palette_hsv"].shape == (2, 120, 3)
    assert got["palette_group_ids"][0].tolist() == list(range(7)) + [-1] * 113
    for i, (fr, _, vals) in enumerate(made):
        np.testing.assert_array_equal(got["blur_bins"][i], np.array(vals))
        cp, st = fr.color_palette.contents, fr.rgb_stats.contents
        assert got["rgb_stats"][i].tolist() == [st.Br, st.Bg, st.Bb, st.Cr, st.Cg, st.Cb]
        assert got["palette_percentages"][i, :cp.N].tolist() == [cp.percentages[k] for k in range(cp.N)]
        assert got["palette_hsv"][i, cp.N - 1].tolist() == [cp.averages[cp.N - 1].h, cp.averages[cp.N - 1].s,
                                                            cp.averages[cp.N - 1].v]
        g = fr.blur_vectors.contents
        assert got["blur_vectors"][i, 9].tolist() == [g.blur_vectors[9].angle, g.blur_vectors[9].magnitude]
        assert got["average_saturation"][i] == 0.4321
    assert got["sharpness_n"].tolist() == [3, 0] and got["sharpness"].shape == (2, 3)
    assert got["sharpness"][0].tolist() == [made[0][0].sharpness.contents.sharpness[k] for k in range(3)]


def test_rehearsal_on_one_card_reports_one_gpu():
    """Two ranks that share one card (a gloo rehearsal on a one-GPU box) are
    2 ranks on 1 GPU in the line, not "2 GPUs" (VERDICT r5 item 7)."""
    env = dict(os.environ, PHD_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--plan-only",
                        "--plan-visible-devices", "1", "--batch", "4", "--config4-images", "8",
                        "--config5-images", "8"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert (d["n_gpus"], d["ranks"]) == (1, 2), d
    assert d["config2"]["images"] == 2 * 4
