"""Cost of the image views' input stage on 64 device-resident 3000 x 4000
images (splitmix64 uniform bytes, seed = image index, as bench.py's headline
images), at the C-ABI (reports freed after each step, as bench.py does).

End to end, images/s, each figure from RUNS runs of STEPS steps after warm-up,
the routes alternating within a run:
  (a) phd_report_batch_device_views on [64, 3, H, W] CHW and [64, H, W, 4] RGBA
  (b) the route without views: permute(0, 2, 3, 1).contiguous() (CHW) or
      [..., :3].contiguous() (RGBA) in torch, then phd_report_batch_device
  (c) phd_report_batch_device on already packed input (the floor)

The pack kernel alone, from profile bit 6 around phd_pack_views_device over
the 64 views of one kind (one launch): microseconds per image, bytes moved per
second (bytes read + bytes written) and the share of the 8 TB/s HBM peak, for
the pitched, 4-byte, planar and generic (BGR: channel stride -1) kinds.

Prints one JSON line per figure."""
import ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
torch.cuda.set_device(0)
import photohive_dsp_amd as phd
from photohive_dsp_amd.core import make_config, make_views
from photohive_dsp_amd.lib import PACK_VIEWS_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Full_Report_Data

H, W, N = 3000, 4000, 64
RUNS, STEPS, WARM = 3, int(os.environ.get("VIEWS_BENCH_STEPS", "30")), 2
HBM_PEAK = 8e12

packed = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
for i in range(N):
    assert lib.phd_fill_uniform_device(packed[i].data_ptr(), packed[i].numel(), i, None) == 0, last_error()
chw = packed.permute(0, 3, 1, 2).contiguous()
rgba = torch.cat([packed, torch.full((N, H, W, 1), 255, dtype=torch.uint8, device="cuda")], dim=3).contiguous()
frame = torch.zeros((N, H, W + 16, 3), dtype=torch.uint8, device="cuda")
frame[:, :, :W] = packed
pitched = frame[:, :, :W]
torch.cuda.synchronize()

cfg = make_config()
outs = (ctypes.POINTER(Full_Report_Data) * N)()
status = (ctypes.c_int * N)()


def run_packed(t):
    rc = lib.phd_report_batch_device(t.data_ptr(), N, H, W, 0, ctypes.byref(cfg), outs, status, None)
    assert rc == 0, last_error()
    lib.phd_free_reports(outs, N)


def run_views(views):
    rc = lib.phd_report_batch_device_views(views, N, ctypes.byref(cfg), None, outs, status, None)
    assert rc == 0, last_error()
    lib.phd_free_reports(outs, N)


v_chw, _ = make_views(chw, "CHW")
v_rgba, _ = make_views(rgba)
routes = {
    "a_views_chw": lambda: run_views(v_chw),
    "b_torch_chw": lambda: run_packed(chw.permute(0, 2, 3, 1).contiguous()),
    "a_views_rgba": lambda: run_views(v_rgba),
    "b_torch_rgba": lambda: run_packed(rgba[..., :3].contiguous()),
    "c_packed": lambda: run_packed(packed),
}
for f in routes.values():
    for _ in range(WARM):
        f()
rates = {k: [] for k in routes}
for _ in range(RUNS):
    for name, f in routes.items():          # the routes alternate within a run
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            f()
        torch.cuda.synchronize()
        rates[name].append(N * STEPS / (time.perf_counter() - t0))
for name, r in rates.items():
    print(json.dumps({"route": name, "images_per_s_runs": [round(x, 1) for x in r],
                      "median": round(statistics.median(r), 1), "spread": round(max(r) - min(r), 1),
                      "size": [H, W], "batch": N, "steps_per_run": STEPS, "lanes": lib.phd_set_lanes(0)}))
med = {k: statistics.median(v) for k, v in rates.items()}
print(json.dumps({"gather_share_of_step_chw": round(1 - med["a_views_chw"] / med["c_packed"], 4),
                  "gather_share_of_step_rgba": round(1 - med["a_views_rgba"] / med["c_packed"], 4),
                  "views_over_torch_chw": round(med["a_views_chw"] / med["b_torch_chw"], 4),
                  "views_over_torch_rgba": round(med["a_views_rgba"] / med["b_torch_rgba"], 4)}))

# ---- the pack kernel alone -------------------------------------------------------
dst = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
d_ptrs = (ctypes.c_void_p * N)(*[dst[i].data_ptr() for i in range(N)])
kinds = {
    "pitched": (make_views(pitched)[0], 3 * H * W + 3 * H * W),
    "px4_rgba": (v_rgba, 4 * H * W + 3 * H * W),
    "planar_chw": (v_chw, 3 * H * W + 3 * H * W),
    "generic_bgr": (make_views(packed, bgr=True)[0], 3 * H * W + 3 * H * W),
}
tot, cnt = ctypes.c_double(), ctypes.c_long()
for name, (views, nbytes) in kinds.items():
    for _ in range(WARM):
        assert lib.phd_pack_views_device(views, N, d_ptrs, None) == 0, last_error()
    assert torch.equal(dst, packed.flip(-1) if name == "generic_bgr" else packed), name
    per_image = []
    for _ in range(RUNS):
        lib.phd_profile_kernels(1 << PACK_VIEWS_KERNEL)
        for _ in range(STEPS):
            assert lib.phd_pack_views_device(views, N, d_ptrs, None) == 0, last_error()
        lib.phd_profile_read(PACK_VIEWS_KERNEL, ctypes.byref(tot), ctypes.byref(cnt))
        lib.phd_profile_kernels(0)
        assert cnt.value == STEPS, (name, cnt.value)
        per_image.append(1e3 * tot.value / cnt.value / N)
    us = statistics.median(per_image)
    print(json.dumps({"pack_kind": name, "us_per_image_runs": [round(x, 2) for x in per_image],
                      "us_per_image": round(us, 2), "bytes_per_image": nbytes,
                      "TB_per_s": round(nbytes / us / 1e6, 3), "share_of_hbm_peak": round(nbytes / us * 1e6 / HBM_PEAK, 3),
                      "launches_per_call": 1}))
