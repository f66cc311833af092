"""Cost of the sharpness stage at 3000 x 4000 with ten crop boxes (the whole
image and nine 500 x 500 boxes), on this build or an older one (PHD_LIB=...):

  single image  median over ITERS warmed-up get_report calls of the device span
                (phd_last_timings()[3]) with the boxes, minus the same median
                without boxes: the per-box launches of k_sharp_pass;
  batch         (builds that have it) report_device over 64 such images with the
                same ten boxes each: the batched kernels' device time per image
                from phd_profile_read(5), and the calls' wall time with and
                without boxes.

Prints one JSON line."""
import ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
torch.cuda.set_device(0)
import photohive_dsp_amd as phd
from photohive_dsp_amd.lib import lib

H, W, ITERS, NB = 3000, 4000, 12, 64
box = lambda t, l: {"top": t, "bottom": t + 500, "left": l, "right": l + 500}
TEN = [{"top": 0, "bottom": H, "left": 0, "right": W}] + [box(250 * k, 380 * k) for k in range(8)] + \
      [box(H - 500, W - 500)]


def span(img, crops):
    ms = (ctypes.c_double * 8)()
    vals = []
    for i in range(ITERS + 3):
        phd.get_report(img, salient_characters=crops)
        lib.phd_last_timings(ms, 8)
        if i >= 3:
            vals.append(ms[3])
    return statistics.median(vals), min(vals), max(vals)


t = torch.empty((NB, H, W, 3), dtype=torch.uint8, device="cuda")
for i in range(NB):
    assert lib.phd_fill_structured_device(t[i].data_ptr(), H, W, 300 + i, 0, 1, None) == 0
img = t[0].cpu().numpy()
res = {"lib": os.path.basename(os.environ.get("PHD_LIB", "libreport_data.so")), "size": [H, W], "boxes": len(TEN)}
with_b = span(img, phd.set_bounding_boxes(TEN))
without = span(img, None)
res["single_ms_with_boxes_median_min_max"] = with_b
res["single_ms_without_boxes_median_min_max"] = without
res["single_sharpness_ms_per_image"] = with_b[0] - without[0]

if hasattr(lib, "phd_report_batch_device_crops"):
    lists = [TEN] * NB
    for _ in range(2):
        phd.report_device(t, salient_characters=lists)
    lib.phd_profile_kernels(0)
    lib.phd_profile_kernels(1 << 5)
    walls = []
    for _ in range(ITERS):
        t0 = time.perf_counter()
        phd.report_device(t, salient_characters=lists)
        walls.append(time.perf_counter() - t0)
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    lib.phd_profile_read(5, ctypes.byref(tot), ctypes.byref(cnt))
    lib.phd_profile_kernels(0)
    plain = []
    for i in range(ITERS + 2):
        t0 = time.perf_counter()
        phd.report_device(t)
        if i >= 2:
            plain.append(time.perf_counter() - t0)
    res["batch_images"] = NB
    res["batch_sharpness_launches_per_call"] = cnt.value / ITERS
    res["batch_sharpness_device_ms_per_image"] = tot.value / ITERS / NB
    res["batch_wall_ms_per_image_with_boxes_profiled"] = 1000 * statistics.median(walls) / NB
    res["batch_wall_ms_per_image_without_boxes"] = 1000 * statistics.median(plain) / NB
    res["ratio_single_over_batch"] = res["single_sharpness_ms_per_image"] / res["batch_sharpness_device_ms_per_image"]
print(json.dumps(res))
