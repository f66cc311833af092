"""The box statistics kernel's time and the cost of asking for box statistics, at
the C-ABI, one process.

1. The kernel alone: 64 structured images of 4000 x 3000 on the device through
phd_box_stats_device with three box sets -- 8 face-sized boxes per image
(600 x 600), 200 small ones (64 x 64) and the whole image: k_box_stats'
microseconds per call from profile slot 12 (the median of three runs of CALLS
calls), the bytes it reads (3 B per box pixel) per second and their share of
the 8 TB/s HBM peak, the wall time of the whole call, and beside it what a
caller does today: a torch reduction per box over the same device images,
synchronised per box.

2. In the call: images per second of phd_report_batch_device_mixed_box_stats
(d_labels and box_palettes NULL) on 64 images of 4000 x 3000 with the 8
face-sized boxes each, against phd_report_batch_device_mixed_crops, alternating,
three runs each.  BOX_BENCH_CALL_ONLY=1: part 2 alone (an A/B of two builds
through PHD_LIB).  Prints one JSON line per figure."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.set_device(0)
from photohive_dsp_amd.core import make_config, normalize_salient
from photohive_dsp_amd.lib import BOX_STATS_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Full_Report_Data, PhdBoxStats

H, W, N = 3000, 4000, int(os.environ.get("BOX_BENCH_IMAGES", "64"))
CALLS = int(os.environ.get("BOX_BENCH_CALLS", "4"))
HBM_PEAK = 8e12


def box_sets(seed):
    rng = np.random.default_rng(seed)

    def some(k, bh, bw):
        out = []
        for _ in range(k):
            t, l = int(rng.integers(0, H - bh + 1)), int(rng.integers(0, W - bw + 1))
            out.append(dict(top=t, bottom=t + bh, left=l, right=l + bw))
        return out
    return {"8_faces_600x600": some(8, 600, 600), "200_small_64x64": some(200, 64, 64),
            "whole_image": [dict(top=0, bottom=H, left=0, right=W)]}


SETS = [box_sets(100 + i) for i in range(N)]


def read(bit):
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert lib.phd_profile_read(bit, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    return tot.value, cnt.value


imgs = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
for i in range(N):
    assert lib.phd_fill_structured_device(imgs[i].data_ptr(), H, W, 500 + i, 0, 1, None) == 0, last_error()
torch.cuda.synchronize()
ptrs = (ctypes.c_void_p * N)(*[imgs[i].data_ptr() for i in range(N)])
hs, ws = (ctypes.c_int * N)(*[H] * N), (ctypes.c_int * N)(*[W] * N)

# ---- 1. the kernel alone ----------------------------------------------------------------
for name in ([] if os.environ.get("BOX_BENCH_CALL_ONLY") else SETS[0]):
    crops = normalize_salient([s[name] for s in SETS], N)
    pixels = sum((b["bottom"] - b["top"]) * (b["right"] - b["left"]) for s in SETS for b in s[name])
    boxes = sum(len(s[name]) for s in SETS)
    bs = (PhdBoxStats * N)()

    def stage():
        assert lib.phd_box_stats_device(ptrs, hs, ws, N, crops[0], bs, None) == 0, last_error()
        nb = bs[0].n_boxes
        first = np.concatenate([np.ctypeslib.as_array(ctypes.cast(bs[0].stats, ctypes.POINTER(ctypes.c_double)),
                                                      shape=(nb, 6)),
                                np.ctypeslib.as_array(bs[0].average_saturation, shape=(nb,))[:, None]], axis=1).copy()
        lib.phd_free_box_stats(bs, N)
        return first

    got = stage()
    us, wall = [], []
    for _ in range(3):
        assert lib.phd_profile_kernels(1 << BOX_STATS_KERNEL) == 0
        t0 = time.perf_counter()
        for _ in range(CALLS):
            stage()
        wall.append((time.perf_counter() - t0) / CALLS * 1e3)
        tot, cnt = read(BOX_STATS_KERNEL)
        lib.phd_profile_kernels(0)
        assert cnt == CALLS
        us.append(tot / cnt * 1e3)
    # what a caller does today: slice, reduce and synchronise per box
    t0 = time.perf_counter()
    want0 = []
    for i in range(N):
        for b in SETS[i][name]:
            c = imgs[i, b["top"]:b["bottom"], b["left"]:b["right"]].reshape(-1, 3).to(torch.float64) / 255.0
            mean = c.mean(dim=0)
            std = ((c - mean) ** 2).mean(dim=0).sqrt()
            mx, mn = c.max(dim=1).values, c.min(dim=1).values
            s = torch.where(mx == 0, torch.zeros_like(mx),
                            torch.where(mn == 0, torch.full_like(mx, 0.999999), (mx - mn) / mx.clamp_min(1e-300)))
            row = torch.cat([mean, std, s.mean().reshape(1)])
            torch.cuda.synchronize()
            if i == 0:
                want0.append(row.cpu().numpy())
    t_torch = (time.perf_counter() - t0) * 1e3
    agree = bool(np.allclose(np.array(want0), got, rtol=1e-9, atol=1e-12))
    k = statistics.median(us)
    print(json.dumps({"boxes": name, "images": N, "boxes_in_call": boxes, "box_pixels": pixels,
                      "k_box_stats_us_per_call": round(k, 1), "us_runs": [round(u, 1) for u in us],
                      "MB_read": round(3 * pixels / 1e6, 1), "TBps": round(3 * pixels / k / 1e6, 3),
                      "of_hbm_peak": round(3 * pixels / k * 1e6 / HBM_PEAK, 3),
                      "call_wall_ms": round(statistics.median(wall), 2),
                      "torch_per_box_wall_ms": round(t_torch, 1), "torch_agrees": agree}), flush=True)

if os.environ.get("BOX_BENCH_KERNEL_ONLY"):      # a row-fetch variant build (PHD_LIB): the kernel's figures only
    sys.exit(0)

# ---- 2. in the report call -------------------------------------------------------------------
cfg = make_config()
outs = (ctypes.POINTER(Full_Report_Data) * N)()
st = (ctypes.c_int * N)()
crops = normalize_salient([s["8_faces_600x600"] for s in SETS], N)
bs = (PhdBoxStats * N)()


def call(kind):
    if kind == "crops":
        rc = lib.phd_report_batch_device_mixed_crops(ptrs, hs, ws, N, ctypes.byref(cfg), crops[0], outs, st, None)
    else:
        rc = lib.phd_report_batch_device_mixed_box_stats(ptrs, hs, ws, N, ctypes.byref(cfg), crops[0], None, None, bs,
                                                         outs, st, None)
        lib.phd_free_box_stats(bs, N)
    assert rc == 0, last_error()
    lib.phd_free_reports(outs, N)


KINDS = ("crops", "box_stats")
for k in KINDS:
    call(k)
rates = {k: [] for k in KINDS}
for _ in range(3):
    for k in KINDS:
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call(k)                              # returns after its downloads: the device is done
        rates[k].append(CALLS * N / (time.perf_counter() - t0))
print(json.dumps({"images": N, "size": [H, W], "boxes_per_image": 8,
                  **{f"images_per_s_{k}": round(statistics.median(rates[k]), 1) for k in KINDS},
                  **{f"runs_{k}": [round(r, 1) for r in rates[k]] for k in KINDS}}), flush=True)
