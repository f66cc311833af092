"""The box palette kernel's time and the cost of asking for box palettes, at the
C-ABI, one process.

1. The kernel alone: 64 label maps of 4000 x 3000 on the device (labels in runs
of 16 along a row, blocks of 8 rows: what a quantised photo looks like to the
counters) through phd_box_palettes_device with three box sets -- 8 face-sized
boxes per image (600 x 600), 200 small ones (64 x 64) and the whole image --
and a 17-slot and a 1000-slot palette: k_box_counts' microseconds per call from
profile slot 11 (the median of three runs of CALLS calls), the bytes it reads
(2 B per box element) per second and their share of the 8 TB/s HBM peak, the
wall time of the whole call, and beside it what a caller does today:
torch.bincount per box over the same device maps, synchronised per box.

2. In the call: images per second of phd_report_batch_device_mixed_box_palettes
with scratch maps (d_labels NULL) on 64 images of 4000 x 3000 with the 8
face-sized boxes each, against phd_report_batch_device_mixed_crops (no maps)
and phd_report_batch_device_mixed_labels (maps, no counts), alternating, three
runs each.  Prints one JSON line per figure."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.set_device(0)
from photohive_dsp_amd.core import make_config, normalize_salient
from photohive_dsp_amd.lib import BOX_PALETTES_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Full_Report_Data, PhdBoxPalette

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


# ---- 1. the kernel alone ----------------------------------------------------------------
for n_slots in (17, 1000):
    low = torch.randint(0, n_slots, (N, H // 8, W // 16), dtype=torch.int16, device="cuda")
    maps = low.repeat_interleave(8, dim=1).repeat_interleave(16, dim=2).contiguous()
    del low
    torch.cuda.synchronize()
    mp = (ctypes.c_void_p * N)(*[maps[i].data_ptr() for i in range(N)])
    hs, ws = (ctypes.c_int * N)(*[H] * N), (ctypes.c_int * N)(*[W] * N)
    ns = (ctypes.c_int * N)(*[n_slots] * N)
    for name in SETS[0]:
        crops = normalize_salient([s[name] for s in SETS], N)
        elems = sum((b["bottom"] - b["top"]) * (b["right"] - b["left"]) for s in SETS for b in s[name])
        boxes = sum(len(s[name]) for s in SETS)
        bp = (PhdBoxPalette * N)()

        def stage():
            assert lib.phd_box_palettes_device(mp, hs, ws, N, ns, crops[0], bp, None) == 0, last_error()
            first = np.ctypeslib.as_array(bp[0].counts, shape=(bp[0].n_boxes, n_slots + 1)).copy()
            lib.phd_free_box_palettes(bp, N)
            return first

        got = stage()
        us, wall = [], []
        for _ in range(3):
            assert lib.phd_profile_kernels(1 << BOX_PALETTES_KERNEL) == 0
            t0 = time.perf_counter()
            for _ in range(CALLS):
                stage()
            wall.append((time.perf_counter() - t0) / CALLS * 1e3)
            tot, cnt = read(BOX_PALETTES_KERNEL)
            lib.phd_profile_kernels(0)
            assert cnt == CALLS
            us.append(tot / cnt * 1e3)
        # what a caller does today: one bincount and one sync per box
        t0 = time.perf_counter()
        want0 = []
        for i in range(N):
            for b in SETS[i][name]:
                part = maps[i, b["top"]:b["bottom"], b["left"]:b["right"]].reshape(-1).to(torch.int32)
                c = torch.bincount(part, minlength=n_slots + 1)
                torch.cuda.synchronize()
                if i == 0:
                    want0.append(c.cpu().numpy())
        t_bin = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(np.array(want0, dtype=np.uint32), got), "kernel and bincount disagree"
        k = statistics.median(us)
        print(json.dumps({"n_slots": n_slots, "boxes": name, "maps": N, "boxes_in_call": boxes,
                          "box_elements": elems, "k_box_counts_us_per_call": round(k, 1),
                          "us_runs": [round(u, 1) for u in us], "MB_read": round(2 * elems / 1e6, 1),
                          "TBps": round(2 * elems / k / 1e6, 3),
                          "of_hbm_peak": round(2 * elems / k * 1e6 / HBM_PEAK, 3),
                          "call_wall_ms": round(statistics.median(wall), 2),
                          "bincount_per_box_wall_ms": round(t_bin, 1)}), flush=True)
    del maps
    torch.cuda.empty_cache()

# ---- 2. in the report call -------------------------------------------------------------------
cfg = make_config()
imgs = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
for i in range(N):
    assert lib.phd_fill_structured_device(imgs[i].data_ptr(), H, W, 500 + i, 0, 1, None) == 0, last_error()
maps = torch.empty((N, H, W), dtype=torch.int16, device="cuda")
torch.cuda.synchronize()
ptrs = (ctypes.c_void_p * N)(*[imgs[i].data_ptr() for i in range(N)])
hs, ws = (ctypes.c_int * N)(*[H] * N), (ctypes.c_int * N)(*[W] * N)
lab = (ctypes.c_void_p * N)(*[maps[i].data_ptr() for i in range(N)])
outs = (ctypes.POINTER(Full_Report_Data) * N)()
st = (ctypes.c_int * N)()
crops = normalize_salient([s["8_faces_600x600"] for s in SETS], N)
bp = (PhdBoxPalette * N)()


def call(kind):
    if kind == "crops":
        rc = lib.phd_report_batch_device_mixed_crops(ptrs, hs, ws, N, ctypes.byref(cfg), crops[0], outs, st, None)
    elif kind == "labels":
        rc = lib.phd_report_batch_device_mixed_labels(ptrs, hs, ws, N, ctypes.byref(cfg), crops[0], lab, outs, st, None)
    else:
        rc = lib.phd_report_batch_device_mixed_box_palettes(ptrs, hs, ws, N, ctypes.byref(cfg), crops[0], None, bp,
                                                            outs, st, None)
        lib.phd_free_box_palettes(bp, N)
    assert rc == 0, last_error()
    lib.phd_free_reports(outs, N)


KINDS = ("crops", "labels", "box_palettes")
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
