"""The palette label kernel's time and the cost of asking for maps, at the
C-ABI, one process.

64 device images of 4000 x 3000 (synth.py:structured, filled on the device)
through phd_report_batch_device_mixed_labels on a grid whose palette runs K1
histogram + Kcut + the batched K3 (phd_debug_palette_path: bit 1 clear, bit 32
set), so k_palette_sums_b (profile slot 4) and k_palette_labels_b (slot 10)
run on the same images in the same calls: milliseconds per launch and
microseconds per image of each (the median of three runs of CALLS calls), and
the label kernel's algorithmic bytes (3 B/px read + 2 B/px written) per second
and their share of the 8 TB/s HBM peak.  Then, with the profiler off, images
per second of the call with and without maps, alternating.

LABELS_BENCH_GRID: h360_s4 (default; saturation class from thresholds) or
s10_twopass (from the table in global memory).  Prints one JSON line per figure."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.cuda.set_device(0)
from photohive_dsp_amd.core import make_config
from photohive_dsp_amd.lib import PALETTE_LABELS_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Full_Report_Data
from tests import palette_grids as pg

H, W, N = 3000, 4000, int(os.environ.get("LABELS_BENCH_IMAGES", "64"))
CALLS = int(os.environ.get("LABELS_BENCH_CALLS", "4"))
GRID = os.environ.get("LABELS_BENCH_GRID", "h360_s4")
HBM_PEAK = 8e12
PAL_SUMS_KERNEL = 4
NPIX = H * W

kw = pg.grid(GRID)
cfg = make_config(**kw)
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


def call(with_maps):
    rc = lib.phd_report_batch_device_mixed_labels(ptrs, hs, ws, N, ctypes.byref(cfg), None,
                                                  lab if with_maps else None, outs, st, None)
    assert rc == 0, last_error()
    slots = max(outs[i].contents.color_palette.contents.N for i in range(N))
    lib.phd_free_reports(outs, N)
    return slots


slots = call(True)
mask = pg.path(kw, slots)
assert mask >= 0 and not mask & pg.FUSED and mask & pg.BATCHED, pg.describe(mask)
print(json.dumps({"grid": GRID, "images": N, "size": [H, W], "max_slots": slots, "path": pg.describe(mask),
                  "lib": os.environ.get("PHD_LIB", "libreport_data.so")}), flush=True)


def read(bit):
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert lib.phd_profile_read(bit, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    return tot.value, cnt.value


runs = []
for _ in range(3):
    assert lib.phd_profile_kernels(1 << PAL_SUMS_KERNEL | 1 << PALETTE_LABELS_KERNEL) == 0
    for _ in range(CALLS):
        call(True)
    runs.append((read(PAL_SUMS_KERNEL), read(PALETTE_LABELS_KERNEL)))
    lib.phd_profile_kernels(0)
for name, k in (("palette_sums (k_palette_sums_b)", 0), ("palette_labels (k_palette_labels_b)", 1)):
    ms = [r[k][0] / max(1, r[k][1]) for r in runs]
    us_img = statistics.median(ms) * 1e3 / N
    fig = {"kernel": name, "ms_per_launch": round(statistics.median(ms), 4), "ms_runs": [round(m, 4) for m in ms],
           "launches": runs[0][k][1], "us_per_image": round(us_img, 2)}
    if k == 1:
        nbytes = 5.0 * NPIX
        fig.update(MB_per_image=nbytes / 1e6, TBps=round(nbytes / us_img / 1e6, 3),
                   of_hbm_peak=round(nbytes / us_img * 1e6 / HBM_PEAK, 3))
    print(json.dumps(fig), flush=True)

rates = {True: [], False: []}
for _ in range(3):
    for with_maps in (False, True):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call(with_maps)                      # returns after its downloads: the device is done
        rates[with_maps].append(CALLS * N / (time.perf_counter() - t0))
print(json.dumps({"images_per_s_without_maps": round(statistics.median(rates[False]), 1),
                  "runs_without": [round(r, 1) for r in rates[False]],
                  "images_per_s_with_maps": round(statistics.median(rates[True]), 1),
                  "runs_with": [round(r, 1) for r in rates[True]]}), flush=True)
