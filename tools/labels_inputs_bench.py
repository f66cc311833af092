"""The fp64 label kernel's time and the cost of asking views, typed views and
YUV frames for label maps, at the C-ABI, one process.

kernel: one 3000 x 4000 uint16 synth.deep("hblur") image (tools/typed_bench.py's)
through phd_report_batch_device_typed_views_labels, which takes the fp64 route:
k_planar_labels (profile slot 10) and, as the yardstick, k_planar_sums (slot 4)
of the same calls: microseconds per launch (the median of three runs of CALLS
calls) and the label kernel's algorithmic bytes (24 B/px read + 2 B/px
written) per second against the 8 TB/s HBM peak.

typed: that call with and without maps, alternating, milliseconds per call.

yuv: FRAMES NV12 frames of 4000 x 3000 with maps through
phd_report_batch_device_yuv_labels, against the route without it:
phd_convert_yuv_device into buffers of the caller's, then
phd_report_batch_device_mixed_labels; alternating, images per second.

LABELS_INPUTS_BENCH_PARTS: the parts to run (default "kernel,typed,yuv").
Prints one JSON line per figure."""
import ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.set_device(0)
from photohive_dsp_amd import synth
from photohive_dsp_amd.core import make_config, make_typed_views, make_yuv_views, nv12_planes
from photohive_dsp_amd.lib import PALETTE_LABELS_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Full_Report_Data

H, W = 3000, 4000
CALLS, WARM = int(os.environ.get("LABELS_INPUTS_BENCH_CALLS", "12")), 2
FRAMES = int(os.environ.get("LABELS_INPUTS_BENCH_FRAMES", "64"))
PARTS = os.environ.get("LABELS_INPUTS_BENCH_PARTS", "kernel,typed,yuv").split(",")
HBM_PEAK = 8e12
PAL_SUMS_KERNEL = 4
NPIX = H * W
cfg = make_config()
print(json.dumps({"lib": os.environ.get("PHD_LIB", "libreport_data.so"), "size": [H, W], "parts": PARTS}), flush=True)


def read(bit):
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert lib.phd_profile_read(bit, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    return tot.value, cnt.value


if "kernel" in PARTS or "typed" in PARTS:
    img = synth.deep("hblur", H, W, 45)
    u16 = np.rint(img * 65535.0).astype(np.uint16)
    assert np.array_equal(u16 / 65535.0, img)
    t_u16 = torch.from_numpy(u16.view(np.int16)).cuda().view(torch.uint16)
    v_u16, _ = make_typed_views([t_u16])
    label = torch.empty((H, W), dtype=torch.int16, device="cuda")
    lab1 = (ctypes.c_void_p * 1)(label.data_ptr())
    outs = (ctypes.POINTER(Full_Report_Data) * 1)()
    status = (ctypes.c_int * 1)()
    torch.cuda.synchronize()

    def run_typed(with_maps):
        rc = lib.phd_report_batch_device_typed_views_labels(v_u16, 1, ctypes.byref(cfg), None,
                                                            lab1 if with_maps else None, outs, status, None)
        assert rc == 0, last_error()
        lib.phd_free_reports(outs, 1)

    for _ in range(WARM):
        run_typed(True)
        run_typed(False)

if "kernel" in PARTS:
    runs = []
    for _ in range(3):
        assert lib.phd_profile_kernels(1 << PAL_SUMS_KERNEL | 1 << PALETTE_LABELS_KERNEL) == 0
        for _ in range(CALLS):
            run_typed(True)
        runs.append((read(PAL_SUMS_KERNEL), read(PALETTE_LABELS_KERNEL)))
        lib.phd_profile_kernels(0)
    for name, k in (("palette_sums (k_planar_sums)", 0), ("palette_labels (k_planar_labels)", 1)):
        us = [r[k][0] * 1e3 / max(1, r[k][1]) for r in runs]
        fig = {"kernel": name, "us_per_launch": round(statistics.median(us), 2), "us_runs": [round(u, 2) for u in us],
               "launches": runs[0][k][1]}
        if k == 1:
            nbytes = 26.0 * NPIX
            fig.update(MB=nbytes / 1e6, TBps=round(nbytes / fig["us_per_launch"] / 1e6, 3),
                       of_hbm_peak=round(nbytes / fig["us_per_launch"] * 1e6 / HBM_PEAK, 3))
        print(json.dumps(fig), flush=True)
    dropped = int((label == -1).sum())
    print(json.dumps({"map_pixels_in_no_list": dropped, "labels_max": int(label.max())}), flush=True)

if "typed" in PARTS:
    times = {True: [], False: []}
    for _ in range(CALLS):
        for with_maps in (False, True):
            t0 = time.perf_counter()
            run_typed(with_maps)                 # returns after its downloads: the device is done
            times[with_maps].append((time.perf_counter() - t0) * 1e3)
    for with_maps in (False, True):
        v = times[with_maps]
        print(json.dumps({"route": "typed_views_labels, uint16 HWC", "maps": with_maps,
                          "ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3),
                          "ms_max": round(max(v), 3), "calls": len(v)}), flush=True)

if "yuv" in PARTS:
    N = FRAMES
    ch, cw = (H + 1) // 2, (W + 1) // 2
    surfaces = torch.empty((N, H + ch, W), dtype=torch.uint8, device="cuda")
    rgb = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    for i in range(N):
        assert lib.phd_fill_structured_device(rgb.data_ptr(), H, W, 700 + i, 0, 1, None) == 0, last_error()
        torch.cuda.synchronize()
        r, g, b = (rgb[..., k].float() for k in range(3))
        y = 0.299 * r + 0.587 * g + 0.114 * b
        surfaces[i, :H] = y.round().clamp(0, 255).to(torch.uint8)
        uv = surfaces[i, H:].view(ch, cw, 2)
        uv[..., 0] = (128 + 0.564 * (b - y))[::2, ::2].round().clamp(0, 255).to(torch.uint8)
        uv[..., 1] = (128 + 0.713 * (r - y))[::2, ::2].round().clamp(0, 255).to(torch.uint8)
    del rgb, r, g, b, y
    views, keep = make_yuv_views([nv12_planes(surfaces[i], H, W) for i in range(N)])
    maps = torch.empty((N, H, W), dtype=torch.int16, device="cuda")
    packed = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lab = (ctypes.c_void_p * N)(*[maps[i].data_ptr() for i in range(N)])
    dst = (ctypes.c_void_p * N)(*[packed[i].data_ptr() for i in range(N)])
    hs, ws = (ctypes.c_int * N)(*[H] * N), (ctypes.c_int * N)(*[W] * N)
    outs = (ctypes.POINTER(Full_Report_Data) * N)()
    status = (ctypes.c_int * N)()

    def yuv_labels():
        rc = lib.phd_report_batch_device_yuv_labels(views, N, ctypes.byref(cfg), None, lab, outs, status, None)
        assert rc == 0, last_error()
        lib.phd_free_reports(outs, N)

    def convert_then_packed():
        assert lib.phd_convert_yuv_device(views, N, dst, None) == 0, last_error()
        rc = lib.phd_report_batch_device_mixed_labels(dst, hs, ws, N, ctypes.byref(cfg), None, lab, outs, status, None)
        assert rc == 0, last_error()
        lib.phd_free_reports(outs, N)

    routes = {"phd_report_batch_device_yuv_labels": yuv_labels,
              "phd_convert_yuv_device + phd_report_batch_device_mixed_labels": convert_then_packed}
    for fn in routes.values():
        fn()
    rates = {k: [] for k in routes}
    for _ in range(3):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            for _ in range(2):
                fn()
            rates[k].append(2 * N / (time.perf_counter() - t0))
    for k, v in rates.items():
        print(json.dumps({"route": k, "frames": N, "images_per_s": round(statistics.median(v), 1),
                          "runs": [round(x, 1) for x in v]}), flush=True)
