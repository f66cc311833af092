"""Cost of the typed-view input stage on one 3000 x 4000 16-bit image
(synth.deep("hblur")), at the C-ABI, one process.

End to end, milliseconds per call, the median of CALLS calls after warm-up, the
two routes alternating:
  (a) phd_report_batch_device_typed_views on the uint16 [H, W, 3] device tensor
  (b) the route without typed views: get_full_report_data on three host planes
      of doubles (288 MB over PCIe)
and of each its input stage: (a) the classify + decode kernels' event time,
(b) the three plane uploads, timed alone as pageable host-to-device copies of
the same planes into a device buffer.

The kernels alone, from the profile bits' event times (7 classify_views, 8
decode_views, 6 pack_views): microseconds per launch, bytes read + written per
second and the share of the 8 TB/s HBM peak, for uint16 HWC and float32 CHW
sources, next to k_pack_views on the uint8 CHW image of the same shape.

Prints one JSON line per figure."""
import ctypes, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
torch.cuda.set_device(0)
import photohive_dsp_amd as phd
from photohive_dsp_amd import synth
from photohive_dsp_amd.core import make_config, make_typed_views, make_views
from photohive_dsp_amd.lib import CLASSIFY_VIEWS_KERNEL, DECODE_VIEWS_KERNEL, PACK_VIEWS_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Full_Report_Data, Image_RGB

H, W = 3000, 4000
CALLS, WARM = int(os.environ.get("TYPED_BENCH_CALLS", "12")), 2
HBM_PEAK = 8e12
NPIX = H * W

img = synth.deep("hblur", H, W, 45)
u16 = np.rint(img * 65535.0).astype(np.uint16)
assert np.array_equal(u16 / 65535.0, img)
planes = [np.ascontiguousarray(img[..., k]).ravel() for k in range(3)]
t_u16 = torch.from_numpy(u16.view(np.int16)).cuda().view(torch.uint16)
t_f32 = torch.from_numpy(np.ascontiguousarray(img.astype(np.float32).transpose(2, 0, 1))).cuda()
t_u8 = torch.from_numpy(np.ascontiguousarray(synth.make("hblur", H, W, 45).transpose(2, 0, 1))).cuda()
torch.cuda.synchronize()
cfg = make_config()
outs = (ctypes.POINTER(Full_Report_Data) * 1)()
status = (ctypes.c_int * 1)()
v_u16, _ = make_typed_views([t_u16])
v_f32, _ = make_typed_views([t_f32], "CHW")


def run_typed(views):
    rc = lib.phd_report_batch_device_typed_views(views, 1, ctypes.byref(cfg), None, outs, status, None)
    assert rc == 0, last_error()
    lib.phd_free_reports(outs, 1)


def run_legacy():
    P = ctypes.POINTER(ctypes.c_double)
    im = Image_RGB(height=H, width=W, r=planes[0].ctypes.data_as(P), g=planes[1].ctypes.data_as(P),
                   b=planes[2].ctypes.data_as(P))
    c = cfg
    ptr = lib.get_full_report_data(ctypes.byref(im), None, c.h_partitions, c.s_partitions, c.v_partitions,
                                   c.black_thresh, c.gray_thresh, c.coverage_thresh, c.linked_list_size,
                                   c.downsample_rate, c.radius_partitions, c.angle_partitions, c.quantity_weight,
                                   c.saturation_value_weight, c.fft_streak_thresh, c.magnitude_thresh,
                                   c.blur_cutoff_ratio_denom)
    assert ptr, last_error()
    lib.free_full_report(ctypes.byref(ptr))


dev_planes = torch.empty(3 * NPIX, dtype=torch.float64, device="cuda")
host_planes = [torch.from_numpy(p) for p in planes]          # pageable, as a C caller's planes


def run_upload():
    for k in range(3):
        dev_planes[k * NPIX:(k + 1) * NPIX].copy_(host_planes[k])
    torch.cuda.synchronize()


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def profiled(bit, fn, n):
    """(microseconds per launch, launches) of kernel `bit` over n calls of fn"""
    assert lib.phd_profile_kernels(1 << bit) == 0
    for _ in range(n):
        fn()
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    lib.phd_profile_read(bit, ctypes.byref(tot), ctypes.byref(cnt))
    lib.phd_profile_kernels(0)
    return tot.value * 1e3 / max(1, cnt.value), cnt.value


routes = {"typed_u16_device": lambda: run_typed(v_u16), "legacy_host_doubles": run_legacy, "upload_alone": run_upload}
for fn in routes.values():
    for _ in range(WARM):
        fn()
times = {k: [] for k in routes}
for _ in range(CALLS):
    for k, fn in routes.items():
        times[k].append(wall(fn))
for k, v in times.items():
    print(json.dumps({"route": k, "ms_median": round(statistics.median(v), 3), "ms_min": round(min(v), 3),
                      "ms_max": round(max(v), 3), "calls": len(v)}), flush=True)

# the kernels alone
dst = torch.empty((3, H, W), dtype=torch.float64, device="cuda")
d_ptr = (ctypes.c_void_p * 1)(dst.data_ptr())
d8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
d8_ptr = (ctypes.c_void_p * 1)(d8.data_ptr())
v_u8, _ = make_views([t_u8], "CHW")


def decode(views):
    assert lib.phd_decode_views_device(views, 1, d_ptr, None) == 0, last_error()


def pack():
    assert lib.phd_pack_views_device(v_u8, 1, d8_ptr, None) == 0, last_error()


figures = [("decode_views", "u16 HWC", DECODE_VIEWS_KERNEL, lambda: decode(v_u16), NPIX * (6 + 24)),
           ("decode_views", "f32 CHW", DECODE_VIEWS_KERNEL, lambda: decode(v_f32), NPIX * (12 + 24)),
           ("classify_views", "u16 HWC", CLASSIFY_VIEWS_KERNEL, lambda: run_typed(v_u16), NPIX * (6 + 3)),
           ("classify_views", "f32 CHW", CLASSIFY_VIEWS_KERNEL, lambda: run_typed(v_f32), NPIX * (12 + 3)),
           ("pack_views", "u8 CHW", PACK_VIEWS_KERNEL, pack, NPIX * (3 + 3))]
for kernel, source, bit, fn, nbytes in figures:
    fn()
    runs = [profiled(bit, fn, CALLS) for _ in range(3)]
    us = statistics.median(r[0] for r in runs)
    print(json.dumps({"kernel": kernel, "source": source, "us_per_launch": round(us, 2),
                      "us_runs": [round(r[0], 2) for r in runs], "launches": runs[0][1], "MB": nbytes / 1e6,
                      "TBps": round(nbytes / us / 1e6, 3), "of_hbm_peak": round(nbytes / us * 1e6 / HBM_PEAK, 3)}),
          flush=True)
