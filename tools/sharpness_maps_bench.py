"""The sharpness map entries beside the batched box entry, one process.

Section 25's workload -- 64 structured images of 4000 x 3000 on the device -- with
the full grids at T = 16, 32, 64 and 128 (stride T), T = 64 at stride 32 and 8
windows of 64 per image, through phd_sharpness_maps_device /
phd_sharpness_windows_device (values left on the device, one launch, profile slot
16) and through phd_sharpness_batch_device (the box entry: values to the host, two
launches, profile slot 5) on the same window lists: kernel microseconds per call
and the wall time of the whole call, the median of three runs of CALLS calls after
a warm-up call, with the runs themselves.  The byte bound is 3 T^2 bytes read plus
16 written per window (sharpness and variance) at the HBM peak of 8 TB/s.  Once
per workload every window's sharpness of the two entries is compared.  Prints one
JSON line per workload."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.set_device(0)
from photohive_dsp_amd.core import window_boundaries, window_grid
from photohive_dsp_amd.lib import WINDOW_SHARP_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Crop_Boundaries

H, W, N = 3000, 4000, int(os.environ.get("WIN_BENCH_IMAGES", "64"))
CALLS = int(os.environ.get("WIN_BENCH_CALLS", "4"))
SHARP_KERNEL = 5
HBM_PEAK = 8.0e12


def eight(seed, T):
    rng = np.random.default_rng(seed)
    return [(t, t + T, l, l + T) for t, l in zip(rng.integers(0, H - T + 1, 8).tolist(),
                                                  rng.integers(0, W - T + 1, 8).tolist())]


# (name, T, stride of the grid or None, per-image window lists)
SETS = [(f"full_grid_{T}", T, T, None) for T in (16, 32, 64, 128)] + \
       [("grid_64_stride_32", 64, 32, None), ("8_windows_64", 64, None, [eight(300 + i, 64) for i in range(N)])]
only = os.environ.get("WIN_BENCH_SETS")
if only:
    SETS = [s for s in SETS if s[0] in only.split(",")]


def read(bit):
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert lib.phd_profile_read(bit, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    return tot.value, cnt.value


def timed(call, bit):
    """A warm-up call, then three runs of CALLS calls: (median kernel us per call, the runs, launches per
    call, median wall ms, the runs)."""
    call()
    us, wall, launches = [], [], 0
    for _ in range(3):
        assert lib.phd_profile_kernels(1 << bit) == 0
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        wall.append((time.perf_counter() - t0) / CALLS * 1e3)
        tot, cnt = read(bit)
        lib.phd_profile_kernels(0)
        assert cnt % CALLS == 0 and cnt > 0
        launches = cnt // CALLS
        us.append(tot / CALLS * 1e3)
    return statistics.median(us), us, launches, statistics.median(wall), wall


imgs = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
for i in range(N):
    assert lib.phd_fill_structured_device(imgs[i].data_ptr(), H, W, 500 + i, 0, 1, None) == 0, last_error()
torch.cuda.synchronize()
ptrs = (ctypes.c_void_p * N)(*[imgs[i].data_ptr() for i in range(N)])
hs, ws = (ctypes.c_int * N)(*[H] * N), (ctypes.c_int * N)(*[W] * N)

for name, T, stride, lists in SETS:
    if lists is None:
        one = window_boundaries(window_grid(H, W, T, stride)[0])
        keep = [one] * N                                         # every image: the same grid
    else:
        keep = [window_boundaries(b) for b in lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * N)(*[ctypes.pointer(k) for k in keep])
    per = [int(k.N) for k in keep]
    windows = sum(per)
    sharp = [torch.empty((n,), dtype=torch.float64, device="cuda") for n in per]
    var = [torch.empty((n,), dtype=torch.float64, device="cuda") for n in per]
    ps = (ctypes.c_void_p * N)(*[t.data_ptr() for t in sharp])
    pv = (ctypes.c_void_p * N)(*[t.data_ptr() for t in var])
    flat = (ctypes.c_double * windows)()
    torch.cuda.synchronize()

    def old():
        assert lib.phd_sharpness_batch_device(imgs.data_ptr(), N, H, W, 3 * H * W, arr, flat, None) == 0, last_error()

    def new_lists():
        assert lib.phd_sharpness_windows_device(ptrs, hs, ws, N, arr, T, ps, pv, None) == 0, last_error()

    def new_maps():
        assert lib.phd_sharpness_maps_device(ptrs, hs, ws, N, T, stride, ps, pv, None) == 0, last_error()

    new = new_maps if stride else new_lists
    # once: both entries' sharpness on every window (the box entry merges fp64 tile sums, this one is exact)
    old()
    new()
    a = np.frombuffer(flat, dtype=np.float64)
    b = np.concatenate([t.cpu().numpy() for t in sharp])
    worst = float(np.max(np.abs(a - b) / np.abs(b)))

    k_new, runs_new, launches_new, wall_new, walls_new = timed(new, WINDOW_SHARP_KERNEL)
    k_old, runs_old, launches_old, wall_old, walls_old = timed(old, SHARP_KERNEL)
    bound_us = windows * (3.0 * T * T + 16.0) / HBM_PEAK * 1e6
    row = {"windows": name, "T": T, "stride": stride, "images": N, "windows_in_call": windows,
           "k_window_sharp_us_per_call": round(k_new, 1), "k_window_sharp_us_runs": [round(u, 1) for u in runs_new],
           "k_window_sharp_launches": launches_new,
           "sharpness_kernels_us_per_call": round(k_old, 1), "sharpness_kernels_us_runs": [round(u, 1) for u in runs_old],
           "sharpness_kernels_launches": launches_old, "kernel_ratio": round(k_new / k_old, 4),
           "new_call_wall_ms": round(wall_new, 3), "new_call_wall_ms_runs": [round(x, 3) for x in walls_new],
           "box_call_wall_ms": round(wall_old, 3), "box_call_wall_ms_runs": [round(x, 3) for x in walls_old],
           "call_ratio": round(wall_new / wall_old, 4),
           "byte_bound_us_at_8TBps": round(bound_us, 1), "kernel_over_byte_bound": round(k_new / bound_us, 2),
           "kernel_GBps": round(windows * (3.0 * T * T + 16.0) / (k_new * 1e-6) / 1e9, 1),
           "worst_relative_difference_of_the_two_entries": worst}
    if stride:
        row["list_entry_call_wall_ms"] = round(timed(new_lists, WINDOW_SHARP_KERNEL)[3], 3)
    print(json.dumps(row), flush=True)
    del sharp, var, flat
