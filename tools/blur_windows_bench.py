"""The window blur kernel's time at the C-ABI, one process.

64 structured images of 4000 x 3000 on the device through
phd_blur_windows_device with three window sets -- the full grid at T = 128
(31 x 23 windows per image), the full grid at T = 64 (62 x 46) and 8 windows of
128 per image -- at the wrappers' 16 x 36 grid: k_window_blur's microseconds per
call from profile slot 14 (summed over the call's chunks; the median of three
runs of CALLS calls), the bytes it moves (3 T^2 read and 8 nbins written per
window) per second and their share of the 8 TB/s HBM peak, and the wall time of
the whole call (launches, downloads and the host's finish).  Beside each, as a
yardstick: the synchronised time of torch's fp64 rfft2 over the same windows
(luma by a matrix product, the windows gathered, one batched transform per
image).  Prints one JSON line per set."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.set_device(0)
from photohive_dsp_amd.core import WINDOW_DEFAULTS, make_config, window_boundaries, window_grid
from photohive_dsp_amd.lib import WINDOW_BLUR_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Crop_Boundaries, PhdWindowBlur

H, W, N = 3000, 4000, int(os.environ.get("WIN_BENCH_IMAGES", "64"))
CALLS = int(os.environ.get("WIN_BENCH_CALLS", "4"))
HBM_PEAK = 8e12
cfg = make_config(**WINDOW_DEFAULTS)
NBINS = cfg.angle_partitions * cfg.radius_partitions


def eight(seed, T):
    rng = np.random.default_rng(seed)
    return [(t, t + T, l, l + T) for t, l in zip(rng.integers(0, H - T + 1, 8).tolist(),
                                                  rng.integers(0, W - T + 1, 8).tolist())]


SETS = [("full_grid_128", 128, [window_grid(H, W, 128)[0]] * N), ("full_grid_64", 64, [window_grid(H, W, 64)[0]] * N),
        ("8_windows_128", 128, [eight(300 + i, 128) for i in range(N)])]


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
coef = torch.tensor([0.299, 0.587, 0.114], dtype=torch.float64, device="cuda")

for name, T, lists in SETS:
    keep = [window_boundaries(b) for b in lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * N)(*[ctypes.pointer(k) for k in keep])
    windows = sum(len(b) for b in lists)
    wb = (PhdWindowBlur * N)()

    def stage():
        assert lib.phd_blur_windows_device(ptrs, hs, ws, N, arr, T, ctypes.byref(cfg), wb, None) == 0, last_error()
        first = float(wb[0].fft_max[0])
        lib.phd_free_window_blur(wb, N)
        return first

    got = stage()
    us, wall, launches = [], [], 0
    for _ in range(3):
        assert lib.phd_profile_kernels(1 << WINDOW_BLUR_KERNEL) == 0
        t0 = time.perf_counter()
        for _ in range(CALLS):
            stage()
        wall.append((time.perf_counter() - t0) / CALLS * 1e3)
        tot, cnt = read(WINDOW_BLUR_KERNEL)
        lib.phd_profile_kernels(0)
        assert cnt % CALLS == 0 and cnt > 0
        launches = cnt // CALLS
        us.append(tot / CALLS * 1e3)
    # the yardstick: torch's fp64 rfft2 over the same windows, synchronised
    idx = torch.arange(T, device="cuda")
    t0 = time.perf_counter()
    first = None
    for i in range(N):
        luma = (imgs[i].to(torch.float64) / 255.0) @ coef
        tl = torch.tensor([(b[0], b[2]) for b in lists[i]], device="cuda")
        rows = (tl[:, 0, None] + idx)[:, :, None]
        cols = (tl[:, 1, None] + idx)[:, None, :]
        win = luma[rows, cols]
        p = torch.fft.rfft2(win - win.mean(dim=(1, 2), keepdim=True))
        mx = (p.real * p.real + p.imag * p.imag).amax(dim=(1, 2))
        if i == 0:
            first = float(mx[0])
    torch.cuda.synchronize()
    t_torch = (time.perf_counter() - t0) * 1e3
    k = statistics.median(us)
    moved = windows * (3 * T * T + 8 * NBINS)
    print(json.dumps({"windows": name, "T": T, "images": N, "windows_in_call": windows, "launches_per_call": launches,
                      "k_window_blur_us_per_call": round(k, 1), "us_runs": [round(u, 1) for u in us],
                      "us_per_window": round(k / windows, 3), "MB_moved": round(moved / 1e6, 1),
                      "TBps": round(moved / k / 1e6, 3), "of_hbm_peak": round(moved / k * 1e6 / HBM_PEAK, 4),
                      "call_wall_ms": round(statistics.median(wall), 2), "torch_rfft2_fp64_wall_ms": round(t_torch, 1),
                      "fft_max_window0": got, "torch_max_window0_mean_removed": first}), flush=True)
