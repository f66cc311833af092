"""The blur vectors entry beside the window blur entry, one process.

Section 24's three workloads -- 64 structured images of 4000 x 3000 on the device,
the full grid at T = 128, the full grid at T = 64 and 8 windows of 128 per image,
at the wrappers' 16 x 36 grid -- through phd_blur_windows_device (bins, vectors
and maxima on the host) and phd_blur_vectors_device (vectors and maxima left on
the device) on the same window lists: k_window_vectors' microseconds per call from
profile slot 15 next to k_window_blur's from slot 14 (summed over that call's
chunks), and the wall time of both whole calls; the median of three runs of CALLS
calls.  For the two grids also the wall time of phd_blur_vector_maps_device, which
forms the grid itself.  Once per workload every window's vectors and fft_max of
the two entries are compared.  Prints one JSON line per workload."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.set_device(0)
from photohive_dsp_amd.core import WINDOW_DEFAULTS, make_config, window_boundaries, window_grid
from photohive_dsp_amd.lib import WINDOW_BLUR_KERNEL, WINDOW_VECTORS_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Crop_Boundaries, PhdWindowBlur

H, W, N = 3000, 4000, int(os.environ.get("WIN_BENCH_IMAGES", "64"))
CALLS = int(os.environ.get("WIN_BENCH_CALLS", "4"))
cfg = make_config(**WINDOW_DEFAULTS)


def eight(seed, T):
    rng = np.random.default_rng(seed)
    return [(t, t + T, l, l + T) for t, l in zip(rng.integers(0, H - T + 1, 8).tolist(),
                                                  rng.integers(0, W - T + 1, 8).tolist())]


SETS = [("full_grid_128", 128, [window_grid(H, W, 128)[0]] * N, True),
        ("full_grid_64", 64, [window_grid(H, W, 64)[0]] * N, True),
        ("8_windows_128", 128, [eight(300 + i, 128) for i in range(N)], False)]


def read(bit):
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    assert lib.phd_profile_read(bit, ctypes.byref(tot), ctypes.byref(cnt)) == 0
    return tot.value, cnt.value


def timed(call, bit):
    """Three runs of CALLS calls: (median kernel us per call, the runs, launches per call, median wall ms)."""
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
    return statistics.median(us), us, launches, statistics.median(wall)


imgs = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
for i in range(N):
    assert lib.phd_fill_structured_device(imgs[i].data_ptr(), H, W, 500 + i, 0, 1, None) == 0, last_error()
torch.cuda.synchronize()
ptrs = (ctypes.c_void_p * N)(*[imgs[i].data_ptr() for i in range(N)])
hs, ws = (ctypes.c_int * N)(*[H] * N), (ctypes.c_int * N)(*[W] * N)

for name, T, lists, is_grid in SETS:
    keep = [window_boundaries(b) for b in lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * N)(*[ctypes.pointer(k) for k in keep])
    per = [len(b) for b in lists]
    windows = sum(per)
    wb = (PhdWindowBlur * N)()
    vec = [torch.empty((n, 10, 2), dtype=torch.int32, device="cuda") for n in per]
    fmax = [torch.empty((n,), dtype=torch.float64, device="cuda") for n in per]
    pv = (ctypes.c_void_p * N)(*[v.data_ptr() for v in vec])
    pf = (ctypes.c_void_p * N)(*[f.data_ptr() for f in fmax])
    torch.cuda.synchronize()

    def old():
        assert lib.phd_blur_windows_device(ptrs, hs, ws, N, arr, T, ctypes.byref(cfg), wb, None) == 0, last_error()
        lib.phd_free_window_blur(wb, N)

    def new():
        assert lib.phd_blur_vectors_device(ptrs, hs, ws, N, arr, T, ctypes.byref(cfg), pv, pf, None) == 0, last_error()

    def maps():
        assert lib.phd_blur_vector_maps_device(ptrs, hs, ws, N, T, T, ctypes.byref(cfg), pv, pf, None) == 0, last_error()

    # once: both entries' values on every window
    assert lib.phd_blur_windows_device(ptrs, hs, ws, N, arr, T, ctypes.byref(cfg), wb, None) == 0, last_error()
    new()
    differ = fmax_differ = 0
    for i in range(N):
        n = per[i]
        a = np.ctypeslib.as_array(ctypes.cast(wb[i].vectors, ctypes.POINTER(ctypes.c_int32)), shape=(n, 10, 2))
        differ += int(np.count_nonzero((vec[i].cpu().numpy() != a).any(axis=(1, 2))))
        f = np.ctypeslib.as_array(wb[i].fft_max, shape=(n,))
        fmax_differ += int(np.count_nonzero(fmax[i].cpu().numpy().view(np.uint64) != f.view(np.uint64)))
    lib.phd_free_window_blur(wb, N)

    k_old, runs_old, launches_old, wall_old = timed(old, WINDOW_BLUR_KERNEL)
    k_new, runs_new, launches_new, wall_new = timed(new, WINDOW_VECTORS_KERNEL)
    row = {"windows": name, "T": T, "images": N, "windows_in_call": windows,
           "k_window_blur_us_per_call": round(k_old, 1), "k_window_blur_us_runs": [round(u, 1) for u in runs_old],
           "k_window_blur_launches": launches_old,
           "k_window_vectors_us_per_call": round(k_new, 1), "k_window_vectors_us_runs": [round(u, 1) for u in runs_new],
           "k_window_vectors_launches": launches_new, "kernel_ratio": round(k_new / k_old, 3),
           "blur_windows_call_wall_ms": round(wall_old, 2), "blur_vectors_call_wall_ms": round(wall_new, 2),
           "call_ratio": round(wall_new / wall_old, 4),
           "host_side_ms_removed": round(wall_old - k_old / 1e3, 2), "kernel_ms_added": round((k_new - k_old) / 1e3, 3),
           "windows_whose_vectors_differ": differ, "windows_whose_fft_max_differs": fmax_differ}
    if is_grid:
        row["blur_vector_maps_call_wall_ms"] = round(timed(maps, WINDOW_VECTORS_KERNEL)[3], 2)
    print(json.dumps(row), flush=True)
