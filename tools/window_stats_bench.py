"""The statistics map entries beside the box statistics entry, one process.

Section 25's workload -- 64 structured images of 4000 x 3000 on the device -- with
the full grids at T = 16, 32, 64 and 128 (stride T), T = 64 at stride 32 and 8
windows of 64 per image, through phd_stats_maps_device / phd_stats_windows_device
(values left on the device, one launch, profile slot 17) and through
phd_box_stats_device (the box entry: values to the host, a memset, two launches --
profile slot 12 brackets the first --, a download and a host finish) on the same
window lists: kernel microseconds per call and the wall time of the whole call
(the box entry's with phd_free_box_stats), the median of three runs of CALLS calls
after a warm-up call, with the runs themselves.  The byte bound is 3 T^2 bytes
read plus 56 written per window at the HBM peak of 8 TB/s.  Once per workload
every window's seven values of the two entries are compared: the worst absolute
difference per output.  Prints one JSON line per workload.
WIN_BENCH_SETS=name,name limits the workloads; WIN_BENCH_NO_BOX=1 leaves the box
entry out."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.set_device(0)
from photohive_dsp_amd.core import _take_box_stats, window_boundaries, window_grid
from photohive_dsp_amd.lib import BOX_STATS_KERNEL, WINDOW_STATS_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Crop_Boundaries, PhdBoxStats

H, W, N = 3000, 4000, int(os.environ.get("WIN_BENCH_IMAGES", "64"))
CALLS = int(os.environ.get("WIN_BENCH_CALLS", "4"))
NO_BOX = os.environ.get("WIN_BENCH_NO_BOX") == "1"
HBM_PEAK = 8.0e12
NAMES = ("Br", "Bg", "Bb", "Cr", "Cg", "Cb", "S_bar")


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
    stats = [torch.empty((n, 7), dtype=torch.float64, device="cuda") for n in per]
    ps = (ctypes.c_void_p * N)(*[t.data_ptr() for t in stats])
    bs = (PhdBoxStats * N)()
    torch.cuda.synchronize()

    def old():
        assert lib.phd_box_stats_device(ptrs, hs, ws, N, arr, bs, None) == 0, last_error()
        lib.phd_free_box_stats(bs, N)

    def new_lists():
        assert lib.phd_stats_windows_device(ptrs, hs, ws, N, arr, T, ps, None) == 0, last_error()

    def new_maps():
        assert lib.phd_stats_maps_device(ptrs, hs, ws, N, T, stride, ps, None) == 0, last_error()

    new = new_maps if stride else new_lists
    new()
    k_new, runs_new, launches_new, wall_new, walls_new = timed(new, WINDOW_STATS_KERNEL)
    bytes_moved = windows * (3.0 * T * T + 56.0)
    bound_us = bytes_moved / HBM_PEAK * 1e6
    row = {"windows": name, "T": T, "stride": stride, "images": N, "windows_in_call": windows,
           "k_window_stats_us_per_call": round(k_new, 1), "k_window_stats_us_runs": [round(u, 1) for u in runs_new],
           "k_window_stats_launches": launches_new,
           "map_call_wall_ms" if stride else "list_call_wall_ms": round(wall_new, 3),
           "new_call_wall_ms_runs": [round(x, 3) for x in walls_new],
           "byte_bound_us_at_8TBps": round(bound_us, 1), "kernel_over_byte_bound": round(k_new / bound_us, 2),
           "kernel_GBps": round(bytes_moved / (k_new * 1e-6) / 1e9, 1)}
    if stride:
        row["list_call_wall_ms"] = round(timed(new_lists, WINDOW_STATS_KERNEL)[3], 3)
    if not NO_BOX:
        # once: the seven values of both entries on every window
        assert lib.phd_box_stats_device(ptrs, hs, ws, N, arr, bs, None) == 0, last_error()
        a = np.concatenate(_take_box_stats(bs, N))
        b = np.concatenate([t.cpu().numpy() for t in stats])
        diff = np.abs(a - b).max(axis=0)
        row["worst_absolute_difference_of_the_two_entries"] = dict(zip(NAMES, [float(d) for d in diff]))
        row["windows_with_any_differing_bit"] = int((a.view(np.int64) != b.view(np.int64)).any(axis=1).sum())
        k_old, runs_old, launches_old, wall_old, walls_old = timed(old, BOX_STATS_KERNEL)
        row.update({"k_box_stats_us_per_call": round(k_old, 1), "k_box_stats_us_runs": [round(u, 1) for u in runs_old],
                    "k_box_stats_launches": launches_old, "kernel_ratio": round(k_new / k_old, 4),
                    "box_call_wall_ms": round(wall_old, 3), "box_call_wall_ms_runs": [round(x, 3) for x in walls_old],
                    "call_ratio": round(wall_new / wall_old, 4)})
    print(json.dumps(row), flush=True)
    del stats
