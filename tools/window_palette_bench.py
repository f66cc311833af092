"""The palette map entries beside the box palette entry, one process.

Section 25's workload -- 64 structured images of 4000 x 3000 on the device, here
their label maps from reports_device_labels -- with the full grids at T = 16, 32,
64 and 128 (stride T), T = 64 at stride 32 and 8 windows of 64 per map, through
phd_palette_maps_device / phd_palette_windows_device (counts and dominant labels
left on the device, one launch, profile slot 18) and through
phd_box_palettes_device (the box entry: counts to the host, a memset, one launch
of global atomics -- profile slot 11 --, a download and a copy per map) on the same
window lists: kernel microseconds per call and the wall time of the whole call
(the box entry's with phd_free_box_palettes), the median of three runs of CALLS
calls after a warm-up call, with the runs themselves.  The byte bound is 2 T^2
bytes read plus 4 (n_slots + 1) + 2 written per window at the HBM peak of 8 TB/s.
Once per workload every counter of every window of the two entries is compared:
the number of differing integers.  Two more workloads repeat the full grids at 64
and 16 on maps of one label (every lane of a wave on one counter: what the copies
are for), the new entry alone, its counts checked to be T^2 in column 0.  Prints
one JSON line per workload.
WIN_BENCH_SETS=name,name limits the workloads; WIN_BENCH_NO_BOX=1 leaves the box
entry out."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
torch.cuda.set_device(0)
import photohive_dsp_amd as phd
from photohive_dsp_amd.core import _take_box_palettes, window_boundaries, window_grid
from photohive_dsp_amd.lib import BOX_PALETTES_KERNEL, WINDOW_PALETTE_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Crop_Boundaries, PhdBoxPalette

H, W, N = 3000, 4000, int(os.environ.get("WIN_BENCH_IMAGES", "64"))
CALLS = int(os.environ.get("WIN_BENCH_CALLS", "4"))
NO_BOX = os.environ.get("WIN_BENCH_NO_BOX") == "1"
HBM_PEAK = 8.0e12


def eight(seed, T):
    rng = np.random.default_rng(seed)
    return [(t, t + T, l, l + T) for t, l in zip(rng.integers(0, H - T + 1, 8).tolist(),
                                                  rng.integers(0, W - T + 1, 8).tolist())]


# (name, T, stride of the grid or None, per-map window lists, maps of one label)
SETS = [(f"full_grid_{T}", T, T, None, False) for T in (16, 32, 64, 128)] + \
       [("grid_64_stride_32", 64, 32, None, False),
        ("8_windows_64", 64, None, [eight(300 + i, 64) for i in range(N)], False),
        ("full_grid_64_single_label", 64, 64, None, True), ("full_grid_16_single_label", 16, 16, None, True)]
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


# the label maps: the images are made, reported and dropped eight at a time
maps, slots = [], []
for i0 in range(0, N, 8):
    k = min(8, N - i0)
    imgs = torch.empty((k, H, W, 3), dtype=torch.uint8, device="cuda")
    for j in range(k):
        assert lib.phd_fill_structured_device(imgs[j].data_ptr(), H, W, 500 + i0 + j, 0, 1, None) == 0, last_error()
    torch.cuda.synchronize()
    reps, labs = phd.reports_device_labels(imgs)
    maps += labs
    slots += [len(r.color_palette.quantities) for r in reps]
    del imgs, reps
torch.cuda.synchronize()
assert all(tuple(m.shape) == (H, W) for m in maps)
real_ptrs = (ctypes.c_void_p * N)(*[m.data_ptr() for m in maps])
flat = torch.zeros((H, W), dtype=torch.int16, device="cuda")            # every element in slot 0
flat_ptrs = (ctypes.c_void_p * N)(*[flat.data_ptr()] * N)
hs, ws = (ctypes.c_int * N)(*[H] * N), (ctypes.c_int * N)(*[W] * N)
ns = (ctypes.c_int * N)(*slots)
print(json.dumps({"maps": N, "n_slots_min": min(slots), "n_slots_max": max(slots),
                  "n_slots_mean": round(sum(slots) / N, 1)}), flush=True)

for name, T, stride, lists, single in SETS:
    ptrs = flat_ptrs if single else real_ptrs
    if lists is None:
        one = window_boundaries(window_grid(H, W, T, stride)[0])
        keep = [one] * N                                         # every map: the same grid
    else:
        keep = [window_boundaries(b) for b in lists]
    arr = (ctypes.POINTER(Crop_Boundaries) * N)(*[ctypes.pointer(k) for k in keep])
    per = [int(k.N) for k in keep]
    windows = sum(per)
    counts = [torch.empty((n, s + 1), dtype=torch.int32, device="cuda") for n, s in zip(per, slots)]
    dom = [torch.empty((n,), dtype=torch.int16, device="cuda") for n in per]
    pc = (ctypes.c_void_p * N)(*[t.data_ptr() for t in counts])
    pd = (ctypes.c_void_p * N)(*[t.data_ptr() for t in dom])
    bp = (PhdBoxPalette * N)()
    torch.cuda.synchronize()

    def old():
        assert lib.phd_box_palettes_device(ptrs, hs, ws, N, ns, arr, bp, None) == 0, last_error()
        lib.phd_free_box_palettes(bp, N)

    def new_lists():
        assert lib.phd_palette_windows_device(ptrs, hs, ws, N, ns, arr, T, pc, pd, None) == 0, last_error()

    def new_maps():
        assert lib.phd_palette_maps_device(ptrs, hs, ws, N, ns, T, stride, pc, pd, None) == 0, last_error()

    new = new_maps if stride else new_lists
    new()
    k_new, runs_new, launches_new, wall_new, walls_new = timed(new, WINDOW_PALETTE_KERNEL)
    bytes_moved = sum(n * (2.0 * T * T + 4.0 * (s + 1) + 2.0) for n, s in zip(per, slots))
    bound_us = bytes_moved / HBM_PEAK * 1e6
    row = {"windows": name, "T": T, "stride": stride, "maps": N, "windows_in_call": windows,
           "k_window_palette_us_per_call": round(k_new, 1),
           "k_window_palette_us_runs": [round(u, 1) for u in runs_new], "k_window_palette_launches": launches_new,
           "map_call_wall_ms" if stride else "list_call_wall_ms": round(wall_new, 3),
           "new_call_wall_ms_runs": [round(x, 3) for x in walls_new],
           "byte_bound_us_at_8TBps": round(bound_us, 1), "kernel_over_byte_bound": round(k_new / bound_us, 2),
           "kernel_GBps": round(bytes_moved / (k_new * 1e-6) / 1e9, 1)}
    if stride:
        row["list_call_wall_ms"] = round(timed(new_lists, WINDOW_PALETTE_KERNEL)[3], 3)
    if single:
        ok = all(bool((t[:, 0] == T * T).all()) and bool((d == 0).all()) for t, d, k in zip(counts, dom, slots) if k > 0)
        row["every_window_T2_in_column_0_and_dominant_0"] = ok
    elif not NO_BOX:
        # once: every counter of both entries on every window
        assert lib.phd_box_palettes_device(ptrs, hs, ws, N, ns, arr, bp, None) == 0, last_error()
        differing = 0
        for a, t in zip(_take_box_palettes(bp, N), counts):
            differing += int((a != t.cpu().numpy().view(np.uint32)).sum())
        row["differing_integers_of_the_two_entries"] = differing
        k_old, runs_old, launches_old, wall_old, walls_old = timed(old, BOX_PALETTES_KERNEL)
        row.update({"k_box_counts_us_per_call": round(k_old, 1),
                    "k_box_counts_us_runs": [round(u, 1) for u in runs_old],
                    "k_box_counts_launches": launches_old, "kernel_ratio": round(k_new / k_old, 4),
                    "box_call_wall_ms": round(wall_old, 3), "box_call_wall_ms_runs": [round(x, 3) for x in walls_old],
                    "call_ratio": round(wall_new / wall_old, 4)})
    print(json.dumps(row), flush=True)
    del counts, dom
