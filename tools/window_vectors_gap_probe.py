"""k_window_vectors' microseconds (profile slot 15) through the list entry, the maps entry, and the list
entry with GAP_MS of host idling before every call, for the library PHD_LIB names: whether the kernel's
time follows the host time spent before the launch.  One JSON line per grid."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
torch.cuda.set_device(0)
from photohive_dsp_amd.core import WINDOW_DEFAULTS, make_config, window_boundaries, window_grid
from photohive_dsp_amd.lib import WINDOW_VECTORS_KERNEL, last_error, lib
from photohive_dsp_amd.structures import Crop_Boundaries

H, W, N, CALLS = 3000, 4000, 64, 4
GAP = float(os.environ.get("GAP_MS", "15")) / 1e3
cfg = make_config(**WINDOW_DEFAULTS)


def timed(call, gap=0.0):
    call()
    us, wall = [], []
    for _ in range(3):
        assert lib.phd_profile_kernels(1 << WINDOW_VECTORS_KERNEL) == 0
        t0 = time.perf_counter()
        for _ in range(CALLS):
            if gap:
                time.sleep(gap)
            call()
        wall.append((time.perf_counter() - t0) / CALLS * 1e3 - gap * 1e3)
        tot, cnt = ctypes.c_double(), ctypes.c_long()
        assert lib.phd_profile_read(WINDOW_VECTORS_KERNEL, ctypes.byref(tot), ctypes.byref(cnt)) == 0
        lib.phd_profile_kernels(0)
        assert cnt.value == CALLS
        us.append(tot.value / CALLS * 1e3)
    return {"kernel_us": round(statistics.median(us), 1), "kernel_us_runs": [round(u, 1) for u in us],
            "wall_ms": round(statistics.median(wall), 2)}


imgs = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
for i in range(N):
    assert lib.phd_fill_structured_device(imgs[i].data_ptr(), H, W, 500 + i, 0, 1, None) == 0, last_error()
torch.cuda.synchronize()
ptrs = (ctypes.c_void_p * N)(*[imgs[i].data_ptr() for i in range(N)])
hs, ws = (ctypes.c_int * N)(*[H] * N), (ctypes.c_int * N)(*[W] * N)
for T in (128, 64):
    one = window_boundaries(window_grid(H, W, T)[0])
    arr = (ctypes.POINTER(Crop_Boundaries) * N)(*[ctypes.pointer(one)] * N)
    n = int(one.N)
    vec = [torch.empty((n, 10, 2), dtype=torch.int32, device="cuda") for _ in range(N)]
    fmax = [torch.empty((n,), dtype=torch.float64, device="cuda") for _ in range(N)]
    pv = (ctypes.c_void_p * N)(*[v.data_ptr() for v in vec])
    pf = (ctypes.c_void_p * N)(*[f.data_ptr() for f in fmax])
    torch.cuda.synchronize()

    def lists():
        assert lib.phd_blur_vectors_device(ptrs, hs, ws, N, arr, T, ctypes.byref(cfg), pv, pf, None) == 0, last_error()

    def maps():
        assert lib.phd_blur_vector_maps_device(ptrs, hs, ws, N, T, T, ctypes.byref(cfg), pv, pf, None) == 0, last_error()

    print(json.dumps({"T": T, "windows_in_call": n * N, "list_entry": timed(lists), "maps_entry": timed(maps),
                      "list_entry_after_host_gap": timed(lists, GAP), "maps_entry_after_host_gap": timed(maps, GAP),
                      "gap_ms": GAP * 1e3}), flush=True)
