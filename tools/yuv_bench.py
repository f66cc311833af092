"""Cost of the YCbCr input stage's kernel on one 4000 x 3000 frame, at the
C-ABI, one process.

k_yuv_views alone, from profile bit 9's event times around
phd_convert_yuv_device: NV12 with replicated chroma, NV12 with the triangle
filter, I420 and YUY2 (replicated), next to k_pack_views (bit 6) on a uint8
CHW image of the same size in the same process -- the existing kernel nearest
in bytes moved.  Microseconds per launch (the median of three runs of CALLS
launches), the algorithmic bytes (source samples read once + 3 bytes per pixel
written) per second and their share of the 8 TB/s HBM peak.

Prints one JSON line per figure."""
import ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
torch.cuda.set_device(0)
from photohive_dsp_amd.core import make_views, make_yuv_views, nv12_planes
from photohive_dsp_amd.lib import PACK_VIEWS_KERNEL, YUV_VIEWS_KERNEL, last_error, lib
from photohive_dsp_amd.structures import PhdYuvView

H, W = 3000, 4000
CALLS = int(os.environ.get("YUV_BENCH_CALLS", "20"))
HBM_PEAK = 8e12
NPIX = H * W

g = torch.Generator().manual_seed(7)
surface = torch.randint(0, 256, (H + H // 2, W), dtype=torch.uint8, generator=g).cuda()
planes = [torch.randint(0, 256, s, dtype=torch.uint8, generator=g).cuda()
          for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]
quads = torch.randint(0, 256, (H, W // 2, 4), dtype=torch.uint8, generator=g).cuda()
chw = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g).cuda()
dst = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
d_ptr = (ctypes.c_void_p * 1)(dst.data_ptr())
torch.cuda.synchronize()

p = quads.data_ptr()
v_yuy2 = (PhdYuvView * 1)(PhdYuvView(p, p + 1, p + 3, H, W, 2 * W, 2, 2 * W, 4, 1, 0, 0, 0, 0))
v_chw, _ = make_views([chw], "CHW")


def convert(views):
    assert lib.phd_convert_yuv_device(views, 1, d_ptr, None) == 0, last_error()


def pack():
    assert lib.phd_pack_views_device(v_chw, 1, d_ptr, None) == 0, last_error()


def profiled(bit, fn, n):
    """(microseconds per launch, launches) of kernel `bit` over n calls of fn"""
    assert lib.phd_profile_kernels(1 << bit) == 0
    for _ in range(n):
        fn()
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    lib.phd_profile_read(bit, ctypes.byref(tot), ctypes.byref(cnt))
    lib.phd_profile_kernels(0)
    return tot.value * 1e3 / max(1, cnt.value), cnt.value


nv12 = nv12_planes(surface, H, W)
figures = [("yuv_views", "NV12 replicate", YUV_VIEWS_KERNEL, make_yuv_views([nv12])[0], NPIX * 1.5),
           ("yuv_views", "NV12 triangle", YUV_VIEWS_KERNEL, make_yuv_views([nv12], chroma="triangle")[0], NPIX * 1.5),
           ("yuv_views", "I420 replicate", YUV_VIEWS_KERNEL, make_yuv_views([tuple(planes)])[0], NPIX * 1.5),
           ("yuv_views", "YUY2 replicate", YUV_VIEWS_KERNEL, v_yuy2, NPIX * 2.0),
           ("pack_views", "u8 CHW", PACK_VIEWS_KERNEL, None, NPIX * 3.0)]
for kernel, source, bit, views, src_bytes in figures:
    fn = pack if views is None else (lambda v=views: convert(v))
    fn()
    runs = [profiled(bit, fn, CALLS) for _ in range(3)]
    us = statistics.median(r[0] for r in runs)
    nbytes = src_bytes + 3.0 * NPIX
    print(json.dumps({"kernel": kernel, "source": source, "us_per_launch": round(us, 2),
                      "us_runs": [round(r[0], 2) for r in runs], "launches": runs[0][1], "MB": nbytes / 1e6,
                      "TBps": round(nbytes / us / 1e6, 3), "of_hbm_peak": round(nbytes / us * 1e6 / HBM_PEAK, 3)}),
          flush=True)
