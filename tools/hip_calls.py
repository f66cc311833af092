"""The HIP API names of one plain device batch call, for comparing two builds
of the library (profiles/labels/hip_calls_*.txt).

    PHD_LIB=<library> rocprofv3 --hip-trace --output-format csv -d DIR -- python tools/hip_calls.py run
    python tools/hip_calls.py list DIR > hip_calls_<build>.txt
    (`buffers` for `run`: the calls of profiles/buffers/, below)

run: one process, no torch: four 401 x 577 device images (filled by
phd_fill_uniform_device) through phd_report_batch_device twice, then
phd_shutdown.  list: the calls of the trace under DIR in start order, per
thread (threads in order of their first call), names only, without the
compiler-generated registration calls a library makes when it is loaded.

buffers: four 3000 x 4000 device images through phd_report_batch_device twice
(the headline's call; the second grows nothing), phd_box_stats_device with one
box, then 72 (both blocks of its pair regrow), then one again, and
phd_pack_views_device with one 8 x 8 planar view, then 128, then one, then
phd_shutdown."""
import csv, ctypes, glob, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run():
    from photohive_dsp_amd.core import make_config
    from photohive_dsp_amd.lib import last_error, lib
    from photohive_dsp_amd.structures import Full_Report_Data
    hip = ctypes.CDLL(None)                      # the runtime the library loaded
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    h, w, n = 401, 577, 4
    d = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d), n * h * w * 3) == 0
    assert lib.phd_fill_uniform_device(d, n * h * w * 3, 1, None) == 0, last_error()
    cfg = make_config()
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    for _ in range(2):
        assert lib.phd_report_batch_device(d, n, h, w, 0, ctypes.byref(cfg), outs, st, None) == 0, last_error()
        lib.phd_free_reports(outs, n)
    lib.phd_shutdown()


def listing(root):
    rows = []
    for path in glob.glob(os.path.join(root, "**", "*hip_api_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    # the runtime API only: not the code objects' registration at load (__hipRegisterFatBinary,
    # __hipRegisterFunction: one per .hip file and kernel of the build, before any call)
    rows = [r for r in rows if not r["Function"].startswith("__hip")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    threads = {}
    for r in rows:
        threads.setdefault(r["Thread_Id"], []).append(r["Function"])
    print(f"# {len(rows)} calls, {len(threads)} threads")
    for k, names in enumerate(threads.values()):
        print(f"## thread {k}: {len(names)} calls")
        print("\n".join(names))


def buffers():
    from photohive_dsp_amd.core import make_config, set_bounding_boxes
    from photohive_dsp_amd.lib import last_error, lib
    from photohive_dsp_amd.structures import Crop_Boundaries, Full_Report_Data, PhdBoxStats, PhdImageView
    hip = ctypes.CDLL(None)
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    h, w, n = 3000, 4000, 4
    d = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d), n * h * w * 3) == 0
    assert lib.phd_fill_uniform_device(d, n * h * w * 3, 1, None) == 0, last_error()
    cfg = make_config()
    outs = (ctypes.POINTER(Full_Report_Data) * n)()
    st = (ctypes.c_int * n)()
    for _ in range(2):
        assert lib.phd_report_batch_device(d, n, h, w, 0, ctypes.byref(cfg), outs, st, None) == 0, last_error()
        lib.phd_free_reports(outs, n)
    for nb in (1, 72, 1):
        cb = set_bounding_boxes([dict(top=k, bottom=k + 40, left=3 + k, right=28 + 2 * k) for k in range(nb)])
        bs = (PhdBoxStats * 1)()
        rc = lib.phd_box_stats_device((ctypes.c_void_p * 1)(d.value + 1), (ctypes.c_int * 1)(h), (ctypes.c_int * 1)(w),
                                      1, (ctypes.POINTER(Crop_Boundaries) * 1)(ctypes.pointer(cb)), bs, None)
        assert rc == 0 and bs[0].n_boxes == nb, last_error()
        lib.phd_free_box_stats(bs, 1)
    dst = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dst), 128 * 192) == 0
    for nv in (1, 128, 1):
        views = (PhdImageView * nv)(*[PhdImageView(d.value + 192 * k, 8, 8, 8, 1, 64) for k in range(nv)])
        dsts = (ctypes.c_void_p * nv)(*[dst.value + 192 * k for k in range(nv)])
        assert lib.phd_pack_views_device(views, nv, dsts, None) == 0, last_error()
    lib.phd_shutdown()


if __name__ == "__main__":
    {"run": run, "buffers": buffers}[sys.argv[1]]() if len(sys.argv) == 2 else listing(sys.argv[2])
