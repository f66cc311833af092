"""The HIP API names of one plain device batch call, for comparing two builds
of the library (profiles/labels/hip_calls_*.txt).

    PHD_LIB=<library> rocprofv3 --hip-trace --output-format csv -d DIR -- python tools/hip_calls.py run
    python tools/hip_calls.py list DIR > hip_calls_<build>.txt

run: one process, no torch: four 401 x 577 device images (filled by
phd_fill_uniform_device) through phd_report_batch_device twice, then
phd_shutdown.  list: the calls of the trace under DIR in start order, per
thread (threads in order of their first call), names only, without the
compiler-generated registration calls a library makes when it is loaded."""
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


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else listing(sys.argv[2])
