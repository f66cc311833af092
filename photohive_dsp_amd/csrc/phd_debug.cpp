// phd_debug.cpp -- the exported defaults, fills, parity traces and
// micro-benchmark hooks (tests and tools; no production caller).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "phd_host.h"

using namespace phd;

extern "C" void phd_config_default(phd_config* c) {
    // get_report defaults, /root/reference/core.py:442-448
    c->h_partitions = 18;
    c->s_partitions = 2;
    c->v_partitions = 3;
    c->black_thresh = 0.1;
    c->gray_thresh = 0.1;
    c->coverage_thresh = 0.95;
    c->linked_list_size = 1000;
    c->downsample_rate = 1;
    c->radius_partitions = 40;
    c->angle_partitions = 72;
    c->quantity_weight = 0.1f;
    c->saturation_value_weight = 0.9f;
    c->fft_streak_thresh = 1.20;
    c->magnitude_thresh = 0.3;
    c->blur_cutoff_ratio_denom = 2;
}

extern "C" int phd_palette_trace_device(const uint8_t* d_rgb, int height, int width, const phd_config* cfg,
                                        int* hist, int* parents, int* kept, int* n_parents) {
    clear_error();
    Context* c = get_context();
    if (!c || !cfg) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    std::vector<unsigned> h;
    PaletteDecision dec;
    std::vector<double> dcount;
    if (!run_palette_trace(c, d_rgb, height, width, *cfg, &h, &dec, &dcount)) return -1;
    const int np = (int)dec.parents.size();
    for (size_t g = 0; g < h.size(); g++) hist[g] = (int)h[g];
    for (int k = 0; k < np; k++) {
        parents[k] = dec.parents[k];
        kept[k] = (int)dcount[k];     // what the device actually summed
    }
    *n_parents = np;
    for (int k = 0; k < np; k++)
        if (dcount[k] != (double)dec.kept[k]) {
            set_error("device kept count differs from the host keep rules");
            return -2;
        }
    return (int)h.size();
}

extern "C" int phd_blur_counts(int height, int width, int radius_partitions, int angle_partitions,
                               long long* counts) {
    clear_error();
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const BlurTable* tb = get_table(c, height, width, radius_partitions, angle_partitions);
    if (!tb) return -1;
    memcpy(counts, tb->counts.data(), sizeof(long long) * tb->counts.size());
    return 0;
}

extern "C" int phd_fill_uniform_device(uint8_t* d_dst, size_t n, uint64_t seed, void* stream) {
    clear_error();
    Context* c = get_context();
    if (!c) return -1;
    hipStream_t st = work_stream(c, stream);
    if (launch_fill_uniform(d_dst, n, seed, st) != hipSuccess) {
        set_error("fill kernel launch failed");
        return -1;
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
        set_error("fill kernel failed");
        return -1;
    }
    return 0;
}

extern "C" int phd_fill_structured_device(uint8_t* d_dst, int height, int width, uint64_t seed, int blur,
                                          int blur_axis, void* stream) {
    clear_error();
    Context* c = get_context();
    if (!c || !d_dst || height < 1 || width < 1 || blur < 0 || (blur_axis != 0 && blur_axis != 1)) return -1;
    hipStream_t st = work_stream(c, stream);
    if (launch_fill_structured(d_dst, height, width, seed, blur, blur_axis, st) != hipSuccess) {
        set_error("structured fill kernel launch failed");
        return -1;
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
        set_error("structured fill kernel failed");
        return -1;
    }
    return 0;
}

extern "C" int phd_debug_hsv_groups_device(const uint8_t* d_rgb, long n_pixels, const phd_config* cfg, int* d_gid,
                                           double* d_hsv) {
    clear_error();
    Context* c = get_context();
    if (!c || !cfg) return -1;
    std::string why;
    if (!validate_config(*cfg, &why)) {
        set_error(why);
        return -1;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    const GridParams gp = make_grid(*cfg);
    const Context::Cls* cls = get_cls(c, gp);
    if (!cls) return -1;
    if (launch_debug_hsv(d_rgb, n_pixels, gp, cls->fc, cls->d, c->d_k255, d_gid, d_hsv, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        set_error("debug hsv kernel failed");
        return -1;
    }
    return 0;
}

// K1's per-pixel logic on the host, no GPU (tests/test_k1_pixel.py): for n
// interleaved RGB8 pixels the hue cell (HueCells layout), h, s and the
// deferred flag exactly as k1.hip classifies them.
extern "C" int phd_debug_k1_pixels(const uint8_t* rgb, long n, const phd_config* cfg, int* cell, double* h,
                                   double* s, int* deferred) {
    clear_error();
    if (!rgb || !cfg || !cell || !h || !s || n < 0) return -1;
    std::string why;
    if (!validate_config(*cfg, &why)) {
        set_error(why);
        return -1;
    }
    const GridParams gp = make_grid(*cfg);
    FastCls fc;
    std::unique_ptr<ClassTables> t(new ClassTables());
    make_class_tables(gp, &fc, t.get());
    if (k1_host_pixels(gp, *t, rgb, n, cell, h, s, deferred) != 0) {
        set_error("phd_debug_k1_pixels: this grid has no K1 code table");
        return -1;
    }
    return 0;
}

// Which palette kernels a full-resolution report of this configuration runs,
// from the functions run_reports itself asks (no device; tests/palette_grids.py).
extern "C" int phd_debug_palette_path(const phd_config* cfg, int max_slots) {
    clear_error();
    std::string why;
    if (!cfg || !validate_config(*cfg, &why)) {
        set_error(cfg ? why : "phd_debug_palette_path: no configuration");
        return -1;
    }
    const GridParams gp = make_grid(*cfg);
    FastCls fc;
    std::unique_ptr<ClassTables> t(new ClassTables());
    make_class_tables(gp, &fc, t.get());
    const bool fused = fused_palette_ok(gp);
    return (fused ? 1 : 0) | (fc.k1t_cshift >= 0 ? 2 : 0) | (fc.k1t_cshift2 >= 0 ? 4 : 0) | (fc.use_thr ? 8 : 0) |
           (t->codes_ok ? 16 : 0) | (palette_tail_batched(gp, 1, fused, max_slots) ? 32 : 0);
}

// One untimed full report of a device image: sets up the pipeline's buffers for
// its size and leaves K1's channel sums at the start of the workspace.
static bool report_once(Context* c, const uint8_t* d_rgb, int height, int width, const phd_config& cfg) {
    Full_Report_Data* r = nullptr;
    int st = -1;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!run_reports(c, &d_rgb, 1, height, width, cfg, nullptr, &r, &st, nullptr)) return false;
    free_full_report(&r);
    return true;
}

// phd_debug_time_kernel's id of K1 without the group histogram (not a profiler slot)
static constexpr int kTimeStatsPass = 6;

// Micro-benchmark hook: launch one pipeline kernel `iters` times on a device
// image (after one untimed full report to set up its inputs) and return the
// average launch time in ms from HIP events.  `ablate` is a debug mask read by
// the kernel to skip parts of its work (0 = the production kernel).
extern "C" int phd_debug_time_kernel(int kernel, const uint8_t* d_rgb, int height, int width, const phd_config* cfg,
                                     int ablate, int iters, double* avg_ms) {
    clear_error();
    Context* c = get_context();
    if (!c || !cfg || iters <= 0) return -1;
    if (!report_once(c, d_rgb, height, width, *cfg)) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const GridParams gp = make_grid(*cfg);
    const int ds = cfg->downsample_rate > 1 ? cfg->downsample_rate : 1;
    const long n_hsv = hsv_count(height, width, ds);
    const int nchunks = (int)((n_hsv + kChunk - 1) / kChunk);
    const Context::Cls* cls = get_cls(c, gp);
    const int wf = width / 2 + 1;
    const BlurTable* tbl = get_table(c, height, width, cfg->radius_partitions, cfg->angle_partitions);
    FftSel fs;
    if (!cls || !tbl || !select_fft(c, height, width, cfg->radius_partitions * cfg->angle_partitions, &d_rgb, 1, &fs, tbl))
        return -1;
    // scratch outputs in the (large enough) workspace of the report just run
    uint8_t* dw = c->dev[kDevWs].as<uint8_t>();
    double2* const inter = c->dev[kDevInter].as<double2>();
    PaletteDev pd;
    pd.sums = (unsigned long long*)dw;
    pd.hist = (unsigned*)(dw + 256);
    pd.s_part = (double*)(dw + 256 + 4 * 4096);
    pd.chunk_hist = (unsigned short*)(dw + 256 + 4 * 4096 + 8 * (size_t)nchunks);
    // K1 is timed as the report runs it: fused when the report fuses
    const bool fused = ds <= 1 && fused_palette_ok(gp);
    void* fscratch = nullptr;
    if (fused || kernel == kTimeStatsPass) {
        // the fused K1's group sums and cell counts; the statistics pass's sums of d
        if (hipMalloc(&fscratch, sizeof(double) * 3 * gp.tl + sizeof(unsigned) * HueCells::count(gp) +
                                     256 * sizeof(unsigned long long)) != hipSuccess)
            return -1;
        pd.kd_sum = (unsigned long long*)fscratch;
        pd.gsum = (double*)fscratch + 256;
        pd.gcell = (unsigned*)((double*)fscratch + 256 + 3 * gp.tl);
    }
    struct FreeOnExit {
        void* p;
        ~FreeOnExit() { if (p) (void)hipFree(p); }
    } free_scratch{fscratch};
    // the column pass's bins and per-block max partials: a buffer of their own
    // (a small image's workspace is smaller than a persistent grid's partials)
    const int nbins = cfg->radius_partitions * cfg->angle_partitions;
    void* cscratch = nullptr;
    if (kernel == kFftCols &&
        hipMalloc(&cscratch, sizeof(double) * ((size_t)nbins + std::max(4096, fs.col_blocks))) != hipSuccess)
        return -1;
    FreeOnExit free_cscratch{cscratch};
    if (!c->dev[kDevPtrs].ensure(sizeof(void*))) return -1;
    const uint8_t** d_ptr = c->dev[kDevPtrs].as<const uint8_t*>();
    if (hipMemcpy(d_ptr, &d_rgb, sizeof(void*), hipMemcpyHostToDevice) != hipSuccess) return -1;
    g_ablate = ablate;
    const hipStream_t st = c->stream;
    hipEvent_t a = c->ev[6], b = c->ev[7];
    for (int it = -1; it < iters; it++) {
        if (it == 0) (void)hipEventRecord(a, st);
        hipError_t e = hipSuccess;
        switch (kernel) {
            case kK1:
            case kTimeStatsPass:   // K1 without the group histogram (the rgb2hsv + statistics pass)
                e = ds > 1 ? launch_hsv_ds(d_rgb, height, width, ds, gp, cls->fc, cls->d, pd, nchunks, c->d_k255, st)
                           : launch_hsv_stats_batch(d_ptr, 1, height, width, gp, cls->fc, cls->d, pd, 0, 0, nchunks,
                                                    c->d_k255, kernel == kK1, kernel == kK1 && fused,
                                                    all_aligned(&d_rgb, 1), st);
                break;
            case kFftRows: e = launch_rows_sel(fs, d_rgb, height, width, pd.sums, c->d_k255, inter, st); break;
            case kFftCols: e = launch_cols_sel(fs, inter, height, width, wf, tbl->d_map, nbins,
                                               (unsigned long long*)cscratch, (double*)cscratch + nbins, pd.sums,
                                               nullptr, st); break;
            default: set_error("kernel not supported by the timing hook"); g_ablate = 0; return -1;
        }
        if (e != hipSuccess) {
            set_error(std::string("launch failed: ") + hipGetErrorString(e));
            g_ablate = 0;
            return -1;
        }
    }
    (void)hipEventRecord(b, st);
    g_ablate = 0;
    if (hipEventSynchronize(b) != hipSuccess) return -1;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    *avg_ms = ms / iters;
    return 0;
}

// Validation hook: the power spectrum |X[u][k]|^2 of one device image through
// the production FFT kernels (compile-time plans only), column-major into
// d_out[(W/2+1) * H] (device).  Returns 0, -2 when the size has no
// compile-time plan, or -1.
extern "C" int phd_debug_log_mant(const double* d_x, double* d_y, long n) {
    clear_error();
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    hipError_t e = launch_log_mant(d_x, d_y, n, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        set_error(std::string("phd_debug_log_mant: ") + hipGetErrorString(e));
        return -1;
    }
    return 0;
}


extern "C" int phd_debug_fft_split_pass(const double* d_x, double* d_X, int n) {
    clear_error();
    Context* c = get_context();
    if (!c || !d_x || !d_X || n < 1) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    // the 3000-row column plan's tables: W_150^jm and W_3000^jm, whatever its last pass's form
    const double2* tw = get_ct_twiddles(c, 3000, false);
    if (!tw) return -1;
    hipError_t e = launch_fft_split_test(reinterpret_cast<const double2*>(d_x), tw, reinterpret_cast<double2*>(d_X), n,
                                         c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        set_error(std::string("phd_debug_fft_split_pass: ") + hipGetErrorString(e));
        return -1;
    }
    return 0;
}

extern "C" int phd_debug_power_spectrum(const uint8_t* d_rgb, int height, int width, double* d_out) {
    clear_error();
    Context* c = get_context();
    if (!c || !d_out) return -1;
    phd_config cfg;
    phd_config_default(&cfg);
    if (!report_once(c, d_rgb, height, width, cfg)) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const int nbins = cfg.radius_partitions * cfg.angle_partitions;
    const BlurTable* tbl = get_table(c, height, width, cfg.radius_partitions, cfg.angle_partitions);
    FftSel fs;
    if (!tbl || !select_fft(c, height, width, nbins, &d_rgb, 1, &fs, tbl)) return -1;
    if (!fs.ct) {
        set_error("no compile-time FFT plan for this size");
        return -2;
    }
    // the report just run left the image's channel sums at the start of the workspace
    uint8_t* dw = c->dev[kDevWs].as<uint8_t>();
    double2* const inter = c->dev[kDevInter].as<double2>();
    const int wf = width / 2 + 1;
    double* scratch = nullptr;
    if (hipMalloc(&scratch, sizeof(double) * (nbins + std::max(4096, fs.col_blocks))) != hipSuccess) return -1;
    auto* scratch_bins = reinterpret_cast<unsigned long long*>(scratch);
    const hipStream_t st = c->stream;
    hipError_t e = launch_rows_sel(fs, d_rgb, height, width, (const unsigned long long*)dw, c->d_k255, inter, st);
    if (e == hipSuccess)
        e = launch_cols_sel(fs, inter, height, width, wf, tbl->d_map, nbins, scratch_bins, scratch + nbins,
                            (const unsigned long long*)dw, d_out, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(scratch);
    if (e != hipSuccess) {
        set_error(std::string("power spectrum hook: ") + hipGetErrorString(e));
        return -1;
    }
    return 0;
}

// The decode kernels' host twin (phd_views.cpp: decode_view_host) behind the C ABI.
extern "C" int phd_debug_decode_view_host(const phd_typed_view* view, double* planes, uint8_t* rgb8, int* is_u8) {
    clear_error();
    std::string why;
    const int rc = decode_view_host(view, planes, rgb8, is_u8, &why);
    if (rc != 0) set_error(why);
    return rc;
}

// The YUV conversion kernel's host twin (phd_yuv.cpp: yuv_view_host) behind the C ABI.
extern "C" int phd_debug_yuv_view_host(const phd_yuv_view* view, uint8_t* dst) {
    clear_error();
    std::string why;
    const int rc = yuv_view_host(view, dst, &why);
    if (rc != 0) set_error(why);
    return rc;
}
