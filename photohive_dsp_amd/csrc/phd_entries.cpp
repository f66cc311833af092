// phd_entries.cpp -- the exported C-ABI report, statistics, blur and sharpness
// entries: argument checks, uploads, grouping and lanes around the pipeline
// (run_reports, phd_report.cpp), and the driver of every device batch
// (run_device_batch).  The entries over views, typed views and YUV views and
// their input stage: phd_inputs.cpp.
#include <cstdio>
#include <cstdlib>
#include <unistd.h>

#include "phd_host.h"

using namespace phd;

static Full_Report_Data* report_from_host(const uint8_t* rgb, int height, int width, size_t row_stride,
                                          const phd_config* cfg, const Crop_Boundaries* crops) {
    clear_error();
    if (!rgb || !cfg) {
        set_error("Error: Image pointer is NULL.");
        return nullptr;
    }
    if (!precheck(height, width)) return nullptr;
    Context* c = get_context();
    if (!c) return nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t row = 3 * (size_t)width;
    const size_t bytes = row * height;
    if (!c->dev[kDevStage].ensure(bytes) || !upload_init(c)) return nullptr;
    uint8_t* const d_stage = c->dev[kDevStage].as<uint8_t>();
    if (row_stride == 0 || row_stride == row) {
        std::string why;
        if (!upload_async(c, d_stage, rgb, bytes, &why)) {
            set_error(why);
            return nullptr;
        }
    } else {
        const hipError_t e = hipMemcpy2DAsync(d_stage, row, rgb, row_stride, row, height, hipMemcpyHostToDevice,
                                              c->h2d);
        if (e != hipSuccess) {
            set_error(std::string("upload failed: ") + hipGetErrorString(e));
            return nullptr;
        }
    }
    if (hipEventRecord(c->ev_up[0], c->h2d) != hipSuccess || hipStreamWaitEvent(c->stream, c->ev_up[0], 0) != hipSuccess) {
        set_error("upload ordering failed");
        return nullptr;
    }
    const uint8_t* imgs[1] = {d_stage};
    Full_Report_Data* out = nullptr;
    int status = -1;
    run_reports(c, imgs, 1, height, width, *cfg, crops, &out, &status, nullptr);
    // the caller's buffer may be freed on return: drain the upload on every path
    (void)hipStreamSynchronize(c->h2d);
    (void)hipStreamSynchronize(c->stream);
    return out;
}

extern "C" Full_Report_Data* phd_report_u8(const uint8_t* rgb, int height, int width, size_t row_stride,
                                           const phd_config* cfg, const Crop_Boundaries* crops) {
    return report_from_host(rgb, height, width, row_stride, cfg, crops);
}

extern "C" Full_Report_Data* get_full_report_data(Image_RGB* image, Crop_Boundaries* crops, int h_partitions,
                                                  int s_partitions, int v_partitions, double black_thresh,
                                                  double gray_thresh, double coverage_thresh,
                                                  int linked_list_size, int downsample_rate,
                                                  int radius_partitions, int angle_partitions,
                                                  float quantity_weight, float saturation_value_weight,
                                                  double fft_streak_thresh, double magnitude_thresh,
                                                  int blur_cutoff_ratio_denom) {
    clear_error();
    // pre_compute_error_checks (src/utilities.c:64-87), same order and messages
    if (!image) {
        set_error("Error: Image pointer is NULL.");
        return nullptr;
    }
    if (!precheck(image->height, image->width)) return nullptr;
    if (!image->r || !image->g || !image->b) {
        set_error("Error: At least one color channel was a NULL pointer.");
        return nullptr;
    }
    phd_config cfg{h_partitions, s_partitions, v_partitions, black_thresh, gray_thresh, coverage_thresh,
                   linked_list_size, downsample_rate, radius_partitions, angle_partitions,
                   quantity_weight, saturation_value_weight, fft_streak_thresh, magnitude_thresh,
                   blur_cutoff_ratio_denom};
    if (getenv("PHD_VERBOSE"))   // interface.c:34-35 prints this unconditionally
        printf("\n There are %d cores available to the C program.\n\n", (int)sysconf(_SC_NPROCESSORS_ONLN));
    // planar doubles: the RGB8 pipeline when they are k/255.0 (utils.py:30-46),
    // else the reference's fp64 arithmetic on them (phd_planar.cpp)
    Context* c = get_context();
    if (!c) return nullptr;
    Full_Report_Data* pooled;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        pooled = report_planar(c, image->r, image->g, image->b, image->height, image->width, cfg, crops);
    }
    if (!pooled) return nullptr;
    // the reference's C callers get the reference's allocation shape: every
    // member its own malloc, so free() of a member is valid (phd_legacy.cpp)
    Full_Report_Data* tree = legacy_tree_copy(pooled);
    free_full_report(&pooled);
    if (!tree) {
        set_error("report allocation failed");
        return nullptr;
    }
    legacy_register(tree);
    return tree;
}

// Runs body(context, lane, lanes) under the context's lock: on lane 0 (this
// thread) only, or -- when `want`, lanes_setting() >= 2 and the lane worker is
// free -- on lanes 0 and 1 concurrently, lane 1 (its own context, streams and
// workspaces) on the lane worker thread.  An error of lane 1 is reported on
// this thread unless lane 0 failed too.
template <class F>
static void on_lanes(Context* c0, bool want, F&& body) {
    Context* c1 = nullptr;
    if (want && lanes_setting() >= 2) {
        c1 = get_context_lane(1);
        if (!c1) clear_error();     // no second context: one lane
    }
    LaneWorker* lw = c1 ? lane_worker() : nullptr;
    if (!lw || !lw->try_acquire()) {
        std::lock_guard<std::mutex> lk(c0->mu);
        CallLanes cl(1);
        body(c0, 0, 1);
        return;
    }
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::string err1;
    lw->run([&] {
        clear_error();
        (void)hipSetDevice(dev);
        {
            std::lock_guard<std::mutex> lk1(c1->mu);
            CallLanes cl(2);
            body(c1, 1, 2);
        }
        err1 = phd_last_error();
    });
    {
        std::lock_guard<std::mutex> lk(c0->mu);
        CallLanes cl(2);
        body(c0, 0, 2);
    }
    lw->wait();
    lw->release();
    if (!err1.empty() && std::string(phd_last_error()).empty()) set_error(err1);
}

// rgb2hsv + get_hsv_average + get_rgb_statistics (src/image_processing.c:372-417,
// 533-553) over a batch of device images: one K1 launch without the group
// histogram.  HSV is never materialised; S-bar is the mean of the HSV s channel.
extern "C" int phd_hsv_stats_batch_device(const uint8_t* d_rgb, int n_images, int height, int width,
                                          size_t image_stride, RGB_Statistics* stats, double* avg_saturation,
                                          void* stream) {
    clear_error();
    if (!d_rgb || !stats || !avg_saturation || n_images <= 0 || height <= 0 || width <= 0 ||
        height > 32767 || width > 32767) {
        set_error("phd_hsv_stats_batch_device: bad arguments");
        return -1;
    }
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const hipStream_t st = work_stream(c, stream);
    const size_t stride = image_stride ? image_stride : 3 * (size_t)width * height;
    const long npix = (long)height * width;
    const int nchunks = (int)((npix + kChunk - 1) / kChunk);
    // A record: 6 moments | per-chunk s partials | 256 sums of d per max value
    const size_t a_kd = al(6 * sizeof(unsigned long long)) + al(sizeof(double) * nchunks);
    const size_t a_stride = a_kd + al(256 * sizeof(unsigned long long));
    const size_t rec = (size_t)n_images * a_stride, ptrs = al(sizeof(void*) * (size_t)n_images);
    const size_t fin = (size_t)n_images * 8 * sizeof(unsigned long long);   // k_stats_finish's records
    if (!c->dev[kDevWs].ensure(rec + ptrs + fin) || !c->pin.ensure(rec + ptrs + fin)) return -1;
    uint8_t* dw = c->dev[kDevWs].as<uint8_t>();
    uint8_t* hp = c->pin.as<uint8_t>();
    const uint8_t** hptr = (const uint8_t**)(hp + rec);
    for (int i = 0; i < n_images; i++) hptr[i] = d_rgb + (size_t)i * stride;
    const GridParams gp = make_grid([] { phd_config d; phd_config_default(&d); return d; }());
    const Context::Cls* cls = get_cls(c, gp);
    if (!cls) return -1;
    PaletteDev pd{};
    pd.sums = (unsigned long long*)dw;
    pd.s_part = (double*)(dw + al(6 * sizeof(unsigned long long)));
    pd.kd_sum = (unsigned long long*)(dw + a_kd);
    auto fail = [&](hipError_t e, const char* what) {
        set_error(std::string("phd_hsv_stats_batch_device: ") + what + ": " + hipGetErrorString(e));
        return -1;
    };
    hipError_t e;
    if ((e = hipMemsetAsync(dw, 0, rec, st)) != hipSuccess) return fail(e, "memset");
    if ((e = hipMemcpyAsync(dw + rec, hptr, sizeof(void*) * n_images, hipMemcpyHostToDevice, st)) != hipSuccess)
        return fail(e, "pointer upload");
    const int ps = c->prof.begin(kK1, st);
    if ((e = launch_hsv_stats_batch((const uint8_t* const*)(dw + rec), n_images, height, width, gp, cls->fc,
                                    cls->d, pd, (long)a_stride, 0, nchunks, c->d_k255, false, false,
                                    all_aligned(hptr, n_images), st)) != hipSuccess)
        return fail(e, "launch");
    c->prof.end(ps, st);
    // sum(s) = the chunk s partials (the partial final group and -(1 - 0.999999)
    // per min == 0 < max pixel) + sum_m (sum of d at max m) / m, finished on the
    // device per image (k_stats_finish): 64 bytes per image come back
    unsigned long long* dfin = (unsigned long long*)(dw + rec + ptrs);
    if ((e = launch_stats_finish(dw, n_images, (long)a_stride, (long)al(6 * sizeof(unsigned long long)),
                                 (long)a_kd, nchunks, npix, dfin, st)) != hipSuccess)
        return fail(e, "finish launch");
    if ((e = hipMemcpyAsync(hp, dfin, fin, hipMemcpyDeviceToHost, st)) != hipSuccess) return fail(e, "readback");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(e, "sync");
    c->prof.collect();
    const unsigned long long* hf = (const unsigned long long*)hp;
    for (int i = 0; i < n_images; i++) {
        stats[i] = stats_from_sums(hf + 8 * (size_t)i, npix);
        avg_saturation[i] = __builtin_bit_cast(double, hf[8 * (size_t)i + 6]);
    }
    return 0;
}

// The FFT + blur-profile path alone (BASELINE config 4) over n same-size
// device images on one context (its lock held by the caller): the row and
// column passes per image on the context's stream, the channel sums of
// remove_dc_bias from the row pass (compile-time plans) or the statistics pass
// (others), one read-back.  `lanes`: the lanes the whole call is split over.
static int blur_run(Context* c, int lanes, const uint8_t* const* imgs, int n_images, int height, int width,
                    const phd_config* cfg, double* bins_out, Blur_Vector* vectors_out, void* stream) {
    const hipStream_t st = work_stream(c, stream);
    const int nbins = cfg->radius_partitions * cfg->angle_partitions, wf = width / 2 + 1;
    const BlurTable* tbl = get_table(c, height, width, cfg->radius_partitions, cfg->angle_partitions);
    if (!tbl) return -1;
    FftSel fs;
    if (!select_fft(c, height, width, nbins, imgs, n_images, &fs, tbl)) return -1;
    // the half-prefetch column form when the other lane's column passes share
    // the CUs (13.12k vs 13.0k images/s at config 4)
    if (FftSel::forced_form() < 0 && lanes >= 2) fs.col_pf = false;
    // per image: bins, max partials, channel sums (+ the statistics pass's chunk slots)
    const long npix = (long)height * width;
    const int nchunks = (int)((npix + kChunk - 1) / kChunk);
    const size_t r_bins = 0, r_fmax = al(sizeof(double) * nbins);
    const size_t r_sums = r_fmax + al(sizeof(double) * (fs.col_blocks > 0 ? fs.col_blocks : 1));
    const size_t r_spart = r_sums + al(6 * sizeof(unsigned long long));
    const size_t r_kd = r_spart + al(sizeof(double) * nchunks);   // the statistics pass's sums of d (unused)
    const size_t rb = r_kd + al(256 * sizeof(unsigned long long));
    const size_t ptrs = al(sizeof(void*) * (size_t)n_images);
    const size_t inter_one = sizeof(double2) * inter_elems(height, width);
    if (!c->dev[kDevWs].ensure((size_t)n_images * rb + ptrs) || !c->pin.ensure((size_t)n_images * rb + ptrs) ||
        !c->dev[kDevInter].ensure(inter_one))
        return -1;
    uint8_t* dw = c->dev[kDevWs].as<uint8_t>();
    uint8_t* hp = c->pin.as<uint8_t>();
    double2* const inter = c->dev[kDevInter].as<double2>();
    auto fail = [&](hipError_t e, const char* what) {
        set_error(std::string("phd_blur_batch_device: ") + what + ": " + hipGetErrorString(e));
        return -1;
    };
    hipError_t e;
    if ((e = hipMemsetAsync(dw, 0, (size_t)n_images * rb, st)) != hipSuccess) return fail(e, "memset");
    if (!fs.ct) {
        // the runtime-plan row pass removes the DC bias itself: channel sums first
        const uint8_t** hptr = (const uint8_t**)(hp + (size_t)n_images * rb);
        for (int i = 0; i < n_images; i++) hptr[i] = imgs[i];
        if ((e = hipMemcpyAsync(dw + (size_t)n_images * rb, hptr, sizeof(void*) * n_images, hipMemcpyHostToDevice,
                                st)) != hipSuccess)
            return fail(e, "pointer upload");
        const GridParams gp = make_grid(*cfg);
        const Context::Cls* cls = get_cls(c, gp);
        if (!cls) return -1;
        PaletteDev pd{};
        pd.sums = (unsigned long long*)(dw + r_sums);
        pd.s_part = (double*)(dw + r_spart);
        pd.kd_sum = (unsigned long long*)(dw + r_kd);
        if ((e = launch_hsv_stats_batch((const uint8_t* const*)(dw + (size_t)n_images * rb), n_images, height,
                                        width, gp, cls->fc, cls->d, pd, (long)rb, 0, nchunks, c->d_k255, false,
                                        false, all_aligned(hptr, n_images), st)) != hipSuccess)
            return fail(e, "statistics pass");
    }
    for (int i = 0; i < n_images; i++) {
        unsigned long long* sums = (unsigned long long*)(dw + (size_t)i * rb + r_sums);
        int ps = c->prof.begin(kFftRows, st);
        if ((e = launch_rows_sel(fs, imgs[i], height, width, sums, c->d_k255, inter, st,
                                 fs.ct ? sums : nullptr)) != hipSuccess)
            return fail(e, "row pass");
        c->prof.end(ps, st);
        ps = c->prof.begin(kFftCols, st);
        if ((e = launch_cols_sel(fs, inter, height, width, wf, tbl->d_map, nbins,
                                 (unsigned long long*)(dw + (size_t)i * rb + r_bins),
                                 (double*)(dw + (size_t)i * rb + r_fmax),
                                 sums, nullptr, st)) != hipSuccess)
            return fail(e, "column pass");
        c->prof.end(ps, st);
    }
    if ((e = hipMemcpyAsync(hp, dw, (size_t)n_images * rb, hipMemcpyDeviceToHost, st)) != hipSuccess)
        return fail(e, "readback");
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(e, "sync");
    c->prof.collect();
    for (int i = 0; i < n_images; i++) {
        const uint8_t* r = hp + (size_t)i * rb;
        const double* fpart = (const double*)(r + r_fmax);
        double fmax = 0.0;
        for (int b = 0; b < fs.col_blocks; b++) fmax = fpart[b] > fmax ? fpart[b] : fmax;
        finish_blur(*tbl, (const unsigned long long*)(r + r_bins), fmax, *cfg, bins_out + (size_t)i * nbins,
                    vectors_out + (size_t)i * 10);
    }
    return 0;
}

extern "C" int phd_blur_batch_device(const uint8_t* d_rgb, int n_images, int height, int width,
                                     size_t image_stride, const phd_config* cfg, double* bins_out,
                                     Blur_Vector* vectors_out, void* stream) {
    clear_error();
    if (!d_rgb || !cfg || !bins_out || !vectors_out || n_images <= 0) {
        set_error("phd_blur_batch_device: bad arguments");
        return -1;
    }
    std::string why;
    if (!validate_config(*cfg, &why)) {
        set_error(why);
        return -1;
    }
    if (!precheck(height, width)) return -1;
    Context* c = get_context();
    if (!c) return -1;
    const size_t stride = image_stride ? image_stride : 3 * (size_t)width * height;
    std::vector<const uint8_t*> imgs(n_images);
    for (int i = 0; i < n_images; i++) imgs[i] = d_rgb + (size_t)i * stride;
    const int nbins = cfg->radius_partitions * cfg->angle_partitions;
    // two lanes for large batches on the library's streams, as the full
    // report's batches: the second half on lane 1 (its own context, stream
    // and intermediate), each lane's launch gaps and kernel tails under the
    // other's kernels
    int rc[2] = {0, 0};
    on_lanes(c, n_images >= 16 && !stream, [&](Context* cl, int lane, int nl) {
        const int h = nl == 2 ? n_images / 2 : n_images;
        const int i0 = lane ? h : 0, m = lane ? n_images - h : h;
        rc[lane] = blur_run(cl, nl, imgs.data() + i0, m, height, width, cfg, bins_out + (size_t)i0 * nbins,
                            vectors_out + (size_t)i0 * 10, stream);
    });
    return rc[0] < 0 || rc[1] < 0 ? -1 : 0;
}

static int count_failures(const int* status, int n) {
    int fails = 0;
    for (int i = 0; i < n; i++) fails += status[i] != 0;
    return fails;
}

// Host images of any sizes: each same-size group (<= 16) is uploaded into one
// of two device staging buffers and reported as one batch; the next group's
// upload (pinned slot ring, copy threads + DMA) runs on an uploader thread
// while the current group computes.
static int report_batch_u8(const uint8_t* const* images, const int* heights, const int* widths, int n_images,
                           const phd_config* cfg, const Crop_Boundaries* const* crops, Full_Report_Data** out,
                           int* status) {
    if (!images || !heights || !widths || !cfg || !out || !status || n_images <= 0) {
        set_error("phd_report_batch_u8: bad arguments");
        return -1;
    }
    for (int i = 0; i < n_images; i++) {
        out[i] = nullptr;
        status[i] = -1;
        if (!images[i]) {
            set_error("Error: Image pointer is NULL.");
            return -1;
        }
    }
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!upload_init(c)) return -1;
    std::vector<std::vector<int>> groups;
    static const int gcap = phd_knob("PHD_HOST_GROUP") ? std::max(1, atoi(phd_knob("PHD_HOST_GROUP"))) : 16;
    for (auto& g : size_groups(heights, widths, n_images, gcap)) {
        if (precheck(heights[g[0]], widths[g[0]])) groups.push_back(std::move(g));
    }
    // device buffers first (the uploader thread must not allocate)
    size_t need = 0;
    for (const auto& g : groups) need = std::max(need, g.size() * 3 * (size_t)widths[g[0]] * heights[g[0]]);
    for (int b = 0; b < 2 && !groups.empty(); b++)
        if (!c->dev[kDevStage2 + b].ensure(need)) return -1;
    struct Up {
        bool ok = true;
        std::string why;
    };
    auto upload = [c, images, heights, widths](const std::vector<int>& g, int b, Up* u) {
        const size_t bytes = 3 * (size_t)widths[g[0]] * heights[g[0]];
        uint8_t* const stage2 = c->dev[kDevStage2 + b].as<uint8_t>();
        if (upload_streams() == 2 && g.size() > 1) {
            // odd images on h2d2 from a second thread: two pageable copies in flight
            Up u2;
            std::thread t2([&] {
                for (size_t k = 1; k < g.size() && u2.ok; k += 2)
                    u2.ok = upload_async(c, stage2 + k * bytes, images[g[k]], bytes, &u2.why, c->h2d2);
            });
            for (size_t k = 0; k < g.size() && u->ok; k += 2)
                u->ok = upload_async(c, stage2 + k * bytes, images[g[k]], bytes, &u->why, c->h2d);
            t2.join();
            if (u->ok && !u2.ok) *u = u2;
            if (u->ok && (hipEventRecord(c->ev_h2d2, c->h2d2) != hipSuccess ||
                          hipStreamWaitEvent(c->h2d, c->ev_h2d2, 0) != hipSuccess)) {
                u->ok = false;
                u->why = "upload event failed";
            }
        } else {
            for (size_t k = 0; k < g.size() && u->ok; k++)
                u->ok = upload_async(c, stage2 + k * bytes, images[g[k]], bytes, &u->why);
        }
        if (u->ok && hipEventRecord(c->ev_up[b], c->h2d) != hipSuccess) {
            u->ok = false;
            u->why = "upload event failed";
        }
    };
    std::vector<Up> ups(groups.size());
    std::thread th;
    if (!groups.empty()) th = std::thread(upload, std::cref(groups[0]), 0, &ups[0]);
    for (size_t gi = 0; gi < groups.size(); gi++) {
        th.join();                                   // group gi is enqueued (its host buffers are read)
        const auto& g = groups[gi];
        const int b = (int)(gi & 1);
        // the next group's upload runs under this group's reports (its buffer's
        // previous group finished: run_reports returns after the GPU is done)
        if (gi + 1 < groups.size()) th = std::thread(upload, std::cref(groups[gi + 1]), 1 - b, &ups[gi + 1]);
        const int m = (int)g.size(), h = heights[g[0]], w = widths[g[0]];
        const size_t bytes = 3 * (size_t)w * h;
        std::vector<const uint8_t*> ptrs(m);
        std::vector<const Crop_Boundaries*> cr(m, nullptr);
        for (int k = 0; k < m; k++) {
            ptrs[k] = c->dev[kDevStage2 + b].as<uint8_t>() + (size_t)k * bytes;
            if (crops) cr[k] = crops[g[k]];
        }
        RunResults r(m);
        if (!ups[gi].ok) set_error(ups[gi].why);
        else if (hipStreamWaitEvent(c->stream, c->ev_up[b], 0) != hipSuccess) set_error("upload ordering failed");
        else run_reports(c, ptrs.data(), m, h, w, *cfg, nullptr, r.o.data(), r.st.data(), nullptr,
                         crops ? cr.data() : nullptr);
        r.scatter(g, out, status);
    }
    if (th.joinable()) th.join();
    // the caller's buffers may be freed on return: every transfer has completed
    (void)hipStreamSynchronize(c->h2d);
    (void)hipStreamSynchronize(c->h2d2);
    (void)hipStreamSynchronize(c->stream);
    return count_failures(status, n_images);
}

extern "C" int phd_report_batch_u8(const uint8_t* const* images, const int* heights, const int* widths,
                                   int n_images, const phd_config* cfg, Full_Report_Data** out, int* status) {
    clear_error();
    return report_batch_u8(images, heights, widths, n_images, cfg, nullptr, out, status);
}

// ---- device batch entries ----------------------------------------------------
// Each entry checks its arguments, keeps the images whose boxes (or view) are
// valid, builds its groups of same-size images and hands them to
// run_device_batch.  Per-image crop boxes: get_variance_sharpness
// (src/filtering.c:151-183) as get_full_report_data calls it (src/interface.c:73).

// The images of a call whose boxes pass check_crops' rules (`keep`, in order;
// crops NULL: every image).  Marks every image failed first.  An image with a
// bad box fails alone: out NULL, status -1, and the message (the last one
// stays in phd_last_error) names the image and the box.
static std::vector<int> valid_box_images(const Crop_Boundaries* const* crops, const int* heights, const int* widths,
                                         int height, int width, int n, Full_Report_Data** out, int* status) {
    std::vector<int> keep;
    std::string bad;
    for (int i = 0; i < n; i++) {
        out[i] = nullptr;
        status[i] = -1;
        std::string why;
        if (!crops || crops_why(crops[i], heights ? heights[i] : height, widths ? widths[i] : width, &why))
            keep.push_back(i);
        else bad = "image " + std::to_string(i) + ": " + why;
    }
    if (!bad.empty()) set_error(bad);
    return keep;
}

namespace phd {

// The entry a report call's messages name: the most derived output present
// picks it (a NULL output is one the entry does not take); with none, `plain`
// -- "" for the family's plain entry, what the mixed entries pass otherwise.
std::string entry_name(const char* family, const char* plain, const CallOutputs& outs) {
    return std::string("phd_report_batch_device_") + family +
           (outs.box_stats ? "_box_stats" : outs.box_palettes ? "_box_palettes" : outs.d_labels ? "_labels" : plain);
}

// What every entry that can take outputs does first: the caller's structs zeroed,
// then the argument check (args_ok) and the label slots' rule, no HIP call yet.
bool report_prologue(const std::string& entry, bool args_ok, int n_images, const phd_config* cfg,
                     const CallOutputs& outs) {
    clear_error();
    outs.reset(n_images);
    if (!args_ok) {
        set_error(entry + ": bad arguments");
        return false;
    }
    if (outs.needs_label_slots() && make_grid(*cfg).tl >= 32768) {
        set_error(entry + ": label maps need fewer than 32768 octree groups (palette slots)");
        return false;
    }
    return true;
}

// One group of a batch large enough for two lanes (two-lane calls on the
// library's streams only): two groups in lane_split's proportion, one per lane.
void split_for_lanes(std::vector<std::vector<int>>* groups, void* stream) {
    if (groups->size() != 1 || (*groups)[0].size() < 16 || stream || lanes_setting() < 2) return;
    std::vector<int>& first = (*groups)[0];
    const int h = lane_split((int)first.size());
    std::vector<int> second(first.begin() + h, first.end());
    first.resize(h);
    groups->push_back(std::move(second));
}

// The groups of the kept images of a mixed-size call: 64 images a run, or as
// many as 64 of the 12 MP headline size hold (small images: one run for a
// whole size instead of one per 64, so the per-run launches, host round trip
// and partly filled grids are paid a few times)
std::vector<std::vector<int>> mixed_groups(const std::vector<BatchImage>& imgs) {
    std::vector<int> hs, ws;
    for (const BatchImage& im : imgs) {
        hs.push_back(im.height);
        ws.push_back(im.width);
    }
    return size_groups(hs.data(), ws.data(), (int)imgs.size(), 64, 64L * 12000000L);
}

void report_group(Context* cl, const std::vector<BatchImage>& imgs, const std::vector<int>& grp,
                  const std::vector<int>& ks, const uint8_t* const* ptrs, bool boxes, const phd_config& cfg,
                  void* stream, RunResults* r) {
    const int m = (int)ks.size();
    if (m == 0) return;
    std::vector<const uint8_t*> rp(m);
    std::vector<const Crop_Boundaries*> cr(m);
    std::vector<ImageOutputs> outs(m);
    for (int q = 0; q < m; q++) {
        rp[q] = ptrs[ks[q]];
        cr[q] = imgs[grp[ks[q]]].boxes;
        outs[q] = imgs[grp[ks[q]]].outs;
    }
    RunResults rr(m);
    run_reports(cl, rp.data(), m, imgs[grp[0]].height, imgs[grp[0]].width, cfg, nullptr, rr.o.data(), rr.st.data(),
                (hipStream_t)stream, boxes ? cr.data() : nullptr, outs.data());
    for (int q = 0; q < m; q++) {
        r->o[ks[q]] = rr.o[q];
        r->st[ks[q]] = rr.st[q];
    }
}

// Two lanes when there are two or more groups on the library's streams: lane
// L starts with group L, then each lane takes the next untaken group when it
// is done with its last.
int run_device_batch(Context* c, const std::vector<BatchImage>& imgs, const std::vector<std::vector<int>>& groups,
                     GroupFn run_group, bool boxes, const phd_config& cfg, Full_Report_Data** out, int* status,
                     int n_images, void* stream) {
    std::atomic<size_t> taken{0};                             // groups taken past each lane's first
    if (!groups.empty())
        on_lanes(c, groups.size() >= 2 && !stream, [&](Context* cl, int lane, int nl) {
            for (size_t gi = lane; gi < groups.size(); gi = nl + taken.fetch_add(1)) {
                const std::vector<int>& grp = groups[gi];
                RunResults r(grp.size());
                std::vector<int> idx(grp.size());
                for (size_t k = 0; k < grp.size(); k++) idx[k] = imgs[grp[k]].index;
                run_group(cl, imgs, grp, boxes, cfg, stream, &r);
                r.scatter(idx, out, status);
            }
        });
    return count_failures(status, n_images);
}

}  // namespace phd

// A group of packed device images: reported where they lie.
static void run_packed_group(Context* cl, const std::vector<BatchImage>& imgs, const std::vector<int>& grp, bool boxes,
                             const phd_config& cfg, void* stream, RunResults* r) {
    std::vector<const uint8_t*> ptrs(grp.size());
    std::vector<int> ks(grp.size());
    for (size_t k = 0; k < grp.size(); k++) {
        ptrs[k] = (const uint8_t*)imgs[grp[k]].src;
        ks[k] = (int)k;
    }
    report_group(cl, imgs, grp, ks, ptrs.data(), boxes, cfg, stream, r);
}

// Same-size device images at a stride: all kept images are one run (never cut
// by size_groups' caps), split in two for two lanes so that each half's host
// phases and launch gaps overlap the other's kernels.
static int report_same_size(const char* entry, const uint8_t* d_rgb, int n_images, int height, int width,
                            size_t image_stride, const phd_config* cfg, const Crop_Boundaries* const* crops,
                            Full_Report_Data** out, int* status, void* stream) {
    clear_error();
    if (!d_rgb || !cfg || !out || !status || n_images <= 0) {
        set_error(std::string(entry) + ": bad arguments");
        return -1;
    }
    Context* c = get_context();
    if (!c) return -1;
    const std::vector<int> keep = valid_box_images(crops, nullptr, nullptr, height, width, n_images, out, status);
    const size_t stride = image_stride ? image_stride : 3 * (size_t)width * height;
    std::vector<BatchImage> imgs;
    std::vector<std::vector<int>> groups(keep.empty() ? 0 : 1);
    for (int i : keep) {
        groups[0].push_back((int)imgs.size());
        imgs.push_back({i, BatchImage::kPacked, d_rgb + (size_t)i * stride, height, width, crops ? crops[i] : nullptr});
    }
    split_for_lanes(&groups, stream);
    return run_device_batch(c, imgs, groups, run_packed_group, crops != nullptr, *cfg, out, status, n_images, stream);
}

extern "C" int phd_report_batch_device(const uint8_t* d_rgb, int n_images, int height, int width,
                                       size_t image_stride, const phd_config* cfg, Full_Report_Data** out,
                                       int* status, void* stream) {
    return report_same_size("phd_report_batch_device", d_rgb, n_images, height, width, image_stride, cfg, nullptr,
                            out, status, stream);
}

extern "C" int phd_report_batch_device_crops(const uint8_t* d_rgb, int n_images, int height, int width,
                                             size_t image_stride, const phd_config* cfg,
                                             const Crop_Boundaries* const* crops, Full_Report_Data** out,
                                             int* status, void* stream) {
    return report_same_size(crops ? "phd_report_batch_device_crops" : "phd_report_batch_device", d_rgb, n_images,
                            height, width, image_stride, cfg, crops, out, status, stream);
}

// Device-resident images of any sizes (BASELINE config 5): one batched run
// (K1, FFTs, palette tail, per-image read-back) per group of same-size images.
// A single size group is not split across lanes.
// plain: what the entry's name ends in when the call has no outputs (entry_name).
static int report_mixed(const char* plain, const uint8_t* const* d_images, const int* heights, const int* widths,
                        int n_images, const phd_config* cfg, const Crop_Boundaries* const* crops,
                        const CallOutputs& outs, Full_Report_Data** out, int* status, void* stream) {
    if (!report_prologue(entry_name("mixed", plain, outs),
                         d_images && heights && widths && cfg && out && status && n_images > 0, n_images, cfg, outs))
        return -1;
    Context* c = get_context();
    if (!c) return -1;
    std::vector<BatchImage> imgs;
    for (int i : valid_box_images(crops, heights, widths, 0, 0, n_images, out, status))
        imgs.push_back({i, BatchImage::kPacked, d_images[i], heights[i], widths[i], crops ? crops[i] : nullptr,
                        outs.of(i)});
    return run_device_batch(c, imgs, mixed_groups(imgs), run_packed_group, crops != nullptr, *cfg, out, status,
                            n_images, stream);
}

extern "C" int phd_report_batch_device_mixed(const uint8_t* const* d_images, const int* heights, const int* widths,
                                             int n_images, const phd_config* cfg, Full_Report_Data** out,
                                             int* status, void* stream) {
    return report_mixed("", d_images, heights, widths, n_images, cfg, nullptr, {}, out, status, stream);
}

extern "C" int phd_report_batch_device_mixed_crops(const uint8_t* const* d_images, const int* heights,
                                                   const int* widths, int n_images, const phd_config* cfg,
                                                   const Crop_Boundaries* const* crops, Full_Report_Data** out,
                                                   int* status, void* stream) {
    return report_mixed(crops ? "_crops" : "", d_images, heights, widths, n_images, cfg, crops, {}, out, status,
                        stream);
}

// phd_report_batch_device_mixed_crops plus each image's palette label map (the
// parents' pixel lists after group_irregular_pixels,
// src/color_quantization.c:342-479: ReportRun::label_maps), its box palette too
// (_box_palettes: per crop box, the elements of every palette slot, counted
// behind the label launch) and its box statistics too (_box_stats:
// ReportRun::box_stat_job, beside the sharpness launch).  An output passed as
// NULL is one the entry does not take.
extern "C" int phd_report_batch_device_mixed_labels(const uint8_t* const* d_images, const int* heights,
                                                    const int* widths, int n_images, const phd_config* cfg,
                                                    const Crop_Boundaries* const* crops,
                                                    uint16_t* const* d_labels, Full_Report_Data** out, int* status,
                                                    void* stream) {
    return report_mixed("_labels", d_images, heights, widths, n_images, cfg, crops, {d_labels}, out, status, stream);
}

extern "C" int phd_report_batch_device_mixed_box_palettes(const uint8_t* const* d_images, const int* heights,
                                                          const int* widths, int n_images, const phd_config* cfg,
                                                          const Crop_Boundaries* const* crops,
                                                          uint16_t* const* d_labels, phd_box_palette* box_palettes,
                                                          Full_Report_Data** out, int* status, void* stream) {
    return report_mixed("_labels", d_images, heights, widths, n_images, cfg, crops, {d_labels, box_palettes}, out,
                        status, stream);
}

extern "C" int phd_report_batch_device_mixed_box_stats(const uint8_t* const* d_images, const int* heights,
                                                       const int* widths, int n_images, const phd_config* cfg,
                                                       const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                                       phd_box_palette* box_palettes, phd_box_stats* box_stats,
                                                       Full_Report_Data** out, int* status, void* stream) {
    return report_mixed("_labels", d_images, heights, widths, n_images, cfg, crops,
                        {d_labels, box_palettes, box_stats}, out, status, stream);
}

extern "C" int phd_report_batch_u8_crops(const uint8_t* const* images, const int* heights, const int* widths,
                                         int n_images, const phd_config* cfg, const Crop_Boundaries* const* crops,
                                         Full_Report_Data** out, int* status) {
    clear_error();
    if (!crops) return report_batch_u8(images, heights, widths, n_images, cfg, nullptr, out, status);
    if (!images || !heights || !widths || !cfg || !out || !status || n_images <= 0) {
        set_error("phd_report_batch_u8_crops: bad arguments");
        return -1;
    }
    const std::vector<int> keep = valid_box_images(crops, heights, widths, 0, 0, n_images, out, status);
    const int m = (int)keep.size();
    std::vector<const uint8_t*> im(m);
    std::vector<int> hs(m), ws(m);
    std::vector<const Crop_Boundaries*> cr(m);
    for (int k = 0; k < m; k++) {
        im[k] = images[keep[k]];
        hs[k] = heights[keep[k]];
        ws[k] = widths[keep[k]];
        cr[k] = crops[keep[k]];
    }
    RunResults r(m);
    const int rc = m > 0 ? report_batch_u8(im.data(), hs.data(), ws.data(), m, cfg, cr.data(), r.o.data(),
                                           r.st.data()) : 0;
    r.scatter(keep, out, status);
    return rc < 0 ? -1 : count_failures(status, n_images);
}

// The sharpness stage alone over n same-size device images, as
// phd_blur_batch_device runs its stage: one batched launch for every box of
// the call, then var / mean per box on the host (the full report's values).
extern "C" int phd_sharpness_batch_device(const uint8_t* d_rgb, int n_images, int height, int width,
                                          size_t image_stride, const Crop_Boundaries* const* crops, double* out,
                                          void* stream) {
    clear_error();
    if (!d_rgb || !crops || n_images <= 0 || height <= 0 || width <= 0) {
        set_error("phd_sharpness_batch_device: bad arguments");
        return -1;
    }
    for (int i = 0; i < n_images; i++) {
        std::string why;
        if (!crops_why(crops[i], height, width, &why)) {
            set_error("image " + std::to_string(i) + ": " + why);
            return -1;
        }
    }
    SharpPlan plan;
    if (!sharp_plan(crops, n_images, true, &plan)) {
        set_error("too many crop boxes in one call");
        return -1;
    }
    const size_t nb = plan.boxes.size();
    if (nb == 0) return 0;
    if (!out) {
        set_error("phd_sharpness_batch_device: bad arguments");
        return -1;
    }
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const hipStream_t st = work_stream(c, stream);
    const size_t stride = image_stride ? image_stride : 3 * (size_t)width * height;
    std::vector<const uint8_t*> imgs(n_images);
    for (int i = 0; i < n_images; i++) imgs[i] = d_rgb + (size_t)i * stride;
    if (!c->pin.ensure(2 * sizeof(double) * nb)) return -1;
    double* d_flat = nullptr;
    if (!enqueue_sharpness(c, imgs.data(), n_images, width, plan, nullptr, 0, st, &d_flat)) return -1;
    hipError_t e;
    if ((e = hipMemcpyAsync(c->pin.as(), d_flat, 2 * sizeof(double) * nb, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess) {
        set_error(std::string("phd_sharpness_batch_device: ") + hipGetErrorString(e));
        return -1;
    }
    c->prof.collect();
    const double* sums = c->pin.as<const double>();
    for (size_t k = 0; k < nb; k++) {
        const SharpBox& b = plan.boxes[k];
        out[k] = sharp_value(sums[2 * k], sums[2 * k + 1], b.right - b.left, b.bottom - b.top);
    }
    return 0;
}
