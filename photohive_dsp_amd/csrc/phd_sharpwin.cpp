// phd_sharpwin.cpp -- window sharpness: per T x T window (T = 16, 32, 64 or 128)
// of a packed RGB8 image the reference's get_variance_sharpness on that crop of
// the full-resolution luma (src/filtering.c:151-183: crop_pgm,
// src/image_processing.c:213-232; rgb2pgm, :505-512; filter_image with the 3 x 3
// Laplacian, src/filtering.c:81-107; get_average and get_variance, :125-148), left
// in device memory.  phd_sharpness_windows_device (window lists) and
// phd_sharpness_maps_device (a regular grid per image) through one body: every
// window of every image of a call in one launch; and the host twin
// phd_debug_window_sharpness_host.
// The entries' windows -- checks, counts and the walk that fills the table -- are a
// WindowPlan and the twin's checks window_twin_why (window_call.h); the launch goes
// through table_call (phd_host.h).
// Row code, the 128-bit D and the finish: sharp_window.h; kernel: window_sharp.hip.
// With PHD_SHARPWIN_HOST_ONLY the twin compiles alone, without HIP
// (tests/native/window_sharp_asan.cpp brings set_error and clear_error).

#include <cstring>
#include <string>
#include <vector>

#ifdef PHD_SHARPWIN_HOST_ONLY
namespace phd {
void set_error(const std::string& msg);
void clear_error();
}  // namespace phd
#else
#include "phd_host.h"
#endif
#include "window_call.h"
#include "sharp_window.h"

using namespace phd;

namespace {

bool sharp_size_why(int window, std::string* why) {
    if (shw_size_ok(window)) return true;
    return *why = "window must be 16, 32, 64 or 128, not " + std::to_string(window), false;
}

}  // namespace

#ifndef PHD_SHARPWIN_HOST_ONLY
// Both entries: the plan of their windows (lists, or a regular grid per image).
static int sharp_windows_call(const char* entry, WindowPlan plan, double* const* d_sharpness,
                              double* const* d_variance, void* stream) {
    clear_error();
    std::string why;
    if (!plan.args_why(d_sharpness, &why) || !sharp_size_why(plan.T, &why) ||
        !plan.build((const void* const*)d_sharpness, "d_sharpness", &why)) {
        set_error(std::string(entry) + ": " + why);
        return -1;
    }
    if (plan.total == 0) return 0;                           // no window at all: nothing for the device
    const int T = plan.T;
    const size_t nw = (size_t)plan.total;
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    // the call's table: window records | their destinations
    const size_t o_dst = al(sizeof(SharpWinRec) * nw), bytes = o_dst + sizeof(SharpWinDst) * nw;
    auto fill = [&](uint8_t* h) {
        SharpWinRec* recs = (SharpWinRec*)h;
        SharpWinDst* dst = (SharpWinDst*)(h + o_dst);
        memset(h + sizeof(SharpWinRec) * nw, 0, o_dst - sizeof(SharpWinRec) * nw);
        size_t w = 0;
        plan.for_each([&](int i, long long k, long long top, long long left) {
            const long long pitch = 3LL * plan.widths[i];
            const unsigned long long edge = (top == 0 && left == 0 ? 1ull : 0ull) |
                                            (top + T == plan.heights[i] && left + T == plan.widths[i] ? 2ull : 0ull);
            recs[w] = SharpWinRec{plan.d_images[i] + top * pitch + 3 * left, (unsigned long long)pitch << 2 | edge};
            dst[w++] = SharpWinDst{d_sharpness[i] + k, d_variance && d_variance[i] ? d_variance[i] + k : nullptr};
        });
    };
    auto launch = [&](const uint8_t* d, hipStream_t st) {
        return launch_window_sharp(T, (const SharpWinRec*)d, (const SharpWinDst*)(d + o_dst), (int)nw, st);
    };
    return table_call(c, stream, bytes, fill, launch, kWindowSharp) ? 0 : -1;
}

extern "C" int phd_sharpness_windows_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                            int n_images, const Crop_Boundaries* const* windows, int window,
                                            double* const* d_sharpness, double* const* d_variance, void* stream) {
    return sharp_windows_call("phd_sharpness_windows_device",
                              WindowPlan(d_images, heights, widths, n_images, windows, true, window, 0), d_sharpness,
                              d_variance, stream);
}

extern "C" int phd_sharpness_maps_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                         int n_images, int window, int stride, double* const* d_sharpness,
                                         double* const* d_variance, void* stream) {
    return sharp_windows_call("phd_sharpness_maps_device",
                              WindowPlan(d_images, heights, widths, n_images, nullptr, false, window, stride),
                              d_sharpness, d_variance, stream);
}
#endif  // PHD_SHARPWIN_HOST_ONLY

// k_window_sharp's twin: the window's luma byte by byte, then the kernel's column
// code over every column and the shared finish.
extern "C" int phd_debug_window_sharpness_host(const uint8_t* rgb, int height, int width,
                                               const Crop_Boundaries* windows, int window, double* sharpness,
                                               double* variance, unsigned long long* sums) {
    clear_error();
    std::string why, size_why;
    sharp_size_why(window, &size_why);
    if (!window_twin_why(rgb, height, width, windows, window, size_why, sharpness, "NULL sharpness", &why)) {
        set_error("phd_debug_window_sharpness_host: " + why);
        return -1;
    }
    if (!windows || windows->N == 0) return 0;
    const int T = window;
    const unsigned long long npix = (unsigned long long)T * T;
    std::vector<int> luma((size_t)T * T);
    for (int k = 0; k < windows->N; k++) {
        const uint8_t* first = rgb + 3LL * ((long long)windows->top[k] * width + windows->left[k]);
        for (int y = 0; y < T; y++) {
            const uint8_t* row = first + 3LL * width * y;
            for (int x = 0; x < T; x++) luma[(size_t)y * T + x] = shw_luma(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
        }
        long long s1 = 0;
        unsigned long long s2 = 0;
        for (int x = 0; x < T; x++) shw_column(luma.data(), T, x, 0, T, &s1, &s2);
        const double num = shw_num(shw_d(npix, (unsigned long long)s1, s2));
        sharpness[k] = shw_sharpness(num, npix, (unsigned long long)s1);
        if (variance) variance[k] = shw_variance(num, npix);
        if (sums) {
            sums[2 * k] = (unsigned long long)s1;
            sums[2 * k + 1] = s2;
        }
    }
    return 0;
}
