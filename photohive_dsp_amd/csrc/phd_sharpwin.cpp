// phd_sharpwin.cpp -- window sharpness: per T x T window (T = 16, 32, 64 or 128)
// of a packed RGB8 image the reference's get_variance_sharpness on that crop of
// the full-resolution luma (src/filtering.c:151-183: crop_pgm,
// src/image_processing.c:213-232; rgb2pgm, :505-512; filter_image with the 3 x 3
// Laplacian, src/filtering.c:81-107; get_average and get_variance, :125-148), left
// in device memory.  phd_sharpness_windows_device (window lists) and
// phd_sharpness_maps_device (a regular grid per image) through one body: every
// window of every image of a call in one launch; and the host twin
// phd_debug_window_sharpness_host.
// Row code, the 128-bit D and the finish: sharp_window.h; kernel: window_sharp.hip.
// With PHD_SHARPWIN_HOST_ONLY the validation and the twin compile alone, without
// HIP (tests/native/window_sharp_asan.cpp brings set_error and clear_error).

#include <cstring>
#include <string>
#include <vector>

#ifdef PHD_SHARPWIN_HOST_ONLY
#include "../../include/photohive_dsp.h"
namespace phd {
void set_error(const std::string& msg);
void clear_error();
}  // namespace phd
#else
#include "phd_host.h"
#endif
#include "blur_window.h"
#include "sharp_window.h"

using namespace phd;

namespace {

// window_list_why's rules and words (phd_blurwin.cpp) at this stage's sizes
bool sharp_list_why(const Crop_Boundaries* b, int T, int height, int width, std::string* why) {
    if (!b || b->N == 0) return true;
    if (b->N < 0 || !b->top || !b->bottom || !b->left || !b->right) return *why = "bad window list", false;
    for (int k = 0; k < b->N; k++) {
        const int rule = win_box_check(b->top[k], b->bottom[k], b->left[k], b->right[k], T, height, width);
        if (rule == 0) continue;
        const std::string box = "window " + std::to_string(k) + " (top " + std::to_string(b->top[k]) + ", bottom " +
                                std::to_string(b->bottom[k]) + ", left " + std::to_string(b->left[k]) + ", right " +
                                std::to_string(b->right[k]) + ")";
        if (rule == 1) return *why = box + " is not " + std::to_string(T) + " x " + std::to_string(T), false;
        return *why = box + " leaves the " + std::to_string(height) + " x " + std::to_string(width) + " image", false;
    }
    return true;
}

bool sharp_size_why(int window, std::string* why) {
    if (shw_size_ok(window)) return true;
    return *why = "window must be 16, 32, 64 or 128, not " + std::to_string(window), false;
}

std::string too_small(int height, int width, int T) {
    return std::to_string(height) + " x " + std::to_string(width) + " is smaller than the window " +
           std::to_string(T);
}

#ifndef PHD_SHARPWIN_HOST_ONLY
// Both entries: window lists (stride 0) or a regular grid per image (stride > 0).
int sharp_windows_call(const char* entry, const uint8_t* const* d_images, const int* heights, const int* widths,
                       int n_images, const Crop_Boundaries* const* windows, int window, int stride,
                       double* const* d_sharpness, double* const* d_variance, void* stream) {
    clear_error();
    auto bad = [&](const std::string& what) {
        set_error(std::string(entry) + ": " + what);
        return -1;
    };
    const bool grid = !windows;
    if (!d_images || !heights || !widths || !d_sharpness) return bad("NULL argument");
    if (n_images <= 0) return bad("n_images must be positive");
    std::string why;
    if (!sharp_size_why(window, &why)) return bad(why);
    if (grid && stride <= 0) return bad("stride must be positive, not " + std::to_string(stride));
    const int T = window;
    // windows of image i: windows[i]->N, or the grid's gh * gw (window_grid's rule)
    std::vector<long long> count(n_images, 0), gws(n_images, 0);
    long long nw = 0;
    for (int i = 0; i < n_images; i++) {
        const std::string img = "image " + std::to_string(i) + ": ";
        if (!d_images[i]) return bad(img + "NULL image");
        if (heights[i] < T || widths[i] < T) return bad(img + too_small(heights[i], widths[i], T));
        if (grid) {
            gws[i] = (widths[i] - T) / stride + 1;
            count[i] = ((long long)(heights[i] - T) / stride + 1) * gws[i];
        } else {
            if (!sharp_list_why(windows[i], T, heights[i], widths[i], &why)) return bad(img + why);
            count[i] = windows[i] ? windows[i]->N : 0;
        }
        if (count[i] > 0 && !d_sharpness[i])
            return bad(img + "NULL d_sharpness for " + std::to_string(count[i]) + " windows");
        nw += count[i];
        if (nw > 0x7FFFFFFFLL) return bad("too many windows");
    }
    if (nw == 0) return 0;                                   // no window at all: nothing for the device
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const hipStream_t st = work_stream(c, stream);
    // the call's table: window records | their destinations
    const size_t o_dst = al(sizeof(SharpWinRec) * (size_t)nw), bytes = o_dst + sizeof(SharpWinDst) * (size_t)nw;
    auto run = [&]() {
        // the context's launch table, filled in place
        uint8_t* h = (uint8_t*)table_begin(c, bytes);
        if (!h) return false;
        uint8_t* d = (uint8_t*)c->d_views;
        SharpWinRec* recs = (SharpWinRec*)h;
        SharpWinDst* dst = (SharpWinDst*)(h + o_dst);
        memset(h + sizeof(SharpWinRec) * (size_t)nw, 0, o_dst - sizeof(SharpWinRec) * (size_t)nw);
        size_t w = 0;
        for (int i = 0; i < n_images; i++) {
            const long long pitch = 3LL * widths[i];
            for (long long k = 0; k < count[i]; k++, w++) {
                const long long top = grid ? (k / gws[i]) * stride : windows[i]->top[k];
                const long long left = grid ? (k % gws[i]) * stride : windows[i]->left[k];
                const unsigned long long edge = (top == 0 && left == 0 ? 1ull : 0ull) |
                                                (top + T == heights[i] && left + T == widths[i] ? 2ull : 0ull);
                recs[w] = SharpWinRec{d_images[i] + top * pitch + 3 * left, (unsigned long long)pitch << 2 | edge};
                dst[w] = SharpWinDst{d_sharpness[i] + k, d_variance && d_variance[i] ? d_variance[i] + k : nullptr};
            }
        }
        if (!table_upload(c, bytes, st)) return false;
        const int ps = c->prof.begin(kWindowSharp, st);
        const hipError_t e = launch_window_sharp(T, (const SharpWinRec*)d, (const SharpWinDst*)(d + o_dst), (int)nw, st);
        c->prof.end(ps, st);
        PHD_HIP(e);
        if (!table_launched(c, st)) return false;
        if (!stream) {                                       // the library's stream: waited for
            PHD_HIP(hipStreamSynchronize(st));
            c->prof.collect();
        }
        return true;
    };
    return run() ? 0 : -1;
}
#endif  // PHD_SHARPWIN_HOST_ONLY

}  // namespace

#ifndef PHD_SHARPWIN_HOST_ONLY
extern "C" int phd_sharpness_windows_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                            int n_images, const Crop_Boundaries* const* windows, int window,
                                            double* const* d_sharpness, double* const* d_variance, void* stream) {
    if (!windows) {
        clear_error();
        set_error("phd_sharpness_windows_device: NULL argument");
        return -1;
    }
    return sharp_windows_call("phd_sharpness_windows_device", d_images, heights, widths, n_images, windows, window, 0,
                              d_sharpness, d_variance, stream);
}

extern "C" int phd_sharpness_maps_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                         int n_images, int window, int stride, double* const* d_sharpness,
                                         double* const* d_variance, void* stream) {
    return sharp_windows_call("phd_sharpness_maps_device", d_images, heights, widths, n_images, nullptr, window,
                              stride, d_sharpness, d_variance, stream);
}
#endif  // PHD_SHARPWIN_HOST_ONLY

// k_window_sharp's twin: the window's luma byte by byte, then the kernel's column
// code over every column and the shared finish.
extern "C" int phd_debug_window_sharpness_host(const uint8_t* rgb, int height, int width,
                                               const Crop_Boundaries* windows, int window, double* sharpness,
                                               double* variance, unsigned long long* sums) {
    clear_error();
    std::string why;
    if (!rgb) why = "NULL image";
    else if (sharp_size_why(window, &why)) {
        if (height < window || width < window) why = too_small(height, width, window);
        else if (sharp_list_why(windows, window, height, width, &why) && windows && windows->N > 0 && !sharpness)
            why = "NULL sharpness";
    }
    if (!why.empty()) {
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
