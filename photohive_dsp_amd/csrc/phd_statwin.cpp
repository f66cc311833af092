// phd_statwin.cpp -- window statistics: per T x T window (T = 16, 32, 64 or 128) of
// a packed RGB8 image get_rgb_statistics (src/image_processing.c:543-553, with
// get_average and get_variance, src/filtering.c:125-148) and get_hsv_average over
// rgb2hsv's s (src/image_processing.c:533-540, 372-417) on crop_image's crop
// (src/image_processing.c:244-266), left in device memory: seven doubles per
// window.  phd_stats_windows_device (window lists) and phd_stats_maps_device (a
// regular grid per image) through one body: every window of every image of a call
// in one launch; and the host twin phd_debug_window_stats_host.
// The entries' windows -- checks, counts and the walk that fills the table -- are a
// WindowPlan and the twin's checks window_twin_why (window_call.h); the launch goes
// through table_call (phd_host.h).
// The 4-pixel unit: stat_unit.h; the finish and the table: stat_window.h; kernel:
// window_stats.hip.
// With PHD_STATWIN_HOST_ONLY the twin compiles alone, without HIP
// (tests/native/window_stats_asan.cpp brings set_error and clear_error).

#include <cstring>
#include <string>

#ifdef PHD_STATWIN_HOST_ONLY
namespace phd {
void set_error(const std::string& msg);
void clear_error();
}  // namespace phd
#else
#include "phd_host.h"
#endif
#include "window_call.h"
#include "stat_unit.h"
#include "stat_window.h"

using namespace phd;

namespace {

bool stat_size_why(int window, std::string* why) {
    if (stw_size_ok(window)) return true;
    return *why = "window must be 16, 32, 64 or 128, not " + std::to_string(window), false;
}

}  // namespace

#ifndef PHD_STATWIN_HOST_ONLY
static_assert(kStatWinRec == kBoxStatRec, "the twin's sums in the box statistics' record layout");

// Both entries: the plan of their windows (lists, or a regular grid per image).
static int stat_windows_call(const char* entry, WindowPlan plan, double* const* d_stats, void* stream) {
    clear_error();
    std::string why;
    if (!plan.args_why(d_stats, &why) || !stat_size_why(plan.T, &why) ||
        !plan.build((const void* const*)d_stats, "d_stats", &why)) {
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
    const size_t o_dst = al(sizeof(StatWinRec) * nw), bytes = o_dst + sizeof(StatWinDst) * nw;
    auto fill = [&](uint8_t* h) {
        StatWinRec* recs = (StatWinRec*)h;
        StatWinDst* dst = (StatWinDst*)(h + o_dst);
        memset(h + sizeof(StatWinRec) * nw, 0, o_dst - sizeof(StatWinRec) * nw);
        size_t w = 0;
        plan.for_each([&](int i, long long k, long long top, long long left) {
            const long long pitch = 3LL * plan.widths[i];
            recs[w] = StatWinRec{plan.d_images[i] + top * pitch + 3 * left, (unsigned long long)pitch};
            dst[w++] = d_stats[i] + kStatWinOut * k;
        });
    };
    auto launch = [&](const uint8_t* d, hipStream_t st) {
        return launch_window_stats(T, (const StatWinRec*)d, (const StatWinDst*)(d + o_dst), (int)nw, st);
    };
    return table_call(c, stream, bytes, fill, launch, kWindowStats) ? 0 : -1;
}

extern "C" int phd_stats_windows_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                        int n_images, const Crop_Boundaries* const* windows, int window,
                                        double* const* d_stats, void* stream) {
    return stat_windows_call("phd_stats_windows_device",
                             WindowPlan(d_images, heights, widths, n_images, windows, true, window, 0), d_stats,
                             stream);
}

extern "C" int phd_stats_maps_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                     int n_images, int window, int stride, double* const* d_stats, void* stream) {
    return stat_windows_call("phd_stats_maps_device",
                             WindowPlan(d_images, heights, widths, n_images, nullptr, false, window, stride), d_stats,
                             stream);
}
#endif  // PHD_STATWIN_HOST_ONLY

// k_window_stats' twin: the window's units row by row in the 4-pixel unit's plain
// form (T is a multiple of 4: a row has no pixels left over for stat1_sums), then
// the shared finish over all 255 quotients.
extern "C" int phd_debug_window_stats_host(const uint8_t* rgb, int height, int width, const Crop_Boundaries* windows,
                                           int window, double* stats, unsigned long long* sums) {
    clear_error();
    std::string why, size_why;
    stat_size_why(window, &size_why);
    if (!window_twin_why(rgb, height, width, windows, window, size_why, stats, "NULL stats", &why)) {
        set_error("phd_debug_window_stats_host: " + why);
        return -1;
    }
    if (!windows || windows->N == 0) return 0;
    const int T = window;
    const unsigned long long npix = (unsigned long long)T * T;
    for (int k = 0; k < windows->N; k++) {
        const uint8_t* first = rgb + 3LL * ((long long)windows->top[k] * width + windows->left[k]);
        StatSums a{};
        unsigned long long d[256] = {};
        for (int y = 0; y < T; y++) {
            const uint8_t* row = first + 3LL * width * y;
            for (int u = 0; u < T / 4; u++) {
                unsigned w[3];
                stat_words(row + 12 * u, w);
                stat4_sums(w[0], w[1], w[2], a, d);
            }
        }
        double* out = stats + (size_t)kStatWinOut * k;
        for (int c = 0; c < 3; c++) {
            out[c] = stw_brightness(a.m[c], npix);
            out[3 + c] = stw_contrast(a.m[c], a.m[3 + c], npix);
        }
        out[6] = stw_sbar(stw_s(d), a.n1, npix);
        if (sums) {
            unsigned long long* rec = sums + (size_t)kStatWinRec * k;
            memcpy(rec, a.m, sizeof a.m);
            rec[6] = a.n1;
            rec[7] = npix;
            memcpy(rec + 8, d, sizeof d);
        }
    }
    return 0;
}
