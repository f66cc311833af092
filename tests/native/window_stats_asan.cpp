// ASan/UBSan driver for the host half of phd_statwin.cpp (built with
// -DPHD_STATWIN_HOST_ONLY; tests/test_window_stats_host.py): the window statistics
// kernel's host twin over heap images of exactly 3 * H * W bytes at each of the
// four window sizes, with windows flush to every edge, so a read past the last
// pixel of the last row (or before the first) is a report.  The values are checked
// against the plain two-pass double form of get_rgb_statistics
// (src/image_processing.c:543-553; get_average and get_variance,
// src/filtering.c:125-148) and get_hsv_average over rgb2hsv's s
// (src/image_processing.c:533-540, 408-414) at the box statistics' bars.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/photohive_dsp.h"

// the library's error slot (phd_context.cpp there)
namespace phd {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
void clear_error() { g_err.clear(); }
}  // namespace phd

// Br Bg Bb Cr Cg Cb S-bar of the window at (t, l): doubles k / 255.0, two passes
static void two_pass(const uint8_t* rgb, int width, int t, int l, int T, double* out) {
    const double n = (double)T * T;
    double ssum = 0.0;
    for (int c = 0; c < 3; c++) {
        double acc = 0.0;
        for (int y = 0; y < T; y++)
            for (int x = 0; x < T; x++) acc += rgb[3 * ((size_t)(y + t) * width + x + l) + c] / 255.0;
        const double avg = acc / n;
        double va = 0.0;
        for (int y = 0; y < T; y++)
            for (int x = 0; x < T; x++) {
                const double v = rgb[3 * ((size_t)(y + t) * width + x + l) + c] / 255.0 - avg;
                va += v * v;
            }
        out[c] = avg;
        out[3 + c] = std::sqrt(va / n);
    }
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++) {
            const uint8_t* p = rgb + 3 * ((size_t)(y + t) * width + x + l);
            const double r = p[0] / 255.0, g = p[1] / 255.0, b = p[2] / 255.0;
            const double mx = std::max(r, std::max(g, b)), mn = std::min(r, std::min(g, b)), d = mx - mn;
            ssum += mx == 0 ? 0.0 : (d == mx ? 0.999999 : d / mx);
        }
    out[6] = ssum / n;
}

// assert_close's bars (tests/box_stats_cases.py): means and contrasts rtol 1e-9, the
// contrasts also atol max(1e-12, n 2^-53); S-bar rtol max(1e-12, n 2^-53)
static bool close(const double* got, const double* want, int T) {
    const double tol = std::max(1e-12, (double)T * T * std::ldexp(1.0, -53));
    for (int c = 0; c < 3; c++) {
        if (!(std::fabs(got[c] - want[c]) <= 1e-9 * std::fabs(want[c]))) return false;
        if (!(std::fabs(got[3 + c] - want[3 + c]) <= tol + 1e-9 * std::fabs(want[3 + c]))) return false;
    }
    return std::fabs(got[6] - want[6]) <= tol * std::fabs(want[6]);
}

static int run_size(int T, int H, int W) {
    uint8_t* img = (uint8_t*)malloc((size_t)3 * H * W);
    unsigned s = 54321u + (unsigned)T;
    for (size_t i = 0; i < (size_t)3 * H * W; i++) {
        s = s * 1664525u + 1013904223u;
        const unsigned v = s >> 24;
        img[i] = (uint8_t)(v % 7 == 0 ? 0 : v % 11 == 0 ? 255 : v);   // zero channels (the 0.999999 path) and 255s
    }
    //           corners, flush with one edge each, inside, the first again
    int top[] = {0, 0, H - T, H - T, 0, (H - T) / 2, H - T, (H - T) / 2, (H - T) / 3, 0};
    int lef[] = {0, W - T, 0, W - T, (W - T) / 2, 0, (W - T) / 3, W - T, (W - T + 1) / 2, 0};
    const int N = (int)(sizeof(top) / sizeof(top[0]));
    std::vector<int> bot(N), rig(N);
    for (int k = 0; k < N; k++) {
        bot[k] = top[k] + T;
        rig[k] = lef[k] + T;
    }
    Crop_Boundaries cb{N, top, bot.data(), lef, rig.data()};
    std::vector<double> st(7 * (size_t)N, -1.0);
    std::vector<unsigned long long> sums(264 * (size_t)N, 0ull);
    int bad = 0;
    if (phd_debug_window_stats_host(img, H, W, &cb, T, st.data(), sums.data()) != 0) {
        fprintf(stderr, "FAIL: T = %d: host twin returned an error: %s\n", T, phd::g_err.c_str());
        bad++;
    }
    for (int k = 0; k < N && !bad; k++) {
        double want[7];
        two_pass(img, W, top[k], lef[k], T, want);
        unsigned long long dsum = 0;
        for (int m = 0; m < 256; m++) dsum += sums[264 * (size_t)k + 8 + m];
        if (!close(&st[7 * (size_t)k], want, T) || sums[264 * (size_t)k + 7] != (unsigned long long)T * T ||
            dsum > 255ull * T * T) {
            fprintf(stderr, "FAIL: T = %d window %d:", T, k);
            for (int j = 0; j < 7; j++) fprintf(stderr, " %.17g against %.17g;", st[7 * (size_t)k + j], want[j]);
            fprintf(stderr, "\n");
            bad++;
        }
    }
    if (!bad && !std::equal(st.begin(), st.begin() + 7, st.end() - 7)) {
        fprintf(stderr, "FAIL: T = %d: the same window twice differs\n", T);
        bad++;
    }
    // only the values asked for
    std::vector<double> only(7 * (size_t)N, 0.0);
    if (phd_debug_window_stats_host(img, H, W, &cb, T, only.data(), nullptr) != 0 || only != st) {
        fprintf(stderr, "FAIL: T = %d: without sums\n", T);
        bad++;
    }
    // a window past the last row or column, or of another size, is refused, not read
    int t2[] = {H - T + 1}, b2[] = {H + 1}, l2[] = {0}, r2[] = {T};
    Crop_Boundaries below{1, t2, b2, l2, r2};
    int t3[] = {0}, b3[] = {T}, l3[] = {W - T + 1}, r3[] = {W + 1};
    Crop_Boundaries beside{1, t3, b3, l3, r3};
    int b4[] = {T + 1};
    Crop_Boundaries tall{1, t3, b4, l2, r2};
    if (phd_debug_window_stats_host(img, H, W, &below, T, st.data(), nullptr) != -1 ||
        phd_debug_window_stats_host(img, H, W, &beside, T, st.data(), nullptr) != -1 ||
        phd_debug_window_stats_host(img, H, W, &tall, T, st.data(), nullptr) != -1 ||
        phd_debug_window_stats_host(img, H, W, &cb, T + 1, st.data(), nullptr) != -1) {
        fprintf(stderr, "FAIL: T = %d: a bad window was accepted\n", T);
        bad++;
    }
    Crop_Boundaries none{0, nullptr, nullptr, nullptr, nullptr};
    if (phd_debug_window_stats_host(img, H, W, &none, T, nullptr, nullptr) != 0) bad++;
    free(img);
    return bad;
}

int main() {
    int bad = 0;
    for (int T : {16, 32, 64, 128}) {
        bad += run_size(T, T + 3, T + 5);            // 3 * W is odd: every byte phase
        bad += run_size(T, T, T);                    // the image is the window
    }
    if (!bad) printf("window statistics host OK\n");
    return bad;
}
