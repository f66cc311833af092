// ASan/UBSan driver for the host half of phd_sharpwin.cpp (built with
// -DPHD_SHARPWIN_HOST_ONLY; tests/test_window_sharpness_host.py): the window
// sharpness kernel's host twin over heap images of exactly 3 * H * W bytes at each
// of the four window sizes, with windows flush to every edge, so a read past the
// last pixel of the last row (or before the first) is a report.  The values are
// checked against the plain two-pass form of get_variance_sharpness
// (src/filtering.c:151-183).
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

static double two_pass(const uint8_t* rgb, int width, int t, int l, int T, double* var) {
    std::vector<double> f((size_t)T * T);
    double acc = 0.0;
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++) {
            double dp = 0.0;
            for (int fy = 0; fy < 3; fy++)
                for (int fx = 0; fx < 3; fx++) {
                    const int iy = y + fy - 1, ix = x + fx - 1;
                    if (iy < 0 || iy >= T || ix < 0 || ix >= T) continue;
                    const uint8_t* p = rgb + 3 * ((size_t)(iy + t) * width + ix + l);
                    const double luma = 0.299 * (p[0] / 255.0) + 0.587 * (p[1] / 255.0) + 0.114 * (p[2] / 255.0);
                    dp += luma * ((fy == 1 && fx == 1) ? 8.0 : -1.0);
                }
            f[(size_t)y * T + x] = dp;
            acc += dp;
        }
    const double n = (double)T * T, avg = acc / n;
    double va = 0.0;
    for (double v : f) va += (v - avg) * (v - avg);
    *var = va / n;
    return (va / n) / avg;
}

static int run_size(int T, int H, int W) {
    uint8_t* img = (uint8_t*)malloc((size_t)3 * H * W);
    unsigned s = 12345u + (unsigned)T;
    for (size_t i = 0; i < (size_t)3 * H * W; i++) {
        s = s * 1664525u + 1013904223u;
        img[i] = (uint8_t)(32 + ((s >> 24) % 200));  // never black: every border ring has luma
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
    std::vector<double> sh(N, 0.0), va(N, 0.0);
    std::vector<unsigned long long> sums(2 * (size_t)N, 0ull);
    int bad = 0;
    if (phd_debug_window_sharpness_host(img, H, W, &cb, T, sh.data(), va.data(), sums.data()) != 0) {
        fprintf(stderr, "FAIL: T = %d: host twin returned an error: %s\n", T, phd::g_err.c_str());
        bad++;
    }
    for (int k = 0; k < N && !bad; k++) {
        double wv = 0.0;
        const double want = two_pass(img, W, top[k], lef[k], T, &wv);
        if (!(std::fabs(sh[k] - want) <= 1e-9 * std::fabs(want)) || !(std::fabs(va[k] - wv) <= 1e-9 * std::fabs(wv)) ||
            sums[2 * k] == 0) {
            fprintf(stderr, "FAIL: T = %d window %d: %.17g against %.17g, variance %.17g against %.17g\n", T, k, sh[k],
                    want, va[k], wv);
            bad++;
        }
    }
    if (!bad && (sh[0] != sh[N - 1] || va[0] != va[N - 1])) {
        fprintf(stderr, "FAIL: T = %d: the same window twice differs\n", T);
        bad++;
    }
    // only the sharpness asked for
    std::vector<double> only(N, 0.0);
    if (phd_debug_window_sharpness_host(img, H, W, &cb, T, only.data(), nullptr, nullptr) != 0 || only != sh) {
        fprintf(stderr, "FAIL: T = %d: without variance and sums\n", T);
        bad++;
    }
    // a window past the last row or column, or of another size, is refused, not read
    int t2[] = {H - T + 1}, b2[] = {H + 1}, l2[] = {0}, r2[] = {T};
    Crop_Boundaries below{1, t2, b2, l2, r2};
    int t3[] = {0}, b3[] = {T}, l3[] = {W - T + 1}, r3[] = {W + 1};
    Crop_Boundaries beside{1, t3, b3, l3, r3};
    int b4[] = {T + 1};
    Crop_Boundaries tall{1, t3, b4, l2, r2};
    if (phd_debug_window_sharpness_host(img, H, W, &below, T, sh.data(), nullptr, nullptr) != -1 ||
        phd_debug_window_sharpness_host(img, H, W, &beside, T, sh.data(), nullptr, nullptr) != -1 ||
        phd_debug_window_sharpness_host(img, H, W, &tall, T, sh.data(), nullptr, nullptr) != -1 ||
        phd_debug_window_sharpness_host(img, H, W, &cb, T + 1, sh.data(), nullptr, nullptr) != -1) {
        fprintf(stderr, "FAIL: T = %d: a bad window was accepted\n", T);
        bad++;
    }
    Crop_Boundaries none{0, nullptr, nullptr, nullptr, nullptr};
    if (phd_debug_window_sharpness_host(img, H, W, &none, T, nullptr, nullptr, nullptr) != 0) bad++;
    free(img);
    return bad;
}

int main() {
    int bad = 0;
    for (int T : {16, 32, 64, 128}) {
        bad += run_size(T, T + 3, T + 5);            // 3 * W is odd: every byte phase
        bad += run_size(T, T, T);                    // the image is the window
    }
    if (!bad) printf("window sharpness host OK\n");
    return bad;
}
