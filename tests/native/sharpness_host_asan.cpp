// ASan/UBSan driver for phd_sharp_host.cpp (tests/test_sharpness_batch.py): the
// host twin of the batched sharpness kernel on edge boxes of an exactly-sized
// heap image, so a read past the last pixel of the last row is a report.  The
// values are checked against the plain two-pass form of
// get_variance_sharpness (src/filtering.c:151-183).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/photohive_dsp.h"

static double two_pass(const uint8_t* rgb, int width, int t, int b, int l, int r) {
    const int ch = b - t, cw = r - l;
    std::vector<double> f((size_t)ch * cw);
    double acc = 0.0;
    for (int y = 0; y < ch; y++)
        for (int x = 0; x < cw; x++) {
            double dp = 0.0;
            for (int fy = 0; fy < 3; fy++)
                for (int fx = 0; fx < 3; fx++) {
                    const int iy = y + fy - 1, ix = x + fx - 1;
                    if (iy < 0 || iy >= ch || ix < 0 || ix >= cw) continue;
                    const uint8_t* p = rgb + 3 * ((size_t)(iy + t) * width + ix + l);
                    const double luma = 0.299 * (p[0] / 255.0) + 0.587 * (p[1] / 255.0) + 0.114 * (p[2] / 255.0);
                    dp += luma * ((fy == 1 && fx == 1) ? 8.0 : -1.0);
                }
            f[(size_t)y * cw + x] = dp;
            acc += dp;
        }
    const double n = (double)ch * cw, avg = acc / n;
    double va = 0.0;
    for (double v : f) va += (v - avg) * (v - avg);
    return (va / n) / avg;
}

int main() {
    const int H = 83, W = 131;                       // no multiple of the 64 x 16 tile
    uint8_t* img = (uint8_t*)malloc((size_t)3 * H * W);
    unsigned s = 12345u;
    for (size_t i = 0; i < (size_t)3 * H * W; i++) {
        s = s * 1664525u + 1013904223u;
        img[i] = (uint8_t)(32 + ((s >> 24) % 200));  // never black: every border ring has luma
    }
    //            1x1     row     column  whole  corner  tile+1  flush   2x2  one tile  tall
    int top[] =  {0,      0,      0,      0,     H - 1,  7,      H - 17, 1,   20,       0};
    int bot[] =  {1,      1,      H,      H,     H,      24,     H,      3,   36,       H};
    int lef[] =  {0,      0,      W - 1,  0,     W - 1,  3,      W - 65, 1,   64,       W - 2};
    int rig[] =  {1,      W,      W,      W,     W,      68,     W,      3,   128,      W};
    const int N = (int)(sizeof(top) / sizeof(top[0]));
    Crop_Boundaries cb{N, top, bot, lef, rig};
    std::vector<double> out(N, 0.0);
    int bad = 0;
    if (phd_debug_sharpness_host(img, H, W, &cb, out.data()) != 0) {
        fprintf(stderr, "FAIL: host twin returned an error\n");
        bad++;
    }
    for (int k = 0; k < N && !bad; k++) {
        const double want = two_pass(img, W, top[k], bot[k], lef[k], rig[k]);
        if (!(std::fabs(out[k] - want) <= 1e-9 * std::fabs(want))) {
            fprintf(stderr, "FAIL: box %d: %.17g against %.17g\n", k, out[k], want);
            bad++;
        }
    }
    // a box outside the image is refused, not read
    int t2[] = {0}, b2[] = {H + 1}, l2[] = {0}, r2[] = {W};
    Crop_Boundaries out_of_range{1, t2, b2, l2, r2};
    if (phd_debug_sharpness_host(img, H, W, &out_of_range, out.data()) != -1) {
        fprintf(stderr, "FAIL: a box past the last row was accepted\n");
        bad++;
    }
    Crop_Boundaries none{0, nullptr, nullptr, nullptr, nullptr};
    if (phd_debug_sharpness_host(img, H, W, &none, out.data()) != 0) bad++;
    free(img);
    if (!bad) printf("sharpness host OK\n");
    return bad;
}
