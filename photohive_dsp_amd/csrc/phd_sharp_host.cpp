// phd_sharp_host.cpp -- the batched sharpness stage's plan on the host, and its
// host-only twin phd_debug_sharpness_host (no HIP: this file and sharp_tiles.h
// compile alone, tests/native/sharpness_host_asan.cpp).
#include <string>
#include <vector>

#include "../../include/photohive_dsp.h"
#include "sharp_plan.h"

namespace phd {

// check_crops' rules (crop_pgm's bounds test, src/image_processing.c:215-218;
// an empty or inverted box makes the reference divide by zero / misallocate)
bool crops_why(const Crop_Boundaries* cb, int height, int width, std::string* why) {
    if (!cb) return true;
    if (cb->N < 0 || (cb->N > 0 && (!cb->top || !cb->bottom || !cb->left || !cb->right))) {
        *why = "Crop_Boundaries has NULL arrays";
        return false;
    }
    for (int k = 0; k < cb->N; k++) {
        const int t = cb->top[k], b = cb->bottom[k], l = cb->left[k], r = cb->right[k];
        if (r > width || l > width || b > height || t > height || l < 0 || r < 0 || t < 0 || b < 0 ||
            r <= l || b <= t) {
            *why = "crop boundaries outside of image boundaries (crop " + std::to_string(k) + ")";
            return false;
        }
    }
    return true;
}

bool sharp_plan(const Crop_Boundaries* const* crops, int n, bool flat, SharpPlan* p) {
    p->boxes.clear();
    p->prefix.assign(1, 0);
    p->max_boxes = 0;
    long total = 0;
    for (int i = 0; i < n; i++) {
        const Crop_Boundaries* cb = crops[i];
        if (!cb) continue;
        p->max_boxes = cb->N > p->max_boxes ? cb->N : p->max_boxes;
        for (int k = 0; k < cb->N; k++) {
            const SharpBox b{i, cb->top[k], cb->bottom[k], cb->left[k], cb->right[k],
                             flat ? (int)p->boxes.size() : k};
            total += sharp_slices(b);
            if (total > (1L << 30)) return false;
            p->boxes.push_back(b);
            p->prefix.push_back((int)total);
        }
    }
    return true;
}

namespace {

// (n, sum f, M2) of tile t of box b: filter_image's f (src/filtering.c:81-107)
// with the taps in (fy, fx) order, those outside the crop skipped
SharpPart tile_part(const uint8_t* rgb, int width, const SharpBox& b, long t, const double* k255) {
    const int cw = b.right - b.left, ch = b.bottom - b.top, tx = sharp_tiles_x(b);
    const int y0 = (int)(t / tx) * kSharpTileH, x0 = (int)(t % tx) * kSharpTileW;
    const int y1 = y0 + kSharpTileH < ch ? y0 + kSharpTileH : ch;
    const int x1 = x0 + kSharpTileW < cw ? x0 + kSharpTileW : cw;
    double f[kSharpTileH * kSharpTileW];
    int m = 0;
    double sum = 0.0;
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) {
            double dp = 0.0;
            for (int fy = 0; fy < 3; fy++)
                for (int fx = 0; fx < 3; fx++) {
                    const int iy = y + fy - 1, ix = x + fx - 1;
                    if (iy < 0 || iy >= ch || ix < 0 || ix >= cw) continue;
                    const uint8_t* px = rgb + 3 * ((size_t)(iy + b.top) * width + ix + b.left);
                    const double luma = 0.299 * k255[px[0]] + 0.587 * k255[px[1]] + 0.114 * k255[px[2]];
                    dp += luma * ((fy == 1 && fx == 1) ? 8.0 : -1.0);
                }
            f[m++] = dp;
            sum += dp;
        }
    const double mean = sum / (double)m;
    double m2 = 0.0;
    for (int i = 0; i < m; i++) {
        const double d = f[i] - mean;
        m2 += d * d;
    }
    return SharpPart{(double)m, sum, m2};
}

}  // namespace

SharpPart sharp_box_host(const uint8_t* rgb, int width, const SharpBox& b, const double* k255) {
    const long tiles = sharp_tiles(b);
    const int S = sharp_slices(b);
    SharpPart box{};
    for (int s = 0; s < S; s++) {
        SharpPart acc = tile_part(rgb, width, b, s, k255);
        for (long t = (long)s + S; t < tiles; t += S) sharp_merge(acc, tile_part(rgb, width, b, t, k255));
        if (s == 0) box = acc;
        else sharp_merge(box, acc);
    }
    return box;
}

}  // namespace phd

extern "C" int phd_debug_sharpness_host(const uint8_t* rgb, int height, int width, const Crop_Boundaries* crops,
                                        double* out) {
    using namespace phd;
    std::string why;
    if (!rgb || !crops || !out || height <= 0 || width <= 0 || !crops_why(crops, height, width, &why)) return -1;
    double k255[256];
    for (int k = 0; k < 256; k++) k255[k] = (double)k / 255.0;
    const Crop_Boundaries* one[1] = {crops};
    SharpPlan plan;
    if (!sharp_plan(one, 1, true, &plan)) return -1;
    for (size_t k = 0; k < plan.boxes.size(); k++) {
        const SharpBox& b = plan.boxes[k];
        const SharpPart p = sharp_box_host(rgb, width, b, k255);
        out[k] = sharp_value(p.sum, p.m2, b.right - b.left, b.bottom - b.top);
    }
    return 0;
}
