// ASan/UBSan driver for phd_views.cpp + decode_view.h (tests/test_typed_views.py):
// the host twin of the typed views' decode kernels -- the kernels' own row
// split, addresses, loads and stores -- over every element type and every
// layout of the descriptor's table.  Each view lives in a malloc of exactly
// its span (lowest to highest addressed element, the last one flush with the
// end of the buffer), the planes in a malloc of exactly 3*H*W doubles and the
// RGB8 bytes in exactly 3*H*W bytes, so a 16-byte load over the last pixels, a
// load rounded down to an aligned address or a store past the planes is a
// report; UBSan's alignment check covers every element, dword and 16-byte
// access.  Base offsets 1..3 put that many spare elements in front of the
// span (malloc returns 16-byte aligned blocks); offset 0 is flush at both
// ends.  The doubles are checked against the plain per-pixel decode (the
// reference reads its planes per pixel, src/image_processing.c:387).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>

#include "../../photohive_dsp_amd/csrc/views_plan.h"

struct Layout {
    const char* name;
    // (row, pixel, channel) strides in elements of an h x w view whose pitch is its minimum + e
    void (*strides)(int h, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs);
};

static const Layout kLayouts[] = {
    {"hwc", [](int, int w, int, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = 3 * w; *ps = 3; *cs = 1; }},
    {"hwc_pitched", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = 3 * w + 1 + e; *ps = 3; *cs = 1; }},
    {"rgba", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = 4 * w + e; *ps = 4; *cs = 1; }},
    {"bgr", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = 3 * w + e; *ps = 3; *cs = -1; }},
    {"bgra", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = 4 * w + e; *ps = 4; *cs = -1; }},
    {"chw", [](int h, int w, int, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = w; *ps = 1; *cs = (int64_t)w * h; }},
    {"chw_pitched", [](int h, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = w + 3 + e; *ps = 1; *cs = (int64_t)(w + 3 + e) * h + e; }},
    {"roi_hwc", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = 3 * (w + 9) + e; *ps = 3; *cs = 1; }},
    {"roi_chw", [](int h, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = w + 9 + e; *ps = 1; *cs = (int64_t)(w + 9 + e) * (h + 8); }},
    {"gray", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = w + e; *ps = 1; *cs = 0; }},
    {"chw_flipped", [](int h, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = -(w + e); *ps = 1; *cs = (int64_t)(w + e) * h; }},
    {"hwc_mirrored", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = 3 * w + e; *ps = -3; *cs = 1; }},
};

// the plain decode of one element
static double plain_value(int elem, const uint8_t* p, double mv) {
    switch (elem) {
    case PHD_ELEM_U8: return (double)*p / mv;
    case PHD_ELEM_U16: {
        uint16_t x;
        memcpy(&x, p, 2);
        return (double)x / mv;
    }
    case PHD_ELEM_F16: {
        uint16_t x;
        memcpy(&x, p, 2);
        const int e = (x >> 10) & 31, m = x & 1023;
        double v = e == 0 ? std::ldexp((double)m, -24)
                   : e == 31 ? (m ? NAN : INFINITY)
                             : std::ldexp((double)(m + 1024), e - 25);
        return (x & 0x8000 ? -v : v) / mv;
    }
    case PHD_ELEM_F32: {
        float x;
        memcpy(&x, p, 4);
        return (double)x / mv;
    }
    default: {
        double x;
        memcpy(&x, p, 8);
        return x / mv;
    }
    }
}

int main() {
    const int shapes[][2] = {{1, 1}, {1, 7}, {5, 1}, {3, 5}, {37, 61}, {64, 64}};
    const int sizes[] = {1, 2, 2, 4, 8};
    const double maxes[] = {0.0, 1023.0, 255.0};
    const double own[] = {255.0, 65535.0, 1.0, 1.0, 1.0};
    unsigned seed = 2463534242u;
    long cases = 0;
    for (int elem = 0; elem < 5; elem++)
        for (const Layout& L : kLayouts)
            for (const auto& sh : shapes)
                for (int off = 0; off < 4; off++) {
                    const int h = sh[0], w = sh[1], es = sizes[elem], e = off % 2 * 4 + off / 2;
                    int64_t rs, ps, cs;
                    L.strides(h, w, e, &rs, &ps, &cs);
                    int64_t lo = 0, hi = 0;
                    for (int y : {0, h - 1})
                        for (int x : {0, w - 1})
                            for (int c : {0, 2}) {
                                const int64_t a = y * rs + x * ps + c * cs;
                                lo = a < lo ? a : lo;
                                hi = a > hi ? a : hi;
                            }
                    const size_t bytes = (size_t)(off + hi - lo + 1) * es;
                    uint8_t* buf = (uint8_t*)malloc(bytes);
                    for (size_t i = 0; i < bytes; i++) {
                        seed ^= seed << 13, seed ^= seed >> 17, seed ^= seed << 5;
                        buf[i] = (uint8_t)(seed >> 11);
                    }
                    const uint8_t* data = buf + (off - lo) * es;
                    const size_t n = (size_t)h * w;
                    const double mv_in = maxes[cases % 3], mv = mv_in != 0.0 ? mv_in : own[elem];
                    const phd_typed_view v{data, h, w, rs * es, ps * es, cs * es, elem, (int)(cases & 1), mv_in};
                    double* planes = (double*)malloc(3 * n * sizeof(double));
                    uint8_t* rgb8 = (uint8_t*)malloc(3 * n);
                    int is_u8 = -1;
                    std::string why;
                    if (phd::decode_view_host(&v, planes, cases % 5 == 4 ? nullptr : rgb8, &is_u8, &why) != 0) {
                        printf("FAILED %s elem %d %dx%d off %d: %s\n", L.name, elem, h, w, off, why.c_str());
                        return 1;
                    }
                    for (int y = 0; y < h; y++)
                        for (int x = 0; x < w; x++)
                            for (int c = 0; c < 3; c++) {
                                const double want = plain_value(elem, data + (y * rs + x * ps + c * cs) * es, mv);
                                const double got = planes[c * n + (size_t)y * w + x];
                                if (memcmp(&want, &got, 8) != 0 && !(want != want && got != got)) {
                                    printf("MISMATCH %s elem %d %dx%d off %d at (%d, %d, %d): %a != %a\n", L.name,
                                           elem, h, w, off, y, x, c, got, want);
                                    return 1;
                                }
                            }
                    free(rgb8);
                    free(planes);
                    free(buf);
                    cases++;
                }
    // a bad view is refused before any access
    const phd_typed_view bad{(const void*)16, 4, 4, 48, 12, 4, 9, 0, 0.0};
    double d[1];
    std::string why;
    if (phd::decode_view_host(&bad, d, nullptr, nullptr, &why) != -1 || why.find("elem") == std::string::npos) {
        printf("bad elem accepted\n");
        return 1;
    }
    printf("decode view host OK (%ld cases)\n", cases);
    return 0;
}
