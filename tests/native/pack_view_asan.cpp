// ASan/UBSan driver for phd_views.cpp + pack_view.h (tests/test_views.py): the
// host twin of the pack kernel -- the kernel's own row split, addresses and
// shuffles -- over every layout of the view descriptor's table.  Each view
// lives in a malloc of exactly its span (lowest to highest addressed byte, the
// last row flush with the end of the buffer) and each destination in a malloc
// of exactly 3*H*W bytes, so a vector load over the last pixels, a load rounded
// down to an aligned address or a store past the image is a report; UBSan's
// alignment check covers every dword and 16-byte access.  Base offsets 1..3
// put that many spare bytes in front of the span (malloc returns 16-byte
// aligned blocks); offset 0 is flush at both ends.  The bytes are checked
// against the plain per-pixel gather (the reference reads its planes per
// pixel, src/image_processing.c:387).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../include/photohive_dsp.h"

struct Layout {
    const char* name;
    // (row, pixel, channel) strides of an h x w view whose pitch is its minimum + e
    void (*strides)(int h, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs);
};

static const Layout kLayouts[] = {
    {"hwc", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = 3 * w + e; *ps = 3; *cs = 1; }},
    {"rgba", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = 4 * w + e; *ps = 4; *cs = 1; }},
    {"bgr", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = 3 * w + e; *ps = 3; *cs = -1; }},
    {"bgra", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = 4 * w + e; *ps = 4; *cs = -1; }},
    {"chw", [](int h, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = w + e; *ps = 1; *cs = (int64_t)(w + e) * h + e; }},
    {"gray", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) { *rs = w + e; *ps = 1; *cs = 0; }},
    {"roi_hwc", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = 3 * (w + 9) + e; *ps = 3; *cs = 1; }},
    {"roi_rgba", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = 4 * (w + 9) + e; *ps = 4; *cs = 1; }},
    {"roi_chw", [](int h, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = w + 9 + e; *ps = 1; *cs = (int64_t)(w + 9 + e) * (h + 8); }},
    {"chw_flipped", [](int h, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = -(w + e); *ps = 1; *cs = (int64_t)(w + e) * h; }},
    {"hwc_mirrored", [](int, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = 3 * w + e; *ps = -3; *cs = 1; }},
    {"chw_bgr", [](int h, int w, int e, int64_t* rs, int64_t* ps, int64_t* cs) {
         *rs = w + e; *ps = 1; *cs = -(int64_t)(w + e) * h; }},
};

int main() {
    const int shapes[][2] = {{1, 1}, {1, 5}, {3, 4}, {5, 7}, {17, 67}, {16, 64}, {33, 129}};
    const int extras[] = {0, 1, 4};
    unsigned seed = 2463534242u;
    long cases = 0;
    for (const Layout& L : kLayouts)
        for (const auto& sh : shapes)
            for (int off = 0; off < 4; off++)
                for (int e : extras) {
                    const int h = sh[0], w = sh[1];
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
                    const size_t span = (size_t)(hi - lo + 1);
                    uint8_t* buf = (uint8_t*)malloc(off + span);
                    for (size_t i = 0; i < off + span; i++) {
                        seed ^= seed << 13, seed ^= seed >> 17, seed ^= seed << 5;
                        buf[i] = (uint8_t)(seed >> 11);
                    }
                    const uint8_t* data = buf + off - lo;
                    const size_t n = (size_t)3 * h * w;
                    uint8_t* want = (uint8_t*)malloc(n);
                    for (int y = 0; y < h; y++)
                        for (int x = 0; x < w; x++)
                            for (int c = 0; c < 3; c++)
                                want[3 * ((size_t)y * w + x) + c] = data[y * rs + x * ps + c * cs];
                    const phd_image_view v{data, h, w, rs, ps, cs};
                    // destinations flush at both ends (16-byte aligned), and at
                    // byte offsets 1..3 flush at the end
                    for (int doff = 0; doff < 4; doff++) {
                        uint8_t* dst = (uint8_t*)malloc(doff + n);
                        memset(dst, 0xA5, doff + n);
                        if (phd_debug_pack_view_host(&v, dst + doff) != 0 || memcmp(dst + doff, want, n) != 0) {
                            printf("MISMATCH %s %dx%d off %d extra %d doff %d\n", L.name, h, w, off, e, doff);
                            return 1;
                        }
                        for (int k = 0; k < doff; k++)
                            if (dst[k] != 0xA5) {
                                printf("WROTE BEFORE %s %dx%d off %d extra %d doff %d\n", L.name, h, w, off, e, doff);
                                return 1;
                            }
                        free(dst);
                        cases++;
                    }
                    free(want);
                    free(buf);
                }
    printf("pack view host OK (%ld cases)\n", cases);
    return 0;
}
