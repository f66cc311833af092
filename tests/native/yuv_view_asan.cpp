// ASan/UBSan driver for phd_yuv.cpp + yuv_view.h (tests/test_yuv_views.py): the
// host twin of the YCbCr conversion kernel -- the kernel's own row split,
// addresses, loads and stores -- over every layout of the YUV descriptor's
// table.  Each plane lives in a malloc of exactly its span (lowest to highest
// addressed byte, the last one flush with the end of the buffer); planes whose
// spans interleave (the Cb Cr pairs of NV12 / NV21, all three of YUY2 / UYVY)
// share one malloc of their joint span; each destination is a malloc of
// exactly 3*H*W bytes.  So a vector load over the last samples, a load rounded
// down to an aligned address or a store past the image is a report; UBSan's
// alignment check covers every 2- and 4-byte access.  Base offsets 1..3 put
// that many spare bytes in front of each span (malloc returns 16-byte aligned
// blocks); offset 0 is flush at both ends.  The bytes are checked against the
// plain per-pixel statement of the conversion (include/photohive_dsp.h).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../photohive_dsp_amd/csrc/yuv_plan.h"

enum Kind { kPlanar, kSemi, kQuad };

struct Layout {
    const char* name;
    Kind kind;
    int sx, sy;
    bool swap, flip, pitched, roi;
    int oy, ob, oc;          // kQuad: byte offsets of Y0, Cb, Cr in the 4-byte quad
};

static const Layout kLayouts[] = {
    {"i420", kPlanar, 1, 1, false, false, false, false, 0, 0, 0},
    {"yv12", kPlanar, 1, 1, true, false, false, false, 0, 0, 0},
    {"nv12", kSemi, 1, 1, false, false, false, false, 0, 0, 0},
    {"nv21", kSemi, 1, 1, true, false, false, false, 0, 0, 0},
    {"i422", kPlanar, 1, 0, false, false, false, false, 0, 0, 0},
    {"i444", kPlanar, 0, 0, false, false, false, false, 0, 0, 0},
    {"yuy2", kQuad, 1, 0, false, false, false, false, 0, 1, 3},
    {"uyvy", kQuad, 1, 0, false, false, false, false, 1, 0, 2},
    {"nv12_pitched", kSemi, 1, 1, false, false, true, false, 0, 0, 0},
    {"nv12_roi", kSemi, 1, 1, false, false, false, true, 0, 0, 0},
    {"i420_flipped", kPlanar, 1, 1, false, true, false, false, 0, 0, 0},
};

static unsigned g_seed = 2463534242u;

// a malloc of off + span random bytes; returns the block, *first = its byte `off`
static uint8_t* block(size_t off, size_t span, uint8_t** first) {
    uint8_t* b = (uint8_t*)malloc(off + span);
    for (size_t i = 0; i < off + span; i++) {
        g_seed ^= g_seed << 13, g_seed ^= g_seed >> 17, g_seed ^= g_seed << 5;
        b[i] = (uint8_t)(g_seed >> 11);
    }
    *first = b + off;
    return b;
}

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the definition, per pixel
static void reference(const phd_yuv_view& v, uint8_t* out) {
    static const int table[4][6] = {{65536, 91881, 22554, 46802, 116130, 0},
                                    {76309, 104597, 25675, 53279, 132201, 16},
                                    {65536, 103206, 12276, 30679, 121609, 0},
                                    {76309, 117489, 13975, 34925, 138438, 16}};
    const int* k = table[2 * v.matrix + v.range];
    const int sx = v.chroma_shift_x, sy = v.chroma_shift_y;
    const int ch = (v.height + sy) >> sy, cw = (v.width + sx) >> sx;
    for (int y = 0; y < v.height; y++)
        for (int x = 0; x < v.width; x++) {
            int C[2];
            for (int pl = 0; pl < 2; pl++) {
                const uint8_t* c = pl ? v.cr : v.cb;
                auto at = [&](int j, int i) { return (int)c[j * v.c_row_stride + i * v.c_pixel_stride]; };
                if (v.chroma == PHD_YUV_CHROMA_REPLICATE || sx == 0) {
                    C[pl] = at(y >> sy, x >> sx);
                    continue;
                }
                const int i = x >> 1, fi = clampi((x & 1) ? i + 1 : i - 1, 0, cw - 1);
                if (sy == 0) {
                    C[pl] = (3 * at(y, i) + at(y, fi) + ((x & 1) ? 2 : 1)) >> 2;
                    continue;
                }
                const int j = y >> 1, fj = clampi((y & 1) ? j + 1 : j - 1, 0, ch - 1);
                const int ti = 3 * at(j, i) + at(fj, i), tf = 3 * at(j, fi) + at(fj, fi);
                C[pl] = (3 * ti + tf + ((x & 1) ? 7 : 8)) >> 4;
            }
            const int Y = v.y[y * v.y_row_stride + x * v.y_pixel_stride];
            const int u = C[0] - 128, w = C[1] - 128, yy = k[0] * (Y - k[5]);
            uint8_t* o = out + 3 * ((size_t)y * v.width + x);
            o[0] = (uint8_t)clampi((yy + k[1] * w + 32768) >> 16, 0, 255);
            o[1] = (uint8_t)clampi((yy - k[2] * u - k[3] * w + 32768) >> 16, 0, 255);
            o[2] = (uint8_t)clampi((yy + k[4] * u + 32768) >> 16, 0, 255);
        }
}

int main() {
    const int shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {3, 5}, {5, 7}, {17, 67}, {33, 129}, {9, 515}};
    const int extras[] = {0, 1, 4};
    long cases = 0;
    for (const Layout& L : kLayouts)
        for (const auto& sh : shapes)
            for (int off = 0; off < 4; off++)
                for (int e : extras) {
                    const int h = sh[0], w = sh[1];
                    const int ch = (h + L.sy) >> L.sy, cw = (w + L.sx) >> L.sx;
                    phd_yuv_view v{};
                    v.height = h, v.width = w, v.chroma_shift_x = L.sx, v.chroma_shift_y = L.sy;
                    std::vector<uint8_t*> blocks;
                    uint8_t *p0, *p1, *p2;
                    if (L.kind == kPlanar) {
                        const int64_t yp = w + e, cp = cw + e;
                        blocks.push_back(block(off, (size_t)((h - 1) * yp + w), &p0));
                        blocks.push_back(block(off, (size_t)((ch - 1) * cp + cw), &p1));
                        blocks.push_back(block(off, (size_t)((ch - 1) * cp + cw), &p2));
                        if (L.swap) std::swap(p1, p2);
                        v.y = p0, v.cb = p1, v.cr = p2;
                        v.y_row_stride = yp, v.y_pixel_stride = 1, v.c_row_stride = cp, v.c_pixel_stride = 1;
                        if (L.flip) {                    // rows bottom-up: the pointers at the last row
                            v.y += (h - 1) * yp, v.cb += (ch - 1) * cp, v.cr += (ch - 1) * cp;
                            v.y_row_stride = -yp, v.c_row_stride = -cp;
                        }
                    } else if (L.kind == kSemi) {
                        const int fw = L.roi ? w + 10 : w;
                        const int64_t pitch = (fw > 2 * ((fw + 1) >> 1) ? fw : 2 * ((fw + 1) >> 1)) + e + (L.pitched ? 5 : 0);
                        blocks.push_back(block(off, (size_t)((h - 1) * pitch + w), &p0));
                        blocks.push_back(block(off, (size_t)((ch - 1) * pitch + 2 * cw), &p1));   // the pairs' joint span
                        v.y = p0, v.cb = p1 + (L.swap ? 1 : 0), v.cr = p1 + (L.swap ? 0 : 1);
                        v.y_row_stride = pitch, v.y_pixel_stride = 1, v.c_row_stride = pitch, v.c_pixel_stride = 2;
                    } else {
                        const int64_t pitch = 4 * cw + e;
                        // the joint span ends at the row's highest addressed byte of the three
                        int last = L.oy + 2 * (w - 1);
                        if (L.ob + 4 * (cw - 1) > last) last = L.ob + 4 * (cw - 1);
                        if (L.oc + 4 * (cw - 1) > last) last = L.oc + 4 * (cw - 1);
                        blocks.push_back(block(off, (size_t)((h - 1) * pitch + last + 1), &p0));
                        v.y = p0 + L.oy, v.cb = p0 + L.ob, v.cr = p0 + L.oc;
                        v.y_row_stride = pitch, v.y_pixel_stride = 2, v.c_row_stride = pitch, v.c_pixel_stride = 4;
                    }
                    const size_t n = (size_t)3 * h * w;
                    uint8_t* want = (uint8_t*)malloc(n);
                    for (int mode = 0; mode < 8; mode++) {
                        v.matrix = mode & 1, v.range = (mode >> 1) & 1, v.chroma = mode >> 2;
                        reference(v, want);
                        // destinations flush at both ends (16-byte aligned), and at
                        // byte offsets 1..3 flush at the end
                        for (int doff = 0; doff < 4; doff++) {
                            uint8_t* dst = (uint8_t*)malloc(doff + n);
                            memset(dst, 0xA5, doff + n);
                            std::string why;
                            if (phd::yuv_view_host(&v, dst + doff, &why) != 0 || memcmp(dst + doff, want, n) != 0) {
                                printf("MISMATCH %s %dx%d off %d extra %d mode %d doff %d %s\n", L.name, h, w, off, e,
                                       mode, doff, why.c_str());
                                return 1;
                            }
                            for (int k = 0; k < doff; k++)
                                if (dst[k] != 0xA5) {
                                    printf("WROTE BEFORE %s %dx%d off %d extra %d mode %d doff %d\n", L.name, h, w, off,
                                           e, mode, doff);
                                    return 1;
                                }
                            free(dst);
                            cases++;
                        }
                    }
                    free(want);
                    for (uint8_t* b : blocks) free(b);
                }
    // a bad view: refused with the field's name, nothing read
    phd_yuv_view bad{};
    uint8_t px[3];
    std::string why;
    if (phd::yuv_view_host(&bad, px, &why) != -1 || why.find("y is NULL") == std::string::npos) {
        printf("a NULL plane was not refused: %s\n", why.c_str());
        return 1;
    }
    printf("yuv view host OK (%ld cases)\n", cases);
    return 0;
}
