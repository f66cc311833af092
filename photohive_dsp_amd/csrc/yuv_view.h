// yuv_view.h -- the input stage's conversion of one YCbCr row to packed RGB8,
// host + device.
//
// A phd_yuv_view (include/photohive_dsp.h: NV12 / NV21, planar 4:2:0, 4:2:2 and
// 4:4:4, packed YUY2 / UYVY, pitched, regions) is converted once into a packed
// RGB8 image (rows of 3*width bytes) by k_yuv_views (yuv_views.hip) and, with
// the same row code, on the host (phd_yuv.cpp: yuv_view_host).  Everything a
// row does -- its split into head, 4-pixel body units and tail, the addresses
// of every load and store, the chroma upsampling and the integer matrix -- is
// yuv_row below; the kernel calls it with a team of lanes, the host with a
// team of one.
//
// The conversion is defined in integers (the header's text; DESIGN.md section
// 18): chroma at a pixel by replication or by libjpeg's "fancy" triangle
// weights, then a 16.16 fixed-point matrix per (matrix, range) row.
//
// The span rule of pack_view.h holds per source row (the luma row and the one
// or two chroma rows a destination row reads): a vector access is taken only
// where each of its bytes is a byte the bytewise gather of that row would also
// touch, or lies between two such bytes:
//  - luma at pixel stride 1: the dword of pixels x0 .. x0+3;
//  - planar chroma: the two bytes of samples i0, i0+1 (4:2:x), the dword of
//    samples x0 .. x0+3 (4:4:4);
//  - NV12 / NV21: the dword Cb Cr Cb Cr of samples i0, i0+1;
//  - YUY2 / UYVY: the two dwords Y U Y V | Y U Y V of pixels x0 .. x0+3.
// Vector accesses are naturally aligned, never rounded down: where a row's
// source is not aligned at its first body unit that source goes bytewise for
// the whole row, as do the head, the tail and a triangle unit's two outer
// samples.  A body unit starts on an even pixel of a subsampled row, so a row
// whose destination is aligned on an odd pixel goes bytewise as a whole.
#pragma once

#include <stdint.h>

#include "pack_view.h"

namespace phd {

// chroma source forms of a view (YuvRec::lay), decided once per view
enum YuvLayout { kYuvGeneric = 0, kYuvPlanar = 1, kYuvPairs = 2, kYuvQuad = 3 };
// per-row chroma arithmetic
enum YuvMode { kYuvDirect = 0, kYuvReplicate = 1, kYuvTri422 = 2, kYuvTri420 = 3 };

// One view of a launch (the device table's record; 128 bytes).  Pointers and
// strides as in phd_yuv_view.
struct YuvRec {
    const uint8_t *y, *cb, *cr;
    uint8_t* dst;
    long long y_rs, y_ps, c_rs, c_ps;
    int height, width, ch, cw;      // luma size, chroma plane size
    int sx, sy;                     // chroma shifts
    int mode;                       // YuvMode
    int band_rows;                  // rows per block of the launch's (row band, view) grid
    int cy, crv, cgu, cgv, cbu, yoff;   // the matrix row
    int lay;                        // YuvLayout
    int shifts;                     // kYuvPairs / kYuvQuad: bit shifts of Y | Cb << 8 | Cr << 16 in the dword
};
static_assert(sizeof(YuvRec) == 128, "the device table's record");

typedef uint16_t __attribute__((may_alias)) pack_u16;

// cy, crv, cgu, cgv, cbu, yoff of (matrix, range): BT.601 full (JFIF, libjpeg's
// constants), BT.601 limited, BT.709 full, BT.709 limited
PACK_HD void yuv_coeffs(int matrix, int range, int* k) {
    const int t[4][6] = {{65536, 91881, 22554, 46802, 116130, 0},
                         {76309, 104597, 25675, 53279, 132201, 16},
                         {65536, 103206, 12276, 30679, 121609, 0},
                         {76309, 117489, 13975, 34925, 138438, 16}};
    for (int j = 0; j < 6; j++) k[j] = t[2 * matrix + range][j];
}

// clamp8(v >> 16) as clamp(v, 0, 2^24 - 1) >> 16: the same value (the shift is
// monotone), clamped before the shift.  Written shift-then-clamp, two
// neighbouring channels compile to gfx950's v_ashr_pk_u8_i32, and the k_yuv_views
// built that way stored 0xffff in the upper half of the dword it was OR-ed into.
PACK_HD uint32_t yuv_clamp8_16(int v) { return (uint32_t)(v < 0 ? 0 : v > 0xffffff ? 0xffffff : v) >> 16; }

// R | G << 8 | B << 16 of one pixel (int32 arithmetic, arithmetic shifts)
PACK_HD uint32_t yuv_rgb(const YuvRec& r, int Y, int Cb, int Cr) {
    const int u = Cb - 128, v = Cr - 128, yy = r.cy * (Y - r.yoff) + 32768;
    const uint32_t R = yuv_clamp8_16(yy + r.crv * v);
    const uint32_t G = yuv_clamp8_16(yy - r.cgu * u - r.cgv * v);
    const uint32_t B = yuv_clamp8_16(yy + r.cbu * u);
    return R | G << 8 | B << 16;
}

// The source rows of destination row y: luma, the chroma rows of j = y >> sy
// (near) and, for the 4:2:0 triangle, of j -+ 1 clamped to the plane (far).
struct YuvRows {
    const uint8_t *y, *cbn, *crn, *cbf, *crf;
    uint8_t* dst;
};

PACK_HD YuvRows yuv_rows(const YuvRec& r, int y) {
    YuvRows w;
    w.y = r.y + (long long)y * r.y_rs;
    const int j = y >> r.sy;
    int jf = j;
    if (r.mode == kYuvTri420) {
        jf = (y & 1) ? j + 1 : j - 1;
        jf = jf < 0 ? 0 : jf > r.ch - 1 ? r.ch - 1 : jf;
    }
    w.cbn = r.cb + (long long)j * r.c_rs;
    w.crn = r.cr + (long long)j * r.c_rs;
    w.cbf = r.cb + (long long)jf * r.c_rs;
    w.crf = r.cr + (long long)jf * r.c_rs;
    w.dst = r.dst + 3LL * r.width * y;
    return w;
}

// Upsampled chroma of pixel p of a unit from the samples s[0..3] = c[i0-1 ..
// i0+2] (near row n, far row f): sample k = 1 + (p >> 1), its far neighbour
// k - 1 for even p and k + 1 for odd p.
PACK_HD int yuv_upsample(int mode, const int* n, const int* f, int p) {
    const int k = 1 + (p >> 1), kf = (p & 1) ? k + 1 : k - 1;
    if (mode == kYuvTri422) return (3 * n[k] + n[kf] + ((p & 1) ? 2 : 1)) >> 2;
    if (mode == kYuvTri420) return (3 * (3 * n[k] + f[k]) + (3 * n[kf] + f[kf]) + ((p & 1) ? 7 : 8)) >> 4;
    return n[k];
}

// pixels [p0, p1) of a row, a byte at a time (every layout)
PACK_HD void yuv_row_bytes(const YuvRec& r, const YuvRows& w, int p0, int p1, int lane, int lanes) {
    const long long cps = r.c_ps;
    for (int x = p0 + lane; x < p1; x += lanes) {
        const int Y = w.y[(long long)x * r.y_ps];
        int Cb, Cr;
        if (r.mode <= kYuvReplicate) {
            const long long o = (long long)(x >> r.sx) * cps;
            Cb = w.cbn[o];
            Cr = w.crn[o];
        } else {
            const int i = x >> 1;
            int fi = (x & 1) ? i + 1 : i - 1;
            fi = fi < 0 ? 0 : fi > r.cw - 1 ? r.cw - 1 : fi;
            const long long oi = (long long)i * cps, of = (long long)fi * cps;
            if (r.mode == kYuvTri422) {
                const int rnd = (x & 1) ? 2 : 1;
                Cb = (3 * w.cbn[oi] + w.cbn[of] + rnd) >> 2;
                Cr = (3 * w.crn[oi] + w.crn[of] + rnd) >> 2;
            } else {
                const int rnd = (x & 1) ? 7 : 8;
                Cb = (3 * (3 * w.cbn[oi] + w.cbf[oi]) + (3 * w.cbn[of] + w.cbf[of]) + rnd) >> 4;
                Cr = (3 * (3 * w.crn[oi] + w.crf[oi]) + (3 * w.crn[of] + w.crf[of]) + rnd) >> 4;
            }
        }
        const uint32_t px = yuv_rgb(r, Y, Cb, Cr);
        uint8_t* d = w.dst + 3LL * x;
        d[0] = (uint8_t)px;
        d[1] = (uint8_t)(px >> 8);
        d[2] = (uint8_t)(px >> 16);
    }
}

// A row's split: pixels [0, head) bytewise, nvec body units of 4 pixels (12
// destination bytes, three aligned dwords), the tail bytewise; which of the
// row's sources take their vector form in the body.
struct YuvSplit {
    int head, nvec;
    bool quad;      // luma and chroma from the row's Y U Y V dwords
    bool ydword;    // luma dwords
    bool cvec;      // chroma: u16 / dword (planar), dword (pairs)
};

PACK_HD bool yuv_al(const uint8_t* p, long long off, unsigned mask) { return !(((uintptr_t)p + (uintptr_t)off) & mask); }

PACK_HD YuvSplit yuv_row_split(const YuvRec& r, const YuvRows& w) {
    YuvSplit s{r.width, 0, false, false, false};
    // dst_row + 3 p is dword aligned where p == dst_row (mod 4)
    const int head = (int)((uintptr_t)w.dst & 3);
    if (head + 4 > r.width) return s;
    if (r.sx && (head & 1)) return s;          // a unit starts on a chroma sample's first pixel
    s.head = head;
    s.nvec = (r.width - head) / 4;
    const long long i0 = head >> 1;
    const bool far = r.mode == kYuvTri420;
    if (r.lay == kYuvQuad) {
        const int sh_y = r.shifts & 0xff;
        const uint8_t* q = w.y - (sh_y >> 3);
        s.quad = yuv_al(q, 2LL * head, 3);
        return s;
    }
    s.ydword = r.y_ps == 1 && yuv_al(w.y, head, 3);
    if (r.lay == kYuvPairs) {
        const uint8_t* n = w.cbn < w.crn ? w.cbn : w.crn;
        const uint8_t* f = w.cbf < w.crf ? w.cbf : w.crf;
        s.cvec = yuv_al(n, 2 * i0, 3) && (!far || yuv_al(f, 2 * i0, 3));
    } else if (r.lay == kYuvPlanar) {
        const unsigned m = r.sx ? 1 : 3;
        const long long o = r.sx ? i0 : head;
        s.cvec = yuv_al(w.cbn, o, m) && yuv_al(w.crn, o, m) && (!far || (yuv_al(w.cbf, o, m) && yuv_al(w.crf, o, m)));
    }
    return s;
}

// The samples c[i0-1 .. i0+2] of one chroma row pair into b[0..3] (cb) and
// c[0..3] (cr); the outer two (clamped to the plane, bytewise) only when the
// mode filters horizontally.  4:4:4: the samples x0 .. x0+3 (i0 = x0).
PACK_HD void yuv_samples(const YuvRec& r, bool cvec, const uint8_t* cbrow, const uint8_t* crrow, int i0, int* b,
                         int* c) {
    const long long ps = r.c_ps;
    if (!r.sx) {
        if (cvec) {
            const uint32_t db = *(const pack_u32*)(cbrow + i0), dc = *(const pack_u32*)(crrow + i0);
            for (int k = 0; k < 4; k++) {
                b[k] = (db >> (8 * k)) & 0xff;
                c[k] = (dc >> (8 * k)) & 0xff;
            }
        } else {
            for (int k = 0; k < 4; k++) {
                b[k] = cbrow[(i0 + k) * ps];
                c[k] = crrow[(i0 + k) * ps];
            }
        }
        return;
    }
    if (cvec && r.lay == kYuvPairs) {
        const uint8_t* lo = cbrow < crrow ? cbrow : crrow;
        const uint32_t d = *(const pack_u32*)(lo + 2LL * i0);
        const int sb = (r.shifts >> 8) & 0xff, sc = (r.shifts >> 16) & 0xff;
        b[1] = (d >> sb) & 0xff;
        c[1] = (d >> sc) & 0xff;
        b[2] = (d >> (sb + 16)) & 0xff;
        c[2] = (d >> (sc + 16)) & 0xff;
    } else if (cvec) {
        const uint32_t db = *(const pack_u16*)(cbrow + i0), dc = *(const pack_u16*)(crrow + i0);
        b[1] = db & 0xff;
        b[2] = db >> 8;
        c[1] = dc & 0xff;
        c[2] = dc >> 8;
    } else {
        b[1] = cbrow[i0 * ps];
        c[1] = crrow[i0 * ps];
        b[2] = cbrow[(i0 + 1) * ps];
        c[2] = crrow[(i0 + 1) * ps];
    }
    if (r.mode >= kYuvTri422) {
        const long long il = i0 > 0 ? i0 - 1 : 0, ir = i0 + 2 < r.cw ? i0 + 2 : r.cw - 1;
        b[0] = cbrow[il * ps];
        c[0] = crrow[il * ps];
        b[3] = cbrow[ir * ps];
        c[3] = crrow[ir * ps];
    }
}

// Row y of view r by `lanes` cooperating lanes (this one is `lane`).
PACK_HD void yuv_row(const YuvRec& r, int y, int lane, int lanes) {
    const YuvRows w = yuv_rows(r, y);
    const YuvSplit s = yuv_row_split(r, w);
    const int sh_y = r.shifts & 0xff, sh_b = (r.shifts >> 8) & 0xff, sh_c = (r.shifts >> 16) & 0xff;
    for (int u = lane; u < s.nvec; u += lanes) {
        const int x0 = s.head + 4 * u, i0 = x0 >> r.sx;
        int Y[4], nb[4], nr[4], fb[4], fr[4];
        if (s.quad) {
            // Y U Y V | Y U Y V (any order of the four): pixels x0, x0+1 | x0+2, x0+3
            const pack_u32* in = (const pack_u32*)(w.y - (sh_y >> 3) + 2LL * x0);
            const uint32_t d0 = in[0], d1 = in[1];
            Y[0] = (d0 >> sh_y) & 0xff;
            Y[1] = (d0 >> (sh_y + 16)) & 0xff;
            Y[2] = (d1 >> sh_y) & 0xff;
            Y[3] = (d1 >> (sh_y + 16)) & 0xff;
            nb[1] = (d0 >> sh_b) & 0xff;
            nr[1] = (d0 >> sh_c) & 0xff;
            nb[2] = (d1 >> sh_b) & 0xff;
            nr[2] = (d1 >> sh_c) & 0xff;
            if (r.mode >= kYuvTri422) {
                const long long il = i0 > 0 ? i0 - 1 : 0, ir = i0 + 2 < r.cw ? i0 + 2 : r.cw - 1;
                nb[0] = w.cbn[il * r.c_ps];
                nr[0] = w.crn[il * r.c_ps];
                nb[3] = w.cbn[ir * r.c_ps];
                nr[3] = w.crn[ir * r.c_ps];
            }
        } else {
            if (s.ydword) {
                const uint32_t d = *(const pack_u32*)(w.y + x0);
                for (int p = 0; p < 4; p++) Y[p] = (d >> (8 * p)) & 0xff;
            } else {
                for (int p = 0; p < 4; p++) Y[p] = w.y[(long long)(x0 + p) * r.y_ps];
            }
            yuv_samples(r, s.cvec, w.cbn, w.crn, i0, nb, nr);
            if (r.mode == kYuvTri420) yuv_samples(r, s.cvec, w.cbf, w.crf, i0, fb, fr);
        }
        uint32_t px[4];
        for (int p = 0; p < 4; p++) {
            const int Cb = r.sx ? yuv_upsample(r.mode, nb, fb, p) : nb[p];
            const int Cr = r.sx ? yuv_upsample(r.mode, nr, fr, p) : nr[p];
            px[p] = yuv_rgb(r, Y[p], Cb, Cr);
        }
        pack_u32* out = (pack_u32*)(w.dst + 3LL * x0);
        out[0] = px[0] | px[1] << 24;            // r0 g0 b0 r1
        out[1] = px[1] >> 8 | px[2] << 16;       // g1 b1 r2 g2
        out[2] = px[2] >> 16 | px[3] << 8;       // b2 r3 g3 b3
    }
    yuv_row_bytes(r, w, 0, s.head, lane, lanes);
    yuv_row_bytes(r, w, s.head + 4 * s.nvec, r.width, lane, lanes);
}

// rows per block: about 16 KB of destination bytes (half the gather's band:
// measured no slower at 12 MP), at most the view; even for
// a vertically subsampled view, so that a band starts on an even row and both
// rows of a chroma row are the same block's
PACK_HD int yuv_band_rows(int height, int width, int sy) {
    const long long row = 3LL * width;
    long long rows = (16384 + row - 1) / row;
    if (rows > height) rows = height;
    if (rows < 1) rows = 1;
    if (sy && (rows & 1)) rows++;
    return (int)rows;
}

}  // namespace phd
