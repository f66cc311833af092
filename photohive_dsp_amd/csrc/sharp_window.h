// sharp_window.h -- the window sharpness's row code and finish, host + device.
//
// A window is a T x T crop (T = 16, 32, 64 or 128) of a packed RGB8 image, rows
// top <= y < top + T and columns left <= x < left + T (crop_pgm's convention,
// src/image_processing.c:213-232).  Its sharpness is the reference's
// get_variance_sharpness (src/filtering.c:151-183) on that crop of the
// full-resolution luma: rgb2pgm (src/image_processing.c:505-512), the 3 x 3
// Laplacian with the taps outside the crop skipped (filter_image,
// src/filtering.c:81-107), then variance / average (get_average and
// get_variance, :125-148).  For 8-bit images every term is an integer:
//   l(y, x) = 299 R + 587 G + 114 B         the luma times 255000, <= 255000
//   f(y, x) = 9 l(y, x) - sum of l over the 3 x 3 neighbourhood inside the
//             window (the centre weighs 8, each neighbour inside -1;
//             |f| <= 2,040,000)
//   n = T^2, S1 = sum f, S2 = sum f^2       S1 >= 0 (only the border ring
//                                           contributes) and fits 32 bits, S2 a u64
//   D = n S2 - S1^2                         never negative, 128 bits (ShwU128)
// and the finish is the only floating point (plain IEEE fp64, no fma):
//   num       = (double)D.hi * 2^64 + (double)D.lo
//   sharpness = num / (((double)n * (double)S1) * 255000.0)
//   variance  = num / (((double)n * (double)n) * 65025000000.0)
// S1 == 0 (a black border ring) divides by zero as IEEE does: NaN when D == 0,
// +inf otherwise.
// The kernel (window_sharp.hip: k_window_sharp) and the host twin
// (phd_sharpwin.cpp: phd_debug_window_sharpness_host) run the same functions over
// a window's T x T luma; the sums are exact, so the two agree bit for bit.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SHW_HD __host__ __device__ __forceinline__
#else
#define SHW_HD inline
#endif

namespace phd {

SHW_HD bool shw_size_ok(int T) { return T == 16 || T == 32 || T == 64 || T == 128; }

// rgb2pgm times 255000
SHW_HD int shw_luma(unsigned r, unsigned g, unsigned b) { return (int)(299u * r + 587u * g + 114u * b); }

// The luma of a 4-pixel unit from its 12 bytes as three little-endian words
// (r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3)
SHW_HD void shw_unit_luma(unsigned w0, unsigned w1, unsigned w2, int* l) {
    l[0] = shw_luma(w0 & 255u, w0 >> 8 & 255u, w0 >> 16 & 255u);
    l[1] = shw_luma(w0 >> 24, w1 & 255u, w1 >> 8 & 255u);
    l[2] = shw_luma(w1 >> 16 & 255u, w1 >> 24, w2 & 255u);
    l[3] = shw_luma(w2 >> 8 & 255u, w2 >> 16 & 255u, w2 >> 24);
}

// Row y of the window's luma (T ints a row) about column x: l(y, x-1) + l(y, x) +
// l(y, x+1) with the positions outside the window 0, and the centre in *c
SHW_HD int shw_row3(const int* luma, int T, int y, int x, int* c) {
    if (y < 0 || y >= T) return *c = 0, 0;
    const int* r = luma + y * T;
    const int m = r[x];
    *c = m;
    return (x > 0 ? r[x - 1] : 0) + m + (x + 1 < T ? r[x + 1] : 0);
}

// Rows y0 <= y < y0 + rows of column x: f added to *s1 and f^2 to *s2
SHW_HD void shw_column(const int* luma, int T, int x, int y0, int rows, long long* s1, unsigned long long* s2) {
    int ca, cb, cc;
    int ha = shw_row3(luma, T, y0 - 1, x, &ca), hb = shw_row3(luma, T, y0, x, &cb);
    long long a1 = 0;
    unsigned long long a2 = 0;
    for (int y = y0; y < y0 + rows; y++) {
        const int hc = shw_row3(luma, T, y + 1, x, &cc);
        const int f = 9 * cb - (ha + hb + hc);
        a1 += f;
        a2 += (unsigned long long)((long long)f * f);
        ha = hb;
        hb = hc;
        cb = cc;
    }
    *s1 += a1;
    *s2 += a2;
}

// ---- D = n S2 - S1^2 in 128 bits ---------------------------------------------------
struct ShwU128 {
    unsigned long long hi, lo;
};
SHW_HD unsigned long long shw_mulhi(unsigned long long a, unsigned long long b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#endif
}
SHW_HD ShwU128 shw_d(unsigned long long n, unsigned long long s1, unsigned long long s2) {
    const unsigned long long ah = shw_mulhi(n, s2), al = n * s2;
    const unsigned long long bh = shw_mulhi(s1, s1), bl = s1 * s1;
    ShwU128 d;
    d.lo = al - bl;
    d.hi = ah - bh - (al < bl ? 1ull : 0ull);
    return d;
}

// ---- the finish ------------------------------------------------------------------------
SHW_HD double shw_num(ShwU128 d) { return (double)d.hi * 18446744073709551616.0 + (double)d.lo; }
SHW_HD double shw_sharpness(double num, unsigned long long n, unsigned long long s1) {
    return num / (((double)n * (double)s1) * 255000.0);
}
SHW_HD double shw_variance(double num, unsigned long long n) {
    return num / (((double)n * (double)n) * 65025000000.0);
}

// ---- the launch table --------------------------------------------------------------------
// One record and one destination pair per window, 16 bytes each.
struct SharpWinRec {
    const uint8_t* first;          // the window's first byte: image + 3 * (top * W + left)
    // 3 * W << 2 | edge: bit 0, the window's first byte is its image's first (the
    // dword holding it may begin before the image); bit 1, its last byte is the
    // image's last (the dword holding it may end behind the image)
    unsigned long long pitch_edge;
};
struct SharpWinDst {
    double* sharpness;             // 8-byte aligned
    double* variance;              // 8-byte aligned, or NULL
};

}  // namespace phd
