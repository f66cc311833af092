// stat_window.h -- the window statistics' finish and launch table, host + device.
//
// The window statistics of a T x T window (T = 16, 32, 64 or 128; rows top <= y <
// top+T, columns left <= x < left+T: crop_image, src/image_processing.c:244-266)
// of a packed RGB8 image are get_rgb_statistics (src/image_processing.c:543-553,
// with get_average and get_variance, src/filtering.c:125-148) and get_hsv_average
// over rgb2hsv's s (src/image_processing.c:533-540, 372-417) of its n = T^2
// pixels, from the exact integer sums of stat_unit.h:
//   M[0..2] = sum k, M[3..5] = sum k^2 per channel; n1 = #(min == 0 < max);
//   D[m] = sum of max - min over the pixels whose max is m.
// At T = 128 every one fits a u32 (sum k^2 <= 16384 * 65025, D[m] <= 16384 * 255)
// and n M[3+c] - M[c]^2 fits a u64 (<= 1.8e13), so nothing needs 128 bits.
// The finish is the only floating point: the rows below, plain IEEE fp64 with no
// fused multiply-add, in the order of stats_from_sums (phd_assemble.cpp),
// box_stat_s (box_stat_tiles.h) and box_stat_finish (phd_boxstats.cpp):
//   B_c   = (double)M[c] / 255.0 / (double)n
//   C_c   = sqrt((double)(n M[3+c] - M[c]^2) / 65025.0 / ((double)n * (double)n))
//   S     = sum over m = 1..255 of (double)D[m] / (double)m, ascending, sequential
//   S-bar = (S - (1.0 - 0.999999) * (double)n1) / (double)n
// Every term of S is >= 0, so a zero term may be left out: the kernel
// (window_stats.hip: k_window_stats) forms the quotients in parallel and one wave
// adds the non-zero ones in ascending m; the host twin (phd_statwin.cpp:
// phd_debug_window_stats_host) adds all 255.  The sums are exact, so the two
// agree bit for bit wherever fp64 division and square root are correctly rounded.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define STW_HD __host__ __device__ __forceinline__
#else
#define STW_HD inline
#endif

namespace phd {

constexpr int kStatWinOut = 7;                    // doubles per window: Br Bg Bb Cr Cg Cb S-bar
constexpr int kStatWinRec = 264;                  // u64 per window of the twin's sums: kBoxStatRec's layout

STW_HD bool stw_size_ok(int T) { return T == 16 || T == 32 || T == 64 || T == 128; }

// ---- the finish ----------------------------------------------------------------------
STW_HD double stw_brightness(unsigned long long m, unsigned long long n) { return (double)m / 255.0 / (double)n; }

// m = sum k, q = sum k^2 over n pixels: n q >= m^2 (Cauchy-Schwarz), both below 2^45
STW_HD double stw_contrast(unsigned long long m, unsigned long long q, unsigned long long n) {
    const unsigned long long num = n * q - m * m;
    const double var = (double)num / 65025.0 / ((double)n * (double)n);
    return sqrt(var);
}

// D[m] / m, the term of bucket m >= 1
STW_HD double stw_quotient(unsigned long long d, int m) { return (double)d / (double)m; }

// S from a whole D: ascending m, sequential (box_stat_s's order)
STW_HD double stw_s(const unsigned long long* d) {
    double s = 0.0;
    for (int m = 1; m < 256; m++) s += stw_quotient(d[m], m);
    return s;
}

STW_HD double stw_sbar(double s, unsigned long long n1, unsigned long long n) {
    return (s - (1.0 - 0.999999) * (double)n1) / (double)n;
}

// ---- the launch table ------------------------------------------------------------------
// One 16-byte record and one 8-byte destination per window.
struct StatWinRec {
    const uint8_t* first;          // the window's first byte: image + 3 * (top * W + left)
    unsigned long long pitch;      // 3 * W
};
typedef double* StatWinDst;        // 8-byte aligned: the window's kStatWinOut doubles

}  // namespace phd
