// box_stat_tiles.h -- the box statistics stage's records and row walk, host + device.
//
// The box statistics of a packed RGB8 image are, per crop box (rows top <= y <
// bottom, columns left <= x < right: crop_image, src/image_processing.c:244-266),
// get_rgb_statistics (src/image_processing.c:543-553) and get_hsv_average over
// rgb2hsv's s (src/image_processing.c:533-540, 372-417) of the box's pixels,
// from exact integer sums: a record of kBoxStatRec u64 per box,
//   M[6] (sum k, sum k^2 per channel) | n1 = #(min == 0 < max) | N | D[256]
// (D[m]: sum of max - min over the pixels whose max is m).
//
// The boxes are cut into items by box_plan (box_tiles.h): bands of whole rows
// of about kBoxBandElems pixels.  A row of an item is walked in units of 4
// pixels (12 bytes) from the row segment's first byte, 3 * (y * W + left) of
// an image base of any alignment -- every 4-byte phase occurs; a unit's three
// words are read at that address (stat_unit.h: stat_words), so every byte read
// is a pixel of the box.  The cols % 4 pixels at a row's end go one by one.  An
// item's units are taken in passes of at most kBoxStatPassUnits, each folded
// on its own, so no u32 partial of the device form can overflow (only a single
// row of more than 4 M pixels needs a second pass).  The kernel
// (box_stats.hip: k_box_stats) and the host twin (phd_boxstats.cpp:
// phd_debug_box_stats_host) walk box_plan's items with box_stat_units and
// box_stat_tails.
#pragma once

#include "box_tiles.h"
#include "stat_unit.h"

namespace phd {

// measured alternatives: make variant VFLAGS="-DPHD_BOXSTAT_THREADS=512 -DPHD_BOXSTAT_BATCH=8"
#if defined(PHD_BOXSTAT_THREADS)
constexpr int kBoxStatThreads = PHD_BOXSTAT_THREADS;
#else
constexpr int kBoxStatThreads = 256;
#endif
constexpr int kBoxStatRec = 264;                  // u64 per box: M[6], n1, N, D[256]
constexpr int kBoxStatOut = 8;                    // u64 per box downloaded: M[6], n1, bits of S
constexpr int kBoxStatPassUnits = 1 << 20;        // units of an item folded at once
#if defined(PHD_BOXSTAT_BATCH)
constexpr int kBoxStatBatch = PHD_BOXSTAT_BATCH;
#else
constexpr int kBoxStatBatch = 4;                  // units a device thread loads before it adds them
#endif

// One box of the launch: its image, the image's width and the box's columns.
struct BoxStatRec {
    const uint8_t* img;
    int w, left, right, pad;
};

// full units of one row of `cols` pixels
BOX_HD int box_stat_row_units(int cols) { return cols >> 2; }

// Walker t of nt over the units u0 <= u < u1 of an item (unit u is unit u % nu
// of row u / nu; base: the item's first row segment, pitch = 3 * W): units(q,
// m) for every batch of m <= B unit addresses.
template <int B, class Units>
BOX_HD void box_stat_units(const uint8_t* base, long long pitch, int nu, int u0, int u1, int t, int nt,
                           Units&& units) {
    int u = u0 + t;
    if (u >= u1) return;
    int row = u / nu, k = u - row * nu;
    const int dq = nt / nu, dr = nt - dq * nu;
    while (u < u1) {
        const uint8_t* q[B] = {};
        int m = 0;
        for (; m < B && u < u1; m++, u += nt) {
            q[m] = base + row * pitch + 12LL * k;
            k += dr;
            row += dq;
            if (k >= nu) {
                k -= nu;
                row++;
            }
        }
        units(q, m);
    }
}

// Walker t of nt over the cols % 4 last pixels of the item's `rows` rows: px(p).
template <class Px>
BOX_HD void box_stat_tails(const uint8_t* base, long long pitch, int cols, int rows, int t, int nt, Px&& px) {
    const int tl = cols & 3;
    if (!tl) return;
    const int n = rows * tl;                                // < 4 rows; rows * cols <= kBoxBandElems or one row
    for (int e = t; e < n; e += nt) {
        const int row = e / tl, j = e - row * tl;
        px(base + row * pitch + 3LL * ((cols & ~3) + j));
    }
}

// The sum S of the definition from a record's D: ascending m, sequential.
BOX_HD double box_stat_s(const unsigned long long* d) {
    double s = 0.0;
    for (int m = 1; m < 256; m++) s += (double)d[m] / (double)m;
    return s;
}

}  // namespace phd
