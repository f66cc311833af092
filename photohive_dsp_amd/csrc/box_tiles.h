// box_tiles.h -- the box palette stage's item plan and row code, host + device.
//
// The box palette of a label map (the lists of src/color_quantization.c:342-479
// kept per pixel, phd_internal.h) is, per crop box (rows top <= y < bottom,
// columns left <= x < right: crop_pgm's convention, src/image_processing.c:
// 213-232), the number of map elements of every palette slot: n_slots + 1
// uint32 counters, the last for PHD_LABEL_NONE and any label >= n_slots.
//
// Every box of a launch is cut into items: bands of whole rows of about
// kBoxBandElems elements (at least one row), in box order.  An item's rows are
// walked in units: unit k of a row covers the 8-byte word k of the row's
// memory counted from the row segment's start rounded down to 8 bytes -- four
// labels, read with one 8-byte load when the word lies inside the segment,
// else element by element (the head and tail of a row; `left`, the map's width
// and its 2-byte aligned base make every phase possible).  A unit merges equal
// adjacent labels before it adds.  The kernel (box_palette.hip: k_box_counts)
// and the host twin (phd_boxpal.cpp: phd_debug_box_counts_host) both walk
// box_plan's items with box_unit.
#pragma once

#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define BOX_HD __host__ __device__ __forceinline__
#else
#define BOX_HD inline
#endif

namespace phd {

constexpr int kBoxBandElems = 65536;             // elements of a band (an item), about
constexpr int kBoxMaxSlots = 4096;               // validate_config's group cap: no report has more slots
constexpr int kBoxThreads = 256;
// LDS counters of a block (32 KiB): as many private copies of an item's
// n_slots + 1 counters as fit, at most kBoxMaxCopies (one per lane of a wave:
// the lanes of a wave never share a copy, the block's four waves do)
constexpr int kBoxLdsCounters = 8192;
constexpr int kBoxMaxCopies = 64;

// One box of the launch: its map, the map's row length, its columns, the
// palette's slots and where its n_slots + 1 counters start in the output.
struct BoxRec {
    const uint16_t* map;
    long long out;
    int mw, left, right, n_slots;
};
// Rows row0 <= y < row1 of box `box`.
struct BoxItem {
    int box, row0, row1, pad;
};

BOX_HD int box_band_rows(int cols) { return cols >= kBoxBandElems ? 1 : kBoxBandElems / cols; }
// units of one row of `cols` elements, whatever its phase (the last may be empty)
BOX_HD int box_row_units(int cols) { return (cols + 6) / 4; }
// copies for an item of `units` units (a thread owns whole units)
BOX_HD int box_copies(int counters, int units) {
    int c = kBoxLdsCounters / counters;
    c = c > kBoxMaxCopies ? kBoxMaxCopies : c;
    return c > units ? units : c;
}

// Unit k of the row segment of n elements at row: add(slot, count) for every
// run of equal labels in it.
template <class Add>
BOX_HD void box_unit(const uint16_t* row, int n, int k, int n_slots, Add&& add) {
    const int off = (int)((reinterpret_cast<uintptr_t>(row) & 7) >> 1);
    const int e0 = 4 * k - off;
    if (e0 >= n) return;
    unsigned l[4] = {0, 0, 0, 0};
    int m = 0;
    if (e0 >= 0 && e0 + 4 <= n) {
        const unsigned long long q = *reinterpret_cast<const unsigned long long*>(row + e0);
        l[0] = (unsigned)(q & 0xFFFFu);
        l[1] = (unsigned)(q >> 16 & 0xFFFFu);
        l[2] = (unsigned)(q >> 32 & 0xFFFFu);
        l[3] = (unsigned)(q >> 48);
        m = 4;
    } else {
        const int lo = e0 < 0 ? 0 : e0, hi = e0 + 4 < n ? e0 + 4 : n;
        for (int i = lo; i < hi; i++) l[m++] = row[i];
    }
    const unsigned ns = (unsigned)n_slots;
    unsigned cur = l[0] < ns ? l[0] : ns, run = 1;
    for (int i = 1; i < m; i++) {
        const unsigned s = l[i] < ns ? l[i] : ns;
        if (s == cur) {
            run++;
        } else {
            add(cur, run);
            cur = s;
            run = 1;
        }
    }
    add(cur, run);
}

// The items of box b (rows top <= y < bottom, cols columns) appended to items.
inline void box_plan(int b, int top, int bottom, int cols, std::vector<BoxItem>* items) {
    if (bottom <= top || cols <= 0) return;
    const int rows = box_band_rows(cols);
    for (long long r = top; r < bottom; r += rows)
        items->push_back(BoxItem{b, (int)r, (int)(r + rows < bottom ? r + rows : bottom), 0});
}

}  // namespace phd
