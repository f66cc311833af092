// pal_window.h -- the window palettes' unit, copies rule, dominant key and launch
// table, host + device.
//
// The window palette of a T x T window (T = 16, 32, 64 or 128; rows top <= y <
// top+T, columns left <= x < left+T of a palette label map, the lists of
// src/color_quantization.c:342-479 kept per pixel, inside crop_pgm's box,
// src/image_processing.c:213-232) is the box palette (box_tiles.h) restricted to
// square windows, left in device memory:
//   counts[s], s < n_slots: the window's elements whose label is s;
//   counts[n_slots]:        every other element (PHD_LABEL_NONE, any label >= n_slots);
//   dominant:               the column of the largest count, the lowest on a tie,
//                           written as s for s < n_slots and PHD_LABEL_NONE for
//                           column n_slots.
// All integers: a window's values depend on its T^2 labels and n_slots alone.
// A window is walked in units of four labels (T is a multiple of 4: T / 4 units a
// row, none left over), each read as the 8 bytes at its own 2-byte aligned
// address; a unit merges equal adjacent labels before it adds (box_unit's rule).
// The kernel (window_palette.hip: k_window_palette) and the host twin
// (phd_palwin.cpp: phd_debug_window_palette_host) share pw_unit and pw_key.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PW_HD __host__ __device__ __forceinline__
#else
#define PW_HD inline
#endif

namespace phd {

constexpr int kPalWinMaxSlots = 4096;             // kBoxMaxSlots: no report has more slots
constexpr int kPalWinMaxCounters = kPalWinMaxSlots + 1;
constexpr unsigned kPalWinNone = 0xFFFFu;         // PHD_LABEL_NONE

PW_HD bool pw_size_ok(int T) { return T == 16 || T == 32 || T == 64 || T == 128; }

// ---- the copies rule ----------------------------------------------------------------------
// A window's LDS histogram has `copies` private copies of its n_slots + 1 counters,
// thread t of the window adding into copy t % copies, so that the lanes of a wave
// that meet on one counter (a single-label window: every lane) are 64 / copies.
// The most the window's threads can use -- 16 for the 256 threads of a 64- or
// 128-px window, 4 for the one wave of a 16- or 32-px window (k_window_stats'
// measured choice for the same shapes: more copies cost their zeroing and their
// fold per window) -- halved until the copies fit kPalWinLdsWords counters.  The
// common palettes of up to 127 slots get all of them; from 1024 slots on, and so
// at 4096, there is one copy.
constexpr int kPalWinLdsWords = 2048;             // a window's copies, unless one copy alone is larger
PW_HD int pw_max_copies(int T) { return T >= 64 ? 16 : 4; }
PW_HD int pw_copies(int counters, int T) {
    int c = pw_max_copies(T);
    while (c > 1 && c * counters > kPalWinLdsWords) c >>= 1;
    return c;
}
// words from one copy to the next: odd, so that a counter's copies lie in different
// LDS banks (k_window_stats pads its 256 buckets to 257 for the same reason)
PW_HD int pw_copy_stride(int counters) { return counters | 1; }
// LDS words of a window with `counters` counters, a multiple of 4 (zeroed as uint4)
PW_HD int pw_lds_words(int counters, int T) {
    return (pw_copies(counters, T) * pw_copy_stride(counters) + 3) & ~3;
}
// pw_lds_words' maximum: one copy of 4097 (several copies take at most 2048 + 16)
constexpr int kPalWinMaxLdsWords = (kPalWinMaxCounters + 3) & ~3;
static_assert(kPalWinLdsWords + 16 <= kPalWinMaxLdsWords, "pw_lds_words' maximum");

// ---- the unit --------------------------------------------------------------------------------
// Four labels as the little-endian u64 of their 8 bytes: add(column, count) for
// every run of equal columns, labels >= n_slots clamped to column n_slots.
template <class Add>
PW_HD void pw_unit(unsigned long long q, unsigned n_slots, Add&& add) {
    const unsigned l0 = (unsigned)(q & 0xFFFFu), l1 = (unsigned)(q >> 16 & 0xFFFFu);
    const unsigned l2 = (unsigned)(q >> 32 & 0xFFFFu), l3 = (unsigned)(q >> 48);
    const unsigned s[4] = {l0 < n_slots ? l0 : n_slots, l1 < n_slots ? l1 : n_slots, l2 < n_slots ? l2 : n_slots,
                           l3 < n_slots ? l3 : n_slots};
    unsigned cur = s[0], run = 1;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 1; i < 4; i++) {
        if (s[i] == cur) {
            run++;
        } else {
            add(cur, run);
            cur = s[i];
            run = 1;
        }
    }
    add(cur, run);
}

// ---- the dominant key ---------------------------------------------------------------------
// key = count * 8192 + (8191 - column): the maximum over the columns is the largest
// count at the lowest column.  count <= 128^2 = 2^14 and column <= 4096 < 2^13.
static_assert(128LL * 128 * 8192 + 8191 < (1LL << 32), "the key of a 128-px window's largest count fits a u32");
static_assert(kPalWinMaxSlots <= 8191, "a column fits the key's low 13 bits");
PW_HD unsigned pw_key(unsigned count, unsigned column) { return count * 8192u + (8191u - column); }
// the label of a key's column: the slot, or PHD_LABEL_NONE for column n_slots
PW_HD unsigned pw_key_label(unsigned key, unsigned n_slots) {
    const unsigned column = 8191u - (key & 8191u);
    return column < n_slots ? column : kPalWinNone;
}

// ---- the launch table ----------------------------------------------------------------------
// One 24-byte record and one 16-byte destination per window.
struct PalWinRec {
    const uint16_t* first;         // the window's first label: map + top * mw + left
    unsigned long long pitch;      // mw, in labels
    int n_slots, pad;              // the window's own palette
};
struct PalWinDst {
    uint32_t* counts;              // 4-byte aligned: the window's n_slots + 1 counters, or NULL
    uint16_t* dominant;            // 2-byte aligned: the window's dominant label, or NULL
};

}  // namespace phd
