// stat_unit.h -- the 4-pixel unit of the RGB statistics passes, shared by
// stats.hip (k_rgb_stats: whole images) and box_stats.hip (k_box_stats: crop
// boxes), and its plain C++ form for the host twin (phd_boxstats.cpp).
//
// A unit is 4 packed RGB8 pixels = 12 bytes = 3 little-endian words.  Per unit:
// the channel moments (sum k, sum k^2: get_rgb_statistics,
// src/image_processing.c:543-553), and for rgb2hsv's s (src/image_processing.c:
// 408-414) d = max - min added to bucket max of a 256-bucket histogram plus the
// count of min == 0 < max pixels (the 0.999999 path) -- stats.hip's header has
// the derivation.  All of it is exact integer arithmetic, so the device form
// (v_perm regrouping, v_dot2_u32_u16, one u32 LDS atomic per pixel) and the
// plain form below give the same sums.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define STAT_HD __host__ __device__ __forceinline__
#else
#define STAT_HD inline
#endif

namespace phd {

// The unit's three words from any byte address (all 12 bytes are the unit's own:
// nothing outside them is read).  On gfx950 this is one global_load_dwordx3 at
// the unaligned address.
STAT_HD void stat_words(const uint8_t* q, unsigned* w) { __builtin_memcpy(w, q, 12); }

// ---- plain form: exact u64 sums ------------------------------------------------
// m[0..2] sum k, m[3..5] sum k^2 per channel; n1 = #(min == 0 < max); d[256]
struct StatSums {
    unsigned long long m[6], n1;
};

STAT_HD void stat1_sums(unsigned r, unsigned g, unsigned b, StatSums& a, unsigned long long* d) {
    a.m[0] += r; a.m[1] += g; a.m[2] += b;
    a.m[3] += r * r; a.m[4] += g * g; a.m[5] += b * b;
    const unsigned mx = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const unsigned mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
    d[mx] += mx - mn;
    a.n1 += mn == 0 && mx != 0;
}

STAT_HD void stat4_sums(unsigned w0, unsigned w1, unsigned w2, StatSums& a, unsigned long long* d) {
    stat1_sums(w0 & 255u, w0 >> 8 & 255u, w0 >> 16 & 255u, a, d);
    stat1_sums(w0 >> 24, w1 & 255u, w1 >> 8 & 255u, a, d);
    stat1_sums(w1 >> 16 & 255u, w1 >> 24, w2 & 255u, a, d);
    stat1_sums(w2 >> 8 & 255u, w2 >> 16 & 255u, w2 >> 24, a, d);
}

#if defined(__HIPCC__)
// ---- device form ---------------------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 as_u16x2(unsigned x) { return __builtin_bit_cast(u16x2, x); }

struct StatAcc {
    unsigned sr, sg, sb, qr, qg, qb;         // per-thread moments of the run (u32: <= 1024 items)
    double s64;                              // the partial final group's s (fp64)
    u16x2 n1;                                // pixels with min == 0 < max (<= 8 per item per half)
};

// 4 pixels (3 little-endian words w0..w2 = r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3):
// moments, d added to bucket max of this lane's LDS histogram copy `hk`, the
// 0.999999 count
__device__ __forceinline__ void stat4(unsigned w0, unsigned w1, unsigned w2, StatAcc& a, unsigned* hk) {
    const u16x2 one = {1, 1};
    const u16x2 r02 = as_u16x2(__builtin_amdgcn_perm(w1, w0, 0x0c060c00u));
    const u16x2 r13 = as_u16x2(__builtin_amdgcn_perm(w2, w0, 0x0c050c03u));
    const u16x2 g02 = as_u16x2(__builtin_amdgcn_perm(w1, w0, 0x0c070c01u));
    const u16x2 g13 = as_u16x2(__builtin_amdgcn_perm(w2, w1, 0x0c060c00u));
    const u16x2 b02 = as_u16x2(__builtin_amdgcn_perm(w2, w0, 0x0c040c02u));
    const u16x2 b13 = as_u16x2(__builtin_amdgcn_perm(w2, w1, 0x0c070c01u));
    a.sr = __builtin_amdgcn_udot2(r02, one, a.sr, false);
    a.sr = __builtin_amdgcn_udot2(r13, one, a.sr, false);
    a.sg = __builtin_amdgcn_udot2(g02, one, a.sg, false);
    a.sg = __builtin_amdgcn_udot2(g13, one, a.sg, false);
    a.sb = __builtin_amdgcn_udot2(b02, one, a.sb, false);
    a.sb = __builtin_amdgcn_udot2(b13, one, a.sb, false);
    a.qr = __builtin_amdgcn_udot2(r02, r02, a.qr, false);
    a.qr = __builtin_amdgcn_udot2(r13, r13, a.qr, false);
    a.qg = __builtin_amdgcn_udot2(g02, g02, a.qg, false);
    a.qg = __builtin_amdgcn_udot2(g13, g13, a.qg, false);
    a.qb = __builtin_amdgcn_udot2(b02, b02, a.qb, false);
    a.qb = __builtin_amdgcn_udot2(b13, b13, a.qb, false);
    const u16x2 m02 = __builtin_elementwise_max(__builtin_elementwise_max(r02, g02), b02);
    const u16x2 m13 = __builtin_elementwise_max(__builtin_elementwise_max(r13, g13), b13);
    const u16x2 n02 = __builtin_elementwise_min(__builtin_elementwise_min(r02, g02), b02);
    const u16x2 n13 = __builtin_elementwise_min(__builtin_elementwise_min(r13, g13), b13);
    const u16x2 d02 = m02 - n02, d13 = m13 - n13;
    atomicAdd(&hk[m02.x], (unsigned)d02.x);
    atomicAdd(&hk[m13.x], (unsigned)d13.x);
    atomicAdd(&hk[m02.y], (unsigned)d02.y);
    atomicAdd(&hk[m13.y], (unsigned)d13.y);
    const u16x2 zero = {0, 0};
    a.n1 += (u16x2)((n02 == zero) & (m02 != zero)) & one;
    a.n1 += (u16x2)((n13 == zero) & (m13 != zero)) & one;
}

// stat_words for a pointer into device global memory (a global_load_dwordx3,
// where the generic form would be a flat load)
typedef unsigned stat_u32u __attribute__((aligned(1)));
__device__ __forceinline__ void stat_words_global(const uint8_t* q, unsigned* w) {
    const __attribute__((address_space(1))) stat_u32u* g = (const __attribute__((address_space(1))) stat_u32u*)q;
    w[0] = g[0];
    w[1] = g[1];
    w[2] = g[2];
}

// One pixel into the same accumulators (the fewer than 4 pixels at a row's end).
__device__ __forceinline__ void stat1(const uint8_t* q, StatAcc& a, unsigned* hk) {
    const __attribute__((address_space(1))) uint8_t* p = (const __attribute__((address_space(1))) uint8_t*)q;
    const unsigned r = p[0], g = p[1], b = p[2];
    a.sr += r; a.sg += g; a.sb += b;
    a.qr += r * r; a.qg += g * g; a.qb += b * b;
    const unsigned mx = max(max(r, g), b), mn = min(min(r, g), b);
    atomicAdd(&hk[mx], mx - mn);
    a.n1.x += (unsigned short)(mn == 0 && mx != 0);
}
#endif

}  // namespace phd
