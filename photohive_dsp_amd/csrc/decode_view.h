// decode_view.h -- the typed input stage's decode of one image row, host + device.
//
// A phd_typed_view (include/photohive_dsp.h) holds 8- or 16-bit integers,
// halves, floats or doubles at byte strides.  The value of an element x is
// (double)x / max_value: the reference's Pixel (typedef double Pixel,
// src/types.h:5) of an 8-, 10-, 12- or 16-bit image or of a float image in
// 0..1 or 0..255.  The widening is exact for every type (a half goes through
// float) and the division is IEEE fp64 division, so the doubles are the ones
// a host caller of get_full_report_data would have computed.
//
// decode_row gathers a row, decodes it and, as asked by the record,
//  - writes the three double planes (k_decode_view, decode_views.hip),
//  - writes the packed RGB8 image j = rint(v * 255) and tests every value
//    against the 8-bit rule of k_planar_to_u8 (planar.hip): v == (double)j /
//    255.0 for an integer j in 0..255 (k_classify_views),
// and returns the row's flag bits.  The kernels call it with a team of lanes,
// the host twin (phd_views.cpp: decode_view_host) with a team of one.
//
// Snap (PHD_VIEW_SNAP_U8, halves and floats at the default maximum): an
// element also counts as 8-bit value j when it equals entry j of the type's
// table (T)((double)j / 255.0), what an 8-bit image divided by 255 in that
// type holds.
//
// The span rule is pack_view.h's: no byte is read outside [lowest, highest]
// addressed byte of the view.  A lane takes a unit of U pixels (decode_row_e)
// with the widest naturally aligned loads (16, 8 or 4 bytes) that divide the
// unit's contiguous bytes.  Such a load is taken only where each of its bytes
// belongs to an element the elementwise gather of the same row also reads, or
// lies between two such elements of the row:
//  - planar rows (pixel stride = element size): U elements of a channel's row
//    are U pixels of that channel;
//  - 3-element pixels (channel stride = +-size): the row's own 3 * width
//    elements;
//  - 4-element pixels: the fourth element of pixel p lies before pixel p + 1,
//    so inside the row for every pixel but the last, which goes elementwise.
// Loads are naturally aligned, never rounded down: pixels ahead of the first
// load boundary of the source go elementwise (head), as do those after the
// last whole unit (tail); a row in which the channels' rows (planar) or the
// pixels (interleaved) never meet a boundary goes elementwise as a whole.
// The planes are stored as 16-byte pairs where the destination is aligned, and
// the RGB8 bytes as dwords.
#pragma once

#include <stdint.h>

#include "pack_view.h"

#if defined(__HIPCC__)
#define DEC_UNROLL _Pragma("unroll")
#else
#define DEC_UNROLL
#endif

namespace phd {

// element types and flags of phd_typed_view (include/photohive_dsp.h: PHD_ELEM_*)
enum DecElemId { kElemU8 = 0, kElemU16 = 1, kElemF16 = 2, kElemF32 = 3, kElemF64 = 4, kNumElems = 5 };
enum DecKind { kDecGeneric = 0, kDecPlanar = 1, kDecPx3 = 3, kDecPx4 = 4 };
// a row's (and an image's) flag word
enum { kDecNotU8 = 1, kDecNonFinite = 2 };

// One view of a launch (the device table's record; 96 bytes).  src is element
// R of pixel (0, 0); strides in bytes as in phd_typed_view.
struct DecodeRec {
    const uint8_t* src;
    double* planes;      // R plane; G at + height * width doubles, B after it (nullptr: no planes)
    uint8_t* rgb8;       // packed 3 * height * width bytes (nullptr: none, and no 8-bit test)
    const void* snap;    // 256 entries of the element type (nullptr: no snap)
    long long row_stride, pixel_stride, channel_stride;
    double max_value;    // the divisor (never 0)
    int height, width;
    int elem;            // DecElemId
    int kind;            // DecKind
    int band_rows;       // rows per block of the launch's (view, row band) grid
    int pad_;
    long long pad2_;
};

PACK_HD int dec_elem_size(int elem) {
    return elem == kElemU8 ? 1 : elem == kElemF64 ? 8 : elem == kElemF32 ? 4 : 2;
}

// half -> float, exact (subnormals, infinities and NaNs included)
PACK_HD float dec_half_to_float(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, h);
#else
    const uint32_t s = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
    if (e == 0) {
        const float f = (float)m * (1.0f / 16777216.0f);      // m * 2^-24, exact
        return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) | s);
    }
    if (e == 31) return __builtin_bit_cast(float, s | 0x7f800000u | (m << 13));
    return __builtin_bit_cast(float, s | ((e + 112u) << 23) | (m << 13));
#endif
}

// The element types: storage type, exact widening, equality of two elements as values
template <int E>
struct DecElem;
template <>
struct DecElem<kElemU8> {
    typedef uint8_t T;
    static PACK_HD double widen(T x) { return (double)x; }
    static PACK_HD bool same(T a, T b) { return a == b; }
};
template <>
struct DecElem<kElemU16> {
    typedef uint16_t T;
    static PACK_HD double widen(T x) { return (double)x; }
    static PACK_HD bool same(T a, T b) { return a == b; }
};
template <>
struct DecElem<kElemF16> {
    typedef uint16_t T;
    static PACK_HD double widen(T x) { return (double)dec_half_to_float(x); }
    static PACK_HD bool same(T a, T b) { return dec_half_to_float(a) == dec_half_to_float(b); }
};
template <>
struct DecElem<kElemF32> {
    typedef float T;
    static PACK_HD double widen(T x) { return (double)x; }
    static PACK_HD bool same(T a, T b) { return a == b; }
};
template <>
struct DecElem<kElemF64> {
    typedef double T;
    static PACK_HD double widen(T x) { return x; }
    static PACK_HD bool same(T a, T b) { return a == b; }
};

// 16-byte pair of doubles at its natural alignment
struct __attribute__((may_alias, aligned(16))) dec_d2 {
    double x, y;
};
typedef double __attribute__((may_alias)) dec_f64;

// one element at its natural alignment (the view's rules: data and strides are
// multiples of the element size)
template <class T>
PACK_HD T dec_load(const uint8_t* p) {
    typedef T __attribute__((may_alias)) A;
    return *(const A*)p;
}

// The widest naturally aligned access (16, 8, 4, 2 or 1 bytes) that divides n bytes
constexpr int dec_chunk_bytes(int n) { return n % 16 == 0 ? 16 : n % 8 == 0 ? 8 : n % 4 == 0 ? 4 : n % 2 == 0 ? 2 : 1; }
template <int B>
struct DecChunk;
template <>
struct DecChunk<16> {
    typedef pack_u128 T;
};
template <>
struct DecChunk<8> {
    struct __attribute__((may_alias, aligned(8))) T {
        uint32_t x, y;
    };
};
template <>
struct DecChunk<4> {
    struct __attribute__((may_alias, aligned(4))) T {
        uint32_t x;
    };
};
template <>
struct DecChunk<2> {
    struct __attribute__((may_alias, aligned(2))) T {
        uint16_t x;
    };
};
template <>
struct DecChunk<1> {
    struct __attribute__((may_alias)) T {
        uint8_t x;
    };
};

// N contiguous elements by loads of dec_chunk_bytes(N * sizeof(T)) bytes, p aligned to them
template <class T, int N>
PACK_HD void dec_load_vec(const uint8_t* p, T* e) {
    constexpr int kBytes = dec_chunk_bytes(N * (int)sizeof(T)), kLoads = N * (int)sizeof(T) / kBytes;
    typedef typename DecChunk<kBytes>::T C;
    C v[kLoads];
DEC_UNROLL
    for (int k = 0; k < kLoads; k++) v[k] = *(const C*)(p + kBytes * k);
    __builtin_memcpy(e, v, sizeof(v));
}

// The value of an element: x / 1.0 is x, bit for bit but for a signalling NaN's quiet bit
template <int E>
PACK_HD double dec_value(typename DecElem<E>::T x, double max_value) {
    const double w = DecElem<E>::widen(x);
    return max_value == 1.0 ? w : w / max_value;
}

// The kind of a validated view
PACK_HD int dec_kind(int elem, long long ps, long long cs) {
    const long long es = dec_elem_size(elem);
    if (ps == es) return kDecPlanar;
    if (cs == es || cs == -es) {
        if (ps == 3 * es) return kDecPx3;
        if (ps == 4 * es) return kDecPx4;
    }
    return kDecGeneric;
}

// The 8-bit test of one decoded value (k_planar_to_u8's): its byte, the flag bits into *bits
template <int E>
PACK_HD int dec_classify(double v, typename DecElem<E>::T x, const typename DecElem<E>::T* snap, int* bits) {
    const bool in = v >= 0.0 && v <= 1.0;      // false for NaN
    const int k = in ? (int)__builtin_rint(v * 255.0) : 0;
    // (the division, not a table of the 256 quotients: the gather measured 35 % slower)
    bool is8 = in && (double)k / 255.0 == v;
    if (snap && in) is8 = is8 || DecElem<E>::same(snap[k], x);
    *bits |= (is8 ? 0 : kDecNotU8) | (__builtin_isfinite(v) ? 0 : kDecNonFinite);
    return k;
}

// U pixels from pixel p of row y, their raw elements in x[channel][pixel]:
// decoded and stored as the record asks
template <int E, int U>
PACK_HD void dec_store_unit(const DecodeRec& r, long long at, const typename DecElem<E>::T (*x)[U], int* bits) {
    typedef typename DecElem<E>::T T;
    const long long n = (long long)r.height * r.width;
    uint8_t k[3 * U];
DEC_UNROLL
    for (int c = 0; c < 3; c++) {
        double v[U];
DEC_UNROLL
        for (int j = 0; j < U; j++) v[j] = dec_value<E>(x[c][j], r.max_value);
        if (r.planes) {
            double* d = r.planes + c * n + at;
            if (!((uintptr_t)d & 15)) {
DEC_UNROLL
                for (int j = 0; j < U; j += 2) *(dec_d2*)(d + j) = dec_d2{v[j], v[j + 1]};
            } else {
DEC_UNROLL
                for (int j = 0; j < U; j++) *(dec_f64*)(d + j) = v[j];
            }
        }
        if (r.rgb8) {
DEC_UNROLL
            for (int j = 0; j < U; j++) k[3 * j + c] = (uint8_t)dec_classify<E>(v[j], x[c][j], (const T*)r.snap, bits);
        }
    }
    if (r.rgb8) {
        uint8_t* d = r.rgb8 + 3 * at;
        if ((3 * U) % 4 == 0 && !((uintptr_t)d & 3)) {
DEC_UNROLL
            for (int q = 0; q < 3 * U / 4; q++)
                *(pack_u32*)(d + 4 * q) = (uint32_t)k[4 * q] | (uint32_t)k[4 * q + 1] << 8 |
                                          (uint32_t)k[4 * q + 2] << 16 | (uint32_t)k[4 * q + 3] << 24;
        } else {
DEC_UNROLL
            for (int q = 0; q < 3 * U; q++) d[q] = k[q];
        }
    }
}

// pixels [p0, p1) of row y, an element at a time (every kind)
template <int E>
PACK_HD void dec_row_elems(const DecodeRec& r, const uint8_t* src_row, int y, int p0, int p1, int lane, int lanes,
                           int* bits) {
    typedef typename DecElem<E>::T T;
    const long long n = (long long)r.height * r.width;
    for (int p = p0 + lane; p < p1; p += lanes) {
        const uint8_t* s = src_row + (long long)p * r.pixel_stride;
        const long long at = (long long)y * r.width + p;
DEC_UNROLL
        for (int c = 0; c < 3; c++) {
            const T x = dec_load<T>(s + c * r.channel_stride);
            const double v = dec_value<E>(x, r.max_value);
            if (r.planes) *(dec_f64*)(r.planes + c * n + at) = v;
            if (r.rgb8) r.rgb8[3 * at + c] = (uint8_t)dec_classify<E>(v, x, (const T*)r.snap, bits);
        }
    }
}

// Row y of view r by `lanes` cooperating lanes (this one is `lane`); the flag
// bits of this lane's elements.
template <int E, int U>
PACK_HD int decode_row_t(const DecodeRec& r, int y, int lane, int lanes) {
    typedef typename DecElem<E>::T T;
    constexpr int es = (int)sizeof(T);
    const uint8_t* src = r.src + (long long)y * r.row_stride;
    const long long cs = r.channel_stride;
    const int W = r.width;
    int bits = 0, head = W, nvec = 0;
    if (r.kind == kDecPlanar) {
        // the three channel rows meet the loads' boundaries at the same pixels
        constexpr int vb = dec_chunk_bytes(U * es);
        const int h = (int)(((0 - (uintptr_t)src) & (vb - 1)) / es);
        if (!((uintptr_t)cs & (vb - 1)) && h + U <= W) {
            head = h;
            nvec = (W - h) / U;
        }
        for (int u = lane; u < nvec; u += lanes) {
            const int p = head + u * U;
            T x[3][U];
DEC_UNROLL
            for (int c = 0; c < 3; c++) dec_load_vec<T, U>(src + c * cs + (long long)p * es, x[c]);
            dec_store_unit<E, U>(r, (long long)y * W + p, x, &bits);
        }
    } else if (r.kind == kDecPx3 || r.kind == kDecPx4) {
        const int S = r.kind;                                   // elements per pixel
        const uint8_t* base = src + (cs < 0 ? 2 * cs : 0);      // the pixel's lowest element
        // (the loads of a unit: 3 U or 4 U elements)
        const int vb = S == 3 ? dec_chunk_bytes(3 * U * es) : dec_chunk_bytes(4 * U * es), m = vb / es;
        const int a = (int)(((uintptr_t)base & (uintptr_t)(vb - 1)) / es);
        const int wv = S == 4 ? W - 1 : W;                      // 4-element pixels: the last one elementwise
        int h = 0;
        while (h < m && ((a + S * h) & (m - 1))) h++;
        if (h < m && h + U <= wv) {
            head = h;
            nvec = (wv - h) / U;
        }
        const bool rev = cs < 0;                                // channel c is the pixel's element 2 - c
        for (int u = lane; u < nvec; u += lanes) {
            const int p = head + u * U;
            T x[3][U];
            if (S == 3) {
                T f[3 * U];
                dec_load_vec<T, 3 * U>(base + (long long)p * 3 * es, f);
DEC_UNROLL
                for (int c = 0; c < 3; c++)
DEC_UNROLL
                    for (int j = 0; j < U; j++) x[c][j] = rev ? f[3 * j + 2 - c] : f[3 * j + c];
            } else {
                T f[4 * U];
                dec_load_vec<T, 4 * U>(base + (long long)p * 4 * es, f);
DEC_UNROLL
                for (int c = 0; c < 3; c++)
DEC_UNROLL
                    for (int j = 0; j < U; j++) x[c][j] = rev ? f[4 * j + 2 - c] : f[4 * j + c];
            }
            dec_store_unit<E, U>(r, (long long)y * W + p, x, &bits);
        }
    }
    dec_row_elems<E>(r, src, y, 0, head < W ? head : W, lane, lanes, &bits);
    if (head < W) dec_row_elems<E>(r, src, y, head + nvec * U, W, lane, lanes, &bits);
    return bits;
}

// The pixels of a lane's unit.  Consecutive lanes take consecutive units, so a
// unit's bytes are what a lane's accesses reach across: PHD_DEC_UNIT_PLANES
// pixels where the planes are written (24 bytes a pixel: the stores decide),
// PHD_DEC_UNIT_RGB8 where only the RGB8 image is (the loads decide); 0: the
// pixels of a 16-byte load, at least 4.  Measured: DESIGN.md section 17.
#ifndef PHD_DEC_UNIT_PLANES
#define PHD_DEC_UNIT_PLANES 2
#endif
#ifndef PHD_DEC_UNIT_RGB8
#define PHD_DEC_UNIT_RGB8 8
#endif
template <int E>
PACK_HD int decode_row_e(const DecodeRec& r, int y, int lane, int lanes) {
    constexpr int nat = 16 / (int)sizeof(typename DecElem<E>::T) < 4 ? 4 : 16 / (int)sizeof(typename DecElem<E>::T);
    constexpr int UP = PHD_DEC_UNIT_PLANES ? PHD_DEC_UNIT_PLANES : nat, UR = PHD_DEC_UNIT_RGB8 ? PHD_DEC_UNIT_RGB8 : nat;
    return r.planes ? decode_row_t<E, UP>(r, y, lane, lanes) : decode_row_t<E, UR>(r, y, lane, lanes);
}

PACK_HD int decode_row(const DecodeRec& r, int y, int lane, int lanes) {
    switch (r.elem) {
    case kElemU8: return decode_row_e<kElemU8>(r, y, lane, lanes);
    case kElemU16: return decode_row_e<kElemU16>(r, y, lane, lanes);
    case kElemF16: return decode_row_e<kElemF16>(r, y, lane, lanes);
    case kElemF32: return decode_row_e<kElemF32>(r, y, lane, lanes);
    default: return decode_row_e<kElemF64>(r, y, lane, lanes);
    }
}

// rows per block: about 8192 pixels, at most the view
PACK_HD int decode_band_rows(int height, int width) {
    long long rows = (8192 + (long long)width - 1) / width;
    if (rows > height) rows = height;
    return (int)(rows < 1 ? 1 : rows);
}

}  // namespace phd
