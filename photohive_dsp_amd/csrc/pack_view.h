// pack_view.h -- the input stage's gather of one image row, host + device.
//
// A phd_image_view (include/photohive_dsp.h) that is not already packed RGB8
// is gathered once into a packed image (rows of 3*width bytes) by k_pack_views
// (pack_views.hip) and, with the same row code, on the host (phd_views.cpp:
// phd_debug_pack_view_host).  Everything a row does -- its split into head,
// vector body and tail, the addresses of every load and store, the byte
// shuffles -- is pack_row below; the kernel calls it with a team of lanes, the
// host with a team of one.
//
// The span rule: no byte is read outside [lowest, highest] addressed byte of
// the view, none written outside the 3*H*W destination bytes.  So a vector
// access is taken only where each of its bytes is a byte the bytewise gather
// of the same row would also touch, or lies between two such bytes of the row:
//  - planar: 4 bytes of each plane are 4 pixels of that plane;
//  - 4-byte pixels: the dword of pixel p holds its three channels and the byte
//    after them (cs = +1) -- before the next pixel's first byte, so inside the
//    row for every pixel but the last, which always goes bytewise;
//  - pitched: the row's own 3*width bytes.
// Vector accesses are naturally aligned (never rounded down to an aligned
// address): pixels ahead of the first position where the destination is
// aligned go bytewise (head), as do those after the last whole unit (tail),
// and a row whose source is not aligned where its destination is goes
// bytewise as a whole.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PACK_HD __host__ __device__ __forceinline__
#else
#define PACK_HD inline
#endif

namespace phd {

enum PackKind { kPackPacked = 0, kPackPitched = 1, kPackPx4 = 2, kPackPlanar = 3, kPackGeneric = 4 };

// One view of a launch (the device table's record; 64 bytes).  src is the R
// byte of pixel (0, 0); strides in bytes as in phd_image_view.
struct PackRec {
    const uint8_t* src;
    uint8_t* dst;
    long long row_stride, pixel_stride, channel_stride;
    int height, width;
    int kind;           // PackKind (never kPackPacked in a launch)
    int band_rows;      // rows per block of the launch's (view, row band) grid
    long long pad_;
};

// 4- and 16-byte accesses at their natural alignment (UBSan checks it on the host)
typedef uint32_t __attribute__((may_alias)) pack_u32;
struct __attribute__((may_alias, aligned(16))) pack_u128 {
    uint32_t x, y, z, w;
};

// v_perm_b32: byte k of the result is byte sel[k] of the eight bytes {hi:lo}
// (0-3 lo, 4-7 hi)
PACK_HD uint32_t pack_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) r |= (uint32_t)((v >> (8 * ((sel >> (8 * k)) & 7))) & 0xff) << (8 * k);
    return r;
#endif
}

// The kind of a validated view (phd_views.cpp: view_why)
PACK_HD int pack_kind(int width, long long rs, long long ps, long long cs) {
    if (ps == 3 && cs == 1) return rs == 3LL * width ? kPackPacked : kPackPitched;
    if (ps == 4 && (cs == 1 || cs == -1)) return kPackPx4;
    if (ps == 1) return kPackPlanar;
    return kPackGeneric;
}

// A row's split.  Pixel kinds: pixels [0, head) bytewise, then nvec units of 4
// pixels (12 destination bytes, three aligned dwords), then the tail bytewise.
// Pitched: the same over the row's 3*width bytes with units of vec bytes.
struct PackSplit {
    int head, nvec, vec;
};

PACK_HD PackSplit pack_row_split(int kind, uintptr_t dst_row, uintptr_t src_row, long long cs, int width) {
    PackSplit s{width, 0, 4};
    if (kind == kPackPitched) {
        const int nbytes = 3 * width;
        s.head = nbytes;
        const uintptr_t d = dst_row ^ src_row;           // equal low bits: aligned together
        const int vec = !(d & 15) ? 16 : !(d & 3) ? 4 : 0;
        if (!vec) return s;
        const int head = (int)((0 - dst_row) & (uintptr_t)(vec - 1));
        if (head >= nbytes) return s;
        s.head = head;
        s.nvec = (nbytes - head) / vec;
        s.vec = vec;
        return s;
    }
    if (kind != kPackPx4 && kind != kPackPlanar) return s;
    // dst_row + 3 p is dword aligned where p == dst_row (mod 4)
    const int head = (int)(dst_row & 3);
    // 4-byte pixels: the row's last pixel never takes the dword load
    const int wv = kind == kPackPx4 ? width - 1 : width;
    if (head + 4 > wv) return s;
    bool ok;
    if (kind == kPackPx4) {
        const uintptr_t q = src_row + 4 * (uintptr_t)head - (cs < 0 ? 2 : 0);
        ok = !(q & 3);
    } else {
        const uintptr_t q = src_row + (uintptr_t)head;
        ok = !(q & 3) && !((q + (uintptr_t)cs) & 3) && !((q + (uintptr_t)(2 * cs)) & 3);
    }
    if (!ok) return s;
    s.head = head;
    s.nvec = (wv - head) / 4;
    return s;
}

// pixels [p0, p1) of a row, a byte at a time (every kind)
PACK_HD void pack_row_bytes(const uint8_t* src_row, uint8_t* dst_row, long long ps, long long cs, int p0, int p1,
                            int lane, int lanes) {
    for (int p = p0 + lane; p < p1; p += lanes) {
        const uint8_t* s = src_row + (long long)p * ps;
        uint8_t* d = dst_row + 3 * (long long)p;
        d[0] = s[0];
        d[1] = s[cs];
        d[2] = s[2 * cs];
    }
}

// Row y of view r by `lanes` cooperating lanes (this one is `lane`).
PACK_HD void pack_row(const PackRec& r, int y, int lane, int lanes) {
    const uint8_t* src = r.src + (long long)y * r.row_stride;
    uint8_t* dst = r.dst + 3LL * r.width * y;
    const long long ps = r.pixel_stride, cs = r.channel_stride;
    const PackSplit s = pack_row_split(r.kind, (uintptr_t)dst, (uintptr_t)src, cs, r.width);
    if (r.kind == kPackPitched) {
        // a row copy: bytes [0, head), nvec units of s.vec bytes, the rest
        const int nbytes = 3 * r.width, body_end = s.head + s.nvec * s.vec;
        if (s.vec == 16) {
            for (int u = lane; u < s.nvec; u += lanes)
                *(pack_u128*)(dst + s.head + 16 * u) = *(const pack_u128*)(src + s.head + 16 * u);
        } else {
            for (int u = lane; u < s.nvec; u += lanes)
                *(pack_u32*)(dst + s.head + 4 * u) = *(const pack_u32*)(src + s.head + 4 * u);
        }
        for (int b = lane; b < s.head; b += lanes) dst[b] = src[b];
        for (int b = body_end + lane; b < nbytes; b += lanes) dst[b] = src[b];
        return;
    }
    if (r.kind == kPackPx4) {
        // dword of pixel p: R G B x (cs = +1) or B G R x (cs = -1, from two bytes below R)
        const uint8_t* q = src + 4LL * s.head - (cs < 0 ? 2 : 0);
        const uint32_t s0 = cs < 0 ? 0x06000102u : 0x04020100u;   // R0 G0 B0 R1
        const uint32_t s1 = cs < 0 ? 0x05060001u : 0x05040201u;   // G1 B1 R2 G2
        const uint32_t s2 = cs < 0 ? 0x04050600u : 0x06050402u;   // B2 R3 G3 B3
        for (int u = lane; u < s.nvec; u += lanes) {
            const pack_u32* in = (const pack_u32*)(q + 16LL * u);
            const uint32_t a = in[0], b = in[1], c = in[2], d = in[3];
            pack_u32* out = (pack_u32*)(dst + 3LL * s.head + 12LL * u);
            out[0] = pack_perm(b, a, s0);
            out[1] = pack_perm(c, b, s1);
            out[2] = pack_perm(d, c, s2);
        }
    } else if (r.kind == kPackPlanar) {
        const uint8_t* q = src + s.head;
        for (int u = lane; u < s.nvec; u += lanes) {
            const uint32_t rr = *(const pack_u32*)(q + 4LL * u);
            const uint32_t gg = *(const pack_u32*)(q + cs + 4LL * u);
            const uint32_t bb = *(const pack_u32*)(q + 2 * cs + 4LL * u);
            pack_u32* out = (pack_u32*)(dst + 3LL * s.head + 12LL * u);
            out[0] = pack_perm(bb, pack_perm(gg, rr, 0x01000400u), 0x03040100u);   // r0 g0 b0 r1
            out[1] = pack_perm(bb, pack_perm(gg, rr, 0x06020005u), 0x03020500u);   // g1 b1 r2 g2
            out[2] = pack_perm(bb, pack_perm(gg, rr, 0x00070300u), 0x07020106u);   // b2 r3 g3 b3
        }
    }
    pack_row_bytes(src, dst, ps, cs, 0, s.head, lane, lanes);
    pack_row_bytes(src, dst, ps, cs, s.head + 4 * s.nvec, r.width, lane, lanes);
}

// rows per block: about 32 KB of destination bytes, at most the view
PACK_HD int pack_band_rows(int height, int width) {
    const long long row = 3LL * width;
    long long rows = (32768 + row - 1) / row;
    if (rows > height) rows = height;
    return (int)(rows < 1 ? 1 : rows);
}

}  // namespace phd
