// palette_tile.h -- what the palette's pixel passes share (palette.hip: K1,
// Kcut, K3; palette_labels.hip: the label map): the LDS carve of the
// classification tables and the 4-pixel group loads.
#pragma once

#include "phd_device.h"

namespace phd {

// Shared LDS carve (one dynamic array, 16-B aligned base: no static __shared__).
struct K1Lds {
    static constexpr int k255 = 0;           // 256 doubles
    static constexpr int ent = 2048;         // 256 ClsEnt (16 B)
    static constexpr int red = 6144;         // 16 waves x 8 x u64
    static constexpr int qn = 7168;          // Kcut scratch (16 B)
    static constexpr int area = 7184;        // K1: 2 x (tl+1) x C chunk-count copies + tl; K3: rules, sums;
                                             // labels: rules
};
static_assert(sizeof(ClsEnt) == 16, "ClsEnt is one 16-B LDS read");

__device__ __forceinline__ void stage_tables(unsigned char* smem, const double* __restrict__ k255g,
                                             const ClassTables* __restrict__ tabs) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 256; i += blockDim.x) {
        reinterpret_cast<double*>(smem + K1Lds::k255)[i] = k255g[i];
        reinterpret_cast<ClsEnt*>(smem + K1Lds::ent)[i] = tabs->ent[i];
    }
}

typedef const __attribute__((address_space(1))) unsigned gu32;   // global (not flat) loads
typedef const __attribute__((address_space(1))) uint8_t gu8;

__device__ __forceinline__ int px_byte(const unsigned (&w)[3], int b) { return (w[b >> 2] >> (8 * (b & 3))) & 255; }
// pixel i (runtime, 0-3) of a 4-pixel group's words w0 w1 w2 in bits 0-23
__device__ __forceinline__ unsigned px_word(unsigned w0, unsigned w1, unsigned w2, int i) {
    const unsigned p1 = __builtin_amdgcn_alignbyte(w1, w0, 3u), p2 = __builtin_amdgcn_alignbyte(w2, w1, 2u);
    return i == 0 ? w0 : (i == 1 ? p1 : (i == 2 ? p2 : w2 >> 8));
}

// The 12 bytes of pixels p0..p0+3 of an image as three little-endian words.
// Groups not wholly inside the image load from pixel 0 and are masked by the
// caller (the `ok` bits); so every load is unconditional and stays in flight.
template <bool kAligned>
__device__ __forceinline__ void load_group(const uint8_t* ip, long p0, bool ok, unsigned (&w)[3]) {
    const long a = ok ? 3 * p0 : 0;
    if (kAligned) {
        gu32* q = (gu32*)(ip + a);
        w[0] = q[0];
        w[1] = q[1];
        w[2] = q[2];
    } else {
        gu8* b = (gu8*)(ip + a);
#pragma unroll
        for (int k = 0; k < 3; k++)
            w[k] = (unsigned)b[4 * k] | (unsigned)b[4 * k + 1] << 8 | (unsigned)b[4 * k + 2] << 16 |
                   (unsigned)b[4 * k + 3] << 24;
    }
}

}  // namespace phd
