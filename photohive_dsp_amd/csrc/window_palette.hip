// window_palette.hip -- the window palettes: per T x T window (T = 16, 32, 64 or
// 128) of a palette label map (the lists of src/color_quantization.c:342-479 and
// :510-576 kept per pixel, inside crop_pgm's box, src/image_processing.c:213-232)
// the number of elements of every palette slot and the slot that dominates.  A
// window's 2 T^2 bytes come in once, its counters stay in LDS, and the block that
// counted it writes its whole row: n_slots + 1 plain stores and one uint16.  Every
// window of every map of a call takes one launch; no global atomic, no zeroed
// output.  The unit, the copies rule, the dominant key and the launch table:
// pal_window.h (shared with the host twin, phd_palwin.cpp).
#include "phd_device.h"
#include "pal_window.h"

namespace phd {

namespace {

// Blocks of 256 threads.  At T = 128 and 64 a block takes one window, at T = 32
// and 16 a wave takes one, four windows a block.  The NTW threads of a window load
// its T * T / 4 four-label units, PER each, all before the first add.
template <int T>
struct PalWinPlan {
    static constexpr int kThreads = 256;
    static constexpr int NTW = T >= 64 ? 256 : 64;
    static constexpr int WPB = kThreads / NTW;
    static constexpr int UPR = T / 4, PER = T * UPR / NTW;
    static_assert((T * UPR) % NTW == 0 && PER >= 1, "whole units per thread");
    static_assert((long long)T * T <= 128 * 128, "pw_key's count");
    // dynamic LDS: the windows' copies, at most one copy of 4097 counters each;
    // static: the waves' keys of a one-window block
    static constexpr size_t kMaxLds = sizeof(unsigned) * kPalWinMaxLdsWords * WPB + sizeof(unsigned) * 4;
    static_assert(2 * kMaxLds <= 160 * 1024, "two blocks resident per CU at 4096 slots");
};

// a unit's 8 bytes from its own 2-byte aligned address: one global_load_dwordx2
typedef unsigned long long pw_u64u __attribute__((aligned(2)));
typedef unsigned pw_gu32 __attribute__((address_space(1)));
typedef unsigned short pw_gu16 __attribute__((address_space(1)));

__device__ __forceinline__ unsigned long long pw_unit_global(const uint16_t* p) {
    return *(const __attribute__((address_space(1))) pw_u64u*)p;
}

__device__ __forceinline__ unsigned pw_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// recs[w], dst[w]: window w of n; stride: LDS words per window of this launch (a
// multiple of 4, at least pw_lds_words of every record).  Plain stores: a window
// has one owner.
template <int T>
__global__ __launch_bounds__(PalWinPlan<T>::kThreads) void k_window_palette(const PalWinRec* __restrict__ recs,
                                                                            const PalWinDst* __restrict__ dst, int n,
                                                                            int stride) {
    using P = PalWinPlan<T>;
    extern __shared__ __attribute__((aligned(16))) unsigned hist[];
    __shared__ unsigned red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sub = P::WPB > 1 ? wave : 0;                   // this thread's window of the block
    const int t = P::WPB > 1 ? lane : tid;                   // and its number among the window's threads
    const long long w = (long long)blockIdx.x * P::WPB + sub;
    const bool has = w < n;                                  // (a block's last waves may have no window)

    // 1. the thread's units: every load issued before the first add
    unsigned long long q[P::PER];
    int nc = 0;                                              // the window's counters: n_slots + 1
    if (has) {
        const PalWinRec rec = recs[w];
        nc = rec.n_slots + 1;
#pragma unroll
        for (int j = 0; j < P::PER; j++) {
            const int u = t + j * P::NTW, y = u / P::UPR, k = u - y * P::UPR;
            q[j] = pw_unit_global(rec.first + (unsigned long long)y * rec.pitch + 4 * k);
        }
    }
    // 2. the window's copies zeroed: pw_lds_words of its own counters, never the stride
    unsigned* hw = hist + (size_t)sub * stride;              // the window's copies
    const int copies = pw_copies(nc, T), cs = pw_copy_stride(nc);
    if (has) {
        const int used4 = pw_lds_words(nc, T) >> 2;
        for (int i = t; i < used4; i += P::NTW) reinterpret_cast<uint4*>(hw)[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();

    // 3. runs of equal labels into the thread's copy
    if (has) {
        unsigned* hk = hw + (t & (copies - 1)) * cs;
        const unsigned ns = (unsigned)(nc - 1);
#pragma unroll
        for (int j = 0; j < P::PER; j++)
            pw_unit(q[j], ns, [&](unsigned s, unsigned run) { atomicAdd(&hk[s], run); });
    }
    __syncthreads();

    // 4. the copies folded; the row's counters out; the dominant key
    unsigned key = 0;                                        // below every real key: 8191 - s >= 4095
    if (has) {
        const PalWinDst d = dst[w];
        pw_gu32* out = (pw_gu32*)d.counts;
        for (int s = t; s < nc; s += P::NTW) {
            unsigned sum = 0;
            for (int c = 0; c < copies; c++) sum += hw[c * cs + s];
            if (out) out[s] = sum;
            key = max(key, pw_key(sum, (unsigned)s));
        }
        if (d.dominant) {                                    // the window's: block-uniform where a block has one
            key = pw_wave_max(key);
            if constexpr (P::WPB == 1) {
                if (lane == 0) red[wave] = key;
                __syncthreads();
                key = max(max(red[0], red[1]), max(red[2], red[3]));
            }
            if (t == 0) *(pw_gu16*)d.dominant = (unsigned short)pw_key_label(key, (unsigned)(nc - 1));
        }
    }
}

template <int T>
hipError_t launch_palette_t(const PalWinRec* d_recs, const PalWinDst* d_dst, int n, int lds_words, hipStream_t st) {
    using P = PalWinPlan<T>;
    if (lds_words < 4 || lds_words % 4 != 0 || lds_words > kPalWinMaxLdsWords) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(((long long)n + P::WPB - 1) / P::WPB);
    const size_t lds = sizeof(unsigned) * (size_t)lds_words * P::WPB;
    // above 64 KiB (four windows of a 4096-slot palette) the kernel's dynamic-LDS limit is
    // raised first; a refusal is the launch's error, not a launch that fails without a cause
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_window_palette<T>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)P::kMaxLds);
        if (e != hipSuccess) return e;
    }
    phd_launch(k_window_palette<T>, dim3(blocks), dim3(P::kThreads), lds, st, d_recs, d_dst, n, lds_words);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_window_palette(int T, const PalWinRec* d_recs, const PalWinDst* d_dst, int n, int lds_words,
                                 hipStream_t st) {
    if (n <= 0) return hipSuccess;
    switch (T) {
        case 16: return launch_palette_t<16>(d_recs, d_dst, n, lds_words, st);
        case 32: return launch_palette_t<32>(d_recs, d_dst, n, lds_words, st);
        case 64: return launch_palette_t<64>(d_recs, d_dst, n, lds_words, st);
        case 128: return launch_palette_t<128>(d_recs, d_dst, n, lds_words, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace phd
