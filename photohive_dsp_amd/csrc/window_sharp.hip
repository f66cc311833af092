// window_sharp.hip -- the window sharpness: per T x T window (T = 16, 32, 64 or
// 128) of a packed RGB8 image the reference's get_variance_sharpness on that crop
// of the full-resolution luma -- crop_pgm (src/image_processing.c:213-232),
// rgb2pgm (:505-512), filter_image with the 3 x 3 Laplacian (src/filtering.c:
// 81-107), get_average and get_variance (:125-148), variance / average
// (:151-183) -- in exact integer arithmetic up to one fp64 finish per window.
// The reference zero-pads at the crop border, so a window needs no halo: its
// 3 T^2 bytes come in once, its luma lies in LDS as int32 and one or two doubles
// go out.  Every window of every image of a call takes one launch.
// Row code, the 128-bit D and the finish: sharp_window.h (shared with the host
// twin, phd_sharpwin.cpp).
#include "phd_device.h"
#include "sharp_window.h"

namespace phd {

namespace {

// Blocks of 256 threads.  At T = 128 and 64 a block takes one window, at T = 32
// and 16 a wave takes one, four windows a block.  The NTW threads of a window
// load its T * T / 4 four-pixel units, PER each, and then filter one column of RG
// rows each (G row groups per column).
template <int T>
struct SharpWinPlan {
    static constexpr int kThreads = 256;
    static constexpr int NTW = T >= 64 ? 256 : 64;
    static constexpr int WPB = kThreads / NTW;
    static constexpr int UPR = T / 4, PER = T * UPR / NTW;
    static constexpr int G = NTW / T, RG = T / G;
    // the windows' luma, then S1 and S2 per wave of a one-window block
    static constexpr size_t kLds = sizeof(int) * T * T * WPB + (WPB == 1 ? sizeof(unsigned long long) * 2 * 4 : 0);
    static_assert((T * UPR) % NTW == 0 && PER >= 1 && NTW % T == 0 && T % G == 0, "whole units and columns per thread");
};
static_assert(2 * SharpWinPlan<128>::kLds <= 163840, "two 128-windows per CU");

typedef unsigned shw_gu32 __attribute__((address_space(1)));
typedef uint8_t shw_gu8 __attribute__((address_space(1)));
typedef double shw_gf64 __attribute__((address_space(1)));

// bits sh .. sh + 31 of hi : lo (sh = 0, 8, 16 or 24)
__device__ __forceinline__ unsigned shw_align(unsigned lo, unsigned hi, unsigned sh) {
    return (unsigned)((((unsigned long long)hi << 32) | lo) >> sh);
}

// The four aligned dwords that hold the 12 bytes of a unit beginning p bytes
// (its row's byte phase) behind q (4-byte aligned).  d[3] holds none of them when
// p == 0 and is not read; it and d[0] are the dwords that may reach over a row's
// end and begin before its start.  head: the image begins with this unit, inside
// d[0] -- bytes p .. 3 one by one; tail: the image ends with this unit, inside
// d[3] -- bytes 0 .. p - 1 one by one.  No dword wholly outside the image and no
// byte outside it is read.
__device__ __forceinline__ void shw_unit_load(const uint8_t* q, unsigned p, bool head, bool tail, unsigned* d) {
    const shw_gu32* g = (const shw_gu32*)q;
    const shw_gu8* b = (const shw_gu8*)q;
    d[1] = g[1];
    d[2] = g[2];
    if (!head) d[0] = g[0];
    else {
        unsigned v = 0;
        for (unsigned i = p; i < 4; i++) v |= (unsigned)b[i] << (8 * i);
        d[0] = v;
    }
    d[3] = 0;
    if (p != 0) {
        if (!tail) d[3] = g[3];
        else {
            unsigned v = 0;
            for (unsigned i = 0; i < p; i++) v |= (unsigned)b[12 + i] << (8 * i);
            d[3] = v;
        }
    }
}

// recs[w], dst[w]: window w of n.  Plain stores: a window has one owner.
template <int T>
__global__ __launch_bounds__(SharpWinPlan<T>::kThreads) void k_window_sharp(const SharpWinRec* __restrict__ recs,
                                                                            const SharpWinDst* __restrict__ dst,
                                                                            int n) {
    using P = SharpWinPlan<T>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int sub = P::WPB > 1 ? wave : 0;                   // this thread's window of the block
    const int t = P::WPB > 1 ? (tid & 63) : tid;             // and its number among the window's threads
    const long long w = (long long)blockIdx.x * P::WPB + sub;
    const bool has = w < n;                                  // (a block's last waves may have no window)
    int* luma = reinterpret_cast<int*>(smem) + sub * T * T;

    // 1. the window's rows as 4-pixel units out of aligned dwords, their luma into LDS
    if (has) {
        const SharpWinRec rec = recs[w];
        const long long pitch = (long long)(rec.pitch_edge >> 2);
        const bool first = (rec.pitch_edge & 1ull) != 0, last = (rec.pitch_edge & 2ull) != 0;
        unsigned d[P::PER][4], ph[P::PER];
#pragma unroll
        for (int j = 0; j < P::PER; j++) {
            const int u = t + j * P::NTW, y = u / P::UPR, k = u - y * P::UPR;
            const uint8_t* row = rec.first + (long long)y * pitch;
            const unsigned p = (unsigned)(reinterpret_cast<uintptr_t>(row) & 3u);
            ph[j] = p;
            shw_unit_load(row - p + 12 * k, p, first && u == 0 && p != 0,
                          last && u == T * P::UPR - 1 && p != 0, d[j]);
        }
#pragma unroll
        for (int j = 0; j < P::PER; j++) {
            const int u = t + j * P::NTW;
            const unsigned sh = 8 * ph[j];
            int l[4];
            shw_unit_luma(shw_align(d[j][0], d[j][1], sh), shw_align(d[j][1], d[j][2], sh),
                          shw_align(d[j][2], d[j][3], sh), l);
            // unit u: pixels 4 u .. 4 u + 3 in row-major order
            reinterpret_cast<int4*>(luma)[u] = make_int4(l[0], l[1], l[2], l[3]);
        }
    }
    __syncthreads();

    // 2. a column of RG rows per thread: f from LDS in int32, S1 in i64, S2 in u64
    long long s1 = 0;
    unsigned long long s2 = 0;
    if (has) {
        const int g = t / T, x = t - g * T;
        shw_column(luma, T, x, g * P::RG, P::RG, &s1, &s2);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);

    // 3. one thread per window: D, the finish, one or two doubles
    unsigned long long S1 = (unsigned long long)s1, S2 = s2;
    if constexpr (P::WPB == 1) {
        unsigned long long* red = reinterpret_cast<unsigned long long*>(smem + sizeof(int) * T * T);
        if (lane_id() == 0) {
            red[2 * wave] = S1;
            red[2 * wave + 1] = S2;
        }
        __syncthreads();
        if (tid != 0) return;
        S1 = red[0] + red[2] + red[4] + red[6];
        S2 = red[1] + red[3] + red[5] + red[7];
    } else {
        if (lane_id() != 0) return;
    }
    if (!has) return;
    const SharpWinDst o = dst[w];
    const unsigned long long npix = (unsigned long long)T * T;
    const double num = shw_num(shw_d(npix, S1, S2));
    *(shw_gf64*)o.sharpness = shw_sharpness(num, npix, S1);
    if (o.variance) *(shw_gf64*)o.variance = shw_variance(num, npix);
}

template <int T>
hipError_t launch_sharp_t(const SharpWinRec* d_recs, const SharpWinDst* d_dst, int n, hipStream_t st) {
    using P = SharpWinPlan<T>;
    static bool once = ((void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_window_sharp<T>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                        true);
    (void)once;
    const unsigned blocks = (unsigned)(((long long)n + P::WPB - 1) / P::WPB);
    phd_launch(k_window_sharp<T>, dim3(blocks), dim3(P::kThreads), P::kLds, st, d_recs, d_dst, n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_window_sharp(int T, const SharpWinRec* d_recs, const SharpWinDst* d_dst, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    switch (T) {
        case 16: return launch_sharp_t<16>(d_recs, d_dst, n, st);
        case 32: return launch_sharp_t<32>(d_recs, d_dst, n, st);
        case 64: return launch_sharp_t<64>(d_recs, d_dst, n, st);
        case 128: return launch_sharp_t<128>(d_recs, d_dst, n, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace phd
