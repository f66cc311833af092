// window_stats.hip -- the window statistics: per T x T window (T = 16, 32, 64 or
// 128) of a packed RGB8 image get_rgb_statistics (src/image_processing.c:543-553;
// get_average and get_variance, src/filtering.c:125-148) and get_hsv_average over
// rgb2hsv's s (src/image_processing.c:533-540, 372-417) on crop_image's crop
// (src/image_processing.c:244-266).  A window's 3 T^2 bytes come in once, its
// exact integer sums stay on chip -- the moments in registers, D in LDS -- and the
// block that summed it finishes it: seven doubles go out.  Every window of every
// image of a call takes one launch; no global atomic, no zeroed output.
// The 4-pixel unit: stat_unit.h (k_rgb_stats' and k_box_stats'); the finish and
// the launch table: stat_window.h (shared with the host twin, phd_statwin.cpp).
#include "phd_device.h"
#include "stat_unit.h"
#include "stat_window.h"

namespace phd {

namespace {

constexpr int kSwPad = 257;                       // a histogram copy: 256 buckets, padded as k_box_stats pads
// measured alternatives: make variant VFLAGS="-DPHD_STATWIN_COPIES16=2 -DPHD_STATWIN_COPIES32=8"
#if !defined(PHD_STATWIN_COPIES16)
#define PHD_STATWIN_COPIES16 4
#endif
#if !defined(PHD_STATWIN_COPIES32)
#define PHD_STATWIN_COPIES32 4
#endif

// Blocks of 256 threads.  At T = 128 and 64 a block takes one window, at T = 32
// and 16 a wave takes one, four windows a block.  The NTW threads of a window
// load its T * T / 4 four-pixel units, PER each, all before the first add.
// COPIES: the window's copies of D, thread t adding into copy t % COPIES, so
// that the lanes of a wave that meet in one bucket (a grey or uniform window:
// every pixel) are 64 / COPIES, not 64.  More copies cost their zeroing and
// their fold per window, which at 16 and 32 px outweighs the adds: on noise-like
// windows 2 / 4 / 8 copies at 16 px took 2.34 / 2.38 / 3.41 ms and 4 / 8 / 16 at
// 32 px 0.85 / 1.04 / 1.83 ms.  At 64 and 128 px the
// figures are k_box_stats' kind of choice, not measured optima.
template <int T>
struct StatWinPlan {
    static constexpr int kThreads = 256;
    static constexpr int NTW = T >= 64 ? 256 : 64;
    static constexpr int WPB = kThreads / NTW;
    static constexpr int UPR = T / 4, PER = T * UPR / NTW;
    static constexpr int COPIES = T == 128 ? 32 : T == 64 ? 16 : T == 32 ? PHD_STATWIN_COPIES32 : PHD_STATWIN_COPIES16;
    static constexpr int kHistWords = COPIES * kSwPad;       // per window
    // the windows' copies of D; in a one-window block the 256 quotients and the waves' moments
    static constexpr size_t kLds = sizeof(unsigned) * kHistWords * WPB +
                                   (WPB == 1 ? sizeof(double) * 256 + sizeof(unsigned) * 4 * 8 : 0);
    static_assert((T * UPR) % NTW == 0 && PER >= 1, "whole units per thread");
    static_assert((WPB * kHistWords) % 4 == 0 && (COPIES & (COPIES - 1)) == 0,
                  "zeroed as uint4; copy = t & (COPIES - 1)");
    // a thread's 4 * PER pixels, the window's T^2: every u32 below holds them
    static_assert(4LL * PER * 255 * 255 < (1LL << 32), "per-thread u32 sums of squares");
    static_assert(4LL * PER < 65536, "packed u16 min == 0 < max counts");
    static_assert((long long)T * T * 255 * 255 < (1LL << 32), "the window's u32 sums of squares");
    static_assert((long long)T * T * 255 < (1LL << 32), "u32 LDS buckets and their fold");
    static_assert(2 * kLds <= 160 * 1024, "two blocks resident per CU");
};

typedef double sw_gf64 __attribute__((address_space(1)));

// lane `i`'s q, i wave-uniform
__device__ __forceinline__ double sw_readlane(double q, int i) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(q), i);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(q), i);
    return __hiloint2double(hi, lo);
}

// recs[w], dst[w]: window w of n.  Plain stores: a window has one owner.
template <int T>
__global__ __launch_bounds__(StatWinPlan<T>::kThreads) void k_window_stats(const StatWinRec* __restrict__ recs,
                                                                           const StatWinDst* __restrict__ dst, int n) {
    using P = StatWinPlan<T>;
    __shared__ __attribute__((aligned(16))) unsigned hist[P::WPB * P::kHistWords];
    __shared__ double quo[P::WPB == 1 ? 256 : 1];
    __shared__ unsigned red[P::WPB == 1 ? 4 * 8 : 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int sub = P::WPB > 1 ? wave : 0;                   // this thread's window of the block
    const int t = P::WPB > 1 ? lane : tid;                   // and its number among the window's threads
    const long long w = (long long)blockIdx.x * P::WPB + sub;
    const bool has = w < n;                                  // (a block's last waves may have no window)

    // 1. the thread's units: every load issued before the first add
    unsigned wd[P::PER][3];
    if (has) {
        const StatWinRec rec = recs[w];
#pragma unroll
        for (int j = 0; j < P::PER; j++) {
            const int u = t + j * P::NTW, y = u / P::UPR, k = u - y * P::UPR;
            stat_words_global(rec.first + (unsigned long long)y * rec.pitch + 12 * k, wd[j]);
        }
    }
    // 2. the copies of D zeroed
    for (int i = tid; i < P::WPB * P::kHistWords / 4; i += P::kThreads)
        reinterpret_cast<uint4*>(hist)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();

    // 3. moments in registers, d into bucket max of the thread's copy
    unsigned* hw = hist + sub * P::kHistWords;               // the window's copies
    StatAcc a{0, 0, 0, 0, 0, 0, 0.0, {0, 0}};
    if (has) {
        unsigned* hk = hw + (t & (P::COPIES - 1)) * kSwPad;
#pragma unroll
        for (int j = 0; j < P::PER; j++) stat4(wd[j][0], wd[j][1], wd[j][2], a, hk);
    }
    __syncthreads();

    // 4. the window's moments and n1 (u32: the plan's asserts) and its quotients
    // D[m] / m, lane l of the finishing wave holding those of m = l, 64 + l, 128 + l, 192 + l
    unsigned mom[7] = {a.sr, a.sg, a.sb, a.qr, a.qg, a.qb, (unsigned)a.n1.x + (unsigned)a.n1.y};
#pragma unroll
    for (int k = 0; k < 7; k++) mom[k] = wave_sum(mom[k]);
    double q[4];
    if constexpr (P::WPB == 1) {
        unsigned d = 0;
#pragma unroll 8
        for (int c = 0; c < P::COPIES; c++) d += hw[c * kSwPad + tid];
        quo[tid] = tid ? stw_quotient(d, tid) : 0.0;         // (D[0] is 0: max == 0 has d == 0)
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 7; k++) red[8 * wave + k] = mom[k];
        }
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int k = 0; k < 7; k++) mom[k] = red[k] + red[8 + k] + red[16 + k] + red[24 + k];
#pragma unroll
        for (int g = 0; g < 4; g++) q[g] = quo[64 * g + lane];
    } else {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int m = 64 * g + lane;
            unsigned d = 0;
#pragma unroll
            for (int c = 0; c < P::COPIES; c++) d += hw[c * kSwPad + m];
            q[g] = m ? stw_quotient(d, m) : 0.0;
        }
    }
    if (!has) return;                                        // wave-uniform

    // 5. S: the non-zero quotients in ascending m, one after the other, the same
    // in every lane (the masks are wave-uniform)
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        unsigned long long live = __ballot(q[g] != 0.0);
        while (live) {
            const int i = __builtin_ctzll(live);
            live &= live - 1;
            s += sw_readlane(q[g], i);
        }
    }

    // 6. the finish, a value per lane: B of channel l, C of channel l - 3, S-bar
    const unsigned long long npix = (unsigned long long)T * T;
    const int c = lane < 3 ? lane : lane - 3;
    const unsigned long long m1 = c == 0 ? mom[0] : c == 1 ? mom[1] : mom[2];
    const unsigned long long m2 = c == 0 ? mom[3] : c == 1 ? mom[4] : mom[5];
    if (lane < kStatWinOut) {
        const double v = lane < 3 ? stw_brightness(m1, npix)
                                  : lane < 6 ? stw_contrast(m1, m2, npix) : stw_sbar(s, mom[6], npix);
        ((sw_gf64*)dst[w])[lane] = v;
    }
}

template <int T>
hipError_t launch_stats_t(const StatWinRec* d_recs, const StatWinDst* d_dst, int n, hipStream_t st) {
    using P = StatWinPlan<T>;
    const unsigned blocks = (unsigned)(((long long)n + P::WPB - 1) / P::WPB);
    phd_launch(k_window_stats<T>, dim3(blocks), dim3(P::kThreads), 0, st, d_recs, d_dst, n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_window_stats(int T, const StatWinRec* d_recs, const StatWinDst* d_dst, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    switch (T) {
        case 16: return launch_stats_t<16>(d_recs, d_dst, n, st);
        case 32: return launch_stats_t<32>(d_recs, d_dst, n, st);
        case 64: return launch_stats_t<64>(d_recs, d_dst, n, st);
        case 128: return launch_stats_t<128>(d_recs, d_dst, n, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace phd
