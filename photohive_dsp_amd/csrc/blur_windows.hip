// blur_windows.hip -- the window blur: per T x T window (T = 64 or 128) of a
// packed RGB8 image the polar bin sums and the spectrum maximum of the
// reference's get_blur_profile on that crop -- crop_image
// (src/image_processing.c:244-266), avg from get_rgb_statistics (:543-553,
// src/interface.c:78), rgb2pgm + remove_dc_bias (:505-512,
// src/blur_profile.c:233-238), the r2c 2-D DFT power (src/fft_processing.c:
// 18-63), pgm_normalize_fft (:173-213) and calculate_blur_profile's binning
// (src/blur_profile.c:34-126) -- with the whole window in LDS: one block takes
// a window from its RGB bytes to its bin sums, nothing in between goes to HBM.
// k_window_vectors goes on in the same block: the bins' normalisation and
// vectorize_blur_profile (src/blur_profile.c:324-416) out of LDS, ten
// Blur_Vectors and the maximum per window to device memory.
// Plan, index maps, butterflies and the finish's rows: blur_window.h (shared
// with the host twin window_bins_host below and the finish's, phd_blurwin.cpp).
#include <cmath>

#include "phd_device.h"
#include "blur_window.h"
#include "stat_unit.h"

namespace phd {

namespace {

// LDS of k_window_blur<T>: [ win_elems(T) complex | T twiddles | log table |
// per-wave partials | nbins u64 bins ].  The 256 doubles k / 255.0 are needed
// only until the luma is formed and the bins only after the transforms, so the
// table lies over the bins (which are zeroed once it has been used): 2 KiB less,
// and four 64-windows instead of three share a CU at the wrappers' 16 x 36 grid.
template <int T>
constexpr size_t win_lds_fixed() {
    return sizeof(double2) * (win_elems(T) + T + kLogTab) + sizeof(unsigned long long) * 4 * (WinPlan<T>::kThreads / 64);
}
constexpr size_t win_lds_bins(int nbins) {
    return sizeof(unsigned long long) * (size_t)(nbins > 256 ? nbins : 256);
}
static_assert(win_lds_fixed<128>() + win_lds_bins(kWinMaxBins) <= 163840, "LDS of a workgroup");
static_assert(4 * (win_lds_fixed<64>() + win_lds_bins(16 * 36)) <= 163840, "four 64-windows per CU at 16 x 36");

// One pass of the T/2 transforms: every butterfly loaded and computed, a
// barrier, every butterfly stored, a barrier.
template <int T, int R, int NS, class Idx>
__device__ __forceinline__ void win_pass(double2* buf, const double2* tw, int tid) {
    constexpr int NT = WinPlan<T>::kThreads, B = win_butterflies<T, R>(), ROUNDS = B / NT;
    static_assert(B % NT == 0 && ROUNDS >= 1, "whole rounds");
    double2 v[ROUNDS][R];
#pragma unroll
    for (int q = 0; q < ROUNDS; q++) win_bfly_load<T, R, NS, Idx>(buf, tw, tid + q * NT, v[q]);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ROUNDS; q++) win_bfly_store<T, R, NS, Idx>(buf, tid + q * NT, v[q]);
    __syncthreads();
}

// A block's LDS, and steps 1 to 5 of a window: from its RGB bytes to its nbins
// fixed-point bin sums in s.lb and the waves' maxima of p in s.red (as doubles,
// one per wave), behind a barrier.  Shared by k_window_blur and k_window_vectors.
template <int T>
struct WinLds {
    double2* buf;                  // win_elems(T): the spectrum
    double2* tw;                   // T twiddles
    double2* lt;                   // the log table
    unsigned long long* red;       // 4 per wave: the channel sums, then the maxima
    unsigned long long* lb;        // the bins (k / 255.0 until step 3 is done)
};
template <int T>
__device__ __forceinline__ WinLds<T> win_lds(unsigned char* smem) {
    WinLds<T> s;
    s.buf = reinterpret_cast<double2*>(smem);
    s.tw = s.buf + win_elems(T);
    s.lt = s.tw + T;
    s.red = reinterpret_cast<unsigned long long*>(s.lt + kLogTab);
    s.lb = s.red + 4 * (WinPlan<T>::kThreads / 64);
    return s;
}
template <int T>
__device__ __forceinline__ void win_bin_sums(const WinRec rec, const double2* __restrict__ twg,
                                             const uint16_t* __restrict__ binmap, int nbins, double bscale,
                                             const WinLds<T>& s, int tid) {
    using P = WinPlan<T>;
    constexpr int NT = P::kThreads, NW = NT / 64;
    double2* buf = s.buf;
    double2* tw = s.tw;
    double2* lt = s.lt;
    unsigned long long* red = s.red;
    unsigned long long* lb = s.lb;
    double* k255 = reinterpret_cast<double*>(lb);            // until step 3 is done

    // 1. the window's rows as 4-pixel units (12 bytes, three words at the unit's
    //    own address: no byte outside the window is read)
    constexpr int UPR = T / 4, UNITS = T * UPR, PER = UNITS / NT;
    static_assert(UNITS % NT == 0, "whole units per thread");
    unsigned w[PER][3];
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int u = tid + j * NT, y = u / UPR, k = u - y * UPR;
        stat_words_global(rec.first + (long long)y * rec.pitch + 12 * k, w[j]);
    }
    for (int i = tid; i < T; i += NT) tw[i] = twg[i];
    for (int i = tid; i < 256; i += NT) k255[i] = (double)i / 255.0;
    log_table_init(lt, tid, NT);

    // 2. the exact channel sums and avg
    unsigned sr = 0, sg = 0, sb = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const unsigned w0 = w[j][0], w1 = w[j][1], w2 = w[j][2];
        sr += (w0 & 255u) + (w0 >> 24) + (w1 >> 16 & 255u) + (w2 >> 8 & 255u);
        sg += (w0 >> 8 & 255u) + (w1 & 255u) + (w1 >> 24) + (w2 >> 16 & 255u);
        sb += (w0 >> 16 & 255u) + (w1 >> 8 & 255u) + (w2 & 255u) + (w2 >> 24);
    }
    sr = wave_sum(sr);
    sg = wave_sum(sg);
    sb = wave_sum(sb);
    if (lane_id() == 0) {
        red[4 * (tid >> 6)] = sr;
        red[4 * (tid >> 6) + 1] = sg;
        red[4 * (tid >> 6) + 2] = sb;
    }
    __syncthreads();
    unsigned long long tr = 0, tg = 0, tb = 0;
#pragma unroll
    for (int q = 0; q < NW; q++) {
        tr += red[4 * q];
        tg += red[4 * q + 1];
        tb += red[4 * q + 2];
    }
    const double avg = win_avg<T>(tr, tg, tb);

    // 3. luma - avg: rows 2p and 2p+1 are the two parts of complex row p
    {
        double* bd = reinterpret_cast<double*>(buf);
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int u = tid + j * NT, y = u / UPR, x = 4 * (u - y * UPR);
            const unsigned w0 = w[j][0], w1 = w[j][1], w2 = w[j][2];
            double* d = bd + 2 * win_pixel_slot<T>(y, x) + (y & 1);
            d[0] = win_luma(k255, w0 & 255u, w0 >> 8 & 255u, w0 >> 16 & 255u, avg);
            d[2] = win_luma(k255, w0 >> 24, w1 & 255u, w1 >> 8 & 255u, avg);
            d[4] = win_luma(k255, w1 >> 16 & 255u, w1 >> 24, w2 & 255u, avg);
            d[6] = win_luma(k255, w2 >> 8 & 255u, w2 >> 16 & 255u, w2 >> 24, avg);
        }
    }
    __syncthreads();
    for (int i = tid; i < nbins; i += NT) lb[i] = 0ull;      // k255 has been used: the bins take its place

    // 4. rows, separation, columns
    win_pass<T, P::R0, 1, WinRowIdx<T>>(buf, tw, tid);
    win_pass<T, P::R1, P::R0, WinRowIdx<T>>(buf, tw, tid);
    for (int i = tid; i < (T / 2) * (T / 2); i += NT) win_separate<T>(buf, i);
    __syncthreads();
    win_pass<T, P::R0, 1, WinColIdx<T>>(buf, tw, tid);
    win_pass<T, P::R1, P::R0, WinColIdx<T>>(buf, tw, tid);

    // 5. p = re re + im im (src/fft_processing.c:49), the maximum, log p for p >= 1
    //    (:197-198) into the element's polar bin (binmap[x][u], src/blur_profile.c:87-100)
    double mx = 0.0;
    constexpr int WF = T / 2 + 1;
    //    (adjacent threads, adjacent columns: adjacent LDS elements; the 2 T WF bytes
    //    of bin ids stay in the CU's cache)
    for (int i = tid; i < T * WF; i += NT) {
        const int u = i / WF, x = i - u * WF;
        const double2 X = win_spectrum<T>(buf, u, x);
        const double p = X.x * X.x + X.y * X.y;
        mx = fmax(mx, p);
        if (p >= 1) atomicAdd(&lb[binmap[x * T + u]], bin_fixed(log_mant(p, lt), bscale));
    }
    mx = wave_max(mx);
    double* redd = reinterpret_cast<double*>(red);
    if (lane_id() == 0) redd[tid >> 6] = mx;            // (red's sums were read before the barriers above)
    __syncthreads();
}

// One block per window.  recs[w]: the window's first byte and its image's row
// pitch.  out: per window nbins u64 bin sums (bin_scale(T, T/2+1) fixed point),
// fmax: per window the largest p.  Plain stores: a window has one owner.
template <int T>
__global__ __launch_bounds__(WinPlan<T>::kThreads) void k_window_blur(const WinRec* __restrict__ recs,
                                                                      const double2* __restrict__ twg,
                                                                      const uint16_t* __restrict__ binmap, int nbins,
                                                                      double bscale,
                                                                      unsigned long long* __restrict__ out,
                                                                      double* __restrict__ fmax_out) {
    constexpr int NT = WinPlan<T>::kThreads, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WinLds<T> s = win_lds<T>(smem);
    const int tid = threadIdx.x;
    win_bin_sums<T>(recs[blockIdx.x], twg, binmap, nbins, bscale, s, tid);
    const unsigned long long* lb = s.lb;
    const double* redd = reinterpret_cast<const double*>(s.red);

    // 6. the bins and the maximum, once
    unsigned long long* o = out + (size_t)blockIdx.x * nbins;
    for (int i = tid; i < nbins; i += NT) o[i] = lb[i];
    if (tid == 0) {
        double m = 0.0;
#pragma unroll
        for (int q = 0; q < NW; q++) m = fmax(m, redd[q]);
        fmax_out[blockIdx.x] = m;
    }
}

// k_window_blur's steps 1 to 5, then the finish (blur_window.h) in the same block:
// the window's ten Blur_Vectors to dst[w].vectors and its spectrum maximum to
// dst[w].fft_max (or nowhere: NULL).  The bins never leave LDS.  After step 5 the
// spectrum, the twiddles and the log table are dead: the per-angle totals, the
// smoothed totals and the maxima live at smem + scr_off (0: over the spectrum;
// the launcher places them behind the bins where 16 na + 64 bytes do not fit
// there), and the flat bins replace the u64 sums in place.
//   6. gs from the maximum (every thread: one fp64 log each, no barrier), one
//      thread per bin: flat[b];                                        barrier
//   7. one thread per angle: tot[i];                                   barrier
//   8. one thread per angle: the smoothed tot[i]; the last thread: avg; barrier
//   9. the last thread: the ordered scan for maxima;                   barrier
//  10. one thread per vector: win_vector of its maximum, or zeros.
template <int T>
__global__ __launch_bounds__(WinPlan<T>::kThreads) void k_window_vectors(
    const WinRec* __restrict__ recs, const WinDst* __restrict__ dst, const double2* __restrict__ twg,
    const uint16_t* __restrict__ binmap, const uint16_t* __restrict__ counts, int nbins, int na, int nr, int rc,
    double bscale, double streak, double mag, int scr_off) {
    constexpr int NT = WinPlan<T>::kThreads, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WinLds<T> s = win_lds<T>(smem);
    const int tid = threadIdx.x;
    win_bin_sums<T>(recs[blockIdx.x], twg, binmap, nbins, bscale, s, tid);
    const WinDst d = dst[blockIdx.x];
    unsigned long long* lb = s.lb;
    const double* redd = reinterpret_cast<const double*>(s.red);
    const double* flat = reinterpret_cast<const double*>(lb);
    double* tot = reinterpret_cast<double*>(smem + scr_off);
    double* sm = tot + na;
    double* avgp = sm + na;                                  // avg, then m and the maxima's angle bins
    int* mx = reinterpret_cast<int*>(avgp + 1);

    double fm = 0.0;
#pragma unroll
    for (int q = 0; q < NW; q++) fm = fmax(fm, redd[q]);
    const double gs = win_gs(fm);
    for (int i = tid; i < nbins; i += NT)
        lb[i] = (unsigned long long)__double_as_longlong(win_flat_bin(lb[i], bscale, gs, counts[i]));
    __syncthreads();
    for (int i = tid; i < na; i += NT) tot[i] = win_angle_total(flat, nr, rc, i);
    __syncthreads();
    for (int i = tid; i < na; i += NT) sm[i] = win_smooth(tot, na, i);
    double avg = 0.0;
    if (tid == NT - 1) avg = win_angle_avg(tot, na);
    __syncthreads();
    if (tid == NT - 1) {
        mx[0] = win_maxima(sm, na, avg * streak, mx + 1);
        avgp[0] = avg;
    }
    __syncthreads();
    if (tid < kWinVectors) {
        WinVector v;
        v.angle = 0;
        v.magnitude = 0.0f;
        if (tid < mx[0]) v = win_vector(flat, na, nr, rc, avgp[0], mag, mx[1 + tid]);
        // (4-byte stores: the vectors are 4-byte aligned)
        d.vectors[tid].angle = v.angle;
        d.vectors[tid].magnitude = v.magnitude;
    }
    if (tid == 0 && d.fft_max) *d.fft_max = fm;
}

template <int T>
hipError_t launch_t(const WinRec* d_recs, int n, const double2* d_tw, const uint16_t* d_binmap, int nbins,
                    unsigned long long* d_bins, double* d_fmax, hipStream_t st) {
    static bool once = ((void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_window_blur<T>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                        true);
    (void)once;
    const size_t lds = win_lds_fixed<T>() + win_lds_bins(nbins);
    phd_launch(k_window_blur<T>, dim3(n), dim3(WinPlan<T>::kThreads), lds, st, d_recs, d_tw, d_binmap, nbins,
               bin_scale(T, T / 2 + 1), d_bins, d_fmax);
    return hipGetLastError();
}

// bytes of k_window_vectors' totals, smoothed totals, avg and maxima
constexpr size_t win_scratch(int na) { return 16 * (size_t)na + 64; }

template <int T>
hipError_t launch_vectors_t(const WinRec* d_recs, const WinDst* d_dst, int n, const double2* d_tw,
                            const uint16_t* d_binmap, const uint16_t* d_counts, int na, int nr, int denom,
                            double streak, double mag, hipStream_t st) {
    static bool once = ((void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_window_vectors<T>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                        true);
    (void)once;
    const int nbins = na * nr;
    size_t lds = win_lds_fixed<T>() + win_lds_bins(nbins);
    // the scratch lies over the dead spectrum, twiddles and log table (everything before the waves'
    // partials); only T = 64 with more than 2172 angle bins (and so one radius bin) needs bytes of its own
    constexpr size_t dead = sizeof(double2) * (win_elems(T) + T + kLogTab);
    static_assert(T == 64 || win_scratch(kWinMaxBins) <= dead, "the scratch of any grid fits a 128-window's spectrum");
    size_t scr_off = 0;
    if (win_scratch(na) > dead) {
        scr_off = lds;
        lds += win_scratch(na);
    }
    if (lds > 163840) return hipErrorInvalidValue;
    phd_launch(k_window_vectors<T>, dim3(n), dim3(WinPlan<T>::kThreads), lds, st, d_recs, d_dst, d_tw, d_binmap,
               d_counts, nbins, na, nr, nr / denom, bin_scale(T, T / 2 + 1), streak, mag, (int)scr_off);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_window_vectors(int T, const WinRec* d_recs, const WinDst* d_dst, int n, const double2* d_tw,
                                 const uint16_t* d_binmap, const uint16_t* d_counts, int na, int nr, int denom,
                                 double streak, double mag, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (na < 2 || nr <= 0 || denom <= 0 || (long long)na * nr > kWinMaxBins || !win_size_ok(T))
        return hipErrorInvalidValue;
    return T == 64 ? launch_vectors_t<64>(d_recs, d_dst, n, d_tw, d_binmap, d_counts, na, nr, denom, streak, mag, st)
                   : launch_vectors_t<128>(d_recs, d_dst, n, d_tw, d_binmap, d_counts, na, nr, denom, streak, mag, st);
}

hipError_t launch_window_blur(int T, const WinRec* d_recs, int n, const double2* d_tw, const uint16_t* d_binmap,
                              int nbins, unsigned long long* d_bins, double* d_fmax, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (nbins <= 0 || nbins > kWinMaxBins || !win_size_ok(T)) return hipErrorInvalidValue;
    return T == 64 ? launch_t<64>(d_recs, n, d_tw, d_binmap, nbins, d_bins, d_fmax, st)
                   : launch_t<128>(d_recs, n, d_tw, d_binmap, nbins, d_bins, d_fmax, st);
}

void window_twiddles(int T, double2* tw) { win_twiddles(T, tw); }

// The kernel's steps on the host, one window: the same sums, avg, luma, plan,
// passes and index maps; the log is the C library's.
template <int T>
static void bins_host_t(const uint8_t* first, long long pitch, const uint16_t* binmap, int nbins,
                        unsigned long long* bins, double* fmax_out) {
    std::vector<double2> buf(win_elems(T)), tmp(win_elems(T)), tw(T);
    win_twiddles(T, tw.data());
    double k255[256];
    for (int k = 0; k < 256; k++) k255[k] = (double)k / 255.0;
    unsigned long long s[3] = {0, 0, 0};
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++)
            for (int c = 0; c < 3; c++) s[c] += first[y * pitch + 3 * x + c];
    const double avg = win_avg<T>(s[0], s[1], s[2]);
    double* bd = reinterpret_cast<double*>(buf.data());
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++) {
            const uint8_t* px = first + y * pitch + 3 * x;
            bd[2 * win_pixel_slot<T>(y, x) + (y & 1)] = win_luma(k255, px[0], px[1], px[2], avg);
        }
    win_transform_host<T>(buf.data(), tw.data(), tmp.data());
    const double scale = bin_scale(T, T / 2 + 1);
    for (int b = 0; b < nbins; b++) bins[b] = 0ull;
    double mx = 0.0;
    for (int i = 0; i < T * (T / 2 + 1); i++) {
        const int x = i / T, u = i - x * T;
        const double2 X = win_spectrum<T>(buf.data(), u, x);
        const double p = X.x * X.x + X.y * X.y;
        mx = std::fmax(mx, p);
        if (p >= 1) bins[binmap[i]] += (unsigned long long)std::nearbyint(std::log(p) * scale);
    }
    *fmax_out = mx;
}

void window_bins_host(int T, const uint8_t* first, long long pitch, const uint16_t* binmap, int nbins,
                      unsigned long long* bins, double* fmax_out) {
    if (T == 64) bins_host_t<64>(first, pitch, binmap, nbins, bins, fmax_out);
    else bins_host_t<128>(first, pitch, binmap, nbins, bins, fmax_out);
}

}  // namespace phd
