// stats.hip -- the rgb2hsv + RGB statistics pass alone (BASELINE config 3):
// per image the channel moments (sum k, sum k^2 for r, g, b) and the sum of
// the HSV saturation s.
//
// Replaces the per-pixel loops of get_rgb_statistics / get_average /
// get_variance (src/image_processing.c:543-553, src/filtering.c:125-148) and
// get_hsv_average over rgb2hsv's s channel (src/image_processing.c:533-540,
// 408-414).  No group histogram: this is the HBM-streaming pass, sized so the
// VALU work per byte stays below the HBM rate.
//
// Per thread, 4 pixels = 12 bytes = one non-temporal dwordx3 load (a wave
// reads 768 contiguous bytes, streamed once: 0.74 of the HBM peak against
// 0.70-0.72 with plain loads).  The 12 bytes are regrouped by v_perm into six
// u16 pairs (R02 = {r0, r2}, R13 = {r1, r3}, likewise G and B); then per 4
// pixels:
//   * moments: v_dot2_u32_u16 of each pair with {1, 1} and with itself (exact
//     u32 per thread, flushed to u64 per run);
//   * max / min: v_pk_max_u16 / v_pk_min_u16, d = max - min (v_pk_sub).
// rgb2hsv's s is d / max except 0.999999 for d == max (min == 0 < max,
// src/image_processing.c:408-414), and it is never divided per pixel
// (the reference's width).  sum(s) = sum_m (sum of d over the pixels with max = m) / m
//                  - (1 - 0.999999) * #(min == 0 < max)
// (a d == max pixel adds m / m = 1 to the first term; 1 - 0.999999 is exact in
// fp64), so the pass only needs, per image, the exact integer sum of d per max
// value m: ONE u32 LDS atomic per pixel into a per-lane copy of a 256-bucket
// histogram (32 copies, padded to 257 so lanes fall on distinct banks), folded
// into the image's u64 buckets when a run ends; the host finishes the sum in
// fp64 (phd_hsv_stats_batch_device).  Within ~1e-15 of the reference's
// sequential fp64 sum of the per-pixel doubles.  (Rounds 2-3 measured fp32
// pair-quotient forms at 0.57-0.74 of the peak and 1e-6 to 2e-9 relative; git
// history.)  The full report's K1 (k1.hip) keeps the exact fp64 s.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "phd_device.h"
#include "stat_unit.h"

namespace phd {

namespace {

constexpr int kStThreads = 512;              // 8 waves; kChunk pixels per work item
constexpr int kStGroups = kChunk / (4 * kStThreads);
static_assert(kStGroups == 8, "stats tile");

typedef const __attribute__((address_space(1))) unsigned gu32s;

// (StatAcc and stat4, the 4-pixel unit: stat_unit.h, shared with box_stats.hip)

// One launch over a batch of same-size, 4-byte-aligned images.  Work items
// are (image, chunk of kChunk pixels); each persistent block takes one
// contiguous run of items and flushes its sums when the run leaves an image
// (or every 1024 items, so the u32 squares cannot overflow: 1024 * 8 groups *
// 4 * 255^2 < 2^32).  Outputs as K1's statistics-only form: out.sums (6 u64,
// atomics) and out.s_part[first chunk of the run] (one fp64 per run).
constexpr int kHistCopies = 32, kHistPad = 257;

__global__ __launch_bounds__(kStThreads, 8) void k_rgb_stats(const uint8_t* const* __restrict__ imgs, long npix,
                                                              int nchunks, long nitems, PaletteDev out,
                                                              long a_stride) {
    __shared__ unsigned long long red[kStThreads / 64][8];
    // sum of d per max value, one copy per lane of a half-wave
    __shared__ unsigned hist[kHistCopies * kHistPad];
    const int tid = threadIdx.x;
    unsigned* hk = hist + (tid & (kHistCopies - 1)) * kHistPad;
    for (int i = tid; i < kHistCopies * kHistPad; i += kStThreads) hist[i] = 0u;
    __syncthreads();
    const long it0 = (long)blockIdx.x * nitems / gridDim.x, it1 = (long)(blockIdx.x + 1) * nitems / gridDim.x;
    if (it0 >= it1) return;                                 // block-uniform
    const long full_end = npix & ~3L;                       // groups wholly inside the image
    int img = (int)(it0 / nchunks), c = (int)(it0 - (long)img * nchunks);
    const uint8_t* ip = imgs[img];
    StatAcc a{0, 0, 0, 0, 0, 0, 0.0, {0, 0}};
    int seg_c0 = c;
    long seg_it0 = it0;
    for (long it = it0; it < it1; it++) {
        const long base = (long)c * kChunk;
        // byte offsets fit 32 bits (pre_compute_error_checks caps images at 120 MP):
        // uniform base + u32 lane offset (saddr loads)
        const unsigned off0 = (unsigned)(3 * (base + 4L * tid));
        if (base + kChunk <= full_end) {                    // block-uniform: the whole chunk is inside
            unsigned w[kStGroups][3];
#pragma unroll
            for (int st = 0; st < kStGroups; st++) {
                gu32s* q = (gu32s*)(ip + (off0 + 12u * kStThreads * st));
                w[st][0] = __builtin_nontemporal_load(q);          // streamed once
                w[st][1] = __builtin_nontemporal_load(q + 1);
                w[st][2] = __builtin_nontemporal_load(q + 2);
            }
#pragma unroll
            for (int st = 0; st < kStGroups; st++) stat4(w[st][0], w[st][1], w[st][2], a, hk);
        } else {
#pragma unroll 1
            for (int st = 0; st < kStGroups; st++) {
                const long p0 = base + 4L * tid + 4L * kStThreads * st;
                if (p0 < full_end) {
                    gu32s* q = (gu32s*)(ip + 3 * p0);
                    stat4(q[0], q[1], q[2], a, hk);
                }
            }
        }
        if (tid == 0 && base + kChunk >= npix) {
            // the < 4 pixels of a partial final group: exact fp64 s
            for (long p = full_end; p < npix; p++) {
                const int kr = ip[3 * p], kg = ip[3 * p + 1], kb = ip[3 * p + 2];
                a.sr += kr; a.sg += kg; a.sb += kb;
                a.qr += kr * kr; a.qg += kg * kg; a.qb += kb * kb;
                a.s64 += sat_only(kr, kg, kb);                   // fp64 s (0.999999 included)
            }
        }
        const int cimg = img;
        if (++c == nchunks) {
            c = 0;
            img++;
        }
        const bool more = it + 1 < it1;
        if (more && img != cimg) ip = imgs[img];
        if (!more || img != cimg || it + 1 - seg_it0 == 1024) {
            const int wv = tid >> 6;
            const unsigned mom[6] = {a.sr, a.sg, a.sb, a.qr, a.qg, a.qb};
            unsigned long long m64[6];
#pragma unroll
            for (int k = 0; k < 6; k++) m64[k] = wave_sum((unsigned long long)mom[k]);
            // less (1 - 0.999999) per min == 0 < max pixel; the partial group's exact s
            const unsigned n1 = (unsigned)a.n1.x + (unsigned)a.n1.y;
            const double mine = __builtin_fma(-(1.0 - 0.999999), (double)n1, a.s64);
            const double sw = wave_sum(mine);
            if (lane_id() == 0) {
#pragma unroll
                for (int k = 0; k < 6; k++) red[wv][k] = m64[k];
                reinterpret_cast<double*>(red[wv])[6] = sw;
            }
            __syncthreads();
            {
                // the run's buckets into the image's (exact u64 sums, any order)
                if (tid < 256) {
                    unsigned long long b = 0;
#pragma unroll 8
                    for (int k = 0; k < kHistCopies; k++) {
                        b += hist[k * kHistPad + tid];
                        hist[k * kHistPad + tid] = 0u;
                    }
                    if (b)
                        atomicAdd(reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(out.kd_sum) +
                                                                        cimg * a_stride) + tid, b);
                }
            }
            if (tid < 6) {
                unsigned long long t = 0;
                for (int q = 0; q < kStThreads / 64; q++) t += red[q][tid];
                atomicAdd(reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(out.sums) + cimg * a_stride) +
                              tid,
                          t);
            } else if (tid == 6) {
                double t = 0.0;
                for (int q = 0; q < kStThreads / 64; q++) t += reinterpret_cast<const double*>(red[q])[6];
                // one slot per run (distinct first chunks)
                reinterpret_cast<double*>(reinterpret_cast<char*>(out.s_part) + cimg * a_stride)[seg_c0] = t;
            }
            a = StatAcc{0, 0, 0, 0, 0, 0, 0.0, {0, 0}};
            seg_c0 = c;
            seg_it0 = it + 1;
            __syncthreads();                                  // red is reused by the next flush
        }
    }
}

// The batch's per-image finish on the device (round 6; the host loop over
// each image's chunk partials and 255 sums of d per max value was ~0.2 ms of
// host time per 512-image call): one wave per image sums sum(s) = its chunk
// partials + sum_m (sum of d at max m) / m in a fixed order (strided lanes,
// then the xor butterfly: deterministic), and copies the six moments.  out:
// 8 u64 per image, the moments then the bits of sum(s) / npix.
__global__ __launch_bounds__(64) void k_stats_finish(const uint8_t* __restrict__ rec, long a_stride, long s_off,
                                                     long kd_off, int nchunks, long npix,
                                                     unsigned long long* __restrict__ out) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const uint8_t* a = rec + (size_t)i * a_stride;
    const double* sp = reinterpret_cast<const double*>(a + s_off);
    const unsigned long long* kd = reinterpret_cast<const unsigned long long*>(a + kd_off);
    double s = 0.0;
    for (int k = lane; k < nchunks; k += 64) s += sp[k];
    for (int m = lane; m < 256; m += 64)
        if (m > 0 && kd[m]) s += (double)kd[m] / (double)m;
    s = wave_sum(s);
    unsigned long long* o = out + (size_t)i * 8;
    if (lane < 6) o[lane] = reinterpret_cast<const unsigned long long*>(a)[lane];
    if (lane == 0) o[6] = __builtin_bit_cast(unsigned long long, s / (double)npix);
}

}  // namespace

hipError_t launch_stats_finish(const uint8_t* rec, int n, long a_stride, long s_off, long kd_off, int nchunks,
                               long npix, unsigned long long* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    phd_launch(k_stats_finish, dim3(n), dim3(64), 0, st, rec, a_stride, s_off, kd_off, nchunks, npix, out);
    return hipGetLastError();
}

hipError_t launch_rgb_stats_batch(const uint8_t* const* d_imgs, int n, int height, int width, const PaletteDev& out0,
                                  long a_stride, int nchunks, hipStream_t st) {
    const long npix = (long)height * width;
    const long nitems = (long)n * nchunks;
    if (!out0.kd_sum) return hipErrorInvalidValue;       // the sums of d per max value are the pass's s
    // the persistent grid: as many blocks as are resident at once
    static const int per_cu = [] {
        int b = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, (const void*)k_rgb_stats, kStThreads, 0) ==
                       hipSuccess && b > 0 ? b : 1;
    }();
    const int grid = (int)std::min<long>(nitems, (long)per_cu * num_cus());
    phd_launch(k_rgb_stats, dim3(grid), dim3(kStThreads), 0, st, d_imgs, npix, nchunks, nitems, out0, a_stride);
    return hipGetLastError();
}

}  // namespace phd
