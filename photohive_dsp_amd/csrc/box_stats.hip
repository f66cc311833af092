// box_stats.hip -- the box statistics: per crop box of a packed RGB8 image the
// exact integer sums behind get_rgb_statistics (src/image_processing.c:543-553)
// and get_hsv_average over rgb2hsv's s (src/image_processing.c:533-540,
// 372-417) on crop_image's box (src/image_processing.c:244-266).  Records, plan
// and row walk: box_stat_tiles.h; the 4-pixel unit: stat_unit.h (stats.hip's).
#include "phd_device.h"
#include "box_stat_tiles.h"

namespace phd {

namespace {

// per-lane copies of the 256-bucket sum-of-d-per-max histogram, as k_rgb_stats
// keeps them (padded to 257 so lanes fall on distinct banks)
constexpr int kBsCopies = 32, kBsPad = 257;
constexpr int kBsWaves = kBoxStatThreads / 64;
static_assert(kBoxStatThreads >= 256 && kBoxStatThreads % 64 == 0, "thread t < 256 folds bucket t");
// One fold covers at most kBoxStatPassUnits units plus the tails of one item
// (<= kBoxBandElems pixels): per thread <= 4 * 2^20 / 256 + 65536 / 256 + 4
// pixels, per LDS copy 8 threads' worth.
constexpr long long kBsFoldPix = 4LL * kBoxStatPassUnits / kBoxStatThreads + kBoxBandElems / kBoxStatThreads + 4;
static_assert(kBsFoldPix * 255 * 255 < (1LL << 32), "per-thread u32 sums of squares");
static_assert(kBsFoldPix * (kBoxStatThreads / kBsCopies) * 255 < (1LL << 32), "u32 LDS buckets");
static_assert(kBsFoldPix < 65536, "packed u16 min == 0 < max counts");

// Every box of every image of a call in one launch.  Persistent blocks take
// contiguous runs of box_plan's items.  Per item (and pass) the block's threads
// take the units strided, kBoxStatBatch loads ahead of their adds; the pass is
// folded into the block's u64 sums in LDS (acc: slot t and bucket t are thread
// t's own), and those are added to the box's record when the run leaves the
// box: u64 integer atomics, so the record does not depend on the order the
// items finish in.
__global__ __launch_bounds__(kBoxStatThreads) void k_box_stats(const BoxStatRec* __restrict__ recs,
                                                               const BoxItem* __restrict__ items, int nitems,
                                                               unsigned long long* __restrict__ out) {
    __shared__ unsigned hist[kBsCopies * kBsPad];
    __shared__ unsigned long long red[kBsWaves][8];
    __shared__ unsigned long long acc[kBoxStatRec];
    const int tid = threadIdx.x;
    unsigned* hk = hist + (tid & (kBsCopies - 1)) * kBsPad;
    for (int i = tid; i < kBsCopies * kBsPad; i += kBoxStatThreads) hist[i] = 0u;
    for (int i = tid; i < kBoxStatRec; i += kBoxStatThreads) acc[i] = 0ull;
    __syncthreads();
    const int it0 = (int)((long)blockIdx.x * nitems / gridDim.x);
    const int it1 = (int)((long)(blockIdx.x + 1) * nitems / gridDim.x);
    for (int it = it0; it < it1; it++) {                    // block-uniform
        const BoxItem item = items[it];
        const BoxStatRec r = recs[item.box];
        const int cols = r.right - r.left, rows = item.row1 - item.row0, nu = box_stat_row_units(cols);
        const int total = rows * nu;                        // <= kBoxBandElems / 4, or one row's
        const long long pitch = 3LL * r.w;
        const uint8_t* base = r.img + 3LL * ((long long)item.row0 * r.w + r.left);
        for (int u0 = 0; u0 == 0 || u0 < total; u0 += kBoxStatPassUnits) {
            StatAcc a{0, 0, 0, 0, 0, 0, 0.0, {0, 0}};
            box_stat_units<kBoxStatBatch>(
                base, pitch, nu, u0, min(total, u0 + kBoxStatPassUnits), tid, kBoxStatThreads,
                [&](const uint8_t* const* q, int m) {
                    unsigned w[kBoxStatBatch][3];
                    if (m == kBoxStatBatch) {
#pragma unroll
                        for (int j = 0; j < kBoxStatBatch; j++) stat_words_global(q[j], w[j]);
#pragma unroll
                        for (int j = 0; j < kBoxStatBatch; j++) stat4(w[j][0], w[j][1], w[j][2], a, hk);
                    } else {
                        for (int j = 0; j < m; j++) {
                            stat_words_global(q[j], w[0]);
                            stat4(w[0][0], w[0][1], w[0][2], a, hk);
                        }
                    }
                });
            if (u0 == 0)
                box_stat_tails(base, pitch, cols, rows, tid, kBoxStatThreads,
                               [&](const uint8_t* p) { stat1(p, a, hk); });
            // fold the pass: the threads' moments by wave, then the LDS copies
            const unsigned mom[7] = {a.sr, a.sg, a.sb, a.qr, a.qg, a.qb, (unsigned)a.n1.x + (unsigned)a.n1.y};
            unsigned long long m64[7];
#pragma unroll
            for (int k = 0; k < 7; k++) m64[k] = wave_sum((unsigned long long)mom[k]);
            if (lane_id() == 0) {
#pragma unroll
                for (int k = 0; k < 7; k++) red[tid >> 6][k] = m64[k];
            }
            __syncthreads();
            if (tid < 256) {
                unsigned long long b = 0;
#pragma unroll 8
                for (int k = 0; k < kBsCopies; k++) {
                    b += hist[k * kBsPad + tid];
                    hist[k * kBsPad + tid] = 0u;
                }
                acc[8 + tid] += b;
            }
            if (tid < 7) {
                unsigned long long t = 0;
                for (int q = 0; q < kBsWaves; q++) t += red[q][tid];
                acc[tid] += t;
            }
            __syncthreads();                                // red and the copies are reused by the next pass
        }
        if (it + 1 == it1 || items[it + 1].box != item.box) {
            unsigned long long* rec = out + (size_t)item.box * kBoxStatRec;
            if (tid < 256) {
                const unsigned long long b = acc[8 + tid];
                if (b) atomicAdd(&rec[8 + tid], b);
                acc[8 + tid] = 0ull;
            }
            if (tid < 7) {
                const unsigned long long t = acc[tid];
                if (t) atomicAdd(&rec[tid], t);
                acc[tid] = 0ull;
            }
        }
    }
}

// One thread per box, in the manner of k_stats_finish: S in the definition's
// order (ascending m, sequential) and the 64 bytes the host downloads.
__global__ __launch_bounds__(64) void k_box_stats_finish(const unsigned long long* __restrict__ rec, int nboxes,
                                                         unsigned long long* __restrict__ fin) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nboxes) return;
    const unsigned long long* r = rec + (size_t)b * kBoxStatRec;
    unsigned long long* o = fin + (size_t)b * kBoxStatOut;
    for (int k = 0; k < 7; k++) o[k] = r[k];
    o[7] = __builtin_bit_cast(unsigned long long, box_stat_s(r + 8));
}

}  // namespace

hipError_t launch_box_stats(const BoxStatRec* d_recs, const BoxItem* d_items, int nitems, unsigned long long* d_out,
                            hipStream_t st) {
    if (nitems <= 0) return hipSuccess;
    // persistent blocks: as many as are resident at once
    static const int per_cu = [] {
        int b = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, (const void*)k_box_stats, kBoxStatThreads, 0) ==
                       hipSuccess && b > 0 ? b : 1;
    }();
    const int grid = (int)std::min<long>(nitems, (long)per_cu * num_cus());
    phd_launch(k_box_stats, dim3(grid), dim3(kBoxStatThreads), 0, st, d_recs, d_items, nitems, d_out);
    return hipGetLastError();
}

hipError_t launch_box_stats_finish(const unsigned long long* d_rec, int nboxes, unsigned long long* d_fin,
                                   hipStream_t st) {
    if (nboxes <= 0) return hipSuccess;
    phd_launch(k_box_stats_finish, dim3((nboxes + 63) / 64), dim3(64), 0, st, d_rec, nboxes, d_fin);
    return hipGetLastError();
}

}  // namespace phd
