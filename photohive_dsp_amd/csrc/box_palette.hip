// box_palette.hip -- the box palettes: per crop box of a palette label map, the
// number of elements of every palette slot (the lists of
// src/color_quantization.c:342-479, counted inside crop_pgm's box,
// src/image_processing.c:213-232).  Plan and row code: box_tiles.h.
#include "phd_device.h"
#include "box_tiles.h"

namespace phd {

namespace {

// Every box of every map of a call in one launch.  Persistent blocks take
// contiguous runs of box_plan's items.  Per item the block counts into LDS:
// box_copies private copies of the box's n_slots + 1 counters, thread t on copy
// t % copies (64 copies for the common palettes of up to 127 slots: no two
// lanes of a wave on one copy, so a single-colour box does not serialise on
// one address), units of four labels strided over the threads.  The copies
// are then summed and the non-zero counters added to the box's row of `counts`
// (zeroed by the host before the launch): integer atomics, so the result does
// not depend on the order the items finish in.
__global__ __launch_bounds__(kBoxThreads) void k_box_counts(const BoxRec* __restrict__ recs,
                                                            const BoxItem* __restrict__ items, int nitems,
                                                            unsigned* __restrict__ counts) {
    __shared__ unsigned hist[kBoxLdsCounters];
    const int tid = threadIdx.x;
    const int it0 = (int)((long)blockIdx.x * nitems / gridDim.x);
    const int it1 = (int)((long)(blockIdx.x + 1) * nitems / gridDim.x);
    for (int it = it0; it < it1; it++) {                    // block-uniform
        const BoxItem item = items[it];
        const BoxRec r = recs[item.box];
        const int cols = r.right - r.left, nu = box_row_units(cols);
        const int total = (item.row1 - item.row0) * nu;     // < 2 kBoxBandElems, or one row's
        const int nc = r.n_slots + 1, copies = box_copies(nc, total), used = copies * nc;
        for (int i = tid; i < used; i += kBoxThreads) hist[i] = 0;
        __syncthreads();
        unsigned* my = hist + (tid % copies) * nc;
        const uint16_t* base = r.map + (long)item.row0 * r.mw + r.left;
        for (int u = tid; u < total; u += kBoxThreads) {
            const int row = u / nu, k = u - row * nu;
            box_unit(base + (long)row * r.mw, cols, k, r.n_slots,
                     [&](unsigned slot, unsigned n) { atomicAdd(&my[slot], n); });
        }
        __syncthreads();
        for (int s = tid; s < nc; s += kBoxThreads) {
            unsigned sum = 0;
            for (int c = 0; c < copies; c++) sum += hist[c * nc + s];
            if (sum) atomicAdd(&counts[r.out + s], sum);
        }
        __syncthreads();                                    // the next item zeroes the copies
    }
}

}  // namespace

hipError_t launch_box_counts(const BoxRec* d_recs, const BoxItem* d_items, int nitems, unsigned* d_counts,
                             hipStream_t st) {
    if (nitems <= 0) return hipSuccess;
    // persistent blocks: as many as are resident at once (32 KiB of LDS each)
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_box_counts, kBoxThreads, 0) != hipSuccess ||
        per_cu < 1)
        per_cu = 1;
    const int grid = (int)std::min<long>(nitems, (long)per_cu * num_cus());
    phd_launch(k_box_counts, dim3(grid), dim3(kBoxThreads), 0, st, d_recs, d_items, nitems, d_counts);
    return hipGetLastError();
}

}  // namespace phd
