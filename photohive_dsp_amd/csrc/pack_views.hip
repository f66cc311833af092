// pack_views.hip -- the input stage: byte-strided image views (planar,
// pitched, 4-byte pixels, anything else) gathered into packed RGB8 images.
//
// One launch packs every view of a run: the grid is (row band, view), a block
// reads its view's record from the device table, so the kind branch is uniform
// over the block.  A band is about 32 KB of destination rows (pack_band_rows).
// Wide rows are taken by the whole block one after the other, narrow rows one
// per wave, so consecutive lanes always write consecutive 12-byte units (or
// 16-byte units of a pitched row).  The row itself -- split, addresses,
// shuffles -- is pack_row (pack_view.h), shared with the host twin.
#include "phd_device.h"

#include "pack_view.h"

namespace phd {

namespace {

// rows of at least this many pixels are taken by the whole block
constexpr int kPackWideRow = 512;

__global__ __launch_bounds__(kThreads) void k_pack_views(const PackRec* __restrict__ recs) {
    const PackRec r = recs[blockIdx.y];
    const int y0 = (int)blockIdx.x * r.band_rows;
    if (y0 >= r.height) return;
    const int y1 = min(r.height, y0 + r.band_rows);
    if (r.width >= kPackWideRow) {
        for (int y = y0; y < y1; y++) pack_row(r, y, (int)threadIdx.x, kThreads);
    } else {
        const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
        for (int y = y0 + wave; y < y1; y += kThreads / 64) pack_row(r, y, lane, 64);
    }
}

}  // namespace

hipError_t launch_pack_views(const PackRec* d_recs, int n, int max_bands, hipStream_t st, KernelProfiler* prof) {
    if (n <= 0 || max_bands <= 0) return hipSuccess;
    const int ps = prof_begin_pack(prof, st);
    phd_launch(k_pack_views, dim3(max_bands, n), dim3(kThreads), 0, st, d_recs);
    prof_end(prof, ps, st);
    return hipGetLastError();
}

}  // namespace phd
