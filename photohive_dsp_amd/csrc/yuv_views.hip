// yuv_views.hip -- the input stage for decoder output: 8-bit YCbCr frames (NV12
// / NV21, planar 4:2:0, 4:2:2, 4:4:4, packed YUY2 / UYVY; pitched, regions)
// converted into packed RGB8 images.
//
// One launch converts every view of a run: the grid is (row band, view), a
// block reads its view's record from the device table, so the layout,
// subsampling, matrix and chroma-mode branches are uniform over the block.  A
// band is about 16 KB of destination rows and starts on an even row of a
// 4:2:0 view (yuv_band_rows), so the two destination rows of a chroma row are
// read by one block.  Wide rows are taken by the whole block one after the
// other, narrow rows one per wave, so consecutive lanes always write
// consecutive 12-byte units.  The row itself -- split, addresses, upsampling,
// matrix -- is yuv_row (yuv_view.h), shared with the host twin.
#include "phd_device.h"

#include "yuv_view.h"

namespace phd {

namespace {

// rows of at least this many pixels are taken by the whole block
constexpr int kYuvWideRow = 512;

__global__ __launch_bounds__(kThreads) void k_yuv_views(const YuvRec* __restrict__ recs) {
    const YuvRec r = recs[blockIdx.y];
    const int y0 = (int)blockIdx.x * r.band_rows;
    if (y0 >= r.height) return;
    const int y1 = min(r.height, y0 + r.band_rows);
    if (r.width >= kYuvWideRow) {
        for (int y = y0; y < y1; y++) yuv_row(r, y, (int)threadIdx.x, kThreads);
    } else {
        const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
        for (int y = y0 + wave; y < y1; y += kThreads / 64) yuv_row(r, y, lane, 64);
    }
}

}  // namespace

hipError_t launch_yuv_views(const YuvRec* d_recs, int n, int max_bands, hipStream_t st, KernelProfiler* prof) {
    if (n <= 0 || max_bands <= 0) return hipSuccess;
    const int ps = prof_begin_kernel(prof, kProfYuv, st);
    phd_launch(k_yuv_views, dim3(max_bands, n), dim3(kThreads), 0, st, d_recs);
    prof_end(prof, ps, st);
    return hipGetLastError();
}

}  // namespace phd
