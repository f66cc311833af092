// decode_views.hip -- the typed input stage: byte-strided views of 8- / 16-bit
// integers, halves, floats or doubles decoded to the reference's Pixels
// ((double)x / max_value, src/types.h:5).
//
// k_classify_views: one launch for every typed view of a run, grid (row band,
// view) as k_pack_views.  It fuses the gather, the decode and the 8-bit test
// of k_planar_to_u8 (planar.hip): each view's packed RGB8 image j = rint(v *
// 255) goes to its staging image and its flag word says whether some value is
// not j / 255.0 (the image then takes the fp64 pipeline) or not finite.
// k_decode_view: one view into three planes of doubles, for the images the
// classifier flagged and for phd_decode_views_device.
//
// Both are element-wise and memory-bound (2-8 source bytes per element, 3 or
// 24 destination bytes per pixel).  A lane takes a unit of pixels with vector
// loads and stores wherever the row allows (decode_view.h: the row's split,
// addresses and the span rule, shared with the host twin): 2 pixels where the
// planes are written, so that a wave's 16-byte stores are consecutive, 8 where
// only the RGB8 image is (measured).  Wide rows are
// taken by the whole block, narrow rows one per wave.
#include "phd_device.h"

#include "decode_view.h"

namespace phd {

namespace {

// rows of at least this many pixels are taken by the whole block
constexpr int kDecodeWideRow = 2048;

__device__ __forceinline__ void decode_band(const DecodeRec& r, int* __restrict__ flag) {
    const int y0 = (int)blockIdx.x * r.band_rows;
    if (y0 >= r.height) return;
    const int y1 = min(r.height, y0 + r.band_rows);
    int bits = 0;
    if (r.width >= kDecodeWideRow) {
        for (int y = y0; y < y1; y++) bits |= decode_row(r, y, (int)threadIdx.x, kThreads);
    } else {
        const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
        for (int y = y0 + wave; y < y1; y += kThreads / 64) bits |= decode_row(r, y, lane, 64);
    }
    if (!flag) return;
    const int w = (__any(bits & kDecNotU8) ? kDecNotU8 : 0) | (__any(bits & kDecNonFinite) ? kDecNonFinite : 0);
    if (w && lane_id() == 0) atomicOr(flag, w);
}

__global__ __launch_bounds__(kThreads) void k_classify_views(const DecodeRec* __restrict__ recs,
                                                            int* __restrict__ flags) {
    const DecodeRec r = recs[blockIdx.y];
    decode_band(r, flags + blockIdx.y);
}

__global__ __launch_bounds__(kThreads) void k_decode_view(const DecodeRec r) { decode_band(r, nullptr); }

}  // namespace

hipError_t launch_classify_views(const DecodeRec* d_recs, int* d_flags, int n, int max_bands, hipStream_t st,
                                 KernelProfiler* prof) {
    if (n <= 0 || max_bands <= 0) return hipSuccess;
    const int ps = prof_begin_kernel(prof, kProfClassify, st);
    phd_launch(k_classify_views, dim3(max_bands, n), dim3(kThreads), 0, st, d_recs, d_flags);
    prof_end(prof, ps, st);
    return hipGetLastError();
}

hipError_t launch_decode_view(const DecodeRec& rec, hipStream_t st, KernelProfiler* prof) {
    const int bands = (rec.height + rec.band_rows - 1) / rec.band_rows;
    const int ps = prof_begin_kernel(prof, kProfDecode, st);
    phd_launch(k_decode_view, dim3(bands), dim3(kThreads), 0, st, rec);
    prof_end(prof, ps, st);
    return hipGetLastError();
}

}  // namespace phd
