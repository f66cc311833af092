// sharpness.hip -- Laplacian-variance sharpness of crop boxes.
//
// Replaces get_variance_sharpness (src/filtering.c:151-183): crop_pgm
// (src/image_processing.c:213-232) of the full-resolution luma, 3x3 Laplacian
// with zero padding at the CROP border (filter_image, filtering.c:81-107),
// then var(filtered) / mean(filtered) with the reference's two passes.
// The luma is recomputed from the RGB8 bytes; the filtered crop is never
// stored: pass 1 sums f, pass 2 sums (f - mean)^2.
//
// Two forms.  k_sharp_pass: one box of one image per launch, two launches per
// box (the single-image entries and the planar fp64 path).  k_sharp_tiles +
// k_sharp_finish: every box of every image of a batch call in one launch,
// single pass over LDS luma tiles, no atomics (the batch entries with
// per-image boxes; plan and merge order in sharp_tiles.h).
#include "phd_device.h"

namespace phd {

namespace {

// the luma of pixel i: rgb2pgm of the RGB8 bytes, or the fp64 plane (planar input)
__device__ __forceinline__ double luma(const uint8_t* __restrict__ img, const double* __restrict__ pgm, long i,
                                       const double* k255) {
    if (pgm) return pgm[i];
    return 0.299 * k255[img[3 * i]] + 0.587 * k255[img[3 * i + 1]] + 0.114 * k255[img[3 * i + 2]];
}

// f(y,x) of filter_image: sum over the 3x3 window in (fy, fx) order of
// input * coef, skipping taps outside the crop.
__device__ __forceinline__ double lap_at(const uint8_t* __restrict__ img, const double* __restrict__ pgm, int width,
                                         int top, int left, int ch, int cw, int y, int x, const double* k255) {
    double dp = 0.0;
#pragma unroll
    for (int fy = 0; fy < 3; fy++)
#pragma unroll
        for (int fx = 0; fx < 3; fx++) {
            const int iy = y + fy - 1, ix = x + fx - 1;
            if (iy >= 0 && iy < ch && ix >= 0 && ix < cw) {
                const double coef = (fy == 1 && fx == 1) ? 8.0 : -1.0;
                dp += luma(img, pgm, (long)(iy + top) * width + ix + left, k255) * coef;
            }
        }
    return dp;
}

__global__ __launch_bounds__(kThreads) void k_sharp_pass(const uint8_t* __restrict__ img,
                                                         const double* __restrict__ pgm, int width, int top,
                                                         int left, int ch, int cw,
                                                         const double* __restrict__ k255g,
                                                         const double* __restrict__ mean_src, long n_mean,
                                                         double* __restrict__ out) {
    __shared__ double k255[256];
    __shared__ double red[kThreads / 64];
    k255[threadIdx.x] = k255g[threadIdx.x];
    __syncthreads();
    const long n = (long)ch * cw;
    const double mean = mean_src ? *mean_src / (double)n_mean : 0.0;
    double acc = 0.0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        const int y = (int)(i / cw), x = (int)(i - (long)y * cw);
        const double f = lap_at(img, pgm, width, top, left, ch, cw, y, x, k255);
        if (mean_src) {
            const double d = f - mean;
            acc += d * d;
        } else {
            acc += f;
        }
    }
    acc = wave_sum(acc);
    if (lane_id() == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int q = 0; q < kThreads / 64; q++) t += red[q];
        atomicAdd(out, t);
    }
}

// ---- every box of every image of a call in one launch ----------------------
// (plan and merge order: sharp_tiles.h)
//
// Block blockIdx.x is slice (blockIdx.x - prefix[k]) of box k, found by a
// binary search over the prefix array.  Per tile: the luma of the tile and its
// one-pixel halo goes ONCE into an fp64 LDS tile (each source byte read once;
// pixels outside the crop are zeros and are never loaded, so nothing outside
// the box -- let alone the image -- is read: x + 0 * coef == x, which is what
// skipping the tap gives), then each thread filters four pixels of one column
// (six LDS rows of three words for the four 3x3 windows, taps in (fy, fx)
// order), and two block reductions of fixed shape give the tile's sum and M2
// about its own mean.  No atomics: the slice's partial goes to parts[blockIdx.x].
__global__ __launch_bounds__(kThreads) void k_sharp_tiles(const uint8_t* const* __restrict__ imgs,
                                                          const SharpBox* __restrict__ boxes,
                                                          const int* __restrict__ prefix, int nboxes, int width,
                                                          const double* __restrict__ k255g,
                                                          SharpPart* __restrict__ parts) {
    static_assert(kThreads == kSharpTileW * kSharpTileH / 4, "four pixels per thread");
    __shared__ double k255[256];
    __shared__ double tile[kSharpRows * kSharpPitch];
    __shared__ double red[2 * (kThreads / 64)];
    const int tid = threadIdx.x;
    k255[tid] = k255g[tid];
    const int bid = blockIdx.x;
    int lo = 0, hi = nboxes;                         // prefix[lo] <= bid < prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid] <= bid) lo = mid;
        else hi = mid;
    }
    const SharpBox box = boxes[lo];
    const int slice = bid - prefix[lo];
    const int cw = box.right - box.left, ch = box.bottom - box.top;
    const int tx = sharp_tiles_x(box);
    const long tiles = sharp_tiles(box);
    const int S = sharp_slices(box);
    const uint8_t* __restrict__ img = imgs[box.img];
    const int lx = tid & (kSharpTileW - 1), ly0 = (tid >> 6) * 4;
    SharpPart acc{0.0, 0.0, 0.0};
    for (long t = slice; t < tiles; t += S) {
        const int y0 = (int)(t / tx) * kSharpTileH, x0 = (int)(t % tx) * kSharpTileW;
        __syncthreads();                             // the table; the previous tile's readers
        for (int i = tid; i < kSharpRows * kSharpPitch; i += kThreads) {
            const int r = i / kSharpPitch, q = i - r * kSharpPitch;
            const int cy = y0 + r - 1, cx = x0 + q - 1;
            double v = 0.0;
            if (cy >= 0 && cy < ch && cx >= 0 && cx < cw) {
                const uint8_t* px = img + 3 * ((size_t)(cy + box.top) * width + cx + box.left);
                v = 0.299 * k255[px[0]] + 0.587 * k255[px[1]] + 0.114 * k255[px[2]];
            }
            tile[i] = v;
        }
        __syncthreads();
        // rows ly0 .. ly0 + 3 of column lx: LDS rows ly0 .. ly0 + 5, words lx .. lx + 2
        double w[6][3];
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int q = 0; q < 3; q++) w[r][q] = tile[(ly0 + r) * kSharpPitch + lx + q];
        double f[4];
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double dp = 0.0;
#pragma unroll
            for (int fy = 0; fy < 3; fy++)
#pragma unroll
                for (int fx = 0; fx < 3; fx++) dp += w[j + fy][fx] * ((fy == 1 && fx == 1) ? 8.0 : -1.0);
            const bool in = x0 + lx < cw && y0 + ly0 + j < ch;
            f[j] = dp;
            s += in ? dp : 0.0;
        }
        s = wave_sum(s);
        if (lane_id() == 0) red[tid >> 6] = s;
        __syncthreads();
        const double tsum = ((red[0] + red[1]) + red[2]) + red[3];
        const int nx = min(kSharpTileW, cw - x0), ny = min(kSharpTileH, ch - y0);
        const double tn = (double)(nx * ny);
        const double mean = tsum / tn;
        double m = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool in = x0 + lx < cw && y0 + ly0 + j < ch;
            const double d = f[j] - mean;
            m += in ? d * d : 0.0;
        }
        m = wave_sum(m);
        if (lane_id() == 0) red[4 + (tid >> 6)] = m;
        __syncthreads();
        const SharpPart tp{tn, tsum, ((red[4] + red[5]) + red[6]) + red[7]};
        if (t == slice) acc = tp;
        else sharp_merge(acc, tp);
    }
    if (tid == 0) parts[bid] = acc;
}

// One thread per box: its slice partials in slice order, then sum f and M2
// into the two doubles of the box's slot (assemble's sharp_sums).
__global__ __launch_bounds__(kThreads) void k_sharp_finish(const SharpBox* __restrict__ boxes,
                                                           const int* __restrict__ prefix, int nboxes,
                                                           const SharpPart* __restrict__ parts,
                                                           double* __restrict__ out0, long out_stride) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= nboxes) return;
    const int p0 = prefix[k], p1 = prefix[k + 1];
    SharpPart acc = parts[p0];
    for (int p = p0 + 1; p < p1; p++) sharp_merge(acc, parts[p]);
    const SharpBox box = boxes[k];
    double* out = out0 + (long)box.img * out_stride + 2 * (long)box.slot;
    out[0] = acc.sum;
    out[1] = acc.m2;
}

}  // namespace

// sums[2*k] = sum f, sums[2*k+1] = sum (f - mean)^2 for crop k.  `sums` zeroed by the caller.
hipError_t launch_sharpness(const uint8_t* img, int height, int width, int n, const int* top,
                            const int* bottom, const int* left, const int* right, const double* k255,
                            double* sums, hipStream_t st, KernelProfiler* prof) {
    return launch_sharpness_src(img, nullptr, height, width, n, top, bottom, left, right, k255, sums, st, prof);
}

hipError_t launch_sharpness_src(const uint8_t* img, const double* pgm, int height, int width, int n, const int* top,
                                const int* bottom, const int* left, const int* right, const double* k255,
                                double* sums, hipStream_t st, KernelProfiler* prof) {
    (void)height;
    for (int k = 0; k < n; k++) {
        const int cw = right[k] - left[k], ch = bottom[k] - top[k];
        const long cn = (long)cw * ch;
        const int blocks = (int)std::min<long>(1024, (cn + kThreads - 1) / kThreads);
        int ps = prof_begin_sharp(prof, st);
        phd_launch(k_sharp_pass, dim3(blocks), dim3(kThreads), 0, st, img, pgm, width, top[k], left[k],
                           ch, cw, k255, (const double*)nullptr, 0L, sums + 2 * k);
        prof_end(prof, ps, st);
        ps = prof_begin_sharp(prof, st);
        phd_launch(k_sharp_pass, dim3(blocks), dim3(kThreads), 0, st, img, pgm, width, top[k], left[k],
                           ch, cw, k255, (const double*)(sums + 2 * k), cn, sums + 2 * k + 1);
        prof_end(prof, ps, st);
    }
    return hipGetLastError();
}

hipError_t launch_sharpness_batch(const uint8_t* const* d_imgs, const SharpBox* d_boxes, const int* d_prefix,
                                  int nboxes, int nslices, int width, const double* k255, SharpPart* d_parts,
                                  double* out0, long out_stride, hipStream_t st, KernelProfiler* prof) {
    if (nboxes <= 0) return hipSuccess;
    int ps = prof_begin_sharp(prof, st);
    phd_launch(k_sharp_tiles, dim3(nslices), dim3(kThreads), 0, st, d_imgs, d_boxes, d_prefix, nboxes, width, k255,
               d_parts);
    prof_end(prof, ps, st);
    ps = prof_begin_sharp(prof, st);
    phd_launch(k_sharp_finish, dim3((nboxes + kThreads - 1) / kThreads), dim3(kThreads), 0, st, d_boxes, d_prefix,
               nboxes, (const SharpPart*)d_parts, out0, out_stride);
    prof_end(prof, ps, st);
    return hipGetLastError();
}

}  // namespace phd
