// palette_labels.hip -- the palette label map: per pixel of the HSV image, the
// palette slot whose average the pixel went into, or PHD_LABEL_NONE.
//
// The reference holds this in its parents' pixel lists after
// group_irregular_pixels (src/color_quantization.c:342-479) -- the pixels
// calculate_avg_hsv (:510-576) averages into color_palette->averages[i] -- and
// frees it with the octree.  Here it is the keep rule of the pixel's arm_octree
// group (GroupRule, phd_internal.h), which the palette tail has on the device:
// label = slot when slot >= 0 and (!partial, or index < cutoff, or (dangle and
// index == last)), else NONE.  One streaming pass, 3 B/px read, 2 B/px written.
//
// Also here: the quantised image of a label map (k_labels_to_rgb).
#include "palette_tile.h"

namespace phd {

namespace {

constexpr int kLabThreads = 1024;            // 16 waves over one kChunk, as K3
constexpr unsigned kNone = kLabelNone;
// waves/SIMD the batched kernel is sized for: two blocks per CU at <= 64 VGPRs
// (the kThr forms spill 3 VGPRs), measured 46.4 / 42.0 us per 4000 x 3000
// image against 52.9 / 45.2 at 4 (one block per CU, 70 VGPRs, no spill):
// profiles/labels/labels_bench_*.log, DESIGN.md section 20
constexpr int kLabMinWaves = 8;

// The label maps of a batch of same-size images (downsample_rate == 1) in one
// launch.  Persistent blocks walk contiguous runs of (destination, chunk)
// items like K3 (k_palette_sums_b) with the same group loads, classify_e and
// exact path for pixels on a hue-bin edge; per image the keep rules are packed
// into LDS ({slot, cut, last}, tl <= 4096 records always fit).  No sums, no LDS
// atomics, no hue arithmetic.  A thread owns 4 consecutive pixels per step and
// writes their labels as one 8-byte store when the map's base is 8-byte
// aligned (4 pixels = 8 bytes, so the base decides for the whole map), else as
// four u16 stores.  The < 4 pixels of a partial final group: one lane.
template <bool kAligned, bool kThr>
__global__ __launch_bounds__(kLabThreads, kLabMinWaves) void k_palette_labels_b(
        const uint8_t* const* __restrict__ imgs, long npix, int nchunks, long nitems, GridParams gp, FastCls fc,
        const ClassTables* __restrict__ tabs, const double* __restrict__ k255g,
        const GroupRule* __restrict__ rules0, long b_stride, const LabelDst* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const double* k255 = reinterpret_cast<const double*>(smem + K1Lds::k255);
    const ClsEnt* ent = reinterpret_cast<const ClsEnt*>(smem + K1Lds::ent);
    const signed char* si8 = tabs->si8;
    const int tl = gp.tl;
    uint4* rec = reinterpret_cast<uint4*>(smem + K1Lds::area);        // [tl + 1]; rec[tl]: keeps nothing
    const int tid = threadIdx.x;
    const long it0 = (long)blockIdx.x * nitems / gridDim.x, it1 = (long)(blockIdx.x + 1) * nitems / gridDim.x;
    if (it0 >= it1) return;                                 // block-uniform
    stage_tables(smem, k255g, tabs);
    if (tid == 0) rec[tl] = make_uint4(0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u);

    constexpr int kSteps = kChunk / (4 * kLabThreads);
    const long full_end = npix & ~3L;
    int k = (int)(it0 / nchunks), c = (int)(it0 - (long)k * nchunks);
    int cur = -1;
    const uint8_t* ip = nullptr;
    uint16_t* lab = nullptr;
    bool wide = false;
    for (long it = it0; it < it1; it++) {
        if (k != cur) {                                      // block-uniform: destination k's image and rules
            __syncthreads();                                 // every wave is done with the last image's rules
            const LabelDst d = dst[k];
            ip = imgs[d.img];
            lab = d.map;
            wide = (reinterpret_cast<uintptr_t>(lab) & 7) == 0;
            const GroupRule* rules =
                    reinterpret_cast<const GroupRule*>(reinterpret_cast<const char*>(rules0) + d.img * b_stride);
            for (int i = tid; i < tl; i += kLabThreads) rec[i] = pack_rule(rules[i]);
            cur = k;
            __syncthreads();
        }
        const long base = (long)c * kChunk;
        unsigned w[kSteps][3];
#pragma unroll
        for (int st = 0; st < kSteps; st++) {
            const long p0 = base + 4L * tid + 4L * kLabThreads * st;
            load_group<kAligned>(ip, p0, p0 < full_end, w[st]);
        }
#pragma unroll
        for (int st = 0; st < kSteps; st++) {
            const long p0 = base + 4L * tid + 4L * kLabThreads * st;
            const bool okg = p0 < full_end;
            // phases over the 4 pixels, so each step has 4 independent LDS reads
            // in flight: class entry -> group -> keep rule
            int kr[4], kg[4], kb[4];
            ClsEnt e[4];
            unsigned l[4], em = 0;                           // labels; edge pixels of the step (bit i)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                kr[i] = px_byte(w[st], 3 * i);
                kg[i] = px_byte(w[st], 3 * i + 1);
                kb[i] = px_byte(w[st], 3 * i + 2);
                e[i] = ent[max(kr[i], max(kg[i], kb[i]))];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int g = classify_e<kThr>(kr[i], kg[i], kb[i], e[i], si8, gp, fc);
                const int edge = g == -2;
                em |= (unsigned)(edge & (int)okg) << i;
                l[i] = label_of(rec[edge ? tl : g], (unsigned)(p0 + i));
            }
            unsigned lo = l[0] | l[1] << 16, hi = l[2] | l[3] << 16;
            // pixels on a hue-bin edge (rare): exact hue and group (rgb2hsv's order)
            while (em) {
                const int i = __ffs(em) - 1;
                em &= em - 1;
                const unsigned pw = px_word(w[st][0], w[st][1], w[st][2], i);
                const int r = pw & 255, g8 = (pw >> 8) & 255, b = (pw >> 16) & 255;
                const int g = edge_group<kThr>(r, g8, b, hue_exact(r, g8, b, k255), ent, si8, gp);
                const unsigned v = label_of(rec[g], (unsigned)(p0 + i));
                const unsigned sh = 16u * (i & 1), m = ~(0xFFFFu << sh);
                if (i < 2) lo = (lo & m) | v << sh;
                else hi = (hi & m) | v << sh;
            }
            if (okg) {
                if (wide) {
                    *reinterpret_cast<uint2*>(lab + p0) = make_uint2(lo, hi);
                } else {
                    lab[p0] = (uint16_t)lo;
                    lab[p0 + 1] = (uint16_t)(lo >> 16);
                    lab[p0 + 2] = (uint16_t)hi;
                    lab[p0 + 3] = (uint16_t)(hi >> 16);
                }
            }
        }
        if (base + kChunk >= npix && tid == 0) {
            // the partial final group of the image: one lane
            for (long p = full_end; p < npix; p++) {
                const int r = ip[3 * p], g8 = ip[3 * p + 1], b = ip[3 * p + 2];
                double sv;
                int g = classify<kThr>(r, g8, b, ent, si8, gp, fc, sv);
                if (g == -2) g = edge_group<kThr>(r, g8, b, hue_exact(r, g8, b, k255), ent, si8, gp);
                lab[p] = (uint16_t)label_of(rec[g], (unsigned)p);
            }
        }
        if (++c == nchunks) {
            c = 0;
            k++;
        }
    }
}

// The label map of one image, any downsample rate: pixels gathered as k_hsv_ds
// / k_palette_sums gather them (src_pixel: downsample_rgb's row quirk), the
// group from rgb2hsv's doubles, the rule from global memory.  For downsampled
// images and the grids whose second pass runs per image.
__global__ __launch_bounds__(kThreads) void k_palette_labels(const uint8_t* __restrict__ img, long npix, int width,
                                                             int ds, int nw, GridParams gp,
                                                             const GroupRule* __restrict__ rules,
                                                             const double* __restrict__ k255g,
                                                             uint16_t* __restrict__ lab) {
    __shared__ double k255[256];
    const int tid = threadIdx.x;
    k255[tid] = k255g[tid];
    __syncthreads();
    const long base = (long)blockIdx.x * kChunk;
    const long end = min(base + (long)kChunk, npix);
    for (long j = base + tid; j < end; j += kThreads) {
        const long p = src_pixel(j, width, ds, nw);
        double h, s, v;
        rgb2hsv(k255[img[3 * p]], k255[img[3 * p + 1]], k255[img[3 * p + 2]], h, s, v);
        lab[j] = (uint16_t)label_of(pack_rule(rules[group_of(gp, h, s, v)]), (unsigned)j);
    }
}

// The quantised image of n label maps in one launch (grid.y = map): pixel k of
// a map gets its label's LUT colour (r | g << 8 | b << 16 per slot), or `none`
// for PHD_LABEL_NONE and for any label >= n_slots.  A thread owns 4 pixels:
// one 8-byte label load and three word stores where the bases allow, else
// element by element.
__global__ __launch_bounds__(kThreads) void k_labels_to_rgb(const LabelRgbRec* __restrict__ recs) {
    const LabelRgbRec r = recs[blockIdx.y];
    const bool wide_in = (reinterpret_cast<uintptr_t>(r.map) & 7) == 0;
    const bool wide_out = (reinterpret_cast<uintptr_t>(r.dst) & 3) == 0;
    const long ngroups = (r.npix + 3) / 4;
    for (long gi = (long)blockIdx.x * kThreads + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * kThreads) {
        const long p0 = 4 * gi;
        const bool full = p0 + 3 < r.npix;
        unsigned l[4] = {kNone, kNone, kNone, kNone}, px[4];
        if (full && wide_in) {
            const uint2 q = *reinterpret_cast<const uint2*>(r.map + p0);
            l[0] = q.x & 0xFFFFu;
            l[1] = q.x >> 16;
            l[2] = q.y & 0xFFFFu;
            l[3] = q.y >> 16;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (p0 + i < r.npix) l[i] = r.map[p0 + i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) px[i] = l[i] < (unsigned)r.n_slots ? r.lut[l[i]] : r.none;
        uint8_t* o = r.dst + 3 * p0;
        if (full && wide_out) {
            unsigned* ow = reinterpret_cast<unsigned*>(o);
            ow[0] = px[0] | px[1] << 24;
            ow[1] = px[1] >> 8 | px[2] << 16;
            ow[2] = px[2] >> 16 | px[3] << 8;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (p0 + i < r.npix) {
                    o[3 * i] = (uint8_t)px[i];
                    o[3 * i + 1] = (uint8_t)(px[i] >> 8);
                    o[3 * i + 2] = (uint8_t)(px[i] >> 16);
                }
        }
    }
}

}  // namespace

static size_t palette_labels_b_lds(int tl) { return (size_t)K1Lds::area + 16 * ((size_t)tl + 1); }

hipError_t launch_palette_labels_batch(const uint8_t* const* d_imgs, bool aligned, int height, int width,
                                       const GridParams& gp, const FastCls& fc, const ClassTables* tabs,
                                       const double* k255, const GroupRule* rules0, long b_stride,
                                       const LabelDst* d_dst, int n_dst, hipStream_t st) {
    if (n_dst <= 0) return hipSuccess;
    const long npix = (long)height * width;
    const int nchunks = (int)((npix + kChunk - 1) / kChunk);
    const long nitems = (long)n_dst * nchunks;
    const size_t lds = palette_labels_b_lds(gp.tl);
    const void* kfn = fc.use_thr ? (aligned ? (const void*)k_palette_labels_b<true, true>
                                            : (const void*)k_palette_labels_b<false, true>)
                                 : (aligned ? (const void*)k_palette_labels_b<true, false>
                                            : (const void*)k_palette_labels_b<false, false>);
    // persistent blocks: as many as are resident at once
    (void)hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, kLabThreads, lds) != hipSuccess || per_cu < 1)
        per_cu = 1;
    const int grid = (int)std::min<long>(nitems, (long)per_cu * num_cus());
#define PHD_LAB_LAUNCH(A, T)                                                                                \
    phd_launch((k_palette_labels_b<A, T>), dim3(grid), dim3(kLabThreads), lds, st, d_imgs, npix, nchunks,  \
               nitems, gp, fc, tabs, k255, rules0, b_stride, d_dst)
    if (fc.use_thr) {
        if (aligned) PHD_LAB_LAUNCH(true, true);
        else PHD_LAB_LAUNCH(false, true);
    } else {
        if (aligned) PHD_LAB_LAUNCH(true, false);
        else PHD_LAB_LAUNCH(false, false);
    }
#undef PHD_LAB_LAUNCH
    return hipGetLastError();
}

hipError_t launch_palette_labels(const uint8_t* img, int height, int width, int ds, const GridParams& gp,
                                 const GroupRule* rules, const double* k255, uint16_t* map, hipStream_t st) {
    const int hh = ds > 1 ? height / ds : height, nw = ds > 1 ? width / ds : width;
    const long n = (long)(short)hh * (short)nw;   // rgb2hsv's short dimensions, image_processing.c:378-383
    const int nchunks = (int)((n + kChunk - 1) / kChunk);
    if (nchunks <= 0) return hipSuccess;
    phd_launch(k_palette_labels, dim3(nchunks), dim3(kThreads), 0, st, img, n, width, ds, nw, gp, rules, k255,
               map);
    return hipGetLastError();
}

hipError_t launch_labels_to_rgb(const LabelRgbRec* d_recs, int n, long max_npix, hipStream_t st) {
    if (n <= 0 || max_npix <= 0) return hipSuccess;
    const long groups = (max_npix + 3) / 4;
    const int bx = (int)std::min<long>(2048, (groups + kThreads - 1) / kThreads);
    phd_launch(k_labels_to_rgb, dim3(bx, n), dim3(kThreads), 0, st, d_recs);
    return hipGetLastError();
}

}  // namespace phd
