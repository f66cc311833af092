// planar.hip -- the legacy entry point's fp64 planar input.
//
// get_full_report_data (src/interface.c:20-94) takes three planes of doubles.
// The Python binding fills them with k/255.0 (utils.py:30-46); then the
// library converts them back to RGB8 on the device (k_planar_to_u8) and runs
// the RGB8 pipeline, whose arithmetic reproduces the reference's on those
// doubles exactly.  A C caller may pass any doubles (a 16-bit image / 65535,
// a tone-mapped float image): this file runs the reference's own fp64
// arithmetic on them --
//   * get_rgb_statistics (src/image_processing.c:543-553, get_average /
//     get_variance src/filtering.c:125-148): fp64 sums per block, reduced in a
//     fixed order (run-to-run identical), the variance's second pass on the
//     means;
//   * rgb2pgm (src/image_processing.c:505-512) into an fp64 luma plane for the
//     generic FFT path (fft_global.hip) and the sharpness crops;
//   * rgb2hsv + arm_octree (src/image_processing.c:372-417,
//     src/color_quantization.c:108-161) per pixel in fp64 (phd_device.h),
//     the group histogram and its per-chunk counts, sum(s) for S-bar;
//   * the tie-overflow cut-off search and calculate_avg_hsv's per-slot sums
//     (src/color_quantization.c:414-450, 510-576) after the host decisions;
//   * the palette label map (the parents' pixel lists after
//     group_irregular_pixels, src/color_quantization.c:342-479) from the same
//     groups and keep rules (k_planar_labels);
//   * the box statistics: get_rgb_statistics and get_hsv_average
//     (src/image_processing.c:543-553, 533-540) on crop_image's boxes
//     (src/image_processing.c:244-266), per band of rows (k_planar_box_stats).
#include "phd_device.h"

namespace phd {

namespace {

constexpr int kPT = 256;

// flags (device int): bit 0 some value is not k/255 (not an 8-bit image);
// bit 1 a value is not finite; bit 2 a pixel's group index falls outside the
// octree (values above 1: the reference indexes out of bounds).  Any other
// finite values are the reference's to report on: negative channels, luma
// outside [0, 1] (the polar bins' fixed-point scale follows the observed luma
// range, bin_scale)
constexpr int kFlagNotU8 = 1, kFlagNonFinite = 2, kFlagGroupRange = 4;

__device__ __forceinline__ void flag_wave(int* flags, bool bad, int bit) {
    if (__any(bad) && lane_id() == 0) atomicOr(flags, bit);
}

// fixed-order block sum of one double per thread (wave shuffles, then waves in order)
__device__ __forceinline__ double block_sum(double x, double* red) {
    x = wave_sum(x);
    __syncthreads();
    if (lane_id() == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    double t = 0.0;
    for (int q = 0; q < kPT / 64; q++) t += red[q];
    return t;
}

// The 8-bit test: every value is exactly (double)k / 255.0 for an integer k
// in [0, 255] (utils.py:30-46); the RGB8 image is written as it goes.
__global__ __launch_bounds__(kPT) void k_planar_to_u8(PlanarSrc P, long n, uint8_t* __restrict__ rgb,
                                                      int* __restrict__ flags) {
    for (long i = (long)blockIdx.x * kPT + threadIdx.x; i - threadIdx.x < n; i += (long)gridDim.x * kPT) {
        bool bad = false;
        if (i < n) {
            const double x[3] = {P.r[i], P.g[i], P.b[i]};
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const bool in = x[c] >= 0.0 && x[c] <= 1.0;      // false for NaN
                const int k = in ? (int)rint(x[c] * 255.0) : 0;
                bad |= !in || (double)k / 255.0 != x[c];
                rgb[3 * i + c] = (uint8_t)k;
            }
        }
        flag_wave(flags, bad, kFlagNotU8);
    }
}

// Channel sums (one partial per block and channel: part[3 * block + c]), the
// luma plane pgm = 0.299 r + 0.587 g + 0.114 b and its range per block
// (lrng[2 * block] = -min, lrng[2 * block + 1] = max; -inf for no pixel).
__global__ __launch_bounds__(kPT) void k_planar_moments(PlanarSrc P, long n, double* __restrict__ pgm,
                                                        double* __restrict__ part, double* __restrict__ lrng,
                                                        int* __restrict__ flags) {
    __shared__ double red[kPT / 64];
    double s[3] = {0.0, 0.0, 0.0};
    double nlo = -__builtin_inf(), hi = -__builtin_inf();
    for (long i0 = (long)blockIdx.x * kPT; i0 < n; i0 += (long)gridDim.x * kPT) {
        const long i = i0 + threadIdx.x;
        bool bad = false;
        if (i < n) {
            const double r = P.r[i], g = P.g[i], b = P.b[i];
            bad = !isfinite(r) || !isfinite(g) || !isfinite(b);
            s[0] += r;
            s[1] += g;
            s[2] += b;
            const double y = 0.299 * r + 0.587 * g + 0.114 * b;
            pgm[i] = y;
            nlo = fmax(nlo, -y);
            hi = fmax(hi, y);
        }
        flag_wave(flags, bad, kFlagNonFinite);
    }
    for (int c = 0; c < 3; c++) {
        const double t = block_sum(s[c], red);
        if (threadIdx.x == 0) part[3 * blockIdx.x + c] = t;
    }
    double m[2] = {nlo, hi};
    for (int k = 0; k < 2; k++) {
        double x = wave_max(m[k]);
        __syncthreads();
        if (lane_id() == 0) red[threadIdx.x >> 6] = x;
        __syncthreads();
        for (int q = 0; q < kPT / 64; q++) x = fmax(x, red[q]);
        if (threadIdx.x == 0) lrng[2 * blockIdx.x + k] = x;
    }
}

// get_average's mean per channel from the block partials, summed in a fixed
// order (the same in every block): B = sum / N.
__device__ __forceinline__ void planar_means(const double* __restrict__ part, int nb, long n, double* mean) {
    if (threadIdx.x < 3) {
        double a = 0.0;
        for (int k = 0; k < nb; k++) a += part[3 * k + threadIdx.x];
        mean[threadIdx.x] = a / (double)n;
    }
    __syncthreads();
}

// get_variance's second pass: sum (x - B)^2 per channel (part2), and the DC
// bias avg = (Br + Bg + Bb) / 3.0 (src/interface.c:78) for the FFT.
__global__ __launch_bounds__(kPT) void k_planar_var(PlanarSrc P, long n, const double* __restrict__ part1, int nb,
                                                    double* __restrict__ part2, double* __restrict__ avg_out) {
    __shared__ double red[kPT / 64];
    __shared__ double mean[3];
    planar_means(part1, nb, n, mean);
    const double br = mean[0], bg = mean[1], bb = mean[2];
    if (blockIdx.x == 0 && threadIdx.x == 0) *avg_out = (br + bg + bb) / 3.0;
    double s[3] = {0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * kPT + threadIdx.x; i < n; i += (long)gridDim.x * kPT) {
        const double dr = P.r[i] - br, dg = P.g[i] - bg, db = P.b[i] - bb;
        s[0] += dr * dr;
        s[1] += dg * dg;
        s[2] += db * db;
    }
    for (int c = 0; c < 3; c++) {
        const double t = block_sum(s[c], red);
        if (threadIdx.x == 0) part2[3 * blockIdx.x + c] = t;
    }
}

// rgb2hsv + arm_octree's group of one pixel's doubles: the one place the fp64
// kernels get a group from (K1, the cut-off search, the sums, the label map).
__device__ __forceinline__ int planar_group(double r, double g, double b, const GridParams& gp, double& h, double& s,
                                            double& v) {
    rgb2hsv(r, g, b, h, s, v);
    return group_of(gp, h, s, v);
}

__device__ __forceinline__ int planar_group(const PlanarSrc& P, long p, const GridParams& gp, double& h, double& s,
                                            double& v) {
    return planar_group(P.r[p], P.g[p], P.b[p], gp, h, s, v);
}

// K1 on doubles: one block per chunk of kChunk hsv pixels (downsample_rgb's
// mapping for ds > 1): group histogram (hist, and the chunk's counts for the
// cut-off search) and the chunk's sum of s (get_hsv_average).
__global__ __launch_bounds__(kPT) void k_planar_k1(PlanarSrc P, long npix, int width, int ds, int nw, GridParams gp,
                                                   unsigned* __restrict__ hist, unsigned short* __restrict__ chunk_hist,
                                                   double* __restrict__ s_part, int* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned* lh = reinterpret_cast<unsigned*>(smem);
    __shared__ double red[kPT / 64];
    for (int i = threadIdx.x; i < gp.tl; i += kPT) lh[i] = 0;
    __syncthreads();
    const long base = (long)blockIdx.x * kChunk;
    const long end = min(base + (long)kChunk, npix);
    double ssum = 0.0;
    for (long j0 = base; j0 < end; j0 += kPT) {
        const long j = j0 + threadIdx.x;
        bool bad = false;
        if (j < end) {
            double h, s, v;
            const int g = planar_group(P, src_pixel(j, width, ds, nw), gp, h, s, v);
            ssum += s;
            bad = g < 0 || g >= gp.tl;
            if (!bad) atomicAdd(&lh[g], 1u);
        }
        flag_wave(flags, bad, kFlagGroupRange);
    }
    const double t = block_sum(ssum, red);
    if (threadIdx.x == 0) s_part[blockIdx.x] = t;
    __syncthreads();
    for (int i = threadIdx.x; i < gp.tl; i += kPT) {
        const unsigned c = lh[i];
        chunk_hist[(long)blockIdx.x * gp.tl + i] = (unsigned short)c;
        if (c) atomicAdd(&hist[i], c);
    }
}

__device__ int scan_excl(int x, int& excl, int* scratch) {
    const int lane = lane_id(), w = threadIdx.x >> 6;
    int incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
    }
    if (lane == 63) scratch[w] = incl;
    __syncthreads();
    int wpre = 0, tot = 0;
    for (int q = 0; q < kPT / 64; q++) {
        if (q < w) wpre += scratch[q];
        tot += scratch[q];
    }
    __syncthreads();
    excl = wpre + incl - x;
    return tot;
}

// The cut-off search of group_irregular_pixels' tie path on doubles: one
// block per searched group, the raster index of its keep-th pixel (the chunk
// from the per-chunk counts, then a block scan inside it) and of its last.
__global__ __launch_bounds__(kPT) void k_planar_cutoffs(PlanarSrc P, long npix, int width, int ds, int nw,
                                                        GridParams gp, const unsigned short* __restrict__ chunk_hist,
                                                        int nchunks, GroupRule* rules,
                                                        const int* __restrict__ search) {
    __shared__ int scratch[kPT / 64];
    __shared__ int s_chunk, s_rank, s_last_chunk, s_found;
    __shared__ unsigned s_idx;
    const int tid = threadIdx.x;
    const int g = search[blockIdx.x];
    const int keep = rules[g].keep;
    const int want_cut = rules[g].partial && keep > 0;
    const int want_last = rules[g].partial && rules[g].dangle;
    if (tid == 0) {
        s_chunk = -1;
        s_last_chunk = -1;
    }
    __syncthreads();
    int carry = 0;
    for (int c0 = 0; c0 < nchunks; c0 += kPT) {
        const int c = c0 + tid;
        const int cnt = c < nchunks ? (int)chunk_hist[(long)c * gp.tl + g] : 0;
        int excl;
        const int tot = scan_excl(cnt, excl, scratch);
        if (want_cut && cnt > 0 && carry + excl < keep && keep <= carry + excl + cnt) {
            s_chunk = c;
            s_rank = keep - (carry + excl);
        }
        if (cnt > 0) atomicMax(&s_last_chunk, c);
        carry += tot;
        __syncthreads();
    }
    for (int pass = 0; pass < 2; pass++) {
        const int c = pass == 0 ? (want_cut ? s_chunk : -1) : (want_last ? s_last_chunk : -1);
        if (c < 0) continue;
        const long base = (long)c * kChunk, end = min(base + (long)kChunk, npix);
        int rank = s_rank;
        if (tid == 0) {
            s_found = 0;
            s_idx = 0;
        }
        __syncthreads();
        for (long j0 = base; j0 < end; j0 += kPT) {
            const long j = j0 + tid;
            int hit = 0;
            if (j < end) {
                double h, s, v;
                hit = planar_group(P, src_pixel(j, width, ds, nw), gp, h, s, v) == g;
            }
            if (pass == 0) {
                int excl;
                const int tot = scan_excl(hit, excl, scratch);
                if (hit && excl + 1 == rank) {
                    s_idx = (unsigned)j;
                    s_found = 1;
                }
                rank -= tot;
                __syncthreads();
                if (s_found) break;
            } else if (hit) {
                atomicMax(&s_idx, (unsigned)j);
            }
        }
        __syncthreads();
        if (tid == 0) {
            if (pass == 0) rules[g].cutoff = s_idx + 1;
            else rules[g].last = s_idx;
        }
        __syncthreads();
    }
}

// calculate_avg_hsv's per-slot sums over the kept pixels (K3 on doubles):
// out[4 slot + {0,1,2,3}] = sum wrap(h + off), sum s, sum v, n.
__global__ __launch_bounds__(kPT) void k_planar_sums(PlanarSrc P, long npix, int width, int ds, int nw, GridParams gp,
                                                     const GroupRule* __restrict__ rules_g,
                                                     const double* __restrict__ off_g, int nslots,
                                                     double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* acc = reinterpret_cast<double*>(smem);                       // nslots * 4
    double* off = acc + 4 * nslots;                                      // nslots
    GroupRule* rules = reinterpret_cast<GroupRule*>(off + nslots);       // tl
    const int tid = threadIdx.x;
    for (int i = tid; i < 4 * nslots; i += kPT) acc[i] = 0.0;
    for (int i = tid; i < nslots; i += kPT) off[i] = off_g[i];
    for (int i = tid; i < gp.tl; i += kPT) rules[i] = rules_g[i];
    __syncthreads();
    const long base = (long)blockIdx.x * kChunk;
    const long end = min(base + (long)kChunk, npix);
    for (long j0 = base; j0 < end; j0 += kPT) {
        const long j = j0 + tid;
        int slot = -1;
        double h = 0.0, s = 0.0, v = 0.0, tp = 0.0;
        if (j < end) {
            const int g = planar_group(P, src_pixel(j, width, ds, nw), gp, h, s, v);
            if (g >= 0 && g < gp.tl) {
                const GroupRule& R = rules[g];
                const unsigned idx = (unsigned)j;
                if (R.slot >= 0 && (!R.partial || idx < R.cutoff || (R.dangle && idx == R.last))) {
                    slot = R.slot;
                    tp = h + off[slot];                    // src/color_quantization.c:538-546
                    if (tp > 360) tp -= 360;
                    else if (tp < 0) tp += 360;
                }
            }
        }
        const int s0 = __builtin_amdgcn_readfirstlane(slot);
        if (__all(slot == s0)) {
            if (s0 >= 0) {
                const double th = wave_sum(tp), ts = wave_sum(s), tv = wave_sum(v);
                const double cnt = wave_sum(1.0);
                if (lane_id() == 0) {
                    atomicAdd(&acc[4 * s0 + 0], th);
                    atomicAdd(&acc[4 * s0 + 1], ts);
                    atomicAdd(&acc[4 * s0 + 2], tv);
                    atomicAdd(&acc[4 * s0 + 3], cnt);
                }
            }
        } else if (slot >= 0) {
            atomicAdd(&acc[4 * slot + 0], tp);
            atomicAdd(&acc[4 * slot + 1], s);
            atomicAdd(&acc[4 * slot + 2], v);
            atomicAdd(&acc[4 * slot + 3], 1.0);
        }
    }
    __syncthreads();
    for (int i = tid; i < 4 * nslots; i += kPT) {
        const double a = acc[i];
        if (a != 0.0) atomicAdd(&out[i], a);
    }
}

// ---- the label map on doubles ---------------------------------------------------
// Threads and minimum waves per SIMD of k_planar_labels, chosen by measurement
// on one 3000 x 4000 image (profiles/labels_inputs/kernel_*.log, DESIGN.md
// section 21): 256 / 8 53.7 us, 256 / 4 54.4, 512 / 8 54.7, 1024 / 4 56.8,
// 1024 / 8 57.3; at most 51 VGPRs and no scratch.  Overridable for A/B
// builds: make variant V=... VFLAGS="-DPHD_PLAB_T=... -DPHD_PLAB_W=..."
#ifndef PHD_PLAB_T
#define PHD_PLAB_T 256
#endif
#ifndef PHD_PLAB_W
#define PHD_PLAB_W 8
#endif
constexpr int kPlabThreads = PHD_PLAB_T, kPlabMinWaves = PHD_PLAB_W;

// Four consecutive doubles of a plane from element j (j % 4 == 0): two 16-byte
// loads when the plane's base is 16-byte aligned (the planes are 3 n contiguous
// doubles, so for odd n every other plane is not), else element by element.
__device__ __forceinline__ void load4(const double* __restrict__ p, long j, bool a16, double* x) {
    if (a16) {
        const double2 lo = *reinterpret_cast<const double2*>(p + j), hi = *reinterpret_cast<const double2*>(p + j + 2);
        x[0] = lo.x;
        x[1] = lo.y;
        x[2] = hi.x;
        x[3] = hi.y;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) x[i] = p[j + i];
    }
}

__device__ __forceinline__ unsigned planar_label(double r, double g, double b, const GridParams& gp,
                                                 const uint4* rec, unsigned idx) {
    double h, s, v;
    const int grp = planar_group(r, g, b, gp, h, s, v);
    // (a group outside the octree cannot pass the flags check: rec[tl] keeps nothing)
    return label_of(rec[(unsigned)grp < (unsigned)gp.tl ? grp : gp.tl], idx);
}

// The palette label map of the fp64 pipeline (palette_labels.hip's rule on the
// group planar_group gives, as K1 and k_planar_sums take it): one streaming
// pass in the manner of k_palette_labels_b.  The keep rules sit packed in LDS
// ({slot, cut, last}, 16 B: one ds_read_b128 per pixel); persistent blocks
// stride over groups of 4 consecutive hsv pixels, one group per thread and
// step; a group's labels leave as one 8-byte store when the map's base is
// 8-byte aligned (4 pixels = 8 bytes: the base decides for the whole map),
// else as four u16 stores.  The < 4 pixels of a partial final group: one lane.
// kDs: downsample_rate > 1, the pixels gathered through src_pixel.
template <bool kDs>
__global__ __launch_bounds__(kPlabThreads, kPlabMinWaves) void k_planar_labels(
        PlanarSrc P, long npix, int width, int ds, int nw, GridParams gp, const GroupRule* __restrict__ rules,
        uint16_t* __restrict__ lab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4* rec = reinterpret_cast<uint4*>(smem);                          // [tl + 1]
    const int tid = threadIdx.x, tl = gp.tl;
    for (int i = tid; i < tl; i += kPlabThreads) rec[i] = pack_rule(rules[i]);
    if (tid == 0) rec[tl] = make_uint4(0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u);
    __syncthreads();
    const bool wide = (reinterpret_cast<uintptr_t>(lab) & 7) == 0;
    const bool ar = (reinterpret_cast<uintptr_t>(P.r) & 15) == 0, ag = (reinterpret_cast<uintptr_t>(P.g) & 15) == 0,
               ab = (reinterpret_cast<uintptr_t>(P.b) & 15) == 0;
    const long ngroups = npix >> 2;
    for (long gi = (long)blockIdx.x * kPlabThreads + tid; gi < ngroups; gi += (long)gridDim.x * kPlabThreads) {
        const long j0 = 4 * gi;
        double r[4], g[4], b[4];
        if constexpr (kDs) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const long p = src_pixel(j0 + i, width, ds, nw);
                r[i] = P.r[p];
                g[i] = P.g[p];
                b[i] = P.b[p];
            }
        } else {
            load4(P.r, j0, ar, r);
            load4(P.g, j0, ag, g);
            load4(P.b, j0, ab, b);
        }
        unsigned l[4];
#pragma unroll
        for (int i = 0; i < 4; i++) l[i] = planar_label(r[i], g[i], b[i], gp, rec, (unsigned)(j0 + i));
        if (wide) {
            *reinterpret_cast<uint2*>(lab + j0) = make_uint2(l[0] | l[1] << 16, l[2] | l[3] << 16);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) lab[j0 + i] = (uint16_t)l[i];
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        for (long j = 4 * ngroups; j < npix; j++) {
            const long p = src_pixel(j, width, ds, nw);
            lab[j] = (uint16_t)planar_label(P.r[p], P.g[p], P.b[p], gp, rec, (unsigned)j);
        }
    }
}

// The fp64 box statistics (get_rgb_statistics, src/image_processing.c:543-553, and
// get_hsv_average over rgb2hsv's s, :533-540, on crop_image's box, :244-266):
// one block per item (a band of whole rows of a box).  kVar == false: the item's
// fixed-order block sums of r, g, b and s into part[4 * item + c].  kVar ==
// true: the box's means B = sum / N from its items' sums in item order
// (sums[4 * k + c], k = first .. first + count - 1), then get_variance's second
// pass, sum (x - B)^2 per channel into part[3 * item + c].  Plain and untuned:
// a division per pixel for its row, one pixel per thread and step.
template <bool kVar>
__global__ __launch_bounds__(kPT) void k_planar_box_stats(PlanarSrc P, int width,
                                                          const PlanarBoxItem* __restrict__ items,
                                                          const double* __restrict__ sums, double* __restrict__ part) {
    __shared__ double red[kPT / 64];
    __shared__ double mean[3];
    const PlanarBoxItem it = items[blockIdx.x];
    if (kVar) {
        if (threadIdx.x < 3) {
            double a = 0.0;
            for (int k = it.first; k < it.first + it.count; k++) a += sums[4 * k + threadIdx.x];
            mean[threadIdx.x] = a / (double)it.npix;
        }
        __syncthreads();
    }
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const int n = it.rows * it.cols;                        // <= kBoxBandElems, or one row's
    for (int e = threadIdx.x; e < n; e += kPT) {
        const int row = e / it.cols, x = e - row * it.cols;
        const long p = (long)(it.row0 + row) * width + it.left + x;
        const double r = P.r[p], g = P.g[p], b = P.b[p];
        if (kVar) {
            const double dr = r - mean[0], dg = g - mean[1], db = b - mean[2];
            s[0] += dr * dr;
            s[1] += dg * dg;
            s[2] += db * db;
        } else {
            double h, sat, v;
            rgb2hsv(r, g, b, h, sat, v);
            s[0] += r;
            s[1] += g;
            s[2] += b;
            s[3] += sat;
        }
    }
    constexpr int nc = kVar ? 3 : 4;
    for (int c = 0; c < nc; c++) {
        const double t = block_sum(s[c], red);
        if (threadIdx.x == 0) part[nc * blockIdx.x + c] = t;
    }
}

unsigned grid_for(long n) { return (unsigned)std::max<long>(1, std::min<long>(kPlanarBlocks, (n + kPT - 1) / kPT)); }

}  // namespace

hipError_t launch_planar_to_u8(const PlanarSrc& P, long n, uint8_t* rgb, int* flags, hipStream_t st) {
    phd_launch(k_planar_to_u8, dim3(grid_for(n)), dim3(kPT), 0, st, P, n, rgb, flags);
    return hipGetLastError();
}

int planar_blocks(long n) { return (int)grid_for(n); }

hipError_t launch_planar_stats(const PlanarSrc& P, long n, double* pgm, double* part1, double* part2, double* avg,
                               double* lrng, int* flags, hipStream_t st) {
    const unsigned nb = grid_for(n);
    phd_launch(k_planar_moments, dim3(nb), dim3(kPT), 0, st, P, n, pgm, part1, lrng, flags);
    phd_launch(k_planar_var, dim3(nb), dim3(kPT), 0, st, P, n, (const double*)part1, (int)nb, part2, avg);
    return hipGetLastError();
}

hipError_t launch_planar_k1(const PlanarSrc& P, int height, int width, int ds, const GridParams& gp, unsigned* hist,
                            unsigned short* chunk_hist, double* s_part, int* flags, hipStream_t st) {
    int nw = width;
    long npix = (long)height * width;
    if (ds > 1) {
        nw = width / ds;
        npix = (long)(short)(height / ds) * (short)nw;
    }
    const unsigned nchunks = (unsigned)((npix + kChunk - 1) / kChunk);
    phd_launch(k_planar_k1, dim3(nchunks), dim3(kPT), sizeof(unsigned) * gp.tl, st, P, npix, width, ds, nw, gp, hist,
               chunk_hist, s_part, flags);
    return hipGetLastError();
}

hipError_t launch_planar_tail(const PlanarSrc& P, int height, int width, int ds, const GridParams& gp,
                              const unsigned short* chunk_hist, int nchunks, GroupRule* rules, const int* search,
                              int n_search, const double* off, int nslots, double* out, hipStream_t st,
                              KernelProfiler* prof) {
    int nw = width;
    long npix = (long)height * width;
    if (ds > 1) {
        nw = width / ds;
        npix = (long)(short)(height / ds) * (short)nw;
    }
    if (n_search > 0)
        phd_launch(k_planar_cutoffs, dim3((unsigned)n_search), dim3(kPT), 0, st, P, npix, width, ds, nw, gp,
                   chunk_hist, nchunks, rules, search);
    if (nslots > 0) {
        const size_t lds = sizeof(double) * 5 * nslots + sizeof(GroupRule) * gp.tl;
        static bool once = ((void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_planar_sums),
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024),
                            true);
        (void)once;
        const int ps = prof_begin_kernel(prof, kProfPalSums, st);
        phd_launch(k_planar_sums, dim3((unsigned)((npix + kChunk - 1) / kChunk)), dim3(kPT), lds, st, P, npix, width,
                   ds, nw, gp, (const GroupRule*)rules, off, nslots, out);
        prof_end(prof, ps, st);
    }
    return hipGetLastError();
}

hipError_t launch_planar_labels(const PlanarSrc& P, int height, int width, int ds, const GridParams& gp,
                                const GroupRule* rules, uint16_t* map, hipStream_t st) {
    int nw = width;
    long npix = (long)height * width;
    if (ds > 1) {
        nw = width / ds;
        npix = (long)(short)(height / ds) * (short)nw;
    }
    if (npix <= 0) return hipSuccess;
    const size_t lds = sizeof(uint4) * ((size_t)gp.tl + 1);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const void* kfn = ds > 1 ? (const void*)k_planar_labels<true> : (const void*)k_planar_labels<false>;
    // persistent blocks: as many as are resident at once
    (void)hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, kPlabThreads, lds) != hipSuccess || per_cu < 1)
        per_cu = 1;
    const long steps = ((npix >> 2) + kPlabThreads - 1) / kPlabThreads;
    const unsigned grid = (unsigned)std::max<long>(1, std::min<long>(steps, (long)per_cu * num_cus()));
    if (ds > 1)
        phd_launch(k_planar_labels<true>, dim3(grid), dim3(kPlabThreads), lds, st, P, npix, width, ds, nw, gp, rules,
                   map);
    else
        phd_launch(k_planar_labels<false>, dim3(grid), dim3(kPlabThreads), lds, st, P, npix, width, ds, nw, gp, rules,
                   map);
    return hipGetLastError();
}

hipError_t launch_planar_box_stats(const PlanarSrc& P, int width, const PlanarBoxItem* d_items, int nitems,
                                   double* part1, double* part2, hipStream_t st) {
    if (nitems <= 0) return hipSuccess;
    phd_launch(k_planar_box_stats<false>, dim3((unsigned)nitems), dim3(kPT), 0, st, P, width, d_items,
               (const double*)nullptr, part1);
    phd_launch(k_planar_box_stats<true>, dim3((unsigned)nitems), dim3(kPT), 0, st, P, width, d_items,
               (const double*)part1, part2);
    return hipGetLastError();
}

}  // namespace phd
