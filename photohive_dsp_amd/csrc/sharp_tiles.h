// sharp_tiles.h -- the batched sharpness stage's plan and merge, host + device.
//
// get_variance_sharpness (src/filtering.c:151-183) of every crop box of every
// image of a call in one launch (sharpness.hip: k_sharp_tiles + k_sharp_finish)
// and, with the same plan and merge order, on the host (phd_sharp_host.cpp:
// phd_debug_sharpness_host).
//
// A box is cut into tiles of kSharpTileW x kSharpTileH pixels anchored at its
// own top-left corner, numbered row-major.  Each tile yields (n, sum f, M2 =
// sum (f - tile mean)^2) of its Laplacian values.  The box has S =
// min(tiles, kSharpSlices) slices; slice s merges tiles s, s + S, s + 2 S, ...
// in increasing order with Chan's pairwise update (sharp_merge), and the box
// merges its S slice partials in slice order.  Every step depends on the box
// and its pixels only, so a box's result is the same whatever else the launch
// holds.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SHARP_HD __host__ __device__ __forceinline__
#else
#define SHARP_HD inline
#endif

namespace phd {

constexpr int kSharpTileW = 64;
constexpr int kSharpTileH = 16;
constexpr int kSharpSlices = 128;                 // most partials (= blocks) of one box
// fp64 luma tile with a one-pixel halo: consecutive lanes on consecutive
// 8-byte words of a row, whatever the pitch
constexpr int kSharpPitch = kSharpTileW + 2;
constexpr int kSharpRows = kSharpTileH + 2;

// One crop box of the call: its image (index into the call's pointer array),
// the box in image coordinates (bottom / right exclusive, crop_pgm's
// convention) and the slot of the image's record its sums go to.
struct SharpBox {
    int img, top, bottom, left, right, slot;
};

// (n, sum f, sum (f - mean)^2) of a set of Laplacian values; 24 bytes
struct SharpPart {
    double n, sum, m2;
};

SHARP_HD int sharp_tiles_x(const SharpBox& b) { return (b.right - b.left + kSharpTileW - 1) / kSharpTileW; }
SHARP_HD int sharp_tiles_y(const SharpBox& b) { return (b.bottom - b.top + kSharpTileH - 1) / kSharpTileH; }
SHARP_HD long sharp_tiles(const SharpBox& b) { return (long)sharp_tiles_x(b) * sharp_tiles_y(b); }
SHARP_HD int sharp_slices(const SharpBox& b) {
    const long t = sharp_tiles(b);
    return t < kSharpSlices ? (int)t : kSharpSlices;
}

// a <- a U b (Chan, Golub, LeVeque): both sets non-empty
SHARP_HD void sharp_merge(SharpPart& a, const SharpPart& b) {
    const double n = a.n + b.n;
    const double delta = b.sum / b.n - a.sum / a.n;
    a.m2 = (a.m2 + b.m2) + (delta * delta) * ((a.n * b.n) / n);
    a.sum = a.sum + b.sum;
    a.n = n;
}

}  // namespace phd
