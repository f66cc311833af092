// phd_views.cpp -- the image-view input stage on the host: the descriptor's
// validation, the pack launch's records, and the kernel's host-only twin
// phd_debug_pack_view_host (no HIP: this file and pack_view.h compile alone,
// tests/native/pack_view_asan.cpp).  The same for typed views: typed_view_why,
// the decode launches' records and the twin decode_view_host over
// decode_view.h (tests/native/decode_view_asan.cpp).
#include <cmath>
#include <string>

#include "views_plan.h"

namespace phd {

bool view_why(const phd_image_view& v, std::string* why) {
    if (!v.data) {
        *why = "view data is NULL";
        return false;
    }
    if (v.height <= 0 || v.width <= 0) {
        *why = "view height and width must be positive (height " + std::to_string(v.height) + ", width " +
               std::to_string(v.width) + ")";
        return false;
    }
    if (v.pixel_stride == 0 && v.width > 1) {
        *why = "view pixel_stride is 0 with width " + std::to_string(v.width);
        return false;
    }
    if (v.row_stride == 0 && v.height > 1) {
        *why = "view row_stride is 0 with height " + std::to_string(v.height);
        return false;
    }
    return true;
}

PackRec pack_record(const phd_image_view& v, uint8_t* dst) {
    PackRec r{};
    r.src = v.data;
    r.dst = dst;
    r.row_stride = v.row_stride;
    r.pixel_stride = v.pixel_stride;
    r.channel_stride = v.channel_stride;
    r.height = v.height;
    r.width = v.width;
    r.kind = pack_kind(v.width, v.row_stride, v.pixel_stride, v.channel_stride);
    // (a packed view copied on request: its rows are a pitched copy)
    if (r.kind == kPackPacked) r.kind = kPackPitched;
    r.band_rows = pack_band_rows(v.height, v.width);
    return r;
}

bool typed_view_why(const phd_typed_view& v, std::string* why) {
    if (v.elem < 0 || v.elem >= kNumElems) {
        *why = "view elem " + std::to_string(v.elem) + " is not a PHD_ELEM_* type";
        return false;
    }
    if (v.flags & ~PHD_VIEW_SNAP_U8) {
        *why = "view flags " + std::to_string(v.flags) + " has unknown bits";
        return false;
    }
    if (!(v.max_value == 0.0 || (v.max_value > 0.0 && std::isfinite(v.max_value)))) {
        *why = "view max_value must be 0 or finite and positive";
        return false;
    }
    if (!view_why(typed_as_u8_view(v), why)) return false;
    const long long es = dec_elem_size(v.elem);
    if ((uintptr_t)v.data % (uintptr_t)es) {
        *why = "view data is not aligned to its " + std::to_string(es) + "-byte elements";
        return false;
    }
    const struct {
        const char* name;
        long long s;
    } st[3] = {{"row_stride", v.row_stride}, {"pixel_stride", v.pixel_stride}, {"channel_stride", v.channel_stride}};
    for (const auto& f : st)
        if (f.s % es) {
            *why = std::string("view ") + f.name + " " + std::to_string(f.s) + " is not a multiple of the " +
                   std::to_string(es) + "-byte element size";
            return false;
        }
    return true;
}

double typed_max_value(const phd_typed_view& v) {
    if (v.max_value != 0.0) return v.max_value;
    return v.elem == kElemU8 ? 255.0 : v.elem == kElemU16 ? 65535.0 : 1.0;
}

bool typed_is_u8_view(const phd_typed_view& v) { return v.elem == kElemU8 && typed_max_value(v) == 255.0; }

phd_image_view typed_as_u8_view(const phd_typed_view& v) {
    return phd_image_view{(const uint8_t*)v.data, v.height, v.width, v.row_stride, v.pixel_stride, v.channel_stride};
}

bool typed_snaps(const phd_typed_view& v) {
    return (v.flags & PHD_VIEW_SNAP_U8) && (v.elem == kElemF16 || v.elem == kElemF32) && typed_max_value(v) == 1.0;
}

namespace {

// (half)x, round to nearest even, for 0 <= x <= 1
uint16_t half_bits(double x) {
    if (x < 6.103515625e-05) return (uint16_t)std::rint(std::ldexp(x, 24));   // subnormal: units of 2^-24
    int e;
    (void)std::frexp(x, &e);                               // x = f * 2^e, f in [0.5, 1)
    int q = (int)std::rint(std::ldexp(x, 11 - e));         // 11 significant bits: [1024, 2048]
    if (q == 2048) {
        q = 1024;
        e++;
    }
    return (uint16_t)(((e - 1 + 15) << 10) | (q - 1024));
}

struct SnapTables {
    alignas(16) uint8_t bytes[kSnapBytes];
    SnapTables() {
        for (int j = 0; j < 256; j++) {
            const uint16_t h = half_bits((double)j / 255.0);
            const float f = (float)((double)j / 255.0);
            __builtin_memcpy(bytes + 2 * j, &h, 2);
            __builtin_memcpy(bytes + kSnapF32Offset + 4 * j, &f, 4);
        }
    }
};

}  // namespace

const uint8_t* snap_tables() {
    static const SnapTables t;
    return t.bytes;
}

DecodeRec decode_record(const phd_typed_view& v, double* planes, uint8_t* rgb8, const uint8_t* snap) {
    DecodeRec r{};
    r.src = (const uint8_t*)v.data;
    r.planes = planes;
    r.rgb8 = rgb8;
    r.snap = typed_snaps(v) && snap ? snap + (v.elem == kElemF32 ? kSnapF32Offset : 0) : nullptr;
    r.row_stride = v.row_stride;
    r.pixel_stride = v.pixel_stride;
    r.channel_stride = v.channel_stride;
    r.max_value = typed_max_value(v);
    r.height = v.height;
    r.width = v.width;
    r.elem = v.elem;
    r.kind = dec_kind(v.elem, v.pixel_stride, v.channel_stride);
    r.band_rows = decode_band_rows(v.height, v.width);
    return r;
}

// The decode of k_classify_views and k_decode_view (decode_views.hip) over
// host memory: the same records and the same row code (decode_view.h:
// decode_row), one lane.
int decode_view_host(const phd_typed_view* view, double* planes, uint8_t* rgb8, int* is_u8, std::string* why) {
    if (!view || !planes) {
        *why = "phd_debug_decode_view_host: bad arguments";
        return -1;
    }
    if (!typed_view_why(*view, why)) return -1;
    // (the 8-bit test runs with the bytes: a scratch image when only the verdict is wanted)
    std::string scratch;
    if (is_u8 && !rgb8) {
        scratch.resize(3 * (size_t)view->height * view->width);
        rgb8 = (uint8_t*)&scratch[0];
    }
    // the two kernels' records: planes alone (k_decode_view), the RGB8 image alone (k_classify_views)
    const DecodeRec rp = decode_record(*view, planes, nullptr, nullptr);
    for (int y = 0; y < rp.height; y++) (void)decode_row(rp, y, 0, 1);
    if (!rgb8) return 0;
    const DecodeRec rc = decode_record(*view, nullptr, rgb8, snap_tables());
    int bits = 0;
    for (int y = 0; y < rc.height; y++) bits |= decode_row(rc, y, 0, 1);
    if (is_u8) *is_u8 = !(bits & kDecNotU8);
    return 0;
}

}  // namespace phd

// The gather of k_pack_views (pack_views.hip) over host memory: the same
// records and the same row code (pack_view.h: pack_row), one lane.
extern "C" int phd_debug_pack_view_host(const phd_image_view* view, uint8_t* dst) {
    using namespace phd;
    std::string why;
    if (!view || !dst) return -1;
    if (!view_why(*view, &why)) return -1;
    const PackRec r = pack_record(*view, dst);
    for (int y = 0; y < r.height; y++) pack_row(r, y, 0, 1);
    return 0;
}

