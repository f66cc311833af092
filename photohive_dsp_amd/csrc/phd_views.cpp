// phd_views.cpp -- the image-view input stage on the host: the descriptor's
// validation, the pack launch's records, and the kernel's host-only twin
// phd_debug_pack_view_host (no HIP: this file and pack_view.h compile alone,
// tests/native/pack_view_asan.cpp).
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

