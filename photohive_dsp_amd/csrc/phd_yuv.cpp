// phd_yuv.cpp -- the YCbCr input stage on the host: the descriptor's
// validation, the conversion launch's records, and the kernel's host-only twin
// yuv_view_host (no HIP: this file, yuv_view.h and pack_view.h compile alone,
// tests/native/yuv_view_asan.cpp).
#include <string>

#include "yuv_plan.h"

namespace phd {

bool yuv_view_why(const phd_yuv_view& v, std::string* why) {
    const struct {
        const char* name;
        const uint8_t* p;
    } planes[3] = {{"y", v.y}, {"cb", v.cb}, {"cr", v.cr}};
    for (const auto& p : planes)
        if (!p.p) {
            *why = std::string("yuv view ") + p.name + " is NULL";
            return false;
        }
    if (v.height <= 0 || v.width <= 0) {
        *why = "yuv view height and width must be positive (height " + std::to_string(v.height) + ", width " +
               std::to_string(v.width) + ")";
        return false;
    }
    const int sx = v.chroma_shift_x, sy = v.chroma_shift_y;
    if (!((sx == 0 && sy == 0) || (sx == 1 && sy == 0) || (sx == 1 && sy == 1))) {
        *why = "yuv view chroma_shift_x, chroma_shift_y (" + std::to_string(sx) + ", " + std::to_string(sy) +
               ") is not (0,0), (1,0) or (1,1)";
        return false;
    }
    const struct {
        const char* name;
        int value, count;
    } enums[3] = {{"matrix", v.matrix, 2}, {"range", v.range, 2}, {"chroma", v.chroma, 2}};
    for (const auto& e : enums)
        if (e.value < 0 || e.value >= e.count) {
            *why = std::string("yuv view ") + e.name + " " + std::to_string(e.value) + " is not a PHD_YUV_* value";
            return false;
        }
    const int ch = (v.height + sy) >> sy, cw = (v.width + sx) >> sx;
    const struct {
        const char* name;
        long long stride;
        int extent;
        const char* of;
    } strides[4] = {{"y_pixel_stride", v.y_pixel_stride, v.width, "width"},
                    {"y_row_stride", v.y_row_stride, v.height, "height"},
                    {"c_pixel_stride", v.c_pixel_stride, cw, "chroma width"},
                    {"c_row_stride", v.c_row_stride, ch, "chroma height"}};
    for (const auto& s : strides)
        if (s.stride == 0 && s.extent > 1) {
            *why = std::string("yuv view ") + s.name + " is 0 with " + s.of + " " + std::to_string(s.extent);
            return false;
        }
    return true;
}

YuvRec yuv_record(const phd_yuv_view& v, uint8_t* dst) {
    YuvRec r{};
    r.y = v.y;
    r.cb = v.cb;
    r.cr = v.cr;
    r.dst = dst;
    r.y_rs = v.y_row_stride;
    r.y_ps = v.y_pixel_stride;
    r.c_rs = v.c_row_stride;
    r.c_ps = v.c_pixel_stride;
    r.height = v.height;
    r.width = v.width;
    r.sx = v.chroma_shift_x;
    r.sy = v.chroma_shift_y;
    r.ch = (v.height + r.sy) >> r.sy;
    r.cw = (v.width + r.sx) >> r.sx;
    r.mode = !r.sx ? kYuvDirect : v.chroma == PHD_YUV_CHROMA_REPLICATE ? kYuvReplicate : r.sy ? kYuvTri420 : kYuvTri422;
    r.band_rows = yuv_band_rows(v.height, v.width, r.sy);
    int k[6];
    yuv_coeffs(v.matrix, v.range, k);
    r.cy = k[0], r.crv = k[1], r.cgu = k[2], r.cgv = k[3], r.cbu = k[4], r.yoff = k[5];
    // the layout's vector form: where the three pointers lie relative to each other
    const uintptr_t py = (uintptr_t)v.y, pb = (uintptr_t)v.cb, pc = (uintptr_t)v.cr;
    const uintptr_t q = py < pb ? (py < pc ? py : pc) : (pb < pc ? pb : pc);
    const uintptr_t oy = py - q, ob = pb - q, oc = pc - q;
    r.lay = kYuvGeneric;
    if (r.sx == 1 && r.sy == 0 && r.y_ps == 2 && r.c_ps == 4 && (r.c_rs == r.y_rs || r.height == 1) && oy <= 1 &&
        ob <= 3 && oc <= 3 && ob != oc && ((ob ^ oy) & 1) && ((oc ^ oy) & 1)) {
        r.lay = kYuvQuad;                               // Y U Y V in any of its four orders
        r.shifts = (int)(8 * oy | (8 * ob) << 8 | (8 * oc) << 16);
    } else if (r.sx == 1 && r.c_ps == 2 && (pb + 1 == pc || pc + 1 == pb)) {
        r.lay = kYuvPairs;                              // NV12 (Cb first) / NV21
        r.shifts = pb < pc ? 8 << 16 : 8 << 8;
    } else if (r.c_ps == 1) {
        r.lay = kYuvPlanar;
    }
    return r;
}

// The conversion of k_yuv_views (yuv_views.hip) over host memory: the same
// record and the same row code (yuv_view.h: yuv_row), one lane.
int yuv_view_host(const phd_yuv_view* view, uint8_t* dst, std::string* why) {
    if (!view || !dst) {
        *why = "phd_debug_yuv_view_host: bad arguments";
        return -1;
    }
    if (!yuv_view_why(*view, why)) return -1;
    const YuvRec r = yuv_record(*view, dst);
    for (int y = 0; y < r.height; y++) yuv_row(r, y, 0, 1);
    return 0;
}

}  // namespace phd
