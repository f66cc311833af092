// phd_labels.cpp -- phd_labels_to_rgb_device, the quantised image of a palette
// label map (the maps themselves: ReportRun::label_maps, phd_report.cpp).
// Kernels: palette_labels.hip.

#include <cstring>

#include "phd_host.h"

using namespace phd;

// The colours calculate_avg_hsv's averages (src/color_quantization.c:510-576)
// stand for, painted per pixel: one launch over all maps; the table is the
// records, then every map's LUT as one word per slot.
extern "C" int phd_labels_to_rgb_device(const uint16_t* const* d_labels, const int* map_heights,
                                        const int* map_widths, int n_maps, const uint8_t* const* luts,
                                        const int* n_slots, const uint8_t none_rgb[3], uint8_t* const* d_dst,
                                        void* stream) {
    clear_error();
    auto bad = [](const std::string& what) {
        set_error("phd_labels_to_rgb_device: " + what);
        return -1;
    };
    if (!d_labels || !map_heights || !map_widths || !luts || !n_slots || !none_rgb || !d_dst)
        return bad("NULL argument");
    if (n_maps <= 0 || n_maps > 65535) return bad("n_maps must be in 1..65535");
    size_t lut_words = 0;
    for (int i = 0; i < n_maps; i++) {
        const std::string im = "map " + std::to_string(i);
        if (!d_labels[i] || !d_dst[i]) return bad(im + ": NULL map or destination");
        if (map_heights[i] <= 0 || map_widths[i] <= 0) return bad(im + ": height and width must be positive");
        if (n_slots[i] < 0 || n_slots[i] > 0xFFFF) return bad(im + ": n_slots must be in 0..65535");
        if (n_slots[i] > 0 && !luts[i]) return bad(im + ": NULL lut");
        lut_words += (size_t)n_slots[i];
    }
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const hipStream_t st = work_stream(c, stream);
    const size_t rec_bytes = al(sizeof(LabelRgbRec) * (size_t)n_maps), bytes = rec_bytes + 4 * lut_words;
    // filled in the pinned block (the device table has its final address by then: the records point into it)
    uint8_t* tab = (uint8_t*)table_begin(c, bytes);
    if (!tab) return -1;
    memset(tab, 0, rec_bytes);
    LabelRgbRec* recs = reinterpret_cast<LabelRgbRec*>(tab);
    unsigned* words = reinterpret_cast<unsigned*>(tab + rec_bytes);
    const unsigned* d_words = reinterpret_cast<const unsigned*>(c->staged[kStViews].d.as<const uint8_t>() + rec_bytes);
    const unsigned none = (unsigned)none_rgb[0] | (unsigned)none_rgb[1] << 8 | (unsigned)none_rgb[2] << 16;
    long max_npix = 0;
    size_t w = 0;
    for (int i = 0; i < n_maps; i++) {
        const long npix = (long)map_heights[i] * map_widths[i];
        max_npix = std::max(max_npix, npix);
        recs[i] = LabelRgbRec{d_labels[i], d_dst[i], d_words + w, npix, n_slots[i], none};
        for (int k = 0; k < n_slots[i]; k++)
            words[w++] = (unsigned)luts[i][3 * k] | (unsigned)luts[i][3 * k + 1] << 8 |
                         (unsigned)luts[i][3 * k + 2] << 16;
    }
    auto run = [&]() {
        if (!table_upload(c, bytes, st)) return false;
        PHD_HIP(launch_labels_to_rgb(c->staged[kStViews].d.as<const LabelRgbRec>(), n_maps, max_npix, st));
        if (!table_launched(c, st)) return false;
        if (!stream) PHD_HIP(hipStreamSynchronize(st));
        return true;
    };
    return run() ? 0 : -1;
}
