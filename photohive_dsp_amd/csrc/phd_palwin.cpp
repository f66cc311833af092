// phd_palwin.cpp -- window palettes: per T x T window (T = 16, 32, 64 or 128) of a
// palette label map (the lists of src/color_quantization.c:342-479 and :510-576
// kept per pixel, inside crop_pgm's box, src/image_processing.c:213-232) the
// number of elements of every palette slot and the slot that dominates, left in
// device memory.  phd_palette_windows_device (window lists) and
// phd_palette_maps_device (a regular grid per map) through one body: every window
// of every map of a call in one launch; and the host twin
// phd_debug_window_palette_host.
// The entries' windows -- checks, counts and the walk that fills the table -- are a
// WindowPlan and the twin's checks window_twin_why (window_call.h), both saying
// "map"; the launch goes through table_call (phd_host.h).
// The unit, the copies rule, the dominant key and the table: pal_window.h; kernel:
// window_palette.hip.
// With PHD_PALWIN_HOST_ONLY the twin compiles alone, without HIP
// (tests/native/window_palette_asan.cpp brings set_error and clear_error).

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#ifdef PHD_PALWIN_HOST_ONLY
namespace phd {
void set_error(const std::string& msg);
void clear_error();
}  // namespace phd
#else
#include "phd_host.h"
#endif
#include "window_call.h"
#include "pal_window.h"

using namespace phd;

namespace {

bool pal_size_why(int window, std::string* why) {
    if (pw_size_ok(window)) return true;
    return *why = "window must be 16, 32, 64 or 128, not " + std::to_string(window), false;
}

bool pal_slots_why(int n_slots, std::string* why) {
    if (n_slots >= 0 && n_slots <= kPalWinMaxSlots) return true;
    return *why = "n_slots must be in 0..4096, not " + std::to_string(n_slots), false;
}

}  // namespace

#ifndef PHD_PALWIN_HOST_ONLY
static_assert(kPalWinMaxSlots == kBoxMaxSlots, "the box palettes' slot cap");
static_assert(kPalWinNone == (unsigned)PHD_LABEL_NONE, "the label maps' none");

namespace {

// After the plan: per map its palette, its base's alignment, and one output at
// least wherever it has windows (either array may be NULL or hold NULL entries).
bool pal_maps_why(const WindowPlan& plan, const int* n_slots, uint32_t* const* d_counts, uint16_t* const* d_dominant,
                  std::string* why) {
    for (int i = 0; i < plan.n_images; i++) {
        const std::string map = "map " + std::to_string(i) + ": ";
        std::string slots_why;
        if (!pal_slots_why(n_slots[i], &slots_why)) return *why = map + slots_why, false;
        if (reinterpret_cast<uintptr_t>(plan.d_images[i]) & 1)
            return *why = map + "the map is not 2-byte aligned", false;
        if (plan.count[i] == 0) continue;
        const uint32_t* c = d_counts ? d_counts[i] : nullptr;
        const uint16_t* d = d_dominant ? d_dominant[i] : nullptr;
        if (!c && !d)
            return *why = map + "neither d_counts nor d_dominant for " + std::to_string(plan.count[i]) + " windows",
                   false;
        if (reinterpret_cast<uintptr_t>(c) & 3) return *why = map + "d_counts is not 4-byte aligned", false;
        if (reinterpret_cast<uintptr_t>(d) & 1) return *why = map + "d_dominant is not 2-byte aligned", false;
    }
    return true;
}

// Both entries: the plan of their windows (lists, or a regular grid per map).
int pal_windows_call(const char* entry, WindowPlan plan, const int* n_slots, uint32_t* const* d_counts,
                     uint16_t* const* d_dominant, void* stream) {
    clear_error();
    std::string why;
    if (!plan.args_why(n_slots && (d_counts || d_dominant), &why) || !pal_size_why(plan.T, &why) ||
        !plan.build(nullptr, nullptr, &why) || !pal_maps_why(plan, n_slots, d_counts, d_dominant, &why)) {
        set_error(std::string(entry) + ": " + why);
        return -1;
    }
    if (plan.total == 0) return 0;                           // no window at all: nothing for the device
    const int T = plan.T;
    const size_t nw = (size_t)plan.total;
    int lds_words = 4;                                       // the launch's LDS: the call's palettes'
    for (int i = 0; i < plan.n_images; i++)
        if (plan.count[i] > 0) lds_words = std::max(lds_words, pw_lds_words(n_slots[i] + 1, T));
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    // the call's table: window records | their destinations
    const size_t o_dst = al(sizeof(PalWinRec) * nw), bytes = o_dst + sizeof(PalWinDst) * nw;
    auto fill = [&](uint8_t* h) {
        PalWinRec* recs = (PalWinRec*)h;
        PalWinDst* dst = (PalWinDst*)(h + o_dst);
        memset(h + sizeof(PalWinRec) * nw, 0, o_dst - sizeof(PalWinRec) * nw);
        size_t w = 0;
        plan.for_each([&](int i, long long k, long long top, long long left) {
            const uint16_t* map = (const uint16_t*)plan.d_images[i];
            const long long mw = plan.widths[i];
            recs[w] = PalWinRec{map + top * mw + left, (unsigned long long)mw, n_slots[i], 0};
            uint32_t* cn = d_counts ? d_counts[i] : nullptr;
            uint16_t* dm = d_dominant ? d_dominant[i] : nullptr;
            dst[w++] = PalWinDst{cn ? cn + ((size_t)n_slots[i] + 1) * (size_t)k : nullptr, dm ? dm + k : nullptr};
        });
    };
    auto launch = [&](const uint8_t* d, hipStream_t st) {
        return launch_window_palette(T, (const PalWinRec*)d, (const PalWinDst*)(d + o_dst), (int)nw, lds_words, st);
    };
    return table_call(c, stream, bytes, fill, launch, kWindowPalette) ? 0 : -1;
}

}  // namespace

extern "C" int phd_palette_windows_device(const uint16_t* const* d_labels, const int* map_heights,
                                          const int* map_widths, int n_maps, const int* n_slots,
                                          const Crop_Boundaries* const* windows, int window,
                                          uint32_t* const* d_counts, uint16_t* const* d_dominant, void* stream) {
    return pal_windows_call("phd_palette_windows_device",
                            WindowPlan((const uint8_t* const*)d_labels, map_heights, map_widths, n_maps, windows, true,
                                       window, 0, "map"),
                            n_slots, d_counts, d_dominant, stream);
}

extern "C" int phd_palette_maps_device(const uint16_t* const* d_labels, const int* map_heights, const int* map_widths,
                                       int n_maps, const int* n_slots, int window, int stride,
                                       uint32_t* const* d_counts, uint16_t* const* d_dominant, void* stream) {
    return pal_windows_call("phd_palette_maps_device",
                            WindowPlan((const uint8_t* const*)d_labels, map_heights, map_widths, n_maps, nullptr, false,
                                       window, stride, "map"),
                            n_slots, d_counts, d_dominant, stream);
}
#endif  // PHD_PALWIN_HOST_ONLY

// k_window_palette's twin: the window's units row by row through pw_unit (T is a
// multiple of 4: a row has no label left over), each unit's 8 bytes read at their
// own address, then the dominant key over the columns in ascending order.
extern "C" int phd_debug_window_palette_host(const uint16_t* map, int mh, int mw, int n_slots,
                                             const Crop_Boundaries* windows, int window, uint32_t* counts,
                                             uint16_t* dominant) {
    clear_error();
    std::string why, size_why;
    pal_size_why(window, &size_why);
    if (!window_twin_why((const uint8_t*)map, mh, mw, windows, window, size_why, counts || dominant,
                         "NULL counts and dominant", &why, "map") ||
        !pal_slots_why(n_slots, &why)) {
        set_error("phd_debug_window_palette_host: " + why);
        return -1;
    }
    if (!windows || windows->N == 0) return 0;
    const int T = window;
    const size_t nc = (size_t)n_slots + 1;
    std::vector<uint32_t> row_counts(nc);
    for (int k = 0; k < windows->N; k++) {
        const uint16_t* first = map + ((long long)windows->top[k] * mw + windows->left[k]);
        std::fill(row_counts.begin(), row_counts.end(), 0u);
        for (int y = 0; y < T; y++) {
            const uint16_t* row = first + (long long)mw * y;
            for (int u = 0; u < T / 4; u++) {
                unsigned long long q;
                memcpy(&q, row + 4 * u, 8);
                pw_unit(q, (unsigned)n_slots, [&](unsigned s, unsigned run) { row_counts[s] += run; });
            }
        }
        if (counts) memcpy(counts + nc * (size_t)k, row_counts.data(), sizeof(uint32_t) * nc);
        if (dominant) {
            unsigned key = 0;
            for (size_t s = 0; s < nc; s++) key = std::max(key, pw_key(row_counts[s], (unsigned)s));
            dominant[k] = (uint16_t)pw_key_label(key, (unsigned)n_slots);
        }
    }
    return 0;
}
