// phd_boxpal.cpp -- box palettes: per crop box of a palette label map (the lists
// of src/color_quantization.c:342-479 kept per pixel) the number of elements of
// every palette slot.  phd_box_palettes_device (the stage alone),
// phd_free_box_palettes and the host twin phd_debug_box_counts_host.
// Plan and row code: box_tiles.h; kernel: box_palette.hip.

#include <cstring>

#include "phd_host.h"
#include "box_tiles.h"

using namespace phd;

namespace {

// crop_pgm's convention (src/image_processing.c:213-232) in map coordinates:
// 0 <= left <= right <= mw, 0 <= top <= bottom <= mh; an empty box counts 0
bool box_ok(const Crop_Boundaries* b, int k, int mh, int mw, std::string* why) {
    const int t = b->top[k], bo = b->bottom[k], l = b->left[k], r = b->right[k];
    if (t < 0 || l < 0 || t > bo || l > r || bo > mh || r > mw) {
        *why = "box " + std::to_string(k) + " (top " + std::to_string(t) + ", bottom " + std::to_string(bo) +
               ", left " + std::to_string(l) + ", right " + std::to_string(r) + ") is inverted or outside the " +
               std::to_string(mh) + " x " + std::to_string(mw) + " map";
        return false;
    }
    return true;
}

// One map's arguments; *nb: its boxes.  No HIP call.
bool map_ok(const uint16_t* map, int mh, int mw, int n_slots, const Crop_Boundaries* boxes, int* nb,
            std::string* why) {
    *nb = 0;
    if (!map) return *why = "NULL map", false;
    if (reinterpret_cast<uintptr_t>(map) & 1) return *why = "the map is not 2-byte aligned", false;
    if (mh <= 0 || mw <= 0) return *why = "height and width must be positive", false;
    if (n_slots < 0 || n_slots > kBoxMaxSlots) return *why = "n_slots must be in 0..4096", false;
    if (!boxes || boxes->N == 0) return true;
    if (boxes->N < 0 || !boxes->top || !boxes->bottom || !boxes->left || !boxes->right)
        return *why = "bad box list (negative N or a NULL array)", false;
    for (int k = 0; k < boxes->N; k++)
        if (!box_ok(boxes, k, mh, mw, why)) return false;
    *nb = boxes->N;
    return true;
}

}  // namespace

namespace phd {

void BoxJob::add(const uint16_t* map, int mw, int n_slots, int top, int bottom, int left, int right) {
    box_plan((int)recs.size(), top, bottom, right - left, &items);
    recs.push_back(BoxRec{map, counters, mw, left, right, n_slots});
    counters += n_slots + 1;
}

// An image's boxes (image coordinates, validated by check_crops) on its mh x mw
// map: at downsample_rate ds > 1 a box covers the elements whose nominal
// position (y * ds, x * ds) lies inside it -- rows ceil(top / ds) ..
// min(ceil(bottom / ds), mh), columns alike; it may come out empty.
void BoxJob::add_image(const uint16_t* map, int mh, int mw, int ds, int n_slots, const Crop_Boundaries* b) {
    auto up = [ds](int v, int lim) { return std::min(ds > 1 ? (v + ds - 1) / ds : v, lim); };
    for (int k = 0; k < b->N; k++) {
        const int t = up(b->top[k], mh), l = up(b->left[k], mw);
        add(map, mw, n_slots, t, std::max(t, up(b->bottom[k], mh)), l, std::max(l, up(b->right[k], mw)));
    }
}

// *bp <- n_boxes rows of n_slots + 1 counters at h (one malloc; none for no boxes).
bool box_palette_fill(phd_box_palette* bp, int n_boxes, int n_slots, const uint32_t* h) {
    *bp = phd_box_palette{0, n_slots, nullptr};
    if (n_boxes <= 0) return true;
    const size_t bytes = sizeof(uint32_t) * (size_t)n_boxes * ((size_t)n_slots + 1);
    bp->counts = (uint32_t*)malloc(bytes);
    if (!bp->counts) {
        set_error("box palettes: out of memory");
        return false;
    }
    memcpy(bp->counts, h, bytes);
    bp->n_boxes = n_boxes;
    return true;
}

// The job's launch on st: records | items go up as one table, the counters
// (kStBoxPal) are zeroed by one memset and come down into its pinned block by
// one copy.  The items are walked by persistent blocks, so no table needs a
// second launch.  The caller waits for st.
bool enqueue_box_job(Context* c, const BoxJob& job, hipStream_t st) {
    const size_t cbytes = sizeof(unsigned) * (size_t)job.counters;
    Staged& S = c->staged[kStBoxPal];
    if (!S.reserve(cbytes, cbytes)) return false;
    PHD_HIP(hipMemsetAsync(S.d.as(), 0, cbytes, st));
    if (!job.items.empty()) {
        if (job.items.size() > 0x7FFFFFFFu) {
            set_error("box palettes: too many items");
            return false;
        }
        const size_t o_items = al(sizeof(BoxRec) * job.recs.size());
        const size_t bytes = o_items + sizeof(BoxItem) * job.items.size();
        uint8_t* tab = (uint8_t*)table_begin(c, bytes);
        if (!tab) return false;
        const size_t rbytes = sizeof(BoxRec) * job.recs.size();
        memcpy(tab, job.recs.data(), rbytes);
        memset(tab + rbytes, 0, o_items - rbytes);
        memcpy(tab + o_items, job.items.data(), sizeof(BoxItem) * job.items.size());
        if (!table_upload(c, bytes, st)) return false;
        const int ps = c->prof.begin(kBoxPalettes, st);
        const uint8_t* dt = c->staged[kStViews].d.as<const uint8_t>();
        PHD_HIP(launch_box_counts((const BoxRec*)dt, (const BoxItem*)(dt + o_items), (int)job.items.size(),
                                  S.d.as<unsigned>(), st));
        c->prof.end(ps, st);
        if (!table_launched(c, st)) return false;
    }
    return S.down(0, cbytes, st);
}

}  // namespace phd

extern "C" void phd_free_box_palettes(phd_box_palette* bp, int n) {
    if (!bp) return;
    for (int i = 0; i < n; i++) {
        free(bp[i].counts);
        bp[i] = phd_box_palette{0, 0, nullptr};
    }
}

extern "C" int phd_box_palettes_device(const uint16_t* const* d_labels, const int* map_heights, const int* map_widths,
                                       int n_maps, const int* n_slots, const Crop_Boundaries* const* boxes,
                                       phd_box_palette* out, void* stream) {
    clear_error();
    auto bad = [](const std::string& what) {
        set_error("phd_box_palettes_device: " + what);
        return -1;
    };
    if (out && n_maps > 0)
        for (int i = 0; i < n_maps; i++) out[i] = phd_box_palette{0, 0, nullptr};
    if (!d_labels || !map_heights || !map_widths || !n_slots || !boxes || !out) return bad("NULL argument");
    if (n_maps <= 0) return bad("n_maps must be positive");
    BoxJob job;
    std::vector<int> nb(n_maps);
    for (int i = 0; i < n_maps; i++) {
        std::string why;
        if (!map_ok(d_labels[i], map_heights[i], map_widths[i], n_slots[i], boxes[i], &nb[i], &why))
            return bad("map " + std::to_string(i) + ": " + why);
        const Crop_Boundaries* b = boxes[i];
        for (int k = 0; k < nb[i]; k++)
            job.add(d_labels[i], map_widths[i], n_slots[i], b->top[k], b->bottom[k], b->left[k], b->right[k]);
    }
    if (job.recs.empty()) {                                  // no box at all: nothing for the device
        for (int i = 0; i < n_maps; i++) out[i].n_slots = n_slots[i];
        return 0;
    }
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const hipStream_t st = work_stream(c, stream);
    auto run = [&]() {
        if (!enqueue_box_job(c, job, st)) return false;
        PHD_HIP(hipStreamSynchronize(st));                   // the result is on the host: waited for on any stream
        c->prof.collect();
        return true;
    };
    if (!run()) return -1;
    const unsigned* h = c->staged[kStBoxPal].h.as<const unsigned>();
    for (int i = 0; i < n_maps; i++) {
        if (!box_palette_fill(&out[i], nb[i], n_slots[i], h)) {
            phd_free_box_palettes(out, n_maps);
            return -1;
        }
        h += (size_t)nb[i] * ((size_t)n_slots[i] + 1);
    }
    return 0;
}

// The kernel's plan and row code on the host: box_plan's items in order, every
// unit of every row through box_unit.
extern "C" int phd_debug_box_counts_host(const uint16_t* map, int mh, int mw, int n_slots,
                                         const Crop_Boundaries* boxes, uint32_t* counts) {
    clear_error();
    std::string why;
    int nb = 0;
    if (!map_ok(map, mh, mw, n_slots, boxes, &nb, &why) || (nb > 0 && !counts)) {
        set_error("phd_debug_box_counts_host: " + (why.empty() ? std::string("NULL counts") : why));
        return -1;
    }
    BoxJob job;
    for (int k = 0; k < nb; k++)
        job.add(map, mw, n_slots, boxes->top[k], boxes->bottom[k], boxes->left[k], boxes->right[k]);
    if (nb > 0) memset(counts, 0, sizeof(uint32_t) * (size_t)job.counters);
    for (const BoxItem& it : job.items) {
        const BoxRec& r = job.recs[it.box];
        const int cols = r.right - r.left, nu = box_row_units(cols);
        uint32_t* row_counts = counts + r.out;
        for (int y = it.row0; y < it.row1; y++)
            for (int k = 0; k < nu; k++)
                box_unit(r.map + (long)y * r.mw + r.left, cols, k, r.n_slots,
                         [&](unsigned slot, unsigned n) { row_counts[slot] += n; });
    }
    return 0;
}
