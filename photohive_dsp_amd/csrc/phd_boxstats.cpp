// phd_boxstats.cpp -- box statistics: per crop box of a packed RGB8 image,
// get_rgb_statistics (src/image_processing.c:543-553) and get_hsv_average over
// rgb2hsv's s (src/image_processing.c:533-540, 372-417) on crop_image's box
// (src/image_processing.c:244-266), from exact integer sums.
// phd_box_stats_device (the stage alone), phd_free_box_stats and the host twin
// phd_debug_box_stats_host.  Records and row walk: box_stat_tiles.h; the
// 4-pixel unit: stat_unit.h; kernels: box_stats.hip.

#include <cstring>

#include "phd_host.h"
#include "box_stat_tiles.h"

using namespace phd;

namespace {

// One box's values from its sums: stats_from_sums, as the report's own
// statistics, and the definition's last line.
void box_stat_finish(const unsigned long long* m, unsigned long long n1, double s, long n, RGB_Statistics* st,
                     double* sbar) {
    *st = stats_from_sums(m, n);
    *sbar = (s - (1.0 - 0.999999) * (double)n1) / (double)n;
}

long box_pixels(const Crop_Boundaries* b, int k) {
    return (long)(b->bottom[k] - b->top[k]) * (long)(b->right[k] - b->left[k]);
}

// Device offsets of a job: records | items | sums | finish
struct BoxStatLayout {
    size_t o_items, o_sums, o_fin, total, up;
    explicit BoxStatLayout(const BoxStatJob& job) {
        const size_t nb = job.recs.size();
        o_items = al(sizeof(BoxStatRec) * nb);
        up = o_items + sizeof(BoxItem) * job.items.size();
        o_sums = al(up);
        o_fin = o_sums + al(sizeof(unsigned long long) * kBoxStatRec * nb);
        total = o_fin + al(sizeof(unsigned long long) * kBoxStatOut * nb);
    }
};

}  // namespace

namespace phd {

void BoxStatJob::add_image(const uint8_t* img, int width, const Crop_Boundaries* b) {
    for (int k = 0; k < b->N; k++) {
        box_plan((int)recs.size(), b->top[k], b->bottom[k], b->right[k] - b->left[k], &items);
        recs.push_back(BoxStatRec{img, width, b->left[k], b->right[k], 0});
    }
}

bool box_stats_alloc(phd_box_stats* bs, int n_boxes) {
    *bs = phd_box_stats{0, nullptr, nullptr};
    if (n_boxes <= 0) return true;
    void* p = malloc((sizeof(RGB_Statistics) + sizeof(double)) * (size_t)n_boxes);
    if (!p) {
        set_error("box statistics: out of memory");
        return false;
    }
    bs->n_boxes = n_boxes;
    bs->stats = (RGB_Statistics*)p;
    bs->average_saturation = (double*)(bs->stats + n_boxes);
    return true;
}

bool box_stats_fill(phd_box_stats* bs, const Crop_Boundaries* b, const unsigned long long* h) {
    const int nb = b ? b->N : 0;
    if (!box_stats_alloc(bs, nb)) return false;
    for (int k = 0; k < nb; k++, h += kBoxStatOut) {
        double s;
        memcpy(&s, h + 7, sizeof s);
        box_stat_finish(h, h[6], s, box_pixels(b, k), &bs->stats[k], &bs->average_saturation[k]);
    }
    return true;
}

const unsigned long long* box_stats_host(const Context* c) {
    return c->staged[kStBoxStat].h.as<const unsigned long long>();
}

// Own buffers, not the launch tables' (upload_table): a report run enqueues the
// job on its FFT stream while its tail stream's label launches use that table.
bool enqueue_box_stat_job(Context* c, const BoxStatJob& job, hipStream_t st) {
    if (job.recs.empty()) return true;
    if (job.items.size() > 0x7FFFFFFFu) {
        set_error("box statistics: too many items");
        return false;
    }
    const BoxStatLayout L(job);
    const size_t nb = job.recs.size(), fin_bytes = sizeof(unsigned long long) * kBoxStatOut * nb;
    Staged& S = c->staged[kStBoxStat];
    if (!S.reserve(L.total, std::max(L.up, fin_bytes))) return false;
    uint8_t* h = S.h.as<uint8_t>();
    uint8_t* d = S.d.as<uint8_t>();
    memset(h, 0, L.up);
    memcpy(h, job.recs.data(), sizeof(BoxStatRec) * nb);
    memcpy(h + L.o_items, job.items.data(), sizeof(BoxItem) * job.items.size());
    if (!S.up(L.up, st)) return false;
    PHD_HIP(hipMemsetAsync(d + L.o_sums, 0, sizeof(unsigned long long) * kBoxStatRec * nb, st));
    const int ps = c->prof.begin(kBoxStats, st);
    PHD_HIP(launch_box_stats((const BoxStatRec*)d, (const BoxItem*)(d + L.o_items), (int)job.items.size(),
                             (unsigned long long*)(d + L.o_sums), st));
    c->prof.end(ps, st);
    PHD_HIP(launch_box_stats_finish((const unsigned long long*)(d + L.o_sums), (int)nb,
                                    (unsigned long long*)(d + L.o_fin), st));
    return S.down(L.o_fin, fin_bytes, st);
}

}  // namespace phd

extern "C" void phd_free_box_stats(phd_box_stats* bs, int n) {
    if (!bs) return;
    for (int i = 0; i < n; i++) {
        free(bs[i].stats);
        bs[i] = phd_box_stats{0, nullptr, nullptr};
    }
}

extern "C" int phd_box_stats_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                    int n_images, const Crop_Boundaries* const* boxes, phd_box_stats* out,
                                    void* stream) {
    clear_error();
    auto bad = [](const std::string& what) {
        set_error("phd_box_stats_device: " + what);
        return -1;
    };
    if (out && n_images > 0)
        for (int i = 0; i < n_images; i++) out[i] = phd_box_stats{0, nullptr, nullptr};
    if (!d_images || !heights || !widths || !boxes || !out) return bad("NULL argument");
    if (n_images <= 0) return bad("n_images must be positive");
    BoxStatJob job;
    for (int i = 0; i < n_images; i++) {
        const std::string img = "image " + std::to_string(i) + ": ";
        if (!d_images[i]) return bad(img + "NULL image");
        if (heights[i] <= 0 || widths[i] <= 0) return bad(img + "height and width must be positive");
        std::string why;
        if (!crops_why(boxes[i], heights[i], widths[i], &why)) return bad(img + why);
        if (boxes[i]) job.add_image(d_images[i], widths[i], boxes[i]);
    }
    if (job.recs.empty()) return 0;                          // no box at all: nothing for the device
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const hipStream_t st = work_stream(c, stream);
    auto run = [&]() {
        if (!enqueue_box_stat_job(c, job, st)) return false;
        PHD_HIP(hipStreamSynchronize(st));                   // the result is on the host: waited for on any stream
        c->prof.collect();
        return true;
    };
    if (!run()) return -1;
    const unsigned long long* h = box_stats_host(c);
    for (int i = 0; i < n_images; i++) {
        if (!box_stats_fill(&out[i], boxes[i], h)) {
            phd_free_box_stats(out, n_images);
            return -1;
        }
        h += (size_t)out[i].n_boxes * kBoxStatOut;
    }
    return 0;
}

// The kernel's plan and row walk on the host: box_plan's items in order, each
// pass's units and tails as walker 0 of 1, the 4-pixel unit in its plain form.
extern "C" int phd_debug_box_stats_host(const uint8_t* rgb, int height, int width, const Crop_Boundaries* boxes,
                                        RGB_Statistics* stats, double* average_saturation,
                                        unsigned long long* sums) {
    clear_error();
    std::string why;
    if (!rgb || height <= 0 || width <= 0) why = "NULL image or non-positive size";
    else if (crops_why(boxes, height, width, &why) && boxes && boxes->N > 0 && (!stats || !average_saturation))
        why = "NULL stats or average_saturation";
    if (!why.empty()) {
        set_error("phd_debug_box_stats_host: " + why);
        return -1;
    }
    if (!boxes || boxes->N == 0) return 0;
    BoxStatJob job;
    job.add_image(rgb, width, boxes);
    std::vector<unsigned long long> rec((size_t)kBoxStatRec * job.recs.size(), 0ull);
    for (const BoxItem& it : job.items) {
        const BoxStatRec& r = job.recs[it.box];
        const int cols = r.right - r.left, rows = it.row1 - it.row0, nu = box_stat_row_units(cols);
        const int total = rows * nu;
        const long long pitch = 3LL * r.w;
        const uint8_t* base = r.img + 3LL * ((long long)it.row0 * r.w + r.left);
        unsigned long long* out = rec.data() + (size_t)it.box * kBoxStatRec;
        StatSums a{};
        for (int u0 = 0; u0 == 0 || u0 < total; u0 += kBoxStatPassUnits) {
            box_stat_units<1>(base, pitch, nu, u0, std::min(total, u0 + kBoxStatPassUnits), 0, 1,
                              [&](const uint8_t* const* q, int) {
                                  unsigned w[3];
                                  stat_words(q[0], w);
                                  stat4_sums(w[0], w[1], w[2], a, out + 8);
                              });
            if (u0 == 0)
                box_stat_tails(base, pitch, cols, rows, 0, 1,
                               [&](const uint8_t* p) { stat1_sums(p[0], p[1], p[2], a, out + 8); });
        }
        for (int k = 0; k < 6; k++) out[k] += a.m[k];
        out[6] += a.n1;
    }
    for (int k = 0; k < boxes->N; k++) {
        unsigned long long* out = rec.data() + (size_t)k * kBoxStatRec;
        out[7] = (unsigned long long)box_pixels(boxes, k);
        box_stat_finish(out, out[6], box_stat_s(out + 8), (long)out[7], &stats[k], &average_saturation[k]);
    }
    if (sums) memcpy(sums, rec.data(), sizeof(unsigned long long) * rec.size());
    return 0;
}
