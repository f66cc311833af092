// phd_assemble.cpp -- a report as one pooled heap block: the pool, the
// assembly of Full_Report_Data from the pipeline's host records, and the
// entries that free reports.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include <unordered_map>
#include <unordered_set>

#include "phd_host.h"

namespace phd {

// pgm_normalize_fft's G_s (src/fft_processing.c:192) applied to the binned
// sums of log(p); calculate_blur_profile's averaging (src/blur_profile.c:106-116);
// vectorize_blur_profile (src/blur_profile.c:324-416).  flat: na x nr.
void finish_blur(const BlurTable& tbl, const unsigned long long* bin_sums, double fmax, const phd_config& cfg,
                 double* flat, Blur_Vector* vectors, double bscale) {
    const int na = cfg.angle_partitions, nr = cfg.radius_partitions;
    const double gs = 1 / (2 * std::log(std::sqrt(fmax) + 1));
    const double scale = bscale > 0.0 ? bscale : bin_scale(tbl.height, tbl.wf);
    for (size_t b = 0; b < (size_t)na * nr; b++) {
        const double q = (double)tbl.counts[b];
        // the device sums are bin_scale fixed point (order-independent)
        const double sum = bin_sums[b] == 0ull ? 0.0 : (double)bin_sums[b] / scale * gs;
        flat[b] = q != 0 ? sum / q : 0;
    }
    vectorize_blur(flat, na, nr, cfg.fft_streak_thresh, cfg.magnitude_thresh, cfg.blur_cutoff_ratio_denom, vectors);
}

namespace {

// A report is one heap block (a 16-byte header with its size, then every
// structure and array of Full_Report_Data), and free_full_report hands the
// block to a pool that the next report of the same size takes it from: a
// 256-image batch's 3,000 separate mallocs and frees (and the heap trims and
// page faults between batches) cost ~0.9 ms per batch with the GPU idle.
constexpr size_t kReportHdr = 16;
constexpr unsigned long long kReportMagic = 0x5048445245504f52ull;   // "PHDREPOR"
// The pool also keeps the set of blocks that are live reports: free_full_report
// pools a block only if it is in that set, so a pointer this library did not
// return (or a report already freed and not yet handed out again) is ignored
// without reading memory around it.  A stale pointer to a block that a later
// report has taken again cannot be told from that report (as with free()):
// freeing it twice after such a reuse is undefined.
struct ReportPool {
    pid_t pid = 0;                                           // the process that made this pool
    std::mutex m;
    std::unordered_map<size_t, std::vector<void*>> blocks;   // by block size
    std::unordered_set<const void*> live;                    // blocks handed out as reports
    size_t bytes = 0;
    static constexpr size_t kCap = (size_t)512 << 20;        // pooled bytes at most
    void* take(size_t sz) {
        void* b = nullptr;
        {
            std::lock_guard<std::mutex> lk(m);
            auto it = blocks.find(sz);
            if (it != blocks.end() && !it->second.empty()) {
                b = it->second.back();
                it->second.pop_back();
                bytes -= sz;
            }
        }
        if (!b) b = malloc(sz);
        if (b) {
            std::lock_guard<std::mutex> lk(m);
            live.insert(b);
        }
        return b;
    }
    // returns false (and leaves the block alone) when b is not a live report
    bool give(void* b) {
        std::lock_guard<std::mutex> lk(m);
        if (!live.erase(b)) return false;
        const size_t sz = (size_t)reinterpret_cast<unsigned long long*>(b)[0];
        reinterpret_cast<unsigned long long*>(b)[1] = 0;
        if (bytes + sz > kCap) {
            free(b);
            return true;
        }
        blocks[sz].push_back(b);
        bytes += sz;
        return true;
    }
};
ReportPool& report_pool() {
    // process lifetime (reports may be freed at exit); a forked child starts a
    // pool of its own (the parent's mutex may have been held at the fork).  One
    // pointer holds both the pool and the pid that made it, so a thread cannot
    // pair one process's pool with another's pid.
    static std::atomic<ReportPool*> p{nullptr};
    ReportPool* q = p.load(std::memory_order_acquire);
    const pid_t me = getpid();
    if (!q || q->pid != me) {
        static std::mutex init;
        std::lock_guard<std::mutex> lk(init);
        q = p.load(std::memory_order_acquire);
        if (!q || q->pid != me) {
            q = new ReportPool;
            q->pid = me;
            p.store(q, std::memory_order_release);
        }
    }
    return *q;
}
size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

Full_Report_Data* assemble(const RGB_Statistics& st, double s_bar, const PaletteDecision& dec,
                           const double* pal, long n_hsv, const BlurTable& tbl, const unsigned long long* bin_sums,
                           double fmax, const phd_config& cfg, const Crop_Boundaries* crops,
                           const double* sharp_sums, std::string* why, double bscale) {
    const int np = (int)dec.parents.size();
    const int na = cfg.angle_partitions, nr = cfg.radius_partitions;
    const int nsh = crops ? (crops->N > 0 ? crops->N : 1) : 0;
    // the block: header | report | stats | palette + arrays | profile + row
    // pointers + rows | vector group + 10 vectors | sharpnesses + values
    size_t o = kReportHdr;
    const size_t o_r = o; o = al16(o + sizeof(Full_Report_Data));
    const size_t o_rs = o; o = al16(o + sizeof(RGB_Statistics));
    const size_t o_cp = o; o = al16(o + sizeof(Color_Palette));
    const size_t o_avg = o; o = al16(o + sizeof(Pixel_HSV) * (np > 0 ? np : 1));
    const size_t o_pct = o; o = al16(o + sizeof(double) * (np > 0 ? np : 1));
    const size_t o_bp = o; o = al16(o + sizeof(Blur_Profile));
    const size_t o_bptr = o; o = al16(o + sizeof(Bin*) * (na > 0 ? na : 1));
    const size_t o_rows = o; o = al16(o + sizeof(Bin) * ((size_t)na * nr > 0 ? (size_t)na * nr : 1));
    const size_t o_bv = o; o = al16(o + sizeof(Blur_Vector_Group));
    const size_t o_vec = o; o = al16(o + sizeof(Blur_Vector) * 10);
    const size_t o_sh = o; o = al16(o + (crops ? sizeof(Sharpnesses) : 0));
    const size_t o_shv = o; o = al16(o + sizeof(Pixel) * (size_t)nsh);
    const size_t size = (o + 4095) & ~(size_t)4095;           // a few size classes for the pool
    char* blk = (char*)report_pool().take(size);
    if (!blk) {
        *why = "report allocation failed";
        return nullptr;
    }
    reinterpret_cast<unsigned long long*>(blk)[0] = size;
    reinterpret_cast<unsigned long long*>(blk)[1] = kReportMagic;
    // calculate_avg_hsv (src/color_quantization.c:510-576)
    Color_Palette* cp = (Color_Palette*)(blk + o_cp);
    cp->N = np;
    cp->averages = (Pixel_HSV*)(blk + o_avg);
    cp->percentages = (double*)(blk + o_pct);
    const double inv_n = 1.0 / (int)n_hsv;
    for (int k = 0; k < np; k++) {
        const double cnt = pal[4 * k + 3];
        static const bool ablating = phd_knob("PHD_ABLATE") != nullptr;   // timing experiments only
        if (cnt != (double)dec.kept[k] && !ablating) {
            *why = "palette self-check failed: device kept " + std::to_string((long long)cnt) +
                   " pixels for slot " + std::to_string(k) + ", host rules predict " +
                   std::to_string(dec.kept[k]);
            report_pool().give(blk);
            return nullptr;
        }
        const int tot = (int)dec.kept[k];
        const double inv = 1.0 / (double)tot;
        double h = pal[4 * k + 0] * inv;
        h -= dec.off[k];
        if (h < 0) h += 360;
        else if (h > 360) h -= 360;
        cp->averages[k].parent_id = dec.parents[k];   // uninitialised in the reference
        cp->averages[k].h = h;
        cp->averages[k].s = pal[4 * k + 1] * inv;
        cp->averages[k].v = pal[4 * k + 2] * inv;
        cp->percentages[k] = (double)tot * inv_n;
    }
    // pgm_normalize_fft's G_s (src/fft_processing.c:192) applied to the binned
    // sums of log(p); calculate_blur_profile's averaging (src/blur_profile.c:106-116)
    Blur_Profile* bp = (Blur_Profile*)(blk + o_bp);
    bp->num_angle_bins = na;
    bp->num_radius_bins = nr;
    bp->angle_bin_size = tbl.angle_bin_size;
    bp->radius_bin_size = tbl.radius_bin_size;
    // bins[angle][radius] as the reference's row pointers into one run of rows
    bp->bins = (Bin**)(blk + o_bptr);
    Bin* rows = (Bin*)(blk + o_rows);                          // finish_blur writes every bin
    for (int a = 0; a < na; a++) bp->bins[a] = rows + (size_t)a * nr;
    Blur_Vector_Group* bv = (Blur_Vector_Group*)(blk + o_bv);
    bv->len_vectors = 10;
    bv->blur_vectors = (Blur_Vector*)(blk + o_vec);
    memset(bv->blur_vectors, 0, sizeof(Blur_Vector) * 10);    // calloc in the reference
    finish_blur(tbl, bin_sums, fmax, cfg, rows, bv->blur_vectors, bscale);
    Sharpnesses* sh = nullptr;
    if (crops) {   // get_variance_sharpness (src/filtering.c:151-183)
        sh = (Sharpnesses*)(blk + o_sh);
        sh->N = crops->N;
        sh->sharpness = (Pixel*)(blk + o_shv);
        memset(sh->sharpness, 0, sizeof(Pixel) * (size_t)nsh);
        for (int k = 0; k < crops->N; k++) {
            const double cn = (double)((long)(crops->right[k] - crops->left[k]) *
                                       (crops->bottom[k] - crops->top[k]));
            const double avg = sharp_sums[2 * k] / cn;
            const double var = sharp_sums[2 * k + 1] / cn;
            sh->sharpness[k] = var / avg;
        }
    }
    RGB_Statistics* rs = (RGB_Statistics*)(blk + o_rs);
    *rs = st;
    Full_Report_Data* r = (Full_Report_Data*)(blk + o_r);
    r->rgb_stats = rs;
    r->color_palette = cp;
    r->blur_profile = bp;
    r->blur_vectors = bv;
    r->average_saturation = s_bar;
    r->sharpness = sh;
    return r;
}

RGB_Statistics stats_from_sums(const unsigned long long* m, long n) {
    // mean = sum(k)/255/N; population variance from exact integer moments:
    // var = (N*sum(k^2) - sum(k)^2) / (255^2 N^2)   (filtering.c:125-148 in exact arithmetic)
    RGB_Statistics s;
    double* out = &s.Br;
    for (int c = 0; c < 3; c++) {
        out[c] = (double)m[c] / 255.0 / (double)n;
        const unsigned __int128 num = (unsigned __int128)n * m[3 + c] - (unsigned __int128)m[c] * m[c];
        const double var = (double)num / 65025.0 / ((double)n * (double)n);
        out[3 + c] = std::sqrt(var);
    }
    return s;
}

}  // namespace phd

using namespace phd;

extern "C" void phd_free_reports(Full_Report_Data** reports, int n) {
    for (int i = 0; reports && i < n; i++) free_full_report(&reports[i]);
}

extern "C" void free_full_report(Full_Report_Data** report) {
    // src/interface.c:97-111 frees each structure.  A report of the batch
    // entry points is one block (assemble), which goes back to the report
    // pool; a report of get_full_report_data is a tree of separate mallocs
    // (phd_legacy.cpp), freed member by member.  Neither (foreign, or already
    // freed): ignored, without reading memory around the pointer.
    if (!report || !*report) return;
    if (legacy_release(*report)) {
        *report = nullptr;
        return;
    }
    char* blk = reinterpret_cast<char*>(*report) - kReportHdr;
    if (!report_pool().give(blk) && getenv("PHD_VERBOSE"))
        fprintf(stderr, "free_full_report: %p is not a live report of this library; ignored\n", (void*)*report);
    *report = nullptr;
}
