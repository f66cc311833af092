// phd_report.cpp -- the report pipeline (its C-ABI entries: phd_entries.cpp
// and phd_inputs.cpp; report assembly: phd_assemble.cpp; hooks: phd_debug.cpp).
//
// Stage order of get_full_report_data (src/interface.c:20-94), per batch of
// same-size device images on one stream:
//
//   K0  gather of non-packed views    views calls only   (pack_views.hip)
//       YCbCr -> RGB8 conversion      YUV calls only     (yuv_views.hip)
//   K1  hsv/stats/histogram           every image        (palette.hip)
//   D2H group histograms + moments    -> host decisions  (phd_palette.cpp)
//   K4  FFT rows, K5 FFT columns      every image        (fft.hip)   || host decides
//   H2D keep rules;  Kcut; K3 sums    every image        (palette.hip)
//   sharpness (crops only)                                (sharpness.hip)
//     shared boxes: two launches per box after each image's column pass;
//     per-image boxes (batch calls): one batched launch after K1
//   D2H bins / max / palette sums -> host finalisation (G_s, averages, vectors)
//
// The FFT of an image depends only on K1's channel sums (for the DC bias), so
// the host's palette decisions overlap the GPU's FFT work.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "phd_host.h"

namespace phd {

namespace {

struct Layout {
    // per-image records
    size_t a_sums, a_hist, a_spart, a_gsum, a_gcell, a_bytes;  // read back after K1 (zeroed)
    size_t c_bins, c_fmax, c_pal, c_sharp, c_bytes;         // read back at the end (zeroed)
    size_t b_rules, b_search, b_off, b_bytes;               // uploaded before K3
    size_t chunk_bytes;                                      // device only
    size_t ptr_bytes;                                        // image pointer array (pinned -> device)
    size_t e_entries, e_ns, e_bytes;                         // Kcut (image, group) list + slots per image
    size_t dev_total, pin_total;
    size_t A(int i) const { return (size_t)i * a_bytes; }
    size_t C(int n, int i) const { return (size_t)n * a_bytes + (size_t)i * c_bytes; }
    size_t B(int n, int i) const { return (size_t)n * (a_bytes + c_bytes) + (size_t)i * b_bytes; }
    // E follows the B records on both sides, so one H2D copy carries both
    size_t E_dev(int n) const { return (size_t)n * (a_bytes + c_bytes + b_bytes); }
    size_t E_pin(int n) const { return E_dev(n); }
    size_t H(int n, int i) const { return E_dev(n) + e_bytes + (size_t)i * chunk_bytes; }
    size_t P_dev(int n) const { return H(n, n); }
    size_t P_pin(int n) const { return E_pin(n) + e_bytes; }
};

// ncell > 0: the fused palette's per-group sums and hue-cell counts ride in
// the K1 record.
Layout make_layout(int n, int tl, int nchunks, int nbins, int ncrops, int ncolblocks, int ncell = 0) {
    Layout L{};
    L.a_sums = 0;
    L.a_hist = al(6 * sizeof(unsigned long long));
    L.a_spart = L.a_hist + al(sizeof(unsigned) * tl);
    L.a_gsum = L.a_spart + al(sizeof(double) * nchunks);
    L.a_gcell = L.a_gsum + (ncell > 0 ? al(sizeof(double) * 3 * tl) : 0);
    L.a_bytes = L.a_gcell + (ncell > 0 ? al(sizeof(unsigned) * ncell) : 0);
    L.c_bins = 0;
    L.c_fmax = al(sizeof(double) * nbins);
    L.c_pal = L.c_fmax + al(sizeof(double) * (ncolblocks > 0 ? ncolblocks : 1));
    L.c_sharp = L.c_pal + al(sizeof(double) * 4 * tl);
    L.c_bytes = L.c_sharp + al(sizeof(double) * 2 * (ncrops > 0 ? ncrops : 1));
    L.b_rules = 0;
    L.b_search = al(sizeof(GroupRule) * tl);
    L.b_off = L.b_search + al(sizeof(int) * tl);
    L.b_bytes = L.b_off + al(sizeof(double) * tl);
    L.chunk_bytes = al(sizeof(unsigned short) * (size_t)nchunks * tl);
    L.ptr_bytes = al(sizeof(void*) * (size_t)n);
    L.e_entries = 0;
    L.e_ns = al(2 * sizeof(int) * (size_t)n * tl);
    L.e_bytes = L.e_ns + al(sizeof(int) * (size_t)n);
    L.dev_total = (size_t)n * (L.a_bytes + L.c_bytes + L.b_bytes + L.chunk_bytes) + L.ptr_bytes + L.e_bytes;
    L.pin_total = (size_t)n * (L.a_bytes + L.c_bytes + L.b_bytes) + L.ptr_bytes + L.e_bytes;
    return L;
}

}  // namespace

// shared with the planar path (phd_planar.cpp)
bool check_crops(const Crop_Boundaries* cb, int height, int width) {
    // the rules: crops_why (phd_sharp_host.cpp)
    std::string why;
    if (crops_why(cb, height, width, &why)) return true;
    set_error(why);
    return false;
}

bool enqueue_sharpness(Context* c, const uint8_t* const* d_imgs, int n, int width, const SharpPlan& plan,
                       double* out0, long out_stride, hipStream_t st, double** flat_dev) {
    const int nb = (int)plan.boxes.size();
    if (flat_dev) *flat_dev = nullptr;
    if (nb == 0) return true;
    const int nslices = plan.prefix[nb];
    // uploaded: image pointers | boxes | prefix; device only: partials | flat sums
    const size_t o_box = al(sizeof(void*) * (size_t)n);
    const size_t o_pre = o_box + al(sizeof(SharpBox) * (size_t)nb);
    const size_t up = o_pre + al(sizeof(int) * ((size_t)nb + 1));
    const size_t o_flat = up + al(sizeof(SharpPart) * (size_t)nslices);
    const size_t total = o_flat + (out0 ? 0 : al(2 * sizeof(double) * (size_t)nb));
    Staged& S = c->staged[kStSharp];
    if (!S.reserve(total, up)) return false;
    uint8_t* hs = S.h.as<uint8_t>();
    uint8_t* ds = S.d.as<uint8_t>();
    memcpy(hs, d_imgs, sizeof(void*) * (size_t)n);
    memcpy(hs + o_box, plan.boxes.data(), sizeof(SharpBox) * (size_t)nb);
    memcpy(hs + o_pre, plan.prefix.data(), sizeof(int) * ((size_t)nb + 1));
    if (!S.up(up, st)) return false;
    double* dst = out0 ? out0 : (double*)(ds + o_flat);
    if (flat_dev) *flat_dev = dst;
    PHD_HIP(launch_sharpness_batch((const uint8_t* const*)ds, (const SharpBox*)(ds + o_box), (const int*)(ds + o_pre),
                                   nb, nslices, width, c->d_k255, (SharpPart*)(ds + up), dst, out0 ? out_stride : 0,
                                   st, &c->prof));
    return true;
}

// pre_compute_error_checks (src/utilities.c:64-87) on the dimensions.
bool precheck(int height, int width) {
    if (height < 350 || width < 350) {
        set_error("Error: Image height and width must be greater than 350. Height: " + std::to_string(height) +
                  "\tWidth" + std::to_string(width));
        return false;
    }
    if ((long long)height * width > 120000000LL) {
        set_error("Error: Image must have less than 120000000 pixels.");
        return false;
    }
    const float ar = (float)height / (float)width;
    if (ar < 1.0 / 5.0 || ar > 5.0 / 1.0) {
        set_error("Error: Invalid aspect ratio: " + std::to_string(ar));
        return false;
    }
    return true;
}

long hsv_count(int height, int width, int ds) {
    const int hh = ds > 1 ? height / ds : height, ww = ds > 1 ? width / ds : width;
    return (long)(short)hh * (short)ww;
}

float ms_between(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return -1.f;
    return ms;
}

bool all_aligned(const uint8_t* const* p, int n) {
    for (int i = 0; i < n; i++)
        if (reinterpret_cast<uintptr_t>(p[i]) & 3) return false;
    return true;
}

// Image i's K1 outputs in the workspace of an n-image call
PaletteDev palette_dev(uint8_t* dw, const Layout& L, int n, int i) {
    PaletteDev pd;
    pd.sums = (unsigned long long*)(dw + L.A(i) + L.a_sums);
    pd.hist = (unsigned*)(dw + L.A(i) + L.a_hist);
    pd.s_part = (double*)(dw + L.A(i) + L.a_spart);
    pd.chunk_hist = (unsigned short*)(dw + L.H(n, i));
    return pd;
}

// A decision's B record at b: keep rules | search list | hue offsets
void fill_b_record(const Layout& L, const PaletteDecision& dec, int tl, uint8_t* b) {
    memcpy(b + L.b_rules, dec.rules.data(), sizeof(GroupRule) * tl);
    memcpy(b + L.b_search, dec.search.data(), sizeof(int) * dec.search.size());
    memcpy(b + L.b_off, dec.off.data(), sizeof(double) * dec.off.size());
}

// K1 for n same-size images: one batched launch (ds == 1) over the device
// pointer array staged in the workspace, or per-image launches (ds > 1).
bool launch_k1(Context* c, const Layout& L, int n, const uint8_t* const* d_imgs, int height, int width, int ds,
               const GridParams& gp, const Context::Cls* cls, int nchunks, bool fused, hipStream_t st) {
    uint8_t* dw = c->dev[kDevWs].as<uint8_t>();
    uint8_t* hp = c->pin.as<uint8_t>();
    PaletteDev pd = palette_dev(dw, L, n, 0);
    pd.gsum = (double*)(dw + L.A(0) + L.a_gsum);
    pd.gcell = (unsigned*)(dw + L.A(0) + L.a_gcell);
    // the device image-pointer array: K1 (ds == 1), the batched runtime-plan FFT
    // passes and the batched palette tail read it, whatever the downsample rate
    memcpy(hp + L.P_pin(n), d_imgs, sizeof(void*) * n);
    PHD_HIP(hipMemcpyAsync(dw + L.P_dev(n), hp + L.P_pin(n), sizeof(void*) * n, hipMemcpyHostToDevice, st));
    const int ps = c->prof.begin(kK1, st);
    if (ds <= 1) {
        PHD_HIP(launch_hsv_stats_batch((const uint8_t* const*)(dw + L.P_dev(n)), n, height, width, gp, cls->fc,
                                       cls->d, pd, (long)L.a_bytes, (long)L.chunk_bytes, nchunks, c->d_k255,
                                       true, fused, all_aligned(d_imgs, n), st));
    } else {
        for (int i = 0; i < n; i++) {
            PHD_HIP(launch_hsv_ds(d_imgs[i], height, width, ds, gp, cls->fc, cls->d, palette_dev(dw, L, n, i), nchunks,
                                  c->d_k255, st));
        }
    }
    c->prof.end(ps, st);
    return true;
}

// calculate_avg_hsv's slot sums (src/color_quantization.c:520-550) of every
// group a slot keeps whole, from the fused K1's per-group records: sum over
// the group of wrap(h + off) = sum(h) + n * off - 360 * #(h + off > 360)
// + 360 * #(h + off < 0), the wrap counts being sums of hue-cell counts on
// one side of the parent's threshold (HueCells).  Partial groups are left to
// the device (k_partial_sums_b).  Adds into hs[4 * slot + {h, s, v, n}].
bool fused_slot_sums(const GridParams& gp, const PaletteDecision& dec, const unsigned* hist, const double* gsum,
                     const unsigned* gcell, double* hs, std::string* why) {
    const int tl = gp.tl, gs = HueCells::gray_start(gp), hp = gp.hp, sv = gp.sp * gp.vp;
    for (int g = 0; g < tl; g++) {
        const GroupRule& r = dec.rules[g];
        if (r.slot < 0 || r.partial || hist[g] == 0) continue;
        const int k = r.slot, p = dec.parents[k];
        // the parent's threshold cell cT and direction: +1 wraps down (-360)
        // above cT, -1 wraps up (+360) below cT, 0 never
        int cT = 0, dir = 0;
        if (p >= gs) {
            cT = hp;                                   // h = 0, off = 180: h > 180 wraps
            dir = 1;
        } else {
            const int t = 2 * (p / sv) + 1;            // 2 * h_parent / Lh
            if (t < hp) { cT = t + hp; dir = 1; }
            else if (t > hp) { cT = t - hp; dir = -1; }
        }
        long long tot = 0, above = 0;
        auto cell = [&](int cg, unsigned cnt) {
            tot += cnt;
            if (cg >= cT) above += cnt;
        };
        if (g < gs) {
            const int hi = g / sv;
            for (int l = 0; l < 4; l++) cell(std::max(0, 2 * hi - 1 + l), gcell[4 * g + l]);
        } else {
            for (int cg = 0; cg < 2 * hp; cg++) cell(cg, gcell[4 * gs + (g - gs) * 2 * hp + cg]);
        }
        if (tot != (long long)hist[g]) {
            *why = "fused palette self-check failed: hue cells of group " + std::to_string(g) + " hold " +
                   std::to_string(tot) + " pixels, the histogram " + std::to_string(hist[g]);
            return false;
        }
        const double n = (double)hist[g];
        double wrap = 0.0;
        if (dir > 0) wrap = -360.0 * (double)above;
        else if (dir < 0) wrap = 360.0 * (double)(tot - above);
        hs[4 * k + 0] += gsum[g] + n * dec.off[k] + wrap;
        hs[4 * k + 1] += gsum[tl + g];
        hs[4 * k + 2] += gsum[2 * tl + g];
        hs[4 * k + 3] += n;
    }
    return true;
}

bool palette_tail_batched(const GridParams& gp, int ds, bool fused, int max_slots) {
    return ds <= 1 && (fused || palette_sums_b_lds(gp.tl, max_slots) <= 160 * 1024);
}

// The palette's second pass for n images on s2, their B records (and the Kcut
// list behind them) filled in the pinned workspace: one upload, then one Kcut
// and one K3 launch over the whole batch, or (downsampled images, grids past
// the batched K3's LDS) a pair of launches per image that has a decision (ok).
bool launch_palette_tail(Context* c, const Layout& L, int n, const uint8_t* const* d_imgs, int height, int width,
                         int ds, const GridParams& gp, const Context::Cls* cls, int nchunks, bool fused,
                         const PaletteDecision* dec, const int* ok, int n_ent, int max_slots, int max_per_img,
                         hipStream_t s2) {
    uint8_t* dw = c->dev[kDevWs].as<uint8_t>();
    const uint8_t* hb = c->pin.as<uint8_t>() + L.B(n, 0);
    const bool batched = palette_tail_batched(gp, ds, fused, max_slots);
    // the B records (and, batched, the Kcut list right after them): one copy
    PHD_HIP(hipMemcpyAsync(dw + L.B(n, 0), hb, (size_t)n * L.b_bytes + (batched ? L.e_bytes : 0),
                           hipMemcpyHostToDevice, s2));
    if (batched) {
        // one Kcut and one K3 launch over the whole batch
        const uint8_t* const* d_ptrs = (const uint8_t* const*)(dw + L.P_dev(n));
        // timing experiments only: PHD_ABLATE bit 1024 skips the tail kernels (wrong palette sums)
        const bool skip_tail = (env_ablate() & 1024) != 0;
        int ps = n_ent ? c->prof.begin(kCutoffs, s2) : -1;
        if (!skip_tail) PHD_HIP(launch_cutoffs_batch(d_ptrs, d_imgs, n, height, width, gp, cls->fc, cls->d, c->d_k255,
                                     (const int2*)(dw + L.E_dev(n) + L.e_entries), n_ent,
                                     (const unsigned short*)(dw + L.H(n, 0)), (long)L.chunk_bytes,
                                     (GroupRule*)(dw + L.B(n, 0) + L.b_rules), (long)L.b_bytes, s2));
        c->prof.end(ps, s2);
        if (fused) {
            // only the partial groups' kept prefixes are left to sum on the device
            ps = n_ent ? c->prof.begin(kPalSums, s2) : -1;
            if (!skip_tail) PHD_HIP(launch_partial_sums_batch(d_ptrs, d_imgs, n, height, width, gp, cls->fc, cls->d, c->d_k255,
                                              (const int2*)(dw + L.E_dev(n) + L.e_entries), n_ent,
                                              (const unsigned short*)(dw + L.H(n, 0)), (long)L.chunk_bytes,
                                              (const GroupRule*)(dw + L.B(n, 0) + L.b_rules),
                                              (const double*)(dw + L.B(n, 0) + L.b_off), (long)L.b_bytes,
                                              (double*)(dw + L.C(n, 0) + L.c_pal), (long)L.c_bytes, max_per_img, s2));
            c->prof.end(ps, s2);
        } else {
            ps = c->prof.begin(kPalSums, s2);
            PHD_HIP(launch_palette_sums_batch(d_ptrs, d_imgs, n, height, width, gp, cls->fc, cls->d, c->d_k255,
                                              (const GroupRule*)(dw + L.B(n, 0) + L.b_rules),
                                              (const double*)(dw + L.B(n, 0) + L.b_off), (long)L.b_bytes,
                                              (const int*)(dw + L.E_dev(n) + L.e_ns), max_slots,
                                              (double*)(dw + L.C(n, 0) + L.c_pal), (long)L.c_bytes, s2));
            c->prof.end(ps, s2);
        }
    } else {
        for (int i = 0; i < n; i++) {
            if (!ok[i]) continue;
            GroupRule* rules = (GroupRule*)(dw + L.B(n, i) + L.b_rules);
            const int* search = (const int*)(dw + L.B(n, i) + L.b_search);
            const double* off = (const double*)(dw + L.B(n, i) + L.b_off);
            int ps = dec[i].search.empty() ? -1 : c->prof.begin(kCutoffs, s2);
            PHD_HIP(launch_palette_cutoffs(d_imgs[i], height, width, ds, gp,
                                           (const unsigned short*)(dw + L.H(n, i)), nchunks, rules, search,
                                           (int)dec[i].search.size(), c->d_k255, s2));
            c->prof.end(ps, s2);
            ps = c->prof.begin(kPalSums, s2);
            PHD_HIP(launch_palette_sums(d_imgs[i], height, width, ds, gp, rules, off,
                                        (int)dec[i].parents.size(), (double*)(dw + L.C(n, i) + L.c_pal),
                                        c->d_k255, s2));
            c->prof.end(ps, s2);
        }
    }
    return true;
}

namespace {

// Arms the thread-local launch_events() for the launches of its scope, so one
// of them records the events with its own dispatch and completion; disarmed
// when the scope ends, on every path.
struct ArmedLaunchEvents {
    const bool armed;
    ArmedLaunchEvents(bool on, hipEvent_t start, hipEvent_t stop) : armed(on) {
        if (armed) launch_events() = LaunchEvents{start, stop, false};
    }
    ArmedLaunchEvents(const ArmedLaunchEvents&) = delete;
    ~ArmedLaunchEvents() { if (armed) launch_events() = LaunchEvents{}; }
    bool used() const { return armed && launch_events().used; }   // a launch has recorded them
};

using Clock = std::chrono::steady_clock;

struct ReportArgs {
    Context* c;
    const uint8_t* const* d_imgs;
    int n, height, width;
    const phd_config& cfg;
    const Crop_Boundaries* crops;
    Full_Report_Data** out;
    int* status;
    hipStream_t stream;
    const Crop_Boundaries* const* img_crops;
    const ImageOutputs* outs;                                 // per image (phd_host.h), or NULL: none
};

// How a call's FFT chain is launched: a row and a column launch per image, or
// one of each per group of Q images (runtime-plan or compile-time kernels).
enum class FftChain { kPerImage, kRuntimeBatch, kCtBatch };

// One run_reports call: its arguments, what plan() derives from them once,
// and what each stage hands to the next.  The stages run in the order of
// run_reports' last line; each returns false with the error set.
struct ReportRun : ReportArgs {
    explicit ReportRun(const ReportArgs& a) : ReportArgs(a) {}
    // plan()
    GridParams gp{};
    int ds = 1, nchunks = 0, nbins = 0, ncrops = 0, wf = 0;
    long n_hsv = 0;
    const BlurTable* tbl = nullptr;
    FftSel fs;
    const Context::Cls* cls = nullptr;
    bool fused = false;                                       // one pixel pass for the palette (else K1 + K3)
    Layout L{};
    FftChain chain = FftChain::kPerImage;
    int Q = 1, dlg = 1;                                       // images per FFT group; per download group
    size_t inter_elems = 0;                                   // one image's half-spectrum intermediate
    SharpPlan splan;                                          // per-image boxes: the whole call's box table
    std::vector<int> crop_arr;                                // shared boxes: top | bottom | left | right
    hipStream_t st = nullptr, s2 = nullptr;                   // K1 + FFT chain; palette tail + downloads
    uint8_t *dw = nullptr, *hp = nullptr;                     // the workspace and its pinned mirror
    // k1(): the event after K1, the stream of the A-record download, K1 recorded ev[0] / ev[1] itself
    hipEvent_t ev_k1 = nullptr;
    hipStream_t sa = nullptr;
    bool k1_rec = false;
    // palette_tail(), assemble_groups()
    std::vector<int> ok;
    std::vector<std::string> fail_why;
    int n_ent = 0, max_slots = 1, max_per_img = 0, failures = 0;
    Clock::time_point t_host0 = Clock::now(), t_enq, t_k1, t_dec_only, t_dec, t_sync, t_end;

    // the last image of a download group (one event and one copy per group;
    // the last image always ends a group)
    bool dl_end(int i) const { return (i + 1) % dlg == 0 || i == n - 1; }
    int dl_last(int i) const { return std::min(n - 1, (i / dlg + 1) * dlg - 1); }
    uint8_t* hc() const { return hp + (size_t)n * L.a_bytes; }   // the C records on the host

    bool plan(), k1(), fft_chain(), palette_tail(), downloads(), assemble_groups(), timings();
    // image i's outputs; whether any image of the run asks for the output m
    ImageOutputs o(int i) const { return outs ? outs[i] : ImageOutputs{}; }
    template <class T>
    bool any(T ImageOutputs::*m) const {
        for (int i = 0; i < n; i++)
            if (o(i).*m) return true;
        return false;
    }
    bool label_maps();                                        // palette_tail()'s last step: maps and box counts
    bool label_launches(const std::vector<LabelDst>& dst, bool aligned);
    // box palettes: image i's boxes are counted (it has a decision, a struct
    // and boxes); where its counters start in kStBoxPal's pinned block (-1: none)
    bool counts_boxes(int i) const {
        return o(i).box_pal && ok[i] && img_crops && img_crops[i] && img_crops[i]->N > 0;
    }
    std::vector<long long> bp_off;
    bool box_palettes();                                      // the last stage: the structs of the reported images
    // box statistics: image i's boxes are summed (it has a struct and boxes);
    // where its boxes start in the job's download (-1: none)
    bool sums_boxes(int i) const {
        return o(i).box_stats && img_crops && img_crops[i] && img_crops[i]->N > 0;
    }
    std::vector<long long> bs_off;
    bool box_stat_job();                                      // fft_chain()'s first step, with the sharpness launch
    bool box_statistics();                                    // after box_palettes(): the reported images' structs
};

// Validation, tables, FFT selection, layout, buffers, the shared-box array.
bool ReportRun::plan() {
    for (int i = 0; i < n; i++) {
        out[i] = nullptr;
        status[i] = -1;
    }
    std::string why;
    if (!validate_config(cfg, &why)) {
        set_error(why);
        return false;
    }
    if (!precheck(height, width) || !check_crops(crops, height, width)) return false;
    if (img_crops) {
        if (crops) {
            set_error("run_reports: shared and per-image crop boxes together");
            return false;
        }
        for (int i = 0; i < n; i++)
            if (!check_crops(img_crops[i], height, width)) return false;
        if (!sharp_plan(img_crops, n, false, &splan)) {
            set_error("too many crop boxes in one call");
            return false;
        }
    }
    st = work_stream(c, stream);
    // ev_img_fft only orders the download stream after a column pass on this
    // device (device_event_flags: no system-scope fence)
    while ((int)c->ev_img_fft.size() < n) {
        hipEvent_t a, b;
        PHD_HIP(hipEventCreateWithFlags(&a, device_event_flags()));
        PHD_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        c->ev_img_fft.push_back(a);
        c->ev_img_dl.push_back(b);
    }
    // a failed earlier call may have left work on the side stream
    PHD_HIP(hipStreamSynchronize(c->tail));
    s2 = c->tail;
    gp = make_grid(cfg);
    ds = cfg.downsample_rate > 1 ? cfg.downsample_rate : 1;
    n_hsv = hsv_count(height, width, ds);
    nchunks = (int)((n_hsv + kChunk - 1) / kChunk);
    nbins = cfg.radius_partitions * cfg.angle_partitions;
    ncrops = crops ? crops->N : 0;
    wf = width / 2 + 1;
    tbl = get_table(c, height, width, cfg.radius_partitions, cfg.angle_partitions);
    if (!tbl) return false;
    // compile-time plans: images small enough that two or more half-spectrum
    // intermediates fit 128 MB (half the MALL) run as one row and one column
    // launch per group of images (sizes whose row pairs form whole line groups
    // of the row schedule); small images are otherwise bound by per-launch costs
    inter_elems = phd::inter_elems(height, width);
    const size_t inter_one = sizeof(double2) * inter_elems;
    static const bool ctbatch_off = phd_knob("PHD_CT_NO_BATCH") != nullptr;
    const int q_ct = (int)std::min<size_t>((size_t)n, ((size_t)128 << 20) / inter_one);
    const bool ct_batchable = !ctbatch_off && n > 1 && q_ct >= 2 && ((height + 1) / 2) % 4 == 0;
    if (!select_fft(c, height, width, nbins, d_imgs, n, &fs, tbl, ct_batchable)) return false;
    cls = get_cls(c, gp);
    if (!cls) return false;
    // the column pass's full-prefetch form (24 KB more LDS per block): on a
    // call split over two lanes whose K1 runs the two-block form (one
    // 512-thread block per CU beside the other lane's FFTs) the half-prefetch
    // form measured 9.05k images/s against its 8.67k at 4000x3000, 18/2/3,
    // where FFT-only calls and the fine grids' one-block K1 gain with the full
    // form
    if (FftSel::forced_form() < 0 && ds <= 1 && k1_blocks_per_cu() == 1 && cls->fc.k1t_cshift2 >= 0)
        fs.col_pf = false;

    // images whose result records go to the host together.  Each event between
    // back-to-back FFT kernels costs ~5 us; larger groups delay the host's
    // assembly of the early images.  Measured at 4000x3000, 8 images: groups
    // of 1 / 2 / 4 / 8 give FFT stages of 0.857 / 0.838 / 0.828 / 0.823 ms and
    // 6.16k / 6.21k / 6.17k / 6.08k images/s.
    static const int dl_group = phd_knob("PHD_DL_GROUP") ? std::max(1, atoi(phd_knob("PHD_DL_GROUP"))) : 2;
    // fused palette (one pixel pass): ds == 1 and the fused K1's LDS fits; else K1 + K3
    fused = ds <= 1 && fused_palette_ok(gp);
    L = make_layout(n, gp.tl, nchunks, nbins, img_crops ? splan.max_boxes : ncrops, fs.col_blocks,
                    fused ? HueCells::count(gp) : 0);
    // half-spectrum intermediates: one per image of a group of Q (the group's row
    // passes run before its column passes); large images one at a time, so the
    // intermediate stays in the 256 MB MALL between its two passes (round 2:
    // a two-stream pipeline of rows i+1 beside columns i measured 10 % slower)
    // (+ 1024 elements of scratch past the tiles for the row pass's dummy stores)
    // runtime-plan sizes: the passes of a group of images are one launch each
    // (grid.y = image), the group's intermediates within 128 MB (half the
    // MALL); small images are otherwise bound by per-launch latency
    static const bool gbatch_off = phd_knob("PHD_FFT_NO_BATCH") != nullptr;
    const bool strided = L.a_bytes % 8 == 0 && L.c_bytes % 8 == 0;   // the batched kernels' record strides
    if (!fs.ct && !fs.generic && !gbatch_off && n > 1 && strided) {
        chain = FftChain::kRuntimeBatch;
        Q = std::max(1, std::min(n, (int)(((size_t)128 << 20) / inter_one)));
    }
    if (fs.ct && ct_batchable && strided) {
        chain = FftChain::kCtBatch;
        Q = q_ct;
    }
    // batched FFT launches finish a whole group of Q images at once: one
    // event, one download and one host wait per group (small images were
    // bound by ~3 HIP calls and a wait per pair of images: DESIGN.md section 12)
    dlg = chain == FftChain::kPerImage ? dl_group : Q;
    if (!c->dev[kDevWs].ensure(L.dev_total) || !c->pin.ensure(L.pin_total) ||
        !c->dev[kDevInter].ensure((size_t)Q * inter_one))
        return false;
    dw = c->dev[kDevWs].as<uint8_t>();
    hp = c->pin.as<uint8_t>();
    if (ncrops) {
        crop_arr.resize(4 * ncrops);
        for (int k = 0; k < ncrops; k++) {
            crop_arr[k] = crops->top[k];
            crop_arr[ncrops + k] = crops->bottom[k];
            crop_arr[2 * ncrops + k] = crops->left[k];
            crop_arr[3 * ncrops + k] = crops->right[k];
        }
    }
    return true;
}

// K1 on st and the A records' download (sa), ev[5] behind it.
bool ReportRun::k1() {
    PHD_HIP(hipMemsetAsync(dw, 0, (size_t)n * (L.a_bytes + L.c_bytes), st));
    // An unprofiled one-launch K1 records its stage events with its own
    // dispatch and completion (no marker packets between it and the first row
    // pass), and ev[1] then stands for ev_k1; the A records go down on the
    // download stream, beside the FFTs instead of ahead of them.
    static const bool k1_events_off = phd_knob("PHD_K1_MARKERS") != nullptr;
    const bool k1_own = ds <= 1 && !(c->prof.mask & (1u << kK1)) && !k1_events_off &&
                        device_event_flags() == hipEventDisableSystemFence;
    if (!k1_own) PHD_HIP(hipEventRecord(c->ev[0], st));
    {
        ArmedLaunchEvents own(k1_own, c->ev[0], c->ev[1]);
        const bool k1_ok = launch_k1(c, L, n, d_imgs, height, width, ds, gp, cls, nchunks, fused, st);
        k1_rec = own.used();
        if (!k1_ok) return false;
    }
    if (k1_own && !k1_rec) PHD_HIP(hipEventRecord(c->ev[0], st));   // (a K1 path without phd_launch: timing only)
    if (!k1_rec) PHD_HIP(hipEventRecord(c->ev[1], st));
    if (!k1_rec) PHD_HIP(hipEventRecord(c->ev_k1, st));
    ev_k1 = k1_rec ? c->ev[1] : c->ev_k1;
    // the A records go down on the side stream (tail), beside the FFTs
    sa = k1_rec ? c->tail : st;
    if (sa != st) PHD_HIP(hipStreamWaitEvent(sa, ev_k1, 0));
    PHD_HIP(hipMemcpyAsync(hp, dw, (size_t)n * L.a_bytes, hipMemcpyDeviceToHost, sa));
    PHD_HIP(hipEventRecord(c->ev[5], sa));
    return true;
}

// The FFT chain follows K1 on its stream and takes its channel sums (the
// column pass's DC bias): a cross-stream event wait left the GPU idle
// ~20 us between K1 and the first row pass.  Per group of Q images: the row
// launch(es), the column launch(es), then the shared boxes' sharpness and the
// download groups' events.
bool ReportRun::fft_chain() {
    const hipStream_t sf = st;
    // per-image boxes: every box of the call once, ahead of the FFTs (and so of
    // every download group's event); the sums land in the images' C records
    if (img_crops && !enqueue_sharpness(c, d_imgs, n, width, splan, (double*)(dw + L.C(n, 0) + L.c_sharp),
                                        (long)(L.c_bytes / 8), sf))
        return false;
    if (any(&ImageOutputs::box_stats) && !box_stat_job()) return false;
    const uint8_t* const* d_ptrs = (const uint8_t* const*)(dw + L.P_dev(n));
    const long a_stride = (long)(L.a_bytes / 8), c_stride = (long)(L.c_bytes / 8);
    double2* const inter = c->dev[kDevInter].as<double2>();
    for (int g0 = 0; g0 < n; g0 += Q) {
        const int g1 = std::min(n, g0 + Q), m = g1 - g0;
        const unsigned long long* sums = (const unsigned long long*)(dw + L.A(g0) + L.a_sums);
        auto* bins = (unsigned long long*)(dw + L.C(n, g0) + L.c_bins);
        double* fmx = (double*)(dw + L.C(n, g0) + L.c_fmax);
        bool recorded = false;                                // a column launch recorded the group's event itself
        int ps = c->prof.begin(kFftRows, sf);
        if (chain == FftChain::kRuntimeBatch)
            PHD_HIP(launch_fft_rows_batch(d_ptrs + g0, m, height, width, fs.prow->plan, sums, a_stride, c->d_k255,
                                          inter, inter_elems, sf));
        else if (chain == FftChain::kCtBatch)
            PHD_HIP(launch_fft_rows_ct_batch(d_ptrs + g0, m, height, width, c->d_k255, fs.tw_r, inter,
                                             (long)inter_elems, sf));
        else   // (a per-image group is one image)
            PHD_HIP(launch_rows_sel(fs, d_imgs[g0], height, width, sums, c->d_k255, inter, sf, nullptr));
        c->prof.end(ps, sf);
        ps = c->prof.begin(kFftCols, sf);
        if (chain == FftChain::kRuntimeBatch) {
            PHD_HIP(launch_fft_cols_batch(inter, inter_elems, m, height, wf, fs.pcol->plan, tbl->d_map, nbins,
                                          bins, fmx, c_stride, sf));
        } else if (chain == FftChain::kCtBatch) {
            PHD_HIP(launch_fft_cols_ct_batch(inter, (long)inter_elems, m, height, width, wf, fs.cbins, bins,
                                             c_stride, fmx, c_stride, fs.tw_c, sums, a_stride, sf, fs.col_pf));
        } else {
            // an unprofiled column pass that ends a download group records the
            // group's event itself (its completion signal): a separate event
            // record between two kernels leaves the GPU idle ~4 us
            // (compile-time plans only: one launch is the whole column pass)
            ArmedLaunchEvents own(fs.ct && ps < 0 && dl_end(g0) && !ncrops &&
                                      device_event_flags() == hipEventDisableSystemFence,
                                  nullptr, c->ev_img_fft[g0]);
            PHD_HIP(launch_cols_sel(fs, inter, height, width, wf, tbl->d_map, nbins, bins, fmx, sums, nullptr,
                                    sf));
            recorded = own.used();
        }
        c->prof.end(ps, sf);
        for (int i = g0; i < g1; i++) {
            // shared crop boxes: sharpness on the full-resolution luma before DC removal
            if (ncrops)
                PHD_HIP(launch_sharpness(d_imgs[i], height, width, ncrops, crop_arr.data(),
                                         crop_arr.data() + ncrops, crop_arr.data() + 2 * ncrops,
                                         crop_arr.data() + 3 * ncrops, c->d_k255,
                                         (double*)(dw + L.C(n, i) + L.c_sharp), sf, &c->prof));
            if (dl_end(i) && !recorded) PHD_HIP(hipEventRecord(c->ev_img_fft[i], sf));
        }
    }
    // the last column pass ends the FFT work (it waited for the last row pass)
    PHD_HIP(hipEventRecord(c->ev[2], sf));
    PHD_HIP(hipEventRecord(c->ev_fft, sf));
    t_enq = Clock::now();
    return true;
}

// The box statistics of every image of the run that has a struct and boxes: one
// job (one table copy, one memset, k_box_stats and its finish, one download) on
// the FFT stream ahead of the FFTs, beside the sharpness launch.  It needs only
// the image bytes and the boxes, so no decision is waited for; its download is
// on the host by the run's final wait (ev[4] follows the FFT stream).
bool ReportRun::box_stat_job() {
    BoxStatJob job;
    bs_off.assign(n, -1);
    for (int i = 0; i < n; i++) {
        if (!sums_boxes(i)) continue;
        bs_off[i] = (long long)job.recs.size();
        job.add_image(d_imgs[i], width, img_crops[i]);
    }
    return enqueue_box_stat_job(c, job, st);
}

// The host's palette decisions while the FFTs run, then the palette's second
// pass on the tail stream, after K1, concurrent with the FFTs.
bool ReportRun::palette_tail() {
    PHD_HIP(hipEventSynchronize(c->ev[5]));
    t_k1 = Clock::now();
    // per-image decision records reused across calls (their vectors keep their
    // capacity: no per-call allocation and release of ~1,500 small vectors)
    if (c->dec_scratch.size() < (size_t)n) c->dec_scratch.resize(n);
    if (c->hsum_scratch.size() < (size_t)n) c->hsum_scratch.resize(n);
    std::vector<PaletteDecision>& dec = c->dec_scratch;
    std::vector<std::vector<double>>& hsum = c->hsum_scratch;   // fused: host part of the slot sums
    ok.assign(n, 1);
    fail_why.assign(n, std::string());
    int* h_ent = (int*)(hp + L.E_pin(n) + L.e_entries);
    int* h_ns = (int*)(hp + L.E_pin(n) + L.e_ns);
    uint8_t* hb = hp + (size_t)n * (L.a_bytes + L.c_bytes);   // the B records on the host
    // per image, independent: the decision, its device records and (fused) the
    // host part of the slot sums; on the host pool when the decisions are
    // costly (fine grids), then the batch-wide lists in image order
    auto decide_one = [&](int i) {
        const unsigned* hist = (const unsigned*)(hp + L.A(i) + L.a_hist);
        uint8_t* b = hb + (size_t)i * L.b_bytes;
        if (!decide_palette(gp, cls->gc, hist, n_hsv, cfg, &dec[i],
                            cls->near.empty() ? nullptr : cls->near.data())) {
            ok[i] = 0;
            GroupRule* r = (GroupRule*)(b + L.b_rules);     // no slot: pass 2 keeps nothing
            for (int g = 0; g < gp.tl; g++) r[g] = GroupRule{-1, 0, 0, 0, 0xFFFFFFFFu, 0u};
            return;
        }
        fill_b_record(L, dec[i], gp.tl, b);
        if (fused) {
            hsum[i].assign(4 * dec[i].parents.size(), 0.0);
            if (!fused_slot_sums(gp, dec[i], hist, (const double*)(hp + L.A(i) + L.a_gsum),
                                 (const unsigned*)(hp + L.A(i) + L.a_gcell), hsum[i].data(), &fail_why[i]))
                ok[i] = 0;
        }
    };
    HostPool* pool = host_pool();
    if (n >= 4 && gp.tl >= 200 && pool->size() > 0) pool->parallel_for(n, decide_one);
    else
        for (int i = 0; i < n; i++) decide_one(i);
    t_dec_only = Clock::now();
    for (int i = 0; i < n; i++) {
        h_ns[i] = 0;
        if (!ok[i]) {
            // the message, on this thread (decide_palette is deterministic)
            if (!fail_why[i].empty()) set_error(fail_why[i]);
            else {
                PaletteDecision d;
                (void)decide_palette(gp, cls->gc, (const unsigned*)(hp + L.A(i) + L.a_hist), n_hsv, cfg, &d);
            }
            continue;
        }
        for (int g : dec[i].search) {
            h_ent[2 * n_ent] = i;
            h_ent[2 * n_ent + 1] = g;
            n_ent++;
        }
        max_per_img = std::max(max_per_img, (int)dec[i].search.size());
        h_ns[i] = (int)dec[i].parents.size();
        max_slots = std::max(max_slots, h_ns[i]);
    }
    if (sa != s2) PHD_HIP(hipStreamWaitEvent(s2, ev_k1, 0));
    if (!launch_palette_tail(c, L, n, d_imgs, height, width, ds, gp, cls, nchunks, fused, dec.data(), ok.data(), n_ent,
                             max_slots, max_per_img, s2))
        return false;
    if ((any(&ImageOutputs::labels) || any(&ImageOutputs::box_pal)) && !label_maps()) return false;
    PHD_HIP(hipEventRecord(c->ev_tail, s2));
    return true;
}

// The label maps of the images that asked for one and have a decision, on the
// tail stream behind the palette's second pass (Kcut has filled the partial
// groups' cutoff and last pixel in the B records): one launch over the run
// where that pass is batched, else one launch per image.  ev_tail follows, so
// the call's last download -- which the call waits for -- is behind the maps.
//
// Box palettes: an image whose boxes are counted and that has no map of the
// caller's gets one in the context's scratch (kDevLabScratch: 2 * mh * mw bytes
// per such image of the run at 256-byte steps), written by the same launches;
// the counting launch and its one download (enqueue_box_job) follow them on
// the tail stream, so the counters are on the host when the call's last
// download is.
bool ReportRun::label_maps() {
    const int mh = ds > 1 ? height / ds : height, mw = ds > 1 ? width / ds : width;
    std::vector<uint16_t*> map(n, nullptr);
    const size_t one = al(sizeof(uint16_t) * (size_t)mh * mw);
    size_t scratch = 0;
    for (int i = 0; i < n; i++) {
        if (ok[i]) map[i] = o(i).labels;
        if (!map[i] && counts_boxes(i)) scratch += one;
    }
    if (scratch) {
        if (!c->dev[kDevLabScratch].ensure(scratch)) return false;
        uint8_t* p = c->dev[kDevLabScratch].as<uint8_t>();
        for (int i = 0; i < n; i++)
            if (!map[i] && counts_boxes(i)) {
                map[i] = (uint16_t*)p;
                p += one;
            }
    }
    std::vector<LabelDst> dst;
    bool aligned = true;
    for (int i = 0; i < n; i++) {
        if (!map[i]) continue;
        dst.push_back(LabelDst{map[i], i, 0});
        aligned = aligned && (reinterpret_cast<uintptr_t>(d_imgs[i]) & 3) == 0;
    }
    if (dst.empty()) return true;
    if (!label_launches(dst, aligned)) return false;
    BoxJob job;
    bp_off.assign(n, -1);
    for (int i = 0; i < n; i++) {
        if (!counts_boxes(i)) continue;
        bp_off[i] = job.counters;
        job.add_image(map[i], mh, mw, ds, (int)c->dec_scratch[i].parents.size(), img_crops[i]);
    }
    return job.recs.empty() || enqueue_box_job(c, job, s2);
}

bool ReportRun::label_launches(const std::vector<LabelDst>& dst, bool aligned) {
    if (palette_tail_batched(gp, ds, fused, max_slots)) {
        const size_t bytes = sizeof(LabelDst) * dst.size();
        if (!upload_table(c, dst.data(), bytes, bytes, s2)) return false;
        const int ps = c->prof.begin(kLabels, s2);
        PHD_HIP(launch_palette_labels_batch((const uint8_t* const*)(dw + L.P_dev(n)), aligned, height, width, gp,
                                            cls->fc, cls->d, c->d_k255,
                                            (const GroupRule*)(dw + L.B(n, 0) + L.b_rules), (long)L.b_bytes,
                                            c->staged[kStViews].d.as<const LabelDst>(), (int)dst.size(), s2));
        c->prof.end(ps, s2);
        return table_launched(c, s2);
    }
    for (const LabelDst& d : dst) {
        const int ps = c->prof.begin(kLabels, s2);
        PHD_HIP(launch_palette_labels(d_imgs[d.img], height, width, ds, gp,
                                      (const GroupRule*)(dw + L.B(n, d.img) + L.b_rules), c->d_k255, d.map, s2));
        c->prof.end(ps, s2);
    }
    return true;
}

// Image i's C record (bins, max partials, palette sums, sharpness) goes to
// the host once its column pass and the palette tail are done (on the tail
// stream, after the tail's kernels); the host assembles it while the later
// images' FFTs run.  Two streams per lane: two lanes fit HIP's default
// four hardware queues (round 5: five streams per lane needed
// GPU_MAX_HW_QUEUES=8 to keep unrelated work from sharing a queue)
bool ReportRun::downloads() {
    // the stream that finishes last downloads the last results after an event
    // of the other that is already complete (waiting on a pending event from
    // another stream costs ~30 us of idle GPU): a single image's palette tail
    // (decisions, Kcut, partial sums) ends after its FFTs, a batch's FFTs end
    // after the tail
    const bool tail_last = n == 1;
    const hipStream_t s_end = tail_last ? s2 : st;           // the last group's stream
    if (!tail_last) PHD_HIP(hipStreamWaitEvent(st, c->ev_tail, 0));
    else PHD_HIP(hipStreamWaitEvent(s2, c->ev_fft, 0));
    PHD_HIP(hipEventRecord(c->ev[3], s_end));
    bool sd_used = false;
    for (int i0 = 0; i0 < n; i0 = dl_last(i0) + 1) {
        const int i1 = dl_last(i0);
        const bool last = i1 == n - 1;
        const hipStream_t s_dl = last ? s_end : s2;
        if (!last) {
            PHD_HIP(hipStreamWaitEvent(s2, c->ev_img_fft[i1], 0));
            sd_used = true;
        }
        PHD_HIP(hipMemcpyAsync(hc() + (size_t)i0 * L.c_bytes, dw + L.C(n, i0), (size_t)(i1 - i0 + 1) * L.c_bytes,
                               hipMemcpyDeviceToHost, s_dl));
        PHD_HIP(hipEventRecord(c->ev_img_dl[i1], s_dl));
    }
    if (sd_used) {
        PHD_HIP(hipEventRecord(c->ev_dl_sd, s2));
        PHD_HIP(hipStreamWaitEvent(s_end, c->ev_dl_sd, 0));
    }
    PHD_HIP(hipEventRecord(c->ev[4], s_end));   // the host waits on it before returning
    t_dec = Clock::now();
    t_sync = t_dec;
    return true;
}

// Each download group's reports are assembled once its copy is done; a
// group of 8 or more (batched FFT groups of small images, ~10 us per
// report at 36/4/5) on the host pool.
bool ReportRun::assemble_groups() {
    std::vector<PaletteDecision>& dec = c->dec_scratch;
    std::vector<std::vector<double>>& hsum = c->hsum_scratch;
    std::vector<std::string>& asm_why = fail_why;             // the decisions' messages are set already
    auto assemble_one = [&](int i) {
        if (!ok[i]) return;
        asm_why[i].clear();
        const uint8_t* a = hp + L.A(i);
        const uint8_t* cc = hc() + (size_t)i * L.c_bytes;
        const unsigned long long* sums = (const unsigned long long*)(a + L.a_sums);
        const double* spart = (const double*)(a + L.a_spart);
        double s_acc = 0.0;
        for (int k = 0; k < nchunks; k++) s_acc += spart[k];
        const RGB_Statistics st_i = stats_from_sums(sums, (long)height * width);
        // pgm_normalize_fft's max (src/fft_processing.c:181-184) over the block partials
        const double* fpart = (const double*)(cc + L.c_fmax);
        double fmax = 0.0;
        for (int b = 0; b < fs.col_blocks; b++) fmax = fpart[b] > fmax ? fpart[b] : fmax;
        const double* pal = (const double*)(cc + L.c_pal);
        if (fused) {                                         // whole groups (host) + partial groups (device)
            for (size_t k = 0; k < hsum[i].size(); k++) hsum[i][k] += pal[k];
            pal = hsum[i].data();
        }
        out[i] = assemble(st_i, s_acc / (double)n_hsv, dec[i], pal, n_hsv, *tbl,
                          (const unsigned long long*)(cc + L.c_bins), fmax, cfg,
                          img_crops ? img_crops[i] : crops, (const double*)(cc + L.c_sharp), &asm_why[i]);
        if (out[i]) status[i] = 0;
    };
    HostPool* pool = host_pool();
    for (int i0 = 0; i0 < n; i0 = dl_last(i0) + 1) {
        const int i1 = dl_last(i0), m = i1 - i0 + 1;
        PHD_HIP(hipEventSynchronize(c->ev_img_dl[i1]));
        if (i1 == n - 1) t_sync = Clock::now();
        if (m >= 8 && pool->size() > 0) pool->parallel_for(m, [&](int k) { assemble_one(i0 + k); });
        else
            for (int i = i0; i <= i1; i++) assemble_one(i);
    }
    for (int i = 0; i < n; i++) {
        if (ok[i] && !out[i]) set_error(asm_why[i]);          // on this thread (thread-local message)
        failures += !out[i];
    }
    t_end = Clock::now();
    return true;
}

bool ReportRun::timings() {
    PHD_HIP(hipEventSynchronize(c->ev[4]));
    c->prof.collect();
    auto ms = [](Clock::time_point a, Clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    // device stages, then host: total, enqueue, decisions + pass-2 enqueue, assembly
    // (a per-image D2H + assembly pipeline was measured slower: extra stream
    // joins; the host pool assembles only groups of 8 or more, where its
    // wake-up latency is paid once per group)
    double tm[8] = {ms_between(c->ev[0], c->ev[1]), ms_between(c->ev[1], c->ev[2]),
                    ms_between(c->ev[2], c->ev[3]), ms_between(c->ev[0], c->ev[4]), ms(t_host0, t_end),
                    ms(t_host0, t_enq), ms(t_k1, t_dec), ms(t_sync, t_end)};
    record_timings(tm, 8);
    static const bool verbose = getenv("PHD_VERBOSE") != nullptr;
    if (verbose) {
        // END_TIMING's format (src/utilities.h:12-18), one line per stage of this
        // pipeline (the device stages are HIP-event spans of the whole batch)
        const char* names[8] = {"rgb2hsv + rgb statistics + hsv average + palette histogram (K1)",
                                "rgb2pgm + fft + blur profile (FFT rows + columns)",
                                "color palette (second pass after the FFTs)", "device total",
                                "full report (host wall clock)", "enqueue", "color palette decisions",
                                "compile full report"};
        for (int k = 0; k < 8; k++) printf("%s took %f seconds to execute \n", names[k], tm[k] / 1e3);
        printf("color palette decisions alone (%d images) took %f seconds to execute \n", n,
               ms(t_k1, t_dec_only) / 1e3);
        printf("palette tail and download enqueue took %f seconds to execute \n", ms(t_dec_only, t_dec) / 1e3);
        printf("palette tail: %d partial-group entries, at most %d per image\n", n_ent, max_per_img);
    }
    return true;
}

// The box palette structs of the reported images, from the counters the run's
// streams brought to kStBoxPal's pinned block (timings() has waited for them): n_slots
// for each, the counts where the image has boxes.  A failed image keeps
// {0, 0, NULL}.
bool ReportRun::box_palettes() {
    for (int i = 0; i < n; i++) {
        if (!o(i).box_pal || !out[i]) continue;
        const bool counted = counts_boxes(i) && !bp_off.empty() && bp_off[i] >= 0;
        if (!box_palette_fill(o(i).box_pal, counted ? img_crops[i]->N : 0, (int)c->dec_scratch[i].parents.size(),
                              counted ? c->staged[kStBoxPal].h.as<const uint32_t>() + bp_off[i] : nullptr))
            return false;
    }
    return true;
}

// The box statistics structs of the reported images, from the 64 bytes per box
// box_stat_job's download left in kStBoxStat's pinned block (timings() has waited for
// it).  A failed image and an image without boxes keep {0, NULL, NULL}.
bool ReportRun::box_statistics() {
    for (int i = 0; i < n; i++) {
        if (!out[i] || !sums_boxes(i) || bs_off.empty() || bs_off[i] < 0) continue;
        if (!box_stats_fill(o(i).box_stats, img_crops[i], box_stats_host(c) + (size_t)bs_off[i] * kBoxStatOut))
            return false;
    }
    return true;
}

}  // namespace

bool run_reports(Context* c, const uint8_t* const* d_imgs, int n, int height, int width,
                 const phd_config& cfg, const Crop_Boundaries* crops, Full_Report_Data** out, int* status,
                 hipStream_t stream, const Crop_Boundaries* const* img_crops, const ImageOutputs* outs) {
    ReportRun r(ReportArgs{c, d_imgs, n, height, width, cfg, crops, out, status, stream, img_crops, outs});
    return r.plan() && r.k1() && r.fft_chain() && r.palette_tail() && r.downloads() && r.assemble_groups() &&
           r.timings() && r.box_palettes() && r.box_statistics() && r.failures == 0;
}

bool run_palette_trace(Context* c, const uint8_t* d_img, int height, int width, const phd_config& cfg,
                       std::vector<unsigned>* hist, PaletteDecision* dec, std::vector<double>* dcounts) {
    std::string why;
    if (!validate_config(cfg, &why)) {
        set_error(why);
        return false;
    }
    const hipStream_t st = c->stream;
    const GridParams gp = make_grid(cfg);
    const GroupCenters gc = make_centers(gp);
    const int ds = cfg.downsample_rate > 1 ? cfg.downsample_rate : 1;
    const long n_hsv = hsv_count(height, width, ds);
    const int nchunks = (int)((n_hsv + kChunk - 1) / kChunk);
    const Layout L = make_layout(1, gp.tl, nchunks, 1, 0, 1);
    if (!c->dev[kDevWs].ensure(L.dev_total) || !c->pin.ensure(L.pin_total)) return false;
    uint8_t* dw = c->dev[kDevWs].as<uint8_t>();
    uint8_t* hp = c->pin.as<uint8_t>();
    PHD_HIP(hipMemsetAsync(dw, 0, L.a_bytes + L.c_bytes, st));
    const Context::Cls* cls = get_cls(c, gp);
    if (!cls) return false;
    if (!launch_k1(c, L, 1, &d_img, height, width, ds, gp, cls, nchunks, false, st)) return false;
    PHD_HIP(hipMemcpyAsync(hp, dw, L.a_bytes, hipMemcpyDeviceToHost, st));
    PHD_HIP(hipStreamSynchronize(st));
    hist->assign((const unsigned*)(hp + L.a_hist), (const unsigned*)(hp + L.a_hist) + gp.tl);
    if (!decide_palette(gp, gc, hist->data(), n_hsv, cfg, dec)) return false;
    // the production tail with a batch of one: the B record, the Kcut list, one upload
    fill_b_record(L, *dec, gp.tl, hp + L.B(1, 0));
    int* h_ent = (int*)(hp + L.E_pin(1) + L.e_entries);
    const int n_ent = (int)dec->search.size(), np = (int)dec->parents.size(), one = 1;
    for (int k = 0; k < n_ent; k++) {
        h_ent[2 * k] = 0;
        h_ent[2 * k + 1] = dec->search[k];
    }
    *(int*)(hp + L.E_pin(1) + L.e_ns) = np;
    if (!launch_palette_tail(c, L, 1, &d_img, height, width, ds, gp, cls, nchunks, false, dec, &one, n_ent,
                             std::max(1, np), n_ent, st))
        return false;
    std::vector<double> pal(4 * np);
    PHD_HIP(hipMemcpyAsync(pal.data(), dw + L.C(1, 0) + L.c_pal, sizeof(double) * 4 * np,
                           hipMemcpyDeviceToHost, st));
    PHD_HIP(hipStreamSynchronize(st));
    dcounts->resize(np);
    for (int k = 0; k < np; k++) (*dcounts)[k] = pal[4 * k + 3];
    return true;
}

}  // namespace phd
