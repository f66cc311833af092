// phd_planar.cpp -- get_full_report_data (src/interface.c:20-94) on the
// caller's three planes of doubles.
//
// The planes go to the device once.  k_planar_to_u8 tests whether every value
// is exactly k/255.0 (what the reference's Python binding produces,
// utils.py:30-46) and writes the RGB8 image as it goes: then the RGB8
// pipeline (run_reports) computes the report, its arithmetic on those doubles
// being the reference's.  Otherwise the fp64 planar kernels (planar.hip) run
// the reference's arithmetic on the doubles themselves, with the generic FFT
// path (fft_global.hip) on the fp64 luma plane.  Values the reference cannot
// handle (non-finite, or a group index past the octree: values above 1 can
// index out of bounds in arm_octree, src/color_quantization.c:131-145) are
// rejected with NULL, like its other undefined cases.  Any other finite values
// (negative channels, luma outside [0, 1]) get a report: the polar bins'
// fixed-point scale follows the image's largest |pgm - avg| (bin_scale).
//
// report_planar is the upload and the 8-bit test; report_planes_device is the
// fp64 pipeline on planes that are on the device, which the typed views' entry
// (phd_inputs.cpp) also runs on the planes k_decode_view filled.
#include <cmath>
#include <cstring>

#include "phd_host.h"

namespace phd {

namespace {

// device / pinned-free host records of one planar call
struct PRec {
    size_t flags, avg, lrng, part1, part2, hist, spart, chunk, rules, search, off, pal, bins, fmax, sharp, total;
};

PRec prec_layout(int nb, int tl, int nchunks, int nbins, int ncolblocks, int ncrops) {
    PRec R{};
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += al(bytes);
        return at;
    };
    R.flags = take(sizeof(int));
    R.avg = take(sizeof(double));
    R.lrng = take(sizeof(double) * 2 * nb);
    R.part1 = take(sizeof(double) * 3 * nb);
    R.part2 = take(sizeof(double) * 3 * nb);
    R.hist = take(sizeof(unsigned) * tl);
    R.spart = take(sizeof(double) * nchunks);
    R.chunk = take(sizeof(unsigned short) * (size_t)nchunks * tl);
    R.rules = take(sizeof(GroupRule) * tl);
    R.search = take(sizeof(int) * tl);
    R.off = take(sizeof(double) * tl);
    R.pal = take(sizeof(double) * 4 * tl);
    R.bins = take(sizeof(unsigned long long) * nbins);
    R.fmax = take(sizeof(double) * std::max(1, ncolblocks));
    R.sharp = take(sizeof(double) * 2 * std::max(1, ncrops));
    R.total = o;
    return R;
}

#define PHD_HIPN(expr)                                                                  \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            set_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " + __FILE__ + ":" + \
                      std::to_string(__LINE__) + " (" #expr ")");                       \
            return nullptr;                                                             \
        }                                                                               \
    } while (0)

}  // namespace

Full_Report_Data* report_planar(Context* c, const double* r, const double* g, const double* b, int height,
                                int width, const phd_config& cfg, const Crop_Boundaries* crops) {
    std::string why;
    if (!validate_config(cfg, &why)) {
        set_error(why);
        return nullptr;
    }
    if (!precheck(height, width) || !check_crops(crops, height, width)) return nullptr;
    const long n = (long)height * width;
    const hipStream_t st = c->stream;
    if (!c->dev[kDevPlanes].ensure(sizeof(double) * 4 * (size_t)n) || !c->dev[kDevStage].ensure(3 * (size_t)n))
        return nullptr;
    double* dp = c->dev[kDevPlanes].as<double>();
    uint8_t* const d_stage = c->dev[kDevStage].as<uint8_t>();
    const PlanarSrc P{dp, dp + n, dp + 2 * n};
    if (!c->dev[kDevPrec].ensure(kAlign)) return nullptr;
    int* flags = c->dev[kDevPrec].as<int>();
    PHD_HIPN(hipMemsetAsync(flags, 0, sizeof(int), st));
    PHD_HIPN(hipMemcpyAsync((void*)P.r, r, sizeof(double) * n, hipMemcpyHostToDevice, st));
    PHD_HIPN(hipMemcpyAsync((void*)P.g, g, sizeof(double) * n, hipMemcpyHostToDevice, st));
    PHD_HIPN(hipMemcpyAsync((void*)P.b, b, sizeof(double) * n, hipMemcpyHostToDevice, st));
    PHD_HIPN(launch_planar_to_u8(P, n, d_stage, flags, st));
    int hflags = 0;
    PHD_HIPN(hipMemcpyAsync(&hflags, flags, sizeof(int), hipMemcpyDeviceToHost, st));
    PHD_HIPN(hipStreamSynchronize(st));
    if (!(hflags & 1)) {
        // an 8-bit image: the RGB8 pipeline, exactly the reference's arithmetic on these doubles
        const uint8_t* imgs[1] = {d_stage};
        Full_Report_Data* out = nullptr;
        int status = -1;
        run_reports(c, imgs, 1, height, width, cfg, crops, &out, &status, nullptr);
        (void)hipStreamSynchronize(c->stream);
        return out;
    }
    Full_Report_Data* out = report_planes_device(c, P, height, width, cfg, crops, st, ImageOutputs{});
    (void)hipStreamSynchronize(st);
    c->prof.collect();                                      // (k_planar_sums' events, when profiled)
    return out;
}

// Everything after the upload: the fp64 planar pipeline on planes that are on
// the device already -- P.r | P.g | P.b are the first 3 n doubles of
// kDevPlanes (4 n doubles), whose fourth plane takes the luma.  cfg, the size
// and the boxes are validated; nothing but the planes' own producer is queued
// on st (no buffer allocated here is in use).  outs (ImageOutputs, phd_host.h):
// the label map is written on st behind the palette tail.
Full_Report_Data* report_planes_device(Context* c, const PlanarSrc& P, int height, int width, const phd_config& cfg,
                                       const Crop_Boundaries* crops, hipStream_t st, const ImageOutputs& outs) {
    std::string why;
    uint16_t* labels = outs.labels;                          // (or a scratch map for the box counts)
    const long n = (long)height * width;
    double* pgm = c->dev[kDevPlanes].as<double>() + 3 * n;
    const int nb = planar_blocks(n);
    const GridParams gp = make_grid(cfg);
    const int ds = cfg.downsample_rate > 1 ? cfg.downsample_rate : 1;
    const long n_hsv = hsv_count(height, width, ds);
    const int nchunks = (int)((n_hsv + kChunk - 1) / kChunk);
    const int nbins = cfg.radius_partitions * cfg.angle_partitions, wf = width / 2 + 1;
    const int ncrops = crops ? crops->N : 0;
    // every allocation of the planar pipeline before its first launch (the stream is idle)
    FftSel fs;
    if (!select_generic(c, height, width, nbins, &fs)) return nullptr;
    const BlurTable* tbl = get_table(c, height, width, cfg.radius_partitions, cfg.angle_partitions);
    const Context::Cls* cls = get_cls(c, gp);
    if (!tbl || !cls) return nullptr;
    const PRec R = prec_layout(nb, gp.tl, nchunks, nbins, fs.col_blocks, ncrops);
    if (!c->dev[kDevPrec].ensure(R.total) ||
        !c->dev[kDevInter].ensure(sizeof(double2) * ((size_t)height * wf + 1024)))
        return nullptr;
    double2* const inter = c->dev[kDevInter].as<double2>();
    // box palettes: the boxes are counted from the caller's map, or from one in the context's scratch
    const bool count_boxes = outs.box_pal && ncrops > 0;
    const int mh = ds > 1 ? height / ds : height, mw = ds > 1 ? width / ds : width;
    if (count_boxes && !labels) {
        if (!c->dev[kDevLabScratch].ensure(sizeof(uint16_t) * (size_t)mh * mw)) return nullptr;
        labels = c->dev[kDevLabScratch].as<uint16_t>();
    }
    // box statistics: box_plan's bands as items; device: items | part1 | part2,
    // pinned: the items going up, then the two partial arrays coming down
    std::vector<PlanarBoxItem> bs_items;
    Staged& BS = c->staged[kStBoxStat];
    size_t bs_o1 = 0, bs_o2 = 0;
    if (outs.box_stats && ncrops > 0) {
        std::vector<BoxItem> bands;
        for (int k = 0; k < ncrops; k++) {
            const int first = (int)bands.size(), cols = crops->right[k] - crops->left[k];
            box_plan(k, crops->top[k], crops->bottom[k], cols, &bands);
            for (size_t q = first; q < bands.size(); q++)
                bs_items.push_back(PlanarBoxItem{crops->left[k], cols, bands[q].row0, bands[q].row1 - bands[q].row0,
                                                 first, (int)bands.size() - first,
                                                 (crops->bottom[k] - crops->top[k]) * cols, 0});
        }
        bs_o1 = al(sizeof(PlanarBoxItem) * bs_items.size());
        bs_o2 = bs_o1 + al(sizeof(double) * 4 * bs_items.size());
        if (!BS.reserve(bs_o2 + sizeof(double) * 3 * bs_items.size(),
                        std::max(sizeof(PlanarBoxItem), sizeof(double) * 7) * bs_items.size()))
            return nullptr;
    }
    uint8_t* dr = c->dev[kDevPrec].as<uint8_t>();
    int* flags = (int*)(dr + R.flags);
    PHD_HIPN(hipMemsetAsync(dr, 0, R.total, st));
    // ---- the fp64 planar pipeline -------------------------------------------------
    double* avg = (double*)(dr + R.avg);
    PHD_HIPN(launch_planar_stats(P, n, pgm, (double*)(dr + R.part1), (double*)(dr + R.part2), avg,
                                 (double*)(dr + R.lrng), flags, st));
    // |pgm - avg| <= max(max - avg, avg - min) bounds every spectrum element
    // (|X| <= N max|pgm - avg|): the polar bins' fixed-point scale
    std::vector<double> lr(2 * nb + 1);
    PHD_HIPN(hipMemcpyAsync(lr.data(), dr + R.avg, sizeof(double), hipMemcpyDeviceToHost, st));
    PHD_HIPN(hipMemcpyAsync(lr.data() + 1, dr + R.lrng, sizeof(double) * 2 * nb, hipMemcpyDeviceToHost, st));
    PHD_HIPN(hipStreamSynchronize(st));
    const double av = lr[0];
    double lrange = 0.0;                                   // (NaN propagates: a non-finite channel)
    for (int k = 0; k < nb; k++) {
        const double nlo = lr[1 + 2 * k], hi = lr[2 + 2 * k];   // -min, max of block k
        const double m = std::max(hi - av, av + nlo);
        lrange = (m != m || lrange != lrange) ? NAN : std::max(lrange, m);
    }
    if (!(lrange < 1e100) || av != av) {
        set_error(std::isfinite(lrange) && av == av ? "Error: channel values too large for a finite power spectrum."
                                                    : "Error: channel values must be finite (NaN or infinity in the "
                                                      "image).");
        return nullptr;
    }
    const double bscale = bin_scale(height, wf, lrange);
    PHD_HIPN(launch_planar_k1(P, height, width, ds, gp, (unsigned*)(dr + R.hist), (unsigned short*)(dr + R.chunk),
                              (double*)(dr + R.spart), flags, st));
    std::vector<uint8_t> h(R.total);
    // the records the host decides on: flags .. s_part
    PHD_HIPN(hipMemcpyAsync(h.data(), dr, R.chunk, hipMemcpyDeviceToHost, st));
    PHD_HIPN(hipEventRecord(c->ev[5], st));
    // the blur profile on the luma plane while the host decides
    unsigned long long* bins = (unsigned long long*)(dr + R.bins);
    double* fmx = (double*)(dr + R.fmax);
    PHD_HIPN(generic_rows(fs, nullptr, pgm, height, width, nullptr, avg, c->d_k255, inter, st));
    PHD_HIPN(generic_cols(fs, inter, height, wf, tbl->d_map, nbins, bins, fmx, st, bscale));
    if (ncrops) {
        // get_variance_sharpness runs on the luma before the DC removal (src/interface.c:70-73)
        std::vector<int> ca(4 * ncrops);
        for (int k = 0; k < ncrops; k++) {
            ca[k] = crops->top[k];
            ca[ncrops + k] = crops->bottom[k];
            ca[2 * ncrops + k] = crops->left[k];
            ca[3 * ncrops + k] = crops->right[k];
        }
        PHD_HIPN(launch_sharpness_src(nullptr, pgm, height, width, ncrops, ca.data(), ca.data() + ncrops,
                                      ca.data() + 2 * ncrops, ca.data() + 3 * ncrops, c->d_k255,
                                      (double*)(dr + R.sharp), st));
    }
    if (!bs_items.empty()) {
        // the two launches of the fp64 box statistics and their one download each,
        // behind the sharpness crops; the host finishes after the call's last wait
        uint8_t* db = BS.d.as<uint8_t>();
        const size_t ni = bs_items.size();
        memcpy(BS.h.as(), bs_items.data(), sizeof(PlanarBoxItem) * ni);
        if (!BS.up(sizeof(PlanarBoxItem) * ni, st)) return nullptr;
        const int ps = c->prof.begin(kPlanarBoxStats, st);
        PHD_HIPN(launch_planar_box_stats(P, width, (const PlanarBoxItem*)db, (int)ni, (double*)(db + bs_o1),
                                         (double*)(db + bs_o2), st));
        c->prof.end(ps, st);
        if (!BS.down(bs_o1, sizeof(double) * 4 * ni, st) ||
            !BS.down(bs_o2, sizeof(double) * 3 * ni, st, sizeof(double) * 4 * ni))
            return nullptr;
    }
    PHD_HIPN(hipEventSynchronize(c->ev[5]));
    const int hf = *(const int*)(h.data() + R.flags);
    if (hf & (2 | 4)) {
        (void)hipStreamSynchronize(st);
        set_error(hf & 2 ? "Error: channel values must be finite (NaN or infinity in the image)."
                         : "Error: channel values put pixels outside the octree (out-of-bounds group in "
                           "arm_octree).");
        return nullptr;
    }
    // get_rgb_statistics: the partials in the order the device summed them
    RGB_Statistics stt;
    double* so = &stt.Br;
    for (int ch = 0; ch < 3; ch++) {
        double a = 0.0;
        for (int k = 0; k < nb; k++) a += ((const double*)(h.data() + R.part1))[3 * k + ch];
        so[ch] = a / (double)n;
    }
    const unsigned* hist = (const unsigned*)(h.data() + R.hist);
    const double* spart = (const double*)(h.data() + R.spart);
    double s_acc = 0.0;
    for (int k = 0; k < nchunks; k++) s_acc += spart[k];
    PaletteDecision dec;
    if (!decide_palette(gp, cls->gc, hist, n_hsv, cfg, &dec, cls->near.empty() ? nullptr : cls->near.data())) {
        (void)hipStreamSynchronize(st);
        return nullptr;
    }
    PHD_HIPN(hipMemcpyAsync(dr + R.rules, dec.rules.data(), sizeof(GroupRule) * gp.tl, hipMemcpyHostToDevice, st));
    if (!dec.search.empty())
        PHD_HIPN(hipMemcpyAsync(dr + R.search, dec.search.data(), sizeof(int) * dec.search.size(),
                                hipMemcpyHostToDevice, st));
    if (!dec.off.empty())
        PHD_HIPN(hipMemcpyAsync(dr + R.off, dec.off.data(), sizeof(double) * dec.off.size(), hipMemcpyHostToDevice,
                                st));
    PHD_HIPN(launch_planar_tail(P, height, width, ds, gp, (const unsigned short*)(dr + R.chunk), nchunks,
                                (GroupRule*)(dr + R.rules), (const int*)(dr + R.search), (int)dec.search.size(),
                                (const double*)(dr + R.off), (int)dec.parents.size(), (double*)(dr + R.pal), st, &c->prof));
    if (labels) {
        // the parents' pixel lists (src/color_quantization.c:342-479): the tail has filled cutoff / last
        const int ps = c->prof.begin(kLabels, st);
        PHD_HIPN(launch_planar_labels(P, height, width, ds, gp, (const GroupRule*)(dr + R.rules), labels, st));
        c->prof.end(ps, st);
    }
    if (count_boxes) {
        // the same counting kernel as the 8-bit runs', behind k_planar_labels on this stream
        BoxJob job;
        job.add_image(labels, mh, mw, ds, (int)dec.parents.size(), crops);
        if (!enqueue_box_job(c, job, st)) return nullptr;
    }
    PHD_HIPN(hipMemcpyAsync(h.data() + R.part2, dr + R.part2, R.total - R.part2, hipMemcpyDeviceToHost, st));
    PHD_HIPN(hipStreamSynchronize(st));
    for (int ch = 0; ch < 3; ch++) {
        double a = 0.0;
        for (int k = 0; k < nb; k++) a += ((const double*)(h.data() + R.part2))[3 * k + ch];
        so[3 + ch] = std::sqrt(a / (double)n);
    }
    const double* fpart = (const double*)(h.data() + R.fmax);
    double fmax = 0.0;
    for (int k = 0; k < fs.col_blocks; k++) fmax = fpart[k] > fmax ? fpart[k] : fmax;
    Full_Report_Data* out = assemble(stt, s_acc / (double)n_hsv, dec, (const double*)(h.data() + R.pal), n_hsv, *tbl,
                                     (const unsigned long long*)(h.data() + R.bins), fmax, cfg, crops,
                                     (const double*)(h.data() + R.sharp), &why, bscale);
    if (!out) set_error(why);
    else if (outs.box_pal)
        (void)box_palette_fill(outs.box_pal, ncrops, (int)dec.parents.size(),
                               c->staged[kStBoxPal].h.as<const uint32_t>());
    if (out && !bs_items.empty() && box_stats_alloc(outs.box_stats, ncrops)) {
        // the items' partials in item order: B = sum / N as the device formed it,
        // C = sqrt(sum (x - B)^2 / N), S-bar = sum(s) / N
        const double* p1 = BS.h.as<const double>();
        const double* p2 = p1 + 4 * bs_items.size();
        int box = 0;
        for (size_t q = 0; q < bs_items.size(); q += bs_items[q].count, box++) {
            const PlanarBoxItem& it = bs_items[q];
            double a1[4] = {0.0, 0.0, 0.0, 0.0}, a2[3] = {0.0, 0.0, 0.0};
            for (int j = it.first; j < it.first + it.count; j++) {
                for (int ch = 0; ch < 4; ch++) a1[ch] += p1[4 * j + ch];
                for (int ch = 0; ch < 3; ch++) a2[ch] += p2[3 * j + ch];
            }
            const double nn = (double)it.npix;
            double* sb = &outs.box_stats->stats[box].Br;
            for (int ch = 0; ch < 3; ch++) {
                sb[ch] = a1[ch] / nn;
                sb[3 + ch] = std::sqrt(a2[ch] / nn);
            }
            outs.box_stats->average_saturation[box] = a1[3] / nn;
        }
    }
    return out;
}

}  // namespace phd
