// phd_inputs.cpp -- the input stage of the device batch entries: images given
// as byte-strided views (phd_image_view), typed views (phd_typed_view) or
// YCbCr views (phd_yuv_view) become packed RGB8 images (or fp64 planes) on the
// lane before the pipeline (run_reports, phd_report.cpp) sees them.  Here: the
// three report entries' shared front end, their groups' staging for the
// driver (run_device_batch, phd_entries.cpp), the launch tables' upload, and
// the three conversion-only entries.  Validation and records: phd_views.cpp,
// phd_yuv.cpp (no HIP); kernels: pack_views.hip, decode_views.hip, yuv_views.hip.
#include <cstring>

#include "phd_host.h"

using namespace phd;

namespace phd {

// ---- launch tables ------------------------------------------------------------
// `bytes` of a launch table go up on st from the context's pinned copy
// (kStViews).  The table of the context's last launch is still read
// until that launch is done (a caller's stream is not drained by the call
// that used it): ev_views, recorded by table_launched, is waited for first --
// here and nowhere else.  The pinned block to fill, or nullptr.
void* table_begin(Context* c, size_t bytes) {
    auto ready = [&]() {
        if (!c->ev_views) PHD_HIP(hipEventCreateWithFlags(&c->ev_views, hipEventDisableTiming));
        else PHD_HIP(hipEventSynchronize(c->ev_views));
        return c->staged[kStViews].reserve(bytes, bytes);
    };
    return ready() ? c->staged[kStViews].h.as() : nullptr;
}

bool table_upload(Context* c, size_t bytes, hipStream_t st) { return c->staged[kStViews].up(bytes, st); }

// The first `filled` bytes from `host`, the rest zero.
bool upload_table(Context* c, const void* host, size_t filled, size_t bytes, hipStream_t st) {
    uint8_t* h = (uint8_t*)table_begin(c, bytes);
    if (!h) return false;
    memcpy(h, host, filled);
    memset(h + filled, 0, bytes - filled);
    return table_upload(c, bytes, st);
}

// After the last operation on st that uses the table.
bool table_launched(Context* c, hipStream_t st) {
    PHD_HIP(hipEventRecord(c->ev_views, st));
    return true;
}

}  // namespace phd

namespace {

// (grid.y = view: at most this many views a launch)
constexpr int kMaxViewsPerLaunch = 32768;

// The launches of a non-empty table of records on st, in chunks of
// kMaxViewsPerLaunch: launch(device records, first record's number, count,
// max_bands).  `extra` zeroed bytes follow the records at the next 256-byte
// step, *o_extra bytes into the kStViews pair.
template <class Rec, class Launch>
bool launch_views(Context* c, const std::vector<Rec>& recs, size_t extra, size_t* o_extra, hipStream_t st,
                  Launch launch) {
    int max_bands = 0;
    for (const Rec& r : recs) max_bands = std::max(max_bands, (r.height + r.band_rows - 1) / r.band_rows);
    const size_t filled = sizeof(Rec) * recs.size();
    if (extra) *o_extra = al(filled);
    if (!upload_table(c, recs.data(), filled, extra ? al(filled) + extra : filled, st)) return false;
    for (size_t k = 0; k < recs.size(); k += kMaxViewsPerLaunch) {
        const int m = (int)std::min<size_t>(kMaxViewsPerLaunch, recs.size() - k);
        PHD_HIP(launch(c->staged[kStViews].d.as<const Rec>() + k, k, m, max_bands));
    }
    return true;
}

// The pack launch of a call's views on st (pack_views.hip): view i goes to
// dst[i] (3 * height * width bytes; nullptr: the view is left out, as a packed
// one read in place).  views: validated (view_why).
bool enqueue_pack_views(Context* c, const phd_image_view* views, uint8_t* const* dst, int n, hipStream_t st) {
    std::vector<PackRec> recs;
    recs.reserve(n);
    for (int i = 0; i < n; i++)
        if (dst[i]) recs.push_back(pack_record(views[i], dst[i]));
    if (recs.empty()) return true;
    return launch_views(c, recs, 0, nullptr, st, [&](const PackRec* d, size_t, int m, int bands) {
        return launch_pack_views(d, m, bands, st, &c->prof);
    }) && table_launched(c, st);
}

// The conversion launch of a call's YUV views on st (yuv_views.hip): view i
// goes to dst[i] (3 * height * width bytes).  views: validated (yuv_view_why).
bool enqueue_yuv_views(Context* c, const phd_yuv_view* views, uint8_t* const* dst, int n, hipStream_t st) {
    if (n <= 0) return true;
    std::vector<YuvRec> recs(n);
    for (int i = 0; i < n; i++) recs[i] = yuv_record(views[i], dst[i]);
    return launch_views(c, recs, 0, nullptr, st, [&](const YuvRec* d, size_t, int m, int bands) {
        return launch_yuv_views(d, m, bands, st, &c->prof);
    }) && table_launched(c, st);
}

// the snap tables' device copy (uploaded once per context)
const uint8_t* device_snap(Context* c) {
    if (c->d_snap) return c->d_snap;
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, kSnapBytes) != hipSuccess ||
        hipMemcpy(d, snap_tables(), kSnapBytes, hipMemcpyHostToDevice) != hipSuccess) {
        if (d) (void)hipFree(d);
        set_error("snap table upload failed");
        return nullptr;
    }
    return c->d_snap = d;
}

// The classify launch of a group's typed views on st (decode_views.hip): view
// i's packed RGB8 image goes to dst[i] (3 * height * width bytes), its flag
// word (kDecNotU8 | kDecNonFinite, decode_view.h) to flags[i] on the host.  The
// flag words (zero) follow the records in the table; returns with the flags
// read back (st drained).  views: validated (typed_view_why).
bool classify_views(Context* c, const phd_typed_view* views, uint8_t* const* dst, int n, hipStream_t st, int* flags) {
    if (n <= 0) return true;
    const uint8_t* snap = device_snap(c);
    if (!snap) return false;
    std::vector<DecodeRec> recs(n);
    for (int i = 0; i < n; i++) recs[i] = decode_record(views[i], nullptr, dst[i], snap);
    const size_t fbytes = sizeof(int) * (size_t)n;
    size_t o_flags = 0;
    Staged& S = c->staged[kStViews];
    if (!launch_views(c, recs, fbytes, &o_flags, st, [&](const DecodeRec* d, size_t k, int m, int bands) {
            return launch_classify_views(d, (int*)(S.d.as<uint8_t>() + o_flags) + k, m, bands, st, &c->prof);
        }))
        return false;
    if (!S.down(o_flags, fbytes, st, o_flags) || !table_launched(c, st)) return false;
    PHD_HIP(hipStreamSynchronize(st));
    memcpy(flags, S.h.as<uint8_t>() + o_flags, fbytes);
    return true;
}

// The decode launch of one validated view into planes (3 * height * width doubles) on st.
bool enqueue_decode_view(Context* c, const phd_typed_view& view, double* planes, hipStream_t st) {
    PHD_HIP(launch_decode_view(decode_record(view, planes, nullptr, nullptr), st, &c->prof));
    return true;
}

// ---- a group's staging on its lane ----------------------------------------------
bool is_packed(const phd_image_view& v) {
    return pack_kind(v.width, v.row_stride, v.pixel_stride, v.channel_stride) == kPackPacked;
}

// The lane's staging images of a same-size group (256-byte steps, K1's aligned
// form): (*slots)[k] for every image with needs(k), nullptr for the others.
// The reference's size checks come first: a size it rejects is neither read
// nor allocated for (named >= 0: the message then names that image of the
// call); size_ok() runs between the check and the allocation.  run_reports
// returns with its results on the host, so the staging images are free for the
// lane's next group.
template <class Needs, class SizeOk>
bool stage_slots(Context* cl, int height, int width, int gm, Needs needs, int named, SizeOk size_ok,
                 std::vector<uint8_t*>* slots) {
    if (!precheck(height, width)) {
        if (named >= 0) set_error("image " + std::to_string(named) + ": " + phd_last_error());
        return false;
    }
    size_ok();
    const size_t step = (3 * (size_t)height * width + 255) & ~(size_t)255;
    size_t staged = 0;
    for (int k = 0; k < gm; k++) staged += needs(k);
    // (every allocation before the first launch that writes into it)
    if (staged && !cl->dev[kDevVstage].ensure(staged * step)) return false;
    slots->assign(gm, nullptr);
    size_t slot = 0;
    for (int k = 0; k < gm; k++)
        if (needs(k)) (*slots)[k] = cl->dev[kDevVstage].as<uint8_t>() + slot++ * step;
    return true;
}

template <class View>
const View& source(const std::vector<BatchImage>& imgs, int i) {
    return *(const View*)imgs[i].src;
}

// A group of views or of YUV views: a packed view is read in place, every
// other one gathered (converted) into its staging image by one launch on the
// call's stream, then one run_reports call.
void run_staged_group(Context* cl, const std::vector<BatchImage>& imgs, const std::vector<int>& grp, bool boxes,
                      const phd_config& cfg, void* stream, RunResults* r) {
    const int gm = (int)grp.size(), height = imgs[grp[0]].height, width = imgs[grp[0]].width;
    const bool yuv = imgs[grp[0]].kind == BatchImage::kYuv;
    std::vector<uint8_t*> dst;
    if (!stage_slots(cl, height, width, gm,
                     [&](int k) { return yuv || !is_packed(source<phd_image_view>(imgs, grp[k])); }, -1, [] {}, &dst))
        return;
    const hipStream_t st = work_stream(cl, stream);
    std::vector<const uint8_t*> ptrs(dst.begin(), dst.end());
    std::vector<int> ks(gm);
    for (int k = 0; k < gm; k++) ks[k] = k;
    bool ok;
    if (yuv) {
        std::vector<phd_yuv_view> gv(gm);
        for (int k = 0; k < gm; k++) gv[k] = source<phd_yuv_view>(imgs, grp[k]);
        ok = enqueue_yuv_views(cl, gv.data(), dst.data(), gm, st);
    } else {
        std::vector<phd_image_view> gv(gm);
        for (int k = 0; k < gm; k++) {
            gv[k] = source<phd_image_view>(imgs, grp[k]);
            if (!dst[k]) ptrs[k] = gv[k].data;
        }
        ok = enqueue_pack_views(cl, gv.data(), dst.data(), gm, st);
    }
    if (ok) report_group(cl, imgs, grp, ks, ptrs.data(), boxes, cfg, stream, r);
}

// A group of typed views.  The classifier writes every non-U8 view's RGB8
// image into the lane's staging area and says which are 8-bit; those, with the
// U8 views (gathered by the pack launch unless packed), are one run_reports
// call; each other finite image is decoded into the lane's double planes and
// reported by the fp64 planar pipeline (phd_planar.cpp), one at a time.
void run_typed_group(Context* cl, const std::vector<BatchImage>& imgs, const std::vector<int>& grp, bool boxes,
                     const phd_config& cfg, void* stream, RunResults* r) {
    const int gm = (int)grp.size(), height = imgs[grp[0]].height, width = imgs[grp[0]].width;
    auto tv = [&](int k) -> const phd_typed_view& { return source<phd_typed_view>(imgs, grp[k]); };
    std::vector<phd_image_view> gv(gm);
    std::vector<char> u8(gm);
    for (int k = 0; k < gm; k++) {
        gv[k] = typed_as_u8_view(tv(k));
        u8[k] = typed_is_u8_view(tv(k));
    }
    std::vector<uint8_t*> slots;
    hipStream_t st = nullptr;                                 // (taken before the staging grows, as ever)
    if (!stage_slots(cl, height, width, gm, [&](int k) { return !u8[k] || !is_packed(gv[k]); },
                     imgs[grp[gm - 1]].index, [&] { st = work_stream(cl, stream); }, &slots))
        return;
    std::vector<const uint8_t*> ptrs(gm);
    std::vector<uint8_t*> pack_dst(gm, nullptr), cls_dst;
    std::vector<phd_typed_view> cls_views;
    std::vector<int> cls_k;                                   // the group's classified images
    for (int k = 0; k < gm; k++) {
        ptrs[k] = slots[k] ? slots[k] : gv[k].data;
        if (u8[k]) pack_dst[k] = slots[k];
        else {
            cls_k.push_back(k);
            cls_dst.push_back(slots[k]);
            cls_views.push_back(tv(k));
        }
    }
    std::vector<int> flags(cls_k.size(), 0);
    if (!classify_views(cl, cls_views.data(), cls_dst.data(), (int)cls_k.size(), st, flags.data())) return;
    if (!enqueue_pack_views(cl, gv.data(), pack_dst.data(), gm, st)) return;
    std::vector<int> route(gm, 0);                            // 0: RGB8 run, else the classifier's flags
    for (size_t q = 0; q < cls_k.size(); q++) route[cls_k[q]] = flags[q];
    // the RGB8 run
    std::vector<int> run_k;
    for (int k = 0; k < gm; k++)
        if (!route[k]) run_k.push_back(k);
    report_group(cl, imgs, grp, run_k, ptrs.data(), boxes, cfg, stream, r);
    // the fp64 images, one at a time; a failing image keeps its message (the last one stays)
    const size_t n = (size_t)height * width;
    std::string bad, why;
    for (int k = 0; k < gm; k++) {
        if (!route[k]) continue;
        const std::string name = "image " + std::to_string(imgs[grp[k]].index) + ": ";
        if (route[k] & kDecNonFinite) {
            bad = name + "Error: channel values must be finite (NaN or infinity in the image).";
            continue;
        }
        if (!validate_config(cfg, &why)) {
            bad = name + why;
            continue;
        }
        // (the stream is idle: the planes may move)
        if (!cl->dev[kDevPlanes].ensure(sizeof(double) * 4 * n)) {
            bad = name + phd_last_error();
            continue;
        }
        double* dp = cl->dev[kDevPlanes].as<double>();
        Full_Report_Data* o = nullptr;
        if (enqueue_decode_view(cl, tv(k), dp, st))
            o = report_planes_device(cl, PlanarSrc{dp, dp + n, dp + 2 * n}, height, width, cfg,
                                     boxes ? imgs[grp[k]].boxes : nullptr, st, imgs[grp[k]].outs);
        (void)hipStreamSynchronize(st);
        cl->prof.collect();
        if (o) {
            r->o[k] = o;
            r->st[k] = 0;
        } else bad = name + phd_last_error();
    }
    if (!bad.empty()) set_error(bad);
}

// ---- the entries ------------------------------------------------------------------
// A report entry over descriptors (the input of get_full_report_data,
// src/interface.c:20-94, as GPU producers hold it): the mixed call over the
// images whose descriptor (view_ok) and boxes are valid, a single size group
// split as a same-size batch.  A bad view or bad boxes fail their image alone
// (the last message stays).  outs: what the call returns per image beside the
// report (CallOutputs, phd_host.h) -- an 8-bit image's from its run
// (ReportRun), an fp64 image's from report_planes_device.
template <class View, class Why>
int report_views(const char* family, BatchImage::Source kind, GroupFn run_group, const View* views, int n_images,
                 const phd_config* cfg, const Crop_Boundaries* const* crops, const CallOutputs& outs,
                 Full_Report_Data** out, int* status, void* stream, Why view_ok) {
    if (!report_prologue(entry_name(family, "", outs), views && cfg && out && status && n_images > 0, n_images, cfg,
                         outs))
        return -1;
    std::vector<BatchImage> imgs;
    std::string bad;
    for (int i = 0; i < n_images; i++) {
        out[i] = nullptr;
        status[i] = -1;
        std::string why;
        if (view_ok(views[i], &why) && (!crops || crops_why(crops[i], views[i].height, views[i].width, &why)))
            imgs.push_back({i, kind, &views[i], views[i].height, views[i].width, crops ? crops[i] : nullptr,
                            outs.of(i)});
        else bad = "image " + std::to_string(i) + ": " + why;
    }
    Context* c = get_context();
    if (!c) return -1;
    if (!bad.empty()) set_error(bad);
    auto groups = mixed_groups(imgs);
    split_for_lanes(&groups, stream);
    return run_device_batch(c, imgs, groups, run_group, crops != nullptr, *cfg, out, status, n_images, stream);
}

// A conversion-only entry: every descriptor and destination checked, then
// enqueue(context, stream) on the call's stream; the library's own stream is
// drained before the call returns.
template <class View, class Dst, class Why, class Enqueue>
int convert_views(const char* entry, const View* views, int n_images, Dst* const* d_dst, void* stream, Why view_ok,
                  Enqueue enqueue) {
    clear_error();
    if (!views || !d_dst || n_images <= 0) {
        set_error(std::string(entry) + ": bad arguments");
        return -1;
    }
    for (int i = 0; i < n_images; i++) {
        std::string why;
        if (!d_dst[i]) why = "destination is NULL";
        if (!why.empty() || !view_ok(views[i], &why)) {
            set_error("image " + std::to_string(i) + ": " + why);
            return -1;
        }
    }
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const hipStream_t st = work_stream(c, stream);
    if (!enqueue(c, st)) return -1;
    if (!stream) {
        const hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            set_error(std::string(entry) + ": " + hipGetErrorString(e));
            return -1;
        }
        c->prof.collect();
    }
    return 0;
}

// The three families' bodies: every report entry below is one call of its own.
int report_image_views(const phd_image_view* views, int n, const phd_config* cfg, const Crop_Boundaries* const* crops,
                       const CallOutputs& outs, Full_Report_Data** out, int* status, void* stream) {
    return report_views("views", BatchImage::kView, run_staged_group, views, n, cfg, crops, outs, out, status, stream,
                        view_why);
}

int report_yuv_views(const phd_yuv_view* views, int n, const phd_config* cfg, const Crop_Boundaries* const* crops,
                     const CallOutputs& outs, Full_Report_Data** out, int* status, void* stream) {
    return report_views("yuv", BatchImage::kYuv, run_staged_group, views, n, cfg, crops, outs, out, status, stream,
                        yuv_view_why);
}

int report_typed_views(const phd_typed_view* views, int n, const phd_config* cfg, const Crop_Boundaries* const* crops,
                       const CallOutputs& outs, Full_Report_Data** out, int* status, void* stream) {
    return report_views("typed_views", BatchImage::kTyped, run_typed_group, views, n, cfg, crops, outs, out, status,
                        stream, typed_view_why);
}

}  // namespace

// Each family has four report entries: the plain one, and with each image's
// palette label map (_labels), its box palette too (_box_palettes: per crop
// box, the elements of every palette slot) and its box statistics too
// (_box_stats: per crop box, get_rgb_statistics and get_hsv_average of its
// pixels).  An output passed as NULL is one the entry does not take.
//
// Device images as byte-strided views, in the layouts GPU producers emit (pack_view.h).
extern "C" int phd_report_batch_device_views(const phd_image_view* views, int n_images, const phd_config* cfg,
                                             const Crop_Boundaries* const* crops, Full_Report_Data** out,
                                             int* status, void* stream) {
    return report_image_views(views, n_images, cfg, crops, {}, out, status, stream);
}

extern "C" int phd_report_batch_device_views_labels(const phd_image_view* views, int n_images, const phd_config* cfg,
                                                    const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                                    Full_Report_Data** out, int* status, void* stream) {
    return report_image_views(views, n_images, cfg, crops, {d_labels}, out, status, stream);
}

extern "C" int phd_report_batch_device_views_box_palettes(const phd_image_view* views, int n_images,
                                                          const phd_config* cfg, const Crop_Boundaries* const* crops,
                                                          uint16_t* const* d_labels, phd_box_palette* box_palettes,
                                                          Full_Report_Data** out, int* status, void* stream) {
    return report_image_views(views, n_images, cfg, crops, {d_labels, box_palettes}, out, status, stream);
}

extern "C" int phd_report_batch_device_views_box_stats(const phd_image_view* views, int n_images,
                                                       const phd_config* cfg, const Crop_Boundaries* const* crops,
                                                       uint16_t* const* d_labels, phd_box_palette* box_palettes,
                                                       phd_box_stats* box_stats, Full_Report_Data** out, int* status,
                                                       void* stream) {
    return report_image_views(views, n_images, cfg, crops, {d_labels, box_palettes, box_stats}, out, status, stream);
}

extern "C" int phd_pack_views_device(const phd_image_view* views, int n_images, uint8_t* const* d_dst, void* stream) {
    return convert_views("phd_pack_views_device", views, n_images, d_dst, stream, view_why,
                         [&](Context* c, hipStream_t st) { return enqueue_pack_views(c, views, d_dst, n_images, st); });
}

// Device YCbCr frames as decoders emit them (yuv_view.h).
extern "C" int phd_report_batch_device_yuv(const phd_yuv_view* views, int n_images, const phd_config* cfg,
                                           const Crop_Boundaries* const* crops, Full_Report_Data** out, int* status,
                                           void* stream) {
    return report_yuv_views(views, n_images, cfg, crops, {}, out, status, stream);
}

extern "C" int phd_report_batch_device_yuv_labels(const phd_yuv_view* views, int n_images, const phd_config* cfg,
                                                  const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                                  Full_Report_Data** out, int* status, void* stream) {
    return report_yuv_views(views, n_images, cfg, crops, {d_labels}, out, status, stream);
}

extern "C" int phd_report_batch_device_yuv_box_palettes(const phd_yuv_view* views, int n_images, const phd_config* cfg,
                                                        const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                                        phd_box_palette* box_palettes, Full_Report_Data** out,
                                                        int* status, void* stream) {
    return report_yuv_views(views, n_images, cfg, crops, {d_labels, box_palettes}, out, status, stream);
}

extern "C" int phd_report_batch_device_yuv_box_stats(const phd_yuv_view* views, int n_images, const phd_config* cfg,
                                                     const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                                     phd_box_palette* box_palettes, phd_box_stats* box_stats,
                                                     Full_Report_Data** out, int* status, void* stream) {
    return report_yuv_views(views, n_images, cfg, crops, {d_labels, box_palettes, box_stats}, out, status, stream);
}

extern "C" int phd_convert_yuv_device(const phd_yuv_view* views, int n_images, uint8_t* const* d_dst, void* stream) {
    return convert_views("phd_convert_yuv_device", views, n_images, d_dst, stream, yuv_view_why,
                         [&](Context* c, hipStream_t st) { return enqueue_yuv_views(c, views, d_dst, n_images, st); });
}

// Device images of any element type, as the reference's Pixels (src/types.h:5).
extern "C" int phd_report_batch_device_typed_views(const phd_typed_view* views, int n_images, const phd_config* cfg,
                                                   const Crop_Boundaries* const* crops, Full_Report_Data** out,
                                                   int* status, void* stream) {
    return report_typed_views(views, n_images, cfg, crops, {}, out, status, stream);
}

extern "C" int phd_report_batch_device_typed_views_labels(const phd_typed_view* views, int n_images,
                                                          const phd_config* cfg, const Crop_Boundaries* const* crops,
                                                          uint16_t* const* d_labels, Full_Report_Data** out,
                                                          int* status, void* stream) {
    return report_typed_views(views, n_images, cfg, crops, {d_labels}, out, status, stream);
}

extern "C" int phd_report_batch_device_typed_views_box_palettes(const phd_typed_view* views, int n_images,
                                                                const phd_config* cfg,
                                                                const Crop_Boundaries* const* crops,
                                                                uint16_t* const* d_labels,
                                                                phd_box_palette* box_palettes, Full_Report_Data** out,
                                                                int* status, void* stream) {
    return report_typed_views(views, n_images, cfg, crops, {d_labels, box_palettes}, out, status, stream);
}

extern "C" int phd_report_batch_device_typed_views_box_stats(const phd_typed_view* views, int n_images,
                                                             const phd_config* cfg,
                                                             const Crop_Boundaries* const* crops,
                                                             uint16_t* const* d_labels, phd_box_palette* box_palettes,
                                                             phd_box_stats* box_stats, Full_Report_Data** out,
                                                             int* status, void* stream) {
    return report_typed_views(views, n_images, cfg, crops, {d_labels, box_palettes, box_stats}, out, status, stream);
}

// (one decode launch per image)
extern "C" int phd_decode_views_device(const phd_typed_view* views, int n_images, double* const* d_planes,
                                       void* stream) {
    return convert_views("phd_decode_views_device", views, n_images, d_planes, stream, typed_view_why,
                         [&](Context* c, hipStream_t st) {
                             for (int i = 0; i < n_images; i++)
                                 if (!enqueue_decode_view(c, views[i], d_planes[i], st)) return false;
                             return true;
                         });
}
