// phd_blurwin.cpp -- window blur: per T x T window (T = 64 or 128) of a packed
// RGB8 image the reference's Blur_Profile and ten Blur_Vectors on that crop:
// crop_image (src/image_processing.c:244-266), avg of get_rgb_statistics
// (:543-553, src/interface.c:78), rgb2pgm + remove_dc_bias (:505-512,
// src/blur_profile.c:233-238), pgm_fft + pgm_normalize_fft
// (src/fft_processing.c:18-63, 173-213), cartesian_to_polar_conversion +
// calculate_blur_profile (src/blur_profile.c:427-458, 34-126) and
// vectorize_blur_profile (:324-416).
// phd_blur_windows_device (every window of every image of a call in one
// launch), phd_free_window_blur and the host twin phd_debug_window_blur_host.
// Blur vectors: phd_blur_vectors_device and phd_blur_vector_maps_device leave
// each window's ten vectors and its maximum in device memory, finished by the
// window's own block; their twin phd_debug_window_vectors_host and the finish
// alone, phd_debug_window_finish_host.
// The entries' windows -- checks, counts and the walk that fills recs and the
// vectors' table -- are a WindowPlan and the twins' checks window_twin_why
// (window_call.h); the vectors' launch goes through table_call (phd_host.h).
// Plan of a size, box rule, index maps and the finish's rows: blur_window.h;
// kernels: blur_windows.hip.

#include <cstring>

#include "phd_host.h"
#include "window_call.h"

using namespace phd;

namespace {

// The polar table of a T x (T/2+1) spectrum on the host, or why the grid has
// none: build_blur_table's two refusals.  One entry per (T, nr, na) asked for.
struct HostTable {
    BlurTable t;
    std::string why;     // empty: usable
};
const HostTable* host_window_table(int T, int nr, int na) {
    static std::mutex mu;
    static std::map<std::tuple<int, int, int>, std::unique_ptr<HostTable>> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto& e = cache[std::make_tuple(T, nr, na)];
    if (!e) {
        e.reset(new HostTable);
        if (!build_blur_table(T, T, nr, na, &e->t, false)) {
            e->why = phd_last_error();
            clear_error();
        }
    }
    return e.get();
}

// cfg, window and grid: what every entry checks first
bool window_grid_why(int window, const phd_config* cfg, std::string* why, const HostTable** tab) {
    if (!cfg) return *why = "NULL cfg", false;
    if (!win_size_ok(window)) return *why = "window must be 64 or 128, not " + std::to_string(window), false;
    if (!validate_config(*cfg, why)) return false;
    const long nbins = (long)cfg->angle_partitions * cfg->radius_partitions;
    if (nbins > kWinMaxBins)
        return *why = "angle_partitions * radius_partitions = " + std::to_string(nbins) + " exceeds " +
                      std::to_string(kWinMaxBins) + " bins",
               false;
    *tab = host_window_table(window, cfg->radius_partitions, cfg->angle_partitions);
    if (!(*tab)->why.empty()) return *why = "window " + std::to_string(window) + ": " + (*tab)->why, false;
    return true;
}

const phd_window_blur kNoWindows = {0, 0, 0, 0, 0, nullptr, nullptr, nullptr};

bool window_blur_alloc(phd_window_blur* wb, int n, const BlurTable& t) {
    *wb = kNoWindows;
    wb->num_angle_bins = t.na;
    wb->num_radius_bins = t.nr;
    wb->angle_bin_size = t.angle_bin_size;
    wb->radius_bin_size = t.radius_bin_size;
    if (n <= 0) return true;
    const size_t nbins = (size_t)t.na * t.nr;
    void* p = malloc(sizeof(double) * nbins * n + sizeof(double) * n + sizeof(Blur_Vector) * 10 * (size_t)n);
    if (!p) {
        set_error("window blur: out of memory");
        return false;
    }
    wb->n_windows = n;
    wb->bins = (double*)p;
    wb->fft_max = wb->bins + nbins * n;
    wb->vectors = (Blur_Vector*)(wb->fft_max + n);
    return true;
}

// Windows of one chunk: their bin sums and maxima fit kWindowBlurBudget bytes
// (the header's PHD_WINDOW_BLUR_BUDGET, on the device and pinned)
constexpr size_t kWindowBlurBudget = PHD_WINDOW_BLUR_BUDGET;

}  // namespace

extern "C" void phd_free_window_blur(phd_window_blur* wb, int n) {
    if (!wb) return;
    for (int i = 0; i < n; i++) {
        free(wb[i].bins);
        wb[i] = kNoWindows;
    }
}

extern "C" int phd_blur_windows_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                       int n_images, const Crop_Boundaries* const* windows, int window,
                                       const phd_config* cfg, phd_window_blur* out, void* stream) {
    clear_error();
    auto bad = [](const std::string& what) {
        set_error("phd_blur_windows_device: " + what);
        return -1;
    };
    if (out && n_images > 0)
        for (int i = 0; i < n_images; i++) out[i] = kNoWindows;
    WindowPlan plan(d_images, heights, widths, n_images, windows, true, window, 0);
    std::string why;
    const HostTable* ht = nullptr;
    if (!plan.args_why(out && cfg, &why) || !window_grid_why(window, cfg, &why, &ht) ||
        !plan.build(nullptr, nullptr, &why))                 // (results go to `out`: no destination array)
        return bad(why);
    const int T = window;
    const int na = cfg->angle_partitions, nr = cfg->radius_partitions, nbins = na * nr;
    if (plan.total == 0) {                                   // no window at all: nothing for the device
        for (int i = 0; i < n_images; i++) window_blur_alloc(&out[i], 0, ht->t);
        return 0;
    }
    for (int i = 0; i < n_images; i++)
        if (!window_blur_alloc(&out[i], (int)plan.count[i], ht->t)) {
            phd_free_window_blur(out, n_images);
            return -1;
        }
    // window w of the call: its record, and -> its image's arrays
    std::vector<WinRec> recs;
    std::vector<std::pair<int, int>> where;
    recs.reserve(plan.total);
    where.reserve(plan.total);
    plan.for_each([&](int i, long long k, long long top, long long left) {
        recs.push_back(WinRec{d_images[i] + 3LL * (top * widths[i] + left), 3LL * widths[i]});
        where.push_back({i, (int)k});
    });
    Context* c = get_context();
    if (!c) {
        phd_free_window_blur(out, n_images);
        return -1;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    const hipStream_t st = work_stream(c, stream);
    const size_t nw = recs.size(), per = sizeof(unsigned long long) * nbins + sizeof(double);
    const size_t chunk = std::min(nw, std::max<size_t>(1, kWindowBlurBudget / per));
    // device: twiddles | records | chunk bins | chunk maxima; pinned: the table going up, a chunk coming down
    const size_t o_recs = al(sizeof(double2) * T), up = o_recs + sizeof(WinRec) * nw;
    const size_t o_bins = al(up), o_fmax = o_bins + al(sizeof(unsigned long long) * nbins * chunk);
    const size_t total = o_fmax + al(sizeof(double) * chunk), down = o_fmax - o_bins + sizeof(double) * chunk;
    auto run = [&]() {
        const BlurTable* tbl = get_table(c, T, T, nr, na);
        if (!tbl) return false;
        Staged& S = c->staged[kStWinBlur];
        if (!S.reserve(total, std::max(up, down))) return false;
        uint8_t* h = S.h.as<uint8_t>();
        uint8_t* d = S.d.as<uint8_t>();
        memset(h, 0, o_recs);
        window_twiddles(T, (double2*)h);
        memcpy(h + o_recs, recs.data(), sizeof(WinRec) * nw);
        if (!S.up(up, st)) return false;
        HostPool* pool = host_pool();
        for (size_t w0 = 0; w0 < nw; w0 += chunk) {
            const int m = (int)std::min(chunk, nw - w0);
            const int ps = c->prof.begin(kWindowBlur, st);
            PHD_HIP(launch_window_blur(T, (const WinRec*)(d + o_recs) + w0, m, (const double2*)d, tbl->d_map, nbins,
                                       (unsigned long long*)(d + o_bins), (double*)(d + o_fmax), st));
            c->prof.end(ps, st);
            if (!S.down(o_bins, down, st)) return false;
            PHD_HIP(hipStreamSynchronize(st));               // the result is on the host: waited for on any stream
            const unsigned long long* hb = (const unsigned long long*)h;
            const double* hf = (const double*)(h + (o_fmax - o_bins));
            auto finish = [&](int j) {
                const std::pair<int, int> at = where[w0 + j];
                phd_window_blur& o = out[at.first];
                o.fft_max[at.second] = hf[j];
                finish_blur(*tbl, hb + (size_t)j * nbins, hf[j], *cfg, o.bins + (size_t)at.second * nbins,
                            o.vectors + (size_t)at.second * 10);
            };
            if (pool->size() > 0 && m >= 64) pool->parallel_for(m, finish);
            else
                for (int j = 0; j < m; j++) finish(j);
        }
        c->prof.collect();
        return true;
    };
    if (!run()) {
        phd_free_window_blur(out, n_images);
        return -1;
    }
    return 0;
}

// ---- blur vectors: the finish in the window's own block ---------------------------
namespace {

static_assert(sizeof(WinVector) == sizeof(Blur_Vector) && offsetof(WinVector, angle) == offsetof(Blur_Vector, angle) &&
                  offsetof(WinVector, magnitude) == offsetof(Blur_Vector, magnitude),
              "WinVector is Blur_Vector");

// The rows of the shared finish (blur_window.h) in sequence, one window: what
// k_window_vectors runs between barriers.  flat: na x nr or nullptr.
void window_finish_host(const BlurTable& t, const unsigned long long* sums, double fmax, int T, const phd_config& cfg,
                        double* flat, Blur_Vector* out) {
    const int na = cfg.angle_partitions, nr = cfg.radius_partitions, rc = nr / cfg.blur_cutoff_ratio_denom;
    const double scale = bin_scale(T, T / 2 + 1), gs = win_gs(fmax);
    std::vector<double> own, tot(na), sm(na);
    if (!flat) {
        own.resize((size_t)na * nr);
        flat = own.data();
    }
    for (int b = 0; b < na * nr; b++) flat[b] = win_flat_bin(sums[b], scale, gs, (unsigned)t.counts[b]);
    for (int i = 0; i < na; i++) tot[i] = win_angle_total(flat, nr, rc, i);
    const double avg = win_angle_avg(tot.data(), na);
    for (int i = 0; i < na; i++) sm[i] = win_smooth(tot.data(), na, i);
    int idx[kWinVectors];
    const int m = win_maxima(sm.data(), na, avg * cfg.fft_streak_thresh, idx);
    for (int k = 0; k < kWinVectors; k++) {
        WinVector v = {0, 0.0f};                             // calloc, src/blur_profile.c:297-302
        if (k < m) v = win_vector(flat, na, nr, rc, avg, cfg.magnitude_thresh, idx[k]);
        out[k] = Blur_Vector{v.angle, v.magnitude};
    }
}

// what the vector entries check on top of window_grid_why
bool vector_grid_why(int window, const phd_config* cfg, std::string* why, const HostTable** tab) {
    if (!window_grid_why(window, cfg, why, tab)) return false;
    if (cfg->angle_partitions < 2)
        return *why = "angle_partitions must be at least 2 (vectorize_blur_profile reads smooth[1] and "
                      "smooth[num_angle_bins - 2], src/blur_profile.c:360-374), not " +
                      std::to_string(cfg->angle_partitions),
               false;
    return true;
}

// Both vector entries: the plan of their windows (lists, or a regular grid per image).
int blur_vectors_call(const char* entry, WindowPlan plan, const phd_config* cfg, Blur_Vector* const* d_vectors,
                      double* const* d_fft_max, void* stream) {
    clear_error();
    std::string why;
    const HostTable* ht = nullptr;
    if (!plan.args_why(d_vectors && cfg, &why) || !vector_grid_why(plan.T, cfg, &why, &ht) ||
        !plan.build((const void* const*)d_vectors, "d_vectors", &why)) {
        set_error(std::string(entry) + ": " + why);
        return -1;
    }
    if (plan.total == 0) return 0;                           // no window at all: nothing for the device
    const int T = plan.T, na = cfg->angle_partitions, nr = cfg->radius_partitions, nbins = na * nr;
    const size_t nw = (size_t)plan.total;
    Context* c = get_context();
    if (!c) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    const BlurTable* tbl = get_table(c, T, T, nr, na);
    if (!tbl) return -1;
    // the call's table: twiddles | the bins' element counts (u16) | window records | their destinations
    const size_t o_counts = al(sizeof(double2) * T), o_recs = o_counts + al(sizeof(uint16_t) * nbins);
    const size_t o_dst = o_recs + al(sizeof(WinRec) * nw), bytes = o_dst + sizeof(WinDst) * nw;
    auto fill = [&](uint8_t* h) {
        memset(h, 0, o_recs);
        window_twiddles(T, (double2*)h);
        uint16_t* hc = (uint16_t*)(h + o_counts);
        for (int b = 0; b < nbins; b++) hc[b] = (uint16_t)tbl->counts[b];
        WinRec* recs = (WinRec*)(h + o_recs);
        WinDst* dst = (WinDst*)(h + o_dst);
        memset(h + o_recs + sizeof(WinRec) * nw, 0, o_dst - o_recs - sizeof(WinRec) * nw);
        size_t w = 0;
        plan.for_each([&](int i, long long k, long long top, long long left) {
            const long long pitch = 3LL * plan.widths[i];
            recs[w] = WinRec{plan.d_images[i] + top * pitch + 3 * left, pitch};
            dst[w++] = WinDst{(WinVector*)d_vectors[i] + kWinVectors * k,
                              d_fft_max && d_fft_max[i] ? d_fft_max[i] + k : nullptr};
        });
    };
    auto launch = [&](const uint8_t* d, hipStream_t st) {
        return launch_window_vectors(T, (const WinRec*)(d + o_recs), (const WinDst*)(d + o_dst), (int)nw,
                                     (const double2*)d, tbl->d_map, (const uint16_t*)(d + o_counts), na, nr,
                                     cfg->blur_cutoff_ratio_denom, cfg->fft_streak_thresh, cfg->magnitude_thresh, st);
    };
    return table_call(c, stream, bytes, fill, launch, kWindowVectors) ? 0 : -1;
}

}  // namespace

extern "C" int phd_blur_vectors_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                       int n_images, const Crop_Boundaries* const* windows, int window,
                                       const phd_config* cfg, Blur_Vector* const* d_vectors,
                                       double* const* d_fft_max, void* stream) {
    return blur_vectors_call("phd_blur_vectors_device",
                             WindowPlan(d_images, heights, widths, n_images, windows, true, window, 0), cfg,
                             d_vectors, d_fft_max, stream);
}

extern "C" int phd_blur_vector_maps_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                           int n_images, int window, int stride, const phd_config* cfg,
                                           Blur_Vector* const* d_vectors, double* const* d_fft_max, void* stream) {
    return blur_vectors_call("phd_blur_vector_maps_device",
                             WindowPlan(d_images, heights, widths, n_images, nullptr, false, window, stride), cfg,
                             d_vectors, d_fft_max, stream);
}

// k_window_vectors' twin: window_bins_host, then the shared finish.
extern "C" int phd_debug_window_vectors_host(const uint8_t* rgb, int height, int width,
                                             const Crop_Boundaries* windows, int window, const phd_config* cfg,
                                             Blur_Vector* vectors, double* fft_max) {
    clear_error();
    std::string why, grid_why;
    const HostTable* ht = nullptr;
    vector_grid_why(window, cfg, &grid_why, &ht);
    if (!window_twin_why(rgb, height, width, windows, window, grid_why, vectors && fft_max, "NULL vectors or fft_max",
                         &why)) {
        set_error("phd_debug_window_vectors_host: " + why);
        return -1;
    }
    if (!windows || windows->N == 0) return 0;
    const int nbins = cfg->angle_partitions * cfg->radius_partitions;
    std::vector<unsigned long long> sums(nbins);
    for (int k = 0; k < windows->N; k++) {
        window_bins_host(window, rgb + 3LL * ((long long)windows->top[k] * width + windows->left[k]), 3LL * width,
                         ht->t.map.data(), nbins, sums.data(), &fft_max[k]);
        window_finish_host(ht->t, sums.data(), fft_max[k], window, *cfg, nullptr, vectors + (size_t)k * 10);
    }
    return 0;
}

// The shared finish alone over caller-given bin sums of one window.
extern "C" int phd_debug_window_finish_host(const unsigned long long* bin_sums, double fft_max, int window,
                                            const phd_config* cfg, double* bins, Blur_Vector* vectors) {
    clear_error();
    std::string why;
    const HostTable* ht = nullptr;
    if (!bin_sums || !vectors) why = "NULL bin_sums or vectors";
    else vector_grid_why(window, cfg, &why, &ht);
    if (!why.empty()) {
        set_error("phd_debug_window_finish_host: " + why);
        return -1;
    }
    window_finish_host(ht->t, bin_sums, fft_max, window, *cfg, bins, vectors);
    return 0;
}

// The kernel's steps on the host (blur_windows.hip: window_bins_host), then the
// device call's own finish.
extern "C" int phd_debug_window_blur_host(const uint8_t* rgb, int height, int width, const Crop_Boundaries* windows,
                                          int window, const phd_config* cfg, double* bins, Blur_Vector* vectors,
                                          double* fft_max) {
    clear_error();
    std::string why, grid_why;
    const HostTable* ht = nullptr;
    window_grid_why(window, cfg, &grid_why, &ht);
    if (!window_twin_why(rgb, height, width, windows, window, grid_why, bins && vectors && fft_max,
                         "NULL bins, vectors or fft_max", &why)) {
        set_error("phd_debug_window_blur_host: " + why);
        return -1;
    }
    if (!windows || windows->N == 0) return 0;
    const int nbins = cfg->angle_partitions * cfg->radius_partitions;
    std::vector<unsigned long long> sums(nbins);
    for (int k = 0; k < windows->N; k++) {
        window_bins_host(window, rgb + 3LL * ((long long)windows->top[k] * width + windows->left[k]), 3LL * width,
                         ht->t.map.data(), nbins, sums.data(), &fft_max[k]);
        finish_blur(ht->t, sums.data(), fft_max[k], *cfg, bins + (size_t)k * nbins, vectors + (size_t)k * 10);
    }
    return 0;
}
