// phd_host.h -- host-side internals of libreport_data.so (C++17).
#pragma once

#include <atomic>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <tuple>
#include <vector>

#include <sys/types.h>

#include "../../include/photohive_dsp.h"
#include "phd_internal.h"
#include "batch_plan.h"
#include "grow_buf.h"
#include "box_tiles.h"
#include "box_stat_tiles.h"
#include "sharp_plan.h"
#include "views_plan.h"
#include "yuv_plan.h"

namespace phd {

// ---- errors ---------------------------------------------------------------
void set_error(const std::string& msg);   // thread-local, also printed to stderr
void clear_error();

#define PHD_HIP(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            ::phd::set_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " \
                             + __FILE__ + ":" + std::to_string(__LINE__) + " (" #expr ")"); \
            return false;                                                               \
        }                                                                               \
    } while (0)

// ---- validated configuration ----------------------------------------------
// Returns false (with phd_last_error) for configurations where the reference's
// behaviour is undefined (see DESIGN.md "Deliberate rejections").
bool validate_config(const phd_config& cfg, std::string* why);
GridParams make_grid(const phd_config& cfg);
// Group centres of initialize_octree (src/color_quantization.c:57-99).
struct GroupCenters {
    std::vector<double> h, s, v;
};
GroupCenters make_centers(const GridParams& gp);
// Exact classification tables for fast_group (phd_device.h).
void make_class_tables(const GridParams& gp, FastCls* fc, ClassTables* t);

// ---- palette decisions (host) ---------------------------------------------
struct PaletteDecision {
    std::vector<int> parents;            // valid_parents, palette order
    std::vector<GroupRule> rules;        // [TL]
    std::vector<long long> kept;         // pixels each parent keeps
    std::vector<double> off;             // 180 - h_centre(parent)
    std::vector<int> search;             // groups needing the device cutoff search
};
// For each group i, every group ordered by (node_distance(i, p), p): the
// nearest-parent search of group_irregular_pixels walks it to the first
// parent instead of measuring every parent.  tl * tl u16; empty above
// kNearMaxGroups groups (then the search measures every parent).
constexpr int kNearMaxGroups = 2048;
std::vector<uint16_t> make_near_order(const GridParams& gp, const GroupCenters& gc);
// find_valid_octree_parents + group_irregular_pixels as keep rules.  near:
// make_near_order's table or nullptr.
bool decide_palette(const GridParams& gp, const GroupCenters& gc, const unsigned* hist, long n_hsv,
                    const phd_config& cfg, PaletteDecision* out, const uint16_t* near = nullptr);

// ---- blur profile helpers (host) ------------------------------------------
struct BlurTable {
    int height = 0, wf = 0, nr = 0, na = 0;
    std::vector<long long> counts;       // [na*nr]
    std::vector<uint16_t> map;           // host [wf][height] (the column run lists are made from it)
    uint16_t* d_map = nullptr;           // device [wf][height]
    int angle_bin_size = 0, radius_bin_size = 0;
};
// The compile-time column pass's polar bins as runs (ColBins): along each
// column the bin id changes a few tens of times (~76 runs per column at
// 4000x3000, 72 x 40 bins), so a column is its list of runs -- u32 start row
// << 16 | bin id, then a sentinel whose start is the height -- and each of the
// kernel's T threads per column gets the index of the run holding its first
// row (rows [t E, t E + E), E = ceil(height / T)).  ~1.5 MB per size instead
// of the 12 MB u16 bin of every element.
struct ColRuns {
    int T = 0, stride = 0;               // threads per column; entries per column (runs + sentinel)
    uint32_t* d_runs = nullptr;          // device [wf][stride]
    uint32_t* d_seg = nullptr;           // device [wf][T]: run index | run-start rows << 8 (ColBins::seg)
    int max_entries = 0;                 // the longest column's runs + sentinel
    bool too_many = false;               // max_entries > kColRunsMax: runtime-plan FFT for this size
};
// false when a column needs more than kColRunsMax entries (too_many: that size
// then takes the runtime-plan FFT) or on an upload error (nothing allocated).
bool build_col_runs(const uint16_t* map, int height, int wf, int T, ColRuns* r);
// Exact (phi_bin, r_bin) of every spectrum element, glibc atan2 + newton_int_sqrt
// exactly as src/blur_profile.c:87-97 / 427-458.
// upload == false: host map and counts only (no device copy)
bool build_blur_table(int height, int width, int nr, int na, BlurTable* t, bool upload = true);
void vectorize_blur(const double* bins, int na, int nr, double streak, double mag, int denom,
                    Blur_Vector* out10);

// ---- FFT plans --------------------------------------------------------------
struct FftPlanHost {
    FftPlan plan{};
    double2* d_tw = nullptr;
};
// composite: radices up to 16 (the image passes' kernels, fft.hip); else 2, 3,
// 4, 5, 8 and generic (fft_global.hip, which runs them at up to 1024 threads)
bool make_fft_plan(int n, FftPlanHost* p, bool composite = false);

// A batched 1-D transform of length n over sequences in HBM (fft_global.hip):
// one LDS pass (direct), two (four-step n = n1 * n2) or Bluestein's
// convolution through a smooth length M >= 2n - 1.
struct GfftPlan {
    enum { kDirect = 0, kFourStep = 1, kBluestein = 2 };
    int n = 0, kind = kDirect;
    const FftPlanHost* p = nullptr;                    // direct
    const FftPlanHost *p1 = nullptr, *p2 = nullptr;    // four-step
    double2* d_twn = nullptr;                          // four-step: W_n^e, e < n
    int M = 0;                                         // Bluestein
    const struct GfftPlan* sub = nullptr;
    double2* d_chirp = nullptr;                        // c_j = exp(-pi i j^2 / n)
    double2* d_bhat = nullptr;                         // FFT_M(conj c, wrapped)
};
// A length the LDS transforms take in one pass (n <= 8192, prime factors <= kMaxDirectPrime).
bool gfft_direct_ok(int n);
size_t gfft_scratch_elems(const GfftPlan& p, long count);
// in -> out (in == out allowed), scratch of gfft_scratch_elems(p, count) elements
bool gfft_run(const GfftPlan& p, const double2* in, double2* out, long count, double2* scr, hipStream_t st);

// ---- per-kernel event timing (opt-in, phd_profile_kernels) -----------------
enum KernelId {
    kK1 = 0, kFftRows = 1, kFftCols = 2, kCutoffs = 3, kPalSums = 4, kSharp = 5, kPack = 6, kClassify = 7,
    kDecode = 8, kYuv = 9, kLabels = 10, kBoxPalettes = 11, kBoxStats = 12, kPlanarBoxStats = 13, kWindowBlur = 14,
    kWindowVectors = 15, kWindowSharp = 16, kWindowStats = 17, kWindowPalette = 18, kNumKernels = 19
};
static_assert(kWindowPalette == kProfWindowPalette, "the window palette launch's profiler slot");
static_assert(kWindowStats == kProfWindowStats, "the window statistics launch's profiler slot");
static_assert(kWindowSharp == kProfWindowSharp, "the window sharpness launch's profiler slot");
static_assert(kWindowVectors == kProfWindowVectors, "the blur vectors launch's profiler slot");
static_assert(kBoxPalettes == kProfBoxPalettes, "the box palette launch's profiler slot");
static_assert(kBoxStats == kProfBoxStats && kPlanarBoxStats == kProfPlanarBoxStats,
              "the box statistics launches' profiler slots");
static_assert(kWindowBlur == kProfWindowBlur, "the window blur launch's profiler slot");
static_assert(kClassify == kProfClassify && kDecode == kProfDecode, "the decode launches' profiler slots");
static_assert(kYuv == kProfYuv, "the YUV conversion launch's profiler slot");
static_assert(kLabels == kProfLabels, "the label map launch's profiler slot");
static_assert(kPalSums == kProfPalSums, "the fp64 pipeline's k_planar_sums launch's profiler slot");
struct KernelProfiler {
    unsigned mask = 0;                              // kernels to bracket with events
    // mask bits 24-30: stride s > 1, only every s-th batch call is bracketed
    // (all its launches; the events between back-to-back launches cost ~6% of
    // a bracketed call's time)
    unsigned calls = 0;                             // batch calls since the mask was set
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    std::vector<int> pending;                       // kernel id per used pair (-1: launch not timed)
    double total_ms[kNumKernels] = {};
    long launches[kNumKernels] = {};
    // record the opening event of a launch of kernel k (no-op unless enabled)
    int begin(int k, hipStream_t st);
    void end(int slot, hipStream_t st);
    void collect();                                 // after the stream is drained
};

// ---- device context ---------------------------------------------------------
// A few persistent host threads for the per-image host work of a batch (the
// palette decisions): parallel_for(n, f) runs f(0 .. n-1) on them and on the
// caller.  The threads are detached and the pool is never destroyed.
class HostPool {
public:
    explicit HostPool(int threads);
    // f(0 .. n-1) on the pool's threads and the caller; a pool busy with
    // another caller's job (the other lane) runs f inline on the caller instead
    // of queueing behind it (one lane's assembly no longer waits for
    // the other lane's palette decisions)
    void parallel_for(int n, const std::function<void(int)>& f);
    int size() const { return nthreads_; }
    // waits for a running job, then ends and joins the threads (phd_shutdown)
    void stop();

private:
    void worker();
    int nthreads_ = 0;
    std::mutex m_, job_m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* fn_ = nullptr;
    std::atomic<int> next_{0};
    int n_ = 0, busy_ = 0;
    unsigned gen_ = 0;
    bool stop_ = false;
    std::vector<std::thread> th_;
};
HostPool* host_pool();
HostPool* copy_pool();   // threads for host-buffer staging copies (phd_upload.cpp)
// phd_shutdown's parts: join the pools' threads (and forget the pools); the
// number of live pool threads
void stop_copy_pool();
int copy_pool_threads();
int library_threads();    // lane worker + pool threads alive in this process

// ---- the context's grow-only blocks (grow_buf.h) -------
struct DeviceMem {
    static void* alloc(size_t sz) { void* p = nullptr; return hipMalloc(&p, sz) == hipSuccess ? p : nullptr; }
    static void free(void* p) { (void)hipFree(p); }
    static void idle() { (void)hipDeviceSynchronize(); }
    static void failed(size_t sz) { set_error("hipMalloc of " + std::to_string(sz) + " bytes failed"); }
};
struct PinnedMem : DeviceMem {                      // (idle: the device's, as pinned copies run on its streams)
    static void* alloc(size_t sz) {
        void* p = nullptr;
        return hipHostMalloc(&p, sz, hipHostMallocDefault) == hipSuccess ? p : nullptr;
    }
    static void free(void* p) { (void)hipHostFree(p); }
    static void failed(size_t) { set_error("hipHostMalloc failed"); }
};
using DevBuf = GrowBuf<DeviceMem>;
using PinBuf = GrowBuf<PinnedMem>;
// A stage's pair and its two copies on st.  Stream order makes the one pinned block
// serve both ways: the table has gone up (and been read) before a copy later on st
// overwrites it; no copy of an earlier call is in flight when reserve() regrows (GrowBuf).
struct Staged : StagedBuf<DeviceMem, PinnedMem> {
    bool up(size_t bytes, hipStream_t st) {          // the first `bytes` of h to the start of d
        PHD_HIP(hipMemcpyAsync(d.as(), h.as(), bytes, hipMemcpyHostToDevice, st));
        return true;
    }
    bool down(size_t dev_off, size_t bytes, hipStream_t st, size_t pin_off = 0) {   // d + dev_off to h (+ pin_off)
        PHD_HIP(hipMemcpyAsync(h.as<char>() + pin_off, d.as<char>() + dev_off, bytes, hipMemcpyDeviceToHost, st));
        return true;
    }
};
// Context::dev[]
enum DevBufId {
    kDevGbuf,                                   // generic 2-D path: row pairs + scratch (double2)
    kDevPlanes,                                 // planar input: r | g | b | luma (fp64)
    kDevPrec,                                   // planar input: per-call records
    kDevWs,                                     // run_reports' workspace (its pinned twin: pin)
    kDevInter,                                  // the half spectra between the FFT passes (double2)
    kDevStage,                                  // upload staging for host images
    kDevPtrs,                                   // small device pointer arrays (debug hooks)
    // the input stage (phd_inputs.cpp): the packed staging images of one run
    // of views, typed views or YUV views
    kDevVstage,
    // the label maps of a run's images that have boxes to count and no map of
    // the caller's: 2 * mh * mw bytes each at 256-byte steps
    kDevLabScratch,
    kDevStage2, kDevStage2b,                    // host-buffer uploads: staging of overlapping groups
    kNumDevBufs
};
// Context::staged[]
enum StagedId {
    // batched sharpness (sharp_tiles.h): device pointers | box table | prefix |
    // slice partials (| flat sums), and the pinned copy of the uploaded part
    kStSharp,
    // the input stage: the device table of the pack, classify or conversion
    // launch and its pinned copy; ev_views follows the last such launch (the
    // table is rewritten only after it).  The label map launches' tables go
    // through the same pair (upload_table)
    kStViews,
    // box palettes (phd_boxpal.cpp): the counters of a launch's boxes and
    // their pinned copy
    kStBoxPal,
    // box statistics (phd_boxstats.cpp): records | items | the boxes' sums | the
    // finish's 64 bytes per box on the device, and the pinned block the table
    // goes up from and those 64 bytes come down to (the fp64 route: its items
    // and partial sums through the same pair)
    kStBoxStat,
    // window blur (phd_blurwin.cpp): twiddles | window records | a chunk's bin
    // sums | its maxima on the device, and the pinned block the table goes up
    // from and a chunk's sums and maxima come down to
    kStWinBlur,
    kNumStaged
};

struct Context {
    int device = -1;
    pid_t pid = 0;                                  // the process that created it (phd_shutdown)
    hipStream_t stream = nullptr;
    double* d_k255 = nullptr;                       // k/255.0 for k in [0,256)
    std::map<std::pair<int, bool>, FftPlanHost> plans;   // (length, composite)
    std::map<std::pair<int, int>, double2*> ct_tw;  // (length, rows?) -> compile-time plan twiddles
    std::map<std::tuple<int, int, int, int>, BlurTable> tables;
    std::map<std::tuple<int, int, int, int, int>, ColRuns> colruns;  // (H, W, nr, na, T): full-table runs
    std::map<int, GfftPlan> gplans;                 // global-memory FFT plans by length
    struct Cls {
        FastCls fc;
        ClassTables* d = nullptr;
        GroupCenters gc;                            // initialize_octree's centres
        std::vector<uint16_t> near;                 // make_near_order
    };
    std::map<std::tuple<int, int, int, double, double>, Cls> cls;
    // grow-only workspaces
    std::vector<PaletteDecision> dec_scratch;       // run_reports' per-image decisions
    std::vector<std::vector<double>> hsum_scratch;  // and host slot sums
    // grow-only blocks: freed and counted in loops (destroy_context, phd_debug_context_bytes)
    DevBuf dev[kNumDevBufs];
    Staged staged[kNumStaged];
    PinBuf pin;
    hipEvent_t ev_views = nullptr;
    // typed views: the snap tables' device copy (views_plan.h: snap_tables)
    uint8_t* d_snap = nullptr;
    hipEvent_t ev[8] = {};
    // two streams per context: `stream` (K1, then the FFT chain) and `tail`
    // (the A-record download, the palette's second pass -- rules upload, Kcut,
    // partial sums -- concurrent with the FFTs, then each image's C-record
    // download as soon as its column pass is done), joined by events
    hipStream_t tail = nullptr;
    hipEvent_t ev_k1 = nullptr, ev_tail = nullptr;
    hipEvent_t ev_dl_sd = nullptr;                  // the tail stream's last copy of a call
    hipEvent_t ev_fft = nullptr;                    // the FFT chain's end
    std::vector<hipEvent_t> ev_img_fft, ev_img_dl;
    KernelProfiler prof;
    hipEvent_t ev_null = nullptr;                   // orders the library stream after the null stream
    // host-buffer uploads (phd_upload.cpp): pinned slot ring on the h2d stream,
    // two device staging buffers for overlapping groups
    hipStream_t h2d = nullptr;
    hipStream_t h2d2 = nullptr;     // second upload stream (every other image of a group)
    hipEvent_t ev_h2d2 = nullptr;
    uint8_t* h2d_slots = nullptr;
    std::vector<hipEvent_t> ev_slot;
    std::vector<char> slot_used;
    int next_slot = 0;
    hipEvent_t ev_up[2] = {};
    std::mutex mu;
};
// The context of the current HIP device (created on first use).  nullptr if no GPU.
// Lanes: independent contexts of one device (own streams, workspaces and
// tables).  A large device batch is split over them and the halves run
// concurrently, so one half's host phases and launch gaps overlap the other's
// kernels.  Lane 0 is the context every single call uses.
constexpr int kLanes = 2;
Context* get_context();
Context* get_context_lane(int lane);
// flags of the events that only order device streams (no system-scope fence
// unless PHD_EV_FENCE is set; timing enabled, so a launch can record them)
unsigned device_event_flags();
std::vector<Context*> device_contexts();
// A persistent thread that runs one job at a time (the second lane).
class LaneWorker {
public:
    LaneWorker();
    void run(std::function<void()> f);
    void wait();
    // ends the thread after its current job (waiting up to timeout_ms for
    // it) and joins it; false (thread detached, left to the process) when
    // the job did not finish in time
    bool stop(int timeout_ms);
    // one caller at a time owns the worker (run .. wait); a busy worker is
    // not waited for: the caller runs its whole batch on lane 0 instead
    bool try_acquire() { return user_mu_.try_lock(); }
    void release() { user_mu_.unlock(); }

private:
    std::mutex user_mu_;
    void loop();
    std::mutex m_;
    std::condition_variable cv_, done_cv_;
    std::function<void()> job_;
    bool has_job_ = false;
    bool stop_ = false;
    std::thread th_;
};
LaneWorker* lane_worker();
// lanes a large device batch is split over (PHD_LANES, default 2; phd_set_lanes)
int lanes_setting();
// The stream a call works on: the caller's, or (NULL) the library's own stream
// ordered after every prior operation of the legacy null stream, so device
// buffers a caller (or PyTorch's default stream) is still producing are
// complete before the library reads them.
hipStream_t work_stream(Context* c, void* stream);
// workspace records start at 256-byte steps
constexpr size_t kAlign = 256;
inline size_t al(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }
const FftPlanHost* get_plan(Context* c, int n, bool composite = false);
// Per-pass twiddle tables of the compile-time plan of length n (rows or columns).
const double2* get_ct_twiddles(Context* c, int n, bool rows);

// The FFT kernels one image size takes: the compile-time plans when both
// lengths have one (fft_ct.hip), else the runtime-plan kernels (fft.hip).
struct FftSel {
    bool ct = false;
    const FftPlanHost* prow = nullptr;
    const FftPlanHost* pcol = nullptr;
    const double2* tw_r = nullptr;
    const double2* tw_c = nullptr;
    int col_blocks = 0;   // entries of the per-block max partials
    ColBins cbins;        // compile-time column pass: its per-column polar-bin runs
    // compile-time column pass: its full-prefetch form (the whole next column
    // streams into LDS during the epilogue) where the plan has one, else the
    // half-prefetch form; run_reports takes the half form when another lane's
    // two-block K1 shares the CUs (measured)
    bool col_pf = true;
    // phd_debug_column_form: -1 the library's choice, 0 half-prefetch, 1 full
    static int forced_form();
    // the generic path (a side above the LDS limit or with a large prime
    // factor): row pairs -> global row transforms -> split / transpose, then
    // the fused runtime column pass (cols_fused) or global column transforms
    // + the power / binning pass
    bool generic = false, cols_fused = false;
    const GfftPlan* grow = nullptr;
    const GfftPlan* gcol = nullptr;
    double2* gbuf = nullptr;
};
// tbl: the polar-bin table of the size (the compile-time column pass's run
// lists are made from it; nullptr: no compile-time column pass can launch)
bool select_fft(Context* c, int height, int width, int nbins, const uint8_t* const* imgs, int n, FftSel* s,
                const BlurTable* tbl, bool batch = false);
hipError_t launch_rows_sel(const FftSel& s, const uint8_t* img, int height, int width,
                           const unsigned long long* sums, const double* k255, double2* inter, hipStream_t st,
                           unsigned long long* rsum = nullptr);
// sums: K1's channel sums of the image (the compile-time column pass removes the DC bias)
hipError_t launch_cols_sel(const FftSel& s, const double2* inter, int height, int width, int wf,
                           const uint16_t* binmap, int nbins, unsigned long long* bin_sums, double* fmax_part,
                           const unsigned long long* sums, double* dbg, hipStream_t st);
const GfftPlan* get_gfft(Context* c, int n);
bool select_generic(Context* c, int height, int width, int nbins, FftSel* s);
// The generic path's row stage: luma from RGB8 (img, sums) or an fp64 plane
// (pgm, avgd) into the column-major half spectrum `inter`.
hipError_t generic_rows(const FftSel& s, const uint8_t* img, const double* pgm, int height, int width,
                        const unsigned long long* sums, const double* avgd, const double* k255, double2* inter,
                        hipStream_t st);
// (bscale: the bins' fixed-point scale, 0 = bin_scale(height, wf))
hipError_t generic_cols(const FftSel& s, double2* inter, int height, int wf, const uint16_t* binmap, int nbins,
                        unsigned long long* bin_sums, double* fmax_part, hipStream_t st, double bscale = 0.0);
const BlurTable* get_table(Context* c, int height, int width, int nr, int na);
// Classification tables of a grid (uploaded once per configuration).
const Context::Cls* get_cls(Context* c, const GridParams& gp);

// ---- the pipeline -----------------------------------------------------------
// pre_compute_error_checks (src/utilities.c:64-87) on the dimensions / crop boxes.
bool precheck(int height, int width);
bool check_crops(const Crop_Boundaries* cb, int height, int width);
// pixels of the HSV image (downsample_rgb's size through `short`, src/image_processing.c:378-379)
long hsv_count(int height, int width, int ds);
// The Full_Report_Data tree (compile_full_report, src/utilities.c:210-226) from
// the statistics, the palette decision and its slot sums pal[4k + {h, s, v, n}],
// the polar bin sums (fixed point at bscale, 0 = bin_scale(H, Wf)) and
// spectrum max, the crop sums.
Full_Report_Data* assemble(const RGB_Statistics& st, double s_bar, const PaletteDecision& dec,
                           const double* pal, long n_hsv, const BlurTable& tbl, const unsigned long long* bin_sums,
                           double fmax, const phd_config& cfg, const Crop_Boundaries* crops,
                           const double* sharp_sums, std::string* why, double bscale = 0.0);
// The blur half of assemble alone (phd_blur_batch_device): flat is na x nr.
void finish_blur(const BlurTable& tbl, const unsigned long long* bin_sums, double fmax, const phd_config& cfg,
                 double* flat, Blur_Vector* vectors, double bscale = 0.0);
RGB_Statistics stats_from_sums(const unsigned long long* m, long n);   // from K1's six moments of n pixels
bool all_aligned(const uint8_t* const* p, int n);                      // every pointer 4-byte aligned
// get_full_report_data's reports in the reference's allocation shape
// (phd_legacy.cpp): a separately malloc'd copy, its registration as a live
// tree, and its release (false when r is not a live tree)
Full_Report_Data* legacy_tree_copy(const Full_Report_Data* src);
void legacy_tree_free(Full_Report_Data* r);
void legacy_register(const Full_Report_Data* r);
bool legacy_release(Full_Report_Data* r);
// get_full_report_data on the caller's planar doubles (phd_planar.cpp): the
// RGB8 pipeline when every value is k/255.0, else the fp64 planar kernels.
Full_Report_Data* report_planar(Context* c, const double* r, const double* g, const double* b, int height,
                                int width, const phd_config& cfg, const Crop_Boundaries* crops);
// What a report call returns per image beside its report; every member optional
// (NULL: not asked for).  One record from the entries to the stage that fills it.
struct ImageOutputs {
    // device: the palette label map, (height / ds) x (width / ds); complete when
    // the run returns, untouched when the image fails before its palette decision
    uint16_t* labels = nullptr;
    // the caller's struct (zeroed by the entry): n_slots of a reported image and
    // the counts of its boxes, from labels or from a scratch map of the context
    // (kDevLabScratch); a failed image keeps {0, 0, NULL}
    phd_box_palette* box_pal = nullptr;
    // the caller's struct (zeroed by the entry): the statistics of its boxes at
    // full resolution; a failed image and one without boxes keep {0, NULL, NULL}
    phd_box_stats* box_stats = nullptr;
};
// The same as the C ABI passes it for a whole call: arrays over the images, or NULL.
struct CallOutputs {
    uint16_t* const* d_labels = nullptr;
    phd_box_palette* box_palettes = nullptr;
    phd_box_stats* box_stats = nullptr;
    ImageOutputs of(int i) const {
        return {d_labels ? d_labels[i] : nullptr, box_palettes ? box_palettes + i : nullptr,
                box_stats ? box_stats + i : nullptr};
    }
    // the caller's structs zeroed: before the argument check, so a failed call leaves nothing to free
    void reset(int n) const {
        for (int i = 0; i < n; i++) {
            if (box_palettes) box_palettes[i] = phd_box_palette{0, 0, nullptr};
            if (box_stats) box_stats[i] = phd_box_stats{0, nullptr, nullptr};
        }
    }
    // a label is a palette slot below PHD_LABEL_NONE's sign bit (int16 readers):
    // these outputs need fewer than 32768 octree groups
    bool needs_label_slots() const { return d_labels || box_palettes; }
};
// report_planar after its upload: the fp64 planar pipeline on planes already
// in kDevPlanes (4 n doubles: P.r | P.g | P.b | luma) on the idle stream st;
// cfg, the size and the boxes validated by the caller.  The typed entry runs
// it on the planes k_decode_view filled.  outs: ImageOutputs, the box
// statistics from the fp64 functions on the planes (k_planar_box_stats).
Full_Report_Data* report_planes_device(Context* c, const PlanarSrc& P, int height, int width, const phd_config& cfg,
                                       const Crop_Boundaries* crops, hipStream_t st, const ImageOutputs& outs);
// Run the full report on n same-size device images.  out[i]/status[i] per image.
// crops: one set of boxes for every image (the single-image entries; two
// launches per box, sharpness.hip's k_sharp_pass).  img_crops (crops must be
// NULL): image i's own boxes, NULL entries allowed, already validated
// (crops_why); every box of the call goes through one batched launch.
// outs (or NULL: none): image i's ImageOutputs, n of them; the boxes of the box
// palettes and statistics are the image's img_crops.
bool run_reports(Context* c, const uint8_t* const* d_imgs, int n, int height, int width,
                 const phd_config& cfg, const Crop_Boundaries* crops, Full_Report_Data** out,
                 int* status, hipStream_t stream, const Crop_Boundaries* const* img_crops = nullptr,
                 const ImageOutputs* outs = nullptr);
// A launch table (phd_inputs.cpp): `bytes` go up on st through the kStViews
// pair.  table_begin returns its pinned block (nullptr: error) once the last
// launch that read the table is done, to be filled in place -- the device
// block has its final address by then;
// table_upload is the one copy; table_launched: after the last operation on st
// that reads the table.  upload_table: the three steps with the first `filled`
// bytes from `host`, the rest zero.
void* table_begin(Context* c, size_t bytes);
bool table_upload(Context* c, size_t bytes, hipStream_t st);
bool upload_table(Context* c, const void* host, size_t filled, size_t bytes, hipStream_t st);
bool table_launched(Context* c, hipStream_t st);
// A whole call of one launch over a table of `bytes` (the window entries), under
// the context's lock: fill(pinned block), the copy, launch(device block, st) ->
// hipError_t under profile slot `slot`, on the caller's stream or -- stream ==
// nullptr -- the library's, which is then waited for.
template <class Fill, class Launch>
bool table_call(Context* c, void* stream, size_t bytes, Fill fill, Launch launch, int slot) {
    const hipStream_t st = work_stream(c, stream);
    uint8_t* h = (uint8_t*)table_begin(c, bytes);
    if (!h) return false;
    fill(h);
    if (!table_upload(c, bytes, st)) return false;
    const int ps = c->prof.begin(slot, st);
    const hipError_t e = launch(c->staged[kStViews].d.as<const uint8_t>(), st);
    c->prof.end(ps, st);
    PHD_HIP(e);
    if (!table_launched(c, st)) return false;
    if (!stream) {                                           // the library's stream: waited for
        PHD_HIP(hipStreamSynchronize(st));
        c->prof.collect();
    }
    return true;
}
// The batched sharpness stage of n same-size device images on st: uploads the
// box table (one copy) and enqueues the two launches.  Box sums go to out0 +
// img * out_stride + 2 * slot (doubles); out0 == nullptr: to a flat array in
// the context's own buffer (*flat_dev; plan slots must be flat).
bool enqueue_sharpness(Context* c, const uint8_t* const* d_imgs, int n, int width, const SharpPlan& plan,
                       double* out0, long out_stride, hipStream_t st, double** flat_dev = nullptr);
// The box palettes of a launch (phd_boxpal.cpp; plan and row code:
// box_tiles.h): the boxes' records, box_plan's items and the counters they
// fill, box b's n_slots + 1 at recs[b].out.
struct BoxJob {
    std::vector<BoxRec> recs;
    std::vector<BoxItem> items;
    long long counters = 0;
    // a box of map coordinates (rows top <= y < bottom, columns left <= x < right)
    void add(const uint16_t* map, int mw, int n_slots, int top, int bottom, int left, int right);
    // the boxes of an image (image coordinates) on its mh x mw map of downsample_rate ds
    void add_image(const uint16_t* map, int mh, int mw, int ds, int n_slots, const Crop_Boundaries* b);
};
bool box_palette_fill(phd_box_palette* bp, int n_boxes, int n_slots, const uint32_t* h);
// The job on st: its table goes up (table_begin), kStBoxPal's device block is zeroed
// by one memset, one launch counts, one copy brings the counters to
// its pinned block.  The caller waits for st before it reads them.
bool enqueue_box_job(Context* c, const BoxJob& job, hipStream_t st);
// The box statistics of a launch (phd_boxstats.cpp; records and row walk:
// box_stat_tiles.h): the boxes' records and box_plan's items.
struct BoxStatJob {
    std::vector<BoxStatRec> recs;
    std::vector<BoxItem> items;
    // the boxes of a packed RGB8 image of `width` columns (validated: crops_why)
    void add_image(const uint8_t* img, int width, const Crop_Boundaries* b);
};
// The job on st: the table goes up through kStBoxStat, one memset zeroes
// the records, k_box_stats (profile slot 12) and its finish run, one copy brings
// kBoxStatOut u64 per box to its pinned block, where box_stats_host() points
// after the caller has waited for st.
bool enqueue_box_stat_job(Context* c, const BoxStatJob& job, hipStream_t st);
const unsigned long long* box_stats_host(const Context* c);
// *bs <- n_boxes boxes from their downloaded kBoxStatOut u64 each (h) and their
// pixel counts (one malloc; none for no boxes)
bool box_stats_fill(phd_box_stats* bs, const Crop_Boundaries* b, const unsigned long long* h);
// the same from finished values: stats[k], average_saturation[k]
bool box_stats_alloc(phd_box_stats* bs, int n_boxes);

// ---- device batches (the driver: phd_entries.cpp; views, typed views and
// ---- YUV views: phd_inputs.cpp) ------------------------------------------------
// A kept image of a device batch call, in caller order.
struct BatchImage {
    enum Source { kPacked, kView, kTyped, kYuv };
    int index;                       // the caller's
    Source kind;
    const void* src;                 // the packed RGB8 device image, or the caller's phd_image_view,
                                     // phd_typed_view or phd_yuv_view of it (staged on the lane)
    int height, width;
    const Crop_Boundaries* boxes;    // NULL: none
    ImageOutputs outs{};             // what the call returns for it beside the report
};
// The reports and statuses of one run of m images, and their way back to the
// caller's arrays: result k belongs to the caller's image idx[k].
struct RunResults {
    std::vector<Full_Report_Data*> o;
    std::vector<int> st;
    explicit RunResults(size_t m) : o(m, nullptr), st(m, -1) {}
    void scatter(const std::vector<int>& idx, Full_Report_Data** out, int* status) const {
        for (size_t k = 0; k < idx.size(); k++) {
            out[idx[k]] = o[k];
            status[idx[k]] = st[k];
        }
    }
};
// One same-size group (indices into imgs) on a lane: stages what its source
// kind needs and reports it; r: the group's results, in the group's order.
// boxes: the call has per-image crop boxes (imgs[].boxes, NULL entries allowed).
using GroupFn = void (*)(Context* cl, const std::vector<BatchImage>& imgs, const std::vector<int>& grp, bool boxes,
                         const phd_config& cfg, void* stream, RunResults* r);
// One run_reports call over the group's images at positions ks (image grp[k]
// packed at ptrs[k]); their results into r at those positions.
void report_group(Context* cl, const std::vector<BatchImage>& imgs, const std::vector<int>& grp,
                  const std::vector<int>& ks, const uint8_t* const* ptrs, bool boxes, const phd_config& cfg,
                  void* stream, RunResults* r);
// Runs the groups on the lanes (the only lane loop of the device entries) and
// returns the call's failure count.
int run_device_batch(Context* c, const std::vector<BatchImage>& imgs, const std::vector<std::vector<int>>& groups,
                     GroupFn run_group, bool boxes, const phd_config& cfg, Full_Report_Data** out, int* status,
                     int n_images, void* stream);
// A report entry's name in its messages, from its family ("mixed", "views",
// "typed_views", "yuv") and the outputs present, and the entries' shared first
// steps: reset, argument check (args_ok), the label slots' rule (phd_entries.cpp)
std::string entry_name(const char* family, const char* plain, const CallOutputs& outs);
bool report_prologue(const std::string& entry, bool args_ok, int n_images, const phd_config* cfg,
                     const CallOutputs& outs);
// The same-size groups of the kept images of a mixed-size call, and one group
// of a batch large enough for two lanes cut in two (views, typed and YUV calls)
std::vector<std::vector<int>> mixed_groups(const std::vector<BatchImage>& imgs);
void split_for_lanes(std::vector<std::vector<int>>* groups, void* stream);
// The palette's second pass runs as one Kcut and one K3 launch over the batch
// (else a pair of launches per image): full-resolution images whose palette is
// fused, or whose batched K3 holds max_slots slots in LDS.
bool palette_tail_batched(const GridParams& gp, int ds, bool fused, int max_slots);
// Palette intermediates only (for parity tests).
bool run_palette_trace(Context* c, const uint8_t* d_img, int height, int width, const phd_config& cfg,
                       std::vector<unsigned>* hist, PaletteDecision* dec,
                       std::vector<double>* device_counts);

void record_timings(const double* ms, int n);

// ---- host-buffer uploads (phd_upload.cpp) -------------------------------------
bool upload_init(Context* c);
// Copy `bytes` host bytes to d_dst through the pinned slot ring on c->h2d.  On
// return the caller's buffer has been read; the DMA may still run.
bool upload_async(Context* c, uint8_t* d_dst, const uint8_t* src, size_t bytes, std::string* why,
                  hipStream_t s = nullptr);
// 2 (PHD_UPLOAD_STREAMS=2; default 1): a group's images alternate between the
// h2d and h2d2 streams, each fed by its own host thread (runtime pageable path only)
int upload_streams();

}  // namespace phd
