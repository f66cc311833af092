// ASan/UBSan driver for window_call.h alone (tests/test_window_sharpness_host.py):
// the plan of a window call -- its walk against window_grid's boxes written out as
// two nested loops, every refusal with its words, the counts at the 2^31 - 1 bar
// and far past it (three grids whose sum does not fit a long long), and the twins'
// ladder.  No pointer to an image is ever read: the plan only offsets them.
#include <cstdio>
#include <string>
#include <vector>

#include "../../photohive_dsp_amd/csrc/window_call.h"

using phd::WindowPlan;

static int bad = 0;
static void expect(bool ok, const char* what, const std::string& got = "") {
    if (ok) return;
    fprintf(stderr, "FAIL: %s%s%s\n", what, got.empty() ? "" : ": ", got.c_str());
    bad++;
}

struct Box {
    long long i, k, top, left;
    bool operator==(const Box& o) const { return i == o.i && k == o.k && top == o.top && left == o.left; }
};

static const uint8_t* const kImg[3] = {(const uint8_t*)4096, (const uint8_t*)8192, (const uint8_t*)12288};
static const void* const kOut[3] = {(const void*)(size_t)(1 << 20), (const void*)(size_t)(2 << 20),
                                    (const void*)(size_t)(3 << 20)};

// core.py's window_grid: boxes at (y * stride, x * stride), y < gh, x < gw, row-major
static std::vector<Box> grid_boxes(int i, int h, int w, int T, int stride) {
    std::vector<Box> v;
    const int gh = h >= T ? (h - T) / stride + 1 : 0, gw = w >= T ? (w - T) / stride + 1 : 0;
    for (int y = 0; y < gh; y++)
        for (int x = 0; x < gw; x++)
            v.push_back(Box{i, (long long)y * gw + x, (long long)y * stride, (long long)x * stride});
    return v;
}

static std::vector<Box> walk(const WindowPlan& p) {
    std::vector<Box> v;
    p.for_each([&](int i, long long k, long long top, long long left) { v.push_back(Box{i, k, top, left}); });
    return v;
}

static void grids() {
    const int hs[3] = {37, 16, 53}, ws[3] = {53, 16, 37}, T = 16;
    for (int stride : {1, T, 5, 100}) {
        WindowPlan p(kImg, hs, ws, 3, nullptr, false, T, stride);
        std::string why;
        expect(p.args_why(true, &why) && p.build(kOut, "d_out", &why), "grid plan", why);
        std::vector<Box> want;
        long long total = 0;
        for (int i = 0; i < 3; i++) {
            const std::vector<Box> g = grid_boxes(i, hs[i], ws[i], T, stride);
            expect(p.count[i] == (long long)g.size(), "grid count");
            total += (long long)g.size();
            want.insert(want.end(), g.begin(), g.end());
        }
        expect(p.total == total && walk(p) == want, "grid walk");
        for (const Box& b : want)
            expect(b.top + T <= hs[b.i] && b.left + T <= ws[b.i], "grid box inside its image");
    }
    // by hand: 37 x 53 at T = 16, stride 5: rows at 0 .. 20, columns at 0 .. 35
    const int h = 37, w = 53;
    WindowPlan p(kImg, &h, &w, 1, nullptr, false, 16, 5);
    std::string why;
    expect(p.build(nullptr, nullptr, &why) && p.total == 5 * 8, "5 x 8 grid", why);
    const std::vector<Box> v = walk(p);
    expect(v.size() == 40 && v[0] == Box{0, 0, 0, 0} && v[7] == Box{0, 7, 0, 35} && v[8] == Box{0, 8, 5, 0} &&
               v[39] == Box{0, 39, 20, 35},
           "5 x 8 grid's corners");
}

static void lists() {
    const int hs[3] = {100, 64, 70}, ws[3] = {200, 64, 133}, T = 64;
    int t0[] = {0, 36, 36}, b0[] = {64, 100, 100}, l0[] = {0, 136, 136}, r0[] = {64, 200, 200};   // a duplicate
    int t2[] = {6}, b2[] = {70}, l2[] = {69}, r2[] = {133};
    const Crop_Boundaries c0{3, t0, b0, l0, r0}, none{0, nullptr, nullptr, nullptr, nullptr}, c2{1, t2, b2, l2, r2};
    const Crop_Boundaries* const all[3] = {&c0, &none, &c2};
    const Crop_Boundaries* const holes[3] = {&c0, nullptr, &c2};
    // an image without windows needs no destination: a NULL list or N == 0
    const void* const out[3] = {kOut[0], nullptr, kOut[2]};
    for (const Crop_Boundaries* const* w : {all, holes}) {
        WindowPlan p(kImg, hs, ws, 3, w, true, T, 0);
        std::string why;
        expect(p.args_why(true, &why) && p.build(out, "d_out", &why), "list plan", why);
        expect(p.count[0] == 3 && p.count[1] == 0 && p.count[2] == 1 && p.total == 4, "list counts");
        const std::vector<Box> want = {{0, 0, 0, 0}, {0, 1, 36, 136}, {0, 2, 36, 136}, {2, 0, 6, 69}};
        expect(walk(p) == want, "list walk");
    }
    // no window at all: a plan of none, whatever the destinations
    const Crop_Boundaries* const empty[3] = {nullptr, &none, nullptr};
    const void* const no_out[3] = {nullptr, nullptr, nullptr};
    WindowPlan p(kImg, hs, ws, 3, empty, true, T, 0);
    std::string why;
    expect(p.build(no_out, "d_out", &why) && p.total == 0 && walk(p).empty(), "empty plan", why);
}

// the plan's refusal, or "" where it builds
static std::string refusal(const uint8_t* const* imgs, const int* hs, const int* ws, int n,
                           const Crop_Boundaries* const* windows, bool lists, int T, int stride, bool rest = true,
                           const void* const* out = kOut) {
    WindowPlan p(imgs, hs, ws, n, windows, lists, T, stride);
    std::string why;
    if (p.args_why(rest, &why) && p.build(out, "d_out", &why)) return "";
    return why;
}

static void refusals() {
    const int hs[2] = {100, 100}, ws[2] = {200, 200};
    int t[] = {0, 36}, b[] = {64, 100}, l[] = {0, 136}, r[] = {64, 200};
    const Crop_Boundaries good{2, t, b, l, r};
    const Crop_Boundaries* const gg[2] = {&good, &good};
    expect(refusal(kImg, hs, ws, 2, gg, true, 64, 0) == "", "a good list call");
    expect(refusal(kImg, hs, ws, 2, nullptr, true, 64, 0) == "NULL argument", "lists required");
    expect(refusal(nullptr, hs, ws, 2, gg, true, 64, 0) == "NULL argument", "NULL d_images");
    expect(refusal(kImg, nullptr, ws, 2, gg, true, 64, 0) == "NULL argument", "NULL heights");
    expect(refusal(kImg, hs, nullptr, 2, gg, true, 64, 0) == "NULL argument", "NULL widths");
    expect(refusal(kImg, hs, ws, 2, gg, true, 64, 0, false) == "NULL argument", "the entry's other pointers");
    expect(refusal(kImg, hs, ws, 0, gg, true, 64, 0) == "n_images must be positive", "n_images 0");
    expect(refusal(kImg, hs, ws, -3, nullptr, false, 64, 64) == "n_images must be positive", "n_images -3");
    expect(refusal(kImg, hs, ws, 2, nullptr, false, 64, 0) == "stride must be positive, not 0", "stride 0");
    expect(refusal(kImg, hs, ws, 2, nullptr, false, 64, -1) == "stride must be positive, not -1", "stride -1");
    expect(refusal(kImg, hs, ws, 2, gg, true, 64, -1) == "", "a list call has no stride");
    const uint8_t* const hole[2] = {kImg[0], nullptr};
    expect(refusal(hole, hs, ws, 2, gg, true, 64, 0) == "image 1: NULL image", "NULL image");
    const int low[2] = {100, 63}, narrow[2] = {15, 200};
    expect(refusal(kImg, low, ws, 2, gg, true, 64, 0) == "image 1: 63 x 200 is smaller than the window 64", "low");
    expect(refusal(kImg, hs, narrow, 2, nullptr, false, 16, 16) == "image 0: 100 x 15 is smaller than the window 16",
           "narrow");
    const void* const half[2] = {kOut[0], nullptr};
    expect(refusal(kImg, hs, ws, 2, gg, true, 64, 0, true, half) == "image 1: NULL d_out for 2 windows", "list output");
    expect(refusal(kImg, hs, ws, 2, nullptr, false, 64, 64, true, half) == "image 1: NULL d_out for 3 windows",
           "grid output");
    expect(refusal(kImg, hs, ws, 2, gg, true, 64, 0, true, nullptr) == "", "an entry without destinations");
    // the list rule
    int b65[] = {64, 101}, tm[] = {-1, 36}, bm[] = {63, 100};
    const Crop_Boundaries tall{2, t, b65, l, r}, above{2, tm, bm, l, r}, minus{-1, t, b, l, r},
        holes{2, t, nullptr, l, r};
    const Crop_Boundaries* const c_tall[2] = {&good, &tall};
    const Crop_Boundaries* const c_above[2] = {&above, &good};
    const Crop_Boundaries* const c_minus[2] = {&minus, &good};
    const Crop_Boundaries* const c_holes[2] = {&good, &holes};
    expect(refusal(kImg, hs, ws, 2, c_tall, true, 64, 0) ==
               "image 1: window 1 (top 36, bottom 101, left 136, right 200) is not 64 x 64",
           "not T x T", refusal(kImg, hs, ws, 2, c_tall, true, 64, 0));
    expect(refusal(kImg, hs, ws, 2, c_above, true, 64, 0) ==
               "image 0: window 0 (top -1, bottom 63, left 0, right 64) leaves the 100 x 200 image",
           "leaves the image", refusal(kImg, hs, ws, 2, c_above, true, 64, 0));
    expect(refusal(kImg, hs, ws, 2, c_minus, true, 64, 0) == "image 0: bad window list", "N < 0");
    expect(refusal(kImg, hs, ws, 2, c_holes, true, 64, 0) == "image 1: bad window list", "a NULL column");
    // sides at the ends of int: the rule's differences are taken in 64 bits
    int te[] = {-2147483647 - 1}, be[] = {2147483647}, le[] = {0}, re[] = {64};
    const Crop_Boundaries ends{1, te, be, le, re};
    const Crop_Boundaries* const c_ends[1] = {&ends};
    expect(refusal(kImg, hs, ws, 1, c_ends, true, 64, 0).find(" is not 64 x 64") != std::string::npos, "int ends");
}

static void too_many() {
    // exactly 2^31 - 1 windows pass: one row of them
    const int h1 = 16, w1 = 2147483647;
    WindowPlan one(kImg, &h1, &w1, 1, nullptr, false, 16, 1);
    std::string why;
    expect(one.build(kOut, "d_out", &why) && one.total == 2147483647LL - 15, "a row of 2^31 - 16 windows", why);
    const int h2[2] = {16, 16}, w2[2] = {2147483647 - 16, 47};    // 2^31 - 32 and 32 windows: one past the bar
    expect(refusal(kImg, h2, w2, 2, nullptr, false, 16, 1) == "too many windows", "2^31 windows");
    const int w3[2] = {2147483647 - 16, 46};                      // 2^31 - 32 and 31 windows: at the bar
    expect(refusal(kImg, h2, w3, 2, nullptr, false, 16, 1) == "", "2^31 - 1 windows in two images");
    // 46341^2 windows in one image
    const int big = 46340 + 64;
    expect(refusal(kImg, &big, &big, 1, nullptr, false, 64, 1) == "too many windows", "46341^2 windows");
    // three grids of about 2^62 windows each: refused at the first, no sum is formed
    const int top[3] = {2147483647, 2147483647, 2147483647};
    for (int T : {16, 64})
        expect(refusal(kImg, top, top, 3, nullptr, false, T, 1) == "too many windows", "three grids of 2^62");
    // the count comes before a later image's defect
    const uint8_t* const hole[2] = {kImg[0], nullptr};
    const int hb[2] = {big, 100}, wb[2] = {big, 200};
    expect(refusal(hole, hb, wb, 2, nullptr, false, 64, 1) == "too many windows", "the count before image 1");
    // lists: 2^31 windows in two lists of 2^30 would need 16 GiB of boxes; the bar is the grids' to reach
}

static void twins() {
    const uint8_t* img = kImg[0];
    int t[] = {0}, b[] = {64}, l[] = {0}, r[] = {64}, r65[] = {65};
    const Crop_Boundaries one{1, t, b, l, r}, wide{1, t, b, l, r65}, none{0, nullptr, nullptr, nullptr, nullptr};
    auto why = [&](const uint8_t* rgb, int h, int w, const Crop_Boundaries* cb, const std::string& size_why, bool outs) {
        std::string s;
        return phd::window_twin_why(rgb, h, w, cb, 64, size_why, outs, "NULL outputs", &s) ? std::string() : s;
    };
    expect(why(img, 100, 200, &one, "", true) == "", "a good twin call");
    expect(why(nullptr, 100, 200, &one, "window must be", true) == "NULL image", "the image first");
    expect(why(img, 10, 200, &one, "window must be", true) == "window must be", "the twin's own rule second");
    expect(why(img, 63, 200, &wide, "", false) == "63 x 200 is smaller than the window 64", "then the size");
    expect(why(img, 100, 200, &wide, "", false) == "window 0 (top 0, bottom 64, left 0, right 65) is not 64 x 64",
           "then the list");
    expect(why(img, 100, 200, &one, "", false) == "NULL outputs", "then the outputs");
    expect(why(img, 100, 200, &none, "", false) == "" && why(img, 100, 200, nullptr, "", false) == "",
           "no window: no outputs needed");
}

int main() {
    grids();
    lists();
    refusals();
    too_many();
    twins();
    if (!bad) printf("window call OK\n");
    return bad;
}
