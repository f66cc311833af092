// ASan/UBSan driver for the host half of phd_palwin.cpp (built with
// -DPHD_PALWIN_HOST_ONLY; tests/test_window_palette_host.py): the window palette
// kernel's host twin over heap label maps of exactly 2 * mh * mw bytes at each of
// the four window sizes, with windows flush to every edge, so a read past the last
// label of the last row (or before the first) is a report.  n_slots is 0, 17 and
// 4096; the counts and the dominant label are checked against a plain per-element
// count.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/photohive_dsp.h"

// the library's error slot (phd_context.cpp there)
namespace phd {
static std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
void clear_error() { g_err.clear(); }
}  // namespace phd

// the window at (t, l), element by element: n_slots + 1 counters and the dominant label
static void plain_count(const uint16_t* map, int mw, int t, int l, int T, int n_slots, std::vector<uint32_t>* counts,
                        uint16_t* dominant) {
    counts->assign((size_t)n_slots + 1, 0u);
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++) {
            const unsigned lab = map[(size_t)(y + t) * mw + x + l];
            (*counts)[lab < (unsigned)n_slots ? lab : (unsigned)n_slots]++;
        }
    int best = 0;
    for (int s = 1; s <= n_slots; s++)
        if ((*counts)[s] > (*counts)[best]) best = s;        // strictly larger: a tie stays at the lower column
    *dominant = best < n_slots ? (uint16_t)best : (uint16_t)0xFFFF;
}

static int run_size(int T, int H, int W, int n_slots) {
    uint16_t* map = (uint16_t*)malloc((size_t)2 * H * W);
    unsigned s = 97531u + (unsigned)T + (unsigned)n_slots;
    unsigned cur = 0;
    for (size_t i = 0; i < (size_t)H * W; i++) {
        s = s * 1664525u + 1013904223u;
        const unsigned v = s >> 16;
        if (v % 3 == 0)
            cur = v % 29 == 0 ? 0xFFFFu : v % 31 == 0 ? (unsigned)n_slots + v % 5 : v % (n_slots ? n_slots : 7);
        map[i] = (uint16_t)(cur > 0xFFFFu ? 0xFFFEu : cur);  // runs of labels, some none, some past the palette
    }
    //           corners, flush with one edge each, inside, the first again
    int top[] = {0, 0, H - T, H - T, 0, (H - T) / 2, H - T, (H - T) / 2, (H - T) / 3, 0};
    int lef[] = {0, W - T, 0, W - T, (W - T) / 2, 0, (W - T) / 3, W - T, (W - T + 1) / 2, 0};
    const int N = (int)(sizeof(top) / sizeof(top[0]));
    std::vector<int> bot(N), rig(N);
    for (int k = 0; k < N; k++) {
        bot[k] = top[k] + T;
        rig[k] = lef[k] + T;
    }
    Crop_Boundaries cb{N, top, bot.data(), lef, rig.data()};
    const size_t nc = (size_t)n_slots + 1;
    std::vector<uint32_t> counts(nc * N, 0xDEADBEEFu);
    std::vector<uint16_t> dom(N, 0xBEEF);
    int bad = 0;
    if (phd_debug_window_palette_host(map, H, W, n_slots, &cb, T, counts.data(), dom.data()) != 0) {
        fprintf(stderr, "FAIL: T = %d, n_slots = %d: host twin returned an error: %s\n", T, n_slots,
                phd::g_err.c_str());
        bad++;
    }
    for (int k = 0; k < N && !bad; k++) {
        std::vector<uint32_t> want;
        uint16_t want_dom;
        plain_count(map, W, top[k], lef[k], T, n_slots, &want, &want_dom);
        if (!std::equal(want.begin(), want.end(), counts.begin() + nc * k) || dom[k] != want_dom) {
            fprintf(stderr, "FAIL: T = %d, n_slots = %d, window %d: dominant %u against %u\n", T, n_slots, k,
                    (unsigned)dom[k], (unsigned)want_dom);
            bad++;
        }
    }
    // only the values asked for
    std::vector<uint32_t> only_c(nc * N, 0u);
    std::vector<uint16_t> only_d(N, 0);
    if (phd_debug_window_palette_host(map, H, W, n_slots, &cb, T, only_c.data(), nullptr) != 0 || only_c != counts ||
        phd_debug_window_palette_host(map, H, W, n_slots, &cb, T, nullptr, only_d.data()) != 0 || only_d != dom) {
        fprintf(stderr, "FAIL: T = %d, n_slots = %d: one output alone\n", T, n_slots);
        bad++;
    }
    // a window past the last row or column, or of another size, is refused, not read
    int t2[] = {H - T + 1}, b2[] = {H + 1}, l2[] = {0}, r2[] = {T};
    Crop_Boundaries below{1, t2, b2, l2, r2};
    int t3[] = {0}, b3[] = {T}, l3[] = {W - T + 1}, r3[] = {W + 1};
    Crop_Boundaries beside{1, t3, b3, l3, r3};
    int b4[] = {T + 1};
    Crop_Boundaries tall{1, t3, b4, l2, r2};
    if (phd_debug_window_palette_host(map, H, W, n_slots, &below, T, counts.data(), nullptr) != -1 ||
        phd_debug_window_palette_host(map, H, W, n_slots, &beside, T, counts.data(), nullptr) != -1 ||
        phd_debug_window_palette_host(map, H, W, n_slots, &tall, T, counts.data(), nullptr) != -1 ||
        phd_debug_window_palette_host(map, H, W, n_slots, &cb, T + 1, counts.data(), nullptr) != -1 ||
        phd_debug_window_palette_host(map, H, W, 4097, &cb, T, counts.data(), nullptr) != -1 ||
        phd_debug_window_palette_host(map, H, W, n_slots, &cb, T, nullptr, nullptr) != -1) {
        fprintf(stderr, "FAIL: T = %d: a bad call was accepted\n", T);
        bad++;
    }
    Crop_Boundaries none{0, nullptr, nullptr, nullptr, nullptr};
    if (phd_debug_window_palette_host(map, H, W, n_slots, &none, T, nullptr, nullptr) != 0) bad++;
    free(map);
    return bad;
}

int main() {
    int bad = 0;
    for (int T : {16, 32, 64, 128})
        for (int n_slots : {0, 17, 4096}) {
            bad += run_size(T, T + 3, T + 5, n_slots);       // an odd width: every row at another phase
            bad += run_size(T, T, T, n_slots);               // the map is the window
        }
    if (!bad) printf("window palette host OK\n");
    return bad;
}
