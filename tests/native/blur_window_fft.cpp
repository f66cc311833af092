// Host check of blur_window.h (tests/test_blur_window_native.py), built from the
// header's host half with no GPU: for T = 64 and 128 a real T x T image is
// packed two rows per complex row (win_pixel_slot), run through the window
// plan's passes butterfly by butterfly (win_transform_host: win_bfly_load /
// win_bfly_store, win_separate, the packed DC + i Nyquist column), and every
// element (u, x <= T/2) read back through win_spectrum is compared with a direct
// 2-D DFT in long double.  Images: random, constant, one bright pixel,
// horizontal and vertical 1-px stripes, a checkerboard (energy in the Nyquist
// column, the Nyquist row and the corner).  Bound: 1e-13 of the largest output.
// Also: the index maps are permutations of the buffer, and the box rule.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../photohive_dsp_amd/csrc/blur_window.h"

using namespace phd;

static int g_fail = 0;

template <int T>
static void direct(const std::vector<double>& img, std::vector<long double>& re, std::vector<long double>& im) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    constexpr int WF = T / 2 + 1;
    std::vector<long double> c(T), s(T);
    for (int e = 0; e < T; e++) {
        c[e] = cosl(two_pi * e / T);
        s[e] = -sinl(two_pi * e / T);
    }
    std::vector<long double> rr((size_t)T * WF), ri((size_t)T * WF);
    for (int y = 0; y < T; y++)
        for (int k = 0; k < WF; k++) {
            long double a = 0, b = 0;
            for (int x = 0; x < T; x++) {
                const int e = (x * k) % T;
                a += img[(size_t)y * T + x] * c[e];
                b += img[(size_t)y * T + x] * s[e];
            }
            rr[(size_t)y * WF + k] = a;
            ri[(size_t)y * WF + k] = b;
        }
    re.assign((size_t)T * WF, 0);
    im.assign((size_t)T * WF, 0);
    for (int u = 0; u < T; u++)
        for (int k = 0; k < WF; k++) {
            long double a = 0, b = 0;
            for (int y = 0; y < T; y++) {
                const int e = (y * u) % T;
                const long double xr = rr[(size_t)y * WF + k], xi = ri[(size_t)y * WF + k];
                a += xr * c[e] - xi * s[e];
                b += xr * s[e] + xi * c[e];
            }
            re[(size_t)u * WF + k] = a;
            im[(size_t)u * WF + k] = b;
        }
}

template <int T>
static void check_image(const char* what, const std::vector<double>& img) {
    constexpr int WF = T / 2 + 1;
    std::vector<double2> buf(win_elems(T)), tmp(win_elems(T)), tw(T);
    win_twiddles(T, tw.data());
    double* d = reinterpret_cast<double*>(buf.data());
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++) d[2 * win_pixel_slot<T>(y, x) + (y & 1)] = img[(size_t)y * T + x];
    win_transform_host<T>(buf.data(), tw.data(), tmp.data());
    std::vector<long double> re, im;
    direct<T>(img, re, im);
    long double mx = 0, err = 0;
    for (int u = 0; u < T; u++)
        for (int x = 0; x < WF; x++) {
            const double2 X = win_spectrum<T>(buf.data(), u, x);
            const long double wr = re[(size_t)u * WF + x], wi = im[(size_t)u * WF + x];
            mx = fmaxl(mx, hypotl(wr, wi));
            err = fmaxl(err, hypotl(X.x - wr, X.y - wi));
        }
    const bool ok = mx > 0 ? err <= 1e-13L * mx : err == 0;
    std::printf("T=%d %-12s max |X| %.6Le  err %.3Le of max%s\n", T, what, mx, mx > 0 ? err / mx : err,
                ok ? "" : "  FAIL");
    if (!ok) g_fail++;
}

template <int T>
static void check_maps() {
    std::vector<int> seen(win_elems(T), 0);
    for (int k = 0; k < T / 2; k++)
        for (int y = 0; y < T; y++) {
            const int i = win_col_index<T>(y, k);
            if (i < 0 || i >= win_elems(T)) {
                std::printf("T=%d win_col_index(%d, %d) = %d out of range  FAIL\n", T, y, k, i);
                g_fail++;
                return;
            }
            seen[i]++;
        }
    // every slot but the row pairs' padding is the place of one column element and of two pixels
    const std::vector<int> cols = seen;
    std::fill(seen.begin(), seen.end(), 0);
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++) seen[win_pixel_slot<T>(y, x)]++;
    for (int i = 0; i < win_elems(T); i++) {
        const bool pad = i % win_pitch(T) >= T;
        if (cols[i] != (pad ? 0 : 1) || seen[i] != (pad ? 0 : 2)) {
            std::printf("T=%d slot %d is the place of %d column elements and %d pixels  FAIL\n", T, i, cols[i],
                        seen[i]);
            g_fail++;
            return;
        }
    }
    std::printf("T=%d index maps are permutations\n", T);
}

template <int T>
static void check_size() {
    check_maps<T>();
    std::mt19937_64 rng(977 + T);
    std::uniform_real_distribution<double> u(-0.5, 0.5);
    std::vector<double> img((size_t)T * T);
    for (auto& v : img) v = u(rng);
    check_image<T>("random", img);
    for (auto& v : img) v = 0.25;
    check_image<T>("constant", img);
    for (auto& v : img) v = -1.0 / (T * T);
    img[(size_t)(T / 3) * T + 5] += 1.0;
    check_image<T>("one pixel", img);
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++) img[(size_t)y * T + x] = (y & 1) ? 0.5 : -0.5;
    check_image<T>("h stripes", img);
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++) img[(size_t)y * T + x] = (x & 1) ? 0.5 : -0.5;
    check_image<T>("v stripes", img);
    for (int y = 0; y < T; y++)
        for (int x = 0; x < T; x++) img[(size_t)y * T + x] = ((x + y) & 1) ? 0.5 : -0.5;
    check_image<T>("checkerboard", img);
}

int main() {
    check_size<64>();
    check_size<128>();
    // the box rule: sides, then position
    const int rule[][8] = {{0, 64, 0, 64, 64, 64, 64, 0},     {1, 65, 3, 67, 64, 65, 67, 0},
                           {0, 63, 0, 64, 64, 100, 100, 1},   {0, 64, 0, 128, 64, 200, 200, 1},
                           {-1, 63, 0, 64, 64, 100, 100, 2},  {0, 64, 37, 101, 64, 100, 100, 2},
                           {37, 101, 0, 64, 64, 100, 100, 2}, {0, 128, 0, 128, 128, 128, 128, 0}};
    for (const auto& r : rule)
        if (win_box_check(r[0], r[1], r[2], r[3], r[4], r[5], r[6]) != r[7]) {
            std::printf("win_box_check(%d %d %d %d, T %d, %d x %d) != %d  FAIL\n", r[0], r[1], r[2], r[3], r[4],
                        r[5], r[6], r[7]);
            g_fail++;
        }
    if (!win_size_ok(64) || !win_size_ok(128) || win_size_ok(32) || win_size_ok(256) || win_size_ok(0)) g_fail++;
    if (g_fail) {
        std::printf("%d FAIL\n", g_fail);
        return 1;
    }
    std::printf("blur window fft OK\n");
    return 0;
}
