// Host check of fft_engine.h's butterflies (tests/test_fft_butterflies.py),
// built from the header's host half with no GPU: dft<R> for the radices with
// coprime factors (the prime-factor form, 6 10 12 15 20 30) and, so the
// unchanged ones stay covered, 8 9 16 25, against a direct fp64 DFT
// (long-double twiddles) on random inputs; the prime-factor index maps as
// permutations; and a two-lane emulation of the split last pass (split_twiddle,
// split_half, split_join; the DPP exchange as a swap of the two lanes' arrays)
// for R = 20 with inter-pass twiddles.  Bound: 1e-14 of the largest output.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../photohive_dsp_amd/csrc/fft_engine.h"

using namespace phd::fe;

static int g_fail = 0;
static std::mt19937_64 g_rng(20240611);

static double rnd() { return std::uniform_real_distribution<double>(-1.0, 1.0)(g_rng); }

// X[k] = sum_n x[n] e^{-2 pi i n k / R}
static void direct_dft(const double2* x, double2* X, int R) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < R; k++) {
        long double re = 0, im = 0;
        for (int n = 0; n < R; n++) {
            const long double a = two_pi * (long double)((n * k) % R) / (long double)R;
            const long double c = cosl(a), s = -sinl(a);
            re += x[n].x * c - x[n].y * s;
            im += x[n].x * s + x[n].y * c;
        }
        X[k] = make_double2((double)re, (double)im);
    }
}

static void compare(const char* what, int R, const double2* got, const double2* want) {
    double mx = 0, err = 0;
    for (int k = 0; k < R; k++) {
        mx = std::fmax(mx, std::hypot(want[k].x, want[k].y));
        err = std::fmax(err, std::hypot(got[k].x - want[k].x, got[k].y - want[k].y));
    }
    const bool ok = err <= 1e-14 * mx;
    std::printf("%s R=%d max err %.3e of max%s\n", what, R, err / mx, ok ? "" : "  FAIL");
    if (!ok) g_fail++;
}

template <int R>
static void check_dft() {
    for (int rep = 0; rep < 50; rep++) {
        double2 v[R], x[R], X[R];
        for (int n = 0; n < R; n++) v[n] = x[n] = make_double2(rnd(), rnd());
        dft<R>(v);
        direct_dft(x, X, R);
        if (rep == 0 || rep == 49) compare("dft", R, v, X);
        else {
            double mx = 0, err = 0;
            for (int k = 0; k < R; k++) {
                mx = std::fmax(mx, std::hypot(X[k].x, X[k].y));
                err = std::fmax(err, std::hypot(v[k].x - X[k].x, v[k].y - X[k].y));
            }
            if (!(err <= 1e-14 * mx)) compare("dft", R, v, X);
        }
    }
}

template <int A, int B>
static void check_maps() {
    static_assert(gcd_of(A, B) == 1, "coprime");
    bool in[A * B] = {}, out[A * B] = {};
    bool ok = true;
    for (int a = 0; a < A; a++)
        for (int b = 0; b < B; b++) {
            const int n = pfa_in<A, B>(a, b), k = pfa_out<A, B>(a, b);
            if (n < 0 || n >= A * B || k < 0 || k >= A * B || in[n] || out[k]) {
                ok = false;
                continue;
            }
            in[n] = out[k] = true;
            // the CRT: output k has residues (a, b)
            if (k % A != a || k % B != b) ok = false;
        }
    std::printf("maps %d x %d %s\n", A, B, ok ? "are permutations" : "FAIL");
    if (!ok) g_fail++;
}

// One butterfly of radix R = 2 M at position jm of NS (twiddle w = W_{NS R}^jm)
// on two emulated lanes, as SplitPass::compute: lane h holds inputs 2 j + h,
// twiddles them (split_twiddle), runs split_half, takes the other lane's values
// and joins.
template <int R>
static void check_split(int NS, int jm) {
    constexpr int M = R / 2;
    const long double two_pi = 6.283185307179586476925286766559005768L;
    double2 x[R], xt[R], X[R], got[R];
    for (int n = 0; n < R; n++) {
        x[n] = make_double2(rnd(), rnd());
        const long double a = two_pi * (long double)(jm * n) / (long double)(NS * R);
        const long double c = cosl(a), s = -sinl(a);
        xt[n] = make_double2((double)(x[n].x * c - x[n].y * s), (double)(x[n].x * s + x[n].y * c));
    }
    direct_dft(xt, X, R);
    // the pass's table entry, as the host builds it (get_ct_twiddles)
    const long double a1 = two_pi * (long double)jm / (long double)(NS * R);
    const double2 w = make_double2((double)cosl(a1), (double)-sinl(a1));
    double2 lane[2][M];
    for (int h = 0; h < 2; h++) {
        for (int j = 0; j < M; j++) lane[h][j] = x[2 * j + h];
        split_twiddle<M>(lane[h], w, h);
        split_half<M>(lane[h], h);
    }
    for (int h = 0; h < 2; h++)
        for (int k = 0; k < M; k++) got[k + h * M] = split_join(lane[h][k], lane[h ^ 1][k], h);
    compare("split pass", R, got, X);
}

int main() {
    check_dft<6>();
    check_dft<10>();
    check_dft<12>();
    check_dft<15>();
    check_dft<20>();
    check_dft<30>();
    check_dft<8>();
    check_dft<9>();
    check_dft<16>();
    check_dft<25>();
    check_maps<3, 2>();
    check_maps<5, 2>();
    check_maps<4, 3>();
    check_maps<5, 3>();
    check_maps<4, 5>();
    check_maps<5, 6>();
    for (int i = 0; i < 20; i++) check_split<20>(150, (i * 37) % 150);
    check_split<20>(1, 0);
    if (g_fail) {
        std::printf("%d checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("fft butterflies OK\n");
    return 0;
}
