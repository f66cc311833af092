// blur_window.h -- the window blur's plan, box rule, LDS layout and finish, host + device.
//
// A window is a T x T crop (T = 64 or 128) of a packed RGB8 image: a
// Crop_Boundaries box with bottom - top == right - left == T inside the image
// (crop_image, src/image_processing.c:244-266).  Its values are the reference's
// get_blur_profile on that crop: rgb2pgm - avg (src/image_processing.c:505-512,
// src/blur_profile.c:233-238), the unnormalised r2c 2-D DFT with p = re re +
// im im (src/fft_processing.c:18-63), pgm_normalize_fft (:173-213) and the
// polar binning of calculate_blur_profile (src/blur_profile.c:34-126) over a
// T x (T/2+1) half spectrum.
//
// The whole transform lives in T*T/2 complex values (128 KiB at T = 128, plus
// one element of padding per row pair):
//  * rows 2p and 2p+1 are the real and imaginary parts of one complex row
//    transform Z of length T (row pair p at buf[p P .. p P + T), P = win_pitch(T));
//  * the two rows' half spectra are separated in place: with A, B the spectra
//    of the two real rows, A[k] = (Z[k] + conj Z[T-k]) / 2 goes to slot k and
//    B[k] = (Z[k] - conj Z[T-k]) / (2i) to slot T-k, 0 < k < T/2;
//  * columns 0 (DC) and T/2 (Nyquist) are real in every row, so they are packed
//    as one complex column DC + i Nyquist: row 2p's pair in slot 0, row 2p+1's
//    in slot T/2 of row pair p;
//  * that leaves T/2 column transforms of length T: columns 1 .. T/2-1 and the
//    packed column, whose transform C separates as D[v] = (C[v] + conj C[T-v])
//    / 2 (DC column) and N[v] = (C[v] - conj C[T-v]) / (2i) (Nyquist column).
// win_col_index is where row y of column k sits; win_spectrum reads element
// (row u, column x <= T/2) of the finished half spectrum.  The kernel
// (blur_windows.hip: k_window_blur) and the host twin (window_bins_host, same
// file, and tests/native/blur_window_fft.cpp) run the same passes through
// win_bfly_load / win_bfly_store: the twin butterfly by butterfly, the kernel
// one or two butterflies per thread with a barrier between load and store.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

// The plan's constants and the box rule build with any host compiler
// (phd_blurwin.cpp); the index maps and butterflies need fft_engine.h and so
// the device compiler (either half: blur_windows.hip, tests/native/).
#if defined(__HIPCC__)
#include "fft_engine.h"
#define WIN_HD __host__ __device__ __forceinline__
#else
#define WIN_HD inline
#endif

namespace phd {

// ---- the plan of a window size ---------------------------------------------------
// Two Stockham passes per dimension (radices R0 then R1, T = R0 R1) over T/2
// transforms; kThreads divides both passes' butterflies ((T/2) T/R): one round
// per thread, two in the radix-8 pass at T = 128.
template <int T>
struct WinPlan;
template <>
struct WinPlan<64> {
    static constexpr int kThreads = 256, R0 = 8, R1 = 8;
};
template <>
struct WinPlan<128> {
    static constexpr int kThreads = 512, R0 = 16, R1 = 8;
};
// Row pairs are win_pitch(T) = T + kWinPad elements apart in LDS.  With a pitch of T the
// 8 lanes of a 16-byte store group of a row pass fall on one 128-byte bank row
// (their elements are a multiple of 8 apart); one element of padding per row
// pair and adjacent lanes on adjacent row pairs spread them over all banks
// (measured against PHD_WIN_PAD=0, DESIGN.md section 24:
// make -C photohive_dsp_amd/csrc variant V=nopad VFLAGS=-DPHD_WIN_PAD=0).
#ifndef PHD_WIN_PAD
#define PHD_WIN_PAD 1
#endif
constexpr int kWinPad = PHD_WIN_PAD;
constexpr int win_pitch(int T) { return T + kWinPad; }
constexpr int kWinMaxBins = 2880;                    // na * nr at most: 22.5 KiB of u64 bins in LDS
WIN_HD bool win_size_ok(int T) { return T == 64 || T == 128; }
// complex elements of a window's LDS spectrum
constexpr int win_elems(int T) { return (T / 2) * win_pitch(T); }

// ---- the box rule ---------------------------------------------------------------
// 0: a window of the height x width image; 1: its sides are not T; 2: it leaves
// the image.
WIN_HD int win_box_check(int top, int bottom, int left, int right, int T, int height, int width) {
    if ((long long)bottom - top != T || (long long)right - left != T) return 1;
    if (top < 0 || left < 0 || bottom > height || right > width) return 2;
    return 0;
}

// ---- the finish: flat bins and vectors ----------------------------------------------
// From a window's nbins fixed-point bin sums and its spectrum maximum to the
// reference's bins and ten Blur_Vectors, as rows that the kernel
// (blur_windows.hip: k_window_vectors) runs one thread per bin, per angle or per
// maximum with barriers between them and the host twin (phd_blurwin.cpp:
// window_finish_host) runs in sequence.  Every row is finish_blur's
// (phd_assemble.cpp) or vectorize_blur's (phd_blur.cpp) expression, operation for
// operation and sum for sum in the reference's order: plain IEEE fp64 and fp32
// operations, no fma.  Only the log differs between the two sides (the C library's
// on the host, the device library's in the kernel).
struct WinVector {             // Blur_Vector's layout (src/blur_profile.h:52-55)
    int angle;
    float magnitude;
};
constexpr int kWinVectors = 10;                      // initialize_blur_vector_group(10), src/blur_profile.c:328
// pgm_normalize_fft's G_s (src/fft_processing.c:192); infinite for fft_max == 0, where every sum is 0
WIN_HD double win_gs(double fft_max) { return 1 / (2 * log(sqrt(fft_max) + 1)); }
// bin b of calculate_blur_profile (src/blur_profile.c:106-116) from its fixed-point sum of log p
WIN_HD double win_flat_bin(unsigned long long sum, double scale, double gs, unsigned count) {
    const double q = (double)count;
    const double s = sum == 0ull ? 0.0 : (double)sum / scale * gs;
    return q != 0 ? s / q : 0;
}
// tot[i] of vectorize_blur_profile (src/blur_profile.c:343-346), rc = nr / denom
WIN_HD double win_angle_total(const double* flat, int nr, int rc, int i) {
    double t = 0.0;
    for (int j = 0; j < rc; j++) t += flat[(size_t)i * nr + j];
    return t;
}
// avg (:341-349)
WIN_HD double win_angle_avg(const double* tot, int na) {
    double avg = 0;
    for (int i = 0; i < na; i++) avg += tot[i];
    return avg / na;
}
// convolve_1d with the 5-tap box of ones, then / 5 (src/filtering.c:12-24)
WIN_HD double win_smooth(const double* tot, int na, int i) {
    double s = 0.0;
    for (int j = 0; j < 5; j++) s += tot[((i - j) % na + na) % na] * 1.0;
    return s / 5;
}
// The local maxima above thr = avg * fft_streak_thresh in increasing angle, ten at
// most (:358-379).  na >= 2: the rules read sm[1] and sm[na - 2].
WIN_HD int win_maxima(const double* sm, int na, double thr, int* idx) {
    int m = 0;
    if (sm[0] > sm[na - 1] && sm[0] > sm[1] && sm[0] > thr) idx[m++] = 0;
    for (int i = 1; i < na - 1 && m < kWinVectors; i++)
        if (sm[i] > sm[i - 1] && sm[i] > sm[i + 1] && sm[i] > thr) idx[m++] = i;
    if (m < kWinVectors && sm[na - 1] > sm[na - 2] && sm[na - 1] > sm[0] && sm[na - 1] > thr) idx[m++] = na - 1;
    return m;
}
// The vector of the maximum at angle bin imax (:384-414)
WIN_HD WinVector win_vector(const double* flat, int na, int nr, int rc, double avg, double mag, int imax) {
    WinVector v;
    v.angle = 0;
    v.magnitude = 0.0f;
    const int a = (imax + na / 2) % na;
    const double* sig = flat + (size_t)a * nr;
    double bavg = 0;
    for (int j = 0; j < rc; j++) bavg += sig[j];
    if (bavg > avg) return v;
    int rmax = nr;
    for (int j = 0; j < nr; j++)
        if (sig[j] < mag) {
            rmax = j;
            break;
        }
    v.magnitude = ((float)rmax / (float)nr);
    v.angle = (int)(180 * ((float)a / (float)na) - 90);
    return v;
}

#if defined(__HIPCC__)
// ---- index maps -----------------------------------------------------------------
// pixel (y, x) of the window before the row transforms: the double at
// 2 * win_pixel_slot + (y & 1) of the buffer seen as doubles
template <int T>
WIN_HD int win_pixel_slot(int y, int x) { return (y >> 1) * win_pitch(T) + x; }
// element j of row transform m (row pair m)
template <int T>
struct WinRowIdx {
    static constexpr int M = T / 2;
    WIN_HD static int at(int m, int j) { return m * win_pitch(T) + j; }
    // butterfly b of a pass of NB butterflies per transform: adjacent b, adjacent row
    // pairs (a pitch apart: conflict-free with the padding; with none, adjacent elements)
    WIN_HD static void split(int b, int NB, int& m, int& bb) {
        if constexpr (kWinPad % 2 != 0) {
            bb = b / M;
            m = b - bb * M;
        } else {
            m = b / NB;
            bb = b - m * NB;
        }
    }
};
// row y of column k after the separation (k = 0: the packed DC + i Nyquist column)
template <int T>
WIN_HD int win_col_index(int y, int k) {
    return (y >> 1) * win_pitch(T) + ((y & 1) ? (k == 0 ? T / 2 : T - k) : k);
}
template <int T>
struct WinColIdx {
    static constexpr int M = T / 2;
    WIN_HD static int at(int m, int j) { return win_col_index<T>(j, m); }
    // adjacent b, adjacent columns: adjacent (or mirrored adjacent) elements
    WIN_HD static void split(int b, int, int& m, int& bb) {
        bb = b / M;
        m = b - bb * M;
    }
};

// ---- one butterfly of a pass ------------------------------------------------------
// Pass (R, NS) of the T/2 transforms of length T laid out by Idx: butterfly b in
// [0, (T/2) (T/R)) reads elements bb + r T/R of its transform, multiplies input
// r by W_{NS R}^{(bb mod NS) r} = tw[(bb mod NS) r T / (NS R)] (tw[e] = W_T^e, e
// < T), runs the R-point DFT and writes output k to (bb / NS) NS R + bb mod NS +
// k NS.  Every load of a pass comes before any of its stores.
template <int T, int R, int NS, class Idx>
WIN_HD void win_bfly_load(const double2* buf, const double2* tw, int b, double2 (&v)[R]) {
    constexpr int NB = T / R;
    int m, bb;
    Idx::split(b, NB, m, bb);
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = buf[Idx::at(m, bb + r * NB)];
    if constexpr (NS > 1) {
        constexpr int step = T / (NS * R);
        const int j = (bb % NS) * step;
#pragma unroll
        for (int r = 1; r < R; r++) v[r] = fe::cmul(v[r], tw[j * r]);
    }
    fe::dft<R>(v);
}
template <int T, int R, int NS, class Idx>
WIN_HD void win_bfly_store(double2* buf, int b, const double2 (&v)[R]) {
    constexpr int NB = T / R;
    int m, bb;
    Idx::split(b, NB, m, bb);
    const int jh = bb / NS, jm = bb - jh * NS;
    const int base = jh * NS * R + jm;
#pragma unroll
    for (int k = 0; k < R; k++) buf[Idx::at(m, base + k * NS)] = v[k];
}
template <int T, int R>
constexpr int win_butterflies() { return (T / 2) * (T / R); }

// ---- the row pairs' separation ------------------------------------------------------
// item i in [0, T/2 * T/2): row pair p = i / (T/2), k = i % (T/2); k = 0 packs
// the pair's DC and Nyquist values.  An item reads and writes its own two slots.
template <int T>
WIN_HD void win_separate(double2* buf, int i) {
    const int p = i / (T / 2), k = i - p * (T / 2);
    double2* row = buf + p * win_pitch(T);
    if (k == 0) {
        const double2 z0 = row[0], zh = row[T / 2];
        row[0] = make_double2(z0.x, zh.x);           // row 2p: A[0] + i A[T/2]
        row[T / 2] = make_double2(z0.y, zh.y);       // row 2p+1: B[0] + i B[T/2]
    } else {
        const double2 zk = row[k], zm = row[T - k];
        row[k] = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
        row[T - k] = make_double2(0.5 * (zk.y + zm.y), -0.5 * (zk.x - zm.x));
    }
}

// ---- the finished half spectrum -------------------------------------------------------
// X[u][x], 0 <= u < T, 0 <= x <= T/2, after the column passes
template <int T>
WIN_HD double2 win_spectrum(const double2* buf, int u, int x) {
    if (x > 0 && x < T / 2) return buf[win_col_index<T>(u, x)];
    const double2 c = buf[win_col_index<T>(u, 0)], cm = buf[win_col_index<T>((T - u) & (T - 1), 0)];
    return x == 0 ? make_double2(0.5 * (c.x + cm.x), 0.5 * (c.y - cm.y))
                  : make_double2(0.5 * (c.y + cm.y), -0.5 * (c.x - cm.x));
}

// avg = (Br + Bg + Bb) / 3 (src/interface.c:78) of a window from its exact integer
// channel sums, as k_fft_rows forms an image's
template <int T>
WIN_HD double win_avg(unsigned long long sr, unsigned long long sg, unsigned long long sb) {
    const double n = (double)T * (double)T;
    return ((double)sr / 255.0 / n + (double)sg / 255.0 / n + (double)sb / 255.0 / n) / 3.0;
}
// rgb2pgm (src/image_processing.c:509), then remove_dc_bias (src/blur_profile.c:236)
WIN_HD double win_luma(const double* k255, unsigned r, unsigned g, unsigned b, double avg) {
    return (0.299 * k255[r] + 0.587 * k255[g] + 0.114 * k255[b]) - avg;
}

// ---- the passes run one butterfly at a time (host) --------------------------------------
template <int T, int R, int NS, class Idx>
inline void win_pass_host(double2* buf, const double2* tw, double2* tmp) {
    constexpr int B = win_butterflies<T, R>();
    for (int b = 0; b < B; b++) {
        double2 v[R];
        win_bfly_load<T, R, NS, Idx>(buf, tw, b, v);
        for (int k = 0; k < R; k++) tmp[(size_t)b * R + k] = v[k];
    }
    for (int b = 0; b < B; b++) {
        double2 v[R];
        for (int k = 0; k < R; k++) v[k] = tmp[(size_t)b * R + k];
        win_bfly_store<T, R, NS, Idx>(buf, b, v);
    }
}
// buf: win_elems(T) values holding the packed row pairs; tmp: as many
template <int T>
inline void win_transform_host(double2* buf, const double2* tw, double2* tmp) {
    using P = WinPlan<T>;
    win_pass_host<T, P::R0, 1, WinRowIdx<T>>(buf, tw, tmp);
    win_pass_host<T, P::R1, P::R0, WinRowIdx<T>>(buf, tw, tmp);
    for (int i = 0; i < (T / 2) * (T / 2); i++) win_separate<T>(buf, i);
    win_pass_host<T, P::R0, 1, WinColIdx<T>>(buf, tw, tmp);
    win_pass_host<T, P::R1, P::R0, WinColIdx<T>>(buf, tw, tmp);
}
// tw[e] = W_T^e = exp(-2 pi i e / T), e < T, rounded from long double
inline void win_twiddles(int T, double2* tw) {
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int e = 0; e < T; e++) {
        // exact at the multiples of T / 4; the octant symmetries hold to the rounding of cosl / sinl
        const long double a = two_pi * (long double)e / (long double)T;
        double c = (double)__builtin_cosl(a), s = (double)__builtin_sinl(a);
        if (e % (T / 4) == 0) {
            const int q = e / (T / 4);
            c = q == 0 ? 1.0 : (q == 2 ? -1.0 : 0.0);
            s = q == 1 ? 1.0 : (q == 3 ? -1.0 : 0.0);
        }
        tw[e] = make_double2(c, -s);
    }
}
#endif  // __HIPCC__

}  // namespace phd
