// window_call.h -- the plan of a window call, host only (any C++17 compiler, no HIP).
//
// A window call takes packed RGB8 images of any sizes and, per image, either a
// list of T x T windows (Crop_Boundaries) or a regular grid at steps of `stride`
// (core.py's window_grid).  Every window entry validates, counts and walks its
// windows through WindowPlan -- phd_blur_windows_device, the blur vector entries
// (phd_blurwin.cpp) and the window sharpness entries (phd_sharpwin.cpp) -- and
// their host twins share window_twin_why.  The palette window entries
// (phd_palwin.cpp) take label maps the same way and say "map" where the others
// say "image": the plan's and the ladder's `noun`.  The rules' words live here and
// nowhere else; tests/native/window_call_asan.cpp runs the header alone.
#pragma once

#include <string>
#include <vector>

#include "../../include/photohive_dsp.h"
#include "blur_window.h"

namespace phd {

inline std::string window_too_small(int height, int width, int T) {
    return std::to_string(height) + " x " + std::to_string(width) + " is smaller than the window " +
           std::to_string(T);
}

// The list rule: no list or an empty one is fine; else every box is T x T inside
// the height x width image (win_box_check).
inline bool window_list_why(const Crop_Boundaries* b, int T, int height, int width, std::string* why,
                            const char* noun = "image") {
    if (!b || b->N == 0) return true;
    if (b->N < 0 || !b->top || !b->bottom || !b->left || !b->right) return *why = "bad window list", false;
    for (int k = 0; k < b->N; k++) {
        const int rule = win_box_check(b->top[k], b->bottom[k], b->left[k], b->right[k], T, height, width);
        if (rule == 0) continue;
        const std::string box = "window " + std::to_string(k) + " (top " + std::to_string(b->top[k]) + ", bottom " +
                                std::to_string(b->bottom[k]) + ", left " + std::to_string(b->left[k]) + ", right " +
                                std::to_string(b->right[k]) + ")";
        if (rule == 1) return *why = box + " is not " + std::to_string(T) + " x " + std::to_string(T), false;
        return *why = box + " leaves the " + std::to_string(height) + " x " + std::to_string(width) + " " + noun, false;
    }
    return true;
}

// The windows of a device call.  An entry checks in three steps, each leaving its
// reason in *why: args_why, its own rule for the window size (and cfg), build.
struct WindowPlan {
    const uint8_t* const* d_images;
    const int* heights;
    const int* widths;
    int n_images;
    const Crop_Boundaries* const* windows;   // per image, NULL entries allowed; the grid entries have none
    bool lists;                              // windows[i]'s boxes, else the grid at `stride`
    int T, stride;
    const char* noun;                        // what the messages call an input: "image", or "map"
    std::vector<long long> count;            // windows of image i
    long long total = 0;                     // at most 2^31 - 1 after build

    WindowPlan(const uint8_t* const* d_images_, const int* heights_, const int* widths_, int n_images_,
               const Crop_Boundaries* const* windows_, bool lists_, int window, int stride_,
               const char* noun_ = "image")
        : d_images(d_images_), heights(heights_), widths(widths_), n_images(n_images_), windows(windows_),
          lists(lists_), T(window), stride(stride_), noun(noun_) {}

    // rest: whether the entry's other required pointers are there
    bool args_why(bool rest, std::string* why) const {
        if (!d_images || !heights || !widths || (lists && !windows) || !rest) return *why = "NULL argument", false;
        if (n_images <= 0) return *why = std::string("n_") + noun + "s must be positive", false;
        return true;
    }

    // Per image in order: the pointer, the size, the list or the grid's count
    // (window_grid's rule), then d_out[i] (the entry's array `out_name`; nullptr:
    // the entry has none) wherever the image has a window, then the running total.
    bool build(const void* const* d_out, const char* out_name, std::string* why) {
        if (!lists && stride <= 0) return *why = "stride must be positive, not " + std::to_string(stride), false;
        count.assign(n_images, 0);
        gws_.assign(n_images, 0);
        total = 0;
        for (int i = 0; i < n_images; i++) {
            const std::string img = std::string(noun) + " " + std::to_string(i) + ": ";
            if (!d_images[i]) return *why = img + "NULL " + noun, false;
            if (heights[i] < T || widths[i] < T)
                return *why = img + window_too_small(heights[i], widths[i], T), false;
            if (lists) {
                std::string list_why;
                if (!window_list_why(windows[i], T, heights[i], widths[i], &list_why, noun))
                    return *why = img + list_why, false;
                count[i] = windows[i] ? windows[i]->N : 0;
            } else {
                gws_[i] = (widths[i] - T) / stride + 1;
                count[i] = ((long long)(heights[i] - T) / stride + 1) * gws_[i];
            }
            if (d_out && count[i] > 0 && !d_out[i])
                return *why = img + "NULL " + out_name + " for " + std::to_string(count[i]) + " windows", false;
            total += count[i];                               // both below 2^62: no overflow before the check
            if (total > 0x7FFFFFFFLL) return *why = "too many windows", false;
        }
        return true;
    }

    // fn(i, k, top, left) for window k of image i, in the table's order (built plans only)
    template <class Fn>
    void for_each(Fn fn) const {
        for (int i = 0; i < n_images; i++) {
            const long long n = count[i], gw = gws_[i];
            if (n == 0) continue;                            // (its list may be NULL)
            if (lists) {
                const int *top = windows[i]->top, *left = windows[i]->left;
                for (long long k = 0; k < n; k++) fn(i, k, (long long)top[k], (long long)left[k]);
            } else {
                for (long long k = 0; k < n; k++) fn(i, k, (k / gw) * stride, (k % gw) * stride);
            }
        }
    }

private:
    std::vector<long long> gws_;             // the grid's columns of image i
};

// The host twins' ladder over one image: the image, the twin's own rule for the
// window size (size_why: its refusal, or empty), the size, the list, and the
// outputs wherever there is a window (no_outputs: the twin's words for theirs).
inline bool window_twin_why(const uint8_t* rgb, int height, int width, const Crop_Boundaries* windows, int T,
                            const std::string& size_why, bool outputs, const char* no_outputs, std::string* why,
                            const char* noun = "image") {
    if (!rgb) return *why = std::string("NULL ") + noun, false;
    if (!size_why.empty()) return *why = size_why, false;
    if (height < T || width < T) return *why = window_too_small(height, width, T), false;
    if (!window_list_why(windows, T, height, width, why, noun)) return false;
    if (windows && windows->N > 0 && !outputs) return *why = no_outputs, false;
    return true;
}

}  // namespace phd
