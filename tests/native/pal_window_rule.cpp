// Prints pal_window.h's copies rule as the library compiles it
// (tests/test_window_palette_host.py): per window size one line
//   T <T> max <pw_max_copies> changes <counters at which pw_copies changes ...>
// and one line "lds <T> <largest pw_lds_words over 1..4097 counters> <pw_lds_words(4097)>",
// after checking for every counters in 1..4097 that the copies are a power of two
// and fit pw_lds_words, and that pw_lds_words is a multiple of 4 within
// kPalWinMaxLdsWords.
#include <cstdio>
#include <initializer_list>

#include "../../photohive_dsp_amd/csrc/pal_window.h"

int main() {
    int bad = 0;
    for (int T : {16, 32, 64, 128}) {
        printf("T %d max %d changes", T, phd::pw_max_copies(T));
        int most = 0;
        for (int nc = 1; nc <= phd::kPalWinMaxCounters; nc++) {
            const int c = phd::pw_copies(nc, T), words = phd::pw_lds_words(nc, T);
            if (nc > 1 && c != phd::pw_copies(nc - 1, T)) printf(" %d", nc);
            if (c < 1 || (c & (c - 1)) || c * phd::pw_copy_stride(nc) > words || words % 4 ||
                words > phd::kPalWinMaxLdsWords || phd::pw_copy_stride(nc) < nc || !(phd::pw_copy_stride(nc) & 1))
                bad++;
            most = words > most ? words : most;
        }
        printf("\nlds %d %d %d\n", T, most, phd::pw_lds_words(phd::kPalWinMaxCounters, T));
    }
    if (bad) fprintf(stderr, "FAIL: %d counter values break the rule's invariants\n", bad);
    return bad ? 1 : 0;
}
