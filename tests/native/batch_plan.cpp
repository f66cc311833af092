// batch_plan.h alone (built with ASan + UBSan by tests/test_batch_plan.py):
// the size groups of the mixed batch entries and the two-lane split.
#include <cstdio>
#include <vector>

#include "../../photohive_dsp_amd/csrc/batch_plan.h"

using phd::kMixedGroupMax;
using phd::lane_split;
using phd::size_groups;

static int fails = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            fails++;                                                    \
        }                                                               \
    } while (0)

static bool ascending(const std::vector<int>& g) {
    for (size_t k = 1; k < g.size(); k++)
        if (g[k] <= g[k - 1]) return false;
    return true;
}

int main() {
    {   // tests/test_gpu_round3.py::test_mixed_batch_groups_past_64_images: 35 + 3 + 35
        std::vector<int> hs, ws;
        for (int i = 0; i < 73; i++) {
            const int s = i >= 35 && i < 38 ? 400 : 352;
            hs.push_back(s);
            ws.push_back(s);
        }
        const auto g = size_groups(hs.data(), ws.data(), 73, 64, 64L * 12000000L);
        CHECK(g.size() == 2);
        CHECK(g[0].size() == 70 && g[0].front() == 0 && g[0][35] == 38 && g[0].back() == 72 && ascending(g[0]));
        CHECK(g[1].size() == 3 && g[1][0] == 35 && g[1][1] == 36 && g[1][2] == 37);
    }
    {   // a size that reaches the cap opens a second group; the other size's group stays open
        const int hs[] = {400, 400, 500, 400, 400, 400, 500, 400}, ws[] = {600, 600, 500, 600, 600, 600, 500, 600};
        const auto g = size_groups(hs, ws, 8, 4);
        CHECK(g.size() == 3);
        CHECK((g[0] == std::vector<int>{0, 1, 3, 4}));
        CHECK((g[1] == std::vector<int>{2, 6}));
        CHECK((g[2] == std::vector<int>{5, 7}));
        // the same height with another width is another size
        const int ws2[] = {600, 601, 600, 601, 600, 601, 600, 601}, hs2[] = {400, 400, 400, 400, 400, 400, 400, 400};
        CHECK(size_groups(hs2, ws2, 8, 64).size() == 2);
    }
    {   // cap wins over a pixel budget that holds less than cap images (here: none)
        std::vector<int> hs(40, 4000), ws(40, 3000);
        const auto g = size_groups(hs.data(), ws.data(), 40, 16, 1L);
        CHECK(g.size() == 3 && g[0].size() == 16 && g[1].size() == 16 && g[2].size() == 8);
        // and the budget over cap when it holds more: 64 of 12 MP are 192 of 2000 x 2000
        std::vector<int> s4(200, 2000);
        const auto g4 = size_groups(s4.data(), s4.data(), 200, 64, 64L * 12000000L);
        CHECK(g4.size() == 2 && g4[0].size() == 192 && g4[1].size() == 8);
    }
    {   // kMixedGroupMax: 1,100 images of 352 x 352 (the budget alone would hold 6,198)
        std::vector<int> s(1100, 352);
        const auto g = size_groups(s.data(), s.data(), 1100, 64, 64L * 12000000L);
        CHECK(kMixedGroupMax == 1024);
        CHECK(g.size() == 2 && g[0].size() == 1024 && g[1].size() == 76 && g[1].front() == 1024);
    }
    CHECK(size_groups(nullptr, nullptr, 0, 64).empty());
    CHECK(lane_split(512) == 262);
    CHECK(lane_split(16) == 8);
    for (int m = 16; m <= 1024; m++) {
        const int a = lane_split(m), b = m - a;
        CHECK(a > 0 && b > 0 && a + b == m);
    }
    if (fails) return 1;
    printf("batch plan OK\n");
    return 0;
}
