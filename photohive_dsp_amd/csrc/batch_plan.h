// batch_plan.h -- host side of the batch entries' grouping (no HIP types):
// which images of a call run together, and how one run splits over two lanes.
#pragma once

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

namespace phd {

constexpr long kMixedGroupMax = 1024;                         // images per run, any size

// Image indices grouped by size (groups in order of first appearance, each in
// index order), at most `cap` per group, or (pix_cap > 0) as many as fit
// pix_cap pixels when that is more: one batched run per group.
inline std::vector<std::vector<int>> size_groups(const int* heights, const int* widths, int n, int cap,
                                                 long pix_cap = 0) {
    std::vector<std::vector<int>> g;
    std::map<std::pair<int, int>, int> open;                  // size -> its group still filling
    for (int i = 0; i < n; i++) {
        const auto key = std::make_pair(heights[i], widths[i]);
        auto it = open.find(key);
        const long npix = (long)heights[i] * widths[i];
        const int c = std::max<long>(cap, std::min<long>(kMixedGroupMax, pix_cap / std::max(npix, 1L)));
        if (it == open.end() || (int)g[it->second].size() >= c) {
            open[key] = (int)g.size();
            g.emplace_back();
        }
        g[open[key]].push_back(i);
    }
    return g;
}

// Lane 0's part of an m-image run split over two lanes: 51.2 % (262 of 512).
// With equal halves lane 1 finished ~1.6 ms after lane 0 per 512-image call at
// 4000x3000, and the call took 56.2 ms against 55.8-55.9 with 262 / 250
// (56.0-56.3 with 268 / 244; profiles/r05/lane_split_ab.log)
inline int lane_split(int m) { return (int)(((long)m * 131 + 128) / 256); }

}  // namespace phd
