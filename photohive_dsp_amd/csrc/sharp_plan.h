// sharp_plan.h -- host side of the batched sharpness stage (no HIP types):
// the box table of a call and the host twin of its kernels.
#pragma once

#include <string>
#include <vector>

#include "../../include/photohive_dsp.h"
#include "sharp_tiles.h"

namespace phd {

// The box table of one launch: every box of every image in image order, and
// the running count of their slices (prefix[k] = first block of box k,
// prefix[boxes.size()] = blocks of the launch).
struct SharpPlan {
    std::vector<SharpBox> boxes;
    std::vector<int> prefix;
    int max_boxes = 0;                 // the largest box count of one image
};
// crops: n entries, NULL = no boxes (validated boxes only: crops_why).  flat:
// slots count over the whole call (phd_sharpness_batch_device's flat output);
// else a box's slot is its index in its image.  false: too many slices.
bool sharp_plan(const Crop_Boundaries* const* crops, int n, bool flat, SharpPlan* p);
// check_crops' rules without the side effects (the message into *why)
bool crops_why(const Crop_Boundaries* cb, int height, int width, std::string* why);
// one box on the host with the kernels' tile plan and merge order
SharpPart sharp_box_host(const uint8_t* rgb, int width, const SharpBox& b, const double* k255);
// get_variance_sharpness' last lines (src/filtering.c:170-175) from the box's sums
inline double sharp_value(double sum, double m2, int cw, int ch) {
    const double cn = (double)((long)cw * ch);
    const double avg = sum / cn;
    const double var = m2 / cn;
    return var / avg;
}

}  // namespace phd
