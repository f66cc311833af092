// yuv_plan.h -- host side of the YCbCr input stage (no HIP types): validation
// of a phd_yuv_view, its record for the conversion launch, and the
// conversion's host twin.
#pragma once

#include <string>

#include "../../include/photohive_dsp.h"
#include "yuv_view.h"

namespace phd {

// The descriptor's rules (include/photohive_dsp.h); false: the field into *why
bool yuv_view_why(const phd_yuv_view& v, std::string* why);
// The record of a validated view converted into dst (its layout, mode and matrix row)
YuvRec yuv_record(const phd_yuv_view& v, uint8_t* dst);
// The conversion over host memory, one lane (phd_debug_yuv_view_host): 0, or -1 and *why
int yuv_view_host(const phd_yuv_view* view, uint8_t* dst, std::string* why);

}  // namespace phd
