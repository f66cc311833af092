// views_plan.h -- host side of the image-view input stage (no HIP types):
// validation of a phd_image_view and its record for the pack launch.
#pragma once

#include <string>

#include "../../include/photohive_dsp.h"
#include "pack_view.h"

namespace phd {

// The descriptor's rules (include/photohive_dsp.h); false: the field into *why
bool view_why(const phd_image_view& v, std::string* why);
// The record of a validated view packed into dst (its kind: pack_kind)
PackRec pack_record(const phd_image_view& v, uint8_t* dst);

}  // namespace phd
