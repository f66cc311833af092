// views_plan.h -- host side of the image-view input stage (no HIP types):
// validation of a phd_image_view and its record for the pack launch; the
// same for a phd_typed_view and the decode launches, and the decode's host twin.
#pragma once

#include <string>

#include "../../include/photohive_dsp.h"
#include "pack_view.h"
#include "decode_view.h"

namespace phd {

// The descriptor's rules (include/photohive_dsp.h); false: the field into *why
bool view_why(const phd_image_view& v, std::string* why);
// The record of a validated view packed into dst (its kind: pack_kind)
PackRec pack_record(const phd_image_view& v, uint8_t* dst);


// The typed descriptor's rules (include/photohive_dsp.h); false: the field into *why
bool typed_view_why(const phd_typed_view& v, std::string* why);
// The divisor of a validated view: max_value, or (0) the type's own
double typed_max_value(const phd_typed_view& v);
// A PHD_ELEM_U8 view at the default maximum: an 8-bit view as it stands
bool typed_is_u8_view(const phd_typed_view& v);
phd_image_view typed_as_u8_view(const phd_typed_view& v);
// PHD_VIEW_SNAP_U8 applies: F16 or F32 at the default maximum with the flag set
bool typed_snaps(const phd_typed_view& v);
// The snap tables on the host: 256 halves (bits) | 256 floats, (T)((double)j / 255.0)
constexpr size_t kSnapF32Offset = 256 * sizeof(uint16_t);
constexpr size_t kSnapBytes = kSnapF32Offset + 256 * sizeof(float);
const uint8_t* snap_tables();
// The record of a validated view decoded into planes and / or rgb8 (either may
// be nullptr); snap: the tables' base (snap_tables() or their device copy)
DecodeRec decode_record(const phd_typed_view& v, double* planes, uint8_t* rgb8, const uint8_t* snap);
// The decode over host memory, one lane (phd_debug_decode_view_host): 0, or -1 and *why
int decode_view_host(const phd_typed_view* view, double* planes, uint8_t* rgb8, int* is_u8, std::string* why);

}  // namespace phd
