/* photohive_dsp.h -- C-ABI of PhotoHive_DSP_lib/libreport_data.so (MI355X build).
 *
 * Drop-in for the reference's libreport_data.so: the three legacy entry points
 * keep their exact signatures and struct layouts, so the reference's own
 * ctypes binding (/root/reference/lib.py:20-37, structures.py:6-106) loads
 * this library unchanged.  Behind them the hot path (rgb2hsv, RGB statistics,
 * HSV-grid colour palette, 2-D FFT magnitude + polar blur binning) runs as
 * hand-written HIP kernels on a gfx950 GPU; there is no CPU fallback -- without
 * a usable GPU every entry point returns NULL / a negative status and
 * phd_last_error() says why.
 *
 * Everything here is plain C: pointers, ints and doubles, no HIP/torch types.
 */
#ifndef PHOTOHIVE_DSP_H
#define PHOTOHIVE_DSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- struct layouts: byte-identical to the reference ------------------- */
typedef double Pixel;                                  /* src/types.h:5 */

typedef struct Pixel_HSV {                             /* src/image_processing.h:12-17 */
    int parent_id;
    double h, s, v;
} Pixel_HSV;

typedef struct Image_RGB {                             /* src/image_processing.h:31-36 */
    int height, width;
    Pixel *r, *g, *b;
} Image_RGB;

typedef struct Image_PGM {                             /* src/image_processing.h:63-66 */
    int height, width;
    Pixel* data;
} Image_PGM;

typedef struct RGB_Statistics {                        /* src/image_processing.h:73-80 */
    Pixel Br, Bg, Bb, Cr, Cg, Cb;
} RGB_Statistics;

typedef struct Crop_Boundaries {                       /* src/image_processing.h:92-98 */
    int N;
    int *top, *bottom, *left, *right;
} Crop_Boundaries;

typedef struct Color_Palette {                         /* src/color_quantization.h:11-15 */
    int N;
    Pixel_HSV* averages;
    double* percentages;
} Color_Palette;

typedef double Bin;                                    /* src/blur_profile.h:8 */

typedef struct Blur_Profile {                          /* src/blur_profile.h:20-24 */
    int num_angle_bins, num_radius_bins;
    int angle_bin_size, radius_bin_size;
    Bin** bins;                                        /* [angle][radius] */
} Blur_Profile;

typedef struct Blur_Vector {                           /* src/blur_profile.h:52-55 */
    int angle;
    float magnitude;
} Blur_Vector;

typedef struct Blur_Vector_Group {                     /* src/blur_profile.h:58-61 */
    int len_vectors;
    Blur_Vector* blur_vectors;
} Blur_Vector_Group;

typedef struct Sharpnesses {                           /* src/utilities.h:25-28 */
    int N;
    Pixel* sharpness;
} Sharpnesses;

typedef struct Full_Report_Data {                      /* src/utilities.h:30-37 */
    RGB_Statistics* rgb_stats;
    Color_Palette* color_palette;
    Blur_Profile* blur_profile;
    Blur_Vector_Group* blur_vectors;
    Pixel average_saturation;
    Sharpnesses* sharpness;
} Full_Report_Data;

/* ---- legacy entry points (reference signatures) ------------------------- */

/* Replaces get_full_report_data, src/interface.h:16-23 / src/interface.c:20-94.
 * Input: planar doubles (as utils.py:30-46 produces).  Inputs that are all
 * exactly k/255.0 take the RGB8 pipeline; any other finite doubles run the fp64
 * planar kernels (planar.hip: the reference's own double arithmetic); non-finite
 * values are rejected with a message.  Returns NULL on the reference's error
 * cases (src/utilities.c:64-87) and on GPU errors. */
Full_Report_Data* get_full_report_data(Image_RGB* image, Crop_Boundaries* salient_characters,
                                       int h_partitions, int s_partitions, int v_partitions,
                                       double black_thresh, double gray_thresh,
                                       double coverage_thresh, int linked_list_size,
                                       int downsample_rate, int radius_partitions,
                                       int angle_partitions, float quantity_weight,
                                       float saturation_value_weight, double fft_streak_thresh,
                                       double magnitude_thresh, int blur_cutoff_ratio_denom);

/* Replaces free_full_report, src/interface.c:97-111: releases the whole tree
 * and sets *report = NULL.
 *  - A report of get_full_report_data has the reference's allocation shape:
 *    every structure and array is its own malloc (the blur profile's row
 *    pointers and each row included), so a C caller may free() a member itself
 *    (then set it to NULL); this call frees the rest member by member.
 *  - A report of the batch / u8 entry points (phd_report_*) is one heap block
 *    holding the whole tree, recycled for later reports of the same size:
 *    release it only through this call (or phd_free_reports), never by free()
 *    on a member.
 * A pointer that is neither (foreign, or already freed) is ignored; freeing a
 * stale pointer after its memory was reused by a later report is undefined,
 * as with free(). */
void free_full_report(Full_Report_Data** report);
/* free_full_report over an array of n reports (a batch call's `out`); NULL entries are skipped. */
void phd_free_reports(Full_Report_Data** reports, int n);

/* Replaces get_blur_profile_visual, src/blur_profile.c:140-180 (bound by
 * /root/reference/lib.py:36-37).  Caller owns the result (free with
 * phd_free_pgm; the reference's Python caller leaks it). */
Image_PGM* get_blur_profile_visual(Blur_Profile* blur_profile, int height, int width);

/* ---- new entry points ---------------------------------------------------- */

/* The 16 scalar hyper-parameters of get_report (core.py:442-448), reentrant. */
typedef struct phd_config {
    int h_partitions, s_partitions, v_partitions;
    double black_thresh, gray_thresh, coverage_thresh;
    int linked_list_size, downsample_rate;
    int radius_partitions, angle_partitions;
    float quantity_weight, saturation_value_weight;
    double fft_streak_thresh, magnitude_thresh;
    int blur_cutoff_ratio_denom;
} phd_config;

/* Fill *cfg with the get_report defaults (18,2,3,0.1,0.1,0.95,1000,1,40,72,
 * 0.1f,0.9f,1.20,0.3,2). */
void phd_config_default(phd_config* cfg);

/* One image from an interleaved RGB8 HOST buffer (row_stride bytes per row;
 * 0 = 3*width).  No planar-double conversion.  NULL on error. */
Full_Report_Data* phd_report_u8(const uint8_t* rgb, int height, int width, size_t row_stride,
                                const phd_config* cfg, const Crop_Boundaries* crops);

/* A batch of same-size images already resident in GPU memory (d_rgb points at
 * n_images * image_stride bytes on the current HIP device; rows are 3*width
 * bytes).  stream: a hipStream_t or NULL for the library's own stream.
 * out[i] receives each report (NULL on per-image error, status[i] < 0).
 * Returns 0 when every image succeeded, else the number of failures, or -1
 * on a setup error. */
int phd_report_batch_device(const uint8_t* d_rgb, int n_images, int height, int width,
                            size_t image_stride, const phd_config* cfg, Full_Report_Data** out,
                            int* status, void* stream);

/* rgb2hsv + get_hsv_average + get_rgb_statistics over n device-resident RGB8
 * images (BASELINE.json config 3).  Replaces the reference's
 * rgb2hsv (src/image_processing.c:372-417), get_hsv_average (:533-540) and
 * get_rgb_statistics (:543-553) as called from get_full_report_data
 * (src/interface.c:46-55) with downsample_rate 1; the HSV image itself is never
 * materialised.  stats[i] / avg_saturation[i] per image.  0 or -1. */
int phd_hsv_stats_batch_device(const uint8_t* d_rgb, int n_images, int height, int width,
                               size_t image_stride, RGB_Statistics* stats, double* avg_saturation,
                               void* stream);

/* The FFT + blur-profile path alone over n device-resident RGB8 images of one
 * size (BASELINE.json config 4): rgb2pgm, remove_dc_bias, pgm_fft,
 * pgm_normalize_fft, cartesian_to_polar_conversion, calculate_blur_profile
 * and vectorize_blur_profile (src/image_processing.c:505-512,
 * src/blur_profile.c:34-126,233-238,324-458, src/fft_processing.c:18-63,
 * 173-213) as get_full_report_data runs them (src/interface.c:50,62-86).
 * bins_out: n x angle_partitions x radius_partitions doubles (the
 * Blur_Profile bins, angle-major); vectors_out: n x 10 Blur_Vector.  The
 * values equal the full report's.  0 or -1. */
int phd_blur_batch_device(const uint8_t* d_rgb, int n_images, int height, int width, size_t image_stride,
                          const phd_config* cfg, double* bins_out, Blur_Vector* vectors_out, void* stream);

/* Device-resident images of any sizes (config 5 of BASELINE.json): one
 * batched run per group of same-size images (64 images, or as many as hold
 * 64 x 12 MP when that is more: up to 1024 small images in one run).  Returns
 * 0 when every image succeeded, else the number of failures, or -1 on a setup
 * error. */
int phd_report_batch_device_mixed(const uint8_t* const* d_images, const int* heights, const int* widths,
                                  int n_images, const phd_config* cfg, Full_Report_Data** out, int* status,
                                  void* stream);

/* A batch of host images of any sizes (config 5 of BASELINE.json). */
int phd_report_batch_u8(const uint8_t* const* images, const int* heights, const int* widths,
                        int n_images, const phd_config* cfg, Full_Report_Data** out, int* status);

/* ---- batch entry points with per-image crop boxes ------------------------
 * The reference reports the sharpness of caller-given boxes per image:
 * get_full_report_data takes Crop_Boundaries* salient_characters and returns
 * Sharpnesses (src/interface.c:73, get_variance_sharpness,
 * src/filtering.c:151-183).  The three calls below are the batch calls above
 * plus `crops`, an array of n_images pointers:
 *  - crops == NULL behaves as the call without boxes;
 *  - crops[i] == NULL gives a report whose `sharpness` is NULL, as the
 *    reference does for NULL bounds; N == 0 gives a Sharpnesses with N == 0;
 *  - an image whose boxes break crop_pgm's bounds (src/image_processing.c:
 *    215-218; empty or inverted boxes too) fails alone: out[i] = NULL,
 *    status[i] < 0, phd_last_error names the image and the box; the other
 *    images are reported.
 * Every box of every image of a run goes through one kernel launch; a box's
 * value depends on the image bytes and the box only (not on the batch, the
 * lanes or the run). */

/* phd_report_batch_device with per-image boxes (src/filtering.c:151-183 as
 * called from src/interface.c:73). */
int phd_report_batch_device_crops(const uint8_t* d_rgb, int n_images, int height, int width,
                                  size_t image_stride, const phd_config* cfg,
                                  const Crop_Boundaries* const* crops, Full_Report_Data** out, int* status,
                                  void* stream);

/* phd_report_batch_device_mixed with per-image boxes (src/filtering.c:151-183,
 * src/interface.c:73). */
int phd_report_batch_device_mixed_crops(const uint8_t* const* d_images, const int* heights, const int* widths,
                                        int n_images, const phd_config* cfg,
                                        const Crop_Boundaries* const* crops, Full_Report_Data** out,
                                        int* status, void* stream);

/* phd_report_batch_u8 with per-image boxes (src/filtering.c:151-183,
 * src/interface.c:73). */
int phd_report_batch_u8_crops(const uint8_t* const* images, const int* heights, const int* widths,
                              int n_images, const phd_config* cfg, const Crop_Boundaries* const* crops,
                              Full_Report_Data** out, int* status);

/* The sharpness stage alone (get_variance_sharpness, src/filtering.c:151-183,
 * as src/interface.c:73 runs it on the full-resolution luma) over n
 * device-resident RGB8 images of one size.  crops: n_images pointers (NULL =
 * no boxes for that image).  out is flat, image by image, box by box: the
 * full report's values.  Any bad box fails the call.  0 or -1. */
int phd_sharpness_batch_device(const uint8_t* d_rgb, int n_images, int height, int width,
                               size_t image_stride, const Crop_Boundaries* const* crops, double* out,
                               void* stream);

/* Validation hook, host only (no GPU): the batched sharpness kernel's tile
 * plan and merge order (src/filtering.c:151-183 restated per tile, the call
 * of src/interface.c:73) in plain C++ over one interleaved host RGB8 image;
 * out[k] per box.  0 or -1. */
int phd_debug_sharpness_host(const uint8_t* rgb, int height, int width, const Crop_Boundaries* crops,
                             double* out);

/* ---- device images in any byte-strided layout ------------------------------
 * The reference takes three independent plane pointers (Image_RGB,
 * src/image_processing.h:31-36); the device calls above take interleaved RGB8
 * with rows of 3*width bytes only.  A view describes what GPU producers emit
 * -- planar, pitched rows, RGBA / BGRA, BGR, a region of a larger frame, an
 * expanded grey plane -- and the library gathers it once into a packed image
 * of its own (one launch per run for all its views); a view that is already
 * packed is read in place. */

/* One device-resident 8-bit image as a byte-strided view: channel c (0 = R,
 * 1 = G, 2 = B) of pixel (y, x) is the byte at
 *   data + y*row_stride + x*pixel_stride + c*channel_stride.
 * Strides are in bytes and may be negative or 0.  (row, pixel, channel):
 * packed HWC (3W, 3, 1); pitched HWC (pitch, 3, 1); RGBA / RGBX (pitch, 4, 1);
 * BGR (pitch, 3, -1) with data at the R byte; BGRA (pitch, 4, -1), data at +2;
 * ARGB data at +1; planar CHW (W or pitch, 1, plane stride); an expanded grey
 * plane (W, 1, 0); any region of interest of these.
 * Valid: data non-NULL, height and width > 0, pixel_stride != 0 when width > 1,
 * row_stride != 0 when height > 1. */
typedef struct phd_image_view {
    const uint8_t* data;
    int height, width;
    int64_t row_stride, pixel_stride, channel_stride;
} phd_image_view;

/* phd_report_batch_device_mixed_crops over views (get_full_report_data,
 * src/interface.c:20-94, per image): any sizes, crops may be NULL, boxes in the
 * view's own coordinates, the reference's size checks (src/utilities.c:64-87)
 * on the view's height and width.  A bad view fails alone like bad boxes:
 * out[i] = NULL, status[i] < 0, phd_last_error names the image and the field.
 * No byte outside a view's span (lowest to highest addressed byte) is read.
 * Returns as that call. */
int phd_report_batch_device_views(const phd_image_view* views, int n_images, const phd_config* cfg,
                                  const Crop_Boundaries* const* crops, Full_Report_Data** out, int* status,
                                  void* stream);

/* The gather alone: d_dst[i] (device) receives the 3*height*width packed RGB8
 * bytes of view i; any size from 1x1.  For the stage-only calls
 * (phd_blur_batch_device, phd_hsv_stats_batch_device,
 * phd_sharpness_batch_device), which take packed input.  Enqueued on `stream`,
 * or (NULL) on the library's stream and waited for.  A bad view fails the
 * call.  0 or -1. */
int phd_pack_views_device(const phd_image_view* views, int n_images, uint8_t* const* d_dst, void* stream);

/* Validation hook, host only (no GPU): the pack kernel's gather (the reference
 * reads its planes per pixel, src/image_processing.c:387; here the row
 * split and addresses of pack_view.h) over one view of host memory into
 * dst[3*height*width].  0 or -1. */
int phd_debug_pack_view_host(const phd_image_view* view, uint8_t* dst);

/* ---- device images of any element type ---------------------------------------
 * The reference's pixel is a double (typedef double Pixel, src/types.h:5) and
 * get_full_report_data (src/interface.c:20-94) reports on whatever doubles it
 * is given; the device calls above take 8-bit images only.  A typed view
 * describes 8- or 16-bit integers, halves, floats or doubles at byte strides:
 * a 10-, 12- or 16-bit decode, a float CHW tensor in 0..1, double planes that
 * are on the GPU already. */
enum { PHD_ELEM_U8 = 0, PHD_ELEM_U16 = 1, PHD_ELEM_F16 = 2, PHD_ELEM_F32 = 3, PHD_ELEM_F64 = 4 };
enum { PHD_VIEW_SNAP_U8 = 1 };

/* One device-resident image as a byte-strided view of typed elements: channel
 * c of pixel (y, x) is the element at
 *   data + y*row_stride + x*pixel_stride + c*channel_stride   (BYTES),
 * and its value -- the reference's Pixel -- is (double)element / max_value
 * (max_value 0: the type's own, 255 for U8, 65535 for U16, 1.0 for the float
 * types; 1023.0 for a 10-bit image in 16-bit storage, 255.0 for floats in
 * 0..255).  The widening is exact and the division is IEEE fp64 division.  NaN
 * and infinity stay what they are and are rejected where the legacy entry
 * rejects them.
 * Valid: the rules of phd_image_view, and elem one of PHD_ELEM_*, data and the
 * three strides multiples of the element size (every access naturally
 * aligned), max_value 0 or finite and > 0, no unknown bit in flags.
 * An image is 8-bit when every value equals (double)j / 255.0 for an integer j
 * in 0..255 (the rule of the legacy entry's planar doubles, utils.py:30-46);
 * 16-bit values that are all multiples of 257 qualify.
 * PHD_VIEW_SNAP_U8 (F16 and F32 views at the default maximum; ignored for the
 * others): an element also counts as 8-bit value j when it equals the type's
 * round-to-nearest value of j / 255, (T)((double)j / 255.0) -- what a uint8
 * image divided by 255 in that type holds.  Without it such a float image is
 * reported as the doubles its floats widen to. */
typedef struct phd_typed_view {
    const void* data;            /* element of channel R of pixel (0,0) */
    int height, width;
    int64_t row_stride, pixel_stride, channel_stride;   /* BYTES, as phd_image_view; may be negative or 0 */
    int elem;                    /* PHD_ELEM_* */
    int flags;                   /* PHD_VIEW_SNAP_U8 or 0 */
    double max_value;            /* 0 = the type's: 255, 65535, 1.0 */
} phd_typed_view;

/* phd_report_batch_device_views over typed views (get_full_report_data,
 * src/interface.c:20-94, per image on the Pixels of src/types.h:5): the same
 * semantics, return values and per-image failure rules; any sizes, boxes in
 * view coordinates, no byte read outside a view's span.  8-bit images (the rule
 * above) join the RGB8 run of their size group, with its results bit for bit;
 * a PHD_ELEM_U8 view at the default maximum is routed exactly as
 * phd_report_batch_device_views routes it (a packed one is read in place).
 * Every other image is decoded into double planes on the device and takes the
 * fp64 pipeline of get_full_report_data, one image at a time.  A non-finite
 * image fails alone. */
int phd_report_batch_device_typed_views(const phd_typed_view* views, int n_images, const phd_config* cfg,
                                        const Crop_Boundaries* const* crops, Full_Report_Data** out, int* status,
                                        void* stream);

/* The decode alone (the planes of Image_RGB, src/image_processing.h:31-36, as
 * Pixels, src/types.h:5): d_planes[i] (device) receives 3*height*width
 * doubles, the R plane, then G, then B; any size from 1x1.  Enqueued on
 * `stream`, or (NULL) on the library's stream and waited for.  A bad view
 * fails the call.  0 or -1. */
int phd_decode_views_device(const phd_typed_view* views, int n_images, double* const* d_planes, void* stream);

/* Validation hook, host only (no GPU): the decode kernels' row code
 * (decode_view.h; the reference reads its planes per pixel,
 * src/image_processing.c:387) over one view of host memory.  planes
 * [3*height*width], rgb8 [3*height*width] (j = rint(value * 255), or NULL)
 * and *is_u8 (1 when the image is 8-bit by the rule above, snap included; or
 * NULL).  0, or -1 with phd_last_error. */
int phd_debug_decode_view_host(const phd_typed_view* view, double* planes, uint8_t* rgb8, int* is_u8);

/* ---- device YCbCr frames ---------------------------------------------------------
 * The reference reports on RGB planes (Image_RGB, src/image_processing.h:31-36);
 * the JPEG and video decoders that feed a GPU pipeline emit 8-bit YCbCr: NV12
 * surfaces with a pitch, planar 4:2:0, 4:2:2 or 4:4:4, packed YUY2.  A YUV view
 * describes such a frame and the library converts it, in one launch per run
 * for all its views, into a packed RGB8 image of its own; the report is the
 * report of that image, field for field.  The conversion is defined in
 * integers, so every caller gets the same RGB8 bytes for the same frame.
 *
 * Step 1, chroma at pixel (y, x) of a plane c (cb or cr) of ch x cw samples,
 * sx = chroma_shift_x, sy = chroma_shift_y, indices clamped to the plane:
 *   REPLICATE:        C = c[y >> sy][x >> sx]
 *   TRIANGLE, 4:4:4:  C = c[y][x]
 *   TRIANGLE, 4:2:2:  i = x >> 1, far = i-1 (x even) or i+1 (x odd), clamped to
 *                     [0, cw-1];  C = (3*c[y][i] + c[y][far] + (x odd ? 2 : 1)) >> 2
 *   TRIANGLE, 4:2:0:  j = y >> 1, farrow = j-1 (y even) or j+1 (y odd), clamped to
 *                     [0, ch-1];  t[k] = 3*c[j][k] + c[farrow][k];
 *                     C = (3*t[i] + t[far] + (x odd ? 7 : 8)) >> 4
 * (the weights and rounding of libjpeg's "fancy" upsampling).
 * Step 2, the matrix, in int32 with arithmetic shifts: u = Cb - 128,
 * v = Cr - 128, yy = cy*(Y - yoff),
 *   R = clamp8((yy + crv*v + 32768) >> 16)
 *   G = clamp8((yy - cgu*u - cgv*v + 32768) >> 16)
 *   B = clamp8((yy + cbu*u + 32768) >> 16)
 *   matrix, range        cy     crv     cgu    cgv    cbu     yoff
 *   BT601 FULL (JFIF)    65536  91881   22554  46802  116130  0
 *   BT601 LIMITED        76309  104597  25675  53279  132201  16
 *   BT709 FULL           65536  103206  12276  30679  121609  0
 *   BT709 LIMITED        76309  117489  13975  34925  138438  16
 * The JFIF row holds libjpeg's constants (cgu 22554); the others are
 * round(value * 65536).  Every row stays within 0.504 of the clamped
 * real-valued result (0.5 + 511 * 0.5 / 65536). */
enum { PHD_YUV_BT601 = 0, PHD_YUV_BT709 = 1 };
enum { PHD_YUV_FULL = 0, PHD_YUV_LIMITED = 1 };
enum { PHD_YUV_CHROMA_REPLICATE = 0, PHD_YUV_CHROMA_TRIANGLE = 1 };

/* One device-resident 8-bit YCbCr frame.  Luma of pixel (y, x) is the byte at
 *   y + y*y_row_stride + x*y_pixel_stride,
 * chroma sample (j, i) the byte at cb + j*c_row_stride + i*c_pixel_stride and
 * the same from cr; the chroma planes are ch = (height + sy) >> sy rows of
 * cw = (width + sx) >> sx samples.  I420 / YV12: three planes; NV12:
 * c_pixel_stride 2, cr = cb + 1; NV21: cb = cr + 1; I422, I444: three planes,
 * shifts (1,0) and (0,0); YUY2: y_pixel_stride 2, c_pixel_stride 4,
 * cb = y + 1, cr = y + 3, shifts (1,0); UYVY: the same with the pointers moved;
 * pitched surfaces: a row stride larger than the row; a region of a larger
 * frame: pointers at the region's first sample, even origin.  (4:0:0 is an
 * expanded grey plane phd_image_view.)
 * Valid: the three pointers non-NULL, height and width > 0, the shifts one of
 * the three pairs, every enum in range, y_pixel_stride != 0 when width > 1,
 * y_row_stride != 0 when height > 1, c_pixel_stride != 0 when cw > 1,
 * c_row_stride != 0 when ch > 1. */
typedef struct phd_yuv_view {
    const uint8_t *y, *cb, *cr;            /* sample (0,0) of each plane */
    int height, width;                     /* luma size */
    int64_t y_row_stride, y_pixel_stride;  /* BYTES; may be negative */
    int64_t c_row_stride, c_pixel_stride;  /* BYTES; shared by cb and cr */
    int chroma_shift_x, chroma_shift_y;    /* (0,0) 4:4:4, (1,0) 4:2:2, (1,1) 4:2:0 */
    int matrix, range, chroma;             /* PHD_YUV_* */
} phd_yuv_view;

/* phd_report_batch_device_views over YUV views (get_full_report_data,
 * src/interface.c:20-94, per image, on the Image_RGB, src/image_processing.h:
 * 31-36, the conversion above defines): the same semantics, return values and
 * per-image failure rules; any sizes, size groups on the lanes, boxes in luma
 * coordinates, the reference's size checks (src/utilities.c:64-87) before
 * anything is read.  A bad view fails alone and phd_last_error names the image
 * and the field.  No byte outside the union of the three planes' spans is
 * read. */
int phd_report_batch_device_yuv(const phd_yuv_view* views, int n_images, const phd_config* cfg,
                                const Crop_Boundaries* const* crops, Full_Report_Data** out, int* status,
                                void* stream);

/* The conversion alone (the Image_RGB of src/image_processing.h:31-36 as
 * packed bytes, the input of get_full_report_data, src/interface.c:20-94):
 * d_dst[i] (device) receives the 3*height*width RGB8 bytes of view i; any size
 * from 1x1.  Enqueued on `stream`, or (NULL) on the library's stream and waited
 * for.  A bad view fails the call.  0 or -1. */
int phd_convert_yuv_device(const phd_yuv_view* views, int n_images, uint8_t* const* d_dst, void* stream);

/* Validation hook, host only (no GPU): the conversion kernel's row code
 * (yuv_view.h; the reference reads its Image_RGB planes per pixel,
 * src/image_processing.h:31-36, src/interface.c:20-94) over one view of host
 * memory into dst[3*height*width].  0, or -1 with phd_last_error. */
int phd_debug_yuv_view_host(const phd_yuv_view* view, uint8_t* dst);

/* ---- palette label maps ----------------------------------------------------------
 * The reference's colour quantisation ends with every pixel in the list of one
 * palette parent, or in none: group_irregular_pixels
 * (src/color_quantization.c:342-479) moves the irregular groups' pixels into
 * valid_parents[i]'s lists and calculate_avg_hsv (:510-576) averages each list
 * into color_palette->averages[i]; the lists are then freed.  A label map is
 * that assignment kept: for an H x W image reported at downsample_rate r it is
 * mh x mw uint16, row-major, (mh, mw) = (H, W) for r <= 1, else (H / r, W / r)
 * (downsample_rgb, src/image_processing.c:344-366); element k belongs to pixel
 * k of the image rgb2hsv sees (src/interface.c:46), the downsampled image with
 * its row-stride quirk.  label[k] = i when pixel k is in valid_parents[i]'s
 * list, PHD_LABEL_NONE when it is in none (a tie's overflow).  Per slot,
 * percentages[i] == (double)count(label == i) * (1.0 / (double)(mh*mw)), bit
 * for bit. */
enum { PHD_LABEL_NONE = 0xFFFF };

/* phd_report_batch_device_mixed_crops plus label maps (the lists of
 * src/color_quantization.c:342-479 that :510-576 averages).  d_labels: n_images
 * device pointers; d_labels[i] receives (height/ds)*(width/ds) uint16 labels of
 * image i (2-byte aligned), NULL = no map for that image; d_labels == NULL is
 * exactly the call without maps.  Reports, statuses and return value as that
 * call; the maps are complete when it returns.  An image that fails (size
 * check, boxes, decision) leaves its buffer untouched or unspecified, never
 * written outside its mh*mw elements. */
int phd_report_batch_device_mixed_labels(const uint8_t* const* d_images, const int* heights,
                                         const int* widths, int n_images, const phd_config* cfg,
                                         const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                         Full_Report_Data** out, int* status, void* stream);

/* The same for device images as producers hold them:
 * phd_report_batch_device_views, _typed_views and _yuv plus label maps, with the
 * semantics of phd_report_batch_device_mixed_labels word for word (d_labels ==
 * NULL is exactly the call without maps; d_labels[i] == NULL: no map for image
 * i; complete on return; a failing image -- descriptor, size check, boxes,
 * non-finite value, decision -- leaves its buffer untouched or unspecified and
 * nothing is written outside its mh*mw elements; fewer than 32768 octree
 * groups).  Map i is (height/ds) x (width/ds) in the view's (the luma's) own
 * coordinates: element k belongs to pixel k of the image rgb2hsv sees
 * (src/interface.c:46, src/image_processing.c:372-417) after the view has
 * been gathered, converted or decoded.  An 8-bit image (a view, a YUV frame's
 * RGB8 conversion, a typed view whose values are all j/255) gets the map of
 * the same bytes through phd_report_batch_device_mixed_labels.  A typed view
 * on the fp64 route gets the lists of src/color_quantization.c:342-479 for
 * the doubles get_full_report_data (src/interface.c:20-94) would be given:
 * the group of rgb2hsv + arm_octree (:108-161) on those doubles and the keep
 * rule of group_irregular_pixels, with percentages[i] == (double)count(label
 * == i) * (1.0 / (double)(mh*mw)) bit for bit as on the 8-bit route. */
int phd_report_batch_device_views_labels(const phd_image_view* views, int n_images, const phd_config* cfg,
                                         const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                         Full_Report_Data** out, int* status, void* stream);
int phd_report_batch_device_typed_views_labels(const phd_typed_view* views, int n_images, const phd_config* cfg,
                                               const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                               Full_Report_Data** out, int* status, void* stream);
int phd_report_batch_device_yuv_labels(const phd_yuv_view* views, int n_images, const phd_config* cfg,
                                       const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                       Full_Report_Data** out, int* status, void* stream);

/* The quantised image of a label map (each pixel painted with the colour of
 * the average calculate_avg_hsv, src/color_quantization.c:510-576, put it
 * into): dst pixel k = the 3 bytes lut[3*label[k]..] or none_rgb for
 * PHD_LABEL_NONE.  d_labels, d_dst: n_maps device pointers (3*mh*mw bytes per
 * destination).  lut: HOST, 3*n_slots bytes (NULL allowed when n_slots is 0).
 * A label >= n_slots that is not NONE fails nothing and is written as
 * none_rgb.  Any map size from 1x1; at most 65535 maps.  One launch for all
 * maps.  Enqueued on `stream`, or (NULL) on the library's stream and waited
 * for.  0 or -1. */
int phd_labels_to_rgb_device(const uint16_t* const* d_labels, const int* map_heights,
                             const int* map_widths, int n_maps, const uint8_t* const* luts, const int* n_slots,
                             const uint8_t none_rgb[3], uint8_t* const* d_dst, void* stream);

/* ---- box palettes ------------------------------------------------------------------
 * Which palette colours a crop box holds: the lists of group_irregular_pixels
 * (src/color_quantization.c:342-479) that calculate_avg_hsv (:510-576)
 * averages, counted inside a box instead of over the image.  The box palette
 * of a label map is counts[n_boxes][n_slots + 1], uint32, row-major: column
 * s < n_slots is the number of map elements inside the box whose label is s,
 * column n_slots everything else (PHD_LABEL_NONE and any label >= n_slots,
 * which phd_labels_to_rgb_device paints as none_rgb).  A box (top, bottom,
 * left, right) covers rows top <= y < bottom and columns left <= x < right,
 * crop_pgm's convention (src/image_processing.c:213-232), as the boxes of
 * salient_characters do for sharpness (src/interface.c:73).  Overlapping boxes
 * are counted independently; every row sums to its box's element count; for a
 * box that is the whole map, (double)counts[b][s] * (1.0 / (double)(mh*mw)) ==
 * percentages[s] bit for bit.  The counts are integers added with integer
 * atomics: the same on every run. */
typedef struct phd_box_palette {
    int n_boxes;        /* boxes[i]->N; 0 when map i has no boxes (boxes[i] NULL, N == 0) */
    int n_slots;        /* n_slots[i]: color_palette->N of the map's report */
    uint32_t* counts;   /* n_boxes x (n_slots + 1), row-major, one malloc; NULL when n_boxes == 0 */
} phd_box_palette;
/* Frees counts and zeroes the structs; bp == NULL is a no-op. */
void phd_free_box_palettes(phd_box_palette* bp, int n);

/* The box palettes of n_maps label maps (the lists of src/color_quantization.c:
 * 342-479 and :510-576; boxes as src/image_processing.c:213-232 cuts them, given
 * as src/interface.c:73 gives them) from any of the four _labels entries:
 * d_labels[i] (device, 2-byte aligned) is map_heights[i] x map_widths[i];
 * boxes[i] in MAP coordinates (NULL or N == 0: n_boxes == 0).  A box is valid
 * when 0 <= left <= right <= mw and 0 <= top <= bottom <= mh; an empty box is
 * allowed and counts 0.  An inverted or out-of-range box, a NULL map,
 * non-positive sizes or n_slots outside 0..4096 (validate_config's group cap)
 * fail the call with -1 before any device work, phd_last_error naming the map
 * and the box, and out is left zeroed.  Every box of every map goes through one
 * launch, enqueued on `stream` or (NULL) on the library's stream, and is waited
 * for in both cases: the result is on the host.  out: n_maps structs, filled
 * (release with phd_free_box_palettes).  0 or -1. */
int phd_box_palettes_device(const uint16_t* const* d_labels, const int* map_heights, const int* map_widths,
                            int n_maps, const int* n_slots, const Crop_Boundaries* const* boxes,
                            phd_box_palette* out, void* stream);

/* The four _labels entries plus box palettes (the lists of
 * src/color_quantization.c:342-479 and :510-576 inside the boxes of
 * src/image_processing.c:213-232 that src/interface.c:73 hands to sharpness):
 * box_palettes, n_images structs, receives image i's box palette for the same
 * `crops` that feed its sharpnesses, validated by the same rule; boxes are in
 * IMAGE coordinates.  At downsample_rate r > 1 the map is mh x mw = (H / r) x
 * (W / r) and a box covers the map elements whose nominal position (y*r, x*r)
 * lies inside it: rows ceil(top / r) .. min(ceil(bottom / r), mh), columns
 * ceil(left / r) .. min(ceil(right / r), mw); a box that is empty after scaling
 * gives a row of zeros.  box_palettes == NULL is exactly the _labels call.
 * d_labels may be NULL or hold NULL entries: an image with boxes and a map of
 * the caller's is counted from that map, one without from a scratch map of the
 * library's, written by the same label launch; an image without boxes gets no
 * scratch and no count work and {0, n_slots, NULL}.  An image that fails (bad
 * boxes or anything else) fails alone as in the _labels call and gets {0, 0,
 * NULL}.  The palettes are complete when the call returns (release with
 * phd_free_box_palettes).  Reports, statuses and return value as the _labels
 * call; results do not depend on lanes, batch or run. */
int phd_report_batch_device_mixed_box_palettes(const uint8_t* const* d_images, const int* heights,
                                               const int* widths, int n_images, const phd_config* cfg,
                                               const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                               phd_box_palette* box_palettes, Full_Report_Data** out, int* status,
                                               void* stream);
int phd_report_batch_device_views_box_palettes(const phd_image_view* views, int n_images, const phd_config* cfg,
                                               const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                               phd_box_palette* box_palettes, Full_Report_Data** out, int* status,
                                               void* stream);
int phd_report_batch_device_typed_views_box_palettes(const phd_typed_view* views, int n_images, const phd_config* cfg,
                                                     const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                                     phd_box_palette* box_palettes, Full_Report_Data** out,
                                                     int* status, void* stream);
int phd_report_batch_device_yuv_box_palettes(const phd_yuv_view* views, int n_images, const phd_config* cfg,
                                             const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                             phd_box_palette* box_palettes, Full_Report_Data** out, int* status,
                                             void* stream);

/* Validation hook, host only (no GPU): the counting kernel's own item plan and
 * row code (box_tiles.h; the lists of src/color_quantization.c:342-479 inside
 * the boxes of src/image_processing.c:213-232) over one map of host memory.
 * counts: boxes->N x (n_slots + 1).  0, or -1 with phd_last_error. */
int phd_debug_box_counts_host(const uint16_t* map, int mh, int mw, int n_slots,
                              const Crop_Boundaries* boxes, uint32_t* counts);

/* ---- box statistics ------------------------------------------------------------
 * The box statistics of an image are, per crop box, what get_rgb_statistics
 * (src/image_processing.c:543-553) and get_hsv_average (src/image_processing.c:
 * 533-540) over rgb2hsv's s (src/image_processing.c:372-417) give on
 * crop_image(image, right, left, bottom, top) (src/image_processing.c:244-266)
 * of the FULL-RESOLUTION image: rows top <= y < bottom, columns left <= x <
 * right; downsample_rate plays no part, as it plays none in get_rgb_statistics
 * or in the sharpness.  For 8-bit images the library keeps exact integers per
 * box -- M[0..2] = sum k and M[3..5] = sum k^2 per channel, D[m] = sum of
 * (max - min) over the pixels whose max is m, n1 = #(min == 0 < max), N pixels
 * -- and finishes them as the report's own statistics are finished:
 *   stats = the report's moment formula on (M, N): a whole-image box gives the
 *           report's rgb_stats bit for bit;
 *   S = sum over m = 1..255, ascending and sequential, of (double)D[m] / (double)m;
 *   average_saturation = (S - (1.0 - 0.999999) * (double)n1) / (double)N.
 * The sums come from integer atomics: the same on every run.  Typed views that
 * are not 8-bit take the fp64 functions themselves (mean sum / N, the variance's
 * second pass sum (x - B)^2 / N, s per pixel), summed in a fixed order. */
typedef struct phd_box_stats {
    int n_boxes;                 /* crops[i]->N; 0 when image i has no boxes */
    RGB_Statistics* stats;       /* n_boxes; NULL when n_boxes == 0 */
    double* average_saturation;  /* n_boxes; same malloc as stats */
} phd_box_stats;
/* Frees stats (and with it average_saturation) and zeroes the structs; bs ==
 * NULL is a no-op. */
void phd_free_box_stats(phd_box_stats* bs, int n);

/* The stage alone (get_rgb_statistics, src/image_processing.c:543-553, and
 * rgb2hsv + get_hsv_average, :372-417 and :533-540, on the boxes crop_image
 * cuts, :244-266): n_images packed RGB8 device images of any sizes from 1 x 1
 * and any base alignment.  boxes[i] NULL or N == 0 gives n_boxes 0.  Boxes
 * follow the rule of the report's crops (inside the image, not empty, not
 * inverted).  Anything else -- a NULL image, a non-positive size, a bad box
 * list -- fails the call with -1 before any device work, phd_last_error naming
 * image and box, and out is left zeroed.  One counting launch for all boxes of
 * all images (and one small finish launch), on `stream` or (NULL) the
 * library's, waited for in both cases.  No byte outside an image's 3 * H * W
 * is read.  out: n_images structs (release with phd_free_box_stats).  0 or -1. */
int phd_box_stats_device(const uint8_t* const* d_images, const int* heights, const int* widths, int n_images,
                         const Crop_Boundaries* const* boxes, phd_box_stats* out, void* stream);

/* The four _box_palettes entries plus box statistics (get_rgb_statistics,
 * src/image_processing.c:543-553, and get_hsv_average, :533-540, on the boxes of
 * :244-266): box_stats, n_images structs, receives image i's box statistics
 * for the same `crops` that feed its sharpnesses and box palettes, in image
 * coordinates, validated once by the same rule.  box_stats == NULL is exactly
 * the _box_palettes call.  d_labels and box_palettes may be NULL independently:
 * box statistics alone cause no label map, no scratch map and no label launch.
 * An image without boxes gets {0, NULL, NULL} and no work; an image that fails
 * for any reason fails alone, as in the _box_palettes call, and gets {0, NULL,
 * NULL}.  The statistics are complete when the call returns (release with
 * phd_free_box_stats) and do not depend on lanes, batch or run. */
int phd_report_batch_device_mixed_box_stats(const uint8_t* const* d_images, const int* heights, const int* widths,
                                            int n_images, const phd_config* cfg,
                                            const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                            phd_box_palette* box_palettes, phd_box_stats* box_stats,
                                            Full_Report_Data** out, int* status, void* stream);
int phd_report_batch_device_views_box_stats(const phd_image_view* views, int n_images, const phd_config* cfg,
                                            const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                            phd_box_palette* box_palettes, phd_box_stats* box_stats,
                                            Full_Report_Data** out, int* status, void* stream);
int phd_report_batch_device_typed_views_box_stats(const phd_typed_view* views, int n_images, const phd_config* cfg,
                                                  const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                                  phd_box_palette* box_palettes, phd_box_stats* box_stats,
                                                  Full_Report_Data** out, int* status, void* stream);
int phd_report_batch_device_yuv_box_stats(const phd_yuv_view* views, int n_images, const phd_config* cfg,
                                          const Crop_Boundaries* const* crops, uint16_t* const* d_labels,
                                          phd_box_palette* box_palettes, phd_box_stats* box_stats,
                                          Full_Report_Data** out, int* status, void* stream);

/* Validation hook, host only (no GPU): the box statistics kernel's own item
 * plan and row code (box_stat_tiles.h; get_rgb_statistics, src/image_processing.c:
 * 543-553, and get_hsv_average, :533-540, on the boxes of :244-266) over one
 * packed RGB8 image of host memory at any alignment.  stats and
 * average_saturation: boxes->N each.  sums (or NULL): 264 unsigned long long per
 * box = M[6], n1, N, D[256].  0, or -1 with phd_last_error. */
int phd_debug_box_stats_host(const uint8_t* rgb, int height, int width, const Crop_Boundaries* boxes,
                             RGB_Statistics* stats, double* average_saturation, unsigned long long* sums);

/* ---- window blur ----------------------------------------------------------------
 * The window blur of an image is, per window, the Blur_Profile and the ten
 * Blur_Vectors of the reference on that crop of the FULL-RESOLUTION image;
 * downsample_rate plays no part.  A window of image i is a Crop_Boundaries box
 * with bottom - top == right - left == T inside the image (rows top <= y <
 * bottom, columns left <= x < right: crop_image, src/image_processing.c:244-266);
 * T is the call's `window`, 64 or 128.  Its values:
 *  1. avg = (Br + Bg + Bb) / 3 of get_rgb_statistics(crop) (src/image_processing.c:
 *     543-553, src/interface.c:78), from the window's exact integer channel sums:
 *     ((double)sum / 255.0 / n per channel, added in r g b order) / 3.0, n = T * T;
 *  2. pgm = rgb2pgm(crop) - avg (src/image_processing.c:505-512,
 *     src/blur_profile.c:233-238);
 *  3. the unnormalised r2c 2-D DFT, p = re * re + im * im (src/fft_processing.c:
 *     18-63), then pgm_normalize_fft (:173-213); fft_max is its maximum;
 *  4. cartesian_to_polar_conversion(T / 2 + 1, T) and calculate_blur_profile
 *     (src/blur_profile.c:427-458, 34-126): bins[na][nr], angle_bin_size and
 *     radius_bin_size;
 *  5. vectorize_blur_profile (src/blur_profile.c:324-416): 10 vectors.
 * A window whose every p < 1 (a constant grey, black or white window) has
 * all-zero bins.  Bin sums are kept as bin_scale(T, T / 2 + 1) fixed point, as
 * everywhere in the library: a window's values depend on its 3 * T * T bytes and
 * the grid only and are bit-identical on every run. */
typedef struct phd_window_blur {
    int n_windows;                         /* windows[i]->N; 0 when image i has none */
    int num_angle_bins, num_radius_bins;   /* cfg's */
    int angle_bin_size, radius_bin_size;   /* Blur_Profile's, for a T x T crop (src/blur_profile.c:56-61) */
    double* bins;                          /* n_windows x na x nr, angle-major; one malloc; NULL when 0 */
    Blur_Vector* vectors;                  /* n_windows x 10; same malloc */
    double* fft_max;                       /* n_windows; same malloc */
} phd_window_blur;
/* Frees bins (and with it vectors and fft_max) and zeroes the structs; wb ==
 * NULL is a no-op. */
void phd_free_window_blur(phd_window_blur* wb, int n);

/* get_blur_profile and vectorize_blur_profile (src/blur_profile.c:250-293,
 * 324-416; pgm_fft and pgm_normalize_fft, src/fft_processing.c:18-63, 173-213) on
 * the T x T windows crop_image cuts (src/image_processing.c:244-266) from
 * n_images packed RGB8 device images of any sizes from T x T and any base
 * alignment; no byte outside an image's 3 * H * W is read, and the reference's
 * 350-px size check does not apply (a stage on crops, as phd_box_stats_device).
 * windows[i] NULL or N == 0 gives n_windows 0.  Of cfg only the five blur fields
 * are used (radius_partitions, angle_partitions, fft_streak_thresh,
 * magnitude_thresh, blur_cutoff_ratio_denom); the whole struct must be valid.
 * Refused with -1 before any device work, phd_last_error naming image and
 * window and out left zeroed: a NULL image, a size below T, a window other than
 * 64 or 128, a box whose sides are not T or that leaves the image,
 * angle_partitions * radius_partitions > 2880, and a grid the polar table of a
 * T x (T / 2 + 1) spectrum has no place for (a radius bin size of 0, where the
 * reference divides by zero, src/utilities.c:43-52, e.g. T = 64 with 46 radius
 * partitions; an element outside the table, where the reference writes out of
 * bounds, src/blur_profile.c:97-99, e.g. T = 64 at 40 x 72).
 * All windows of all images go through one launch, one block per window with
 * the whole window in LDS (profile slot 14); when their bin sums and maxima
 * exceed PHD_WINDOW_BLUR_BUDGET bytes the call is cut into chunks of that
 * size, one launch and one download each.  Per call one table upload (twiddles
 * and window records).  On `stream` or (NULL) the library's, waited for in both
 * cases.  out: n_images structs (release with phd_free_window_blur).  0 or -1. */
#define PHD_WINDOW_BLUR_BUDGET 33554432u   /* 32 MiB, on the device and pinned */
int phd_blur_windows_device(const uint8_t* const* d_images, const int* heights, const int* widths, int n_images,
                            const Crop_Boundaries* const* windows, int window, const phd_config* cfg,
                            phd_window_blur* out, void* stream);

/* Validation hook, host only (no GPU): the window blur kernel's own plan, passes
 * and index maps (blur_window.h; get_blur_profile, src/blur_profile.c:250-293, on
 * the windows of src/image_processing.c:244-266) over one packed RGB8 image of
 * host memory at any alignment, finished as the device call finishes; the log
 * is the C library's.  bins: windows->N x na x nr, vectors: windows->N x 10,
 * fft_max: windows->N.  0, or -1 with phd_last_error. */
int phd_debug_window_blur_host(const uint8_t* rgb, int height, int width, const Crop_Boundaries* windows,
                               int window, const phd_config* cfg, double* bins, Blur_Vector* vectors,
                               double* fft_max);

/* ---- blur vectors: the window blur finished on the device ------------------------
 * Per window the ten Blur_Vectors and fft_max of the window blur above, left in
 * device memory; the bins are never formed outside the window's block.  After
 * the kernel's binning the same block runs the finish (blur_window.h):
 *  - G_s = 1 / (2 * log(sqrt(fft_max) + 1)) (pgm_normalize_fft,
 *    src/fft_processing.c:192) and, per bin, (double)sum / bin_scale * G_s / count
 *    (calculate_blur_profile's averaging, src/blur_profile.c:106-116; 0 for an
 *    empty bin or a zero sum), one thread per bin;
 *  - vectorize_blur_profile (src/blur_profile.c:324-416): the per-angle totals over
 *    the first nr / blur_cutoff_ratio_denom radii and their average (:341-349),
 *    convolve_1d with the 5-tap box and / 5 (src/filtering.c:12-24), the three
 *    local-maximum rules in increasing angle with at most ten maxima (:358-379),
 *    and per maximum the perpendicular angle, the blur_avg > avg rejection, the
 *    first radius below magnitude_thresh, magnitude = (float)r / (float)nr and
 *    angle = (int)(180 * ((float)a / (float)na) - 90) (:384-414); entries past the
 *    last maximum are zero (calloc, :297-302).  Every fp64 sum runs in the
 *    reference's order.
 * fft_max is bit-identical to phd_blur_windows_device's (the same code).  The
 * vectors are the reference's on that crop; they equal phd_blur_windows_device's
 * unless a bin lies within the last-place difference of the two logs (the device
 * library's fp64 log here, the C library's on the host there) of
 * magnitude_thresh or of another comparison the rules make.  A window's values
 * depend on its 3 * T * T bytes and the grid only: bit-identical on every run and
 * wherever the window sits in the call.
 *
 * d_vectors[i]: device pointer, 4-byte aligned, receives n_i x 10 Blur_Vectors;
 * d_fft_max[i]: device pointer, 8-byte aligned, receives n_i doubles (d_fft_max ==
 * NULL or d_fft_max[i] == NULL: no maxima for that image).  n_i is windows[i]->N
 * or gh * gw; d_vectors[i] may be NULL only when n_i == 0.  Nothing is written
 * outside those 80 * n_i and 8 * n_i bytes.  Images as for
 * phd_blur_windows_device: packed RGB8 device images of any sizes from T x T at
 * any base alignment, no byte outside an image's 3 * H * W read.
 * Refused with -1 before any device work, phd_last_error naming image and window:
 * everything phd_blur_windows_device refuses, a non-positive stride, a NULL
 * d_vectors entry of an image that has windows, and angle_partitions < 2
 * (vectorize_blur_profile reads smooth[1] and smooth[num_angle_bins - 2], which
 * lie outside the array at one angle bin, src/blur_profile.c:360-374).
 * One launch (profile slot 15) takes every window of every image; the result is
 * 88 bytes per window, so there are no chunks and PHD_WINDOW_BLUR_BUDGET plays no
 * part.  Per call one table upload (twiddles, the bins' element counts, window
 * records and destinations).  Enqueued on `stream` and not waited for, or (NULL)
 * on the library's stream and waited for, as phd_pack_views_device.  A call with
 * no window at all does no device work.  0 or -1. */
/* Window lists, as phd_blur_windows_device takes them. */
int phd_blur_vectors_device(const uint8_t* const* d_images, const int* heights, const int* widths, int n_images,
                            const Crop_Boundaries* const* windows, int window, const phd_config* cfg,
                            Blur_Vector* const* d_vectors, double* const* d_fft_max, void* stream);
/* A regular grid per image: window_grid's rule, gh = (H - T) / stride + 1, gw = (W - T) / stride + 1,
 * row-major; stride > 0, may be smaller (overlap) or larger than the window. */
int phd_blur_vector_maps_device(const uint8_t* const* d_images, const int* heights, const int* widths, int n_images,
                                int window, int stride, const phd_config* cfg,
                                Blur_Vector* const* d_vectors, double* const* d_fft_max, void* stream);

/* Validation hook, host only (no GPU): the blur vector kernel's twin, the window
 * blur kernel's steps on the host (as phd_debug_window_blur_host) and then the
 * shared finish (blur_window.h; vectorize_blur_profile, src/blur_profile.c:
 * 324-416) with the C library's log.  vectors: windows->N x 10, fft_max:
 * windows->N.  0, or -1 with phd_last_error. */
int phd_debug_window_vectors_host(const uint8_t* rgb, int height, int width, const Crop_Boundaries* windows,
                                  int window, const phd_config* cfg, Blur_Vector* vectors, double* fft_max);
/* Validation hook, host only (no GPU): the shared finish alone over caller-given
 * bin sums of one window (nbins u64, bin_scale(T, T / 2 + 1) fixed point; fft_max
 * as pgm_normalize_fft's maximum, src/fft_processing.c:173-213): bins (na x nr, or
 * NULL) and 10 vectors.  0, or -1 with phd_last_error. */
int phd_debug_window_finish_host(const unsigned long long* bin_sums, double fft_max, int window,
                                 const phd_config* cfg, double* bins, Blur_Vector* vectors);

/* ---- sharpness maps: the Laplacian sharpness of window grids, on the device ------
 * The window sharpness of a T x T window (rows top <= y < top+T, columns
 * left <= x < left+T, crop_pgm's convention, src/image_processing.c:213-232) is
 * get_variance_sharpness (src/filtering.c:151-183) on that crop of the
 * full-resolution luma.  The steps are rgb2pgm (src/image_processing.c:505-512),
 * the 3x3 Laplacian with taps outside the crop skipped (filter_image,
 * src/filtering.c:81-107), and then variance / average (get_average and
 * get_variance, src/filtering.c:125-148).  downsample_rate plays no part.
 *
 * For 8-bit images every term is an integer, and the library keeps it so:
 *  - l(y,x) = 299 R + 587 G + 114 B.  This is the reference's luma times 255000
 *    and is at most 255000.
 *  - f(y,x) = 9 l(y,x) - sum of l over the 3x3 neighbourhood inside the window.
 *    Positions outside the window count as 0, so the centre weighs 8 and each
 *    neighbour inside weighs -1.  |f| <= 2,040,000.
 *  - n = T^2, S1 = sum f, S2 = sum f^2.  Only the window's border ring contributes
 *    to S1, so S1 >= 0 and fits 32 bits.  S2 fits a u64.
 *  - D = n S2 - S1^2.  It is never negative and exceeds 64 bits at T = 128; it is
 *    kept as 128 bits (two u64 words).
 *  - The finish is the only floating point.  It is shared by the kernel and the
 *    host twin (sharp_window.h), plain IEEE fp64 operations with no fused
 *    multiply-add:
 *      num       = (double)hi * 18446744073709551616.0 + (double)lo
 *      sharpness = num / (((double)n * (double)S1) * 255000.0)
 *      variance  = num / (((double)n * (double)n) * 65025000000.0)
 *  - S1 == 0 means the window's border ring is black.  The reference's average is
 *    then 0.  The division above gives what IEEE gives: NaN when D == 0 (an
 *    all-black window) and +inf otherwise.  It is left unguarded.
 * Because the integer sums are exact, a window's values depend on its 3 T^2 bytes
 * only.  They are bit-identical on every run and wherever the window sits in the
 * call, and the kernel and its host twin agree bit for bit.
 *
 * window is 16, 32, 64 or 128; at 64 and 128 one window_grid serves the blur
 * vector map and this map.  d_sharpness[i]: device pointer, 8-byte aligned,
 * receives n_i doubles (n_i is windows[i]->N or gh * gw); it may be NULL only when
 * n_i == 0.  d_variance is optional: NULL, or NULL entries, give no variances for
 * those images; an entry is 8-byte aligned and receives n_i doubles.  Nothing is
 * written outside those bytes.  Images are packed RGB8 device images of any sizes
 * from T x T at any base alignment; no byte outside an image's 3 * H * W is read
 * (rows are read as aligned dwords; the dwords that hold an image's first and
 * last bytes are read byte by byte).
 * Refused with -1 before any device work (also on a machine without a GPU),
 * phd_last_error naming image and window: NULL arguments, a NULL image,
 * n_images <= 0, a size below T, a window size outside the four, a box whose sides
 * are not T or that leaves the image, a non-positive stride, a NULL d_sharpness
 * entry of an image that has windows, more than 2^31 - 1 windows.
 * One launch (profile slot 16) takes every window of every image: 256-thread
 * blocks, one window per block at 128 and 64 and one per wave at 32 and 16, the
 * window's luma in LDS as int32.  Per call one table upload (a 16-byte record and
 * a destination pair per window) and no allocation.  Enqueued on `stream` and not
 * waited for, or (NULL) on the library's stream and waited for, as
 * phd_pack_views_device.  A call with no window at all does no device work and
 * returns 0.  0 or -1. */
/* Window lists, as phd_blur_vectors_device takes them. */
int phd_sharpness_windows_device(const uint8_t* const* d_images, const int* heights, const int* widths,
                                 int n_images, const Crop_Boundaries* const* windows, int window,
                                 double* const* d_sharpness, double* const* d_variance, void* stream);
/* A regular grid per image: window_grid's rule, gh = (H - T) / stride + 1, gw = (W - T) / stride + 1,
 * row-major; stride > 0, may be smaller (overlap) or larger than the window. */
int phd_sharpness_maps_device(const uint8_t* const* d_images, const int* heights, const int* widths, int n_images,
                              int window, int stride, double* const* d_sharpness, double* const* d_variance,
                              void* stream);
/* Validation hook, host only (no GPU): the window sharpness kernel's twin
 * (get_variance_sharpness, src/filtering.c:151-183, with filter_image, :81-107,
 * get_average and get_variance, :125-148, on the crops of
 * src/image_processing.c:213-232 after rgb2pgm, :505-512): the same row code and
 * the same finish (sharp_window.h) over one packed RGB8 image of host memory at
 * any alignment.  sharpness: windows->N doubles; variance: as many, or NULL; sums:
 * S1, S2 per window (2 * windows->N), or NULL.  0, or -1 with phd_last_error. */
int phd_debug_window_sharpness_host(const uint8_t* rgb, int height, int width, const Crop_Boundaries* windows,
                                    int window, double* sharpness, double* variance, unsigned long long* sums);

/* ---- statistics maps: brightness, contrast, saturation of window grids, on the device
 * The window statistics of a T x T window (rows top <= y < top+T, columns
 * left <= x < left+T of a packed RGB8 image: crop_image's crop,
 * src/image_processing.c:244-266) are get_rgb_statistics
 * (src/image_processing.c:543-553, with get_average and get_variance,
 * src/filtering.c:125-148) and get_hsv_average over rgb2hsv's s
 * (src/image_processing.c:533-540, 372-417) of its n = T^2 pixels: the box
 * statistics' definition (phd_box_stats_device) restricted to square windows and
 * finished on the device.
 *  - M[0..2] = sum k and M[3..5] = sum k^2 per channel; n1 = #(min == 0 < max);
 *    D[m], m = 0..255: the sum of max - min over the pixels whose max is m.  All
 *    integers; at T = 128 each fits 32 bits and n M[3+c] - M[c]^2 fits 64.
 *  - The finish is the only floating point, shared by the kernel and the host twin
 *    (stat_window.h), plain IEEE fp64 operations with no fused multiply-add:
 *      B_c   = (double)M[c] / 255.0 / (double)n
 *      C_c   = sqrt((double)(n M[3+c] - M[c]^2) / 65025.0 / ((double)n * (double)n))
 *      S     = sum over m = 1..255 of (double)D[m] / (double)m, ascending, sequential
 *              (a zero term may be left out: every term is >= 0)
 *      S-bar = (S - (1.0 - 0.999999) * (double)n1) / (double)n
 * A window's seven values depend on its 3 T^2 bytes only: the same on every run
 * and wherever the window sits in a call.  None is NaN or infinite.
 *
 * window is 16, 32, 64 or 128.  d_stats[i]: device pointer, 8-byte aligned,
 * receives 7 * n_i doubles, window-major: Br Bg Bb Cr Cg Cb S-bar per window (n_i
 * is windows[i]->N or gh * gw); it may be NULL only when n_i == 0.  Nothing else
 * is written.  Images are packed RGB8 device images of any sizes from T x T at any
 * base alignment; no byte outside a window's own pixels is read (a 4-pixel unit's
 * 12 bytes are read at their own address).
 * Refused with -1 before any device work (also on a machine without a GPU),
 * phd_last_error naming image and window: NULL arguments, a NULL image,
 * n_images <= 0, a size below T, a window size outside the four, a box whose sides
 * are not T or that leaves the image, a non-positive stride, a NULL d_stats entry
 * of an image that has windows, more than 2^31 - 1 windows.
 * One launch (profile slot 17) takes every window of every image: 256-thread
 * blocks, one window per block at 128 and 64 and one per wave at 32 and 16; the
 * moments in registers, D in LDS, the finish in the block that summed the window;
 * no global atomic, no zeroed buffer, no second launch.  Per call one table upload
 * (a 16-byte record and an 8-byte destination per window) and no allocation.
 * Enqueued on `stream` and not waited for, or (NULL) on the library's stream and
 * waited for, as phd_pack_views_device.  A call with no window at all does no
 * device work and returns 0.  0 or -1. */
/* Window lists, as phd_sharpness_windows_device takes them. */
int phd_stats_windows_device(const uint8_t* const* d_images, const int* heights, const int* widths, int n_images,
                             const Crop_Boundaries* const* windows, int window, double* const* d_stats,
                             void* stream);
/* A regular grid per image: window_grid's rule, gh = (H - T) / stride + 1, gw = (W - T) / stride + 1,
 * row-major; stride > 0, may be smaller (overlap) or larger than the window. */
int phd_stats_maps_device(const uint8_t* const* d_images, const int* heights, const int* widths, int n_images,
                          int window, int stride, double* const* d_stats, void* stream);
/* Validation hook, host only (no GPU): the window statistics kernel's twin
 * (get_rgb_statistics, src/image_processing.c:543-553, and get_hsv_average,
 * :533-540, over rgb2hsv, :372-417, on the crops of :244-266; get_average and
 * get_variance, src/filtering.c:125-148): the 4-pixel unit's plain form and the
 * same finish (stat_window.h) over one packed RGB8 image of host memory at any
 * alignment.  stats: 7 doubles per window; sums: NULL, or 264 u64 per window in
 * the box statistics' record layout (M[6], n1, N, D[256]).  0, or -1 with
 * phd_last_error. */
int phd_debug_window_stats_host(const uint8_t* rgb, int height, int width, const Crop_Boundaries* windows,
                                int window, double* stats, unsigned long long* sums);

/* ---- palette maps: palette slot counts of window grids, on the device
 * The window palette of a T x T window of a label map (what the _labels entries
 * write: mh x mw uint16, row-major, PHD_LABEL_NONE for a pixel of no slot -- the
 * lists of src/color_quantization.c:342-479 and :510-576 kept per pixel; the
 * window in MAP coordinates, rows top <= y < top+T and columns left <= x <
 * left+T, as phd_box_palettes_device takes the boxes of
 * src/image_processing.c:213-232) of a palette of n_slots slots (0..4096) is the
 * box palette's definition restricted to square windows, left on the device:
 *  - counts: n_slots + 1 uint32.  Column s < n_slots is the number of the window's
 *    T^2 elements whose label is s; column n_slots counts every other element
 *    (PHD_LABEL_NONE and any label >= n_slots).  A row sums to T^2.  The integers
 *    of phd_box_palettes_device and phd_debug_box_counts_host on the same boxes.
 *  - dominant: one uint16, the column of the largest count over columns
 *    0..n_slots, the lowest column on a tie, written as s for s < n_slots and as
 *    PHD_LABEL_NONE for column n_slots ("none" wins only when strictly larger than
 *    every slot; n_slots == 0 always gives PHD_LABEL_NONE).  A grid's dominant
 *    values are a gh x gw label map of the same palette, which
 *    phd_labels_to_rgb_device paints.
 * No floating point: a window's values depend on its T^2 labels and n_slots only,
 * the same on every run and wherever the window sits in a call.
 *
 * window is 16, 32, 64 or 128.  d_counts[i]: device pointer, 4-byte aligned,
 * receives n_i x (n_slots[i] + 1) uint32, window-major; d_dominant[i]: device
 * pointer, 2-byte aligned, receives n_i uint16 (n_i is windows[i]->N or gh * gw).
 * Either array may be NULL and either may hold NULL entries -- not wanted for that
 * map --, but a map that has windows needs one of the two.  Every counter of a
 * wanted row is written (the caller zeroes nothing) and nothing else is.  Maps are
 * device label maps of any sizes from T x T at any 2-byte aligned base; no byte
 * outside a window's own labels is read (a 4-label unit's 8 bytes are read at
 * their own address).
 * Refused with -1 before any device work (also on a machine without a GPU),
 * phd_last_error naming map and window: NULL arguments or both output arrays
 * NULL, n_maps <= 0, a NULL map, a size below T, a window size outside the four,
 * a box whose sides are not T or that leaves the map, a non-positive stride,
 * n_slots[i] outside 0..4096, a map with windows and neither output, more than
 * 2^31 - 1 windows; also a misaligned map or output.
 * One launch (profile slot 18) takes every window of every map: 256-thread
 * blocks, one window per block at 128 and 64 and one per wave at 32 and 16; the
 * counters in LDS (sized by the call's largest palette, in several private copies
 * for small palettes), folded and written by the block that counted the window;
 * no global atomic, no zeroed buffer, no second launch.  Per call one table upload
 * (a 24-byte record and a 16-byte destination per window) and no allocation.
 * Enqueued on `stream` and not waited for, or (NULL) on the library's stream and
 * waited for, as phd_pack_views_device.  A call with no window at all does no
 * device work and returns 0.  0 or -1. */
/* Window lists, as phd_stats_windows_device takes them, in map coordinates. */
int phd_palette_windows_device(const uint16_t* const* d_labels, const int* map_heights, const int* map_widths,
                               int n_maps, const int* n_slots, const Crop_Boundaries* const* windows, int window,
                               uint32_t* const* d_counts, uint16_t* const* d_dominant, void* stream);
/* A regular grid per map: window_grid's rule on the map's size, gh = (mh - T) / stride + 1,
 * gw = (mw - T) / stride + 1, row-major; stride > 0, may be smaller (overlap) or larger than the window. */
int phd_palette_maps_device(const uint16_t* const* d_labels, const int* map_heights, const int* map_widths,
                            int n_maps, const int* n_slots, int window, int stride,
                            uint32_t* const* d_counts, uint16_t* const* d_dominant, void* stream);
/* Validation hook, host only (no GPU): the window palette kernel's twin -- the same
 * unit walk, clamp and dominant key (pal_window.h) over one label map of host
 * memory at any 2-byte aligned base.  counts: windows->N x (n_slots + 1) uint32;
 * dominant: windows->N uint16; either may be NULL, not both when there are
 * windows.  0, or -1 with phd_last_error. */
int phd_debug_window_palette_host(const uint16_t* map, int mh, int mw, int n_slots, const Crop_Boundaries* windows,
                                  int window, uint32_t* counts, uint16_t* dominant);

/* Palette intermediates of one device-resident image, for bit-exact checks:
 * hist[TL] (arm_octree quantities), parents[*n_parents] (valid_parents in
 * palette order), kept[*n_parents] (pixels surviving group_irregular_pixels).
 * Arrays must hold total_length (hist) / total_length (parents, kept) ints.
 * Returns total_length, or < 0 on error. */
int phd_palette_trace_device(const uint8_t* d_rgb, int height, int width, const phd_config* cfg,
                             int* hist, int* parents, int* kept, int* n_parents);

/* Per-bin element counts of the polar blur table for a height x width image
 * (image-independent, src/blur_profile.c:87-98), [angle][radius] row-major.
 * Returns 0 or < 0. */
int phd_blur_counts(int height, int width, int radius_partitions, int angle_partitions,
                    long long* counts);

/* Fill n bytes of device memory with the splitmix64 stream of
 * photohive_dsp_amd/synth.py:uniform (byte j = byte j%8 of word j/8). */
int phd_fill_uniform_device(uint8_t* d_dst, size_t n, uint64_t seed, void* stream);

/* Fill height x width x 3 bytes of device memory with
 * photohive_dsp_amd/synth.py:structured(height, width, seed, blur, blur_axis)
 * (gradient + disks + noise, then a `blur`-tap box blur along blur_axis when
 * blur > 1): the bench's SURVEY 8(d) row 2(b) images.  0 or -1. */
int phd_fill_structured_device(uint8_t* d_dst, int height, int width, uint64_t seed, int blur, int blur_axis,
                               void* stream);

/* Validation hook: per-pixel rgb2hsv and octree group id of n_pixels device
 * RGB8 pixels into d_gid[n] (and d_hsv[3n] if non-NULL). */
int phd_debug_hsv_groups_device(const uint8_t* d_rgb, long n_pixels, const phd_config* cfg, int* d_gid,
                                double* d_hsv);

/* Validation hook, host only (no GPU): the production K1's per-pixel
 * classification (k1_pixel.h) of n interleaved host RGB8 pixels -- the hue
 * cell of the fused palette, h, s, and (if deferred != NULL) whether the pixel
 * took the exact double path.  Returns 0 or -1. */
int phd_debug_k1_pixels(const uint8_t* rgb, long n, const phd_config* cfg, int* cell, double* h, double* s,
                        int* deferred);

/* Host only (no device needed): which palette kernels a full-resolution report
 * of this configuration runs, as the library's own limits decide it.  -1 for a
 * configuration the library rejects, else a mask: 1 the one-pass (fused)
 * palette, else K1 histogram + Kcut + K3; 2 the table K1 runs word-aligned
 * batches, 4 in its two-block form; 8 the saturation class comes from
 * per-value thresholds (s_partitions <= 6), else from the table in global
 * memory; 16 the grid has a K1 code table; 32 the palette's second pass of an
 * image with max_slots palette slots is the batched one (one Kcut and one K3
 * launch per batch), else one pair of launches per image. */
int phd_debug_palette_path(const phd_config* cfg, int max_slots);

/* Micro-benchmark hook: average ms per launch of one pipeline kernel (0 hsv_stats,
 * 1 fft_rows, 2 fft_cols) over `iters` launches on a device image; `ablate` is a
 * debug mask (0 = production kernel). */
int phd_debug_time_kernel(int kernel, const uint8_t* d_rgb, int height, int width, const phd_config* cfg,
                          int ablate, int iters, double* avg_ms);

/* Validation hook: the power spectrum |X[u][k]|^2 (src/fft_processing.c:48-50)
 * of one device RGB8 image through the production FFT kernels, column-major
 * into d_out[(width/2+1) * height] (device memory).  0, -2 when the size has
 * no compile-time FFT plan, or -1. */
int phd_debug_power_spectrum(const uint8_t* d_rgb, int height, int width, double* d_out);
/* log_mant, the polar bins' table-driven fp64 log, over n positive device doubles. */
int phd_debug_log_mant(const double* d_x, double* d_y, long n);
/* Test hook: n complex transforms of length 3000 (interleaved re, im; device
 * memory, natural order in and out, unnormalised, e^{-i}) through the
 * 320-thread column plan whose radix-20 last pass is split over lane pairs
 * (DESIGN.md section 16), one block each.  0 or -1. */
int phd_debug_fft_split_pass(const double* d_x, double* d_X, int n);
/* Host only (no device needed): entries (runs of one polar bin + a sentinel)
 * of the longest spectrum column of this size and bin grid.  Above 256 the
 * compile-time column pass cannot hold the column's list and the size takes
 * the runtime-plan FFT.  Returns the count or -1. */
int phd_debug_col_runs_max(int height, int width, int radius_partitions, int angle_partitions);
/* Test hook: the compile-time column pass's form for later calls of this
 * process: -1 the library's choice (default), 0 the half-prefetch form, 1 the
 * full-prefetch form where the plan has one.
 * Returns the previous setting. */
int phd_debug_column_form(int mode);

/* Validation hook for the global-memory FFTs behind sides above 8192 px and
 * lengths with a large prime factor (the reference's FFTW r2c takes any
 * length, src/fft_processing.c:18-63): `count` contiguous complex sequences
 * of length n (device, interleaved re/im) -> their unnormalised forward DFTs
 * (e^{-i}) in d_out (d_out == d_in allowed).  Returns the plan kind (0 one
 * LDS pass, 1 four-step, 2 Bluestein) or -1. */
int phd_debug_gfft(const double* d_in, double* d_out, int n, long count);

/* Test hook (no GPU): a report tree in get_full_report_data's allocation shape
 * (n_palette colours, na x nr bins, n_crops sharpnesses or none when < 0),
 * filled with a fixed pattern and live for free_full_report. */
Full_Report_Data* phd_debug_legacy_report(int n_palette, int na, int nr, int n_crops);

/* Free an Image_PGM returned by get_blur_profile_visual. */
void phd_free_pgm(Image_PGM* img);

/* Human-readable reason for the last failure on this thread ("" if none). */
const char* phd_last_error(void);

/* Device name / arch / CU count into buf; returns the HIP device ordinal or < 0. */
int phd_device_info(char* buf, int buflen);

/* Stage timing of the most recent report call (ms).  Device, from HIP events:
 * [0] K1 (hsv + stats + palette sums), [1] FFT rows + columns, [2] palette
 * pass 2 left after the FFTs, [3] whole device span.  Host wall clock: [4]
 * whole call, [5] enqueue, [6] palette decisions + pass-2 enqueue, [7]
 * report assembly.  Returns the number of stages written (<= n). */
int phd_last_timings(double* ms, int n);

/* Per-kernel GPU time from HIP events recorded on the launch stream around
 * every launch of the kernels in `mask` (bit k = kernel k: 0 hsv_stats,
 * 1 fft_rows, 2 fft_cols, 3 palette_cutoffs, 4 palette_sums, 5 sharpness,
 * 6 pack_views, 7 classify_views, 8 decode_views, 9 yuv_views,
 * 10 palette_labels, 11 box_palettes, 12 box_stats, 13 the fp64 route's
 * planar_box_stats, 14 window_blur, 15 window_vectors, 16 window_sharp,
 * 17 window_stats, 18 window_palette).
 * phd_profile_kernels resets the counters; phd_profile_read returns the
 * accumulated milliseconds and launch count of one kernel. */
int phd_profile_kernels(unsigned mask);
int phd_profile_read(int kernel, double* total_ms, long* launches);

/* Lanes a device batch of >= 16 images on the library's stream is split over
 * (1 or 2; default 2, or PHD_LANES).  Each lane is an independent context with
 * its own streams and workspaces; the second runs on a library thread, so the
 * two halves' kernels, host phases and launch gaps overlap (+10-13 % images/s
 * at 4000x3000 over one lane, bench.py's one_lane object).  It applies to
 * phd_report_batch_device, phd_blur_batch_device (the second half of the
 * batch on lane 1) and phd_report_batch_device_mixed (size groups to the
 * lanes in turn).  Results do not
 * depend on it.  With
 * two lanes, phd_last_timings and PHD_VERBOSE's stage lines cover lane 0's half
 * of a batch only (the stage timings are per calling thread).  lanes < 1 only
 * queries.  Returns the previous setting. */
int phd_set_lanes(int lanes);

/* Explicit teardown (no counterpart in the reference, which frees per call,
 * src/interface.c:88-92): joins the library's threads (the second lane's
 * worker, the host pools) and releases every context's device buffers, pinned
 * buffers, events and streams after their queued work.  The library registers
 * it with atexit at its first HIP use, so it also runs before HIP's own
 * finalizers at exit; a caller may run it earlier (the next call then starts
 * afresh).  Do not call it while another thread is inside a library call. */
void phd_shutdown(void);

/* Crash triage: on SIGSEGV / SIGBUS / SIGILL / SIGFPE / SIGABRT write
 * /proc/self/maps to "<prefix>.<pid>.maps" (async-signal-safe), then hand the
 * signal to the handler installed before (or the default action).  0 on
 * success. */
int phd_install_crash_maps(const char* prefix);

/* Test hook: the library threads alive in this process (lane worker + host
 * pool threads); start != 0 creates them first. */
int phd_debug_library_threads(int start);

/* Test hook: the bytes of the grow-only device and pinned blocks of the current
 * device's contexts (lanes summed; plans and tables not counted).  Creates no
 * context: 0, 0 before the first call and after phd_shutdown.  Returns 0. */
int phd_debug_context_bytes(unsigned long long* device, unsigned long long* pinned);

#ifdef __cplusplus
}
#endif
#endif /* PHOTOHIVE_DSP_H */
