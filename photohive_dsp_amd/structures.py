"""ctypes mirrors of the C structs (layouts of /root/reference/structures.py:6-106,
byte-identical to include/photohive_dsp.h), plus the new phd_config."""
import ctypes
from ctypes import POINTER, Structure, c_double, c_float, c_int, c_int64, c_uint, c_uint32, c_void_p

Pixel = c_double


class Sharpnesses(Structure):
    _fields_ = [("N", c_int), ("sharpness", POINTER(Pixel))]


class Blur_Vector(Structure):
    _fields_ = [("angle", c_int), ("magnitude", c_float)]


class Blur_Vector_Group(Structure):
    _fields_ = [("len_vectors", c_int), ("blur_vectors", POINTER(Blur_Vector))]


class Pixel_HSV(Structure):
    _fields_ = [("parent_id", c_int), ("h", c_double), ("s", c_double), ("v", c_double)]


class Image_RGB(Structure):
    # c_uint as in the reference binding (structures.py:36-37); same size as C int
    _fields_ = [("height", c_uint), ("width", c_uint),
                ("r", POINTER(c_double)), ("g", POINTER(c_double)), ("b", POINTER(c_double))]


class Image_PGM(Structure):
    _fields_ = [("height", c_uint), ("width", c_uint), ("data", POINTER(c_double))]


class Color_Palette(Structure):
    _fields_ = [("N", c_int), ("averages", POINTER(Pixel_HSV)), ("percentages", POINTER(c_double))]


class RGB_Statistics(Structure):
    _fields_ = [("Br", c_double), ("Bg", c_double), ("Bb", c_double),
                ("Cr", c_double), ("Cg", c_double), ("Cb", c_double)]


class Crop_Boundaries(Structure):
    _fields_ = [("N", c_int), ("top", POINTER(c_int)), ("bottom", POINTER(c_int)),
                ("left", POINTER(c_int)), ("right", POINTER(c_int))]


class Blur_Profile(Structure):
    _fields_ = [("num_angle_bins", c_int), ("num_radius_bins", c_int),
                ("angle_bin_size", c_int), ("radius_bin_size", c_int),
                ("bins", POINTER(POINTER(c_double)))]

    def get_bin_values(self):
        return [[self.bins[i][j] for j in range(self.num_radius_bins)]
                for i in range(self.num_angle_bins)]


class Full_Report_Data(Structure):
    _fields_ = [("rgb_stats", POINTER(RGB_Statistics)), ("color_palette", POINTER(Color_Palette)),
                ("blur_profile", POINTER(Blur_Profile)), ("blur_vectors", POINTER(Blur_Vector_Group)),
                ("average_saturation", c_double), ("sharpness", POINTER(Sharpnesses))]


class PhdConfig(Structure):
    """The 16 scalar get_report hyper-parameters (include/photohive_dsp.h: phd_config)."""
    _fields_ = [("h_partitions", c_int), ("s_partitions", c_int), ("v_partitions", c_int),
                ("black_thresh", c_double), ("gray_thresh", c_double), ("coverage_thresh", c_double),
                ("linked_list_size", c_int), ("downsample_rate", c_int),
                ("radius_partitions", c_int), ("angle_partitions", c_int),
                ("quantity_weight", c_float), ("saturation_value_weight", c_float),
                ("fft_streak_thresh", c_double), ("magnitude_thresh", c_double),
                ("blur_cutoff_ratio_denom", c_int)]


class PhdImageView(Structure):
    """One device-resident 8-bit image as a byte-strided view (include/photohive_dsp.h:
    phd_image_view): channel c of pixel (y, x) is the byte at
    data + y*row_stride + x*pixel_stride + c*channel_stride."""
    _fields_ = [("data", c_void_p), ("height", c_int), ("width", c_int),
                ("row_stride", c_int64), ("pixel_stride", c_int64), ("channel_stride", c_int64)]


class PhdTypedView(Structure):
    """One device-resident image of 8- / 16-bit integers, halves, floats or doubles as a
    byte-strided view (include/photohive_dsp.h: phd_typed_view): channel c of pixel (y, x)
    is the element at data + y*row_stride + x*pixel_stride + c*channel_stride (bytes) and
    its value is (double)element / max_value (0: the type's own 255, 65535 or 1.0)."""
    _fields_ = [("data", c_void_p), ("height", c_int), ("width", c_int),
                ("row_stride", c_int64), ("pixel_stride", c_int64), ("channel_stride", c_int64),
                ("elem", c_int), ("flags", c_int), ("max_value", c_double)]


class PhdYuvView(Structure):
    """One device-resident 8-bit YCbCr frame (include/photohive_dsp.h: phd_yuv_view): luma of
    pixel (y, x) is the byte at y + y*y_row_stride + x*y_pixel_stride, chroma sample (j, i)
    the byte at cb (or cr) + j*c_row_stride + i*c_pixel_stride."""
    _fields_ = [("y", c_void_p), ("cb", c_void_p), ("cr", c_void_p), ("height", c_int), ("width", c_int),
                ("y_row_stride", c_int64), ("y_pixel_stride", c_int64),
                ("c_row_stride", c_int64), ("c_pixel_stride", c_int64),
                ("chroma_shift_x", c_int), ("chroma_shift_y", c_int),
                ("matrix", c_int), ("range", c_int), ("chroma", c_int)]


class PhdBoxPalette(Structure):
    """The box palette of one label map (include/photohive_dsp.h: phd_box_palette): counts is
    n_boxes x (n_slots + 1) uint32, row-major, owned by the library until phd_free_box_palettes."""
    _fields_ = [("n_boxes", c_int), ("n_slots", c_int), ("counts", POINTER(c_uint32))]


class PhdBoxStats(Structure):
    """The box statistics of one image (include/photohive_dsp.h: phd_box_stats): n_boxes
    RGB_Statistics and n_boxes average saturations in one block, owned by the library until
    phd_free_box_stats."""
    _fields_ = [("n_boxes", c_int), ("stats", POINTER(RGB_Statistics)), ("average_saturation", POINTER(c_double))]


class PhdWindowBlur(Structure):
    """The window blur of one image (include/photohive_dsp.h: phd_window_blur): n_windows x
    na x nr bins, n_windows x 10 vectors and n_windows spectrum maxima in one block, owned by
    the library until phd_free_window_blur."""
    _fields_ = [("n_windows", c_int), ("num_angle_bins", c_int), ("num_radius_bins", c_int),
                ("angle_bin_size", c_int), ("radius_bin_size", c_int),
                ("bins", POINTER(c_double)), ("vectors", POINTER(Blur_Vector)), ("fft_max", POINTER(c_double))]


# phd_yuv_view.matrix, .range and .chroma
PHD_YUV_BT601, PHD_YUV_BT709 = range(2)
PHD_YUV_FULL, PHD_YUV_LIMITED = range(2)
PHD_YUV_CHROMA_REPLICATE, PHD_YUV_CHROMA_TRIANGLE = range(2)

# phd_typed_view.elem and .flags
PHD_ELEM_U8, PHD_ELEM_U16, PHD_ELEM_F16, PHD_ELEM_F32, PHD_ELEM_F64 = range(5)
PHD_VIEW_SNAP_U8 = 1
