"""PhotoHive_DSP for MI355X: drop-in get_report / Report / set_bounding_boxes
backed by hand-written HIP kernels (PhotoHive_DSP_lib/libreport_data.so)."""
from .core import (Report, blur_map_device, blur_vector_maps_device, blur_vectors_device,  # noqa: F401
                   blur_windows_device, box_palettes_device,
                   box_stats_device, convert_yuv_device, window_grid,
                   decode_views_device, get_report, get_reports, make_typed_views, make_views, make_yuv_views,
                   nv12_planes, pack_views_device, palette_maps_device, palette_windows_device, quantize_device,
                   report_device, reports_device_labels,
                   reports_device_mixed, reports_device_typed, reports_device_views, reports_device_yuv,
                   set_bounding_boxes, sharpness_device, sharpness_maps_device, sharpness_windows_device,
                   stats_maps_device, stats_windows_device)
from .lib import configure_hw_queues  # noqa: F401  (opt-in GPU_MAX_HW_QUEUES, before HIP starts)
