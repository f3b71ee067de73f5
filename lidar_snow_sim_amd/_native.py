"""ctypes binding of libsnowgpu.so (include/snowgpu.h).  No compute happens in this file.

The library is hand-written HIP for gfx950; it is built in-tree by ``python -m lidar_snow_sim_amd.build``
(or ``__graft_entry__.build()``).  If it is missing every entry point raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path

import numpy as np

_LIB_PATH = Path(__file__).resolve().parent / "libsnowgpu.so"
_lib = None
_lock = threading.Lock()

E_OK, E_INVALID, E_HIP, E_TABLE, E_RANGE, E_CHANNELS, E_OVERFLOW, E_GROUND, E_NO_DEVICE = range(9)

EXPORTS = [
    "snowgpu_create", "snowgpu_destroy", "snowgpu_last_error", "snowgpu_version", "snowgpu_set_lasers",
    "snowgpu_upload_table", "snowgpu_table_count", "snowgpu_range_grid", "snowgpu_augment_batch",
    "snowgpu_augment_batch_device", "snowgpu_debug_occlusions", "snowgpu_wet_ground_batch",
    "snowgpu_profile_begin", "snowgpu_profile_end", "snowgpu_set_exact_math", "snowgpu_augment_wet_batch",
    "snowgpu_sample_table", "snowgpu_host_alloc", "snowgpu_host_free", "snowgpu_set_fov",
    "snowgpu_augment_wet_batch_device", "snowgpu_last_status", "snowgpu_free_table", "snowgpu_debug_table", "snowgpu_debug_table_bins", "snowgpu_file_table_device", "snowgpu_set_fov_precrop",
    "snowgpu_set_pipeline", "snowgpu_set_wet_lines", "snowgpu_set_plane_method", "snowgpu_estimate_planes",
    "snowgpu_estimate_planes_device", "snowgpu_prepass_stats", "snowgpu_set_wet_estimation", "snowgpu_wet_last_fit", "snowgpu_debug_ransac_polyfit", "snowgpu_set_result_transfer", "snowgpu_debug_transfer_times", "snowgpu_status_error", "snowgpu_set_threshold_callback", "snowgpu_augment_batch_compact", "snowgpu_set_serial", "snowgpu_lane_stream", "snowgpu_device_numa_node",
    "snowgpu_augment_batch_device_aligned", "snowgpu_wet_ground_batch_device_aligned", "snowgpu_augment_wet_batch_device_aligned",
    "snowgpu_augment_batch_device_aligned_masked", "snowgpu_augment_wet_batch_device_aligned_masked", "snowgpu_fov_mask_device",
    "snowgpu_augment_weather_batch_device_aligned", "snowgpu_draw_weather_device", "snowgpu_dror_mask_device",
    "snowgpu_voxelize_device", "snowgpu_fps_device", "snowgpu_ball_query_device", "snowgpu_range_image_device",
    "snowgpu_nearest_centres_device", "snowgpu_points_in_boxes_device", "snowgpu_boxes_iou_device", "snowgpu_nms_device", "snowgpu_fps_sectors_device",
    "snowgpu_roi_point_pool_device", "snowgpu_roi_voxel_pool_device", "snowgpu_sample_rois_device",
    "snowgpu_assign_anchors_device", "snowgpu_paste_objects_device", "snowgpu_transform_scene_device", "snowgpu_assign_centers_device",
]

WET_ESTIMATION = {"linear": 0, "poly": 1}

PLANE_METHODS = {"reference": 0, "lsq": 1, "ransac": 2}


class WeatherPlanStruct(ctypes.Structure):
    """snowgpu_weather_plan (include/snowgpu.h)."""
    _fields_ = [("p_snow", ctypes.c_double), ("p_wet", ctypes.c_double), ("n_water", ctypes.c_int32), ("n_pave", ctypes.c_int32),
                ("water_heights", ctypes.c_double * 16), ("pavement_depths", ctypes.c_double * 16), ("wet_noise_floor", ctypes.c_double),
                ("power_factor", ctypes.c_double), ("delta", ctypes.c_double), ("shuffle", ctypes.c_int32)]


def weather_plan_struct(p_snow, p_wet, water_heights, pavement_depths, noise_floor, power_factor, delta, shuffle):
    """The plan of snowgpu_draw_weather_device from Python values.  More than 16 choices are kept in n_water / n_pave as they are (the
    first 16 stored): the entry refuses them."""
    wh, pd = [float(v) for v in water_heights], [float(v) for v in pavement_depths]
    s = WeatherPlanStruct()
    s.p_snow, s.p_wet, s.n_water, s.n_pave = float(p_snow), float(p_wet), len(wh), len(pd)
    for i, v in enumerate(wh[:16]):
        s.water_heights[i] = v
    for i, v in enumerate(pd[:16]):
        s.pavement_depths[i] = v
    s.wet_noise_floor, s.power_factor, s.delta, s.shuffle = float(noise_floor), float(power_factor), float(delta), int(bool(shuffle))
    return s


CLS_SCORE_TYPES = {"roi_iou": 0, "cls": 1}


class RoiSamplerStruct(ctypes.Structure):
    """snowgpu_roi_sampler (include/snowgpu.h)."""
    _fields_ = [("roi_per_image", ctypes.c_int32), ("fg_per_image", ctypes.c_int32), ("reg_fg_thresh", ctypes.c_double), ("cls_fg_thresh", ctypes.c_double),
                ("cls_bg_thresh", ctypes.c_double), ("cls_bg_thresh_lo", ctypes.c_double), ("hard_bg_ratio", ctypes.c_double), ("cls_mode", ctypes.c_int32)]


def roi_sampler_struct(roi_per_image, fg_per_image, reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo, hard_bg_ratio, cls_mode):
    """The settings of snowgpu_sample_rois_device from Python values; a count beyond int32 reaches the entry as one it refuses."""
    s = RoiSamplerStruct()
    s.roi_per_image, s.fg_per_image, s.cls_mode = _i32(roi_per_image), _i32(fg_per_image), _i32(cls_mode)
    s.reg_fg_thresh, s.cls_fg_thresh, s.cls_bg_thresh = float(reg_fg_thresh), float(cls_fg_thresh), float(cls_bg_thresh)
    s.cls_bg_thresh_lo, s.hard_bg_ratio = float(cls_bg_thresh_lo), float(hard_bg_ratio)
    return s


OUTSIDE_MODES = {"clamp": 0, "drop": 1}


class CenterCfgStruct(ctypes.Structure):
    """snowgpu_center_cfg (include/snowgpu.h)."""
    _fields_ = [("x0", ctypes.c_double), ("y0", ctypes.c_double), ("vx", ctypes.c_double), ("vy", ctypes.c_double), ("gaussian_overlap", ctypes.c_double),
                ("stride", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("n_classes", ctypes.c_int32), ("n_heads", ctypes.c_int32),
                ("max_objs", ctypes.c_int32), ("min_radius", ctypes.c_int32), ("outside", ctypes.c_int32), ("class_head", ctypes.c_int32 * 16)]


def center_cfg_struct(x0, y0, vx, vy, stride, width, height, n_classes, n_heads, class_head, max_objs, gaussian_overlap, min_radius, outside):
    """The settings of snowgpu_assign_centers_device from Python values; a count beyond int32 reaches the entry as one it refuses.  More
    than 16 classes are kept in n_classes as they are (the first 16 heads stored): the entry refuses them."""
    s = CenterCfgStruct()
    s.x0, s.y0, s.vx, s.vy, s.gaussian_overlap = float(x0), float(y0), float(vx), float(vy), float(gaussian_overlap)
    s.stride, s.width, s.height, s.n_classes, s.n_heads = _i32(stride), _i32(width), _i32(height), _i32(n_classes), _i32(n_heads)
    s.max_objs, s.min_radius, s.outside = _i32(max_objs), _i32(min_radius), _i32(outside)
    for i, h in enumerate(list(class_head)[:16]):
        s.class_head[i] = _i32(h)
    return s


class SnowGPUError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libsnowgpu error {code}: {msg}")
        self.code = code


def lib():
    """Load libsnowgpu.so (once).  Raises RuntimeError if it has not been built."""
    global _lib
    with _lock:
        if _lib is None:
            if not _LIB_PATH.exists():
                raise RuntimeError(
                    f"{_LIB_PATH} is missing: the HIP extension has not been built. Run "
                    "`python -m lidar_snow_sim_amd.build` (needs hipcc). There is no CPU fallback.")
            L = ctypes.CDLL(str(_LIB_PATH))
            vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
            L.snowgpu_create.restype = ctypes.c_int
            L.snowgpu_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
            L.snowgpu_destroy.restype = None
            L.snowgpu_destroy.argtypes = [vp]
            L.snowgpu_last_error.restype = ctypes.c_char_p
            L.snowgpu_last_error.argtypes = [vp]
            L.snowgpu_version.restype = ctypes.c_char_p
            L.snowgpu_version.argtypes = []
            L.snowgpu_set_lasers.restype = ctypes.c_int
            L.snowgpu_set_lasers.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp]
            L.snowgpu_upload_table.restype = ctypes.c_int
            L.snowgpu_upload_table.argtypes = [vp, ctypes.c_int, vp, i64]
            L.snowgpu_file_table_device.restype = ctypes.c_int
            L.snowgpu_file_table_device.argtypes = [vp, ctypes.c_int, vp, i64]
            L.snowgpu_debug_table.restype = ctypes.c_int
            L.snowgpu_debug_table.argtypes = [vp, ctypes.c_int, vp, i64]
            L.snowgpu_debug_table_bins.restype = ctypes.c_int
            L.snowgpu_debug_table_bins.argtypes = [vp, ctypes.c_int, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp]
            L.snowgpu_free_table.restype = ctypes.c_int
            L.snowgpu_free_table.argtypes = [vp, ctypes.c_int]
            L.snowgpu_table_count.restype = ctypes.c_int
            L.snowgpu_table_count.argtypes = [vp]
            L.snowgpu_range_grid.restype = ctypes.c_int
            L.snowgpu_range_grid.argtypes = [vp]
            L.snowgpu_augment_batch.restype = ctypes.c_int
            L.snowgpu_augment_batch.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, dbl, vp, vp, dbl, vp,
                                                vp, vp, vp, vp, vp]
            L.snowgpu_augment_batch_compact.restype = ctypes.c_int
            L.snowgpu_augment_batch_compact.argtypes = [vp, ctypes.c_int, vp, vp, vp, vp, dbl, vp, vp, dbl, vp, vp, vp, vp, vp]
            L.snowgpu_augment_batch_device.restype = ctypes.c_int
            L.snowgpu_augment_batch_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, vp, dbl, vp, vp,
                                                       dbl, vp, vp, vp, vp, vp, vp, vp, vp]
            L.snowgpu_augment_batch_device_aligned.restype = ctypes.c_int
            L.snowgpu_augment_batch_device_aligned.argtypes = L.snowgpu_augment_batch_device.argtypes      # (d_out_keep where d_out_src is)
            L.snowgpu_debug_occlusions.restype = ctypes.c_int
            L.snowgpu_debug_occlusions.argtypes = [vp, i64, vp, ctypes.c_int, vp, dbl, ctypes.c_int, vp, vp, vp, vp]
            L.snowgpu_wet_ground_batch.restype = ctypes.c_int
            L.snowgpu_wet_ground_batch.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, dbl, dbl, dbl, dbl,
                                                   ctypes.c_int, dbl, ctypes.c_int, vp, vp, vp, vp]
            L.snowgpu_augment_wet_batch.restype = ctypes.c_int
            L.snowgpu_augment_wet_batch.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, dbl, vp, vp, dbl, vp, vp,
                                                    dbl, dbl, dbl, dbl, ctypes.c_int, dbl, ctypes.c_int, vp, vp, vp, vp, vp]
            L.snowgpu_augment_wet_batch_device.restype = ctypes.c_int
            L.snowgpu_augment_wet_batch_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, vp, dbl, vp, vp, dbl, vp,
                                                           vp, dbl, dbl, dbl, dbl, ctypes.c_int, dbl, ctypes.c_int, vp, vp, vp, vp, vp,
                                                           vp, vp]
            L.snowgpu_wet_ground_batch_device_aligned.restype = ctypes.c_int
            L.snowgpu_wet_ground_batch_device_aligned.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, vp, vp, dbl, dbl, dbl, dbl,
                                                                  ctypes.c_int, dbl, ctypes.c_int, vp, vp, vp, vp, vp, vp]
            L.snowgpu_augment_wet_batch_device_aligned.restype = ctypes.c_int
            L.snowgpu_augment_wet_batch_device_aligned.argtypes = L.snowgpu_augment_batch_device_aligned.argtypes + [
                vp, dbl, dbl, dbl, dbl, ctypes.c_int, dbl, ctypes.c_int, vp]
            base = L.snowgpu_augment_batch_device_aligned.argtypes                  # (the masked forms: d_keep_in behind d_perm)
            L.snowgpu_augment_batch_device_aligned_masked.restype = ctypes.c_int
            L.snowgpu_augment_batch_device_aligned_masked.argtypes = base[:13] + [vp] + base[13:]
            L.snowgpu_augment_wet_batch_device_aligned_masked.restype = ctypes.c_int
            L.snowgpu_augment_wet_batch_device_aligned_masked.argtypes = base[:13] + [vp] + base[13:] + [
                vp, dbl, dbl, dbl, dbl, ctypes.c_int, dbl, ctypes.c_int, vp]
            L.snowgpu_augment_weather_batch_device_aligned.restype = ctypes.c_int               # (d_weather in place of the five wet doubles)
            L.snowgpu_augment_weather_batch_device_aligned.argtypes = base[:13] + [vp] + base[13:] + [vp, vp, ctypes.c_int, ctypes.c_int, vp]
            L.snowgpu_draw_weather_device.restype = ctypes.c_int
            L.snowgpu_draw_weather_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.POINTER(WeatherPlanStruct),
                                                      ctypes.c_uint64, vp, vp, vp, vp]
            L.snowgpu_sample_rois_device.restype = ctypes.c_int
            L.snowgpu_sample_rois_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int,
                                                     ctypes.POINTER(RoiSamplerStruct), ctypes.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.snowgpu_assign_anchors_device.restype = ctypes.c_int
            L.snowgpu_assign_anchors_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), vp, vp, vp, vp, vp, vp]
            L.snowgpu_assign_centers_device.restype = ctypes.c_int
            L.snowgpu_assign_centers_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(CenterCfgStruct), vp, vp, vp, vp,
                                                        vp, vp, vp, vp, vp]
            L.snowgpu_paste_objects_device.restype = ctypes.c_int
            L.snowgpu_paste_objects_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, i64, i64, vp, vp, vp, vp, vp,
                                                       ctypes.c_int, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.snowgpu_transform_scene_device.restype = ctypes.c_int
            L.snowgpu_transform_scene_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp,
                                                         ctypes.c_int, vp, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.snowgpu_fov_mask_device.restype = ctypes.c_int
            L.snowgpu_fov_mask_device.argtypes = [vp, i64, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
            L.snowgpu_dror_mask_device.restype = ctypes.c_int
            L.snowgpu_dror_mask_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, dbl, dbl, dbl, i64, vp, vp, vp, vp]
            L.snowgpu_voxelize_device.restype = ctypes.c_int
            L.snowgpu_voxelize_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  vp, vp, vp, vp, vp, vp, vp]
            L.snowgpu_fps_device.restype = ctypes.c_int
            L.snowgpu_fps_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp]
            L.snowgpu_fps_sectors_device.restype = ctypes.c_int
            L.snowgpu_fps_sectors_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp,
                                                     ctypes.c_int, ctypes.c_int, dbl, vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.snowgpu_ball_query_device.restype = ctypes.c_int
            L.snowgpu_ball_query_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp,
                                                    ctypes.c_int, vp, vp, vp, vp, vp]
            L.snowgpu_range_image_device.restype = ctypes.c_int
            L.snowgpu_range_image_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_int,
                                                     vp, vp, vp, vp, vp, vp]
            L.snowgpu_nearest_centres_device.restype = ctypes.c_int
            L.snowgpu_nearest_centres_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int,
                                                         vp, vp, vp, vp, vp]
            L.snowgpu_points_in_boxes_device.restype = ctypes.c_int
            L.snowgpu_points_in_boxes_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, vp, vp,
                                                         vp, vp]
            L.snowgpu_roi_point_pool_device.restype = ctypes.c_int
            L.snowgpu_roi_point_pool_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int,
                                                        ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
            L.snowgpu_roi_voxel_pool_device.restype = ctypes.c_int
            L.snowgpu_roi_voxel_pool_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, vp, ctypes.c_int,
                                                        ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.snowgpu_boxes_iou_device.restype = ctypes.c_int
            L.snowgpu_boxes_iou_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   vp, vp, vp, vp, vp, vp]
            L.snowgpu_nms_device.restype = ctypes.c_int
            L.snowgpu_nms_device.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                             ctypes.c_int, vp, vp, vp, vp, vp, vp, vp]
            L.snowgpu_set_fov_precrop.restype = ctypes.c_int
            L.snowgpu_set_fov_precrop.argtypes = [vp, ctypes.c_int]
            L.snowgpu_last_status.restype = ctypes.c_int
            L.snowgpu_last_status.argtypes = [vp, vp]
            L.snowgpu_set_threshold_callback.restype = ctypes.c_int
            L.snowgpu_set_threshold_callback.argtypes = [vp, vp, vp]
            L.snowgpu_status_error.restype = ctypes.c_int
            L.snowgpu_status_error.argtypes = [vp, vp]
            L.snowgpu_set_fov.restype = ctypes.c_int
            L.snowgpu_set_fov.argtypes = [vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_int]
            L.snowgpu_sample_table.restype = ctypes.c_int
            L.snowgpu_sample_table.argtypes = [vp, ctypes.c_int, dbl, dbl, dbl, ctypes.c_uint64, vp, i64, vp]
            L.snowgpu_set_wet_lines.restype = ctypes.c_int
            L.snowgpu_set_wet_lines.argtypes = [vp, ctypes.c_int, vp]
            L.snowgpu_set_wet_estimation.restype = ctypes.c_int
            L.snowgpu_set_wet_estimation.argtypes = [vp, ctypes.c_int, ctypes.c_uint64]
            L.snowgpu_debug_ransac_polyfit.restype = ctypes.c_int
            L.snowgpu_debug_ransac_polyfit.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_uint64, ctypes.c_uint64, vp]
            L.snowgpu_wet_last_fit.restype = ctypes.c_int
            L.snowgpu_wet_last_fit.argtypes = [vp, ctypes.c_int, vp]
            L.snowgpu_set_plane_method.restype = ctypes.c_int
            L.snowgpu_set_plane_method.argtypes = [vp, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, dbl]
            L.snowgpu_estimate_planes.restype = ctypes.c_int
            L.snowgpu_estimate_planes.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp]
            L.snowgpu_estimate_planes_device.restype = ctypes.c_int
            L.snowgpu_estimate_planes_device.argtypes = [vp, ctypes.c_int, i64, i64, vp, vp, ctypes.c_int, vp, vp, vp]
            L.snowgpu_prepass_stats.restype = ctypes.c_int
            L.snowgpu_prepass_stats.argtypes = [vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp, vp]
            L.snowgpu_device_numa_node.restype = ctypes.c_int
            L.snowgpu_device_numa_node.argtypes = [ctypes.c_int]
            L.snowgpu_set_result_transfer.restype = ctypes.c_int
            L.snowgpu_set_result_transfer.argtypes = [vp, ctypes.c_int, ctypes.c_int]
            L.snowgpu_debug_transfer_times.restype = ctypes.c_int
            L.snowgpu_debug_transfer_times.argtypes = [vp, vp]
            L.snowgpu_set_pipeline.restype = ctypes.c_int
            L.snowgpu_set_pipeline.argtypes = [vp, i64]
            L.snowgpu_set_serial.restype = ctypes.c_int
            L.snowgpu_set_serial.argtypes = [vp, ctypes.c_int]
            L.snowgpu_lane_stream.restype = ctypes.c_int
            L.snowgpu_lane_stream.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
            L.snowgpu_set_exact_math.restype = ctypes.c_int
            L.snowgpu_set_exact_math.argtypes = [vp, ctypes.c_int]
            L.snowgpu_profile_begin.restype = ctypes.c_int
            L.snowgpu_profile_begin.argtypes = [vp, ctypes.c_int]
            L.snowgpu_profile_end.restype = ctypes.c_int
            L.snowgpu_profile_end.argtypes = [vp, vp, vp]
            L.snowgpu_host_alloc.restype = ctypes.c_int
            L.snowgpu_host_alloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
            L.snowgpu_host_free.restype = ctypes.c_int
            L.snowgpu_host_free.argtypes = [vp, vp]
            _lib = L
    return _lib


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _dtype_code(dt):
    if dt == np.float32:
        return 0
    if dt == np.float64:
        return 1
    raise TypeError(f"rows must be float32 or float64, not {dt}")


def _i32(v):
    """int(v) clamped to int32: a count beyond it reaches the entry as one it refuses, not as a ctypes error."""
    return max(-(2 ** 31), min(int(v), 2 ** 31 - 1))


def _range6(who, rng):
    """point_cloud_range as 6 contiguous float64, None for None."""
    if rng is None:
        return None
    rng = np.ascontiguousarray(rng, np.float64).reshape(-1)
    if rng.shape != (6,):
        raise ValueError(f"{who}: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1)")
    return rng


def range_grid():
    out = np.zeros(1230)
    rc = lib().snowgpu_range_grid(_p(out))
    if rc:
        raise SnowGPUError(rc, "snowgpu_range_grid")
    return out


class Context:
    """One libsnowgpu context = one device + one stream + its uploaded tables."""

    def __init__(self, device: int = 0):
        self._L = lib()
        h = ctypes.c_void_p()
        rc = self._L.snowgpu_create(int(device), ctypes.byref(h))
        self._h = h
        self.device = int(device)
        if rc:
            msg = self._L.snowgpu_last_error(h).decode() if h else "no usable HIP device"
            if h:
                self._L.snowgpu_destroy(h)
                self._h = None
            raise SnowGPUError(rc, msg)
        self.n_lasers = 0
        self._call_lock = threading.Lock()

    def close(self):
        if getattr(self, "_h", None):
            self._L.snowgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise SnowGPUError(rc, self._L.snowgpu_last_error(self._h).decode())

    def _check_args(self, rc):
        """_check() for the stage entries: an argument outside the domain (E_INVALID) raises ValueError with the entry's words."""
        if rc == E_INVALID:
            raise ValueError(self._L.snowgpu_last_error(self._h).decode())
        self._check(rc)

    @property
    def handle(self):
        return self._h

    def set_lasers(self, focal_slope, focal_offset, min_intensity, max_intensity):
        fs = np.ascontiguousarray(focal_slope, np.float64)
        fo = np.ascontiguousarray(focal_offset, np.float64)
        mi = np.ascontiguousarray(min_intensity, np.int32)
        ma = np.ascontiguousarray(max_intensity, np.int32)
        self._check(self._L.snowgpu_set_lasers(self._h, len(fs), _p(fs), _p(fo), _p(mi), _p(ma)))
        self.n_lasers = len(fs)

    def upload_table(self, table_id: int, xyr):
        t = np.ascontiguousarray(xyr, np.float64)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("a particle table is K x 3 (x, y, disk radius)")
        with self._call_lock:             # never while a batch of this context is in flight (it reads the table list)
            self._check(self._L.snowgpu_upload_table(self._h, int(table_id), _p(t), t.shape[0]))

    def file_table_device(self, table_id: int, d_xyr: int, n_flakes: int):
        """File a K x 3 float64 table that already lives in device memory (d_xyr: device pointer as int)."""
        with self._call_lock:
            self._check(self._L.snowgpu_file_table_device(self._h, int(table_id), ctypes.c_void_p(d_xyr), int(n_flakes)))

    def free_table(self, table_id: int):
        with self._call_lock:
            self._check(self._L.snowgpu_free_table(self._h, int(table_id)))

    def pinned_empty(self, shape, dtype):
        """An uninitialised NumPy array in page-locked host memory (snowgpu_host_alloc); freed with the array."""
        import weakref
        dtype = np.dtype(dtype)
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(v) for v in shape)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        ptr = ctypes.c_void_p()
        self._check(self._L.snowgpu_host_alloc(self._h, ctypes.c_size_t(nbytes), ctypes.byref(ptr)))
        buf = (ctypes.c_char * max(nbytes, 1)).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)
        L, addr = self._L, ptr.value       # page-locked memory is not tied to the context: the array may outlive it
        weakref.finalize(buf, lambda: L.snowgpu_host_free(None, ctypes.c_void_p(addr)))
        return arr

    def augment_batch(self, rows, frame_offsets, table_ids, beam_divergence, thr_poly=None, plane=None,
                      noise_floor=0.7, perm=None, want_thr=False, out_rows=None, out_src=None, want_src=True, rows_resident=False):
        """rows: N_total x 5 (float32/float64), frame_offsets: n_frames + 1, table_ids: n_frames x n_lasers.
        out_rows / out_src: optional caller-owned result buffers (at least N_total rows; pinned_empty() ones move at
        PCIe speed and are not page-faulted in on every call).  want_src=False: the source indices stay on the device
        (out_src is returned as None).  rows_resident: `rows` are the rows of the immediately preceding prepass_stats() call --
        they are still on the device and are not uploaded again (rows = NULL at the C ABI).

        Returns (out_rows [N_total x 5, only the first counts[f] rows of each frame slot are valid],
                 out_src, counts, stats[n_frames x 3], thr_poly or None)."""
        rows = np.ascontiguousarray(rows)
        code = _dtype_code(rows.dtype)
        off = np.ascontiguousarray(frame_offsets, np.int64)
        nf = len(off) - 1
        tids = np.ascontiguousarray(table_ids, np.int32).reshape(nf, -1)
        if tids.shape[1] != self.n_lasers:
            raise ValueError("table_ids must be n_frames x n_lasers")
        n = int(off[-1])
        if out_rows is None:
            out_rows = np.empty((n, 5), rows.dtype)
        elif out_rows.dtype != rows.dtype or out_rows.ndim != 2 or out_rows.shape[1] != 5 or out_rows.shape[0] < n \
                or not out_rows.flags.c_contiguous:
            raise ValueError("out_rows must be a C-contiguous (>= N_total) x 5 array of the input dtype")
        if not want_src:
            out_src = None
        elif out_src is None:
            out_src = np.empty(n, np.int32)
        elif out_src.dtype != np.int32 or out_src.ndim != 1 or out_src.shape[0] < n or not out_src.flags.c_contiguous:
            raise ValueError("out_src must be a C-contiguous int32 array of >= N_total entries")
        counts = np.zeros(nf, np.int64)
        stats = np.zeros((nf, 3), np.int64)
        thr = None if thr_poly is None else np.ascontiguousarray(thr_poly, np.float64).reshape(nf, 3)
        pl = None if plane is None else np.ascontiguousarray(plane, np.float64).reshape(nf, 4)
        pm = None if perm is None else np.ascontiguousarray(perm, np.int32)
        out_thr = np.zeros((nf, 3)) if want_thr else None
        with self._call_lock:
            rc = self._L.snowgpu_augment_batch(self._h, nf, _p(off), None if rows_resident else _p(rows), code, _p(tids), float(beam_divergence),
                                               _p(thr), _p(pl), float(noise_floor), _p(pm), _p(out_rows), _p(out_src),
                                               _p(counts), _p(stats), _p(out_thr))
            err = getattr(self, "_thr_error", None)
            if rc and err is not None:                       # the threshold callback raised: its exception, not the status code
                self._thr_error = None
                raise err
            self._check(rc)
        return out_rows, out_src, counts, stats, out_thr

    def augment_batch_compact(self, xyzi, channels, frame_offsets, table_ids, beam_divergence, thr_poly=None, plane=None, noise_floor=0.7,
                              want_thr=False, out_rows=None, out_src=None, want_src=True):
        """augment_batch for frames given as (x, y, z, intensity) float32 rows + one channel byte per row (17 instead of 20 bytes per point up
        the link: snowgpu_augment_batch_compact).  Same results as augment_batch on the (x, y, z, intensity, channel) rows."""
        xyzi = np.ascontiguousarray(xyzi, np.float32)
        ch = np.ascontiguousarray(channels, np.uint8)
        off = np.ascontiguousarray(frame_offsets, np.int64)
        nf, n = len(off) - 1, int(off[-1])
        if xyzi.ndim != 2 or xyzi.shape[1] != 4 or xyzi.shape[0] < n or ch.shape[0] < n:
            raise ValueError("xyzi must be N x 4 float32 and channels N uint8")
        tids = np.ascontiguousarray(table_ids, np.int32).reshape(nf, -1)
        if tids.shape[1] != self.n_lasers:
            raise ValueError("table_ids must be n_frames x n_lasers")
        if out_rows is None:
            out_rows = np.empty((n, 5), np.float32)
        if not want_src:
            out_src = None
        elif out_src is None:
            out_src = np.empty(n, np.int32)
        counts = np.zeros(nf, np.int64)
        stats = np.zeros((nf, 3), np.int64)
        thr = None if thr_poly is None else np.ascontiguousarray(thr_poly, np.float64).reshape(nf, 3)
        pl = None if plane is None else np.ascontiguousarray(plane, np.float64).reshape(nf, 4)
        out_thr = np.zeros((nf, 3)) if want_thr else None
        with self._call_lock:
            rc = self._L.snowgpu_augment_batch_compact(self._h, nf, _p(off), _p(xyzi), _p(ch), _p(tids), float(beam_divergence), _p(thr), _p(pl),
                                                       float(noise_floor), _p(out_rows), _p(out_src), _p(counts), _p(stats), _p(out_thr))
            err = getattr(self, "_thr_error", None)
            if rc and err is not None:
                self._thr_error = None
                raise err
            self._check(rc)
        return out_rows, out_src, counts, stats, out_thr

    def augment_batch_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, d_table_ids, beam_divergence,
                             d_thr_poly, d_plane, noise_floor, d_perm, d_out_rows, d_out_src, d_out_counts,
                             d_out_stats, d_out_thr, d_status, stream=0):
        """Raw device-pointer entry (ints from tensor.data_ptr()); asynchronous on `stream`."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_augment_batch_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off), vp(d_rows),
                                                  int(dtype_code), vp(d_table_ids), float(beam_divergence),
                                                  vp(d_thr_poly or None), vp(d_plane or None), float(noise_floor),
                                                  vp(d_perm or None), vp(d_out_rows), vp(d_out_src), vp(d_out_counts),
                                                  vp(d_out_stats), vp(d_out_thr or None), vp(d_status), vp(stream or None))
        self._check(rc)

    def augment_batch_device_aligned(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, d_table_ids, beam_divergence,
                                     d_thr_poly, d_plane, noise_floor, d_perm, d_out_rows, d_out_keep, d_out_counts,
                                     d_out_stats, d_out_thr, d_status, stream=0):
        """Raw device-pointer entry with the aligned result layout (rows in input order + one keep byte per row; d_out_rows may be
        d_rows); asynchronous on `stream`."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_augment_batch_device_aligned(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off), vp(d_rows),
                                                          int(dtype_code), vp(d_table_ids), float(beam_divergence),
                                                          vp(d_thr_poly or None), vp(d_plane or None), float(noise_floor),
                                                          vp(d_perm or None), vp(d_out_rows), vp(d_out_keep), vp(d_out_counts),
                                                          vp(d_out_stats), vp(d_out_thr or None), vp(d_status), vp(stream or None))
        self._check(rc)

    def augment_wet_batch_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, d_table_ids,
                                 beam_divergence, d_thr_poly, d_plane, noise_floor, d_perm, d_wet_plane, water_height,
                                 pavement_depth, wet_noise_floor, power_factor, flat_earth, delta, replace, d_out_rows, d_out_src,
                                 d_out_counts, d_out_stats, d_out_flags, d_status, stream=0):
        """Raw device-pointer entry of the fused snowfall + wet-ground chain; asynchronous on `stream`."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_augment_wet_batch_device(
            self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off), vp(d_rows), int(dtype_code),
            vp(d_table_ids), float(beam_divergence), vp(d_thr_poly or None), vp(d_plane or None), float(noise_floor),
            vp(d_perm or None), vp(d_wet_plane or None), float(water_height), float(pavement_depth), float(wet_noise_floor),
            float(power_factor), int(bool(flat_earth)), float(delta), int(bool(replace)), vp(d_out_rows), vp(d_out_src),
            vp(d_out_counts), vp(d_out_stats), vp(d_out_flags), vp(d_status), vp(stream or None))
        self._check(rc)

    def wet_ground_batch_device_aligned(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, d_keep_in, d_plane,
                                        water_height, pavement_depth, noise_floor, power_factor, flat_earth, delta, replace, d_out_rows,
                                        d_out_keep, d_out_counts, d_out_flags, d_status, stream=0):
        """Raw device-pointer entry of the wet-ground model with the aligned result (rows of the input's dtype in input order + one keep
        byte per row; d_keep_in 0 = every row present; d_out_rows may be d_rows, d_out_keep d_keep_in); asynchronous on `stream`."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_wet_ground_batch_device_aligned(
            self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off), vp(d_rows or None), int(dtype_code),
            vp(d_keep_in or None), vp(d_plane or None), float(water_height), float(pavement_depth), float(noise_floor), float(power_factor),
            int(bool(flat_earth)), float(delta), int(bool(replace)), vp(d_out_rows or None), vp(d_out_keep or None), vp(d_out_counts or None),
            vp(d_out_flags or None), vp(d_status or None), vp(stream or None))
        self._check(rc)

    def augment_wet_batch_device_aligned(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, d_table_ids,
                                         beam_divergence, d_thr_poly, d_plane, noise_floor, d_perm, d_out_rows, d_out_keep, d_out_counts,
                                         d_out_stats, d_out_thr, d_status, stream, d_wet_plane, water_height, pavement_depth,
                                         wet_noise_floor, power_factor, flat_earth, delta, replace, d_out_flags):
        """Raw device-pointer entry of the fused snowfall + wet-ground chain with the aligned result: augment_batch_device_aligned's
        arguments, then the wet ones, then d_out_flags; asynchronous on `stream`."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_augment_wet_batch_device_aligned(
            self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off), vp(d_rows or None), int(dtype_code),
            vp(d_table_ids), float(beam_divergence), vp(d_thr_poly or None), vp(d_plane or None), float(noise_floor),
            vp(d_perm or None), vp(d_out_rows or None), vp(d_out_keep or None), vp(d_out_counts or None), vp(d_out_stats or None),
            vp(d_out_thr or None), vp(d_status or None), vp(stream or None), vp(d_wet_plane or None), float(water_height),
            float(pavement_depth), float(wet_noise_floor), float(power_factor), int(bool(flat_earth)), float(delta), int(bool(replace)),
            vp(d_out_flags or None))
        self._check(rc)

    def augment_batch_device_aligned_masked(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, d_table_ids, beam_divergence,
                                            d_thr_poly, d_plane, noise_floor, d_perm, d_keep_in, d_out_rows, d_out_keep, d_out_counts,
                                            d_out_stats, d_out_thr, d_status, stream=0):
        """augment_batch_device_aligned with an input keep mask (d_keep_in: one byte per row, 0 = the row is not there; 0 as the pointer =
        all present; d_out_keep may be d_keep_in); asynchronous on `stream`."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_augment_batch_device_aligned_masked(
            self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off), vp(d_rows or None), int(dtype_code), vp(d_table_ids),
            float(beam_divergence), vp(d_thr_poly or None), vp(d_plane or None), float(noise_floor), vp(d_perm or None), vp(d_keep_in or None),
            vp(d_out_rows or None), vp(d_out_keep or None), vp(d_out_counts), vp(d_out_stats), vp(d_out_thr or None), vp(d_status), vp(stream or None))
        self._check(rc)

    def augment_wet_batch_device_aligned_masked(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, d_table_ids,
                                                beam_divergence, d_thr_poly, d_plane, noise_floor, d_perm, d_keep_in, d_out_rows, d_out_keep,
                                                d_out_counts, d_out_stats, d_out_thr, d_status, stream, d_wet_plane, water_height,
                                                pavement_depth, wet_noise_floor, power_factor, flat_earth, delta, replace, d_out_flags):
        """augment_wet_batch_device_aligned whose snowfall stage takes an input keep mask (d_keep_in behind d_perm); asynchronous on `stream`."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_augment_wet_batch_device_aligned_masked(
            self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off), vp(d_rows or None), int(dtype_code),
            vp(d_table_ids), float(beam_divergence), vp(d_thr_poly or None), vp(d_plane or None), float(noise_floor),
            vp(d_perm or None), vp(d_keep_in or None), vp(d_out_rows or None), vp(d_out_keep or None), vp(d_out_counts or None),
            vp(d_out_stats or None), vp(d_out_thr or None), vp(d_status or None), vp(stream or None), vp(d_wet_plane or None),
            float(water_height), float(pavement_depth), float(wet_noise_floor), float(power_factor), int(bool(flat_earth)), float(delta),
            int(bool(replace)), vp(d_out_flags or None))
        self._check(rc)

    def augment_weather_batch_device_aligned(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, d_table_ids,
                                             beam_divergence, d_thr_poly, d_plane, noise_floor, d_perm, d_keep_in, d_out_rows, d_out_keep,
                                             d_out_counts, d_out_stats, d_out_thr, d_status, stream, d_wet_plane, d_weather, flat_earth,
                                             replace, d_out_flags):
        """augment_wet_batch_device_aligned_masked with per-frame weather records in device memory (d_weather: n_frames x 8 float64 --
        snow gate, wet gate, water height, pavement depth, wet noise floor, power factor, delta, 0) in place of its five wet scalars;
        asynchronous on `stream`."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_augment_weather_batch_device_aligned(
            self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off), vp(d_rows or None), int(dtype_code),
            vp(d_table_ids), float(beam_divergence), vp(d_thr_poly or None), vp(d_plane or None), float(noise_floor),
            vp(d_perm or None), vp(d_keep_in or None), vp(d_out_rows or None), vp(d_out_keep or None), vp(d_out_counts or None),
            vp(d_out_stats or None), vp(d_out_thr or None), vp(d_status or None), vp(stream or None), vp(d_wet_plane or None),
            vp(d_weather or None), int(bool(flat_earth)), int(bool(replace)), vp(d_out_flags or None))
        self._check(rc)

    def draw_weather_device(self, n_frames, n_lasers, n_sets, d_set_ids, plan, seed, d_step, d_table_ids, d_weather, stream=0):
        """Draw every frame's table ids (n_frames x n_lasers int32) and weather record (n_frames x 8 float64) on the device from Philox keyed
        by (seed; the step in device memory, frame).  plan: a WeatherPlanStruct (weather_plan_struct); asynchronous on `stream`."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_draw_weather_device(self._h, int(n_frames), int(n_lasers), int(n_sets), vp(d_set_ids or None),
                                                 ctypes.byref(plan) if plan is not None else None, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                 vp(d_step or None), vp(d_table_ids or None), vp(d_weather or None), vp(stream or None))
        self._check(rc)

    def fov_mask_device(self, n_total, d_rows, dtype_code, calib, img_shape, d_keep_in, d_out_keep, stream=0):
        """d_out_keep[i] = (d_keep_in ? d_keep_in[i] : 1) and the camera-FOV test of row i (calib: V2C, R0, P2 as for set_fov);
        asynchronous on `stream`."""
        vp = ctypes.c_void_p
        v2c = np.ascontiguousarray(calib.V2C, np.float64).reshape(3, 4)
        r0 = np.ascontiguousarray(calib.R0, np.float64).reshape(3, 3)
        p2 = np.ascontiguousarray(calib.P2, np.float64).reshape(3, 4)
        self._check(self._L.snowgpu_fov_mask_device(self._h, int(n_total), vp(d_rows or None), int(dtype_code), _p(v2c), _p(r0), _p(p2),
                                                    int(img_shape[0]), int(img_shape[1]), vp(d_keep_in or None), vp(d_out_keep or None),
                                                    vp(stream or None)))

    def dror_mask_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, alpha, beta, sr_min, k_min, d_keep_in,
                         d_out_keep, d_out_neighbours=0, stream=0):
        """Dynamic radius outlier removal as a keep mask (include/snowgpu.h: snowgpu_dror_mask_device); asynchronous on `stream`.  A
        parameter outside the domain, or d_out_keep overlapping d_keep_in, raises ValueError."""
        vp = ctypes.c_void_p
        k = int(k_min)
        rc = self._L.snowgpu_dror_mask_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                              int(dtype_code), float(alpha), float(beta), float(sr_min), max(-1, min(k, 1 << 62)), vp(d_keep_in or None),
                                              vp(d_out_keep or None), vp(d_out_neighbours or None), vp(stream or None))
        self._check_args(rc)

    def voxelize_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, point_cloud_range, voxel_size, max_points,
                        max_voxels, n_features, d_keep_in, d_out_voxels, d_out_coords, d_out_num_points, d_out_voxel_offsets, d_out_voxel_of=0,
                        stream=0):
        """Point-to-voxel grouping of an aligned batch (include/snowgpu.h: snowgpu_voxelize_device); asynchronous on `stream`.  An argument
        outside the domain, or d_out_voxel_of overlapping d_keep_in, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        rng = np.ascontiguousarray(point_cloud_range, np.float64).reshape(-1)
        size = np.ascontiguousarray(voxel_size, np.float64).reshape(-1)
        if rng.shape != (6,) or size.shape != (3,):
            raise ValueError("snowgpu_voxelize_device: point_cloud_range holds 6 numbers (x0, y0, z0, x1, y1, z1), voxel_size 3")
        rc = self._L.snowgpu_voxelize_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                             int(dtype_code), _p(rng), _p(size), _i32(max_points), _i32(max_voxels), _i32(n_features), vp(d_keep_in or None),
                                             vp(d_out_voxels or None), vp(d_out_coords or None), vp(d_out_num_points or None),
                                             vp(d_out_voxel_offsets or None), vp(d_out_voxel_of or None), vp(stream or None))
        self._check_args(rc)

    def fps_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, point_cloud_range, n_samples, n_features, d_keep_in,
                   d_out_index, d_out_points, d_out_dist, d_out_usable, stream=0):
        """Farthest-point keypoints of an aligned batch (include/snowgpu.h: snowgpu_fps_device); asynchronous on `stream`.
        point_cloud_range: 6 numbers or None.  An argument outside the domain, or an output overlapping the mask or the rows, raises
        ValueError with the entry's words."""
        vp = ctypes.c_void_p
        rng = _range6("snowgpu_fps_device", point_cloud_range)
        rc = self._L.snowgpu_fps_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                        int(dtype_code), _p(rng), _i32(n_samples), _i32(n_features), vp(d_keep_in or None),
                                        vp(d_out_index or None), vp(d_out_points or None), vp(d_out_dist or None), vp(d_out_usable or None),
                                        vp(stream or None))
        self._check_args(rc)

    def fps_sectors_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, point_cloud_range, n_samples, n_features, d_keep_in,
                           n_sectors, d_rois, n_rois, roi_features, roi_margin, d_out_index, d_out_points, d_out_dist, d_out_usable, d_out_sector_offsets,
                           d_out_sector_count, d_out_sector_of=0, d_out_reach2=0, stream=0):
        """Sectorized, proposal-centric keypoints of an aligned batch (include/snowgpu.h: snowgpu_fps_sectors_device); asynchronous on
        `stream`.  point_cloud_range: 6 numbers or None; d_rois 0: no roi test.  An argument outside the domain, or an output overlapping
        the mask, the rows, the rois or another output, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        rng = _range6("snowgpu_fps_sectors_device", point_cloud_range)
        rc = self._L.snowgpu_fps_sectors_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                                int(dtype_code), _p(rng), _i32(n_samples), _i32(n_features), vp(d_keep_in or None),
                                                _i32(n_sectors), vp(d_rois or None), _i32(n_rois), _i32(roi_features), float(roi_margin),
                                                vp(d_out_index or None), vp(d_out_points or None), vp(d_out_dist or None), vp(d_out_usable or None),
                                                vp(d_out_sector_offsets or None), vp(d_out_sector_count or None), vp(d_out_sector_of or None),
                                                vp(d_out_reach2 or None), vp(stream or None))
        self._check_args(rc)

    def ball_query_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, point_cloud_range, n_centres, d_centres,
                          centre_features, radii, n_samples, n_features, d_keep_in, d_out_index, d_out_count, d_out_points, stream=0):
        """Ball-query neighbour groups around centres (include/snowgpu.h: snowgpu_ball_query_device); asynchronous on `stream`.
        point_cloud_range: 6 numbers or None; radii and n_samples: sequences of equal length.  An argument outside the domain, or an
        output overlapping the mask, the rows or the centres, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        rng = _range6("snowgpu_ball_query_device", point_cloud_range)
        rad = np.ascontiguousarray(radii, np.float64).reshape(-1)
        ns = np.ascontiguousarray([_i32(v) for v in n_samples], np.int32).reshape(-1)
        if len(rad) != len(ns):
            raise ValueError("snowgpu_ball_query_device: as many radii as sample counts")
        rc = self._L.snowgpu_ball_query_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                               int(dtype_code), _p(rng), _i32(n_centres), vp(d_centres or None),
                                               _i32(centre_features), len(rad), _p(rad), _p(ns), _i32(n_features), vp(d_keep_in or None),
                                               vp(d_out_index or None), vp(d_out_count or None), vp(d_out_points or None), vp(stream or None))
        self._check_args(rc)

    def range_image_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, height, width, fov, d_ring, range_limits,
                           n_features, d_keep_in, d_out_image, d_out_index, d_out_pixel_of, d_out_count, stream=0):
        """Range-image projection of an aligned batch (include/snowgpu.h: snowgpu_range_image_device); asynchronous on `stream`.
        fov: (up, down) in RADIANS or None (image rows by channel: d_ring); range_limits: (lo, hi) or None.  An argument outside the
        domain, or an output overlapping the rows, the mask, the channels or another output, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        pair = {}
        for name, v in (("fov", fov), ("range_limits", range_limits)):
            pair[name] = None
            if v is not None:
                pair[name] = np.ascontiguousarray(v, np.float64).reshape(-1)
                if pair[name].shape != (2,):
                    raise ValueError(f"snowgpu_range_image_device: {name} holds 2 numbers")
        rc = self._L.snowgpu_range_image_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                                int(dtype_code), _i32(height), _i32(width), None if pair["fov"] is None else _p(pair["fov"]),
                                                vp(d_ring or None), None if pair["range_limits"] is None else _p(pair["range_limits"]), _i32(n_features),
                                                vp(d_keep_in or None), vp(d_out_image or None), vp(d_out_index or None), vp(d_out_pixel_of or None),
                                                vp(d_out_count or None), vp(stream or None))
        self._check_args(rc)

    def nearest_centres_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, point_cloud_range, n_centres, d_centres,
                               centre_features, k, d_keep_in, d_out_index, d_out_dist2, d_out_weight, stream=0):
        """The k nearest centres of every row (include/snowgpu.h: snowgpu_nearest_centres_device); asynchronous on `stream`.
        point_cloud_range: 6 numbers or None.  An argument outside the domain, or an output overlapping the mask, the rows, the centres
        or another output, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        rng = _range6("snowgpu_nearest_centres_device", point_cloud_range)
        rc = self._L.snowgpu_nearest_centres_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                                    int(dtype_code), _p(rng), _i32(n_centres), vp(d_centres or None),
                                                    _i32(centre_features), _i32(k), vp(d_keep_in or None), vp(d_out_index or None),
                                                    vp(d_out_dist2 or None), vp(d_out_weight or None), vp(stream or None))
        self._check_args(rc)

    def points_in_boxes_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, n_boxes, d_boxes, box_features, d_pose_in,
                               d_keep_in, d_out_box_of, d_out_count, d_out_local, d_out_pose, stream=0):
        """The box of every row and the rows of every box (include/snowgpu.h: snowgpu_points_in_boxes_device); asynchronous on `stream`.
        d_pose_in, d_keep_in, d_out_count, d_out_local and d_out_pose may be 0.  An argument outside the domain, or an output overlapping
        the mask, the rows, the boxes, the given pose or another output, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_points_in_boxes_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                                    int(dtype_code), _i32(n_boxes), vp(d_boxes or None), _i32(box_features), vp(d_pose_in or None),
                                                    vp(d_keep_in or None), vp(d_out_box_of or None), vp(d_out_count or None), vp(d_out_local or None),
                                                    vp(d_out_pose or None), vp(stream or None))
        self._check_args(rc)

    def roi_point_pool_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, n_rois, d_rois, roi_features, extra_width,
                              n_samples, num_features, d_pose_in, d_keep_in, d_out_index, d_out_count, d_out_points, d_out_local, d_out_pose, stream=0):
        """The first n_samples rows inside every enlarged roi, in row order (include/snowgpu.h: snowgpu_roi_point_pool_device); asynchronous
        on `stream`.  extra_width: None or three numbers (host).  d_pose_in, d_keep_in, d_out_points, d_out_local and d_out_pose may be 0.
        An argument outside the domain, or an output overlapping the mask, the rows, the rois, the given pose or another output, raises
        ValueError with the entry's words."""
        vp = ctypes.c_void_p
        ew = None if extra_width is None else np.ascontiguousarray(extra_width, np.float64).reshape(3)
        rc = self._L.snowgpu_roi_point_pool_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                                   int(dtype_code), _i32(n_rois), vp(d_rois or None), _i32(roi_features), None if ew is None else _p(ew),
                                                   _i32(n_samples), _i32(num_features), vp(d_pose_in or None), vp(d_keep_in or None),
                                                   vp(d_out_index or None), vp(d_out_count or None), vp(d_out_points or None), vp(d_out_local or None),
                                                   vp(d_out_pose or None), vp(stream or None))
        self._check_args(rc)

    def roi_voxel_pool_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, n_rois, d_rois, roi_features, extra_width,
                              out_size, max_points, roi_capacity, d_features, feature_channels, d_pose_in, d_keep_in, d_out_roi_count, d_out_count,
                              d_out_index, d_out_max, d_out_argmax, d_out_avg, d_out_pose, stream=0):
        """The members of every sub-voxel of every enlarged roi and their pooled features (include/snowgpu.h: snowgpu_roi_voxel_pool_device);
        asynchronous on `stream`.  extra_width: None or three numbers (host); out_size: three whole numbers (host).  d_features, d_pose_in,
        d_keep_in, d_out_index, d_out_max, d_out_argmax, d_out_avg and d_out_pose may be 0.  An argument outside the domain, or an output
        overlapping the mask, the rows, the rois, the given pose, the features or another output, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        ew = None if extra_width is None else np.ascontiguousarray(extra_width, np.float64).reshape(3)
        grid = np.ascontiguousarray(out_size, np.int32).reshape(3)
        rc = self._L.snowgpu_roi_voxel_pool_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                                   int(dtype_code), _i32(n_rois), vp(d_rois or None), _i32(roi_features), None if ew is None else _p(ew),
                                                   _p(grid), _i32(max_points), _i32(roi_capacity), vp(d_features or None), _i32(feature_channels),
                                                   vp(d_pose_in or None), vp(d_keep_in or None), vp(d_out_roi_count or None), vp(d_out_count or None),
                                                   vp(d_out_index or None), vp(d_out_max or None), vp(d_out_argmax or None), vp(d_out_avg or None),
                                                   vp(d_out_pose or None), vp(stream or None))
        self._check_args(rc)

    def boxes_iou_device(self, n_frames, n_a, d_boxes_a, a_features, n_b, d_boxes_b, b_features, dtype_code, mode, d_pose_a, d_pose_b, d_out_iou,
                         d_out_best, d_out_best_iou, stream=0):
        """The IoU of every box a with every box b of its frame and the best b of every a (include/snowgpu.h: snowgpu_boxes_iou_device);
        asynchronous on `stream`.  mode 0: BEV, 1: 3D.  The poses and up to two of the outputs may be 0.  An argument outside the domain, or an
        output overlapping an input or another output, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_boxes_iou_device(self._h, _i32(n_frames), _i32(n_a), vp(d_boxes_a or None), _i32(a_features), _i32(n_b), vp(d_boxes_b or None),
                                              _i32(b_features), int(dtype_code), int(mode), vp(d_pose_a or None), vp(d_pose_b or None), vp(d_out_iou or None),
                                              vp(d_out_best or None), vp(d_out_best_iou or None), vp(stream or None))
        self._check_args(rc)

    def nms_device(self, n_frames, n_boxes, d_boxes, box_features, d_scores, dtype_code, mode, iou_thresh, score_thresh, post_max, d_pose_in, d_out_index,
                   d_out_count, d_out_boxes, d_out_scores, d_out_kept, stream=0):
        """The keep list of rotated NMS per frame (include/snowgpu.h: snowgpu_nms_device); asynchronous on `stream`.  d_pose_in, d_out_boxes,
        d_out_scores and d_out_kept may be 0.  An argument outside the domain, or an output overlapping an input or another output, raises
        ValueError with the entry's words."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_nms_device(self._h, _i32(n_frames), _i32(n_boxes), vp(d_boxes or None), _i32(box_features), vp(d_scores or None), int(dtype_code),
                                        int(mode), float(iou_thresh), float(score_thresh), _i32(post_max), vp(d_pose_in or None), vp(d_out_index or None),
                                        vp(d_out_count or None), vp(d_out_boxes or None), vp(d_out_scores or None), vp(d_out_kept or None), vp(stream or None))
        self._check_args(rc)

    def sample_rois_device(self, n_frames, n_rois, d_rois, roi_features, d_overlap, d_assignment, n_gt, d_gt_boxes, gt_features, dtype_code, cfg, seed, d_step,
                           d_pose, d_out_index, d_out_rois, d_out_roi_iou, d_out_gt_index, d_out_gt_of_rois, d_out_reg_valid, d_out_cls_label, d_out_segments,
                           d_out_class_count, d_out_pose, d_out_gt_local, stream=0):
        """The sampled rois of every frame and their targets (include/snowgpu.h: snowgpu_sample_rois_device); asynchronous on `stream`.
        cfg: a RoiSamplerStruct (roi_sampler_struct), read during the call; d_step: a uint64 in device memory, read by the kernel.  d_pose,
        d_out_pose and d_out_gt_local may be 0.  An argument outside the domain, or an output overlapping an input or another output,
        raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_sample_rois_device(self._h, _i32(n_frames), _i32(n_rois), vp(d_rois or None), _i32(roi_features), vp(d_overlap or None),
                                                vp(d_assignment or None), _i32(n_gt), vp(d_gt_boxes or None), _i32(gt_features), int(dtype_code),
                                                ctypes.byref(cfg) if cfg is not None else None, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), vp(d_step or None),
                                                vp(d_pose or None), vp(d_out_index or None), vp(d_out_rois or None), vp(d_out_roi_iou or None),
                                                vp(d_out_gt_index or None), vp(d_out_gt_of_rois or None), vp(d_out_reg_valid or None),
                                                vp(d_out_cls_label or None), vp(d_out_segments or None), vp(d_out_class_count or None),
                                                vp(d_out_pose or None), vp(d_out_gt_local or None), vp(stream or None))
        self._check_args(rc)

    def assign_anchors_device(self, n_frames, n_anchors, d_anchors, anchor_features, d_anchor_class, n_gt, d_gt_boxes, gt_features, dtype_code, matched, unmatched,
                              d_out_label, d_out_gt_index, d_out_count, d_out_gt_count, d_out_iou, stream=0):
        """The anchor targets of every frame (include/snowgpu.h: snowgpu_assign_anchors_device); asynchronous on `stream`.  matched and
        unmatched: one host float per class, read during the call; their common length is n_classes.  d_out_iou may be 0.  An argument
        outside the domain, or an output overlapping an input or another output, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        m, u = [float(v) for v in matched], [float(v) for v in unmatched]
        if len(m) != len(u):
            raise ValueError("assign_anchors_device: matched and unmatched hold one value per class each")
        rc = self._L.snowgpu_assign_anchors_device(self._h, _i32(n_frames), _i32(n_anchors), vp(d_anchors or None), _i32(anchor_features), vp(d_anchor_class or None),
                                                   _i32(n_gt), vp(d_gt_boxes or None), _i32(gt_features), int(dtype_code), _i32(len(m)),
                                                   (ctypes.c_double * max(len(m), 1))(*m), (ctypes.c_double * max(len(u), 1))(*u), vp(d_out_label or None),
                                                   vp(d_out_gt_index or None), vp(d_out_count or None), vp(d_out_gt_count or None), vp(d_out_iou or None),
                                                   vp(stream or None))
        self._check_args(rc)

    def assign_centers_device(self, n_frames, n_gt, d_gt_boxes, gt_features, dtype_code, cfg, d_out_heatmap, d_out_gt_index, d_out_ind, d_out_mask, d_out_offset,
                              d_out_radius, d_out_count, d_out_state, stream=0):
        """The centre heatmap targets of every frame (include/snowgpu.h: snowgpu_assign_centers_device); asynchronous on `stream`.  cfg: a
        CenterCfgStruct (center_cfg_struct), read during the call.  An argument outside the domain, or an output overlapping the gt boxes
        or another output, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        rc = self._L.snowgpu_assign_centers_device(self._h, _i32(n_frames), _i32(n_gt), vp(d_gt_boxes or None), _i32(gt_features), int(dtype_code),
                                                   ctypes.byref(cfg) if cfg is not None else None, vp(d_out_heatmap or None), vp(d_out_gt_index or None),
                                                   vp(d_out_ind or None), vp(d_out_mask or None), vp(d_out_offset or None), vp(d_out_radius or None),
                                                   vp(d_out_count or None), vp(d_out_state or None), vp(stream or None))
        self._check_args(rc)

    def paste_objects_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, n_gt, d_gt_boxes, gt_features, d_pose_in, n_bank_points,
                             n_bank_objects, d_bank_points, d_bank_offsets, d_bank_boxes, d_bank_pose, d_class_offsets, sample_groups, extra_width, seed, d_step,
                             d_keep_in, d_out_rows, d_out_keep, d_out_gt_boxes, d_out_object, d_out_state, d_out_source, d_out_count, d_out_pose, stream=0):
        """Database objects pasted into the absent slots of an aligned batch (include/snowgpu.h: snowgpu_paste_objects_device); asynchronous
        on `stream`.  sample_groups: one whole number per class (host), their number is n_classes; extra_width: None or three numbers (host);
        d_step: a uint64 in device memory, read by the kernel.  d_pose_in, d_keep_in, d_out_source and d_out_pose may be 0.  An argument
        outside the domain, or an output overlapping an input or another output, raises ValueError with the entry's words."""
        vp = ctypes.c_void_p
        groups = np.ascontiguousarray([_i32(v) for v in sample_groups], np.int32).reshape(-1)
        ew = None if extra_width is None else np.ascontiguousarray(extra_width, np.float64).reshape(3)
        rc = self._L.snowgpu_paste_objects_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                                  int(dtype_code), _i32(n_gt), vp(d_gt_boxes or None), _i32(gt_features), vp(d_pose_in or None),
                                                  int(n_bank_points), int(n_bank_objects), vp(d_bank_points or None), vp(d_bank_offsets or None),
                                                  vp(d_bank_boxes or None), vp(d_bank_pose or None), vp(d_class_offsets or None), _i32(len(groups)),
                                                  _p(groups if len(groups) else np.zeros(1, np.int32)), None if ew is None else _p(ew), ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                  vp(d_step or None), vp(d_keep_in or None), vp(d_out_rows or None), vp(d_out_keep or None),
                                                  vp(d_out_gt_boxes or None), vp(d_out_object or None), vp(d_out_state or None), vp(d_out_source or None),
                                                  vp(d_out_count or None), vp(d_out_pose or None), vp(stream or None))
        self._check_args(rc)

    def transform_scene_device(self, n_frames, n_total, max_frame_rows, d_frame_off, d_rows, dtype_code, n_boxes, d_gt_boxes, box_features, d_pose_in, flip,
                               rotation, scaling, tries, local_translation, local_rotation, local_scaling, seed, d_step, d_box_of, d_keep_in, d_out_rows,
                               d_out_keep, d_out_gt_boxes, d_out_world, d_out_state, d_out_tried, d_out_local, d_out_pose, d_out_tries, stream=0):
        """World flip, rotation and scaling and per-object noise of an aligned batch and its gt boxes (include/snowgpu.h:
        snowgpu_transform_scene_device); asynchronous on `stream`.  flip: bit 0 the x axis, bit 1 the y axis; rotation, scaling,
        local_rotation, local_scaling: None or (lo, hi), local_translation: None or three numbers (all host); tries 0: no local part; d_step:
        a uint64 in device memory, read by the kernel.  d_pose_in, d_box_of, d_keep_in, d_out_pose and d_out_tries may be 0; d_out_rows may
        be d_rows.  An argument outside the domain, or an output overlapping an input or another output, raises ValueError with the
        entry's words."""
        vp = ctypes.c_void_p
        held = [None if v is None else np.ascontiguousarray(v, np.float64).reshape(n) for v, n in
                ((rotation, 2), (scaling, 2), (local_translation, 3), (local_rotation, 2), (local_scaling, 2))]
        rot, sc, lt, lr, ls = (None if v is None else _p(v) for v in held)
        rc = self._L.snowgpu_transform_scene_device(self._h, int(n_frames), int(n_total), int(max_frame_rows), vp(d_frame_off or None), vp(d_rows or None),
                                                    int(dtype_code), _i32(n_boxes), vp(d_gt_boxes or None), _i32(box_features), vp(d_pose_in or None), _i32(flip),
                                                    rot, sc, _i32(tries), lt, lr, ls, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), vp(d_step or None),
                                                    vp(d_box_of or None), vp(d_keep_in or None), vp(d_out_rows or None), vp(d_out_keep or None),
                                                    vp(d_out_gt_boxes or None), vp(d_out_world or None), vp(d_out_state or None), vp(d_out_tried or None),
                                                    vp(d_out_local or None), vp(d_out_pose or None), vp(d_out_tries or None), vp(stream or None))
        self._check_args(rc)

    def set_fov(self, calib=None, img_shape=(1024, 1920), pre_crop=False):
        """Camera-FOV crop inside the compaction of every later batch (None switches it off).  `calib` carries V2C (3 x 4),
        R0 (3 x 3) and P2 (3 x 4), as lidar_snow_sim_amd.calibration.Calibration does.  pre_crop: also crop the input frames
        before the augmentation (precompute.py:96-99)."""
        with self._call_lock:
            self._check(self._L.snowgpu_set_fov_precrop(self._h, int(bool(pre_crop and calib is not None))))
            if calib is None:
                self._check(self._L.snowgpu_set_fov(self._h, 0, None, None, None, 0, 0))
                return
            v2c = np.ascontiguousarray(calib.V2C, np.float64).reshape(3, 4)
            r0 = np.ascontiguousarray(calib.R0, np.float64).reshape(3, 3)
            p2 = np.ascontiguousarray(calib.P2, np.float64).reshape(3, 4)
            self._check(self._L.snowgpu_set_fov(self._h, 1, _p(v2c), _p(r0), _p(p2), int(img_shape[0]), int(img_shape[1])))

    def set_plane_method(self, method="reference", seed=0, trials=1000, min_rows=5, standard_height=-1.55):
        """How this context estimates the ground plane when a call brings none (planes.py:12-50): 'reference' (what the
        reference returns today: the flat-earth plane), 'lsq' or 'ransac' (Philox-seeded)."""
        if method not in PLANE_METHODS:
            raise ValueError("plane method must be 'reference', 'lsq' or 'ransac'")
        with self._call_lock:
            self._check(self._L.snowgpu_set_plane_method(self._h, PLANE_METHODS[method], ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                         int(trials), int(min_rows), float(standard_height)))

    def estimate_planes(self, rows, frame_offsets):
        """(planes n_frames x 4 (wx, wy, wz, h), info n_frames x 4 int32) by the context's plane method."""
        rows = np.ascontiguousarray(rows)
        code = _dtype_code(rows.dtype)
        off = np.ascontiguousarray(frame_offsets, np.int64)
        nf = len(off) - 1
        planes = np.zeros((nf, 4), np.float64)
        info = np.zeros((nf, 4), np.int32)
        with self._call_lock:
            self._check(self._L.snowgpu_estimate_planes(self._h, nf, _p(off), _p(rows), code, _p(planes), _p(info)))
        return planes, info

    def prepass_stats(self, rows, frame_offsets, plane=None, hist_out=None):
        """(hist n_frames x 50 x 2555 int32, rec n_frames x 18 float64): the device half of the noise-threshold prepass
        (snowgpu_prepass_stats) for a caller that takes the histogram's row minima with its own NumPy (quirk Q8)."""
        rows = np.ascontiguousarray(rows)
        code = _dtype_code(rows.dtype)
        off = np.ascontiguousarray(frame_offsets, np.int64)
        nf = len(off) - 1
        pl = None if plane is None else np.ascontiguousarray(plane, np.float64).reshape(nf, 4)
        if hist_out is not None and hist_out.size >= nf * 50 * 2555 and hist_out.dtype == np.int32 and hist_out.flags.c_contiguous:
            hist = hist_out.reshape(-1)[:nf * 50 * 2555].reshape(nf, 50, 2555)     # e.g. a page-locked buffer kept by the caller
        else:
            hist = np.empty((nf, 50, 2555), np.int32)
        rec = np.empty((nf, 18), np.float64)
        with self._call_lock:
            self._check(self._L.snowgpu_prepass_stats(self._h, nf, _p(off), _p(rows), code, _p(pl), _p(hist), _p(rec)))
        return hist, rec

    def sample_table(self, table_id, occupancy_ratio, diameter_scale_mm, r_0, seed, want_rows=True):
        """Sample a snowflake table on the device (and file it there under table_id >= 0).  Returns the K x 3 rows, or K
        when want_rows is False (the rows then never leave the device)."""
        n = ctypes.c_int64(0)
        args = (float(occupancy_ratio), float(diameter_scale_mm), float(r_0), ctypes.c_uint64(int(seed)))
        with self._call_lock:
            if not want_rows:
                self._check(self._L.snowgpu_sample_table(self._h, int(table_id), *args, None, 0, ctypes.byref(n)))
                return n.value
            # one run: a buffer for twice the expected flake count (E[disk area] = pi s^2 / 3 for Exp(s) sphere diameters)
            s_m = float(diameter_scale_mm) / 1000.0
            cap = int(2.0 * occupancy_ratio * r_0 * r_0 / (s_m * s_m / 3.0)) + 4096
            out = np.empty((cap, 3), np.float64)
            rc = self._L.snowgpu_sample_table(self._h, int(table_id), *args, _p(out), cap, ctypes.byref(n))
            if rc == E_INVALID and n.value > cap:            # buffer too small after all: fetch with the exact size
                out = np.empty((n.value, 3), np.float64)
                rc = self._L.snowgpu_sample_table(self._h, int(table_id), *args, _p(out), n.value, ctypes.byref(n))
            self._check(rc)
        return np.ascontiguousarray(out[:n.value])

    def debug_table(self, table_id, n_flakes):
        """K x 4 per-flake quantities of a filed table by table row: range, azimuth, right and left tangent angle."""
        out = np.zeros((int(n_flakes), 4), np.float64)
        with self._call_lock:
            self._check(self._L.snowgpu_debug_table(self._h, int(table_id), _p(out), int(n_flakes)))
        return out

    ENTRY_DTYPE = np.dtype([("phi", "f8"), ("x", "f8"), ("y", "f8"), ("r", "f8"), ("t0", "f8"), ("t1", "f8"), ("rho", "f8"),
                            ("flags", "u4"), ("src", "u4")])        # SgEntry (csrc/sg_common.h), 64 bytes

    def debug_table_bins(self, table_id):
        """The whole filed table as the scan reads it (snowgpu_debug_table_bins): dict of bin_start (2049 uint32), entries (n_entries + 1
        records of ENTRY_DTYPE, the last one the spare record), bin_q (2048 x 16 uint32), bin_qs (qs_steps x 2049 uint32, or None for a
        table without one), n_flakes, n_entries, max_bin, qs_steps, qs_per_m."""
        info, per_m = np.full(5, -1, np.int64), np.zeros(1, np.float64)
        n_bins, q_steps = 2048, 16                                  # SG_NBINS, SG_QSTEPS
        start, q = np.zeros(n_bins + 1, np.uint32), np.zeros((n_bins, q_steps), np.uint32)
        ent, qs = np.zeros(1, self.ENTRY_DTYPE), np.zeros(1, np.uint32)
        with self._call_lock:
            # sizes first: the entry writes info before it checks the capacities
            rc = self._L.snowgpu_debug_table_bins(self._h, int(table_id), _p(start), 0, _p(ent), 0, _p(q), 0, _p(qs), 0, _p(info), _p(per_m))
            if rc != E_INVALID or info[1] < 0:
                self._check(rc)
                raise SnowGPUError(E_INVALID, "snowgpu_debug_table_bins accepted buffers of no capacity")
            n_entries, qs_steps, has_qs = int(info[1]), int(info[3]), bool(info[4])
            ent = np.zeros(n_entries + 1, self.ENTRY_DTYPE)
            qs = np.zeros((qs_steps, n_bins + 1) if has_qs else (1, 1), np.uint32)
            self._check(self._L.snowgpu_debug_table_bins(self._h, int(table_id), _p(start), start.size, _p(ent), ent.size, _p(q), q.size,
                                                         _p(qs), qs.size if has_qs else 0, _p(info), _p(per_m)))
        return dict(bin_start=start, entries=ent, bin_q=q, bin_qs=qs if has_qs else None, n_flakes=int(info[0]), n_entries=int(info[1]),
                    max_bin=int(info[2]), qs_steps=int(info[3]), qs_per_m=float(per_m[0]))

    def last_status(self):
        """int32[8] status words of the last host-entry batch ([2..5]: beams per later capacity tier; [6]: beams the row kernels redid with the pairwise sum)."""
        out = np.zeros(8, np.int32)
        self._check(self._L.snowgpu_last_status(self._h, _p(out)))
        return out

    THRESHOLD_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
                                    ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double))

    def set_threshold_callback(self, fit=None):
        """fit(first_frame, hist[n, 50, 2555] int32, rec[n, 18] float64) -> n x 3 polynomials, called by the following augment_batch calls
        (those without thr_poly) once per group of frames while the per-beam kernels of the group run (snowgpu_set_threshold_callback);
        None: the device fits the threshold itself again.  An exception raised by `fit` fails the call and is re-raised by augment_batch."""
        self._thr_error = None
        if fit is None:
            self._thr_cb = None
            self._check(self._L.snowgpu_set_threshold_callback(self._h, None, None))
            return

        def trampoline(_user, first, n, hist_p, rec_p, out_p):
            try:
                hist = np.ctypeslib.as_array(hist_p, shape=(n, 50, 2555))
                rec = np.ctypeslib.as_array(rec_p, shape=(n, 18))
                out = np.ctypeslib.as_array(out_p, shape=(n, 3))
                out[...] = np.asarray(fit(int(first), hist, rec), np.float64).reshape(n, 3)
                return 0
            except BaseException as ex:      # (no exception may cross the C frames)
                self._thr_error = ex
                return 1

        self._thr_cb = self.THRESHOLD_FN(trampoline)             # kept alive as long as the library may call it
        self._check(self._L.snowgpu_set_threshold_callback(self._h, ctypes.cast(self._thr_cb, ctypes.c_void_p), None))

    def check_status(self, status8):
        """Raise what the int32[8] status words of a device-pointer call say (snowgpu_status_error); no-op for status8[0] == 0."""
        st = np.ascontiguousarray(status8, np.int32)
        if st[0] != 0:
            self._check(self._L.snowgpu_status_error(self._h, _p(st)))

    def set_result_transfer(self, mode="rows", threads=0):
        """How a pipelined host batch's results cross the link: 'rows' (output rows + source indices) or 'packed' (source | label +
        intensity per kept row; `threads` host threads of the library assemble the rows from the caller's input)."""
        if mode not in ("rows", "packed"):
            raise ValueError("mode must be 'rows' or 'packed'")
        with self._call_lock:
            self._check(self._L.snowgpu_set_result_transfer(self._h, 1 if mode == "packed" else 0, int(threads)))

    def transfer_times(self):
        out = np.zeros(4, np.float64)
        self._check(self._L.snowgpu_debug_transfer_times(self._h, _p(out)))
        return {"enqueued_ms": float(out[0]), "downloaded_ms": float(out[1]), "assembled_ms": float(out[2]), "host_threads": int(out[3])}

    def set_pipeline(self, chunk_rows: int):
        """Rows per chunk of the host entry's upload / compute / download pipeline (0: off)."""
        with self._call_lock:
            self._check(self._L.snowgpu_set_pipeline(self._h, int(chunk_rows)))

    def set_serial(self, on: bool):
        """Every kernel of a device-pointer batch on the caller's stream (snowgpu_set_serial): for contexts that run as one of several compute
        lanes, whose batches overlap each other instead of their own side streams."""
        self._check(self._L.snowgpu_set_serial(self._h, int(bool(on))))

    def lane_stream(self, level: int) -> int:
        """hipStream_t (as an integer) of the context's stream at priority level 0 / 1 / 2 = highest / normal / lowest (snowgpu_lane_stream)."""
        h = ctypes.c_void_p(0)
        self._check(self._L.snowgpu_lane_stream(self._h, int(level), ctypes.byref(h)))
        return int(h.value or 0)

    def set_exact_math(self, on: bool):
        self._check(self._L.snowgpu_set_exact_math(self._h, int(bool(on))))

    def profile_begin(self, max_launches):
        self._check(self._L.snowgpu_profile_begin(self._h, int(max_launches)))

    def profile_end(self):
        ms, n = ctypes.c_double(0.0), ctypes.c_int(0)
        self._check(self._L.snowgpu_profile_end(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def debug_occlusions(self, rows, table_ids, beam_divergence, cap=64):
        rows = np.ascontiguousarray(rows)
        code = _dtype_code(rows.dtype)
        n = rows.shape[0]
        tids = np.ascontiguousarray(table_ids, np.int32).reshape(-1)
        count = np.zeros(n, np.int32)
        rj = np.zeros((n, cap))
        ratio = np.zeros((n, cap))
        src = np.zeros(n, np.int32)
        with self._call_lock:
            self._check(self._L.snowgpu_debug_occlusions(self._h, n, _p(rows), code, _p(tids), float(beam_divergence),
                                                         int(cap), _p(count), _p(rj), _p(ratio), _p(src)))
        return count, rj, ratio, src

    def augment_wet_batch(self, rows, frame_offsets, table_ids, beam_divergence, wet_plane, thr_poly=None, plane=None,
                          noise_floor=0.7, perm=None, water_height=0.001, pavement_depth=0.0012, wet_noise_floor=0.7,
                          power_factor=15, flat_earth=False, delta=0.5, replace=False):
        rows = np.ascontiguousarray(rows)
        code = _dtype_code(rows.dtype)
        off = np.ascontiguousarray(frame_offsets, np.int64)
        nf = len(off) - 1
        tids = np.ascontiguousarray(table_ids, np.int32).reshape(nf, -1)
        n = int(off[-1])
        out_rows = np.empty((n, 5), np.float64)
        out_src = np.empty(n, np.int32)
        counts = np.zeros(nf, np.int64)
        stats = np.zeros((nf, 3), np.int64)
        flags = np.zeros(nf, np.int32)
        thr = None if thr_poly is None else np.ascontiguousarray(thr_poly, np.float64).reshape(nf, 3)
        pl = None if plane is None else np.ascontiguousarray(plane, np.float64).reshape(nf, 4)
        wpl = None if wet_plane is None else np.ascontiguousarray(wet_plane, np.float64).reshape(nf, 4)
        pm = None if perm is None else np.ascontiguousarray(perm, np.int32)
        with self._call_lock:
            self._check(self._L.snowgpu_augment_wet_batch(
                self._h, nf, _p(off), _p(rows), code, _p(tids), float(beam_divergence), _p(thr), _p(pl), float(noise_floor),
                _p(pm), _p(wpl), float(water_height), float(pavement_depth), float(wet_noise_floor), float(power_factor),
                int(bool(flat_earth)), float(delta), int(bool(replace)), _p(out_rows), _p(out_src), _p(counts), _p(stats),
                _p(flags)))
        return out_rows, out_src, counts, stats, flags

    def set_wet_estimation(self, method="linear", seed=0):
        """estimation_method of the wet-ground calls of this context: 'linear' or 'poly' (RANSAC draws from Philox keyed by `seed`)."""
        if method not in WET_ESTIMATION:
            raise ValueError("estimation_method must be 'linear' or 'poly'")
        with self._call_lock:
            self._check(self._L.snowgpu_set_wet_estimation(self._h, WET_ESTIMATION[method], int(seed) & 0xFFFFFFFFFFFFFFFF))

    def set_wet_lines(self, lines=None):
        """The two fitted lines (n_frames x 4: p slope, p intercept, noise-line slope, intercept) for the NEXT wet-ground call of this
        context, fitted by the caller (quirk Q8); one use, None clears."""
        with self._call_lock:
            if lines is None:
                self._check(self._L.snowgpu_set_wet_lines(self._h, 0, None))
            else:
                ln = np.ascontiguousarray(lines, np.float64).reshape(-1, 4)
                self._check(self._L.snowgpu_set_wet_lines(self._h, ln.shape[0], _p(ln)))

    def debug_ransac_polyfit(self, x, y, seed=0, frame=0):
        """The device's ransac_polyfit(x, y, order=2) with the draws of (seed; frame): (coefficients[3], trial kept or -1)."""
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(y, np.float64)
        out = np.zeros(4, np.float64)
        with self._call_lock:
            self._check(self._L.snowgpu_debug_ransac_polyfit(self._h, int(x.shape[0]), _p(x), _p(y), int(seed), int(frame), _p(out)))
        return out[:3], int(out[3])

    def wet_last_fit(self, n_frames):
        """The curves the last wet-ground call fitted: n_frames x 8 (power c2 c1 c0, noise c2 c1 c0, ground rows, RANSAC trial kept or -1)."""
        out = np.zeros((int(n_frames), 8), np.float64)
        with self._call_lock:
            self._check(self._L.snowgpu_wet_last_fit(self._h, int(n_frames), _p(out)))
        return out

    def wet_ground_batch(self, rows, frame_offsets, plane, water_height, pavement_depth, noise_floor, power_factor,
                         flat_earth, delta, replace, lines=None):
        """lines: optional n_frames x 4 (p slope, p intercept, noise-line slope, intercept) fitted by the caller (quirk Q8)."""
        rows = np.ascontiguousarray(rows)
        code = _dtype_code(rows.dtype)
        off = np.ascontiguousarray(frame_offsets, np.int64)
        nf = len(off) - 1
        n = int(off[-1])
        pl = None if plane is None else np.ascontiguousarray(plane, np.float64).reshape(nf, 4)
        out_rows = np.empty((n, 5), np.float64)
        out_src = np.empty(n, np.int32)
        counts = np.zeros(nf, np.int64)
        flags = np.zeros(nf, np.int32)
        with self._call_lock:
            if lines is not None:
                ln = np.ascontiguousarray(lines, np.float64).reshape(nf, 4)
                self._check(self._L.snowgpu_set_wet_lines(self._h, nf, _p(ln)))
            self._check(self._L.snowgpu_wet_ground_batch(self._h, nf, _p(off), _p(rows), code, _p(pl), float(water_height),
                                                         float(pavement_depth), float(noise_floor), float(power_factor),
                                                         int(bool(flat_earth)), float(delta), int(bool(replace)),
                                                         _p(out_rows), _p(out_src), _p(counts), _p(flags)))
        return out_rows, out_src, counts, flags
