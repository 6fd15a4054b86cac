"""ctypes binding of include/d2pc_sectors.h: the obstacle sectors of the companion library libd2pc_sectors.so.

One-to-one with the header: every function it declares is bound here and nothing else.  No compute: a polar
min-range grid is made on the device, behind the producer of the cloud, or not at all.
"""
import ctypes
import os

import numpy as np

from .capi import D2pcError

_HERE = os.path.dirname(os.path.abspath(__file__))

MAX_SECTORS, MAX_LAYERS, SHARE_POINTS = 360, 16, 1024
MAX_ELEVATION_LAYERS = 64
LAYERS_HEIGHT, LAYERS_ELEVATION = 0, 1   # layer_kind: height slabs and horizontal range / elevation angles and Euclidean range
EMPTY = 0xFFFFFFFF   # `nearest` of an empty cell

# every symbol include/d2pc_sectors.h declares (tests check the library exports all of them and nothing else)
SECTORS_SYMBOLS = [
    "d2pc_sectors_config_init", "d2pc_sectors_geometry", "d2pc_sectors_table", "d2pc_sectors_elevation_table", "d2pc_sectors_create",
    "d2pc_sectors_destroy", "d2pc_sectors_last_error", "d2pc_sectors_blocks", "d2pc_sectors_desc_init",
    "d2pc_sectors_desc_check", "d2pc_sectors_process_device",
    "d2pc_sectors_memory_create", "d2pc_sectors_memory_destroy", "d2pc_sectors_memory_last_error", "d2pc_sectors_memory_desc_init",
    "d2pc_sectors_memory_desc_check", "d2pc_sectors_memory_update_device", "d2pc_sectors_memory_reset_device",
    "d2pc_sectors_memory_coverage",
    "d2pc_sectors_steer_config_init", "d2pc_sectors_steer_reach", "d2pc_sectors_steer_goal_cell", "d2pc_sectors_steer_create",
    "d2pc_sectors_steer_destroy", "d2pc_sectors_steer_last_error", "d2pc_sectors_steer_desc_init", "d2pc_sectors_steer_desc_check",
    "d2pc_sectors_steer_device",
    "d2pc_sectors_ground_config_init", "d2pc_sectors_ground_geometry", "d2pc_sectors_ground_spread_of_std", "d2pc_sectors_ground_create",
    "d2pc_sectors_ground_destroy", "d2pc_sectors_ground_last_error", "d2pc_sectors_ground_blocks", "d2pc_sectors_ground_desc_init",
    "d2pc_sectors_ground_desc_check", "d2pc_sectors_ground_process_device",
    "d2pc_sectors_terrain_config_init", "d2pc_sectors_terrain_geometry", "d2pc_sectors_terrain_create", "d2pc_sectors_terrain_destroy",
    "d2pc_sectors_terrain_last_error", "d2pc_sectors_terrain_state", "d2pc_sectors_terrain_reset_device", "d2pc_sectors_terrain_desc_init",
    "d2pc_sectors_terrain_desc_check", "d2pc_sectors_terrain_update_device",
    "d2pc_sectors_slope_config_init", "d2pc_sectors_slope_geometry", "d2pc_sectors_slope_of_degrees", "d2pc_sectors_slope_create",
    "d2pc_sectors_slope_destroy", "d2pc_sectors_slope_last_error", "d2pc_sectors_slope_blocks", "d2pc_sectors_slope_desc_init",
    "d2pc_sectors_slope_desc_check", "d2pc_sectors_slope_process_device",
    "d2pc_sectors_relief_geometry", "d2pc_sectors_relief_create", "d2pc_sectors_relief_destroy", "d2pc_sectors_relief_last_error",
    "d2pc_sectors_relief_state", "d2pc_sectors_relief_reset_device", "d2pc_sectors_relief_desc_init", "d2pc_sectors_relief_desc_check",
    "d2pc_sectors_relief_update_device",
]
EMPTY_AGE, OLDEST_AGE = 0xFFFFFFFF, 0xFFFFFFFE   # the age word of an empty record; where an age saturates
STEER_MAX_REACH_SECTORS, STEER_MAX_REACH_LAYERS, STEER_MAX_CANDIDATES, STEER_MAX_WEIGHT = 32, 16, 32, 4095
STEER_OFF = 0xFFFFFFFF            # a goal_sector / prev_sector that switches its term off
STEER_NO_CANDIDATE = 0xFFFFFFFFFFFFFFFF   # a candidate slot beyond the free cells
STEER_BLOCKED = 0xFFFFFFFF        # the cost of a cell that is not free
GROUND_MAX_CELLS_PER_AXIS, GROUND_MAX_WINDOW, GROUND_MAX_CANDIDATES, GROUND_MAX_WEIGHT, GROUND_MAX_K = 64, 8, 32, 4095, 32767
GROUND_EMPTY_MEAN, GROUND_EMPTY_SPREAD = 0x80000000, 0xFFFFFFFF   # mean_q (as a uint32) and spread_q2 of an empty cell
GROUND_OFF = 0xFFFFFFFF           # a goal_i / goal_j that switches the distance term off
GROUND_NO_CANDIDATE = 0xFFFFFFFFFFFFFFFF  # a candidate slot beyond the sites
TERRAIN_MAX_DEPTH, TERRAIN_HEADER_BYTES, TERRAIN_MAX_CORNER = 16, 16, 536870912
SLOPE_CELL_BYTES, SLOPE_MAX_CELLS, SLOPE_MOMENTS = 76, 2155, 7
SLOPE_NOT_FITTED = 0x7FC00000     # slope_a / slope_b of a cell that is not fitted, as bits


class SectorsConfig(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("device_id", ctypes.c_int32), ("n_sectors", ctypes.c_int32),
        ("n_layers", ctypes.c_int32), ("azimuth0", ctypes.c_double), ("r_min", ctypes.c_float), ("r_max", ctypes.c_float),
        ("u_min", ctypes.c_float), ("u_max", ctypes.c_float), ("axes", ctypes.c_int32 * 3), ("min_count", ctypes.c_int32),
        ("no_obstacle_cm", ctypes.c_uint32), ("layer_kind", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3),
    ]


class SectorsGeometry(ctypes.Structure):
    _fields_ = [
        ("n_cells", ctypes.c_int32), ("table_entries", ctypes.c_int32), ("rmin2", ctypes.c_float), ("rmax2", ctypes.c_float),
        ("inv_h", ctypes.c_float), ("share_points", ctypes.c_int32), ("blocks_per_cu", ctypes.c_int32),
        ("elevation_entries", ctypes.c_int32), ("lds_bytes", ctypes.c_size_t), ("block_bytes", ctypes.c_size_t),
        ("device_bytes", ctypes.c_size_t), ("reserved", ctypes.c_int32 * 4),
    ]


class SectorsDesc(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("point_step", ctypes.c_int32), ("n_clouds", ctypes.c_int32),
        ("reserved", ctypes.c_int32), ("points", ctypes.c_void_p), ("counts", ctypes.c_void_p),
        ("cloud_points", ctypes.c_size_t), ("points_frame_stride_points", ctypes.c_size_t), ("range", ctypes.c_void_p),
        ("count", ctypes.c_void_p), ("nearest", ctypes.c_void_p), ("distance_cm", ctypes.c_void_p),
    ]


class SectorsMemoryConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_age", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


class SectorsMemoryStep(ctypes.Structure):   # 64 bytes, in device memory
    _fields_ = [("R", ctypes.c_float * 9), ("t", ctypes.c_float * 3), ("dt", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class SectorsFov(ctypes.Structure):
    _fields_ = [("yaw", ctypes.c_double), ("pitch", ctypes.c_double), ("h_fov", ctypes.c_double), ("v_fov", ctypes.c_double),
                ("margin", ctypes.c_double)]


class SectorsMemoryDesc(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("point_step", ctypes.c_int32), ("n_clouds", ctypes.c_int32),
        ("reserved", ctypes.c_int32), ("points", ctypes.c_void_p), ("cloud_points", ctypes.c_size_t),
        ("points_frame_stride_points", ctypes.c_size_t), ("count", ctypes.c_void_p), ("nearest", ctypes.c_void_p),
        ("step", ctypes.c_void_p), ("covered", ctypes.c_void_p), ("range", ctypes.c_void_p), ("distance_cm", ctypes.c_void_p),
        ("age", ctypes.c_void_p), ("records", ctypes.c_void_p),
    ]


class SectorsSteerConfig(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("radius", ctypes.c_float), ("max_reach_sectors", ctypes.c_int32),
        ("max_reach_layers", ctypes.c_int32), ("free_cm", ctypes.c_uint32), ("min_clearance_cm", ctypes.c_uint32),
        ("horizon_cm", ctypes.c_uint32), ("w_goal", ctypes.c_uint32), ("w_prev", ctypes.c_uint32), ("w_near", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 2),
    ]


class SectorsSteerStep(ctypes.Structure):   # 32 bytes, in device memory
    _fields_ = [("goal_sector", ctypes.c_uint32), ("goal_layer", ctypes.c_uint32), ("prev_sector", ctypes.c_uint32),
                ("prev_layer", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]


class SectorsSteerCandidate(ctypes.Structure):   # as a little-endian uint64: (cost << 32) | cell
    _fields_ = [("cell", ctypes.c_uint32), ("cost", ctypes.c_uint32)]


class SectorsSteerDesc(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("n_candidates", ctypes.c_int32), ("distance_cm", ctypes.c_void_p),
        ("allowed", ctypes.c_void_p), ("step", ctypes.c_void_p), ("clearance_cm", ctypes.c_void_p), ("cost", ctypes.c_void_p),
        ("candidates", ctypes.c_void_p), ("summary", ctypes.c_void_p),
    ]


class SectorsGroundConfig(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("device_id", ctypes.c_int32), ("n_a", ctypes.c_int32), ("n_b", ctypes.c_int32),
        ("cell_size", ctypes.c_float), ("quantum", ctypes.c_float), ("axes", ctypes.c_int32 * 3), ("min_count", ctypes.c_uint32),
        ("max_spread_q2", ctypes.c_uint32), ("max_step_q", ctypes.c_uint32), ("window", ctypes.c_int32), ("w_dist", ctypes.c_uint32),
        ("w_rough", ctypes.c_uint32), ("rough_cap", ctypes.c_uint32), ("max_points", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3),
    ]


class SectorsGroundGeometry(ctypes.Structure):
    _fields_ = [
        ("n_cells", ctypes.c_int32), ("inv_c", ctypes.c_float), ("inv_q", ctypes.c_float), ("share_points", ctypes.c_int32),
        ("blocks_per_cu", ctypes.c_int32), ("blocks", ctypes.c_int32), ("lds_bytes", ctypes.c_size_t), ("block_bytes", ctypes.c_size_t),
        ("device_bytes", ctypes.c_size_t), ("reserved", ctypes.c_int32 * 4),
    ]


class SectorsGroundStep(ctypes.Structure):   # 80 bytes, in device memory
    _fields_ = [("R", ctypes.c_float * 9), ("t", ctypes.c_float * 3), ("origin", ctypes.c_float * 3), ("goal_i", ctypes.c_uint32),
                ("goal_j", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class SectorsGroundDesc(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("point_step", ctypes.c_int32), ("n_clouds", ctypes.c_int32), ("n_candidates", ctypes.c_int32),
        ("points", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("cloud_points", ctypes.c_size_t),
        ("points_frame_stride_points", ctypes.c_size_t), ("step", ctypes.c_void_p), ("allowed", ctypes.c_void_p),
        ("count", ctypes.c_void_p), ("sum", ctypes.c_void_p), ("sum2", ctypes.c_void_p), ("mean_q", ctypes.c_void_p),
        ("spread_q2", ctypes.c_void_p), ("flat", ctypes.c_void_p), ("site", ctypes.c_void_p), ("candidates", ctypes.c_void_p),
        ("summary", ctypes.c_void_p),
    ]


class SectorsTerrainConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("depth", ctypes.c_int32), ("reserved", ctypes.c_uint32 * 6)]


class SectorsTerrainGeometry(ctypes.Structure):
    _fields_ = [
        ("n_cells", ctypes.c_int32), ("inv_c", ctypes.c_float), ("slot_bytes", ctypes.c_size_t), ("state_bytes", ctypes.c_size_t),
        ("headers_offset", ctypes.c_size_t), ("tables_offset", ctypes.c_size_t), ("reserved", ctypes.c_int32 * 6),
    ]


class SectorsTerrainDesc(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("n_candidates", ctypes.c_int32), ("step", ctypes.c_void_p), ("frame_count", ctypes.c_void_p),
        ("frame_sum", ctypes.c_void_p), ("frame_sum2", ctypes.c_void_p), ("allowed", ctypes.c_void_p), ("count", ctypes.c_void_p),
        ("sum", ctypes.c_void_p), ("sum2", ctypes.c_void_p), ("mean_q", ctypes.c_void_p), ("spread_q2", ctypes.c_void_p),
        ("flat", ctypes.c_void_p), ("site", ctypes.c_void_p), ("candidates", ctypes.c_void_p), ("summary", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
    ]


class SectorsSlopeConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("sub", ctypes.c_int32), ("max_slope", ctypes.c_float), ("reserved", ctypes.c_uint32 * 5)]


class SectorsSlopeGeometry(ctypes.Structure):
    _fields_ = [
        ("n_cells", ctypes.c_int32), ("blocks_per_cu", ctypes.c_int32), ("blocks", ctypes.c_int32), ("sub", ctypes.c_int32),
        ("lds_bytes", ctypes.c_size_t), ("block_bytes", ctypes.c_size_t), ("device_bytes", ctypes.c_size_t),
        ("scale", ctypes.c_double), ("max_tilt2", ctypes.c_double), ("reserved", ctypes.c_int32 * 4),
    ]


class SectorsSlopeDesc(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("point_step", ctypes.c_int32), ("n_clouds", ctypes.c_int32), ("n_candidates", ctypes.c_int32),
        ("points", ctypes.c_void_p), ("counts", ctypes.c_void_p), ("cloud_points", ctypes.c_size_t),
        ("points_frame_stride_points", ctypes.c_size_t), ("step", ctypes.c_void_p), ("allowed", ctypes.c_void_p),
        ("count", ctypes.c_void_p), ("sum", ctypes.c_void_p), ("sum2", ctypes.c_void_p), ("moments", ctypes.c_void_p),
        ("slope_a", ctypes.c_void_p), ("slope_b", ctypes.c_void_p), ("level_q", ctypes.c_void_p), ("resid_q2", ctypes.c_void_p),
        ("flat", ctypes.c_void_p), ("site", ctypes.c_void_p), ("candidates", ctypes.c_void_p), ("summary", ctypes.c_void_p),
    ]


class SectorsReliefGeometry(ctypes.Structure):
    _fields_ = [
        ("n_cells", ctypes.c_int32), ("inv_c", ctypes.c_float), ("slot_bytes", ctypes.c_size_t), ("state_bytes", ctypes.c_size_t),
        ("headers_offset", ctypes.c_size_t), ("tables_offset", ctypes.c_size_t), ("scale", ctypes.c_double), ("max_tilt2", ctypes.c_double),
        ("blocks", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5),
    ]


class SectorsReliefDesc(ctypes.Structure):
    _fields_ = [
        ("struct_size", ctypes.c_uint32), ("n_candidates", ctypes.c_int32), ("step", ctypes.c_void_p), ("frame_count", ctypes.c_void_p),
        ("frame_sum", ctypes.c_void_p), ("frame_sum2", ctypes.c_void_p), ("frame_moments", ctypes.c_void_p), ("allowed", ctypes.c_void_p),
        ("count", ctypes.c_void_p), ("sum", ctypes.c_void_p), ("sum2", ctypes.c_void_p), ("moments", ctypes.c_void_p),
        ("slope_a", ctypes.c_void_p), ("slope_b", ctypes.c_void_p), ("level_q", ctypes.c_void_p), ("resid_q2", ctypes.c_void_p),
        ("flat", ctypes.c_void_p), ("site", ctypes.c_void_p), ("candidates", ctypes.c_void_p), ("summary", ctypes.c_void_p),
        ("status", ctypes.c_void_p),
    ]


_lib = None


def sectors_library_path(variant=None) -> str:
    return os.path.join(_HERE, "libd2pc_sectors.so" if variant is None else "libd2pc_sectors_%s.so" % variant)


def load_sectors_library(variant=None):
    """Load libd2pc_sectors.so (`variant`: libd2pc_sectors_<variant>.so, the A/B builds of tools/sectors_bench.py; not
    cached).  Raises, never falls back, when it is not built."""
    global _lib
    if variant is None and _lib is not None:
        return _lib
    path = sectors_library_path(variant)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    # torch ships its own HIP runtime; import it first so both share ONE (as capi.load_library does)
    try:
        import torch  # noqa: F401
    except Exception:  # torch is plumbing only; the ABI works without it
        pass
    L = ctypes.CDLL(path)
    vp, fp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)
    cfg, desc = ctypes.POINTER(SectorsConfig), ctypes.POINTER(SectorsDesc)
    L.d2pc_sectors_config_init.argtypes = [cfg]
    L.d2pc_sectors_config_init.restype = None
    L.d2pc_sectors_geometry.argtypes = [cfg, ctypes.POINTER(SectorsGeometry)]
    L.d2pc_sectors_table.argtypes = [cfg, fp, fp, ctypes.c_int]
    if variant is None or hasattr(L, "d2pc_sectors_elevation_table"):   # (an A/B variant may be a build from before it)
        L.d2pc_sectors_elevation_table.argtypes = [cfg, fp, fp, ctypes.c_int]
    L.d2pc_sectors_create.argtypes = [cfg, ctypes.POINTER(vp)]
    L.d2pc_sectors_destroy.argtypes = [vp]
    L.d2pc_sectors_last_error.argtypes = [vp]
    L.d2pc_sectors_last_error.restype = ctypes.c_char_p
    L.d2pc_sectors_blocks.argtypes = [vp]
    L.d2pc_sectors_desc_init.argtypes = [desc]
    L.d2pc_sectors_desc_init.restype = None
    L.d2pc_sectors_desc_check.argtypes = [cfg, desc]
    L.d2pc_sectors_process_device.argtypes = [vp, desc, vp]
    if variant is None or hasattr(L, "d2pc_sectors_memory_create"):   # (an A/B variant may be a build from before the memory)
        mcfg, mdesc = ctypes.POINTER(SectorsMemoryConfig), ctypes.POINTER(SectorsMemoryDesc)
        L.d2pc_sectors_memory_create.argtypes = [cfg, mcfg, ctypes.POINTER(vp)]
        L.d2pc_sectors_memory_destroy.argtypes = [vp]
        L.d2pc_sectors_memory_last_error.argtypes = [vp]
        L.d2pc_sectors_memory_last_error.restype = ctypes.c_char_p
        L.d2pc_sectors_memory_desc_init.argtypes = [mdesc]
        L.d2pc_sectors_memory_desc_init.restype = None
        L.d2pc_sectors_memory_desc_check.argtypes = [cfg, mcfg, mdesc]
        L.d2pc_sectors_memory_update_device.argtypes = [vp, mdesc, vp]
        L.d2pc_sectors_memory_reset_device.argtypes = [vp, vp]
        L.d2pc_sectors_memory_coverage.argtypes = [cfg, ctypes.POINTER(SectorsFov), ctypes.c_int, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int]
    if variant is None or hasattr(L, "d2pc_sectors_steer_create"):   # (an A/B variant may be a build from before the steer)
        scfg, sdesc, u16 = ctypes.POINTER(SectorsSteerConfig), ctypes.POINTER(SectorsSteerDesc), ctypes.POINTER(ctypes.c_uint16)
        u32 = ctypes.POINTER(ctypes.c_uint32)
        L.d2pc_sectors_steer_config_init.argtypes = [scfg]
        L.d2pc_sectors_steer_config_init.restype = None
        L.d2pc_sectors_steer_reach.argtypes = [cfg, scfg, u16, ctypes.c_int, u16, ctypes.c_int]
        L.d2pc_sectors_steer_goal_cell.argtypes = [cfg, ctypes.c_double, ctypes.c_double, u32, u32]
        L.d2pc_sectors_steer_create.argtypes = [cfg, scfg, ctypes.POINTER(vp)]
        L.d2pc_sectors_steer_destroy.argtypes = [vp]
        L.d2pc_sectors_steer_last_error.argtypes = [vp]
        L.d2pc_sectors_steer_last_error.restype = ctypes.c_char_p
        L.d2pc_sectors_steer_desc_init.argtypes = [sdesc]
        L.d2pc_sectors_steer_desc_init.restype = None
        L.d2pc_sectors_steer_desc_check.argtypes = [cfg, scfg, sdesc]
        L.d2pc_sectors_steer_device.argtypes = [vp, sdesc, vp]
    if variant is None or hasattr(L, "d2pc_sectors_ground_create"):   # (an A/B variant may be a build from before the ground)
        gcfg, gdesc = ctypes.POINTER(SectorsGroundConfig), ctypes.POINTER(SectorsGroundDesc)
        L.d2pc_sectors_ground_config_init.argtypes = [gcfg]
        L.d2pc_sectors_ground_config_init.restype = None
        L.d2pc_sectors_ground_geometry.argtypes = [gcfg, ctypes.POINTER(SectorsGroundGeometry)]
        L.d2pc_sectors_ground_spread_of_std.argtypes = [ctypes.c_double, ctypes.c_double]
        L.d2pc_sectors_ground_spread_of_std.restype = ctypes.c_uint32
        L.d2pc_sectors_ground_create.argtypes = [gcfg, ctypes.POINTER(vp)]
        L.d2pc_sectors_ground_destroy.argtypes = [vp]
        L.d2pc_sectors_ground_last_error.argtypes = [vp]
        L.d2pc_sectors_ground_last_error.restype = ctypes.c_char_p
        L.d2pc_sectors_ground_blocks.argtypes = [vp]
        L.d2pc_sectors_ground_desc_init.argtypes = [gdesc]
        L.d2pc_sectors_ground_desc_init.restype = None
        L.d2pc_sectors_ground_desc_check.argtypes = [gcfg, gdesc]
        L.d2pc_sectors_ground_process_device.argtypes = [vp, gdesc, vp]
    if variant is None or hasattr(L, "d2pc_sectors_terrain_create"):   # (an A/B variant may be a build from before the terrain)
        gcfg, tcfg, tdesc = ctypes.POINTER(SectorsGroundConfig), ctypes.POINTER(SectorsTerrainConfig), ctypes.POINTER(SectorsTerrainDesc)
        L.d2pc_sectors_terrain_config_init.argtypes = [tcfg]
        L.d2pc_sectors_terrain_config_init.restype = None
        L.d2pc_sectors_terrain_geometry.argtypes = [gcfg, tcfg, ctypes.POINTER(SectorsTerrainGeometry)]
        L.d2pc_sectors_terrain_create.argtypes = [gcfg, tcfg, ctypes.POINTER(vp)]
        L.d2pc_sectors_terrain_destroy.argtypes = [vp]
        L.d2pc_sectors_terrain_last_error.argtypes = [vp]
        L.d2pc_sectors_terrain_last_error.restype = ctypes.c_char_p
        L.d2pc_sectors_terrain_state.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
        L.d2pc_sectors_terrain_reset_device.argtypes = [vp, vp]
        L.d2pc_sectors_terrain_desc_init.argtypes = [tdesc]
        L.d2pc_sectors_terrain_desc_init.restype = None
        L.d2pc_sectors_terrain_desc_check.argtypes = [gcfg, tcfg, tdesc]
        L.d2pc_sectors_terrain_update_device.argtypes = [vp, tdesc, vp]
    if variant is None or hasattr(L, "d2pc_sectors_slope_create"):   # (an A/B variant may be a build from before the slope)
        gcfg, scfg, sdesc = ctypes.POINTER(SectorsGroundConfig), ctypes.POINTER(SectorsSlopeConfig), ctypes.POINTER(SectorsSlopeDesc)
        L.d2pc_sectors_slope_config_init.argtypes = [scfg]
        L.d2pc_sectors_slope_config_init.restype = None
        L.d2pc_sectors_slope_geometry.argtypes = [gcfg, scfg, ctypes.POINTER(SectorsSlopeGeometry)]
        L.d2pc_sectors_slope_of_degrees.argtypes = [ctypes.c_double]
        L.d2pc_sectors_slope_of_degrees.restype = ctypes.c_float
        L.d2pc_sectors_slope_create.argtypes = [gcfg, scfg, ctypes.POINTER(vp)]
        L.d2pc_sectors_slope_destroy.argtypes = [vp]
        L.d2pc_sectors_slope_last_error.argtypes = [vp]
        L.d2pc_sectors_slope_last_error.restype = ctypes.c_char_p
        L.d2pc_sectors_slope_blocks.argtypes = [vp]
        L.d2pc_sectors_slope_desc_init.argtypes = [sdesc]
        L.d2pc_sectors_slope_desc_init.restype = None
        L.d2pc_sectors_slope_desc_check.argtypes = [gcfg, scfg, sdesc]
        L.d2pc_sectors_slope_process_device.argtypes = [vp, sdesc, vp]
    if variant is None or hasattr(L, "d2pc_sectors_relief_create"):   # (an A/B variant may be a build from before the relief)
        gcfg, scfg, tcfg = ctypes.POINTER(SectorsGroundConfig), ctypes.POINTER(SectorsSlopeConfig), ctypes.POINTER(SectorsTerrainConfig)
        rdesc = ctypes.POINTER(SectorsReliefDesc)
        L.d2pc_sectors_relief_geometry.argtypes = [gcfg, scfg, tcfg, ctypes.POINTER(SectorsReliefGeometry)]
        L.d2pc_sectors_relief_create.argtypes = [gcfg, scfg, tcfg, ctypes.POINTER(vp)]
        L.d2pc_sectors_relief_destroy.argtypes = [vp]
        L.d2pc_sectors_relief_last_error.argtypes = [vp]
        L.d2pc_sectors_relief_last_error.restype = ctypes.c_char_p
        L.d2pc_sectors_relief_state.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
        L.d2pc_sectors_relief_reset_device.argtypes = [vp, vp]
        L.d2pc_sectors_relief_desc_init.argtypes = [rdesc]
        L.d2pc_sectors_relief_desc_init.restype = None
        L.d2pc_sectors_relief_desc_check.argtypes = [gcfg, scfg, tcfg, rdesc]
        L.d2pc_sectors_relief_update_device.argtypes = [vp, rdesc, vp]
    if variant is None:
        _lib = L
    return L


def _set(struct, kw):
    fields = dict(struct._fields_)
    for k, v in kw.items():
        if k not in fields:
            raise TypeError("%s has no field %r" % (type(struct).__name__, k))
        setattr(struct, k, tuple(v) if k == "axes" else v)
    return struct


def sectors_config_init(**kw) -> SectorsConfig:
    """d2pc_sectors_config_init, then the given fields."""
    c = SectorsConfig()
    load_sectors_library().d2pc_sectors_config_init(ctypes.byref(c))
    return _set(c, kw)


def sectors_desc_init(**kw) -> SectorsDesc:
    """d2pc_sectors_desc_init, then the given fields."""
    d = SectorsDesc()
    load_sectors_library().d2pc_sectors_desc_init(ctypes.byref(d))
    return _set(d, kw)


def sectors_geometry(cfg: SectorsConfig) -> SectorsGeometry:
    """d2pc_sectors_geometry (host arithmetic); raises D2pcError as the C function refuses."""
    g = SectorsGeometry()
    st = load_sectors_library().d2pc_sectors_geometry(ctypes.byref(cfg), ctypes.byref(g))
    if st != 0:
        raise D2pcError(st, "sectors_geometry(%d x %d)" % (cfg.n_sectors, cfg.n_layers))
    return g


def sectors_table(cfg: SectorsConfig):
    """d2pc_sectors_table: the boundary directions (c, s), two float32 arrays of n_sectors / 2."""
    c = np.zeros(MAX_SECTORS // 2, dtype=np.float32)
    s = np.zeros(MAX_SECTORS // 2, dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    n = load_sectors_library().d2pc_sectors_table(ctypes.byref(cfg), c.ctypes.data_as(fp), s.ctypes.data_as(fp), len(c))
    if n <= 0:
        raise D2pcError(-n, "sectors_table(%d)" % cfg.n_sectors)
    return c[:n].copy(), s[:n].copy()


def sectors_elevation_table(cfg: SectorsConfig):
    """d2pc_sectors_elevation_table: (ce, se) of the n_layers + 1 boundary elevations of an elevation-mode configuration."""
    c = np.zeros(MAX_ELEVATION_LAYERS + 1, dtype=np.float32)
    s = np.zeros(MAX_ELEVATION_LAYERS + 1, dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    n = load_sectors_library().d2pc_sectors_elevation_table(ctypes.byref(cfg), c.ctypes.data_as(fp), s.ctypes.data_as(fp), len(c))
    if n <= 0:
        raise D2pcError(-n, "sectors_elevation_table(%d layers, kind %d)" % (cfg.n_layers, cfg.layer_kind))
    return c[:n].copy(), s[:n].copy()


def sectors_desc_check(cfg: SectorsConfig, desc: SectorsDesc) -> int:
    """d2pc_sectors_desc_check: the status d2pc_sectors_process_device would refuse `desc` with (0: accepted)."""
    return load_sectors_library().d2pc_sectors_desc_check(ctypes.byref(cfg), ctypes.byref(desc))


def _ptr(x):
    """A raw device pointer of a torch tensor, an int, or None."""
    return x.data_ptr() if hasattr(x, "data_ptr") else x


class _Session:
    """What the sessions share: a handle of `libd2pc_sectors[_<variant>].so`, made by `<_PREFIX>_create` and given back to
    `<_PREFIX>_destroy` once."""

    _PREFIX = None

    def _create(self, variant, what, *args):
        self._L, self._h = load_sectors_library(variant), None
        h = ctypes.c_void_p()
        st = getattr(self._L, self._PREFIX + "_create")(*args, ctypes.byref(h))
        if st:
            raise D2pcError(st, what)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._PREFIX + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    def last_error(self) -> str:
        return getattr(self._L, self._PREFIX + "_last_error")(self._h).decode()


class Sectors(_Session):
    """d2pc_sectors_*: one session = one grid geometry (of height or of elevation layers: `layer_kind`) on one device.  `process` takes torch tensors or raw device
    pointers, is asynchronous on `stream` and allocates nothing."""

    _PREFIX = "d2pc_sectors"

    def __init__(self, cfg: SectorsConfig = None, variant=None, **kw):
        self.cfg = _set(cfg, kw) if cfg is not None else sectors_config_init(**kw)
        self._create(variant, "sectors_create(%d x %d)" % (self.cfg.n_sectors, self.cfg.n_layers), ctypes.byref(self.cfg))
        self.geometry = sectors_geometry(self.cfg)
        self.n_cells, self.blocks = self.geometry.n_cells, int(self._L.d2pc_sectors_blocks(self._h))

    def process_desc(self, desc: SectorsDesc, stream_ptr=None):
        """d2pc_sectors_process_device."""
        st = self._L.d2pc_sectors_process_device(self._h, ctypes.byref(desc), stream_ptr)
        if st:
            raise D2pcError(st, self.last_error())

    def process(self, points, cloud_points, point_step=16, n_clouds=1, counts=None, frame_stride_points=0, range=None,
                count=None, nearest=None, distance_cm=None, stream_ptr=None):
        """The descriptor from tensors (their data_ptr) or raw device pointers, then the call."""
        self.process_desc(sectors_desc_init(
            point_step=point_step, n_clouds=n_clouds, points=_ptr(points), counts=_ptr(counts), cloud_points=cloud_points,
            points_frame_stride_points=frame_stride_points, range=_ptr(range), count=_ptr(count), nearest=_ptr(nearest),
            distance_cm=_ptr(distance_cm)), stream_ptr)


def sectors_memory_config(max_age=OLDEST_AGE) -> SectorsMemoryConfig:
    """A d2pc_sectors_memory_config with its struct_size and `max_age` ticks."""
    return SectorsMemoryConfig(struct_size=ctypes.sizeof(SectorsMemoryConfig), max_age=max_age)


def sectors_memory_desc_init(**kw) -> SectorsMemoryDesc:
    """d2pc_sectors_memory_desc_init, then the given fields."""
    d = SectorsMemoryDesc()
    load_sectors_library().d2pc_sectors_memory_desc_init(ctypes.byref(d))
    return _set(d, kw)


def sectors_memory_desc_check(cfg: SectorsConfig, mcfg: SectorsMemoryConfig, desc: SectorsMemoryDesc) -> int:
    """d2pc_sectors_memory_desc_check: the status d2pc_sectors_memory_update_device would refuse `desc` with (0: accepted)."""
    return load_sectors_library().d2pc_sectors_memory_desc_check(ctypes.byref(cfg), ctypes.byref(mcfg), ctypes.byref(desc))


def sectors_memory_step(R, t, dt) -> np.ndarray:
    """The 16 words of a d2pc_sectors_memory_step (R row-major, t, dt, three zeros) as uint32, to copy to the device."""
    w = np.zeros(16, dtype=np.uint32)
    w[:9] = np.asarray(R, dtype=np.float32).reshape(9).view(np.uint32)
    w[9:12] = np.asarray(t, dtype=np.float32).reshape(3).view(np.uint32)
    w[12] = dt
    return w


def sectors_memory_coverage(cfg: SectorsConfig, fovs) -> np.ndarray:
    """d2pc_sectors_memory_coverage: uint8 per cell, 1 where a field of view of `fovs` (SectorsFov, or (yaw, pitch, h_fov,
    v_fov, margin) tuples) holds the cell's centre direction."""
    fovs = [f if isinstance(f, SectorsFov) else SectorsFov(*f) for f in fovs]
    arr = (SectorsFov * max(len(fovs), 1))(*fovs)
    out = np.zeros(MAX_SECTORS * MAX_LAYERS, dtype=np.uint8)
    n = load_sectors_library().d2pc_sectors_memory_coverage(ctypes.byref(cfg), arr, len(fovs),
                                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(out))
    if n <= 0:
        raise D2pcError(-n, "sectors_memory_coverage(%d x %d)" % (cfg.n_sectors, cfg.n_layers))
    return out[:n].copy()


class SectorsMemory(_Session):
    """d2pc_sectors_memory_*: one world-frame point per cell of a grid, kept on the device between calls.  `update` takes
    torch tensors or raw device pointers, is asynchronous on `stream` and allocates nothing."""

    _PREFIX = "d2pc_sectors_memory"

    def __init__(self, cfg: SectorsConfig, max_age=OLDEST_AGE, variant=None):
        self.cfg, self.mcfg = cfg, sectors_memory_config(max_age)
        self._create(variant, "sectors_memory_create(%d x %d, max_age %d)" % (cfg.n_sectors, cfg.n_layers, max_age),
                     ctypes.byref(self.cfg), ctypes.byref(self.mcfg))
        self.n_cells = cfg.n_sectors * cfg.n_layers

    def update_desc(self, desc: SectorsMemoryDesc, stream_ptr=None):
        """d2pc_sectors_memory_update_device."""
        st = self._L.d2pc_sectors_memory_update_device(self._h, ctypes.byref(desc), stream_ptr)
        if st:
            raise D2pcError(st, self.last_error())

    def update(self, points, cloud_points, count, nearest, step, point_step=16, n_clouds=1, frame_stride_points=0, covered=None,
               range=None, distance_cm=None, age=None, records=None, stream_ptr=None):
        """The descriptor from tensors (their data_ptr) or raw device pointers, then the call."""
        self.update_desc(sectors_memory_desc_init(
            point_step=point_step, n_clouds=n_clouds, points=_ptr(points), cloud_points=cloud_points,
            points_frame_stride_points=frame_stride_points, count=_ptr(count), nearest=_ptr(nearest), step=_ptr(step),
            covered=_ptr(covered), range=_ptr(range), distance_cm=_ptr(distance_cm), age=_ptr(age), records=_ptr(records)),
            stream_ptr)

    def reset(self, stream_ptr=None):
        """d2pc_sectors_memory_reset_device."""
        st = self._L.d2pc_sectors_memory_reset_device(self._h, stream_ptr)
        if st:
            raise D2pcError(st, self.last_error())


def sectors_steer_config_init(**kw) -> SectorsSteerConfig:
    """d2pc_sectors_steer_config_init, then the given fields."""
    c = SectorsSteerConfig()
    load_sectors_library().d2pc_sectors_steer_config_init(ctypes.byref(c))
    return _set(c, kw)


def sectors_steer_desc_init(**kw) -> SectorsSteerDesc:
    """d2pc_sectors_steer_desc_init, then the given fields."""
    d = SectorsSteerDesc()
    load_sectors_library().d2pc_sectors_steer_desc_init(ctypes.byref(d))
    return _set(d, kw)


def sectors_steer_desc_check(cfg: SectorsConfig, scfg: SectorsSteerConfig, desc: SectorsSteerDesc) -> int:
    """d2pc_sectors_steer_desc_check: the status d2pc_sectors_steer_device would refuse `desc` with (0: accepted)."""
    return load_sectors_library().d2pc_sectors_steer_desc_check(ctypes.byref(cfg), ctypes.byref(scfg), ctypes.byref(desc))


def sectors_steer_reach(cfg: SectorsConfig, scfg: SectorsSteerConfig):
    """d2pc_sectors_steer_reach: (reach_s uint16 (n_layers, Wa + 1), reach_l uint16 (We + 1))."""
    rs = np.zeros(MAX_ELEVATION_LAYERS * (STEER_MAX_REACH_SECTORS + 1), dtype=np.uint16)
    rl = np.zeros(STEER_MAX_REACH_LAYERS + 1, dtype=np.uint16)
    u16 = ctypes.POINTER(ctypes.c_uint16)
    n = load_sectors_library().d2pc_sectors_steer_reach(ctypes.byref(cfg), ctypes.byref(scfg), rs.ctypes.data_as(u16), len(rs),
                                                        rl.ctypes.data_as(u16), len(rl))
    if n <= 0:
        raise D2pcError(-n, "sectors_steer_reach(%d x %d, reach %d / %d)" % (cfg.n_sectors, cfg.n_layers, scfg.max_reach_sectors,
                                                                           scfg.max_reach_layers))
    return rs[:n].reshape(cfg.n_layers, scfg.max_reach_sectors + 1).copy(), rl[:scfg.max_reach_layers + 1].copy()


def sectors_steer_goal_cell(cfg: SectorsConfig, yaw, pitch_or_layer=0.0):
    """d2pc_sectors_steer_goal_cell: (sector, layer) of a direction; raises D2pcError as the C function refuses."""
    s, l = ctypes.c_uint32(), ctypes.c_uint32()
    st = load_sectors_library().d2pc_sectors_steer_goal_cell(ctypes.byref(cfg), yaw, pitch_or_layer, ctypes.byref(s), ctypes.byref(l))
    if st:
        raise D2pcError(st, "sectors_steer_goal_cell(%r, %r)" % (yaw, pitch_or_layer))
    return s.value, l.value


def sectors_steer_step(goal_sector=STEER_OFF, goal_layer=0, prev_sector=STEER_OFF, prev_layer=0) -> np.ndarray:
    """The 8 words of a d2pc_sectors_steer_step as uint32, to copy to the device."""
    return np.array([goal_sector, goal_layer, prev_sector, prev_layer, 0, 0, 0, 0], dtype=np.uint64).astype(np.uint32)


class SectorsSteer(_Session):
    """d2pc_sectors_steer_*: clearance, cost and the best free cells of a grid's distance_cm, in one launch.  `steer` takes
    torch tensors or raw device pointers, is asynchronous on `stream` and allocates nothing."""

    _PREFIX = "d2pc_sectors_steer"

    def __init__(self, cfg: SectorsConfig, scfg: SectorsSteerConfig = None, variant=None, **kw):
        self.cfg = cfg
        self.scfg = _set(scfg, kw) if scfg is not None else sectors_steer_config_init(**kw)
        self._create(variant, "sectors_steer_create(%d x %d, reach %d / %d)" % (
            cfg.n_sectors, cfg.n_layers, self.scfg.max_reach_sectors, self.scfg.max_reach_layers), ctypes.byref(self.cfg), ctypes.byref(self.scfg))
        self.n_cells = cfg.n_sectors * cfg.n_layers

    def steer_desc(self, desc: SectorsSteerDesc, stream_ptr=None):
        """d2pc_sectors_steer_device."""
        st = self._L.d2pc_sectors_steer_device(self._h, ctypes.byref(desc), stream_ptr)
        if st:
            raise D2pcError(st, self.last_error())

    def steer(self, distance_cm, step, allowed=None, clearance_cm=None, cost=None, candidates=None, n_candidates=1, summary=None,
              stream_ptr=None):
        """The descriptor from tensors (their data_ptr) or raw device pointers, then the call."""
        self.steer_desc(sectors_steer_desc_init(
            n_candidates=n_candidates, distance_cm=_ptr(distance_cm), allowed=_ptr(allowed), step=_ptr(step),
            clearance_cm=_ptr(clearance_cm), cost=_ptr(cost), candidates=_ptr(candidates), summary=_ptr(summary)), stream_ptr)


def sectors_ground_config_init(**kw) -> SectorsGroundConfig:
    """d2pc_sectors_ground_config_init, then the given fields."""
    c = SectorsGroundConfig()
    load_sectors_library().d2pc_sectors_ground_config_init(ctypes.byref(c))
    return _set(c, kw)


def sectors_ground_desc_init(**kw) -> SectorsGroundDesc:
    """d2pc_sectors_ground_desc_init, then the given fields."""
    d = SectorsGroundDesc()
    load_sectors_library().d2pc_sectors_ground_desc_init(ctypes.byref(d))
    return _set(d, kw)


def sectors_ground_geometry(gcfg: SectorsGroundConfig) -> SectorsGroundGeometry:
    """d2pc_sectors_ground_geometry (host arithmetic); raises D2pcError as the C function refuses."""
    g = SectorsGroundGeometry()
    st = load_sectors_library().d2pc_sectors_ground_geometry(ctypes.byref(gcfg), ctypes.byref(g))
    if st != 0:
        raise D2pcError(st, "sectors_ground_geometry(%d x %d)" % (gcfg.n_a, gcfg.n_b))
    return g


def sectors_ground_spread_of_std(quantum, std_dev) -> int:
    """d2pc_sectors_ground_spread_of_std: max_spread_q2 from a standard deviation in the cloud's unit."""
    return int(load_sectors_library().d2pc_sectors_ground_spread_of_std(quantum, std_dev))


def sectors_ground_desc_check(gcfg: SectorsGroundConfig, desc: SectorsGroundDesc) -> int:
    """d2pc_sectors_ground_desc_check: the status d2pc_sectors_ground_process_device would refuse `desc` with (0: accepted)."""
    return load_sectors_library().d2pc_sectors_ground_desc_check(ctypes.byref(gcfg), ctypes.byref(desc))


def sectors_ground_step(R, t, origin, goal_i=GROUND_OFF, goal_j=GROUND_OFF) -> np.ndarray:
    """The 20 words of a d2pc_sectors_ground_step (R row-major, t, origin, the goal cell, three zeros) as uint32, to copy to
    the device."""
    w = np.zeros(20, dtype=np.uint32)
    w[:9] = np.asarray(R, dtype=np.float32).reshape(9).view(np.uint32)
    w[9:12] = np.asarray(t, dtype=np.float32).reshape(3).view(np.uint32)
    w[12:15] = np.asarray(origin, dtype=np.float32).reshape(3).view(np.uint32)
    w[15:17] = np.array([goal_i, goal_j], dtype=np.uint64).astype(np.uint32)
    return w


class SectorsGround(_Session):
    """d2pc_sectors_ground_*: per-cell ground height statistics in a levelled world frame and ranked landing sites, from any
    cloud and a pose.  `process` takes torch tensors or raw device pointers, is asynchronous on `stream` and allocates nothing."""

    _PREFIX = "d2pc_sectors_ground"

    def __init__(self, gcfg: SectorsGroundConfig = None, variant=None, **kw):
        self.cfg = _set(gcfg, kw) if gcfg is not None else sectors_ground_config_init(**kw)
        self._create(variant, "sectors_ground_create(%d x %d)" % (self.cfg.n_a, self.cfg.n_b), ctypes.byref(self.cfg))
        self.geometry = sectors_ground_geometry(self.cfg)
        self.n_cells, self.blocks = self.geometry.n_cells, int(self._L.d2pc_sectors_ground_blocks(self._h))

    def process_desc(self, desc: SectorsGroundDesc, stream_ptr=None):
        """d2pc_sectors_ground_process_device."""
        st = self._L.d2pc_sectors_ground_process_device(self._h, ctypes.byref(desc), stream_ptr)
        if st:
            raise D2pcError(st, self.last_error())

    def process(self, points, cloud_points, step, point_step=16, n_clouds=1, counts=None, frame_stride_points=0, allowed=None,
                count=None, sum=None, sum2=None, mean_q=None, spread_q2=None, flat=None, site=None, candidates=None,
                n_candidates=1, summary=None, stream_ptr=None):
        """The descriptor from tensors (their data_ptr) or raw device pointers, then the call."""
        self.process_desc(sectors_ground_desc_init(
            point_step=point_step, n_clouds=n_clouds, n_candidates=n_candidates, points=_ptr(points), counts=_ptr(counts),
            cloud_points=cloud_points, points_frame_stride_points=frame_stride_points, step=_ptr(step), allowed=_ptr(allowed),
            count=_ptr(count), sum=_ptr(sum), sum2=_ptr(sum2), mean_q=_ptr(mean_q), spread_q2=_ptr(spread_q2), flat=_ptr(flat),
            site=_ptr(site), candidates=_ptr(candidates), summary=_ptr(summary)), stream_ptr)


def sectors_terrain_config_init(**kw) -> SectorsTerrainConfig:
    """d2pc_sectors_terrain_config_init, then the given fields."""
    c = SectorsTerrainConfig()
    load_sectors_library().d2pc_sectors_terrain_config_init(ctypes.byref(c))
    return _set(c, kw)


def sectors_terrain_desc_init(**kw) -> SectorsTerrainDesc:
    """d2pc_sectors_terrain_desc_init, then the given fields."""
    d = SectorsTerrainDesc()
    load_sectors_library().d2pc_sectors_terrain_desc_init(ctypes.byref(d))
    return _set(d, kw)


def sectors_terrain_geometry(gcfg: SectorsGroundConfig, tcfg: SectorsTerrainConfig) -> SectorsTerrainGeometry:
    """d2pc_sectors_terrain_geometry (host arithmetic); raises D2pcError as the C function refuses."""
    g = SectorsTerrainGeometry()
    st = load_sectors_library().d2pc_sectors_terrain_geometry(ctypes.byref(gcfg), ctypes.byref(tcfg), ctypes.byref(g))
    if st != 0:
        raise D2pcError(st, "sectors_terrain_geometry(%d x %d, depth %d)" % (gcfg.n_a, gcfg.n_b, tcfg.depth))
    return g


def sectors_terrain_desc_check(gcfg: SectorsGroundConfig, tcfg: SectorsTerrainConfig, desc: SectorsTerrainDesc) -> int:
    """d2pc_sectors_terrain_desc_check: the status d2pc_sectors_terrain_update_device would refuse `desc` with (0: accepted)."""
    return load_sectors_library().d2pc_sectors_terrain_desc_check(ctypes.byref(gcfg), ctypes.byref(tcfg), ctypes.byref(desc))


class _StateView:
    """A session's state block for torch.as_tensor."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "strides": None, "typestr": "|u1", "data": (ptr, False), "version": 2}


class SectorsTerrain(_Session):
    """d2pc_sectors_terrain_*: the ground's per-cell tables of the last `depth` frames, kept on the device, and the landing grid
    of that scrolling window in one launch.  `update` takes torch tensors or raw device pointers, is asynchronous on `stream`
    and allocates nothing."""

    _PREFIX = "d2pc_sectors_terrain"

    def __init__(self, gcfg: SectorsGroundConfig, tcfg: SectorsTerrainConfig = None, variant=None, **kw):
        self.cfg = gcfg
        self.tcfg = _set(tcfg, kw) if tcfg is not None else sectors_terrain_config_init(**kw)
        self._create(variant, "sectors_terrain_create(%d x %d, depth %d)" % (gcfg.n_a, gcfg.n_b, self.tcfg.depth),
                     ctypes.byref(self.cfg), ctypes.byref(self.tcfg))
        self.geometry = sectors_terrain_geometry(self.cfg, self.tcfg)
        self.n_cells, self.depth = self.geometry.n_cells, self.tcfg.depth

    def state(self):
        """d2pc_sectors_terrain_state: (the state block's device pointer, its bytes)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        st = self._L.d2pc_sectors_terrain_state(self._h, ctypes.byref(p), ctypes.byref(n))
        if st:
            raise D2pcError(st, self.last_error())
        return p.value, n.value

    def state_tensor(self):
        """The state block as a torch uint8 tensor that VIEWS it (the CUDA array interface, no copy): `.clone()` saves a map and
        `.copy_()` restores one, in stream order with the updates.  The view must not outlive the session."""
        import torch

        ptr, n = self.state()
        return torch.as_tensor(_StateView(ptr, n), device="cuda:%d" % self.cfg.device_id)

    def update_desc(self, desc: SectorsTerrainDesc, stream_ptr=None):
        """d2pc_sectors_terrain_update_device."""
        st = self._L.d2pc_sectors_terrain_update_device(self._h, ctypes.byref(desc), stream_ptr)
        if st:
            raise D2pcError(st, self.last_error())

    def update(self, step, frame_count, frame_sum, frame_sum2, allowed=None, count=None, sum=None, sum2=None, mean_q=None,
               spread_q2=None, flat=None, site=None, candidates=None, n_candidates=1, summary=None, status=None, stream_ptr=None):
        """The descriptor from tensors (their data_ptr) or raw device pointers, then the call."""
        self.update_desc(sectors_terrain_desc_init(
            n_candidates=n_candidates, step=_ptr(step), frame_count=_ptr(frame_count), frame_sum=_ptr(frame_sum),
            frame_sum2=_ptr(frame_sum2), allowed=_ptr(allowed), count=_ptr(count), sum=_ptr(sum), sum2=_ptr(sum2), mean_q=_ptr(mean_q),
            spread_q2=_ptr(spread_q2), flat=_ptr(flat), site=_ptr(site), candidates=_ptr(candidates), summary=_ptr(summary),
            status=_ptr(status)), stream_ptr)

    def reset(self, stream_ptr=None):
        """d2pc_sectors_terrain_reset_device."""
        st = self._L.d2pc_sectors_terrain_reset_device(self._h, stream_ptr)
        if st:
            raise D2pcError(st, self.last_error())


def sectors_slope_config_init(**kw) -> SectorsSlopeConfig:
    """d2pc_sectors_slope_config_init, then the given fields."""
    c = SectorsSlopeConfig()
    load_sectors_library().d2pc_sectors_slope_config_init(ctypes.byref(c))
    return _set(c, kw)


def sectors_slope_desc_init(**kw) -> SectorsSlopeDesc:
    """d2pc_sectors_slope_desc_init, then the given fields."""
    d = SectorsSlopeDesc()
    load_sectors_library().d2pc_sectors_slope_desc_init(ctypes.byref(d))
    return _set(d, kw)


def sectors_slope_geometry(gcfg: SectorsGroundConfig, scfg: SectorsSlopeConfig) -> SectorsSlopeGeometry:
    """d2pc_sectors_slope_geometry (host arithmetic); raises D2pcError as the C function refuses."""
    g = SectorsSlopeGeometry()
    st = load_sectors_library().d2pc_sectors_slope_geometry(ctypes.byref(gcfg), ctypes.byref(scfg), ctypes.byref(g))
    if st != 0:
        raise D2pcError(st, "sectors_slope_geometry(%d x %d, sub %d)" % (gcfg.n_a, gcfg.n_b, scfg.sub))
    return g


def sectors_slope_of_degrees(degrees) -> float:
    """d2pc_sectors_slope_of_degrees: max_slope (rise over run, a float32) from an angle."""
    return float(load_sectors_library().d2pc_sectors_slope_of_degrees(degrees))


def sectors_slope_desc_check(gcfg: SectorsGroundConfig, scfg: SectorsSlopeConfig, desc: SectorsSlopeDesc) -> int:
    """d2pc_sectors_slope_desc_check: the status d2pc_sectors_slope_process_device would refuse `desc` with (0: accepted)."""
    return load_sectors_library().d2pc_sectors_slope_desc_check(ctypes.byref(gcfg), ctypes.byref(scfg), ctypes.byref(desc))


class SectorsSlope(_Session):
    """d2pc_sectors_slope_*: a plane fit per cell of the landing grid -- slope along a and b, the level at the cell's centre,
    the roughness about the plane -- and ranked landing sites, from any cloud and a pose (a sectors_ground_step).  `process`
    takes torch tensors or raw device pointers, is asynchronous on `stream` and allocates nothing."""

    _PREFIX = "d2pc_sectors_slope"

    def __init__(self, gcfg: SectorsGroundConfig, scfg: SectorsSlopeConfig = None, variant=None, **kw):
        self.cfg = gcfg
        self.scfg = _set(scfg, kw) if scfg is not None else sectors_slope_config_init(**kw)
        self._create(variant, "sectors_slope_create(%d x %d, sub %d)" % (gcfg.n_a, gcfg.n_b, self.scfg.sub),
                     ctypes.byref(self.cfg), ctypes.byref(self.scfg))
        self.geometry = sectors_slope_geometry(self.cfg, self.scfg)
        self.n_cells, self.blocks = self.geometry.n_cells, int(self._L.d2pc_sectors_slope_blocks(self._h))

    def process_desc(self, desc: SectorsSlopeDesc, stream_ptr=None):
        """d2pc_sectors_slope_process_device."""
        st = self._L.d2pc_sectors_slope_process_device(self._h, ctypes.byref(desc), stream_ptr)
        if st:
            raise D2pcError(st, self.last_error())

    def process(self, points, cloud_points, step, point_step=16, n_clouds=1, counts=None, frame_stride_points=0, allowed=None,
                count=None, sum=None, sum2=None, moments=None, slope_a=None, slope_b=None, level_q=None, resid_q2=None, flat=None,
                site=None, candidates=None, n_candidates=1, summary=None, stream_ptr=None):
        """The descriptor from tensors (their data_ptr) or raw device pointers, then the call."""
        self.process_desc(sectors_slope_desc_init(
            point_step=point_step, n_clouds=n_clouds, n_candidates=n_candidates, points=_ptr(points), counts=_ptr(counts),
            cloud_points=cloud_points, points_frame_stride_points=frame_stride_points, step=_ptr(step), allowed=_ptr(allowed),
            count=_ptr(count), sum=_ptr(sum), sum2=_ptr(sum2), moments=_ptr(moments), slope_a=_ptr(slope_a), slope_b=_ptr(slope_b),
            level_q=_ptr(level_q), resid_q2=_ptr(resid_q2), flat=_ptr(flat), site=_ptr(site), candidates=_ptr(candidates),
            summary=_ptr(summary)), stream_ptr)


def sectors_relief_desc_init(**kw) -> SectorsReliefDesc:
    """d2pc_sectors_relief_desc_init, then the given fields."""
    d = SectorsReliefDesc()
    load_sectors_library().d2pc_sectors_relief_desc_init(ctypes.byref(d))
    return _set(d, kw)


def sectors_relief_geometry(gcfg: SectorsGroundConfig, scfg: SectorsSlopeConfig, tcfg: SectorsTerrainConfig) -> SectorsReliefGeometry:
    """d2pc_sectors_relief_geometry (host arithmetic); raises D2pcError as the C function refuses."""
    g = SectorsReliefGeometry()
    st = load_sectors_library().d2pc_sectors_relief_geometry(ctypes.byref(gcfg), ctypes.byref(scfg), ctypes.byref(tcfg), ctypes.byref(g))
    if st != 0:
        raise D2pcError(st, "sectors_relief_geometry(%d x %d, sub %d, depth %d)" % (gcfg.n_a, gcfg.n_b, scfg.sub, tcfg.depth))
    return g


def sectors_relief_desc_check(gcfg: SectorsGroundConfig, scfg: SectorsSlopeConfig, tcfg: SectorsTerrainConfig, desc: SectorsReliefDesc) -> int:
    """d2pc_sectors_relief_desc_check: the status d2pc_sectors_relief_update_device would refuse `desc` with (0: accepted)."""
    return load_sectors_library().d2pc_sectors_relief_desc_check(ctypes.byref(gcfg), ctypes.byref(scfg), ctypes.byref(tcfg), ctypes.byref(desc))


class SectorsRelief(_Session):
    """d2pc_sectors_relief_*: the slope's per-cell tables (count and nine sums) of the last `depth` frames, kept on the device,
    and the plane fit, the landing grid and the ranked sites of that scrolling window in two launches.  `update` takes torch
    tensors or raw device pointers, is asynchronous on `stream` and allocates nothing."""

    _PREFIX = "d2pc_sectors_relief"

    def __init__(self, gcfg: SectorsGroundConfig, scfg: SectorsSlopeConfig = None, tcfg: SectorsTerrainConfig = None, variant=None, **kw):
        self.cfg = gcfg
        self.scfg = scfg if scfg is not None else sectors_slope_config_init()
        self.tcfg = _set(tcfg, kw) if tcfg is not None else sectors_terrain_config_init(**kw)
        self._create(variant, "sectors_relief_create(%d x %d, sub %d, depth %d)" % (gcfg.n_a, gcfg.n_b, self.scfg.sub, self.tcfg.depth),
                     ctypes.byref(self.cfg), ctypes.byref(self.scfg), ctypes.byref(self.tcfg))
        self.geometry = sectors_relief_geometry(self.cfg, self.scfg, self.tcfg)
        self.n_cells, self.depth, self.blocks = self.geometry.n_cells, self.tcfg.depth, self.geometry.blocks

    def state(self):
        """d2pc_sectors_relief_state: (the state block's device pointer, its bytes)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        st = self._L.d2pc_sectors_relief_state(self._h, ctypes.byref(p), ctypes.byref(n))
        if st:
            raise D2pcError(st, self.last_error())
        return p.value, n.value

    def state_tensor(self):
        """The state block as a torch uint8 tensor that VIEWS it (the CUDA array interface, no copy): `.clone()` saves a map and
        `.copy_()` restores one, in stream order with the updates.  The view must not outlive the session."""
        import torch

        ptr, n = self.state()
        return torch.as_tensor(_StateView(ptr, n), device="cuda:%d" % self.cfg.device_id)

    def update_desc(self, desc: SectorsReliefDesc, stream_ptr=None):
        """d2pc_sectors_relief_update_device."""
        st = self._L.d2pc_sectors_relief_update_device(self._h, ctypes.byref(desc), stream_ptr)
        if st:
            raise D2pcError(st, self.last_error())

    def update(self, step, frame_count, frame_sum, frame_sum2, frame_moments, allowed=None, count=None, sum=None, sum2=None, moments=None,
               slope_a=None, slope_b=None, level_q=None, resid_q2=None, flat=None, site=None, candidates=None, n_candidates=1,
               summary=None, status=None, stream_ptr=None):
        """The descriptor from tensors (their data_ptr) or raw device pointers, then the call."""
        self.update_desc(sectors_relief_desc_init(
            n_candidates=n_candidates, step=_ptr(step), frame_count=_ptr(frame_count), frame_sum=_ptr(frame_sum),
            frame_sum2=_ptr(frame_sum2), frame_moments=_ptr(frame_moments), allowed=_ptr(allowed), count=_ptr(count), sum=_ptr(sum),
            sum2=_ptr(sum2), moments=_ptr(moments), slope_a=_ptr(slope_a), slope_b=_ptr(slope_b), level_q=_ptr(level_q),
            resid_q2=_ptr(resid_q2), flat=_ptr(flat), site=_ptr(site), candidates=_ptr(candidates), summary=_ptr(summary),
            status=_ptr(status)), stream_ptr)

    def reset(self, stream_ptr=None):
        """d2pc_sectors_relief_reset_device."""
        st = self._L.d2pc_sectors_relief_reset_device(self._h, stream_ptr)
        if st:
            raise D2pcError(st, self.last_error())
