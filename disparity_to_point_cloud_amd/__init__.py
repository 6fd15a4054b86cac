"""disparity_to_point_cloud_amd -- MI355X-native disparity -> point-cloud path.

The product is the C-ABI shared library `libd2pc.so` (include/d2pc.h) built
from the hand-written gfx950 kernels under csrc/.  This package is only the
Python plumbing used by the tests, bench.py and the multi-GPU harness:
a ctypes binding of that ABI plus torch.distributed helpers.  It contains no
compute path of its own and no CPU fallback: if the library is missing or no
GPU is usable, calls raise.
"""
from .capi import (  # noqa: F401
    D2pcError,
    PinnedBuffer,
    Context,
    DTYPE_F32,
    DTYPE_U8,
    DTYPE_U16,
    DTYPE_MONO16,
    MODE_PARITY,
    MODE_COMPACT,
    FORM_DEFAULT,
    FORM_CV24,
    FORM_CV4,
    CALIB_BLOB_BYTES,
    abi_version,
    calib_pack,
    calib_unpack,
    device_count,
    library_path,
    load_library,
    make_q,
    make_q_disparity_image,
    make_q_flavour,
    STEREORECTIFY_CONTINUOUS,
    STEREORECTIFY_CV24,
    STEREORECTIFY_CV3,
    roi_points,
    status_string,
    FuseDesc,
    fuse_desc_init,
    crop_to_square,
    FUSE_WEIGHTED_AVERAGE,
    FUSE_MAX_DIST,
    FUSE_MAX_DIST_UNLESS_BLACK,
    FUSE_BETTER_SCORE,
    FUSE_ONLY_GOOD_1,
    FUSE_ONLY_GOOD_AVG,
    FUSE_OVERLAP,
    FUSE_BLACK_TO_WHITE,
    FUSE_GRAD_FILTER,
    ScoreFilterDesc,
    score_filter_desc_init,
    SCORE_FORM_CV4,
    SCORE_FORM_CV3,
    ColorizeDesc,
    colorize_desc_init,
    colorize_table,
    FusionNodeConfig,
    FusionNodeGeometry,
    FusionNodeTopics,
    FusionNodeHostTopics,
    FusionSession,
    fusion_node_config_init,
    fusion_node_geometry,
    NODE_DISPARITY_1,
    NODE_DISPARITY_2,
    NODE_MATCHING_SCORE_1,
    NODE_MATCHING_SCORE_2,
    NODE_TOPICS,
    RIG_MAX_CAMERAS,
    RigConfig,
    RigGeometry,
    RigSession,
    rig_compose_q,
    rig_config_init,
    rig_geometry,
    POINT_XYZI,
    POINT_XYZRGB,
    TEX_U8,
    TEX_U16,
    TEX_F32,
    TEX_RGB8,
    TEX_BGR8,
    TEX_MONO8,
    TextureDesc,
    TexturedCloudMeta,
    texture_desc_init,
    textured_cloud_meta,
)
from .sectors import (  # noqa: F401  (include/d2pc_sectors.h: the companion library libd2pc_sectors.so)
    Sectors,
    SectorsConfig,
    SectorsDesc,
    SectorsGeometry,
    load_sectors_library,
    sectors_config_init,
    sectors_desc_check,
    sectors_desc_init,
    sectors_geometry,
    sectors_library_path,
    sectors_table,
)


def __getattr__(name):
    # the fusion-node session needs torch; the binding above does not, so torch is imported on first use only
    if name == "FusionNode":
        from .fusion_node import FusionNode
        return FusionNode
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
