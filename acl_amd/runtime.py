"""ctypes binding of the C ABI in include/aclhip.h (acl_amd/lib/libaclhip.so).

Mirrors the reference's decompression surface (acl::decompression_context::initialize / seek /
decompress_tracks / decompress_track, /root/reference/includes/acl/decompression/decompress.h:76-201)
for batches of clip instances. torch is used only for device memory and streams.

The HIP library is the only implementation: if it cannot be loaded this module raises, it never falls back to a CPU path.
"""
import ctypes
import functools
import os

import numpy as np

# ACLHIP_LIBRARY: another build of the same library (A/B measurements of kernel variants, see tools/)
_LIB_PATH = os.environ.get("ACLHIP_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libaclhip.so")

ROUND_NONE, ROUND_FLOOR, ROUND_CEIL, ROUND_NEAREST, ROUND_PER_TRACK = 0, 1, 2, 3, 4
LOOP_CLAMP, LOOP_WRAP, LOOP_AS_COMPRESSED = 0, 1, 2
NORMALIZE_NEVER, NORMALIZE_LERP_ONLY, NORMALIZE_ALWAYS = 0, 1, 2
DEFAULT_SKIPPED, DEFAULT_CONSTANT, DEFAULT_VARIABLE, DEFAULT_LEGACY, DEFAULT_BIND_POSE = 0, 1, 2, 3, 4
# aclhip_status
(OK, ERROR_INVALID_ARGUMENT, ERROR_INVALID_CLIP, ERROR_UNSUPPORTED_FORMAT, ERROR_UNKNOWN_CLIP, ERROR_OUT_OF_MEMORY, ERROR_DEVICE, ERROR_NO_DEVICE,
 ERROR_UNKNOWN_DATABASE, ERROR_NOT_IN_DATABASE, ERROR_NO_METADATA) = range(11)
INVALID_HANDLE = 0xFFFFFFFF

EXPORTED_SYMBOLS = [
    "aclhip_status_string", "aclhip_last_error_message", "aclhip_abi_version", "aclhip_create", "aclhip_destroy", "aclhip_default_params",
    "aclhip_register_clip", "aclhip_unregister_clip", "aclhip_get_clip_info", "aclhip_clip_matches",
    "aclhip_decompress_tracks_batch", "aclhip_decompress_track_batch", "aclhip_decompress_tracks_host", "aclhip_decompress_track_host",
    "aclhip_get_rejected_instance_count", "aclhip_time_decompress_tracks_batch", "aclhip_batch_algorithmic_bytes",
    "aclhip_measure_write_bandwidth", "aclhip_measure_pose_store_bandwidth", "aclhip_describe_tracks_kernel",
    "aclhip_register_database", "aclhip_unregister_database", "aclhip_get_database_info", "aclhip_register_clip_with_database",
    "aclhip_database_stream_in", "aclhip_database_stream_out",
    "aclhip_all_gather_poses", "aclhip_probe_rccl", "aclhip_decompress_all_samples", "aclhip_check_clip", "aclhip_check_database",
    "aclhip_decompress_scalar_tracks_batch", "aclhip_decompress_scalar_track_batch", "aclhip_decompress_scalar_tracks_host", "aclhip_decompress_scalar_track_host",
    "aclhip_decompress_tracks_batch_rows", "aclhip_order_track_requests_for_locality", "aclhip_order_instances_for_locality", "aclhip_order_instances_device", "aclhip_order_instances_for_pose_windows",
    "aclhip_get_negative_scale_count", "aclhip_register_database_streamed", "aclhip_database_stream_in_from", "aclhip_get_lifetime_stats", "aclhip_peer_export_buffer", "aclhip_peer_open_buffer", "aclhip_peer_close_buffer", "aclhip_push_poses_to_peer",
    "aclhip_decompress_tracks_batch_out", "aclhip_decompress_tracks_host_out", "aclhip_layout_bytes_per_track",
    "aclhip_forget_stream", "aclhip_instance_list_create", "aclhip_instance_list_destroy", "aclhip_instance_list_set_clips", "aclhip_instance_list_update",
    "aclhip_decompress_tracks_list", "aclhip_instance_list_get_order", "aclhip_instance_list_attach", "aclhip_instance_list_note_changes",
    "aclhip_strip_database_tier", "aclhip_plan_hierarchy_walk", "aclhip_set_clip_hierarchy", "aclhip_decompress_poses_batch", "aclhip_decompress_poses_host", "aclhip_time_decompress_poses_batch",
    "aclhip_pose_windows_of_launch", "aclhip_order_instances_device_for_windows", "aclhip_describe_tracks_launch", "aclhip_analyze_clip",
    "aclhip_get_clip_metadata_info", "aclhip_get_clip_parent_indices", "aclhip_get_clip_track_descriptions", "aclhip_set_clip_hierarchy_from_metadata", "aclhip_read_clip_metadata",
    "aclhip_order_track_requests_device", "aclhip_decompress_track_batch_rows",
    "aclhip_check_track_map", "aclhip_register_track_map", "aclhip_unregister_track_map", "aclhip_get_track_map_info", "aclhip_decompress_tracks_batch_mapped",
    "aclhip_check_skeleton", "aclhip_register_skeleton", "aclhip_unregister_skeleton", "aclhip_get_skeleton_info", "aclhip_decompress_poses_batch_mapped",
    "aclhip_check_blend_mask", "aclhip_register_blend_mask", "aclhip_unregister_blend_mask", "aclhip_get_blend_mask_info", "aclhip_decompress_poses_batch_masked",
    "aclhip_decompress_track_object_batch", "aclhip_decompress_bone_object_batch_mapped", "aclhip_plan_bone_chain",
    "aclhip_decompress_poses_batch_bounds",
    "aclhip_decompress_poses_batch_additive_weighted",
    "aclhip_transform_poses_batch",
    "aclhip_blend_poses_batch",
    "aclhip_inverse_transform_poses_batch",
    "aclhip_measure_pose_error_batch",
    "aclhip_pose_matrices_batch", "aclhip_measure_pose_error_metric_batch",
    "aclhip_check_skin", "aclhip_register_skin", "aclhip_unregister_skin", "aclhip_get_skin_info", "aclhip_skinning_matrices_batch",
    "aclhip_check_raw_tracks", "aclhip_register_raw_tracks", "aclhip_unregister_raw_tracks", "aclhip_get_raw_tracks_info",
    "aclhip_sample_raw_tracks_batch",
    "aclhip_check_raw_scalar_tracks", "aclhip_register_raw_scalar_tracks", "aclhip_unregister_raw_scalar_tracks", "aclhip_get_raw_scalar_tracks_info",
    "aclhip_sample_raw_scalar_tracks_batch", "aclhip_sample_raw_scalar_track_batch", "aclhip_measure_scalar_error_batch",
    "aclhip_scalar_compress_bound", "aclhip_scalar_compress_workspace_bytes", "aclhip_compress_raw_scalar_tracks_batch",
    "aclhip_transform_compress_bound", "aclhip_transform_compress_workspace_bytes", "aclhip_compress_raw_tracks_batch",
    "aclhip_compress_tracks_workspace_bytes", "aclhip_compress_tracks_batch",
    "aclhip_variable_compress_num_segments", "aclhip_variable_compress_bound", "aclhip_compress_variable_workspace_bytes", "aclhip_compress_tracks_variable_batch",
    "aclhip_find_bit_rates_workspace_bytes", "aclhip_find_bit_rates_batch",
    "aclhip_compress_tracks_metric_batch", "aclhip_compress_tracks_variable_metric_batch", "aclhip_find_bit_rates_metric_batch",
    "aclhip_find_bit_rates_level_workspace_bytes", "aclhip_find_bit_rates_level_batch",
    "aclhip_compress_tracks_additive_batch", "aclhip_compress_tracks_variable_additive_batch", "aclhip_find_bit_rates_additive_batch",
]


class DecompressParams(ctypes.Structure):
    """aclhip_decompress_params"""
    _fields_ = [
        ("rounding_policy", ctypes.c_uint8), ("looping_policy", ctypes.c_uint8), ("normalization", ctypes.c_uint8), ("per_track_rounding", ctypes.c_uint8),
        ("default_rotation_mode", ctypes.c_uint8), ("default_translation_mode", ctypes.c_uint8), ("default_scale_mode", ctypes.c_uint8), ("reserved0", ctypes.c_uint8),
        ("default_values", ctypes.c_void_p), ("track_rounding_policies", ctypes.c_void_p), ("instance_rounding_policies", ctypes.c_void_p),
        ("instance_looping_policies", ctypes.c_void_p),
        ("track_rounding_table", ctypes.c_void_p), ("instance_rounding_tables", ctypes.c_void_p), ("track_rounding_stride", ctypes.c_uint32), ("flags", ctypes.c_uint32),
    ]


class PoseConsumers(ctypes.Structure):
    """aclhip_pose_consumers"""
    _fields_ = [
        ("additive_format", ctypes.c_uint32), ("object_space", ctypes.c_uint32),
        ("base_clips", ctypes.c_void_p), ("base_sample_times", ctypes.c_void_p), ("base_poses", ctypes.c_void_p), ("base_pose_stride_bytes", ctypes.c_uint64),
        ("num_blend_clips", ctypes.c_uint32), ("flags", ctypes.c_uint32),
        ("blend_clips", ctypes.c_void_p), ("blend_sample_times", ctypes.c_void_p), ("blend_weights", ctypes.c_void_p),
    ]


class OutputDesc(ctypes.Structure):
    """aclhip_output_desc"""
    _fields_ = [
        ("layout", ctypes.c_uint32), ("skip_rotations", ctypes.c_uint8), ("skip_translations", ctypes.c_uint8), ("skip_scales", ctypes.c_uint8), ("reserved0", ctypes.c_uint8),
        ("rows", ctypes.c_void_p), ("skip_tracks", ctypes.c_void_p),
        ("mask_table", ctypes.c_void_p), ("instance_masks", ctypes.c_void_p), ("instance_track_counts", ctypes.c_void_p), ("mask_stride", ctypes.c_uint32), ("reserved1", ctypes.c_uint32),
    ]


class TrackMapInfo(ctypes.Structure):
    """aclhip_track_map_info"""
    _fields_ = [
        ("num_tracks", ctypes.c_uint32), ("num_slots", ctypes.c_uint32), ("num_mapped", ctypes.c_uint32), ("num_dropped", ctypes.c_uint32),
        ("num_unmapped_slots", ctypes.c_uint32), ("is_identity", ctypes.c_uint32), ("is_order_preserving", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]


class TrackMapping(ctypes.Structure):
    """aclhip_track_mapping"""
    _fields_ = [
        ("map", ctypes.c_uint32), ("instance_maps", ctypes.c_void_p), ("fill_pose", ctypes.c_void_p), ("fill_unmapped", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]


class SkeletonInfo(ctypes.Structure):
    """aclhip_skeleton_info"""
    _fields_ = [
        ("num_bones", ctypes.c_uint32), ("has_hierarchy", ctypes.c_uint32), ("num_roots", ctypes.c_uint32), ("depth", ctypes.c_uint32),
        ("walk_steps", ctypes.c_uint32), ("has_negative_scale", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2),
    ]


class PoseMapping(ctypes.Structure):
    """aclhip_pose_mapping"""
    _fields_ = [
        ("skeleton", ctypes.c_uint32), ("instance_skeletons", ctypes.c_void_p), ("map", ctypes.c_uint32), ("instance_maps", ctypes.c_void_p),
        ("blend_maps", ctypes.c_void_p), ("base_maps", ctypes.c_void_p), ("reserved", ctypes.c_uint32 * 2),
    ]


class BlendMaskInfo(ctypes.Structure):
    """aclhip_blend_mask_info"""
    _fields_ = [("num_slots", ctypes.c_uint32), ("num_zero", ctypes.c_uint32), ("num_one", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class BlendMasking(ctypes.Structure):
    """aclhip_blend_masking"""
    _fields_ = [("mode", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("instance_masks", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2)]


class AdditiveLayering(ctypes.Structure):
    """aclhip_additive_layering"""
    _fields_ = [("instance_weights", ctypes.c_void_p), ("instance_masks", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2)]


class PoseBounds(ctypes.Structure):
    """aclhip_pose_bounds"""
    _fields_ = [("bounds", ctypes.c_void_p), ("bone_flags", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2)]


class PoseBufferConsumers(ctypes.Structure):
    """aclhip_pose_buffer_consumers; `bounds` is the address of a PoseBounds the caller keeps alive (ctypes.addressof), or None"""
    _fields_ = [
        ("skeleton", ctypes.c_uint32), ("instance_skeletons", ctypes.c_void_p), ("object_space", ctypes.c_uint32), ("additive_format", ctypes.c_uint32),
        ("additive_poses", ctypes.c_void_p), ("additive_pose_stride_bytes", ctypes.c_uint64), ("bounds", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2),
    ]


class PoseBufferInverse(ctypes.Structure):
    """aclhip_pose_buffer_inverse; `base_poses` and `instance_skeletons` are device addresses or None"""
    _fields_ = [
        ("skeleton", ctypes.c_uint32), ("instance_skeletons", ctypes.c_void_p), ("local_space", ctypes.c_uint32), ("additive_format", ctypes.c_uint32),
        ("base_poses", ctypes.c_void_p), ("base_pose_stride_bytes", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 3),
    ]


class PoseError(ctypes.Structure):
    """aclhip_pose_error: the worst bone of one instance; {-1, NO_BONE}: not measured, or nothing to measure"""
    _fields_ = [("error", ctypes.c_float), ("bone", ctypes.c_uint32)]


class PoseErrorWorst(ctypes.Structure):
    """aclhip_pose_error_worst: the worst record of a launch"""
    _fields_ = [("error", ctypes.c_float), ("bone", ctypes.c_uint32), ("instance", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


POSE_ERROR_DTYPE = np.dtype([("error", np.float32), ("bone", np.uint32)])                  # aclhip_pose_error as a numpy record
POSE_ERROR_WORST_DTYPE = np.dtype([("error", np.float32), ("bone", np.uint32), ("instance", np.uint32), ("reserved", np.uint32)])
NO_BONE = 0xFFFFFFFF        # ACLHIP_NO_BONE


class PoseErrorDesc(ctypes.Structure):
    """aclhip_pose_error_desc; every pointer is a device address or None"""
    _fields_ = [
        ("skeleton", ctypes.c_uint32), ("instance_skeletons", ctypes.c_void_p), ("object_space", ctypes.c_uint32), ("additive_format", ctypes.c_uint32),
        ("base_poses", ctypes.c_void_p), ("base_pose_stride_bytes", ctypes.c_uint64), ("shell_distances", ctypes.c_void_p), ("num_shell_distances", ctypes.c_uint32),
        ("shell_distance", ctypes.c_float), ("bone_errors", ctypes.c_void_p), ("bone_error_stride_bytes", ctypes.c_uint64), ("worst", ctypes.c_void_p),
        ("reserved", ctypes.c_uint64 * 2),
    ]


class PoseMatricesDesc(ctypes.Structure):
    """aclhip_pose_matrices_desc; `instance_skeletons` is a device address or None"""
    _fields_ = [
        ("skeleton", ctypes.c_uint32), ("instance_skeletons", ctypes.c_void_p), ("object_space", ctypes.c_uint32), ("layout", ctypes.c_uint32),
        ("reserved", ctypes.c_uint64 * 2),
    ]


MATRIX_3X4F_64 = 0                                          # aclhip_matrix_layout: 64 bytes per bone, x_axis | y_axis | z_axis | w_axis
ERROR_METRIC_QVVF, ERROR_METRIC_QVVF_MATRIX3X4F = 0, 1      # aclhip_error_metric


class SkinInfo(ctypes.Structure):
    """aclhip_skin_info"""
    _fields_ = [
        ("num_joints", ctypes.c_uint32), ("num_bones", ctypes.c_uint32), ("is_identity_joint_list", ctypes.c_uint32), ("has_inverse_bind", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 4),
    ]


class SkinningDesc(ctypes.Structure):
    """aclhip_skinning_desc; `instance_skeletons` and `instance_skins` are device addresses or None"""
    _fields_ = [
        ("skeleton", ctypes.c_uint32), ("instance_skeletons", ctypes.c_void_p), ("skin", ctypes.c_uint32), ("instance_skins", ctypes.c_void_p),
        ("object_space", ctypes.c_uint32), ("layout", ctypes.c_uint32), ("reserved", ctypes.c_uint64 * 2),
    ]


PALETTE_3X4F_64, PALETTE_3X4F_TRANSPOSED_48 = 0, 1         # aclhip_palette_layout: 64 bytes per joint as MATRIX_3X4F_64 | three float4 rows, 48 bytes
PALETTE_RECORD_BYTES = {PALETTE_3X4F_64: 64, PALETTE_3X4F_TRANSPOSED_48: 48}
MAX_SKINS = 4096            # ACLHIP_MAX_SKINS


class RawTracksInfo(ctypes.Structure):
    """aclhip_raw_tracks_info"""
    _fields_ = [
        ("num_tracks", ctypes.c_uint32), ("num_samples", ctypes.c_uint32), ("sample_rate", ctypes.c_float), ("duration", ctypes.c_float),
        ("looping_policy", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3),
    ]


class RawSampleDesc(ctypes.Structure):
    """aclhip_raw_sample_desc; every pointer is a device address or None"""
    _fields_ = [
        ("rounding_policy", ctypes.c_uint8), ("reserved0", ctypes.c_uint8 * 7), ("instance_rounding_policies", ctypes.c_void_p),
        ("track_rounding_policies", ctypes.c_void_p), ("num_track_rounding_policies", ctypes.c_uint32), ("reserved1", ctypes.c_uint32),
        ("rows", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2),
    ]


MAX_RAW_TRACKS = 4096       # ACLHIP_MAX_RAW_TRACKS


class RawScalarTracksInfo(ctypes.Structure):
    """aclhip_raw_scalar_tracks_info"""
    _fields_ = [
        ("num_tracks", ctypes.c_uint32), ("num_samples", ctypes.c_uint32), ("sample_rate", ctypes.c_float), ("duration", ctypes.c_float),
        ("looping_policy", ctypes.c_uint32), ("track_type", ctypes.c_uint32), ("num_components", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]


class ScalarErrorDesc(ctypes.Structure):
    """aclhip_scalar_error_desc; every pointer is a device address or None"""
    _fields_ = [
        ("num_tracks", ctypes.c_uint32), ("num_components", ctypes.c_uint32), ("track_errors", ctypes.c_void_p), ("track_error_stride_bytes", ctypes.c_uint64),
        ("worst", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2),
    ]


class ScalarCompressDesc(ctypes.Structure):
    """aclhip_scalar_compress_desc; track_precisions and workspace are device addresses"""
    _fields_ = [
        ("precision", ctypes.c_float), ("flags", ctypes.c_uint32), ("track_precisions", ctypes.c_void_p), ("num_track_precisions", ctypes.c_uint32),
        ("max_tracks", ctypes.c_uint32), ("workspace", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2),
    ]


class TransformCompressDesc(ctypes.Structure):
    """aclhip_transform_compress_desc; the four tables and the workspace are device addresses"""
    _fields_ = [
        ("flags", ctypes.c_uint32), ("max_tracks", ctypes.c_uint32), ("default_pose", ctypes.c_void_p), ("parent_indices", ctypes.c_void_p),
        ("track_precisions", ctypes.c_void_p), ("track_shell_distances", ctypes.c_void_p), ("num_table_tracks", ctypes.c_uint32), ("precision", ctypes.c_float),
        ("shell_distance", ctypes.c_float), ("workspace", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2),
    ]


class CompressTracksDesc(ctypes.Structure):
    """aclhip_compress_tracks_desc; the four tables, the workspace and shell_metadata are device addresses"""
    _fields_ = [
        ("rotation_format", ctypes.c_uint32), ("translation_format", ctypes.c_uint32), ("scale_format", ctypes.c_uint32), ("flags", ctypes.c_uint32),
        ("max_tracks", ctypes.c_uint32), ("num_table_tracks", ctypes.c_uint32), ("default_pose", ctypes.c_void_p), ("parent_indices", ctypes.c_void_p),
        ("track_precisions", ctypes.c_void_p), ("track_shell_distances", ctypes.c_void_p), ("precision", ctypes.c_float), ("shell_distance", ctypes.c_float),
        ("workspace", ctypes.c_void_p), ("shell_metadata", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2),
    ]


class CompressVariableDesc(ctypes.Structure):
    """aclhip_compress_variable_desc; the four tables, the workspace, shell_metadata and bit_rates are device addresses"""
    _fields_ = [
        ("flags", ctypes.c_uint32), ("max_tracks", ctypes.c_uint32), ("max_samples", ctypes.c_uint32), ("num_table_tracks", ctypes.c_uint32),
        ("default_pose", ctypes.c_void_p), ("parent_indices", ctypes.c_void_p), ("track_precisions", ctypes.c_void_p), ("track_shell_distances", ctypes.c_void_p),
        ("precision", ctypes.c_float), ("shell_distance", ctypes.c_float), ("workspace", ctypes.c_void_p), ("shell_metadata", ctypes.c_void_p),
        ("bit_rates", ctypes.c_void_p), ("bit_rate_instance_stride", ctypes.c_uint64), ("bit_rate_segment_stride", ctypes.c_uint64),
        ("rotation_bit_rate", ctypes.c_uint8), ("translation_bit_rate", ctypes.c_uint8), ("scale_bit_rate", ctypes.c_uint8), ("reserved_rate", ctypes.c_uint8),
        ("reserved_word", ctypes.c_uint32), ("reserved", ctypes.c_uint64 * 2),
    ]


class FindBitRatesDesc(ctypes.Structure):
    """aclhip_find_bit_rates_desc; the four tables, the workspace and shell_metadata are device addresses"""
    _fields_ = [
        ("flags", ctypes.c_uint32), ("max_tracks", ctypes.c_uint32), ("max_samples", ctypes.c_uint32), ("num_table_tracks", ctypes.c_uint32),
        ("default_pose", ctypes.c_void_p), ("parent_indices", ctypes.c_void_p), ("track_precisions", ctypes.c_void_p), ("track_shell_distances", ctypes.c_void_p),
        ("precision", ctypes.c_float), ("shell_distance", ctypes.c_float), ("workspace", ctypes.c_void_p), ("shell_metadata", ctypes.c_void_p),
        ("level", ctypes.c_uint32), ("reserved_word", ctypes.c_uint32), ("reserved", ctypes.c_uint64 * 2),
    ]


class AdditiveBase(ctypes.Structure):
    """aclhip_additive_base: base_raws is a device address, uint32 [num_instances] handles of registered raw track arrays"""
    _fields_ = [("base_raws", ctypes.c_void_p), ("additive_format", ctypes.c_uint32), ("reserved_word", ctypes.c_uint32), ("reserved", ctypes.c_uint64 * 2)]


COMPRESSION_LEVELS = {"lowest": 0, "low": 1, "medium": 2, "high": 3, "highest": 4, "automatic": 100}     # acl::compression_level8 (aclhip_find_bit_rates_desc::level)
LEVEL_AUTOMATIC = 100                   # ACLHIP_LEVEL_AUTOMATIC: aclhip_find_bit_rates_level_batch alone takes it, and the levels 3 and 4
ROTATION_QUATF_FULL, ROTATION_QUATF_DROP_W_FULL = 0, 2                                      # acl::rotation_format8 (aclhip_compress_tracks_desc::rotation_format)
VECTOR_VECTOR3F_FULL = 0                                                                    # acl::vector_format8
COMPRESS_OPTIMIZE_LOOPS = 1                                                                 # ACLHIP_COMPRESS_OPTIMIZE_LOOPS
COMPRESS_INCLUDE_PARENT_TRACK_INDICES, COMPRESS_INCLUDE_TRACK_DESCRIPTIONS = 2, 4           # ACLHIP_COMPRESS_INCLUDE_* (the transform compressor's)
COMPRESS_OK, COMPRESS_NOT_FINITE, COMPRESS_REFUSED = 0, 1, 2                                # aclhip_compress_result::status
COMPRESS_NOT_NORMALIZED = 3                                                                 # (the transform compressor's)
COMPRESS_RESULT_DTYPE = np.dtype([("status", np.uint32), ("size", np.uint32)])              # aclhip_compress_result as a numpy record
MAX_RAW_SCALAR_TRACKS = 4096        # ACLHIP_MAX_RAW_SCALAR_TRACKS
NO_TRACK = 0xFFFFFFFF               # ACLHIP_NO_TRACK
TRACK_FLOAT1F, TRACK_FLOAT2F, TRACK_FLOAT3F, TRACK_FLOAT4F, TRACK_VECTOR4F, TRACK_QVVF = 0, 1, 2, 3, 4, 12     # acl::track_type8
SCALAR_TRACK_COMPONENTS = {TRACK_FLOAT1F: 1, TRACK_FLOAT2F: 2, TRACK_FLOAT3F: 3, TRACK_FLOAT4F: 4, TRACK_VECTOR4F: 4}
TRACK_ERROR_DTYPE = np.dtype([("error", np.float32), ("track", np.uint32)])                 # aclhip_track_error as a numpy record
TRACK_ERROR_WORST_DTYPE = np.dtype([("error", np.float32), ("track", np.uint32), ("instance", np.uint32), ("reserved", np.uint32)])


class PoseBufferBlend(ctypes.Structure):
    """aclhip_pose_buffer_blend; `buffers` are device addresses (entries behind num_buffers stay None), `bounds` is the address of a
    PoseBounds the caller keeps alive (ctypes.addressof), or None"""
    _fields_ = [
        ("skeleton", ctypes.c_uint32), ("instance_skeletons", ctypes.c_void_p), ("num_buffers", ctypes.c_uint32), ("mode", ctypes.c_uint32),
        ("buffers", ctypes.c_void_p * 4), ("buffer_stride_bytes", ctypes.c_uint64 * 4), ("weights", ctypes.c_void_p), ("instance_masks", ctypes.c_void_p),
        ("object_space", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("bounds", ctypes.c_void_p), ("reserved", ctypes.c_uint64 * 2),
    ]


BLEND_WEIGHTED, BLEND_LAYERED = 0, 1   # ACLHIP_BLEND_WEIGHTED / ACLHIP_BLEND_LAYERED
MAX_BLEND_MASKS = 4096      # ACLHIP_MAX_BLEND_MASKS
MAX_SKELETONS = 1024        # ACLHIP_MAX_SKELETONS
TRACK_DROPPED = 0xFFFFFFFF  # ACLHIP_TRACK_DROPPED
MAX_TRACK_MAPS = 16384      # ACLHIP_MAX_TRACK_MAPS
ABI_VERSION = 6             # ACLHIP_ABI_VERSION: the struct layouts mirrored above
PEER_HANDLE_BYTES = 72      # ACLHIP_PEER_HANDLE_BYTES
LAYOUT_QVV48, LAYOUT_QVV40, LAYOUT_QV32 = 0, 1, 2  # aclhip_pose_layout
LAYOUTS = {"qvv48": (LAYOUT_QVV48, 48), "qvv40": (LAYOUT_QVV40, 40), "qv32": (LAYOUT_QV32, 32)}     # name -> (aclhip_pose_layout, bytes per track)


def relayout_pose(pose, layout, skip=(False, False, False), into=None):
    """Test helper (numpy, host): what a [..., num_tracks, 12] QVV48 pose looks like through `layout` with the sub-track kinds of
    `skip` (rotation, translation, scale) left untouched. Returns [..., num_tracks, floats per track]; skipped pieces keep the
    values of `into` (zeros when it is not given)."""
    pose = np.asarray(pose, dtype=np.float32)
    columns = {LAYOUT_QVV48: ([0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]), LAYOUT_QVV40: ([0, 1, 2, 3], [4, 5, 6], [7, 8, 9]), LAYOUT_QV32: ([0, 1, 2, 3], [4, 5, 6, 7], [])}[layout]
    sources = ([0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11])
    width = {LAYOUT_QVV48: 12, LAYOUT_QVV40: 10, LAYOUT_QV32: 8}[layout]
    out = np.zeros(pose.shape[:-1] + (width,), dtype=np.float32) if into is None else np.array(into, dtype=np.float32, copy=True)
    for kind in range(3):
        if skip[kind] or not columns[kind]:
            continue
        out[..., columns[kind]] = pose[..., sources[kind][: len(columns[kind])]]
    return out


ADDITIVE_NONE, ADDITIVE_RELATIVE, ADDITIVE_ADDITIVE0, ADDITIVE_ADDITIVE1 = 0, 1, 2, 3  # aclhip_additive_format
CONSUMERS_FAST = 1          # ACLHIP_CONSUMERS_FAST (aclhip_pose_consumers::flags)
DECODE_FAST = 1             # ACLHIP_DECODE_FAST (aclhip_decompress_params::flags)
NO_PARENT = 0xFFFFFFFF


class ClipInfo(ctypes.Structure):
    """aclhip_clip_info"""
    _fields_ = [
        ("num_tracks", ctypes.c_uint32), ("num_samples", ctypes.c_uint32), ("sample_rate", ctypes.c_float), ("duration", ctypes.c_float),
        ("num_segments", ctypes.c_uint32), ("has_scale", ctypes.c_uint32), ("looping_policy", ctypes.c_uint32), ("compressed_size", ctypes.c_uint32),
        ("hash", ctypes.c_uint32), ("num_animated_sub_tracks", ctypes.c_uint32), ("has_database", ctypes.c_uint32), ("has_stripped_keyframes", ctypes.c_uint32),
        ("track_type", ctypes.c_uint32), ("num_components", ctypes.c_uint32),
    ]


class ClipMetadataInfo(ctypes.Structure):
    """aclhip_clip_metadata_info"""
    _fields_ = [("has_metadata", ctypes.c_uint32), ("has_parent_track_indices", ctypes.c_uint32), ("has_track_descriptions", ctypes.c_uint32),
                ("has_track_names", ctypes.c_uint32), ("has_track_list_name", ctypes.c_uint32), ("has_contributing_error", ctypes.c_uint32)]


class DatabaseInfo(ctypes.Structure):
    """aclhip_database_info"""
    _fields_ = [
        ("num_clips", ctypes.c_uint32), ("num_segments", ctypes.c_uint32), ("max_chunk_size", ctypes.c_uint32),
        ("num_chunks", ctypes.c_uint32 * 2), ("num_loaded_chunks", ctypes.c_uint32 * 2), ("bulk_data_size", ctypes.c_uint32 * 2),
    ]


TIER_MEDIUM_IMPORTANCE = 1  # quality_tier::medium_importance (core/quality_tiers.h)
TIER_LOWEST_IMPORTANCE = 2


class AclHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"aclhip status {status}: {message}")
        self.status = status


_lib = None


def library_path():
    return _LIB_PATH


def load_library():
    """Loads libaclhip.so (raises when it was not built -- there is no fallback).

    PyTorch is imported first when it is installed: it bundles its own HIP runtime and the two cannot be loaded in the other order."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`; there is no CPU fallback")
    # Load order: this Python layer hands torch tensors' device pointers to the library, and the PyTorch wheel bundles its own HIP
    # runtime. Whichever of the two runtimes is loaded second finds "no HIP device", so torch (when present) always goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(_LIB_PATH)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    pparams = ctypes.POINTER(DecompressParams)
    lib.aclhip_status_string.argtypes = [i32]
    lib.aclhip_status_string.restype = ctypes.c_char_p
    lib.aclhip_last_error_message.argtypes = [vp]
    lib.aclhip_last_error_message.restype = ctypes.c_char_p
    lib.aclhip_abi_version.argtypes = []
    lib.aclhip_abi_version.restype = ctypes.c_uint32
    if lib.aclhip_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{_LIB_PATH} was built with ABI version {lib.aclhip_abi_version()}, this binding mirrors version {ABI_VERSION}: rebuild the library")
    lib.aclhip_create.argtypes = [i32, ctypes.POINTER(vp)]
    lib.aclhip_destroy.argtypes = [vp]
    lib.aclhip_destroy.restype = None
    lib.aclhip_default_params.argtypes = [pparams]
    lib.aclhip_default_params.restype = None
    lib.aclhip_register_clip.argtypes = [vp, vp, u64, i32, ctypes.POINTER(u32)]
    lib.aclhip_unregister_clip.argtypes = [vp, u32]
    lib.aclhip_get_clip_info.argtypes = [vp, u32, ctypes.POINTER(ClipInfo)]
    lib.aclhip_clip_matches.argtypes = [vp, u32, vp, ctypes.POINTER(i32)]
    lib.aclhip_decompress_tracks_batch.argtypes = [vp, vp, vp, u32, pparams, vp, u64, vp]
    lib.aclhip_decompress_track_batch.argtypes = [vp, vp, vp, vp, u32, pparams, vp, vp]
    lib.aclhip_decompress_tracks_host.argtypes = [vp, vp, vp, u32, pparams, u32, vp, u64]
    lib.aclhip_decompress_track_host.argtypes = [vp, vp, vp, vp, u32, pparams, u32, vp]
    lib.aclhip_get_rejected_instance_count.argtypes = [vp, ctypes.POINTER(u64)]
    lib.aclhip_time_decompress_tracks_batch.argtypes = [vp, vp, vp, u32, pparams, vp, u64, vp, u32, ctypes.POINTER(ctypes.c_float)]
    lib.aclhip_measure_write_bandwidth.argtypes = [vp, vp, u64, u32, vp, ctypes.POINTER(ctypes.c_float)]
    lib.aclhip_describe_tracks_kernel.argtypes = [vp, pparams, ctypes.c_char_p, u32]
    lib.aclhip_batch_algorithmic_bytes.argtypes = [vp, vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.aclhip_register_database.argtypes = [vp, vp, u64, vp, vp, i32, ctypes.POINTER(u32)]
    lib.aclhip_unregister_database.argtypes = [vp, u32]
    lib.aclhip_get_database_info.argtypes = [vp, u32, ctypes.POINTER(DatabaseInfo)]
    lib.aclhip_register_clip_with_database.argtypes = [vp, vp, u64, i32, u32, ctypes.POINTER(u32)]
    lib.aclhip_database_stream_in.argtypes = [vp, u32, u32, u32, vp, ctypes.POINTER(u32)]
    lib.aclhip_database_stream_out.argtypes = [vp, u32, u32, u32, vp, ctypes.POINTER(u32)]
    lib.aclhip_check_clip.argtypes = [vp, u64, i32, ctypes.c_char_p, u32]
    lib.aclhip_analyze_clip.argtypes = [vp, u64, i32, ctypes.POINTER(ctypes.c_uint32)]
    lib.aclhip_check_database.argtypes = [vp, u64, vp, vp, i32, ctypes.c_char_p, u32]
    lib.aclhip_decompress_all_samples.argtypes = [vp, u32, pparams, vp, vp, u64, vp]
    lib.aclhip_all_gather_poses.argtypes = [vp, vp, vp, vp, u64, vp]
    lib.aclhip_decompress_scalar_tracks_batch.argtypes = [vp, vp, vp, u32, pparams, vp, u64, vp]
    lib.aclhip_decompress_scalar_track_batch.argtypes = [vp, vp, vp, vp, u32, pparams, vp, u64, vp]
    lib.aclhip_decompress_scalar_tracks_host.argtypes = [vp, vp, vp, u32, pparams, vp, u64]
    lib.aclhip_decompress_scalar_track_host.argtypes = [vp, vp, vp, vp, u32, pparams, vp, u64]
    lib.aclhip_decompress_tracks_batch_rows.argtypes = [vp, vp, vp, vp, u32, pparams, vp, u64, vp]
    lib.aclhip_order_instances_for_locality.argtypes = [vp, vp, u32, vp]
    lib.aclhip_order_instances_for_pose_windows.argtypes = [u32, vp, u32, vp]
    lib.aclhip_order_track_requests_for_locality.argtypes = [vp, u32, vp]
    lib.aclhip_order_instances_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
    lib.aclhip_order_track_requests_device.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    lib.aclhip_decompress_track_batch_rows.argtypes = [vp, vp, vp, vp, vp, u32, pparams, vp, vp]
    pconsumers = ctypes.POINTER(PoseConsumers)
    poutput = ctypes.POINTER(OutputDesc)
    lib.aclhip_get_lifetime_stats.argtypes = [vp, ctypes.POINTER(u64)]
    lib.aclhip_get_negative_scale_count.argtypes = [vp, ctypes.POINTER(u64)]
    lib.aclhip_register_database_streamed.argtypes = [vp, vp, u64, i32, ctypes.POINTER(u32)]
    lib.aclhip_database_stream_in_from.argtypes = [vp, u32, u32, u32, vp, vp, ctypes.POINTER(u32)]
    lib.aclhip_peer_export_buffer.argtypes = [vp, vp, vp]
    lib.aclhip_peer_open_buffer.argtypes = [vp, vp, ctypes.POINTER(vp)]
    lib.aclhip_peer_close_buffer.argtypes = [vp, vp]
    lib.aclhip_push_poses_to_peer.argtypes = [vp, vp, u64, vp, u64, vp]
    lib.aclhip_decompress_tracks_batch_out.argtypes = [vp, vp, vp, u32, pparams, poutput, vp, u64, vp]
    lib.aclhip_decompress_tracks_host_out.argtypes = [vp, vp, vp, u32, pparams, u32, poutput, vp, u64]
    lib.aclhip_layout_bytes_per_track.argtypes = [u32]
    lib.aclhip_layout_bytes_per_track.restype = u32
    lib.aclhip_strip_database_tier.argtypes = [vp, u64, u32, vp, u64, ctypes.POINTER(u64)]
    lib.aclhip_plan_hierarchy_walk.argtypes = [vp, u32, u32, vp, ctypes.POINTER(u32)]
    lib.aclhip_set_clip_hierarchy.argtypes = [vp, u32, vp, u32]
    lib.aclhip_decompress_poses_batch.argtypes = [vp, vp, vp, u32, pparams, pconsumers, vp, u64, vp]
    lib.aclhip_decompress_poses_host.argtypes = [vp, vp, vp, u32, pparams, pconsumers, vp, u64]
    lib.aclhip_time_decompress_poses_batch.argtypes = [vp, vp, vp, u32, pparams, pconsumers, vp, u64, vp, u32, ctypes.POINTER(ctypes.c_float)]
    lib.aclhip_pose_windows_of_launch.argtypes = [vp, u32, u64, ctypes.POINTER(u32)]
    lib.aclhip_order_instances_device_for_windows.argtypes = [vp, u32, vp, vp, u32, vp, vp, vp, vp]
    lib.aclhip_describe_tracks_launch.argtypes = [vp, pparams, poutput, u64, ctypes.c_char_p, u32, ctypes.POINTER(u32)]
    lib.aclhip_get_clip_metadata_info.argtypes = [vp, u32, ctypes.POINTER(ClipMetadataInfo)]
    lib.aclhip_get_clip_parent_indices.argtypes = [vp, u32, vp, u32]
    lib.aclhip_get_clip_track_descriptions.argtypes = [vp, u32, vp, vp, vp, u32]
    lib.aclhip_set_clip_hierarchy_from_metadata.argtypes = [vp, u32]
    lib.aclhip_read_clip_metadata.argtypes = [vp, u64, ctypes.POINTER(ClipMetadataInfo), vp, vp, vp, vp, u32]
    lib.aclhip_check_track_map.argtypes = [vp, u32, u32, ctypes.POINTER(TrackMapInfo), ctypes.c_char_p, u32]
    lib.aclhip_register_track_map.argtypes = [vp, vp, u32, u32, ctypes.POINTER(u32)]
    lib.aclhip_unregister_track_map.argtypes = [vp, u32]
    lib.aclhip_get_track_map_info.argtypes = [vp, u32, ctypes.POINTER(TrackMapInfo)]
    lib.aclhip_decompress_tracks_batch_mapped.argtypes = [vp, vp, vp, u32, pparams, poutput, ctypes.POINTER(TrackMapping), vp, u64, vp]
    lib.aclhip_check_skeleton.argtypes = [vp, vp, u32, ctypes.POINTER(SkeletonInfo), ctypes.c_char_p, u32]
    lib.aclhip_register_skeleton.argtypes = [vp, vp, vp, u32, ctypes.POINTER(u32)]
    lib.aclhip_unregister_skeleton.argtypes = [vp, u32]
    lib.aclhip_get_skeleton_info.argtypes = [vp, u32, ctypes.POINTER(SkeletonInfo)]
    lib.aclhip_decompress_poses_batch_mapped.argtypes = [vp, vp, vp, u32, pparams, ctypes.POINTER(PoseConsumers), ctypes.POINTER(PoseMapping), vp, u64, vp]
    lib.aclhip_check_blend_mask.argtypes = [vp, u32, ctypes.POINTER(BlendMaskInfo), ctypes.c_char_p, u32]
    lib.aclhip_register_blend_mask.argtypes = [vp, vp, u32, ctypes.POINTER(u32)]
    lib.aclhip_unregister_blend_mask.argtypes = [vp, u32]
    lib.aclhip_get_blend_mask_info.argtypes = [vp, u32, ctypes.POINTER(BlendMaskInfo)]
    lib.aclhip_decompress_poses_batch_masked.argtypes = [vp, vp, vp, u32, pparams, ctypes.POINTER(PoseConsumers), ctypes.POINTER(PoseMapping), ctypes.POINTER(BlendMasking), vp, u64, vp]
    lib.aclhip_decompress_track_object_batch.argtypes = [vp, vp, vp, vp, u32, pparams, vp, vp]
    lib.aclhip_decompress_bone_object_batch_mapped.argtypes = [vp, vp, vp, vp, u32, pparams, ctypes.POINTER(PoseMapping), vp, vp]
    lib.aclhip_plan_bone_chain.argtypes = [vp, u32, u32, vp, u32, ctypes.POINTER(u32)]
    lib.aclhip_decompress_poses_batch_bounds.argtypes = [vp, vp, vp, u32, pparams, ctypes.POINTER(PoseConsumers), ctypes.POINTER(PoseMapping), ctypes.POINTER(BlendMasking),
                                                         ctypes.POINTER(PoseBounds), vp, u64, vp]
    lib.aclhip_decompress_poses_batch_additive_weighted.argtypes = [vp, vp, vp, u32, pparams, ctypes.POINTER(PoseConsumers), ctypes.POINTER(PoseMapping),
                                                                    ctypes.POINTER(AdditiveLayering), vp, u64, vp]
    lib.aclhip_transform_poses_batch.argtypes = [vp, vp, u64, u32, ctypes.POINTER(PoseBufferConsumers), vp, u64, vp]
    lib.aclhip_blend_poses_batch.argtypes = [vp, ctypes.POINTER(PoseBufferBlend), u32, vp, u64, vp]
    lib.aclhip_inverse_transform_poses_batch.argtypes = [vp, vp, u64, u32, ctypes.POINTER(PoseBufferInverse), vp, u64, vp]
    lib.aclhip_measure_pose_error_batch.argtypes = [vp, vp, u64, vp, u64, u32, ctypes.POINTER(PoseErrorDesc), vp, vp]
    lib.aclhip_measure_pose_error_metric_batch.argtypes = [vp, vp, u64, vp, u64, u32, ctypes.POINTER(PoseErrorDesc), u32, vp, vp]
    lib.aclhip_pose_matrices_batch.argtypes = [vp, vp, u64, u32, ctypes.POINTER(PoseMatricesDesc), vp, u64, vp]
    lib.aclhip_check_skin.argtypes = [vp, vp, u32, u32, ctypes.POINTER(SkinInfo), ctypes.c_char_p, u32]
    lib.aclhip_register_skin.argtypes = [vp, vp, vp, u32, u32, ctypes.POINTER(u32)]
    lib.aclhip_unregister_skin.argtypes = [vp, u32]
    lib.aclhip_get_skin_info.argtypes = [vp, u32, ctypes.POINTER(SkinInfo)]
    lib.aclhip_skinning_matrices_batch.argtypes = [vp, vp, u64, u32, ctypes.POINTER(SkinningDesc), vp, u64, vp]
    lib.aclhip_check_raw_tracks.argtypes = [vp, u32, u32, ctypes.c_float, u32, ctypes.POINTER(RawTracksInfo), ctypes.c_char_p, u32]
    lib.aclhip_register_raw_tracks.argtypes = [vp, vp, u32, u32, ctypes.c_float, u32, ctypes.POINTER(u32)]
    lib.aclhip_unregister_raw_tracks.argtypes = [vp, u32]
    lib.aclhip_get_raw_tracks_info.argtypes = [vp, u32, ctypes.POINTER(RawTracksInfo)]
    lib.aclhip_sample_raw_tracks_batch.argtypes = [vp, vp, vp, u32, ctypes.POINTER(RawSampleDesc), vp, u64, vp]
    lib.aclhip_check_raw_scalar_tracks.argtypes = [vp, u32, u32, u32, ctypes.c_float, u32, ctypes.POINTER(RawScalarTracksInfo), ctypes.c_char_p, u32]
    lib.aclhip_register_raw_scalar_tracks.argtypes = [vp, vp, u32, u32, u32, ctypes.c_float, u32, ctypes.POINTER(u32)]
    lib.aclhip_unregister_raw_scalar_tracks.argtypes = [vp, u32]
    lib.aclhip_get_raw_scalar_tracks_info.argtypes = [vp, u32, ctypes.POINTER(RawScalarTracksInfo)]
    lib.aclhip_sample_raw_scalar_tracks_batch.argtypes = [vp, vp, vp, u32, ctypes.POINTER(RawSampleDesc), vp, u64, vp]
    lib.aclhip_sample_raw_scalar_track_batch.argtypes = [vp, vp, vp, vp, u32, ctypes.POINTER(RawSampleDesc), vp, u64, vp]
    lib.aclhip_measure_scalar_error_batch.argtypes = [vp, vp, u64, vp, u64, u32, ctypes.POINTER(ScalarErrorDesc), vp, vp]
    lib.aclhip_scalar_compress_bound.argtypes = [u32, u32, u32]
    lib.aclhip_scalar_compress_bound.restype = u64
    lib.aclhip_scalar_compress_workspace_bytes.argtypes = [u32, u32]
    lib.aclhip_scalar_compress_workspace_bytes.restype = u64
    lib.aclhip_compress_raw_scalar_tracks_batch.argtypes = [vp, vp, u32, ctypes.POINTER(ScalarCompressDesc), vp, u64, vp, vp]
    lib.aclhip_transform_compress_bound.argtypes = [u32, u32, u32]
    lib.aclhip_transform_compress_bound.restype = u64
    lib.aclhip_transform_compress_workspace_bytes.argtypes = [u32, u32]
    lib.aclhip_transform_compress_workspace_bytes.restype = u64
    lib.aclhip_compress_raw_tracks_batch.argtypes = [vp, vp, u32, ctypes.POINTER(TransformCompressDesc), vp, u64, vp, vp]
    lib.aclhip_compress_tracks_workspace_bytes.argtypes = [u32, u32]
    lib.aclhip_compress_tracks_workspace_bytes.restype = u64
    lib.aclhip_compress_tracks_batch.argtypes = [vp, vp, u32, ctypes.POINTER(CompressTracksDesc), vp, u64, vp, vp]
    lib.aclhip_variable_compress_num_segments.argtypes = [u32]
    lib.aclhip_variable_compress_num_segments.restype = u32
    lib.aclhip_variable_compress_bound.argtypes = [u32, u32, u32]
    lib.aclhip_variable_compress_bound.restype = u64
    lib.aclhip_compress_variable_workspace_bytes.argtypes = [u32, u32, u32]
    lib.aclhip_compress_variable_workspace_bytes.restype = u64
    lib.aclhip_compress_tracks_variable_batch.argtypes = [vp, vp, u32, ctypes.POINTER(CompressVariableDesc), vp, u64, vp, vp]
    lib.aclhip_find_bit_rates_workspace_bytes.argtypes = [u32, u32, u32]
    lib.aclhip_find_bit_rates_workspace_bytes.restype = u64
    lib.aclhip_find_bit_rates_batch.argtypes = [vp, vp, u32, ctypes.POINTER(FindBitRatesDesc), vp, u64, u64, vp, vp]
    lib.aclhip_compress_tracks_metric_batch.argtypes = [vp, vp, u32, ctypes.POINTER(CompressTracksDesc), vp, u64, vp, u32, vp]
    lib.aclhip_compress_tracks_variable_metric_batch.argtypes = [vp, vp, u32, ctypes.POINTER(CompressVariableDesc), vp, u64, vp, u32, vp]
    lib.aclhip_find_bit_rates_metric_batch.argtypes = [vp, vp, u32, ctypes.POINTER(FindBitRatesDesc), vp, u64, u64, vp, u32, vp]
    lib.aclhip_find_bit_rates_level_workspace_bytes.argtypes = [u32, u32, u32]
    lib.aclhip_find_bit_rates_level_workspace_bytes.restype = u64
    lib.aclhip_find_bit_rates_level_batch.argtypes = [vp, vp, u32, ctypes.POINTER(FindBitRatesDesc), vp, u64, u64, vp, u32, vp]
    lib.aclhip_compress_tracks_additive_batch.argtypes = [vp, vp, u32, ctypes.POINTER(CompressTracksDesc), vp, u64, vp, ctypes.POINTER(AdditiveBase), vp]
    lib.aclhip_compress_tracks_variable_additive_batch.argtypes = [vp, vp, u32, ctypes.POINTER(CompressVariableDesc), vp, u64, vp, ctypes.POINTER(AdditiveBase), vp]
    lib.aclhip_find_bit_rates_additive_batch.argtypes = [vp, vp, u32, ctypes.POINTER(FindBitRatesDesc), vp, u64, u64, vp, ctypes.POINTER(AdditiveBase), vp]
    _lib = lib
    return lib


def _skeleton_arrays(parent_indices, reference_pose, num_bones):
    parents = np.ascontiguousarray(parent_indices, dtype=np.uint32) if parent_indices is not None else None
    pose = np.ascontiguousarray(reference_pose, dtype=np.float32) if reference_pose is not None else None
    if num_bones is None:
        num_bones = pose.size // 12 if pose is not None else (parents.size if parents is not None else 0)
    return parents, pose, int(num_bones)


def check_skeleton(parent_indices, reference_pose, num_bones=None):
    """Host only validation of a skeleton (no GPU needed): what aclhip_register_skeleton checks. parent_indices may be None (local space
    only), reference_pose is float32 [num_bones, 12]. Returns (status, message, SkeletonInfo)."""
    parents, pose, num_bones = _skeleton_arrays(parent_indices, reference_pose, num_bones)
    message, info = ctypes.create_string_buffer(256), SkeletonInfo()
    status = load_library().aclhip_check_skeleton(parents.ctypes.data if parents is not None else None, pose.ctypes.data if pose is not None else None,
                                                  num_bones, ctypes.byref(info), message, 256)
    return status, message.value.decode(), info


def check_blend_mask(weights, num_slots=None):
    """Host only validation of a blend mask (no GPU needed): what aclhip_register_blend_mask checks. weights: float32 [num_slots] in
    skeleton slot order, or None. Returns (status, message, BlendMaskInfo)."""
    table = np.ascontiguousarray(weights, dtype=np.float32) if weights is not None else None
    if num_slots is None:
        num_slots = table.size if table is not None else 0
    message, info = ctypes.create_string_buffer(256), BlendMaskInfo()
    status = load_library().aclhip_check_blend_mask(table.ctypes.data if table is not None else None, int(num_slots), ctypes.byref(info), message, 256)
    return status, message.value.decode(), info


def _skin_arrays(joint_bones, inverse_bind, num_joints, num_bones):
    joints = np.ascontiguousarray(joint_bones, dtype=np.uint32) if joint_bones is not None else None
    matrices = np.ascontiguousarray(inverse_bind, dtype=np.float32) if inverse_bind is not None else None
    if num_joints is None:
        num_joints = joints.size if joints is not None else (matrices.size // 16 if matrices is not None else num_bones)
    num_joints = int(num_joints)
    # (the library reads num_joints entries of each array it is handed: never more than the caller's arrays hold)
    if joints is not None and joints.size < num_joints:
        raise ValueError(f"joint_bones holds {joints.size} entries, num_joints is {num_joints}")
    if matrices is not None and matrices.size < 16 * num_joints:
        raise ValueError(f"inverse_bind holds {matrices.size} floats, {num_joints} joints need {16 * num_joints}")
    return joints, matrices, num_joints


def check_skin(joint_bones, inverse_bind, num_bones, num_joints=None):
    """Host only validation of a skin (no GPU needed): what aclhip_register_skin checks. joint_bones: uint32 [num_joints] or None (the
    identity list); inverse_bind: float32 [num_joints, 4, 4] in the MATRIX_3X4F_64 layout or None (identity matrices). Returns (status,
    message, SkinInfo)."""
    joints, matrices, num_joints = _skin_arrays(joint_bones, inverse_bind, num_joints, num_bones)
    message, info = ctypes.create_string_buffer(256), SkinInfo()
    status = load_library().aclhip_check_skin(joints.ctypes.data if joints is not None else None, matrices.ctypes.data if matrices is not None else None,
                                              num_joints, int(num_bones), ctypes.byref(info), message, 256)
    return status, message.value.decode(), info


def _raw_samples(samples):
    """[num_samples, num_tracks, 12] float32, contiguous: the sample major QVV48 layout the library takes"""
    array = np.ascontiguousarray(samples, dtype=np.float32)
    if array.ndim != 3 or array.shape[2] != 12:
        raise ValueError(f"raw samples are [num_samples, num_tracks, 12] floats, not {array.shape}")
    return array


def check_raw_tracks(samples, sample_rate, looping_policy=LOOP_CLAMP):
    """Host only validation of a raw track array (no GPU needed): what aclhip_register_raw_tracks checks. samples: float32
    [num_samples, num_tracks, 12]. Returns (status, message, RawTracksInfo)."""
    array = _raw_samples(samples)
    message, info = ctypes.create_string_buffer(256), RawTracksInfo()
    status = load_library().aclhip_check_raw_tracks(array.ctypes.data, array.shape[1], array.shape[0], float(sample_rate), int(looping_policy), ctypes.byref(info), message, 256)
    return status, message.value.decode(), info


def _raw_scalar_samples(samples, track_type):
    """[num_samples, num_tracks, C] float32, contiguous ([num_samples, num_tracks] is taken as C = 1): the sample major layout the library takes"""
    array = np.ascontiguousarray(samples, dtype=np.float32)
    if array.ndim == 2:
        array = array[:, :, None]
    components = SCALAR_TRACK_COMPONENTS.get(int(track_type))
    if array.ndim != 3 or (components is not None and array.shape[2] != components):
        raise ValueError(f"raw scalar samples of track type {track_type} are [num_samples, num_tracks, {components}] floats, not {array.shape}")
    return array


def check_raw_scalar_tracks(samples, track_type, sample_rate, looping_policy=LOOP_CLAMP):
    """Host only validation of a raw scalar track array (no GPU needed): what aclhip_register_raw_scalar_tracks checks. samples: float32
    [num_samples, num_tracks, C] or [num_samples, num_tracks]. Returns (status, message, RawScalarTracksInfo)."""
    array = _raw_scalar_samples(samples, track_type)
    message, info = ctypes.create_string_buffer(256), RawScalarTracksInfo()
    status = load_library().aclhip_check_raw_scalar_tracks(array.ctypes.data, int(track_type), array.shape[1], array.shape[0], float(sample_rate), int(looping_policy),
                                                           ctypes.byref(info), message, 256)
    return status, message.value.decode(), info


def check_track_map(track_to_slot, num_slots):
    """Host only validation of a track map (no GPU needed): what aclhip_register_track_map checks. Returns (status, message, TrackMapInfo)."""
    table = np.ascontiguousarray(track_to_slot, dtype=np.uint32)
    message, info = ctypes.create_string_buffer(256), TrackMapInfo()
    status = load_library().aclhip_check_track_map(table.ctypes.data, table.size, int(num_slots), ctypes.byref(info), message, 256)
    return status, message.value.decode(), info


def probe_rccl():
    """aclhip_probe_rccl: (version code, path of the library, how it was found) of the RCCL aclhip_all_gather_poses would call; raises AclHipError when there is none"""
    lib = load_library()
    version, path, how = ctypes.c_int(0), ctypes.create_string_buffer(512), ctypes.create_string_buffer(128)
    status = lib.aclhip_probe_rccl(ctypes.byref(version), path, 512, how, 128)
    if status != 0:
        raise AclHipError(status, lib.aclhip_last_error_message(None).decode())
    return version.value, path.value.decode(), how.value.decode()


def check_clip(blob, check_hash=True):
    """Host only validation of a compressed_tracks blob (no GPU needed). Returns (status, message); status 0 = valid."""
    array = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    message = ctypes.create_string_buffer(512)
    status = load_library().aclhip_check_clip(array.ctypes.data, array.size, 1 if check_hash else 0, message, 512)
    return status, message.value.decode()


CLIP_FACT_SHORT_EXACT_MATH, CLIP_FACT_RAW_ROTATIONS, CLIP_FACT_NEGATIVE_SCALE = 1, 2, 4


def read_clip_metadata(blob):
    """aclhip_read_clip_metadata (host only): (ClipMetadataInfo, parents or None, (default_values [n, 12], precisions, shell_distances) or None)"""
    lib = load_library()
    num_tracks = int(np.frombuffer(bytes(blob[16:20]), dtype=np.uint32)[0])
    info = ClipMetadataInfo()
    parents = np.zeros(max(num_tracks, 1), dtype=np.uint32)
    defaults, precisions, shells = np.zeros((max(num_tracks, 1), 12), dtype=np.float32), np.zeros(max(num_tracks, 1), dtype=np.float32), np.zeros(max(num_tracks, 1), dtype=np.float32)
    status = lib.aclhip_read_clip_metadata(blob.ctypes.data, blob.size, ctypes.byref(info), parents.ctypes.data, defaults.ctypes.data, precisions.ctypes.data, shells.ctypes.data, max(num_tracks, 1))
    if status != 0:
        raise AclHipError(status, lib.aclhip_last_error_message(None).decode())
    return (info, parents[:num_tracks] if info.has_parent_track_indices else None,
            (defaults[:num_tracks], precisions[:num_tracks], shells[:num_tracks]) if info.has_track_descriptions else None)


def analyze_clip(blob, check_hash=True):
    """Host only: what registration derives about the values a clip can decode to (aclhip_analyze_clip). Returns the CLIP_FACT_* bits."""
    array = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    facts = ctypes.c_uint32(0)
    status = load_library().aclhip_analyze_clip(array.ctypes.data, array.size, 1 if check_hash else 0, ctypes.byref(facts))
    if status != 0:
        raise AclHipError(status, "aclhip_analyze_clip")
    return int(facts.value)


def check_database(database, bulk_data_medium=None, bulk_data_low=None, check_hash=True):
    """Host only validation of a compressed_database (+ split bulk data). Returns (status, message)."""
    as_array = lambda b: None if b is None else (np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else b)
    array, medium, low = as_array(database), as_array(bulk_data_medium), as_array(bulk_data_low)
    message = ctypes.create_string_buffer(512)
    status = load_library().aclhip_check_database(array.ctypes.data, array.size, _host_ptr(medium), _host_ptr(low), 1 if check_hash else 0, message, 512)
    return status, message.value.decode()


def order_instances_for_locality(clips, windows_per_instance=1):
    """aclhip_order_instances_for_pose_windows (no context: the caller says how many wavefronts a pose takes): host only, no GPU needed."""
    clips = np.ascontiguousarray(clips, dtype=np.uint32)
    order = np.empty(clips.size, dtype=np.uint32)
    status = load_library().aclhip_order_instances_for_pose_windows(windows_per_instance, clips.ctypes.data, clips.size, order.ctypes.data)
    if status != 0:
        raise AclHipError(status, "aclhip_order_instances_for_pose_windows failed")
    return order


def order_track_requests_for_locality(clips):
    """aclhip_order_track_requests_for_locality: host only, no GPU needed."""
    clips = np.ascontiguousarray(clips, dtype=np.uint32)
    order = np.empty(clips.size, dtype=np.uint32)
    status = load_library().aclhip_order_track_requests_for_locality(clips.ctypes.data, clips.size, order.ctypes.data)
    if status != 0:
        raise AclHipError(status, "aclhip_order_track_requests_for_locality failed")
    return order


def strip_database_tier(database, tier):
    """aclhip_strip_database_tier (host only): (status, stripped compressed_database as a 16 byte aligned uint8 array or None)"""
    from .synth import aligned_bytes
    array = np.frombuffer(database, dtype=np.uint8) if not isinstance(database, np.ndarray) else database
    lib = load_library()
    size = ctypes.c_uint64(0)
    status = lib.aclhip_strip_database_tier(array.ctypes.data, array.size, int(tier), None, 0, ctypes.byref(size))
    if status != 0:
        return status, None
    out = aligned_bytes(size.value)
    status = lib.aclhip_strip_database_tier(array.ctypes.data, array.size, int(tier), out.ctypes.data, out.size, ctypes.byref(size))
    return status, (out if status == 0 else None)


def plan_hierarchy_walk(parent_indices, transforms_per_step):
    """aclhip_plan_hierarchy_walk (host only): (number of steps, 1-based step per transform with 0 for roots)"""
    parents = np.ascontiguousarray(parent_indices, dtype=np.uint32)
    steps = np.zeros(parents.size, dtype=np.uint32)
    num_steps = ctypes.c_uint32(0)
    status = load_library().aclhip_plan_hierarchy_walk(parents.ctypes.data, parents.size, int(transforms_per_step), steps.ctypes.data, ctypes.byref(num_steps))
    if status != 0:
        raise AclHipError(status, "aclhip_plan_hierarchy_walk: transforms must be sorted parent first")
    return num_steps.value, steps


def plan_bone_chain(parent_indices, bone, chain_capacity=None, query_length_only=False):
    """aclhip_plan_bone_chain (host only): the chain of `bone`, root first, as the object space single bone requests walk it.
    query_length_only: passes a NULL chain and returns the length alone."""
    parents = np.ascontiguousarray(parent_indices, dtype=np.uint32)
    length = ctypes.c_uint32(0)
    lib = load_library()
    if query_length_only:
        status = lib.aclhip_plan_bone_chain(parents.ctypes.data, parents.size, int(bone), None, 0, ctypes.byref(length))
        if status != 0:
            raise AclHipError(status, "aclhip_plan_bone_chain")
        return length.value
    capacity = int(chain_capacity) if chain_capacity is not None else max(parents.size, 1)
    chain = np.full(max(capacity, 1), 0xFFFFFFFF, dtype=np.uint32)
    status = lib.aclhip_plan_bone_chain(parents.ctypes.data, parents.size, int(bone), chain.ctypes.data, capacity, ctypes.byref(length))
    if status != 0:
        raise AclHipError(status, "aclhip_plan_bone_chain: transforms sorted parent first, bone < num_tracks, a chain that fits")
    return chain[:length.value].copy()


def default_params(**overrides):
    params = DecompressParams()
    load_library().aclhip_default_params(ctypes.byref(params))
    for key, value in overrides.items():
        if not hasattr(params, key):
            raise AttributeError(f"aclhip_decompress_params has no field '{key}'")
        setattr(params, key, value)
    return params


def _host_ptr(array):
    return array.ctypes.data if array is not None else None


class Context:
    """An aclhip_context bound to one HIP device: owns the HBM copies of registered clips."""

    def __init__(self, device_index=0):
        self._lib = load_library()
        handle = ctypes.c_void_p()
        status = self._lib.aclhip_create(device_index, ctypes.byref(handle))
        if status != 0:
            raise AclHipError(status, self._lib.aclhip_status_string(status).decode())
        self._handle = handle
        self.device_index = device_index

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.aclhip_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, status):
        if status != 0:
            message = self._lib.aclhip_last_error_message(self._handle).decode() or self._lib.aclhip_status_string(status).decode()
            raise AclHipError(status, message)

    # ---- clips (decompression_context::initialize) ----
    def register_clip(self, blob, check_hash=True):
        """blob: bytes-like / uint8 numpy array holding one compressed_tracks. Returns the clip handle."""
        array = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
        handle = ctypes.c_uint32(INVALID_HANDLE)
        self._check(self._lib.aclhip_register_clip(self._handle, array.ctypes.data, array.size, 1 if check_hash else 0, ctypes.byref(handle)))
        return handle.value

    def unregister_clip(self, clip):
        self._check(self._lib.aclhip_unregister_clip(self._handle, clip))

    # ---- persistent instance lists (aclhip_instance_list_*): device pointers, stream ordered ----
    def instance_list_create(self, num_instances):
        handle = ctypes.c_uint32(INVALID_HANDLE)
        self._check(self._lib.aclhip_instance_list_create(self._handle, ctypes.c_uint32(num_instances), ctypes.byref(handle)))
        return handle.value

    def instance_list_destroy(self, instance_list):
        self._check(self._lib.aclhip_instance_list_destroy(self._handle, ctypes.c_uint32(instance_list)))

    def instance_list_set_clips(self, instance_list, clips_ptr, stream=None):
        self._check(self._lib.aclhip_instance_list_set_clips(self._handle, ctypes.c_uint32(instance_list), ctypes.c_void_p(clips_ptr), ctypes.c_void_p(stream)))

    def instance_list_update(self, instance_list, instances_ptr, clips_ptr, count, stream=None):
        self._check(self._lib.aclhip_instance_list_update(self._handle, ctypes.c_uint32(instance_list), ctypes.c_void_p(instances_ptr), ctypes.c_void_p(clips_ptr),
                                                          ctypes.c_uint32(count), ctypes.c_void_p(stream)))

    def instance_list_attach(self, instance_list, caller_clips_ptr, stream=None):
        """aclhip_instance_list_attach: the list decodes the caller's own device clip array (kept alive and in place by the caller)"""
        self._check(self._lib.aclhip_instance_list_attach(self._handle, ctypes.c_uint32(instance_list), ctypes.c_void_p(caller_clips_ptr), ctypes.c_void_p(stream)))

    def instance_list_note_changes(self, instance_list, count):
        self._check(self._lib.aclhip_instance_list_note_changes(self._handle, ctypes.c_uint32(instance_list), ctypes.c_uint32(count)))

    def decompress_tracks_list(self, instance_list, times_ptr, poses_ptr, pose_stride_bytes, params=None, output=None, poses_in_instance_order=False, stream=None):
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_tracks_list(self._handle, ctypes.c_uint32(instance_list), ctypes.c_void_p(times_ptr), ctypes.byref(params),
                                                            ctypes.byref(output) if output is not None else None, ctypes.c_int(1 if poses_in_instance_order else 0),
                                                            ctypes.c_void_p(poses_ptr), ctypes.c_uint64(pose_stride_bytes), ctypes.c_void_p(stream)))

    def instance_list_order(self, instance_list):
        """(device address of the slot -> instance order, number of orderings so far)"""
        order, count = ctypes.c_void_p(0), ctypes.c_uint64(0)
        self._check(self._lib.aclhip_instance_list_get_order(self._handle, ctypes.c_uint32(instance_list), ctypes.byref(order), ctypes.byref(count)))
        return order.value, count.value

    def forget_stream(self, stream):
        """aclhip_forget_stream: before destroying a stream the context has launched on"""
        self._check(self._lib.aclhip_forget_stream(self._handle, ctypes.c_void_p(stream)))

    def clip_info(self, clip):
        info = ClipInfo()
        self._check(self._lib.aclhip_get_clip_info(self._handle, clip, ctypes.byref(info)))
        return info

    def clip_metadata_info(self, clip):
        info = ClipMetadataInfo()
        self._check(self._lib.aclhip_get_clip_metadata_info(self._handle, clip, ctypes.byref(info)))
        return info

    def clip_parent_indices(self, clip):
        """compressed_tracks::get_parent_track_index of every track (NO_PARENT for roots); AclHipError(ERROR_NO_METADATA) when not stored"""
        parents = np.zeros(self.clip_info(clip).num_tracks, dtype=np.uint32)
        self._check(self._lib.aclhip_get_clip_parent_indices(self._handle, clip, parents.ctypes.data, parents.size))
        return parents

    def clip_track_descriptions(self, clip):
        """(default_values [num_tracks, 12], precisions, shell_distances) from the blob's track descriptions"""
        num_tracks = self.clip_info(clip).num_tracks
        defaults, precisions, shells = np.zeros((num_tracks, 12), dtype=np.float32), np.zeros(num_tracks, dtype=np.float32), np.zeros(num_tracks, dtype=np.float32)
        self._check(self._lib.aclhip_get_clip_track_descriptions(self._handle, clip, defaults.ctypes.data, precisions.ctypes.data, shells.ctypes.data, num_tracks))
        return defaults, precisions, shells

    def set_clip_hierarchy_from_metadata(self, clip):
        self._check(self._lib.aclhip_set_clip_hierarchy_from_metadata(self._handle, clip))

    def clip_matches(self, clip, blob):
        matches = ctypes.c_int(0)
        self._check(self._lib.aclhip_clip_matches(self._handle, clip, blob.ctypes.data, ctypes.byref(matches)))
        return bool(matches.value)

    # ---- databases (database_context) ----
    def register_database(self, database, bulk_data_medium=None, bulk_data_low=None, check_hash=True):
        """database: one compressed_database (bytes-like / uint8 array); bulk data arrays when it was split off. Returns the handle."""
        as_array = lambda b: None if b is None else (np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else b)
        array, medium, low = as_array(database), as_array(bulk_data_medium), as_array(bulk_data_low)
        handle = ctypes.c_uint32(INVALID_HANDLE)
        self._check(self._lib.aclhip_register_database(self._handle, array.ctypes.data, array.size, _host_ptr(medium), _host_ptr(low),
                                                       1 if check_hash else 0, ctypes.byref(handle)))
        return handle.value

    def register_database_streamed(self, database, check_hash=True):
        """aclhip_register_database_streamed: the bulk data arrives with the stream-in requests (database_stream_in_from)"""
        handle = ctypes.c_uint32(INVALID_HANDLE)
        self._check(self._lib.aclhip_register_database_streamed(self._handle, database.ctypes.data, database.size, int(check_hash), ctypes.byref(handle)))
        return handle.value

    def database_stream_in_from(self, database, tier, tier_bulk_data, num_chunks=0xFFFFFFFF, stream=None):
        moved = ctypes.c_uint32(0)
        self._check(self._lib.aclhip_database_stream_in_from(self._handle, database, tier, num_chunks, tier_bulk_data.ctypes.data, stream, ctypes.byref(moved)))
        return moved.value

    def unregister_database(self, database):
        self._check(self._lib.aclhip_unregister_database(self._handle, database))

    def database_info(self, database):
        info = DatabaseInfo()
        self._check(self._lib.aclhip_get_database_info(self._handle, database, ctypes.byref(info)))
        return info

    def register_clip_with_database(self, blob, database, check_hash=True):
        array = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
        handle = ctypes.c_uint32(INVALID_HANDLE)
        self._check(self._lib.aclhip_register_clip_with_database(self._handle, array.ctypes.data, array.size, 1 if check_hash else 0, database, ctypes.byref(handle)))
        return handle.value

    def database_stream_in(self, database, tier, num_chunks=0xFFFFFFFF, stream=None):
        """database_context::stream_in(tier, num_chunks); returns how many chunks were enqueued (0 = nothing left)."""
        moved = ctypes.c_uint32(0)
        self._check(self._lib.aclhip_database_stream_in(self._handle, database, tier, num_chunks, stream, ctypes.byref(moved)))
        return moved.value

    def database_stream_out(self, database, tier, num_chunks=0xFFFFFFFF, stream=None):
        moved = ctypes.c_uint32(0)
        self._check(self._lib.aclhip_database_stream_out(self._handle, database, tier, num_chunks, stream, ctypes.byref(moved)))
        return moved.value

    # ---- device pointer API (inputs and outputs resident in HBM) ----
    def decompress_tracks_batch(self, clips_ptr, times_ptr, num_instances, poses_ptr, pose_stride_bytes, params=None, stream=None):
        """seek + decompress_tracks for every instance. All pointers are device addresses (ints)."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_tracks_batch(self._handle, clips_ptr, times_ptr, num_instances, ctypes.byref(params), poses_ptr, pose_stride_bytes, stream))

    def decompress_tracks_batch_rows(self, clips_ptr, times_ptr, rows_ptr, num_instances, poses_ptr, pose_stride_bytes, params=None, stream=None):
        """aclhip_decompress_tracks_batch with the pose of instance i stored at row rows[i] (device array)."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_tracks_batch_rows(self._handle, clips_ptr, times_ptr, rows_ptr, num_instances, ctypes.byref(params), poses_ptr, pose_stride_bytes, stream))

    def decompress_tracks_batch_out(self, clips_ptr, times_ptr, num_instances, poses_ptr, pose_stride_bytes, output, params=None, stream=None):
        """aclhip_decompress_tracks_batch with an OutputDesc (layout, skipped sub-track kinds, rows)."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_tracks_batch_out(self._handle, clips_ptr, times_ptr, num_instances, ctypes.byref(params), ctypes.byref(output), poses_ptr, pose_stride_bytes, stream))

    # ---- track maps (track_writer::write_*(track_index, value): the writer chooses the destination) ----
    def register_track_map(self, track_to_slot, num_slots):
        """track_to_slot: host array, slot of every track or TRACK_DROPPED. Returns the map handle (>= 1)."""
        table = np.ascontiguousarray(track_to_slot, dtype=np.uint32)
        handle = ctypes.c_uint32(0)
        self._check(self._lib.aclhip_register_track_map(self._handle, table.ctypes.data, table.size, int(num_slots), ctypes.byref(handle)))
        return handle.value

    def unregister_track_map(self, track_map):
        self._check(self._lib.aclhip_unregister_track_map(self._handle, track_map))

    def track_map_info(self, track_map):
        info = TrackMapInfo()
        self._check(self._lib.aclhip_get_track_map_info(self._handle, track_map, ctypes.byref(info)))
        return info

    def decompress_tracks_batch_mapped(self, clips, sample_times, poses, pose_stride_bytes, track_map=0, instance_maps=None, fill_pose=None, output=None, params=None, stream=None):
        """aclhip_decompress_tracks_batch_mapped on torch tensors (device): clips int32/uint32 [n], sample_times float32 [n], poses the
        output buffer (rows pose_stride_bytes apart), instance_maps int32 [n] or None, fill_pose a tensor (unmapped slots are written from it) or None."""
        params = params if params is not None else default_params()
        mapping = TrackMapping()
        mapping.map = int(track_map)
        mapping.instance_maps = instance_maps.data_ptr() if instance_maps is not None else None
        mapping.fill_pose = fill_pose.data_ptr() if fill_pose is not None else None
        mapping.fill_unmapped = 1 if fill_pose is not None else 0
        self._check(self._lib.aclhip_decompress_tracks_batch_mapped(self._handle, clips.data_ptr(), sample_times.data_ptr(), int(clips.numel()), ctypes.byref(params),
                                                                   ctypes.byref(output) if output is not None else None, ctypes.byref(mapping), poses.data_ptr(), int(pose_stride_bytes), stream))

    def decompress_tracks_batch_mapped_at(self, clips_ptr, times_ptr, num_instances, poses_ptr, pose_stride_bytes, track_map=0, instance_maps_ptr=None,
                                          fill_pose_ptr=None, output=None, params=None, stream=None):
        """aclhip_decompress_tracks_batch_mapped on device ADDRESSES (ints), like decompress_tracks_batch"""
        params = params if params is not None else default_params()
        mapping = TrackMapping()
        mapping.map, mapping.instance_maps, mapping.fill_pose, mapping.fill_unmapped = int(track_map), instance_maps_ptr, fill_pose_ptr, 1 if fill_pose_ptr else 0
        self._check(self._lib.aclhip_decompress_tracks_batch_mapped(self._handle, clips_ptr, times_ptr, int(num_instances), ctypes.byref(params),
                                                                   ctypes.byref(output) if output is not None else None, ctypes.byref(mapping), poses_ptr, int(pose_stride_bytes), stream))

    # ---- skeletons: the pose consumers in skeleton space ----
    def register_skeleton(self, parent_indices, reference_pose, num_bones=None):
        """parent_indices: host array in slot order or None (local space only); reference_pose: float32 [num_bones, 12]. Returns the handle (>= 1)."""
        parents, pose, num_bones = _skeleton_arrays(parent_indices, reference_pose, num_bones)
        handle = ctypes.c_uint32(0)
        self._check(self._lib.aclhip_register_skeleton(self._handle, parents.ctypes.data if parents is not None else None, pose.ctypes.data if pose is not None else None,
                                                       num_bones, ctypes.byref(handle)))
        return handle.value

    def unregister_skeleton(self, skeleton):
        self._check(self._lib.aclhip_unregister_skeleton(self._handle, skeleton))

    def skeleton_info(self, skeleton):
        info = SkeletonInfo()
        self._check(self._lib.aclhip_get_skeleton_info(self._handle, skeleton, ctypes.byref(info)))
        return info

    def decompress_poses_batch_mapped(self, clips_ptr, times_ptr, num_instances, poses_ptr, pose_stride_bytes, consumers, mapping, params=None, stream=None):
        """aclhip_decompress_poses_batch_mapped; `consumers` (PoseConsumers) and `mapping` (PoseMapping) hold device addresses."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_poses_batch_mapped(self._handle, clips_ptr, times_ptr, num_instances, ctypes.byref(params), ctypes.byref(consumers),
                                                                  ctypes.byref(mapping) if mapping is not None else None, poses_ptr, pose_stride_bytes, stream))

    # ---- blend masks: a weight per bone for the blends of skeleton space ----
    def register_blend_mask(self, weights):
        """weights: host float32 [num_slots] in skeleton slot order, each in [0, 1]. Returns the mask handle (>= 1)."""
        table = np.ascontiguousarray(weights, dtype=np.float32)
        handle = ctypes.c_uint32(0)
        self._check(self._lib.aclhip_register_blend_mask(self._handle, table.ctypes.data, table.size, ctypes.byref(handle)))
        return handle.value

    def unregister_blend_mask(self, mask):
        self._check(self._lib.aclhip_unregister_blend_mask(self._handle, mask))

    def blend_mask_info(self, mask):
        info = BlendMaskInfo()
        self._check(self._lib.aclhip_get_blend_mask_info(self._handle, mask, ctypes.byref(info)))
        return info

    def decompress_poses_batch_masked(self, clips_ptr, times_ptr, num_instances, poses_ptr, pose_stride_bytes, consumers, mapping, masking, params=None, stream=None):
        """aclhip_decompress_poses_batch_masked; `consumers` (PoseConsumers), `mapping` (PoseMapping) and `masking` (BlendMasking) hold device addresses."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_poses_batch_masked(self._handle, clips_ptr, times_ptr, num_instances, ctypes.byref(params), ctypes.byref(consumers),
                                                                  ctypes.byref(mapping) if mapping is not None else None, ctypes.byref(masking) if masking is not None else None,
                                                                  poses_ptr, pose_stride_bytes, stream))

    def decompress_poses_batch_additive_weighted(self, clips_ptr, times_ptr, num_instances, poses_ptr, pose_stride_bytes, consumers, mapping, layering, params=None, stream=None):
        """aclhip_decompress_poses_batch_additive_weighted: the mapped launch with a strength per (instance, slot) on the additive pose;
        `consumers` (PoseConsumers), `mapping` (PoseMapping) and `layering` (AdditiveLayering) hold device addresses."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_poses_batch_additive_weighted(self._handle, clips_ptr, times_ptr, num_instances, ctypes.byref(params), ctypes.byref(consumers),
                                                                             ctypes.byref(mapping) if mapping is not None else None, ctypes.byref(layering) if layering is not None else None,
                                                                             poses_ptr, pose_stride_bytes, stream))

    def decompress_poses_batch_bounds(self, clips_ptr, times_ptr, num_instances, bounds, poses_ptr, pose_stride_bytes, consumers, mapping=None, masking=None,
                                      params=None, stream=None):
        """aclhip_decompress_poses_batch_bounds: the unmapped launch (mapping None), the mapped one, or the masked one (masking set too), in
        object space, with one box per instance into `bounds` (PoseBounds, device addresses: num_instances x 8 floats, min.xyz 0 | max.xyz 0).
        poses_ptr None: the boxes alone, no row is written."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_poses_batch_bounds(self._handle, clips_ptr, times_ptr, num_instances, ctypes.byref(params), ctypes.byref(consumers),
                                                                  ctypes.byref(mapping) if mapping is not None else None, ctypes.byref(masking) if masking is not None else None,
                                                                  ctypes.byref(bounds) if bounds is not None else None, poses_ptr, pose_stride_bytes, stream))

    def transform_poses_batch(self, local_poses_ptr, local_pose_stride_bytes, num_instances, consumers, poses_ptr, pose_stride_bytes, bounds=None, stream=None):
        """aclhip_transform_poses_batch: apply_additive_to_base and / or local_to_object_space over the caller's QVV48 rows (device addresses);
        poses_ptr == local_poses_ptr with equal strides: in place. `consumers` is a PoseBufferConsumers; `bounds` (a PoseBounds) is put into
        it for the call. poses_ptr None (with bounds): the boxes alone."""
        if bounds is not None:
            consumers.bounds = ctypes.addressof(bounds)
        self._check(self._lib.aclhip_transform_poses_batch(self._handle, local_poses_ptr, local_pose_stride_bytes, num_instances,
                                                           ctypes.byref(consumers) if consumers is not None else None, poses_ptr, pose_stride_bytes, stream))

    def blend_poses_batch(self, blend, num_instances, poses_ptr, pose_stride_bytes, bounds=None, stream=None):
        """aclhip_blend_poses_batch: the masked blend of the K QVV48 row buffers `blend` (a PoseBufferBlend, device addresses) names, in local
        or object space; poses_ptr equal to one of the buffers with its stride: in place. `bounds` (a PoseBounds) is put into the struct for
        the call. poses_ptr None (with bounds): the boxes alone."""
        if bounds is not None:
            blend.bounds = ctypes.addressof(bounds)
        self._check(self._lib.aclhip_blend_poses_batch(self._handle, ctypes.byref(blend) if blend is not None else None, num_instances, poses_ptr, pose_stride_bytes, stream))

    def inverse_transform_poses_batch(self, source_poses_ptr, source_pose_stride_bytes, num_instances, inverse, poses_ptr, pose_stride_bytes, stream=None):
        """aclhip_inverse_transform_poses_batch: object -> local space and / or convert_to_relative / additive0 / additive1 against a base
        buffer over the caller's QVV48 rows (device addresses); poses_ptr == source_poses_ptr with equal strides: in place. `inverse` is a
        PoseBufferInverse."""
        self._check(self._lib.aclhip_inverse_transform_poses_batch(self._handle, source_poses_ptr, source_pose_stride_bytes, num_instances,
                                                                   ctypes.byref(inverse) if inverse is not None else None, poses_ptr, pose_stride_bytes, stream))

    def measure_pose_error(self, raw_poses_ptr, raw_pose_stride_bytes, lossy_poses_ptr, lossy_pose_stride_bytes, num_instances, desc, errors_ptr, stream=None):
        """aclhip_measure_pose_error_batch: per instance the worst bone's shell error between two QVV48 pose buffers (device addresses) into
        the 8 byte records at errors_ptr; `desc` is a PoseErrorDesc (per bone errors and the launch's worst record on request)."""
        self._check(self._lib.aclhip_measure_pose_error_batch(self._handle, raw_poses_ptr, raw_pose_stride_bytes, lossy_poses_ptr, lossy_pose_stride_bytes, num_instances,
                                                              ctypes.byref(desc) if desc is not None else None, errors_ptr, stream))

    def measure_pose_error_metric(self, raw_poses_ptr, raw_pose_stride_bytes, lossy_poses_ptr, lossy_pose_stride_bytes, num_instances, desc, metric, errors_ptr, stream=None):
        """aclhip_measure_pose_error_metric_batch: measure_pose_error with the error metric as an argument -- ERROR_METRIC_QVVF is
        measure_pose_error itself, ERROR_METRIC_QVVF_MATRIX3X4F the reference's matrix metric (no additive format)."""
        self._check(self._lib.aclhip_measure_pose_error_metric_batch(self._handle, raw_poses_ptr, raw_pose_stride_bytes, lossy_poses_ptr, lossy_pose_stride_bytes,
                                                                     num_instances, ctypes.byref(desc) if desc is not None else None, metric, errors_ptr, stream))

    def pose_matrices_batch(self, local_poses_ptr, local_pose_stride_bytes, num_instances, desc, matrices_ptr, matrix_stride_bytes, stream=None):
        """aclhip_pose_matrices_batch: 3x4 matrices (64 bytes per bone) of the QVV48 rows at local_poses_ptr into the rows at matrices_ptr
        (device addresses), in local space or, with desc.object_space, through the matrix walk; `desc` is a PoseMatricesDesc."""
        self._check(self._lib.aclhip_pose_matrices_batch(self._handle, local_poses_ptr, local_pose_stride_bytes, num_instances,
                                                         ctypes.byref(desc) if desc is not None else None, matrices_ptr, matrix_stride_bytes, stream))

    # ---- skins: a mesh's joint list and inverse bind matrices, and the skinning palettes made with them ----
    def register_skin(self, joint_bones, inverse_bind, num_bones, num_joints=None):
        """joint_bones: host uint32 [num_joints], each < num_bones, or None (the identity list); inverse_bind: host float32 [num_joints, 4, 4]
        in the MATRIX_3X4F_64 layout, or None (identity matrices). Returns the skin handle (>= 1)."""
        joints, matrices, num_joints = _skin_arrays(joint_bones, inverse_bind, num_joints, num_bones)
        handle = ctypes.c_uint32(0)
        self._check(self._lib.aclhip_register_skin(self._handle, joints.ctypes.data if joints is not None else None, matrices.ctypes.data if matrices is not None else None,
                                                   num_joints, int(num_bones), ctypes.byref(handle)))
        return handle.value

    def unregister_skin(self, skin):
        self._check(self._lib.aclhip_unregister_skin(self._handle, skin))

    def skin_info(self, skin):
        info = SkinInfo()
        self._check(self._lib.aclhip_get_skin_info(self._handle, skin, ctypes.byref(info)))
        return info

    def skinning_matrices_batch(self, poses_ptr, pose_stride_bytes, num_instances, desc, palettes_ptr, palette_stride_bytes, stream=None):
        """aclhip_skinning_matrices_batch: per joint of desc's skin inverse_bind * object matrix of its bone, from the QVV48 rows at poses_ptr
        into the rows at palettes_ptr (device addresses), 64 or 48 bytes per joint by desc.layout; with desc.object_space the rows are local
        and go through the matrix walk. `desc` is a SkinningDesc."""
        self._check(self._lib.aclhip_skinning_matrices_batch(self._handle, poses_ptr, pose_stride_bytes, num_instances,
                                                             ctypes.byref(desc) if desc is not None else None, palettes_ptr, palette_stride_bytes, stream))

    # ---- raw track arrays: uncompressed clips (acl::track_array_qvvf) and their sample_tracks ----
    def register_raw_tracks(self, samples, sample_rate, looping_policy=LOOP_CLAMP):
        """samples: host float32 [num_samples, num_tracks, 12], QVV48 records, sample major (what the tests hand to ref_compress); the array
        is copied. looping_policy: LOOP_CLAMP or LOOP_WRAP. Returns the raw tracks handle (>= 1)."""
        array = _raw_samples(samples)
        handle = ctypes.c_uint32(0)
        self._check(self._lib.aclhip_register_raw_tracks(self._handle, array.ctypes.data, array.shape[1], array.shape[0], float(sample_rate), int(looping_policy),
                                                         ctypes.byref(handle)))
        return handle.value

    def unregister_raw_tracks(self, raw):
        self._check(self._lib.aclhip_unregister_raw_tracks(self._handle, raw))

    def raw_tracks_info(self, raw):
        info = RawTracksInfo()
        self._check(self._lib.aclhip_get_raw_tracks_info(self._handle, raw, ctypes.byref(info)))
        return info

    def sample_raw_tracks_batch(self, raws_ptr, times_ptr, num_instances, poses_ptr, pose_stride_bytes, desc=None, stream=None):
        """aclhip_sample_raw_tracks_batch: track_array_qvvf::sample_tracks of the raw track arrays named at raws_ptr (device uint32
        [num_instances]) at the times at times_ptr into QVV48 rows at poses_ptr (device addresses). `desc` is a RawSampleDesc or None
        (ROUND_NONE, row i)."""
        self._check(self._lib.aclhip_sample_raw_tracks_batch(self._handle, raws_ptr, times_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                             poses_ptr, pose_stride_bytes, stream))

    # ---- raw scalar track arrays: uncompressed curve sets (acl::track_array of float1f .. vector4f), sample_tracks / sample_track ----
    def register_raw_scalar_tracks(self, samples, track_type, sample_rate, looping_policy=LOOP_CLAMP):
        """samples: host float32 [num_samples, num_tracks, C] (or [num_samples, num_tracks] for float1f), sample major (what the tests hand to
        ref_scalar_compress); the array is copied. track_type: TRACK_FLOAT1F .. TRACK_VECTOR4F. Returns the raw scalar tracks handle (>= 1)."""
        array = _raw_scalar_samples(samples, track_type)
        handle = ctypes.c_uint32(0)
        self._check(self._lib.aclhip_register_raw_scalar_tracks(self._handle, array.ctypes.data, int(track_type), array.shape[1], array.shape[0], float(sample_rate),
                                                                int(looping_policy), ctypes.byref(handle)))
        return handle.value

    def unregister_raw_scalar_tracks(self, raw):
        self._check(self._lib.aclhip_unregister_raw_scalar_tracks(self._handle, raw))

    def raw_scalar_tracks_info(self, raw):
        info = RawScalarTracksInfo()
        self._check(self._lib.aclhip_get_raw_scalar_tracks_info(self._handle, raw, ctypes.byref(info)))
        return info

    def sample_raw_scalar_tracks_batch(self, raws_ptr, times_ptr, num_instances, values_ptr, stride_bytes, desc=None, stream=None):
        """aclhip_sample_raw_scalar_tracks_batch: track_array::sample_tracks of the raw scalar track arrays named at raws_ptr (device uint32
        [num_instances]) at the times at times_ptr into rows of T * C floats at values_ptr (device addresses). `desc` is a RawSampleDesc or
        None (ROUND_NONE, row i)."""
        self._check(self._lib.aclhip_sample_raw_scalar_tracks_batch(self._handle, raws_ptr, times_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                                    values_ptr, stride_bytes, stream))

    def sample_raw_scalar_track_batch(self, raws_ptr, times_ptr, tracks_ptr, num_instances, values_ptr, stride_bytes, desc=None, stream=None):
        """aclhip_sample_raw_scalar_track_batch: track_array::sample_track, C floats per request of the track at tracks_ptr (device uint32
        [num_instances])."""
        self._check(self._lib.aclhip_sample_raw_scalar_track_batch(self._handle, raws_ptr, times_ptr, tracks_ptr, num_instances,
                                                                   ctypes.byref(desc) if desc is not None else None, values_ptr, stride_bytes, stream))

    def measure_scalar_error(self, raw_values_ptr, raw_stride_bytes, lossy_values_ptr, lossy_stride_bytes, num_instances, desc, errors_ptr, stream=None):
        """aclhip_measure_scalar_error_batch: calculate_scalar_track_error between the rows of T * C floats at the two device addresses, into
        the 8 byte records at errors_ptr; `desc` is a ScalarErrorDesc (per track errors and the launch's worst record on request)."""
        self._check(self._lib.aclhip_measure_scalar_error_batch(self._handle, raw_values_ptr, raw_stride_bytes, lossy_values_ptr, lossy_stride_bytes, num_instances,
                                                                ctypes.byref(desc) if desc is not None else None, errors_ptr, stream))

    def compress_raw_scalar_tracks_batch(self, raws_ptr, num_instances, desc, blobs_ptr, blob_stride_bytes, results_ptr, stream=None):
        """aclhip_compress_raw_scalar_tracks_batch: compress_track_list of the raw scalar track arrays named at raws_ptr (device uint32
        [num_instances]) into the rows at blobs_ptr, one aclhip_compress_result per instance at results_ptr (device addresses); `desc` is
        a ScalarCompressDesc with its workspace."""
        self._check(self._lib.aclhip_compress_raw_scalar_tracks_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                                      blobs_ptr, blob_stride_bytes, results_ptr, stream))

    def compress_raw_tracks_batch(self, raws_ptr, num_instances, desc, blobs_ptr, blob_stride_bytes, results_ptr, stream=None):
        """aclhip_compress_raw_tracks_batch: compress_track_list with the reference's raw compression settings of the raw track arrays named
        at raws_ptr (device uint32 [num_instances]) into the rows at blobs_ptr, one aclhip_compress_result per instance at results_ptr
        (device addresses); `desc` is a TransformCompressDesc with its workspace."""
        self._check(self._lib.aclhip_compress_raw_tracks_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                               blobs_ptr, blob_stride_bytes, results_ptr, stream))

    def compress_tracks_metric_batch(self, raws_ptr, num_instances, desc, blobs_ptr, blob_stride_bytes, results_ptr, metric, stream=None):
        """aclhip_compress_tracks_metric_batch: compress_tracks_batch with the error metric of the vote and of the constant and default
        rotations as an argument -- ERROR_METRIC_QVVF is compress_tracks_batch itself, ERROR_METRIC_QVVF_MATRIX3X4F the reference's matrix
        metric."""
        self._check(self._lib.aclhip_compress_tracks_metric_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                                  blobs_ptr, blob_stride_bytes, results_ptr, int(metric) & 0xFFFFFFFF, stream))

    def compress_tracks_variable_metric_batch(self, raws_ptr, num_instances, desc, blobs_ptr, blob_stride_bytes, results_ptr, metric, stream=None):
        """aclhip_compress_tracks_variable_metric_batch: compress_tracks_variable_batch with the error metric of the vote and of the
        compaction of all three kinds as an argument."""
        self._check(self._lib.aclhip_compress_tracks_variable_metric_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                                           blobs_ptr, blob_stride_bytes, results_ptr, int(metric) & 0xFFFFFFFF, stream))

    def find_bit_rates_metric_batch(self, raws_ptr, num_instances, desc, bit_rates_ptr, instance_stride, segment_stride, results_ptr, metric, stream=None):
        """aclhip_find_bit_rates_metric_batch: find_bit_rates_batch with the error metric the search optimises as an argument."""
        self._check(self._lib.aclhip_find_bit_rates_metric_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                                 bit_rates_ptr, instance_stride, segment_stride, results_ptr, int(metric) & 0xFFFFFFFF, stream))

    def find_bit_rates_level_batch(self, raws_ptr, num_instances, desc, bit_rates_ptr, instance_stride, segment_stride, results_ptr, metric=ERROR_METRIC_QVVF, stream=None):
        """aclhip_find_bit_rates_level_batch: find_bit_rates_metric_batch at every level -- desc.level 0 to 4 or LEVEL_AUTOMATIC --; its
        workspace is find_bit_rates_level_workspace_bytes, and the second word of an instance's result is the level that was searched."""
        self._check(self._lib.aclhip_find_bit_rates_level_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                                bit_rates_ptr, instance_stride, segment_stride, results_ptr, int(metric) & 0xFFFFFFFF, stream))

    def compress_tracks_additive_batch(self, raws_ptr, num_instances, desc, blobs_ptr, blob_stride_bytes, results_ptr, additive_base, stream=None):
        """aclhip_compress_tracks_additive_batch: compress_tracks_batch for additive clips -- every decision taken after the clip has been
        applied onto its base; `additive_base` is an AdditiveBase (ADDITIVE_NONE: compress_tracks_batch itself)."""
        self._check(self._lib.aclhip_compress_tracks_additive_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                                    blobs_ptr, blob_stride_bytes, results_ptr, ctypes.byref(additive_base) if additive_base is not None else None, stream))

    def compress_tracks_variable_additive_batch(self, raws_ptr, num_instances, desc, blobs_ptr, blob_stride_bytes, results_ptr, additive_base, stream=None):
        """aclhip_compress_tracks_variable_additive_batch: compress_tracks_variable_batch for additive clips (compress_tracks_additive_batch)."""
        self._check(self._lib.aclhip_compress_tracks_variable_additive_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                                             blobs_ptr, blob_stride_bytes, results_ptr,
                                                                             ctypes.byref(additive_base) if additive_base is not None else None, stream))

    def find_bit_rates_additive_batch(self, raws_ptr, num_instances, desc, bit_rates_ptr, instance_stride, segment_stride, results_ptr, additive_base, stream=None):
        """aclhip_find_bit_rates_additive_batch: find_bit_rates_level_batch under the qvvf metric for additive clips: both errors of the
        search measured on the base. Its workspace is find_bit_rates_level_workspace_bytes."""
        self._check(self._lib.aclhip_find_bit_rates_additive_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                                   bit_rates_ptr, instance_stride, segment_stride, results_ptr,
                                                                   ctypes.byref(additive_base) if additive_base is not None else None, stream))

    def compress_tracks_batch(self, raws_ptr, num_instances, desc, blobs_ptr, blob_stride_bytes, results_ptr, stream=None):
        """aclhip_compress_tracks_batch: compress_track_list with quatf_full or quatf_drop_w_full rotations (the rigid shell, the looping vote,
        constant and default rotations by the error metric) of the raw track arrays named at raws_ptr (device uint32 [num_instances]) into
        the rows at blobs_ptr, one aclhip_compress_result per instance at results_ptr (device addresses); `desc` is a CompressTracksDesc
        with its workspace."""
        self._check(self._lib.aclhip_compress_tracks_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                           blobs_ptr, blob_stride_bytes, results_ptr, stream))

    def compress_tracks_variable_batch(self, raws_ptr, num_instances, desc, blobs_ptr, blob_stride_bytes, results_ptr, stream=None):
        """aclhip_compress_tracks_variable_batch: compress_track_list with quatf_drop_w_variable / vector3f_variable / vector3f_variable at the
        bit rates `desc` (a CompressVariableDesc with its workspace) names, of the raw track arrays named at raws_ptr (device uint32
        [num_instances]) into the rows at blobs_ptr, one aclhip_compress_result per instance at results_ptr (device addresses)."""
        self._check(self._lib.aclhip_compress_tracks_variable_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                                    blobs_ptr, blob_stride_bytes, results_ptr, stream))

    def find_bit_rates_batch(self, raws_ptr, num_instances, desc, bit_rates_ptr, instance_stride, segment_stride, results_ptr, stream=None):
        """aclhip_find_bit_rates_batch: find_optimal_bit_rates (levels lowest to medium) of the raw track arrays named at raws_ptr (device
        uint32 [num_instances]): the { rotation, translation, scale, 0 } entry of every (instance, segment, track) into the table at
        bit_rates_ptr with the two strides, in the layout aclhip_compress_tracks_variable_batch reads; one aclhip_compress_result (size 0)
        per instance at results_ptr (device addresses); `desc` is a FindBitRatesDesc with its workspace."""
        self._check(self._lib.aclhip_find_bit_rates_batch(self._handle, raws_ptr, num_instances, ctypes.byref(desc) if desc is not None else None,
                                                          bit_rates_ptr, instance_stride, segment_stride, results_ptr, stream))

    def decompress_poses_mapped(self, clips, sample_times, skeletons, maps, num_bones, additive_format=ADDITIVE_NONE, object_space=False, base_clips=None,
                                base_sample_times=None, base_maps=None, base_poses=None, params=None, out=None, instance_rounding=None, instance_looping=None,
                                blend_clips=None, blend_sample_times=None, blend_maps=None, blend_weights=None, flags=0):
        """Host arrays in, host poses out, like decompress_poses: float32 [n, num_bones, 12] in skeleton order. `skeletons` and `maps` are one
        handle or an array of n; blend_maps [n, K - 1] and base_maps [n] go with blend_clips and base_clips. The library has no host form of
        this launch: the arrays are staged through torch tensors on the context's device and the call is synchronous."""
        import torch
        device = torch.device("cuda", self.device_index)
        keep = []

        def upload(array, dtype):
            tensor = torch.from_numpy(np.ascontiguousarray(array, dtype=dtype).view(np.int32 if dtype == np.uint32 else dtype)).to(device)
            keep.append(tensor)
            return tensor.data_ptr()

        clips = np.ascontiguousarray(clips, dtype=np.uint32)
        n = clips.size
        if out is None:
            out = np.zeros((n, num_bones, 12), dtype=np.float32)
        params = params if params is not None else default_params()
        if instance_rounding is not None:
            params.instance_rounding_policies = upload(instance_rounding, np.uint8)
        if instance_looping is not None:
            params.instance_looping_policies = upload(instance_looping, np.uint8)
        consumers, mapping = PoseConsumers(), PoseMapping()
        consumers.additive_format = int(additive_format)
        consumers.object_space = 1 if object_space else 0
        consumers.flags = int(flags)
        if np.ndim(skeletons) == 0:
            mapping.skeleton = int(skeletons)
        else:
            mapping.instance_skeletons = upload(skeletons, np.uint32)
        if np.ndim(maps) == 0:
            mapping.map = int(maps)
        else:
            mapping.instance_maps = upload(maps, np.uint32)
        if base_clips is not None:
            consumers.base_clips = upload(base_clips, np.uint32)
            consumers.base_sample_times = upload(base_sample_times, np.float32)
            if base_maps is not None:
                mapping.base_maps = upload(base_maps, np.uint32)
        if base_poses is not None:
            base_poses = np.ascontiguousarray(base_poses, dtype=np.float32)
            consumers.base_poses = upload(base_poses, np.float32)
            consumers.base_pose_stride_bytes = base_poses.strides[0] if base_poses.ndim == 3 else num_bones * 48
        if blend_weights is not None:
            blend_weights = np.ascontiguousarray(blend_weights, dtype=np.float32).reshape(n, -1)
            consumers.num_blend_clips = blend_weights.shape[1]
            consumers.blend_clips = upload(blend_clips, np.uint32)
            consumers.blend_sample_times = upload(blend_sample_times, np.float32)
            consumers.blend_weights = upload(blend_weights, np.float32)
            if blend_maps is not None:
                mapping.blend_maps = upload(blend_maps, np.uint32)
        d_out = torch.from_numpy(out.reshape(n, -1)).to(device)
        stream = torch.cuda.current_stream(device)
        self.decompress_poses_batch_mapped(upload(clips, np.uint32), upload(sample_times, np.float32), n, d_out.data_ptr(), num_bones * 48, consumers, mapping,
                                           params=params, stream=stream.cuda_stream)
        stream.synchronize()
        out[...] = d_out.cpu().numpy().reshape(out.shape)
        return out

    def order_instances_for_locality(self, clips):
        """Host only: the permutation aclhip_order_instances_for_locality computes for the instance list `clips`."""
        clips = np.ascontiguousarray(clips, dtype=np.uint32)
        order = np.empty(clips.size, dtype=np.uint32)
        self._check(self._lib.aclhip_order_instances_for_locality(self._handle, clips.ctypes.data, clips.size, order.ctypes.data))
        return order

    def order_instances_device(self, clips_ptr, times_ptr, num_instances, order_ptr, out_clips_ptr=None, out_times_ptr=None, stream=None):
        """aclhip_order_instances_device: the locality order of a DEVICE instance list, stream ordered (device pointers)."""
        self._check(self._lib.aclhip_order_instances_device(self._handle, clips_ptr, times_ptr, num_instances, order_ptr, out_clips_ptr, out_times_ptr, stream))

    def order_instances_device_for_windows(self, windows_per_instance, clips_ptr, times_ptr, num_instances, order_ptr, out_clips_ptr=None, out_times_ptr=None, stream=None):
        """aclhip_order_instances_device_for_windows: the same for launches of `windows_per_instance` wavefronts per pose (pose_windows_of_launch)."""
        self._check(self._lib.aclhip_order_instances_device_for_windows(self._handle, windows_per_instance, clips_ptr, times_ptr, num_instances, order_ptr, out_clips_ptr, out_times_ptr, stream))

    def pose_windows_of_launch(self, pose_stride_bytes, layout=LAYOUT_QVV48):
        """Wavefronts per instance of a pose launch with rows of `pose_stride_bytes` and the clips registered now."""
        windows = ctypes.c_uint32(0)
        self._check(self._lib.aclhip_pose_windows_of_launch(self._handle, int(layout), int(pose_stride_bytes), ctypes.byref(windows)))
        return windows.value

    def decompress_track_batch(self, clips_ptr, times_ptr, tracks_ptr, num_instances, out_ptr, params=None, stream=None):
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_track_batch(self._handle, clips_ptr, times_ptr, tracks_ptr, num_instances, ctypes.byref(params), out_ptr, stream))

    def decompress_track_object_batch(self, clips_ptr, times_ptr, tracks_ptr, num_requests, out_ptr, params=None, stream=None):
        """aclhip_decompress_track_object_batch: one bone per request in OBJECT space (device pointers, 48 bytes per request)."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_track_object_batch(self._handle, clips_ptr, times_ptr, tracks_ptr, num_requests, ctypes.byref(params), out_ptr, stream))

    def decompress_bone_object_batch_mapped(self, clips_ptr, times_ptr, slots_ptr, num_requests, out_ptr, mapping, params=None, stream=None):
        """aclhip_decompress_bone_object_batch_mapped: one skeleton slot per request in object space; `mapping` (PoseMapping) holds device addresses."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_bone_object_batch_mapped(self._handle, clips_ptr, times_ptr, slots_ptr, num_requests, ctypes.byref(params),
                                                                         ctypes.byref(mapping), out_ptr, stream))

    def order_track_requests_device(self, clips_ptr, times_ptr, tracks_ptr, num_requests, order_ptr, out_clips_ptr=None, out_times_ptr=None, out_tracks_ptr=None,
                                    out_positions_ptr=None, stream=None):
        """aclhip_order_track_requests_device: the locality order of a DEVICE single track request list, stream ordered (device pointers)."""
        self._check(self._lib.aclhip_order_track_requests_device(self._handle, clips_ptr, times_ptr, tracks_ptr, num_requests, order_ptr, out_clips_ptr, out_times_ptr,
                                                                 out_tracks_ptr, out_positions_ptr, stream))

    def decompress_track_batch_rows(self, clips_ptr, times_ptr, tracks_ptr, rows_ptr, num_requests, out_ptr, params=None, stream=None):
        """aclhip_decompress_track_batch with the transform of request k stored at row rows[k] (device array)."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_track_batch_rows(self._handle, clips_ptr, times_ptr, tracks_ptr, rows_ptr, num_requests, ctypes.byref(params), out_ptr, stream))

    def time_decompress_tracks_batch(self, clips_ptr, times_ptr, num_instances, poses_ptr, pose_stride_bytes, repeats, params=None, stream=None):
        """Average device milliseconds per launch, HIP events recorded on `stream`."""
        params = params if params is not None else default_params()
        ms = ctypes.c_float(0.0)
        self._check(self._lib.aclhip_time_decompress_tracks_batch(self._handle, clips_ptr, times_ptr, num_instances, ctypes.byref(params), poses_ptr, pose_stride_bytes, stream, repeats, ctypes.byref(ms)))
        return ms.value

    # ---- pose consumers: additive apply and local -> object space fused into the decode ----
    def set_clip_hierarchy(self, clip, parent_indices):
        parents = np.ascontiguousarray(parent_indices, dtype=np.uint32)
        self._check(self._lib.aclhip_set_clip_hierarchy(self._handle, clip, parents.ctypes.data, parents.size))

    def decompress_poses_batch(self, clips_ptr, times_ptr, num_instances, poses_ptr, pose_stride_bytes, consumers, params=None, stream=None):
        """aclhip_decompress_poses_batch; `consumers` is a PoseConsumers holding device addresses."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_poses_batch(self._handle, clips_ptr, times_ptr, num_instances, ctypes.byref(params), ctypes.byref(consumers), poses_ptr, pose_stride_bytes, stream))

    def time_decompress_poses_batch(self, clips_ptr, times_ptr, num_instances, poses_ptr, pose_stride_bytes, consumers, repeats, params=None, stream=None):
        params = params if params is not None else default_params()
        ms = ctypes.c_float(0.0)
        self._check(self._lib.aclhip_time_decompress_poses_batch(self._handle, clips_ptr, times_ptr, num_instances, ctypes.byref(params), ctypes.byref(consumers), poses_ptr, pose_stride_bytes, stream, repeats, ctypes.byref(ms)))
        return ms.value

    def decompress_poses(self, clips, sample_times, additive_format=ADDITIVE_NONE, object_space=False, base_clips=None, base_sample_times=None, base_poses=None,
                         params=None, num_tracks=None, out=None, instance_rounding=None, blend_clips=None, blend_sample_times=None, blend_weights=None, flags=0):
        """Host arrays in, host poses out: float32 [n, num_tracks, 12] after the consumers. The base of an additive instance is either
        (base_clips[i], base_sample_times[i]) or base_poses[i] ([n, num_tracks, 12]). A blend of K clips per instance: blend_clips /
        blend_sample_times [n, K - 1] (the further clips), blend_weights [n, K]."""
        clips = np.ascontiguousarray(clips, dtype=np.uint32)
        sample_times = np.ascontiguousarray(sample_times, dtype=np.float32)
        n = clips.size
        if num_tracks is None:
            num_tracks = max((self.clip_info(int(c)).num_tracks for c in np.unique(clips)), default=0)
        if out is None:
            out = np.zeros((n, num_tracks, 12), dtype=np.float32)
        params = params if params is not None else default_params()
        if instance_rounding is not None:
            instance_rounding = np.ascontiguousarray(instance_rounding, dtype=np.uint8)
            params.instance_rounding_policies = instance_rounding.ctypes.data
        consumers = PoseConsumers()
        consumers.additive_format = int(additive_format)
        consumers.object_space = 1 if object_space else 0
        consumers.flags = int(flags)
        if base_clips is not None:
            base_clips = np.ascontiguousarray(base_clips, dtype=np.uint32)
            base_sample_times = np.ascontiguousarray(base_sample_times, dtype=np.float32)
            consumers.base_clips = base_clips.ctypes.data
            consumers.base_sample_times = base_sample_times.ctypes.data
        if base_poses is not None:
            base_poses = np.ascontiguousarray(base_poses, dtype=np.float32)
            consumers.base_poses = base_poses.ctypes.data
            consumers.base_pose_stride_bytes = base_poses.strides[0] if base_poses.ndim == 3 else num_tracks * 48
        if blend_weights is not None:
            blend_weights = np.ascontiguousarray(blend_weights, dtype=np.float32).reshape(n, -1)
            blend_clips = np.ascontiguousarray(blend_clips, dtype=np.uint32).reshape(n, -1)
            blend_sample_times = np.ascontiguousarray(blend_sample_times, dtype=np.float32).reshape(n, -1)
            consumers.num_blend_clips = blend_weights.shape[1]
            consumers.blend_clips = blend_clips.ctypes.data
            consumers.blend_sample_times = blend_sample_times.ctypes.data
            consumers.blend_weights = blend_weights.ctypes.data
        self._check(self._lib.aclhip_decompress_poses_host(self._handle, clips.ctypes.data, sample_times.ctypes.data, n, ctypes.byref(params), ctypes.byref(consumers), out.ctypes.data, num_tracks * 48))
        return out

    # ---- host pointer convenience API ----
    def decompress_tracks(self, clips, sample_times, params=None, num_tracks=None, out=None, default_values=None, track_rounding=None, instance_rounding=None):
        """Host arrays in, host poses out: returns float32 [n, num_tracks, 12]."""
        clips = np.ascontiguousarray(clips, dtype=np.uint32)
        sample_times = np.ascontiguousarray(sample_times, dtype=np.float32)
        n = clips.size
        if num_tracks is None:
            num_tracks = max((self.clip_info(int(c)).num_tracks for c in np.unique(clips)), default=0)
        if out is None:
            out = np.zeros((n, num_tracks, 12), dtype=np.float32)
        params = params if params is not None else default_params()
        count = 0
        if default_values is not None:
            default_values = np.ascontiguousarray(default_values, dtype=np.float32)
            params.default_values = default_values.ctypes.data
            count = default_values.size // 12
        if track_rounding is not None:
            track_rounding = np.ascontiguousarray(track_rounding, dtype=np.uint8)
            params.track_rounding_policies = track_rounding.ctypes.data
        if instance_rounding is not None:
            instance_rounding = np.ascontiguousarray(instance_rounding, dtype=np.uint8)
            params.instance_rounding_policies = instance_rounding.ctypes.data
        self._check(self._lib.aclhip_decompress_tracks_host(self._handle, clips.ctypes.data, sample_times.ctypes.data, n, ctypes.byref(params), count, out.ctypes.data, num_tracks * 48))
        return out

    def decompress_track(self, clips, sample_times, track_indices, params=None, out=None, default_values=None, track_rounding=None, instance_rounding=None):
        """Host arrays in, one qvv (12 floats) per instance out."""
        clips = np.ascontiguousarray(clips, dtype=np.uint32)
        sample_times = np.ascontiguousarray(sample_times, dtype=np.float32)
        track_indices = np.ascontiguousarray(track_indices, dtype=np.uint32)
        n = clips.size
        if out is None:
            out = np.zeros((n, 12), dtype=np.float32)
        params = params if params is not None else default_params()
        count = 0
        if default_values is not None:
            default_values = np.ascontiguousarray(default_values, dtype=np.float32)
            params.default_values = default_values.ctypes.data
            count = default_values.size // 12
        if track_rounding is not None:
            track_rounding = np.ascontiguousarray(track_rounding, dtype=np.uint8)
            params.track_rounding_policies = track_rounding.ctypes.data
        if instance_rounding is not None:
            instance_rounding = np.ascontiguousarray(instance_rounding, dtype=np.uint8)
            params.instance_rounding_policies = instance_rounding.ctypes.data
        self._check(self._lib.aclhip_decompress_track_host(self._handle, clips.ctypes.data, sample_times.ctypes.data, track_indices.ctypes.data, n, ctypes.byref(params), count, out.ctypes.data))
        return out

    # ---- scalar track lists (float1f .. vector4f) ----
    def decompress_scalar_tracks_batch(self, clips_ptr, times_ptr, num_instances, values_ptr, stride_bytes, params=None, stream=None):
        """seek + decompress_tracks of scalar track lists. All pointers are device addresses (ints)."""
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_scalar_tracks_batch(self._handle, clips_ptr, times_ptr, num_instances, ctypes.byref(params), values_ptr, stride_bytes, stream))

    def decompress_scalar_track_batch(self, clips_ptr, times_ptr, tracks_ptr, num_instances, values_ptr, stride_bytes, params=None, stream=None):
        params = params if params is not None else default_params()
        self._check(self._lib.aclhip_decompress_scalar_track_batch(self._handle, clips_ptr, times_ptr, tracks_ptr, num_instances, ctypes.byref(params), values_ptr, stride_bytes, stream))

    def _scalar_shape(self, clips):
        infos = [self.clip_info(int(c)) for c in np.unique(clips)]
        return max((i.num_tracks for i in infos), default=0), max((i.num_components for i in infos), default=1)

    def decompress_scalar_tracks(self, clips, sample_times, params=None, out=None, track_rounding=None, instance_rounding=None):
        """Host arrays in, host values out: float32 [n, max num_tracks, max num_components] (rows of clips with fewer components are packed tighter)."""
        clips = np.ascontiguousarray(clips, dtype=np.uint32)
        sample_times = np.ascontiguousarray(sample_times, dtype=np.float32)
        if out is None:
            num_tracks, num_components = self._scalar_shape(clips)
            out = np.zeros((clips.size, num_tracks, num_components), dtype=np.float32)
        params = params if params is not None else default_params()
        if track_rounding is not None:
            track_rounding = np.ascontiguousarray(track_rounding, dtype=np.uint8)
            params.track_rounding_policies = track_rounding.ctypes.data
        if instance_rounding is not None:
            instance_rounding = np.ascontiguousarray(instance_rounding, dtype=np.uint8)
            params.instance_rounding_policies = instance_rounding.ctypes.data
        stride = out.strides[0] if clips.size else 4
        self._check(self._lib.aclhip_decompress_scalar_tracks_host(self._handle, clips.ctypes.data, sample_times.ctypes.data, clips.size, ctypes.byref(params), out.ctypes.data, max(stride, 4)))
        return out

    def decompress_scalar_track(self, clips, sample_times, track_indices, params=None, out=None, track_rounding=None):
        clips = np.ascontiguousarray(clips, dtype=np.uint32)
        sample_times = np.ascontiguousarray(sample_times, dtype=np.float32)
        track_indices = np.ascontiguousarray(track_indices, dtype=np.uint32)
        if out is None:
            out = np.zeros((clips.size, self._scalar_shape(clips)[1]), dtype=np.float32)
        params = params if params is not None else default_params()
        if track_rounding is not None:
            track_rounding = np.ascontiguousarray(track_rounding, dtype=np.uint8)
            params.track_rounding_policies = track_rounding.ctypes.data
        self._check(self._lib.aclhip_decompress_scalar_track_host(self._handle, clips.ctypes.data, sample_times.ctypes.data, track_indices.ctypes.data, clips.size,
                                                                 ctypes.byref(params), out.ctypes.data, max(out.strides[0], 4) if clips.size else 4))
        return out

    def decompress_all_samples(self, clip, scratch_ptr, out_ptr, stride_bytes, params=None, stream=None):
        """convert_track_list's sampling loop: every sample of `clip`, nearest rounding. Device pointers; scratch = 8 * num_samples bytes."""
        self._check(self._lib.aclhip_decompress_all_samples(self._handle, clip, ctypes.byref(params) if params is not None else None, scratch_ptr, out_ptr, stride_bytes, stream))

    def all_gather_poses(self, rccl_comm, shard_ptr, all_ptr, shard_bytes, stream=None):
        """One RCCL all-gather of pose shards (rank order); `rccl_comm` is an ncclComm_t handle (int / c_void_p)."""
        self._check(self._lib.aclhip_all_gather_poses(self._handle, rccl_comm, shard_ptr, all_ptr, shard_bytes, stream))

    # ---- peer gather (aclhip_peer_*): one GPU collects every rank's shard over xGMI ----
    def peer_export_buffer(self, buffer_ptr):
        handle = (ctypes.c_uint8 * PEER_HANDLE_BYTES)()
        self._check(self._lib.aclhip_peer_export_buffer(self._handle, buffer_ptr, handle))
        return bytes(handle)

    def peer_open_buffer(self, handle):
        raw = (ctypes.c_uint8 * PEER_HANDLE_BYTES)(*handle)
        pointer = ctypes.c_void_p()
        self._check(self._lib.aclhip_peer_open_buffer(self._handle, raw, ctypes.byref(pointer)))
        return pointer.value

    def peer_close_buffer(self, buffer_ptr):
        self._check(self._lib.aclhip_peer_close_buffer(self._handle, buffer_ptr))

    def push_poses_to_peer(self, peer_ptr, offset_bytes, shard_ptr, shard_bytes, stream=None):
        self._check(self._lib.aclhip_push_poses_to_peer(self._handle, peer_ptr, offset_bytes, shard_ptr, shard_bytes, stream))

    def negative_scale_count(self):
        count = ctypes.c_uint64(0)
        self._check(self._lib.aclhip_get_negative_scale_count(self._handle, ctypes.byref(count)))
        return count.value

    def lifetime_stats(self):
        """aclhip_get_lifetime_stats as a dict"""
        values = (ctypes.c_uint64 * 8)()
        self._check(self._lib.aclhip_get_lifetime_stats(self._handle, values))
        names = ("registered", "unregistered", "recycled", "pending", "table_capacity", "table_is_virtual", "table_address", "launch_streams")
        return dict(zip(names, (int(v) for v in values)))

    def rejected_instance_count(self):
        count = ctypes.c_uint64(0)
        self._check(self._lib.aclhip_get_rejected_instance_count(self._handle, ctypes.byref(count)))
        return count.value

    def measure_write_bandwidth(self, buffer_ptr, size_bytes, repeats=20, stream=None):
        """GB/s of a plain 16 byte per lane store stream into the given device buffer."""
        gbps = ctypes.c_float(0.0)
        self._check(self._lib.aclhip_measure_write_bandwidth(self._handle, buffer_ptr, size_bytes, repeats, stream, ctypes.byref(gbps)))
        return gbps.value

    def measure_pose_store_bandwidth(self, poses_ptr, pose_stride_bytes, num_instances, num_tracks, repeats=20, stream=None):
        """(GB/s, waves per CU) of the pose batch's own store stream alone, best of 32 / 16 / 12 / 8 resident waves per CU"""
        gbps, waves = ctypes.c_float(0.0), ctypes.c_uint32(0)
        self._check(self._lib.aclhip_measure_pose_store_bandwidth(self._handle, ctypes.c_void_p(poses_ptr), ctypes.c_uint64(pose_stride_bytes), ctypes.c_uint32(num_instances),
                                                                  ctypes.c_uint32(num_tracks), ctypes.c_uint32(repeats), ctypes.c_void_p(stream), ctypes.byref(gbps), ctypes.byref(waves)))
        return gbps.value, waves.value

    def tracks_kernel_name(self, params=None, pose_stride_bytes=None, output=None):
        """Name of the kernel a pose launch takes: for rows as wide as the largest registered clip, or (pose_stride_bytes given) for the
        launch aclhip_decompress_tracks_batch_out makes with `output` and that stride."""
        params = params if params is not None else default_params()
        name = ctypes.create_string_buffer(128)
        if pose_stride_bytes is None and output is None:
            self._check(self._lib.aclhip_describe_tracks_kernel(self._handle, ctypes.byref(params), name, 128))
        else:
            stride = int(pose_stride_bytes) if pose_stride_bytes is not None else 0xFFFFFFFFFFFFFFFF
            self._check(self._lib.aclhip_describe_tracks_launch(self._handle, ctypes.byref(params), ctypes.byref(output) if output is not None else None, stride, name, 128, None))
        return name.value.decode()

    def batch_algorithmic_bytes(self, clips):
        clips = np.ascontiguousarray(clips, dtype=np.uint32)
        written, read = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.aclhip_batch_algorithmic_bytes(self._handle, clips.ctypes.data, clips.size, ctypes.byref(written), ctypes.byref(read)))
        return written.value, read.value


def clip_error(ctx, clip_a, clip_b, skeleton, shells, object_space=True, params_a=None, params_b=None, metric=ERROR_METRIC_QVVF):
    """acl::calculate_compression_error's loop (impl/track_error.impl.h:219-387) as three launches: both registered clips decoded at
    min(i / sample_rate, duration) for every sample i of clip_a -- instances are samples --, then aclhip_measure_pose_error_batch over the
    two buffers with the launch's worst record. clip_a plays the raw clip and clip_b the lossy one; both have the skeleton's bones as
    their tracks, in its order. `shells` is one shell distance for every bone or an array of one per bone. Returns (bone, error,
    sample_time) of the worst bone of the worst sample -- the lowest sample and bone among equals; (NO_BONE, -1.0, nan) when nothing could
    be measured. `metric` is an aclhip_error_metric: ERROR_METRIC_QVVF_MATRIX3X4F measures with the reference's matrix metric
    (aclhip_measure_pose_error_metric_batch); the default is aclhip_measure_pose_error_batch as before. Synchronous; the buffers are torch
    tensors on the context's device."""
    import torch
    device = torch.device("cuda", ctx.device_index)
    info = ctx.clip_info(clip_a)
    num_bones, num_samples = int(info.num_tracks), int(info.num_samples)
    sample_times = np.minimum(np.arange(num_samples, dtype=np.float32) / np.float32(info.sample_rate), np.float32(info.duration)).astype(np.float32)
    if num_samples == 0:
        return NO_BONE, -1.0, float("nan")
    stride = max(num_bones, 1) * 48
    d_times = torch.from_numpy(sample_times).to(device)
    d_poses = [torch.zeros((num_samples, stride // 4), dtype=torch.float32, device=device) for _ in range(2)]
    d_errors = torch.zeros((num_samples, 2), dtype=torch.int32, device=device)
    d_worst = torch.zeros(4, dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device)
    for clip, d_pose, params in ((clip_a, d_poses[0], params_a), (clip_b, d_poses[1], params_b)):
        d_clips = torch.full((num_samples,), int(clip), dtype=torch.int32, device=device)
        ctx.decompress_tracks_batch(d_clips.data_ptr(), d_times.data_ptr(), num_samples, d_pose.data_ptr(), stride, params=params, stream=stream.cuda_stream)
    desc = PoseErrorDesc()
    desc.skeleton, desc.object_space = int(skeleton), 1 if object_space else 0
    if np.ndim(shells) == 0:
        desc.shell_distance = float(shells)
    else:
        d_shells = torch.from_numpy(np.ascontiguousarray(shells, dtype=np.float32)).to(device)
        desc.shell_distances, desc.num_shell_distances = d_shells.data_ptr(), d_shells.numel()
    desc.worst = d_worst.data_ptr()
    if metric == ERROR_METRIC_QVVF:
        ctx.measure_pose_error(d_poses[0].data_ptr(), stride, d_poses[1].data_ptr(), stride, num_samples, desc, d_errors.data_ptr(), stream=stream.cuda_stream)
    else:
        ctx.measure_pose_error_metric(d_poses[0].data_ptr(), stride, d_poses[1].data_ptr(), stride, num_samples, desc, metric, d_errors.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    worst = d_worst.cpu().numpy().view(POSE_ERROR_WORST_DTYPE)[0]
    if int(worst["instance"]) == 0xFFFFFFFF:
        return NO_BONE, -1.0, float("nan")
    return int(worst["bone"]), float(worst["error"]), float(sample_times[int(worst["instance"])])


def raw_clip_error(ctx, raw, clip, skeleton, shells, object_space=True, params=None, metric=ERROR_METRIC_QVVF, additive_base=None, additive_format=ADDITIVE_NONE,
                   rounding=None):
    """acl::calculate_compression_error(allocator, raw_tracks, context, error_metric, additive_base_tracks) (impl/track_error.impl.h:581-689,
    loop :319-376) as launches: what a compression setting costs a clip. `raw` is a raw track array (register_raw_tracks) and `clip` its
    registered compressed form; the clip's tracks are the raw array's, in order, and the skeleton's bones. Instances are the raw array's
    samples: the array is sampled (aclhip_sample_raw_tracks_batch) and the clip decoded at min(i / rate, duration) with the array's rate
    and duration, both with `rounding` -- by default the reference's choice: ROUND_NONE when the clip has a database or stripped key
    frames, ROUND_NEAREST otherwise --, then the two buffers are measured with the launch's worst record. `additive_base` is another raw
    track array: it fills a base buffer at (t / duration) * its own duration (at 0 when it has one sample) and the measure applies both
    poses onto it with `additive_format`; the matrix metric takes no additive base (the measure refuses it). `params` are the decode's
    (its rounding policy is replaced). Returns (bone, error, sample_time) like clip_error. Synchronous."""
    import torch
    device = torch.device("cuda", ctx.device_index)
    info = ctx.raw_tracks_info(raw)
    num_bones, num_samples = int(info.num_tracks), int(info.num_samples)
    duration = np.float32(info.duration)
    sample_times = np.minimum(np.arange(num_samples, dtype=np.float32) / np.float32(info.sample_rate), duration).astype(np.float32)
    if rounding is None:
        clip_info = ctx.clip_info(clip)
        rounding = ROUND_NONE if clip_info.has_database or clip_info.has_stripped_keyframes else ROUND_NEAREST
    stride = num_bones * 48
    stream = torch.cuda.current_stream(device)
    d_times = torch.from_numpy(sample_times).to(device)
    d_raw, d_lossy = (torch.zeros((num_samples, stride // 4), dtype=torch.float32, device=device) for _ in range(2))
    d_errors = torch.zeros((num_samples, 2), dtype=torch.int32, device=device)
    d_worst = torch.zeros(4, dtype=torch.int32, device=device)

    sample_desc = RawSampleDesc()
    sample_desc.rounding_policy = int(rounding)
    d_raws = torch.full((num_samples,), int(raw), dtype=torch.int32, device=device)
    ctx.sample_raw_tracks_batch(d_raws.data_ptr(), d_times.data_ptr(), num_samples, d_raw.data_ptr(), stride, desc=sample_desc, stream=stream.cuda_stream)
    decode_params = DecompressParams.from_buffer_copy(params) if params is not None else default_params()
    decode_params.rounding_policy = int(rounding)
    d_clips = torch.full((num_samples,), int(clip), dtype=torch.int32, device=device)
    ctx.decompress_tracks_batch(d_clips.data_ptr(), d_times.data_ptr(), num_samples, d_lossy.data_ptr(), stride, params=decode_params, stream=stream.cuda_stream)

    desc = PoseErrorDesc()
    desc.skeleton, desc.object_space = int(skeleton), 1 if object_space else 0
    if additive_base is not None:
        base_info = ctx.raw_tracks_info(additive_base)
        if int(base_info.num_samples) > 1:
            with np.errstate(invalid="ignore", divide="ignore"):
                base_times = ((sample_times / duration) * np.float32(base_info.duration)).astype(np.float32)
            base_times[np.isnan(base_times)] = 0.0          # (a raw array of one sample: its duration is 0)
        else:
            base_times = np.zeros(num_samples, dtype=np.float32)
        base_stride = int(base_info.num_tracks) * 48
        d_base_times = torch.from_numpy(base_times).to(device)
        d_base = torch.zeros((num_samples, base_stride // 4), dtype=torch.float32, device=device)
        d_bases = torch.full((num_samples,), int(additive_base), dtype=torch.int32, device=device)
        ctx.sample_raw_tracks_batch(d_bases.data_ptr(), d_base_times.data_ptr(), num_samples, d_base.data_ptr(), base_stride, desc=sample_desc, stream=stream.cuda_stream)
        desc.additive_format, desc.base_poses, desc.base_pose_stride_bytes = int(additive_format), d_base.data_ptr(), base_stride
    if np.ndim(shells) == 0:
        desc.shell_distance = float(shells)
    else:
        d_shells = torch.from_numpy(np.ascontiguousarray(shells, dtype=np.float32)).to(device)
        desc.shell_distances, desc.num_shell_distances = d_shells.data_ptr(), d_shells.numel()
    desc.worst = d_worst.data_ptr()
    if metric == ERROR_METRIC_QVVF:
        ctx.measure_pose_error(d_raw.data_ptr(), stride, d_lossy.data_ptr(), stride, num_samples, desc, d_errors.data_ptr(), stream=stream.cuda_stream)
    else:
        ctx.measure_pose_error_metric(d_raw.data_ptr(), stride, d_lossy.data_ptr(), stride, num_samples, desc, metric, d_errors.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    worst = d_worst.cpu().numpy().view(POSE_ERROR_WORST_DTYPE)[0]
    if int(worst["instance"]) == 0xFFFFFFFF:
        return NO_BONE, -1.0, float("nan")
    return int(worst["bone"]), float(worst["error"]), float(sample_times[int(worst["instance"])])


def _worst_scalar_error(ctx, device, stream, d_raw, d_lossy, stride, num_samples, num_tracks, num_components, sample_times):
    """aclhip_measure_scalar_error_batch with the worst record over two filled value buffers: (track, error, sample_time)"""
    import torch
    d_errors = torch.zeros((num_samples, 2), dtype=torch.int32, device=device)
    d_worst = torch.zeros(4, dtype=torch.int32, device=device)
    desc = ScalarErrorDesc()
    desc.num_tracks, desc.num_components, desc.worst = num_tracks, num_components, d_worst.data_ptr()
    ctx.measure_scalar_error(d_raw.data_ptr(), stride, d_lossy.data_ptr(), stride, num_samples, desc, d_errors.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    worst = d_worst.cpu().numpy().view(TRACK_ERROR_WORST_DTYPE)[0]
    if int(worst["instance"]) == 0xFFFFFFFF:
        return NO_TRACK, -1.0, float("nan")
    return int(worst["track"]), float(worst["error"]), float(sample_times[int(worst["instance"])])


def raw_scalar_clip_error(ctx, raw, clip, rounding=None):
    """acl::calculate_compression_error(allocator, raw_tracks, context) (impl/track_error.impl.h:399-462) for scalar tracks as launches:
    what a precision setting costs a scalar clip. `raw` is a raw scalar track array (register_raw_scalar_tracks) and `clip` its registered
    compressed form. Instances are the raw array's samples at min(i / rate, duration) with the array's rate and duration: the array is
    sampled (aclhip_sample_raw_scalar_tracks_batch) and the clip decoded (aclhip_decompress_scalar_tracks_batch) with `rounding` -- by
    default the reference's choice: ROUND_NONE when the clip has a database or stripped key frames, ROUND_NEAREST otherwise --, then the
    two buffers are measured (aclhip_measure_scalar_error_batch) with the launch's worst record. Returns (track, error, sample_time): the
    lowest sample and track among equals; (NO_TRACK, -1.0, nan) when nothing could be measured. A clip whose track type or track count
    differs from the array's raises ValueError. Synchronous; the buffers are torch tensors on the context's device."""
    import torch
    device = torch.device("cuda", ctx.device_index)
    info, clip_info = ctx.raw_scalar_tracks_info(raw), ctx.clip_info(clip)
    if int(clip_info.track_type) != int(info.track_type) or int(clip_info.num_tracks) != int(info.num_tracks):
        raise ValueError(f"the clip holds {clip_info.num_tracks} tracks of type {clip_info.track_type}, the raw array {info.num_tracks} of type {info.track_type}")
    num_tracks, num_components, num_samples = int(info.num_tracks), int(info.num_components), int(info.num_samples)
    sample_times = np.minimum(np.arange(num_samples, dtype=np.float32) / np.float32(info.sample_rate), np.float32(info.duration)).astype(np.float32)
    if rounding is None:
        rounding = ROUND_NONE if clip_info.has_database or clip_info.has_stripped_keyframes else ROUND_NEAREST
    stride = num_tracks * num_components * 4
    stream = torch.cuda.current_stream(device)
    d_times = torch.from_numpy(sample_times).to(device)
    d_raw, d_lossy = (torch.zeros((num_samples, stride // 4), dtype=torch.float32, device=device) for _ in range(2))
    sample_desc = RawSampleDesc()
    sample_desc.rounding_policy = int(rounding)
    d_raws = torch.full((num_samples,), int(raw), dtype=torch.int32, device=device)
    ctx.sample_raw_scalar_tracks_batch(d_raws.data_ptr(), d_times.data_ptr(), num_samples, d_raw.data_ptr(), stride, desc=sample_desc, stream=stream.cuda_stream)
    decode_params = default_params()
    decode_params.rounding_policy = int(rounding)
    d_clips = torch.full((num_samples,), int(clip), dtype=torch.int32, device=device)
    ctx.decompress_scalar_tracks_batch(d_clips.data_ptr(), d_times.data_ptr(), num_samples, d_lossy.data_ptr(), stride, params=decode_params, stream=stream.cuda_stream)
    return _worst_scalar_error(ctx, device, stream, d_raw, d_lossy, stride, num_samples, num_tracks, num_components, sample_times)


def scalar_compress_bound(track_type, num_tracks, num_samples):
    """aclhip_scalar_compress_bound (host only): the bytes a blob of such an array can take, rounded up to 16; 0 for a track type that is no
    scalar type"""
    return int(load_library().aclhip_scalar_compress_bound(int(track_type), int(num_tracks), int(num_samples)))


def scalar_compress_workspace_bytes(num_instances, max_tracks):
    """aclhip_scalar_compress_workspace_bytes (host only)"""
    return int(load_library().aclhip_scalar_compress_workspace_bytes(int(num_instances), int(max_tracks)))


def _compress_batch(ctx, launch, handles, noun, stride, workspace_bytes, desc):
    """What compress_scalar_tracks, compress_raw_tracks and compress_tracks share: rows of `stride` bytes, the results and the workspace are allocated on the
    context's device, `launch` (the context's method) runs on the current stream and is waited for, and each result becomes a 16 byte
    aligned blob or the documented exception. `desc` comes filled in but for the workspace."""
    import torch
    from .synth import aligned_bytes
    device = torch.device("cuda", ctx.device_index)
    num_instances = len(handles)
    stream = torch.cuda.current_stream(device)
    d_raws = torch.from_numpy(handles.view(np.int32)).to(device)
    d_blobs = torch.zeros((num_instances, stride), dtype=torch.uint8, device=device)
    d_results = torch.zeros((num_instances, 2), dtype=torch.int32, device=device)
    d_workspace = torch.zeros(workspace_bytes + 16, dtype=torch.uint8, device=device)
    desc.workspace = d_workspace.data_ptr()
    launch(d_raws.data_ptr(), num_instances, desc, d_blobs.data_ptr(), stride, d_results.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    results = d_results.cpu().numpy().view(np.uint32).reshape(num_instances, 2)
    rows = d_blobs.cpu().numpy()
    blobs = []
    for i in range(num_instances):
        status, size = int(results[i, 0]), int(results[i, 1])
        if status == COMPRESS_NOT_FINITE:
            raise RuntimeError("Some samples are not finite")
        if status == COMPRESS_NOT_NORMALIZED:
            raise ValueError(f"instance {i} ({noun} {int(handles[i])}) holds a rotation that is not normalized (ACLHIP_COMPRESS_NOT_NORMALIZED)")
        if status != COMPRESS_OK:
            raise ValueError(f"instance {i} ({noun} {int(handles[i])}) was refused (ACLHIP_COMPRESS_REFUSED)")
        blob = aligned_bytes(size)
        blob[:] = rows[i, :size]
        blobs.append(blob)
    return blobs


def compress_scalar_tracks(ctx, raws, precision=1.0e-5, track_precisions=None, optimize_loops=False):
    """acl::compress_track_list for raw scalar track arrays as one launch: `raws` is a handle or a list of handles
    (register_raw_scalar_tracks; they may repeat and differ in type and shape), `precision` the tracks' precision (the reference's default)
    or `track_precisions` one per track, shared by the arrays. Rows are sized from aclhip_scalar_compress_bound, the workspace is allocated,
    the results and the blobs are copied back: returns a list of 16 byte aligned numpy uint8 blobs, byte for byte the reference's.
    aclhip_register_clip takes a host pointer, so a blob comes back before it is registered. Raises RuntimeError with the reference's
    message when a sample is not finite, ValueError when an instance is refused. Synchronous; the buffers are torch tensors on the
    context's device."""
    import torch
    handles = np.atleast_1d(np.asarray(raws, dtype=np.uint32))
    infos = [ctx.raw_scalar_tracks_info(int(handle)) for handle in handles]
    if len(handles) == 0:
        return []
    stride = max(scalar_compress_bound(info.track_type, info.num_tracks, info.num_samples) for info in infos)
    desc = ScalarCompressDesc()
    desc.precision = float(precision)
    desc.flags = COMPRESS_OPTIMIZE_LOOPS if optimize_loops else 0
    desc.max_tracks = max(int(info.num_tracks) for info in infos)
    if track_precisions is not None:        # (d_precisions: alive until the launch has run)
        d_precisions = torch.from_numpy(np.ascontiguousarray(track_precisions, dtype=np.float32)).to(torch.device("cuda", ctx.device_index))
        desc.track_precisions, desc.num_track_precisions = d_precisions.data_ptr(), d_precisions.numel()
    return _compress_batch(ctx, ctx.compress_raw_scalar_tracks_batch, handles, "raw scalar track array", stride,
                           scalar_compress_workspace_bytes(len(handles), desc.max_tracks), desc)


def transform_compress_bound(num_tracks, num_samples, flags=0):
    """aclhip_transform_compress_bound (host only): the bytes a blob of such an array can take with these ACLHIP_COMPRESS_* flags, rounded up to 16"""
    return int(load_library().aclhip_transform_compress_bound(int(num_tracks), int(num_samples), int(flags)))


def transform_compress_workspace_bytes(num_instances, max_tracks):
    """aclhip_transform_compress_workspace_bytes (host only)"""
    return int(load_library().aclhip_transform_compress_workspace_bytes(int(num_instances), int(max_tracks)))


def _upload_track_tables(ctx, default_pose, parents, track_precisions, track_shell_distances):
    """The four per-track tables a transform compress desc or a search desc names, on the context's device: a list of
    (field, tensor, tracks) for _set_track_tables; the tensors stay alive as long as the list does."""
    import torch
    tables = []
    for field, table, dtype, width in (("default_pose", default_pose, np.float32, 12), ("parent_indices", parents, np.uint32, 1),
                                       ("track_precisions", track_precisions, np.float32, 1), ("track_shell_distances", track_shell_distances, np.float32, 1)):
        if table is None:
            continue
        host = np.ascontiguousarray(table, dtype=dtype).reshape(-1, width)
        if tables and host.shape[0] != tables[0][2]:
            raise ValueError("default_pose, parents, track_precisions and track_shell_distances hold the same number of tracks")
        d_table = torch.from_numpy(host.view(np.int32) if dtype is np.uint32 else host).to(torch.device("cuda", ctx.device_index))
        tables.append((field, d_table, host.shape[0]))
    return tables


def _set_track_tables(desc, tables):
    for field, d_table, num_tracks in tables:
        setattr(desc, field, d_table.data_ptr())
        desc.num_table_tracks = num_tracks


def _compress_transform_tracks(ctx, launch, workspace_bytes, desc, raws, flags, default_pose, parents, precision, shell_distance, track_precisions, track_shell_distances,
                               bound=None, tables=None):
    """What compress_raw_tracks, compress_tracks and compress_tracks_variable share: `desc` (any of the three structs: the fields have one
    name in all) comes with its formats or rates and gets the flag word, max_tracks, the two settings and the four per-track tables,
    uploaded; `launch` is the context's method, `workspace_bytes` the size function of its workspace, `bound` that of a row
    (transform_compress_bound when None); `tables`: those four as _upload_track_tables left them, when a call before this one has
    uploaded them already."""
    handles = np.atleast_1d(np.asarray(raws, dtype=np.uint32))
    infos = [ctx.raw_tracks_info(int(handle)) for handle in handles]
    if len(handles) == 0:
        return []
    stride = max((bound or transform_compress_bound)(info.num_tracks, info.num_samples, flags) for info in infos)
    desc.flags, desc.max_tracks, desc.precision, desc.shell_distance = flags, max(int(info.num_tracks) for info in infos), float(precision), float(shell_distance)
    if tables is None:
        tables = _upload_track_tables(ctx, default_pose, parents, track_precisions, track_shell_distances)       # (kept alive until the launch has run)
    _set_track_tables(desc, tables)
    return _compress_batch(ctx, launch, handles, "raw track array", stride, workspace_bytes(len(handles), desc.max_tracks), desc)


def compress_raw_tracks(ctx, raws, default_pose=None, parents=None, precision=1.0e-4, shell_distance=1.0, track_precisions=None, track_shell_distances=None,
                        include_parent_track_indices=False, include_track_descriptions=False):
    """acl::compress_track_list with the reference's raw compression settings (quatf_full, vector3f_full, vector3f_full) for raw track
    arrays as one launch: `raws` is a handle or a list of handles (register_raw_tracks; they may repeat and differ in shape). default_pose
    float32 [tracks, 12] (QVV48; None: the identity), parents uint32 [tracks] (NO_PARENT for a root; None: every track a root),
    track_precisions and track_shell_distances float32 [tracks] are shared by the arrays and hold at least as many tracks as the largest;
    parents, precisions and shell distances only reach the optional metadata. Rows are sized from aclhip_transform_compress_bound, the
    workspace is allocated, the results and the blobs are copied back: returns a list of 16 byte aligned numpy uint8 blobs, byte for
    byte the reference's and lossless. Raises RuntimeError with the reference's message when a sample is not finite, ValueError when a
    rotation is not normalized (ACLHIP_COMPRESS_NOT_NORMALIZED) or an instance is refused. Synchronous; the buffers are torch tensors on
    the context's device."""
    flags = (COMPRESS_INCLUDE_PARENT_TRACK_INDICES if include_parent_track_indices else 0) | (COMPRESS_INCLUDE_TRACK_DESCRIPTIONS if include_track_descriptions else 0)
    return _compress_transform_tracks(ctx, ctx.compress_raw_tracks_batch, transform_compress_workspace_bytes, TransformCompressDesc(), raws, flags, default_pose, parents,
                                      precision, shell_distance, track_precisions, track_shell_distances)


def compress_tracks_workspace_bytes(num_instances, max_tracks):
    """aclhip_compress_tracks_workspace_bytes (host only)"""
    return int(load_library().aclhip_compress_tracks_workspace_bytes(int(num_instances), int(max_tracks)))


def compress_tracks(ctx, raws, rotation_format=ROTATION_QUATF_DROP_W_FULL, default_pose=None, parents=None, precision=1.0e-4, shell_distance=1.0, track_precisions=None,
                    track_shell_distances=None, optimize_loops=False, include_parent_track_indices=False, include_track_descriptions=False, metric=ERROR_METRIC_QVVF,
                    additive_base=None, additive_format=ADDITIVE_NONE):
    """acl::compress_track_list with quatf_drop_w_full (or quatf_full) rotations and vector3f_full translations and scales for raw track
    arrays as one launch, like compress_raw_tracks: `raws` is a handle or a list of handles. With quatf_drop_w_full the parents, precisions
    and shell distances make the rigid shell at which constant and default rotations and the looping vote (optimize_loops) are decided;
    every parent index is smaller than its child's. Rows are sized from aclhip_transform_compress_bound. Returns a list of 16 byte
    aligned numpy uint8 blobs. `metric` is an aclhip_error_metric: ERROR_METRIC_QVVF_MATRIX3X4F decides the vote and the rotations with
    the reference's matrix metric (quatf_full uses none). `additive_base` (a raw track array's handle, or one per instance) and
    `additive_format` (ADDITIVE_RELATIVE, _ADDITIVE0, _ADDITIVE1) compress an additive clip against its base
    (aclhip_compress_tracks_additive_batch): every decision is taken on the clip applied onto the base. Raises RuntimeError with the reference's message when a sample is not finite
    (a zero quaternion included), ValueError when an instance is refused. Synchronous; the buffers are torch tensors on the context's device."""
    flags = ((COMPRESS_OPTIMIZE_LOOPS if optimize_loops else 0) | (COMPRESS_INCLUDE_PARENT_TRACK_INDICES if include_parent_track_indices else 0)
             | (COMPRESS_INCLUDE_TRACK_DESCRIPTIONS if include_track_descriptions else 0))
    desc = CompressTracksDesc()
    desc.rotation_format, desc.translation_format, desc.scale_format = int(rotation_format), VECTOR_VECTOR3F_FULL, VECTOR_VECTOR3F_FULL
    handles = np.atleast_1d(np.asarray(raws, dtype=np.uint32))
    launch, workspace_bytes, _, alive = transform_compress_route(ctx, "tracks", handles, metric, None, additive_base, additive_format)     # (alive until the launch has run)
    return _compress_transform_tracks(ctx, launch, workspace_bytes, desc, raws, flags, default_pose, parents, precision, shell_distance, track_precisions, track_shell_distances)


def variable_compress_num_segments(num_samples):
    """aclhip_variable_compress_num_segments (host only): the segments of an array of that many samples"""
    return int(load_library().aclhip_variable_compress_num_segments(int(num_samples)))


def variable_compress_bound(num_tracks, num_samples, flags=0):
    """aclhip_variable_compress_bound (host only): the bytes a variable blob of such an array can take with any rate table, rounded up to 16"""
    return int(load_library().aclhip_variable_compress_bound(int(num_tracks), int(num_samples), int(flags)))


def compress_variable_workspace_bytes(num_instances, max_tracks, max_samples):
    """aclhip_compress_variable_workspace_bytes (host only)"""
    return int(load_library().aclhip_compress_variable_workspace_bytes(int(num_instances), int(max_tracks), int(max_samples)))


def find_bit_rates_workspace_bytes(num_instances, max_tracks, max_samples):
    """aclhip_find_bit_rates_workspace_bytes (host only)"""
    return int(load_library().aclhip_find_bit_rates_workspace_bytes(int(num_instances), int(max_tracks), int(max_samples)))


def find_bit_rates_level_workspace_bytes(num_instances, max_tracks, max_samples):
    """aclhip_find_bit_rates_level_workspace_bytes (host only)"""
    return int(load_library().aclhip_find_bit_rates_level_workspace_bytes(int(num_instances), int(max_tracks), int(max_samples)))


# per call of the transform compressor family: the Context method without a front, and the size function of its workspace
_TRANSFORM_COMPRESS_CALLS = {"tracks": ("compress_tracks", compress_tracks_workspace_bytes), "variable": ("compress_tracks_variable", compress_variable_workspace_bytes),
                             "search": ("find_bit_rates", find_bit_rates_workspace_bytes)}


def transform_compress_route(ctx, call, handles, metric=ERROR_METRIC_QVVF, level=None, additive_base=None, additive_format=ADDITIVE_NONE, device=None):
    """The entry point one call of the transform compressor family goes through. `call` is "tracks" (compress_tracks_batch),
    "variable" (compress_tracks_variable_batch) or "search" (find_bit_rates_batch), `handles` the instances' raw track arrays; `level`
    (a name of COMPRESSION_LEVELS or its number) counts for the search alone. Returns (launch, workspace_bytes, with_levels, alive):
    the context's method with its extra argument bound, the size function of its workspace, whether the second word of a result is
    the level that was searched, and what must stay alive until the launch has run.
      tracks, variable: without a base the method itself for ERROR_METRIC_QVVF (it is that call), else the _metric method at `metric`
        (an unknown one is the library's to refuse).
      search: without a base, at a level above medium find_bit_rates_level_batch at `metric`; else find_bit_rates_batch for
        ERROR_METRIC_QVVF, else find_bit_rates_metric_batch.
      With additive_base (a handle for every instance, or one per instance) or an additive_format other than ADDITIVE_NONE: the _additive
        method with an AdditiveBase whose handles are uploaded here, to `device` (None: the context's); for the search that is the
        level search at every level. ValueError with another metric than ERROR_METRIC_QVVF, or a count of bases that is neither.
    find_bit_rates_level_batch and find_bit_rates_additive_batch have with_levels and find_bit_rates_level_workspace_bytes."""
    stem, workspace_bytes = _TRANSFORM_COMPRESS_CALLS[call]
    front, extra, alive = "", {}, None
    if additive_base is not None or additive_format != ADDITIVE_NONE:
        if metric != ERROR_METRIC_QVVF:
            raise ValueError("an additive base goes with the qvvf error metric: the reference has no additive matrix metric")
        import torch
        record = AdditiveBase()
        record.additive_format = int(additive_format) & 0xFFFFFFFF
        d_bases = None
        if additive_base is not None:
            bases = np.atleast_1d(np.asarray(additive_base, dtype=np.uint32))
            if len(bases) == 1:
                bases = np.repeat(bases, len(handles))
            if len(bases) != len(handles):
                raise ValueError(f"{len(bases)} additive bases for {len(handles)} instances: one handle, or one per instance")
            d_bases = torch.from_numpy(np.ascontiguousarray(bases).view(np.int32)).to(torch.device("cuda", ctx.device_index) if device is None else device)
            record.base_raws = d_bases.data_ptr()
        front, extra, alive = "_additive", {"additive_base": record}, (record, d_bases)
    elif call == "search" and COMPRESSION_LEVELS.get(level, level) > COMPRESSION_LEVELS["medium"]:
        front, extra = "_level", {"metric": metric}
    elif metric != ERROR_METRIC_QVVF:
        front, extra = "_metric", {"metric": metric}
    with_levels = call == "search" and front in ("_level", "_additive")
    return (functools.partial(getattr(ctx, stem + front + "_batch"), **extra), find_bit_rates_level_workspace_bytes if with_levels else workspace_bytes,
            with_levels, alive)


def _find_bit_rates(ctx, handles, infos, level, flags, default_pose, parents, precision, shell_distance, track_precisions, track_shell_distances, tables=None,
                    metric=ERROR_METRIC_QVVF, additive_base=None, additive_format=ADDITIVE_NONE):
    """The search over `handles` into a zero-filled device table uint8 [instances, segments, tracks, 4] of the largest array's segments
    and tracks: (the table, still on the device, the results as a host array [instances, 2], and the level that was searched per
    instance as a uint32 array). The entry point is transform_compress_route's; the calls without the levels leave 0 in a result's
    second word: their one search is the level they were asked for. Synchronous."""
    import torch
    device = torch.device("cuda", ctx.device_index)
    desc = FindBitRatesDesc()
    if level not in COMPRESSION_LEVELS and level not in COMPRESSION_LEVELS.values():
        raise ValueError(f"a compression level of {level!r}: one of {sorted(COMPRESSION_LEVELS, key=COMPRESSION_LEVELS.get)}, 0 to 4 or {LEVEL_AUTOMATIC}")
    desc.level = COMPRESSION_LEVELS.get(level, level)
    desc.flags, desc.precision, desc.shell_distance = flags, float(precision), float(shell_distance)
    desc.max_tracks = max(int(info.num_tracks) for info in infos)
    desc.max_samples = max(int(info.num_samples) for info in infos)
    if tables is None:
        tables = _upload_track_tables(ctx, default_pose, parents, track_precisions, track_shell_distances)       # (kept alive until the launch has run)
    _set_track_tables(desc, tables)
    num_instances, num_segments = len(handles), variable_compress_num_segments(desc.max_samples)
    stream = torch.cuda.current_stream(device)
    d_raws = torch.from_numpy(handles.view(np.int32)).to(device)
    d_rates = torch.zeros((num_instances, num_segments, desc.max_tracks, 4), dtype=torch.uint8, device=device)
    d_results = torch.zeros((num_instances, 2), dtype=torch.int32, device=device)
    launch, workspace_bytes, with_levels, alive = transform_compress_route(ctx, "search", handles, metric, desc.level, additive_base, additive_format)
    d_workspace = torch.zeros(workspace_bytes(num_instances, desc.max_tracks, desc.max_samples) + 16, dtype=torch.uint8, device=device)
    desc.workspace = d_workspace.data_ptr()
    launch(d_raws.data_ptr(), num_instances, desc, d_rates.data_ptr(), num_segments * desc.max_tracks * 4, desc.max_tracks * 4, d_results.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    del alive
    results = d_results.cpu().numpy().view(np.uint32).reshape(num_instances, 2)
    return d_rates, results, results[:, 1].copy() if with_levels else np.full(num_instances, desc.level, dtype=np.uint32)


def find_bit_rates(ctx, raws, level="medium", default_pose=None, parents=None, precision=1.0e-4, shell_distance=1.0, track_precisions=None, track_shell_distances=None,
                   optimize_loops=False, metric=ERROR_METRIC_QVVF, return_levels=False, additive_base=None, additive_format=ADDITIVE_NONE):
    """acl::find_optimal_bit_rates -- the bit rate search of compress_track_list with quatf_drop_w_variable / vector3f_variable /
    vector3f_variable at `level`: "lowest", "low" and "medium" (one search), "high", "highest", or "automatic", the reference's default,
    which picks one of the last three per array (medium above 500 samples, else by the longest bone chain) -- for raw track arrays as
    one launch. With return_levels the result is (the table, the level that was searched per instance as a uint32 array). `raws` is a handle
    or a list of handles; the settings are compress_tracks_variable's. Returns a uint8 array [instances, segments, tracks, 4] of
    { rotation, translation, scale, 0 } entries over the segments and tracks of the largest array, zero-filled before the launch: 255
    marks a constant or default sub-track, rows and entries an instance does not have stay 0. It is the table compress_tracks_variable
    takes. `metric` is the aclhip_error_metric the search optimises: ERROR_METRIC_QVVF_MATRIX3X4F is the reference's matrix metric, what
    clip_error and raw_clip_error measure with metric=1. `additive_base` (a handle, or one per instance) and `additive_format` search
    for an additive clip against its base (aclhip_find_bit_rates_additive_batch): both errors are measured on the clip applied onto the
    base, what raw_clip_error(additive_base=, additive_format=) measures. Raises RuntimeError with the reference's message when a sample
    is not finite, ValueError when an instance is refused. Synchronous; the buffers are torch tensors on the context's device."""
    handles = np.atleast_1d(np.asarray(raws, dtype=np.uint32))
    infos = [ctx.raw_tracks_info(int(handle)) for handle in handles]
    if len(handles) == 0:
        return np.zeros((0, 0, 0, 4), dtype=np.uint8)
    d_rates, results, levels = _find_bit_rates(ctx, handles, infos, level, COMPRESS_OPTIMIZE_LOOPS if optimize_loops else 0, default_pose, parents, precision, shell_distance,
                                               track_precisions, track_shell_distances, metric=metric, additive_base=additive_base, additive_format=additive_format)
    _raise_for_search_results(handles, results)
    return (d_rates.cpu().numpy(), levels) if return_levels else d_rates.cpu().numpy()


def _raise_for_search_results(handles, results):
    for i in range(len(handles)):
        if int(results[i, 0]) == COMPRESS_NOT_FINITE:
            raise RuntimeError("Some samples are not finite")
        if int(results[i, 0]) != COMPRESS_OK:
            raise ValueError(f"instance {i} (raw track array {int(handles[i])}) was refused (ACLHIP_COMPRESS_REFUSED)")


def compress_tracks_variable(ctx, raws, bit_rates=(16, 16, 16), default_pose=None, parents=None, precision=1.0e-4, shell_distance=1.0, track_precisions=None,
                             track_shell_distances=None, optimize_loops=False, include_parent_track_indices=False, include_track_descriptions=False, level="medium",
                             metric=ERROR_METRIC_QVVF, return_levels=False, additive_base=None, additive_format=ADDITIVE_NONE):
    """acl::compress_track_list with quatf_drop_w_variable rotations and vector3f_variable translations and scales AT GIVEN BIT RATES for
    raw track arrays as one launch, like compress_tracks: `raws` is a handle or a list of handles. bit_rates is three uniform rates
    (rotation, translation, scale: 0 .. 24), or a uint8 table of { rotation, translation, scale, 0 } entries: [tracks, 4] shared by every
    instance and segment, [segments, tracks, 4] shared by the instances, or [instances, segments, tracks, 4]; it covers
    variable_compress_num_segments(samples) rows and the tracks of the largest array. bit_rates="search" runs find_bit_rates at `level`
    with the same settings first and compresses at its table, which stays on the device: the reference's compress_track_list at
    that level ("automatic" is its default); with return_levels the result is (the blobs, the level that was searched per instance). `metric` is the aclhip_error_metric of the vote, the compaction and the search (find_bit_rates). Rows are
    sized from aclhip_variable_compress_bound. `additive_base` (a handle, or one per instance) and `additive_format` compress an additive
    clip against its base (aclhip_compress_tracks_variable_additive_batch); with bit_rates="search" both steps get the base.
    Returns a list of 16 byte aligned numpy uint8 blobs in the format the fast decode paths read. Raises RuntimeError with the
    reference's message when a sample is not finite, ValueError when an instance is refused (a rate above 24, a rate of 0 in a blob of
    one segment included). Synchronous; the buffers are torch tensors on the context's device."""
    import torch
    flags = ((COMPRESS_OPTIMIZE_LOOPS if optimize_loops else 0) | (COMPRESS_INCLUDE_PARENT_TRACK_INDICES if include_parent_track_indices else 0)
             | (COMPRESS_INCLUDE_TRACK_DESCRIPTIONS if include_track_descriptions else 0))
    if return_levels and not isinstance(bit_rates, str):
        raise ValueError('return_levels goes with bit_rates="search"')
    handles = np.atleast_1d(np.asarray(raws, dtype=np.uint32))
    infos = [ctx.raw_tracks_info(int(handle)) for handle in handles]
    if len(handles) == 0:
        return ([], np.zeros(0, dtype=np.uint32)) if return_levels else []
    desc = CompressVariableDesc()
    desc.max_samples = max(int(info.num_samples) for info in infos)
    tables = None
    if isinstance(bit_rates, str):
        if bit_rates != "search":
            raise ValueError('bit_rates is three rates, a table or "search"')
        tables = _upload_track_tables(ctx, default_pose, parents, track_precisions, track_shell_distances)         # (once, for both calls)
        d_rates, results, levels = _find_bit_rates(ctx, handles, infos, level, flags, default_pose, parents, precision, shell_distance, track_precisions, track_shell_distances,
                                                   tables, metric=metric, additive_base=additive_base, additive_format=additive_format)
        _raise_for_search_results(handles, results)
        desc.bit_rates = d_rates.data_ptr()                                                 # (alive until the launch has run)
        desc.bit_rate_segment_stride = d_rates.shape[2] * 4
        desc.bit_rate_instance_stride = d_rates.shape[1] * d_rates.shape[2] * 4
    else:
        rates = np.asarray(bit_rates, dtype=np.uint8)
        if rates.ndim == 1:
            if rates.shape[0] != 3:
                raise ValueError("uniform bit rates are three: rotation, translation, scale")
            desc.rotation_bit_rate, desc.translation_bit_rate, desc.scale_bit_rate = (int(rate) for rate in rates)
        else:
            if rates.shape[-1] != 4:
                raise ValueError("a bit rate table holds { rotation, translation, scale, 0 } per track")
            rates = np.ascontiguousarray(rates)
            d_rates = torch.from_numpy(rates).to(torch.device("cuda", ctx.device_index))        # (alive until the launch has run)
            desc.bit_rates = d_rates.data_ptr()
            desc.bit_rate_segment_stride = rates.shape[-2] * 4 if rates.ndim >= 3 else 0
            desc.bit_rate_instance_stride = rates.shape[-3] * rates.shape[-2] * 4 if rates.ndim == 4 else 0

    launch, size_function, _, alive = transform_compress_route(ctx, "variable", handles, metric, None, additive_base, additive_format)      # (alive until the launch has run)

    def workspace_bytes(num_instances, max_tracks):
        return size_function(num_instances, max_tracks, desc.max_samples)
    blobs = _compress_transform_tracks(ctx, launch, workspace_bytes, desc, raws, flags, default_pose, parents, precision, shell_distance,
                                       track_precisions, track_shell_distances, bound=variable_compress_bound, tables=tables)
    return (blobs, levels) if return_levels else blobs


def compress_tracks_at_precision(ctx, raw, skeleton, shells, precision, parents=None, default_pose=None, shell_distance=1.0, optimize_loops=False,
                                 metric=ERROR_METRIC_QVVF, **error_settings):
    """For ONE raw track array: the smallest uniform bit rate whose blob is within `precision` of the array by raw_clip_error(ctx, raw, clip,
    skeleton, shells, **error_settings). Scans the rate from 1 upward -- compress_tracks_variable, register, raw_clip_error, unregister --
    and returns (blob, rate) of the first rate whose error is at most `precision`; when rate 24 fails too, the drop-w full blob of
    compress_tracks with rate None. A host loop over existing launches, up to 24 of each: NOT the reference's search
    (find_optimal_bit_rates chooses a rate per sub-track and segment and walks the hierarchy); it is here so that a blob of the fast
    format at a stated error can be had today. `metric` is the aclhip_error_metric of both the compressors' decisions and the measure."""
    settings = {"default_pose": default_pose, "parents": parents, "precision": precision, "shell_distance": shell_distance, "optimize_loops": optimize_loops,
                "metric": metric}
    for rate in range(1, 25):
        blob = compress_tracks_variable(ctx, raw, bit_rates=(rate, rate, rate), **settings)[0]
        clip = ctx.register_clip(blob)
        try:
            _, error, _ = raw_clip_error(ctx, raw, clip, skeleton, shells, metric=metric, **error_settings)
        finally:
            ctx.unregister_clip(clip)
        if error <= precision:
            return blob, rate
    return compress_tracks(ctx, raw, **settings)[0], None


def scalar_clip_error(ctx, clip_a, clip_b):
    """The two-context overload (impl/track_error.impl.h:692-750) for scalar tracks, as clip_error is for transforms: both registered scalar
    clips decoded at min(i / sample_rate, duration) for every sample i of clip_a with ROUND_NEAREST, then measured. clip_a plays the raw
    clip. Returns (track, error, sample_time) like raw_scalar_clip_error; clips of different track types or counts raise ValueError."""
    import torch
    device = torch.device("cuda", ctx.device_index)
    info, info_b = ctx.clip_info(clip_a), ctx.clip_info(clip_b)
    if int(info.track_type) == TRACK_QVVF or int(info.track_type) != int(info_b.track_type) or int(info.num_tracks) != int(info_b.num_tracks):
        raise ValueError(f"two scalar clips of one track type and count are needed, not {info.num_tracks} of type {info.track_type} and {info_b.num_tracks} of type {info_b.track_type}")
    num_tracks, num_components, num_samples = int(info.num_tracks), int(info.num_components), int(info.num_samples)
    if num_samples == 0 or num_tracks == 0:
        return NO_TRACK, -1.0, float("nan")
    sample_times = np.minimum(np.arange(num_samples, dtype=np.float32) / np.float32(info.sample_rate), np.float32(info.duration)).astype(np.float32)
    stride = num_tracks * num_components * 4
    stream = torch.cuda.current_stream(device)
    d_times = torch.from_numpy(sample_times).to(device)
    d_values = [torch.zeros((num_samples, stride // 4), dtype=torch.float32, device=device) for _ in range(2)]
    decode_params = default_params()
    decode_params.rounding_policy = ROUND_NEAREST
    for clip, d_value in zip((clip_a, clip_b), d_values):
        d_clips = torch.full((num_samples,), int(clip), dtype=torch.int32, device=device)
        ctx.decompress_scalar_tracks_batch(d_clips.data_ptr(), d_times.data_ptr(), num_samples, d_value.data_ptr(), stride, params=decode_params, stream=stream.cuda_stream)
    return _worst_scalar_error(ctx, device, stream, d_values[0], d_values[1], stride, num_samples, num_tracks, num_components, sample_times)
