"""cuda-raytracing_amd -- MI355X-native raycast hot path behind the reference's host API.

Python here is plumbing only: ctypes bindings of the two in-tree libraries
(``librt_hip.so`` = HIP kernels + C-ABI ``include/rt_hip.h``; ``librt_host.so`` = host C++
API mirror + C facade ``include/rt_host.h``) and small helpers used by ``bench.py`` and the
tests.  There is no CPU fallback: if the libraries are missing or no GPU is present, device
calls fail loudly.

The directory name is not a Python identifier; import it with
``importlib.import_module("cuda-raytracing_amd")``.
"""
import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIP_SO = os.path.join(HERE, "librt_hip.so")
HOST_SO = os.path.join(HERE, "librt_host.so")

_f = C.POINTER(C.c_float)
_i = C.POINTER(C.c_int32)
_vp = C.c_void_p


class RtError(RuntimeError):
    pass


class RtCameraParams(C.Structure):          # include/rt_hip.h
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("K_inv", C.c_float * 9), ("D", C.c_float * 4),
                ("camera_pose", C.c_float * 6), ("inv_camera_pose", C.c_float * 6)]


class RtDebugPlanes(C.Structure):
    _fields_ = [(n, _vp) for n in ("hit_instance", "hit_triangle", "node_pops", "aabb_tests", "tri_tests", "inside_hits")]


class RtMeshDesc(C.Structure):              # include/rt_hip.h
    _fields_ = [("num_triangles", C.c_int32), ("vertices", _f), ("normals", _f), ("uvs", _f), ("num_nodes", C.c_int32),
                ("node_bounds", _f), ("node_children", _i), ("node_leaf_first", _i), ("node_leaf_count", _i),
                ("num_leaf_indices", C.c_int32), ("leaf_indices", _i)]


class RtMaterialDesc(C.Structure):
    _fields_ = [("roughness", C.c_float), ("albedo", C.c_float * 3), ("metallic", C.c_float), ("illumination", C.c_float),
                ("texture", _vp), ("texture_width", C.c_int32), ("texture_height", C.c_int32), ("texture_pitch", C.c_size_t)]


class RtInstanceDesc(C.Structure):
    _fields_ = [("mesh_index", C.c_int32), ("material_index", C.c_int32), ("pose", C.c_float * 6), ("inv_pose", C.c_float * 6),
                ("rotation", C.c_float * 3), ("inv_rotation", C.c_float * 3), ("scale", C.c_float * 3), ("inv_scale", C.c_float * 3)]


# The fields of the query result structs of include/rt_hip.h, in struct order: the structs below and Scene.*_OUTPUTS are made of these
# tuples (a list struct is its slot fields, then its per-query tail), and _FIELDS has each name's trailing shape and dtype.
_RAY_OUTPUTS = ("t", "instance", "triangle", "location", "normal", "uv", "pops")
_POINT_OUTPUTS = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv", "pops")
_CROSSING_OUTPUTS = ("count", "winding", "pops")
_CROSSING_LIST_OUTPUTS = ("t", "instance", "triangle", "sign", "barycentric", "uv", "point")
_NEARBY_LIST_OUTPUTS = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")
_INTERSECT_COUNT_OUTPUTS = ("count", "any", "pops")
_INTERSECT_LIST_OUTPUTS = ("instance", "triangle", "normal", "segment")
_BOX_COUNT_OUTPUTS = ("count", "any", "pops")
_BOX_LIST_OUTPUTS = ("instance", "triangle")
_SECTION_COUNT_OUTPUTS = ("count", "any", "pops")
_SECTION_LIST_OUTPUTS = ("instance", "triangle", "segment", "normal")
_REGION_COUNT_OUTPUTS = ("count", "inside", "any", "pops")
_REGION_LIST_OUTPUTS = ("instance", "triangle", "inside", "normal")
_SEGMENT_OUTPUTS = ("distance", "instance", "triangle", "parameter", "segment_point", "point", "normal", "barycentric", "uv", "crossings",
                    "clearance", "within", "pops")
_SWEEP_OUTPUTS = ("time", "distance", "instance", "triangle", "centre", "point", "normal", "contact_normal", "barycentric", "uv", "hit",
                  "pops")
_TRIANGLE_HIT_OUTPUTS = ("distance", "instance", "triangle", "query_barycentric", "query_point", "point", "normal", "barycentric", "uv",
                         "intersections", "clearance", "within", "pops")


class RtRayHits(C.Structure):               # include/rt_hip.h (device pointers, any may be NULL)
    _fields_ = [(n, _vp) for n in _RAY_OUTPUTS]


RT_MAX_BATCH = 32                                   # RT_MAX_BATCH of include/rt_hip.h: frames per batched launch
_GBUFFER_OUTPUTS = ("t", "depth", "instance", "triangle", "location", "normal", "uv")


class RtGBuffer(C.Structure):               # include/rt_hip.h (device planes [count][height][width](xk), any may be NULL)
    _fields_ = [(n, _vp) for n in _GBUFFER_OUTPUTS]


_VISIBILITY_OUTPUTS = ("visible", "facing")


class RtVisibility(C.Structure):            # include/rt_hip.h, "visibility masks" (device planes [count][height][width], at least one)
    _fields_ = [(n, _vp) for n in _VISIBILITY_OUTPUTS]


class RtRollingPose(C.Structure):          # include/rt_hip.h, "rolling frames": the pose of one slice and its inverse
    _fields_ = [("camera_pose", C.c_float * 6), ("inv_camera_pose", C.c_float * 6)]


ROLLING_AXES = {"x": 0, "y": 1}             # the axis argument of the rolling calls: "x" = a slice is columns, "y" = rows


# the fields of a point cloud in RT_CLOUD_* bit order (include/rt_hip.h, "point clouds"): name -> (trailing shape, type)
_CLOUD_FIELDS = dict(range=((), np.float32), pixel=((), np.int32), frame=((), np.int32), instance=((), np.int32), triangle=((), np.int32),
                     position=((3,), np.float32), local=((3,), np.float32), normal=((3,), np.float32), uv=((2,), np.float32))
_CLOUD_OUTPUTS = tuple(_CLOUD_FIELDS)
RT_CLOUD_BITS = {k: 1 << i for i, k in enumerate(_CLOUD_OUTPUTS)}     # RT_CLOUD_RANGE .. RT_CLOUD_UV


class RtPointCloud(C.Structure):            # include/rt_hip.h (device arrays [capacity](xk), any may be NULL)
    _fields_ = [(n, _vp) for n in _CLOUD_OUTPUTS]


class RtPointHits(C.Structure):             # include/rt_hip.h (device pointers, any may be NULL)
    _fields_ = [(n, _vp) for n in _POINT_OUTPUTS]


class RtCrossings(C.Structure):             # include/rt_hip.h (device pointers, any may be NULL)
    _fields_ = [(n, _vp) for n in _CROSSING_OUTPUTS]


class RtCrossingList(C.Structure):          # include/rt_hip.h (device pointers, any may be NULL, at least one given)
    _fields_ = [(n, _vp) for n in _CROSSING_LIST_OUTPUTS + ("count",)]


class RtNearbyList(C.Structure):            # include/rt_hip.h (device pointers; distance, instance, triangle required)
    _fields_ = [(n, _vp) for n in _NEARBY_LIST_OUTPUTS + ("count", "pops")]


class RtIntersectCounts(C.Structure):       # include/rt_hip.h (device pointers, any may be NULL, at least one given)
    _fields_ = [(n, _vp) for n in _INTERSECT_COUNT_OUTPUTS]


class RtIntersectList(C.Structure):         # include/rt_hip.h (device pointers; instance, triangle required)
    _fields_ = [(n, _vp) for n in _INTERSECT_LIST_OUTPUTS + ("count", "pops")]


class RtBoxCounts(C.Structure):             # include/rt_hip.h (device pointers, any may be NULL, at least one given)
    _fields_ = [(n, _vp) for n in _BOX_COUNT_OUTPUTS]


class RtBoxList(C.Structure):               # include/rt_hip.h (device pointers; instance, triangle required)
    _fields_ = [(n, _vp) for n in _BOX_LIST_OUTPUTS + ("count", "pops")]


class RtSectionCounts(C.Structure):         # include/rt_hip.h (device pointers, any may be NULL, at least one given)
    _fields_ = [(n, _vp) for n in _SECTION_COUNT_OUTPUTS]


class RtSectionList(C.Structure):           # include/rt_hip.h (device pointers; instance, triangle required)
    _fields_ = [(n, _vp) for n in _SECTION_LIST_OUTPUTS + ("count", "pops")]


class RtRegionCounts(C.Structure):          # include/rt_hip.h (device pointers, any may be NULL, at least one given)
    _fields_ = [(n, _vp) for n in _REGION_COUNT_OUTPUTS]


class RtRegionList(C.Structure):            # include/rt_hip.h (device pointers; instance, triangle required)
    _fields_ = [(n, _vp) for n in _REGION_LIST_OUTPUTS + ("count", "pops")]


class RtSegmentHits(C.Structure):           # include/rt_hip.h (device pointers, any may be NULL, at least one given)
    _fields_ = [(n, _vp) for n in _SEGMENT_OUTPUTS]


class RtSweepHits(C.Structure):             # include/rt_hip.h (device pointers, any may be NULL, at least one given)
    _fields_ = [(n, _vp) for n in _SWEEP_OUTPUTS]


class RtTriangleHits(C.Structure):          # include/rt_hip.h (device pointers, any may be NULL, at least one given)
    _fields_ = [(n, _vp) for n in _TRIANGLE_HIT_OUTPUTS]


class RtSceneDesc(C.Structure):
    _fields_ = [("num_meshes", C.c_int32), ("meshes", C.POINTER(RtMeshDesc)), ("num_materials", C.c_int32),
                ("materials", C.POINTER(RtMaterialDesc)), ("num_instances", C.c_int32), ("instances", C.POINTER(RtInstanceDesc))]


# every exported symbol of include/rt_hip.h and include/rt_host.h (tests check the libraries export them all)
RT_HIP_SYMBOLS = [
    "rt_abi_version", "rt_build_info", "rt_device_count", "rt_set_device", "rt_malloc", "rt_malloc_pitch", "rt_free", "rt_memcpy_d2h",
    "rt_memcpy_h2d", "rt_memcpy2d_d2h", "rt_stream_synchronize", "rt_device_synchronize", "rt_error_string",
    "rt_bvh_build", "rt_scene_upload", "rt_scene_update_instance", "rt_scene_update_instance_async", "rt_scene_refit_mesh", "rt_scene_refit_mesh_device", "rt_scene_rebuild_mesh_device", "rt_scene_debug_read", "rt_scene_destroy", "rt_scene_info", "rt_scene_mesh_capacity", "rt_scene_mesh_flags", "rt_render", "rt_render_overlapped", "rt_render_overlapped_stats", "rt_scene_view_stats", "rt_scene_view_cull_stats", "rt_scene_dir_table_stats", "rt_scene_reserve_views", "rt_scene_memory", "rt_scene_loop_stats", "rt_render_batch",
    "rt_render_debug", "rt_render_ids", "rt_render_gbuffer", "rt_render_gbuffer_table", "rt_ray_table_create", "rt_ray_table_info", "rt_ray_table_destroy", "rt_ray_table_rays", "rt_camera_directions", "rt_point_cloud_workspace_bytes", "rt_point_cloud_offsets", "rt_point_cloud_offsets_table", "rt_point_cloud_fill", "rt_rolling_slices", "rt_rolling_workspace_bytes", "rt_render_gbuffer_rolling", "rt_point_cloud_rolling_workspace_bytes", "rt_point_cloud_offsets_rolling", "rt_point_cloud_fill_rolling", "rt_visibility", "rt_render_ex", "rt_render_ex_stripes", "rt_stripe_rows", "rt_render_stripes", "rt_render_stripes_batch", "rt_render_stripes_batch_rotating", "rt_unstripe", "rt_unstripe_batch", "rt_unstripe_batch_rotating",
    "rt_comm_available", "rt_comm_last_error", "rt_comm_last_error_any", "rt_comm_unique_id", "rt_comm_init_rank", "rt_comm_init_all", "rt_comm_info", "rt_comm_destroy",
    "rt_group_start", "rt_group_end", "rt_gather", "rt_all_to_all", "rt_render_tiled", "rt_render_tiled_all", "rt_timer_create", "rt_timer_start", "rt_timer_stop",
    "rt_timer_elapsed_ms", "rt_timer_destroy", "rt_trace_workspace_bytes", "rt_trace_rays", "rt_occluded", "rt_camera_rays",
    "rt_closest_points", "rt_count_crossings", "rt_winding_numbers", "rt_signed_distance", "rt_crossing_offsets_workspace_bytes",
    "rt_crossing_offsets", "rt_list_crossings", "rt_nearby_offsets_workspace_bytes", "rt_nearby_offsets", "rt_list_nearby",
    "rt_count_intersecting", "rt_intersecting_offsets_workspace_bytes", "rt_intersecting_offsets", "rt_list_intersecting",
    "rt_count_in_boxes", "rt_box_offsets_workspace_bytes", "rt_box_offsets", "rt_list_in_boxes", "rt_occupancy_grid",
    "rt_count_sections", "rt_section_offsets_workspace_bytes", "rt_section_offsets", "rt_list_sections",
    "rt_closest_to_segments", "rt_closest_to_triangles", "rt_sweep_spheres",
    "rt_count_in_regions", "rt_region_offsets_workspace_bytes", "rt_region_offsets", "rt_list_in_regions"]
RT_HOST_SYMBOLS = [
    "rth_obj_load", "rth_obj_parse", "rth_scan_float", "rth_obj_load_for_device", "rth_mesh_from_triangles_for_device", "rth_obj_load_lenient", "rth_obj_load_gpu", "rth_mesh_from_triangles", "rth_mesh_from_triangles_gpu", "rth_mesh_single_triangle", "rth_mesh_free", "rth_mesh_num_triangles",
    "rth_mesh_num_nodes", "rth_mesh_max_level", "rth_mesh_get_triangles", "rth_mesh_get_nodes", "rth_mesh_get_leaf_indices",
    "rth_mesh_print_stats", "rth_scene_create", "rth_scene_free", "rth_scene_add_material", "rth_scene_add_material_ppm",
    "rth_scene_set_material_params", "rth_scene_add_mesh", "rth_scene_add_mesh_instance", "rth_scene_upload_to_device", "rth_scene_update_mesh_instance", "rth_scene_update_mesh_instance_async", "rth_scene_refit_mesh", "rth_scene_rebuild_mesh",
    "rth_scene_num_mesh_instances", "rth_scene_device_handle", "rth_scene_visibility", "rth_instance_build", "rth_camera_create", "rth_camera_free",
    "rth_camera_set_pose", "rth_camera_set_stream", "rth_camera_render_scene", "rth_camera_render_scene_stripes",
    "rth_camera_render_scene_tiled", "rth_camera_render_scene_batch", "rth_camera_render_gbuffer", "rth_camera_directions", "rth_sensor_create", "rth_sensor_destroy", "rth_sensor_set_pose", "rth_sensor_set_stream", "rth_sensor_rays", "rth_sensor_render_gbuffer", "rth_camera_point_cloud_offsets", "rth_sensor_point_cloud_offsets", "rth_point_cloud_fill", "rth_sensor_render_rolling", "rth_sensor_point_cloud_offsets_rolling", "rth_point_cloud_fill_rolling","rth_camera_render_scene_stripes_batch", "rth_camera_render_scene_stripes_batch_rotating", "rth_camera_set_options",
    "rth_camera_render_scene_ex", "rth_xorwow", "rth_save_png", "rth_write_png_bgr",
    "rth_read_image_bgr", "rth_zlib_inflate", "rth_overlay_text_bgr", "rth_display_image", "rth_on_mouse", "rth_on_key",
    "rth_camera_params", "rth_q_rsqrt", "rth_atanf", "rth_normalize", "rth_invert_lre", "rth_apply_lre", "rth_euler2quat",
    "rth_apply_quat", "rth_invert_intrinsic", "rth_last_error"]

_hip = None
_host = None


def build(force=False, verbose=False):
    from . import _build as _b
    return _b.build(force=force, verbose=verbose)


def libs():
    """(librt_hip, librt_host) as ctypes CDLLs; raises RtError if they have not been built."""
    global _hip, _host
    if _hip is None:
        for p in (HIP_SO, HOST_SO):
            if not os.path.exists(p):
                raise RtError("%s is missing: run __graft_entry__.build() (no CPU fallback exists)" % p)
        # When PyTorch is installed it must be loaded FIRST: it ships its own libamdhip64 / librccl under the same sonames,
        # and a process must not end up with two HIP runtimes or two RCCLs (librt_hip.so dlopens "librccl.so.1" on first use
        # of rt_comm_*: after torch that resolves to torch's copy, before it to ROCm's -- and torch would then be handed
        # ROCm's copy in place of the one it was built against; seen as a double free at process exit).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        # The library must be the build of the sources next to it: profiles, roofline fractions and parity claims are about
        # one build of the kernels, and file times prove nothing (a variant copied over the shipped library is newer than
        # every source).  A mismatch is rebuilt when the compiler is here, else refused; RT_ALLOW_VARIANT_LIB=1
        # (tools/ab_variants.sh) loads the variant as it is -- bench.py's line then carries the variant's own hash.
        from . import _build as _b
        try:
            why = _b.library_mismatch(HIP_SO)
        except _b.BuildError as e:                               # (the sources next to the library cannot be read: nothing to check it against)
            raise RtError(str(e))
        if why is not None and not _b.variant_allowed():
            try:
                _b.build()
            except Exception as e:
                raise RtError("%s; rebuilding failed: %s" % (why, e))
            why = _b.library_mismatch(HIP_SO)
            if why is not None:
                raise RtError(why + " (after a rebuild)")
        hip = C.CDLL(HIP_SO, mode=C.RTLD_GLOBAL)
        host = C.CDLL(HOST_SO)
        _declare(hip, host)
        loaded = library_hash(hip)
        if loaded != _b.library_code_hash(HIP_SO) or (loaded != _b.kernel_code_hash() and not _b.variant_allowed()):
            raise RtError("the loaded librt_hip.so reports kernel code hash %s; the file holds %s and the sources hash to %s"
                          % (loaded, _b.library_code_hash(HIP_SO), _b.kernel_code_hash()))
        _hip, _host = hip, host
    return _hip, _host


def library_hash(hip=None):
    """The kernel code hash the LOADED librt_hip.so was compiled with (rt_build_info)."""
    h = hip if hip is not None else libs()[0]
    text = h.rt_build_info().decode()
    return text.split("=", 1)[1] if "=" in text else text


def _declare(h, s):
    h.rt_error_string.restype = C.c_char_p
    h.rt_build_info.restype = C.c_char_p
    h.rt_build_info.argtypes = []
    h.rt_error_string.argtypes = [C.c_int]
    h.rt_device_count.argtypes = [_i]
    h.rt_malloc.argtypes = [C.POINTER(_vp), C.c_size_t]
    h.rt_malloc_pitch.argtypes = [C.POINTER(_vp), C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t]
    h.rt_free.argtypes = [_vp]
    h.rt_memcpy_d2h.argtypes = [_vp, _vp, C.c_size_t, _vp]
    h.rt_memcpy_h2d.argtypes = [_vp, _vp, C.c_size_t, _vp]
    h.rt_memcpy2d_d2h.argtypes = [_vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp]
    h.rt_stream_synchronize.argtypes = [_vp]
    h.rt_scene_upload.argtypes = [C.POINTER(RtSceneDesc), C.POINTER(_vp)]
    h.rt_scene_info.argtypes = [_vp, C.POINTER(C.c_size_t), _i]
    h.rt_scene_mesh_capacity.argtypes = [_vp, C.c_int32, _i]
    h.rt_scene_mesh_flags.argtypes = [_vp, C.c_int32, _i]
    h.rt_scene_update_instance.argtypes = [_vp, C.c_int32, _vp]
    h.rt_scene_update_instance_async.argtypes = [_vp, C.c_int32, _vp, _vp]
    h.rt_scene_refit_mesh.argtypes = [_vp, C.c_int32, _f, _f, C.c_int32, _vp]
    h.rt_scene_refit_mesh_device.argtypes = [_vp, C.c_int32, _vp, _vp, C.c_int32, _vp]
    h.rt_scene_rebuild_mesh_device.argtypes = [_vp, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp]
    h.rt_scene_debug_read.argtypes = [_vp, C.c_int32, _vp, C.c_size_t, C.POINTER(C.c_size_t)]
    h.rt_scene_destroy.argtypes = [_vp]
    h.rt_render.argtypes = [_vp, C.POINTER(RtCameraParams), _vp, C.c_size_t, _vp, C.c_int]
    h.rt_render_overlapped.argtypes = [_vp, C.POINTER(RtCameraParams), _vp, C.c_size_t]
    h.rt_render_overlapped_stats.argtypes = [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    h.rt_scene_view_stats.argtypes = [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    h.rt_scene_view_cull_stats.argtypes = [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    h.rt_scene_dir_table_stats.argtypes = [_vp, C.POINTER(C.c_uint64)]
    h.rt_scene_reserve_views.argtypes = [_vp, C.c_int32]
    h.rt_scene_memory.argtypes = [_vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _i, _i]
    h.rt_scene_loop_stats.argtypes = [_vp, C.POINTER(RtCameraParams), C.POINTER(_vp), C.c_size_t, C.c_int32, _vp, C.POINTER(C.c_uint64)]
    h.rt_render_debug.argtypes = [_vp, C.POINTER(RtCameraParams), _vp, C.c_size_t, C.POINTER(RtDebugPlanes), _vp, C.c_int]
    h.rt_render_ids.argtypes = [_vp, C.POINTER(RtCameraParams), _vp, C.c_size_t, _vp, _vp, _vp, C.c_int]
    h.rt_render_batch.argtypes = [_vp, C.POINTER(RtCameraParams), C.POINTER(_vp), C.c_size_t, C.c_int32, _vp, C.c_int]
    h.rt_render_gbuffer.argtypes = [_vp, C.POINTER(RtCameraParams), C.c_int32, C.POINTER(_vp), C.c_size_t, C.POINTER(RtGBuffer), _vp, C.c_int]
    h.rt_render_gbuffer_table.argtypes = [_vp, _vp, C.POINTER(RtCameraParams), C.c_int32, C.POINTER(_vp), C.c_size_t, C.POINTER(RtGBuffer), _vp, C.c_int]
    h.rt_point_cloud_workspace_bytes.restype = C.c_size_t
    h.rt_point_cloud_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint32]
    cloud_tail = [C.c_int32, C.c_float, C.c_float, _vp, C.c_uint32, _vp, _vp, C.c_size_t, _vp, C.c_int]
    h.rt_point_cloud_offsets.argtypes = [_vp, C.POINTER(RtCameraParams)] + cloud_tail
    h.rt_point_cloud_offsets_table.argtypes = [_vp, _vp, C.POINTER(RtCameraParams)] + cloud_tail
    h.rt_point_cloud_fill.argtypes = [C.POINTER(RtCameraParams), C.c_int32, C.c_uint32, _vp, C.c_size_t, C.c_int64, C.POINTER(RtPointCloud), _vp, C.c_int]
    s.rth_camera_point_cloud_offsets.argtypes = [_vp, _vp, _f] + cloud_tail
    s.rth_sensor_point_cloud_offsets.argtypes = [_vp, _vp, _f] + cloud_tail
    h.rt_rolling_slices.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i]
    h.rt_rolling_workspace_bytes.restype = C.c_size_t
    h.rt_rolling_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    h.rt_render_gbuffer_rolling.argtypes = [_vp, _vp, C.POINTER(RtRollingPose), C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp), C.c_size_t,
                                            C.POINTER(RtGBuffer), _vp, _vp, C.c_size_t, _vp, C.c_int]
    h.rt_point_cloud_rolling_workspace_bytes.restype = C.c_size_t
    h.rt_point_cloud_rolling_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32]
    h.rt_point_cloud_offsets_rolling.argtypes = [_vp, _vp, C.POINTER(RtRollingPose), C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _vp,
                                                 C.c_uint32, _vp, _vp, C.c_size_t, _vp, C.c_int]
    roll_fill = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, _vp, C.c_size_t, C.c_int64, C.POINTER(RtPointCloud), _vp, C.c_int]
    h.rt_point_cloud_fill_rolling.argtypes = roll_fill
    s.rth_point_cloud_fill_rolling.argtypes = roll_fill
    s.rth_sensor_render_rolling.argtypes = [_vp, _vp, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(RtGBuffer), _vp, C.POINTER(_vp),
                                            C.c_size_t, _vp, C.c_size_t, _vp, C.c_int]
    s.rth_sensor_point_cloud_offsets_rolling.argtypes = [_vp, _vp, _f, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _vp,
                                                         C.c_uint32, _vp, _vp, C.c_size_t, _vp, C.c_int]
    s.rth_point_cloud_fill.argtypes = [C.c_int32, C.c_int32, _f, C.c_int32, C.c_uint32, _vp, C.c_size_t, C.c_int64, C.POINTER(RtPointCloud), _vp, C.c_int]
    h.rt_ray_table_create.argtypes = [_vp, C.c_int32, C.c_int32, _vp, C.c_int, C.POINTER(_vp)]
    h.rt_ray_table_info.argtypes = [_vp, _i, _i, C.POINTER(C.c_size_t)]
    h.rt_ray_table_destroy.argtypes = [_vp]
    h.rt_ray_table_rays.argtypes = [_vp, C.POINTER(RtCameraParams), _vp, _vp, _vp, C.c_int]
    h.rt_camera_directions.argtypes = [C.POINTER(RtCameraParams), _vp, _vp, C.c_int]
    h.rt_stripe_rows.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _i]
    h.rt_render_stripes.argtypes = [_vp, C.POINTER(RtCameraParams), _vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int]
    h.rt_unstripe.argtypes = [_vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp]
    h.rt_unstripe_batch.argtypes = [_vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_int32, _vp]
    h.rt_unstripe_batch_rotating.argtypes = [_vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, _vp]
    _sz = C.POINTER(C.c_size_t)
    h.rt_comm_last_error.restype = C.c_char_p
    h.rt_comm_last_error_any.restype = C.c_char_p
    h.rt_comm_available.argtypes = [_i]
    h.rt_comm_unique_id.argtypes = [_vp]
    h.rt_comm_init_rank.argtypes = [_vp, C.c_int32, C.c_int32, C.POINTER(_vp)]
    h.rt_comm_init_all.argtypes = [_i, C.c_int32, C.POINTER(_vp)]
    h.rt_comm_info.argtypes = [_vp, _i, _i, _i]
    h.rt_comm_destroy.argtypes = [_vp]
    h.rt_gather.argtypes = [_vp, _vp, C.c_size_t, _vp, C.c_int32, _vp]
    h.rt_all_to_all.argtypes = [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _vp]
    h.rt_render_tiled.argtypes = [_vp, _vp, C.POINTER(RtCameraParams), _vp, _vp, C.c_size_t, C.c_int32, C.c_int32, _vp, C.c_int]
    h.rt_render_tiled_all.argtypes = [C.POINTER(_vp), C.POINTER(_vp), C.c_int32, C.POINTER(RtCameraParams), _vp, _vp, C.c_size_t,
                                      C.c_int32, C.c_int32, C.POINTER(_vp), C.c_int]
    h.rt_trace_workspace_bytes.restype = C.c_size_t
    h.rt_trace_workspace_bytes.argtypes = [C.c_int32]
    h.rt_trace_rays.argtypes = [_vp, _vp, _vp, C.c_int32, C.POINTER(RtRayHits), _vp, C.c_size_t, _vp, C.c_int]
    h.rt_occluded.argtypes = [_vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, C.c_size_t, _vp, C.c_int]
    visibility = [_vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, C.c_float, C.POINTER(RtVisibility), _vp, C.c_int]
    h.rt_visibility.argtypes = visibility
    s.rth_scene_visibility.argtypes = visibility
    h.rt_closest_points.argtypes = [_vp, _vp, _vp, C.c_int32, C.POINTER(RtPointHits), _vp, C.c_int]
    h.rt_count_crossings.argtypes = [_vp, _vp, _vp, _vp, C.c_int32, C.POINTER(RtCrossings), _vp, C.c_int]
    h.rt_winding_numbers.argtypes = [_vp, _vp, C.c_int32, _vp, _vp, C.c_int]
    h.rt_signed_distance.argtypes = [_vp, _vp, _vp, C.c_int32, _vp, _vp, _vp, C.c_int]
    h.rt_crossing_offsets_workspace_bytes.restype = C.c_size_t
    h.rt_crossing_offsets_workspace_bytes.argtypes = [C.c_int32]
    h.rt_crossing_offsets.argtypes = [_vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, C.c_size_t, _vp, C.c_int]
    h.rt_list_crossings.argtypes = [_vp, _vp, _vp, _vp, C.c_int32, _vp, C.c_int32, C.POINTER(RtCrossingList), _vp, C.c_int]
    h.rt_nearby_offsets_workspace_bytes.restype = C.c_size_t
    h.rt_nearby_offsets_workspace_bytes.argtypes = [C.c_int32]
    h.rt_nearby_offsets.argtypes = [_vp, _vp, _vp, C.c_int32, _vp, _vp, C.c_size_t, _vp, C.c_int]
    h.rt_list_nearby.argtypes = [_vp, _vp, _vp, C.c_int32, _vp, C.c_int32, C.POINTER(RtNearbyList), _vp, C.c_int]
    h.rt_count_intersecting.argtypes = [_vp, _vp, _vp, C.c_int32, C.POINTER(RtIntersectCounts), _vp, C.c_int]
    h.rt_intersecting_offsets_workspace_bytes.restype = C.c_size_t
    h.rt_intersecting_offsets_workspace_bytes.argtypes = [C.c_int32]
    h.rt_intersecting_offsets.argtypes = [_vp, _vp, _vp, C.c_int32, _vp, _vp, C.c_size_t, _vp, C.c_int]
    h.rt_list_intersecting.argtypes = [_vp, _vp, _vp, C.c_int32, _vp, C.c_int32, C.POINTER(RtIntersectList), _vp, C.c_int]
    h.rt_count_in_boxes.argtypes = [_vp, _vp, C.c_int32, C.POINTER(RtBoxCounts), _vp, C.c_int]
    h.rt_box_offsets_workspace_bytes.restype = C.c_size_t
    h.rt_box_offsets_workspace_bytes.argtypes = [C.c_int32]
    h.rt_box_offsets.argtypes = [_vp, _vp, C.c_int32, _vp, _vp, C.c_size_t, _vp, C.c_int]
    h.rt_list_in_boxes.argtypes = [_vp, _vp, C.c_int32, _vp, C.c_int32, C.POINTER(RtBoxList), _vp, C.c_int]
    h.rt_count_sections.argtypes = [_vp, _vp, C.c_int32, C.POINTER(RtSectionCounts), _vp, C.c_int]
    h.rt_section_offsets_workspace_bytes.restype = C.c_size_t
    h.rt_section_offsets_workspace_bytes.argtypes = [C.c_int32]
    h.rt_section_offsets.argtypes = [_vp, _vp, C.c_int32, _vp, _vp, C.c_size_t, _vp, C.c_int]
    h.rt_list_sections.argtypes = [_vp, _vp, C.c_int32, _vp, C.c_int32, C.POINTER(RtSectionList), _vp, C.c_int]
    h.rt_count_in_regions.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.POINTER(RtRegionCounts), _vp, C.c_int]
    h.rt_region_offsets_workspace_bytes.restype = C.c_size_t
    h.rt_region_offsets_workspace_bytes.argtypes = [C.c_int32]
    h.rt_region_offsets.argtypes = [_vp, _vp, C.c_int32, C.c_int32, _vp, _vp, C.c_size_t, _vp, C.c_int]
    h.rt_list_in_regions.argtypes = [_vp, _vp, C.c_int32, C.c_int32, _vp, C.c_int32, C.POINTER(RtRegionList), _vp, C.c_int]
    h.rt_closest_to_segments.argtypes = [_vp, _vp, _vp, C.c_int32, C.POINTER(RtSegmentHits), _vp, C.c_int]
    h.rt_sweep_spheres.argtypes = [_vp, _vp, _vp, C.c_int32, C.POINTER(RtSweepHits), _vp, C.c_int]
    h.rt_closest_to_triangles.argtypes = [_vp, _vp, _vp, _vp, C.c_int32, C.POINTER(RtTriangleHits), _vp, C.c_int]
    h.rt_occupancy_grid.argtypes = [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32), _vp, _vp, _vp, C.c_int]
    h.rt_camera_rays.argtypes = [C.POINTER(RtCameraParams), _vp, _vp, _vp, C.c_int]
    h.rt_timer_create.argtypes = [C.POINTER(_vp)]
    h.rt_timer_start.argtypes = [_vp, _vp]
    h.rt_timer_stop.argtypes = [_vp, _vp]
    h.rt_timer_elapsed_ms.argtypes = [_vp, _f]
    h.rt_timer_destroy.argtypes = [_vp]

    s.rth_last_error.restype = C.c_char_p
    for n in ("rth_obj_load", "rth_obj_load_for_device", "rth_mesh_from_triangles_for_device", "rth_obj_load_lenient", "rth_obj_load_gpu", "rth_mesh_from_triangles", "rth_mesh_from_triangles_gpu", "rth_mesh_single_triangle", "rth_scene_create", "rth_camera_create",
              "rth_scene_device_handle"):
        getattr(s, n).restype = _vp
    s.rth_obj_load.argtypes = [C.c_char_p]
    s.rth_obj_load_lenient.argtypes = [C.c_char_p]
    s.rth_obj_load_gpu.argtypes = [C.c_char_p]
    s.rth_obj_load_for_device.argtypes = [C.c_char_p]
    s.rth_mesh_from_triangles_for_device.argtypes = [_f, C.c_int32]
    s.rth_obj_parse.restype = C.c_int32
    s.rth_obj_parse.argtypes = [C.c_char_p, C.c_int32, _vp, C.c_int32]
    s.rth_scan_float.restype = C.c_int
    s.rth_scan_float.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_float)]
    s.rth_mesh_from_triangles_gpu.argtypes = [_f, C.c_int32]
    s.rth_mesh_from_triangles.argtypes = [_f, C.c_int32]
    s.rth_mesh_single_triangle.argtypes = [_f]
    for n in ("rth_mesh_free", "rth_mesh_num_triangles", "rth_mesh_num_nodes", "rth_mesh_max_level", "rth_mesh_print_stats",
              "rth_scene_free", "rth_scene_upload_to_device", "rth_scene_num_mesh_instances", "rth_scene_device_handle",
              "rth_camera_free"):
        getattr(s, n).argtypes = [_vp]
    s.rth_mesh_free.restype = None
    s.rth_scene_free.restype = None
    s.rth_camera_free.restype = None
    s.rth_mesh_get_triangles.argtypes = [_vp, _f]
    s.rth_mesh_get_nodes.argtypes = [_vp, _f, _i, _i]
    s.rth_mesh_get_leaf_indices.argtypes = [_vp, _i]
    s.rth_scene_add_material.argtypes = [_vp, _f, _vp, C.c_int32, C.c_int32, C.c_size_t]
    s.rth_scene_add_material_ppm.argtypes = [_vp, _f, C.c_char_p]
    s.rth_scene_add_mesh.argtypes = [_vp, _vp]
    s.rth_scene_add_mesh_instance.argtypes = [_vp, C.c_int32, C.c_int32, _f, _f]
    s.rth_scene_update_mesh_instance.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32, _f, _f]
    s.rth_scene_update_mesh_instance_async.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32, _f, _f, _vp]
    s.rth_scene_refit_mesh.argtypes = [_vp, C.c_int32, _f, C.c_int32, _vp]
    s.rth_scene_rebuild_mesh.argtypes = [_vp, C.c_int32, _f, C.c_int32, _vp]
    s.rth_instance_build.argtypes = [_f, _f, _f]
    s.rth_camera_create.argtypes = [C.c_int32, C.c_int32, _f, _f]
    s.rth_camera_set_pose.argtypes = [_vp, _f]
    s.rth_camera_set_stream.argtypes = [_vp, _vp]
    s.rth_camera_render_scene.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int]
    s.rth_camera_render_scene_stripes.argtypes = [_vp, _vp, _vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int]
    s.rth_camera_render_scene_tiled.argtypes = [_vp, _vp, _vp, _vp, C.c_size_t, C.c_int32, C.c_int32, C.c_int]
    s.rth_camera_render_scene_batch.argtypes = [_vp, _vp, _f, C.POINTER(_vp), C.c_size_t, C.c_int32, C.c_int]
    s.rth_camera_render_gbuffer.argtypes = [_vp, _vp, _f, C.c_int32, C.POINTER(RtGBuffer), C.POINTER(_vp), C.c_size_t, _vp, C.c_int]
    s.rth_camera_directions.argtypes = [_vp, _vp, _vp, C.c_int]
    s.rth_sensor_create.argtypes = [_f, C.c_int32, C.c_int32, C.POINTER(_vp)]
    s.rth_sensor_destroy.argtypes = [_vp]
    s.rth_sensor_destroy.restype = None
    s.rth_sensor_set_pose.argtypes = [_vp, _f]
    s.rth_sensor_set_pose.restype = None
    s.rth_sensor_set_stream.argtypes = [_vp, _vp]
    s.rth_sensor_set_stream.restype = None
    s.rth_sensor_rays.argtypes = [_vp, _f, _vp, _vp, _vp, C.c_int]
    s.rth_sensor_render_gbuffer.argtypes = [_vp, _vp, _f, C.c_int32, C.POINTER(RtGBuffer), C.POINTER(_vp), C.c_size_t, _vp, C.c_int]
    s.rth_camera_render_scene_stripes_batch.argtypes = [_vp, _vp, _f, C.POINTER(_vp), C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                                                        C.c_int32, C.c_int]
    s.rth_camera_render_scene_stripes_batch_rotating.argtypes = [_vp, _vp, _f, C.POINTER(_vp), C.c_size_t, C.c_int32, C.c_int32, C.c_int32,
                                                                 C.c_int32, C.c_int32, C.c_int]
    s.rth_camera_params.argtypes = [_vp, _vp]
    s.rth_scene_set_material_params.argtypes = [_vp, C.c_int32, C.c_float, C.c_float, C.c_float]
    s.rth_camera_set_options.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32]
    s.rth_camera_render_scene_ex.argtypes = [_vp, _vp, _vp, C.c_size_t, _vp, C.c_int]
    s.rth_save_png.argtypes = [C.c_char_p, _vp, C.c_int32, C.c_int32, C.c_size_t]
    s.rth_write_png_bgr.argtypes = [C.c_char_p, _vp, C.c_int32, C.c_int32, C.c_size_t]
    s.rth_read_image_bgr.argtypes = [C.c_char_p, _vp, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    s.rth_zlib_inflate.argtypes = [_vp, C.c_size_t, _vp, C.c_size_t, C.POINTER(C.c_size_t)]
    s.rth_overlay_text_bgr.argtypes = [_vp, C.c_int32, C.c_int32, C.c_size_t, C.c_char_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_uint8, C.c_uint8, C.c_uint8]
    s.rth_overlay_text_bgr.restype = None
    s.rth_display_image.argtypes = [_vp, C.c_int32, C.c_int32, C.c_size_t, C.c_double, C.c_char_p]
    s.rth_on_mouse.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32]
    s.rth_on_mouse.restype = None
    s.rth_on_key.argtypes = [C.POINTER(C.c_float), C.c_int32]
    s.rth_xorwow.restype = C.c_uint32
    s.rth_xorwow.argtypes = [C.c_uint64, C.c_int32, _vp, _vp]
    s.rth_q_rsqrt.restype = C.c_float
    s.rth_q_rsqrt.argtypes = [C.c_float]
    s.rth_atanf.restype = C.c_float
    s.rth_atanf.argtypes = [C.c_float]


def _fa(a):
    return np.ascontiguousarray(a, np.float32)


def _fp(a):
    return a.ctypes.data_as(_f)


def _pose_batch(poses, d_ptrs):
    """The arguments of a batched launch: (n, poses as float32 [n, 6], the n device pointers as a ctypes void* array)"""
    n = len(poses)
    P = _fa(np.asarray(poses, np.float32).reshape(n, 6))
    return n, P, (_vp * n)(*[int(x) if not isinstance(x, _vp) else x.value for x in d_ptrs])


def check(rc, what="rt call"):
    if rc != 0:
        h, s = libs()
        msg = h.rt_error_string(rc).decode() if rc > 0 or rc >= -5 else "?"
        extra = s.rth_last_error().decode()
        if rc == -5:
            extra = h.rt_comm_last_error().decode()
        raise RtError("%s failed: %d (%s) %s" % (what, rc, msg, extra))


def device_count():
    h, _ = libs()
    n = C.c_int32(0)
    rc = h.rt_device_count(C.byref(n))
    return n.value if rc == 0 else 0


# ------------------------------------------------------------------------------------------------
# Thin object wrappers over the C facade.  Names and call order follow the reference's kernel.cu
# main(): load meshes, add materials / meshes / instances, upload_to_device, camera.render_scene.
# ------------------------------------------------------------------------------------------------

class Mesh:
    """MeshPrimitive (host triangles + BVH)."""

    def __init__(self, handle):
        if not handle:
            raise RtError("mesh creation failed: " + libs()[1].rth_last_error().decode())
        self.h = handle

    @classmethod
    def load_obj(cls, path, lenient=False, gpu_build=False, for_device=False):    # OBJLoader::load / load_lenient; BVH on host or GPU
        """for_device: OBJLoader::load_for_device -- no host tree, the GPU builds it inside the scene at Scene.upload_to_device."""
        if for_device:
            return cls(libs()[1].rth_obj_load_for_device(os.fsencode(path)))
        fn = libs()[1].rth_obj_load_gpu if gpu_build else (libs()[1].rth_obj_load_lenient if lenient else libs()[1].rth_obj_load)
        return cls(fn(os.fsencode(path)))

    @classmethod
    def from_triangles(cls, tris18, gpu_build=False, for_device=False):  # MeshPrimitive(std::vector<TrianglePrimitive>[, build_on_device])
        t = _fa(tris18).reshape(-1, 18)
        fn = libs()[1].rth_mesh_from_triangles_for_device if for_device else (libs()[1].rth_mesh_from_triangles_gpu if gpu_build else libs()[1].rth_mesh_from_triangles)
        return cls(fn(_fp(t), t.shape[0]))

    @classmethod
    def single_triangle(cls, abc9):                   # TrianglePrimitive(a, b, c)
        return cls(libs()[1].rth_mesh_single_triangle(_fp(_fa(abc9))))

    @property
    def num_triangles(self):
        return libs()[1].rth_mesh_num_triangles(self.h)

    @property
    def num_nodes(self):
        return libs()[1].rth_mesh_num_nodes(self.h)

    @property
    def max_level(self):
        return libs()[1].rth_mesh_max_level(self.h)

    def dump(self):
        s = libs()[1]
        nt, nn = self.num_triangles, self.num_nodes
        tris = np.zeros((nt, 18), np.float32)
        s.rth_mesh_get_triangles(self.h, _fp(tris))
        boxes = np.zeros((nn, 6), np.float32)
        child = np.zeros((nn, 2), np.int32)
        lc = np.zeros(nn, np.int32)
        total = s.rth_mesh_get_nodes(self.h, _fp(boxes), child.ctypes.data_as(_i), lc.ctypes.data_as(_i))
        li = np.zeros(max(total, 1), np.int32)
        s.rth_mesh_get_leaf_indices(self.h, li.ctypes.data_as(_i))
        return dict(tris=tris, boxes=boxes, child=child, leaf_count=lc, leaf_idx=li[:total])

    def close(self):
        if self.h:
            libs()[1].rth_mesh_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene:
    def __init__(self):
        self.h = libs()[1].rth_scene_create()
        if not self.h:
            raise RtError("scene creation failed")

    def add_material(self, albedo, texture_bgr=None, ppm=None, roughness=0.0, metallic=0.0, illumination=0.0, texture_path=None):
        """texture_path (or its older name ppm): a PNG, baseline-JPEG or binary-PPM file for Material::upload_texture;
        texture_bgr: [h, w, 3] uint8 B,G,R pixels."""
        s = libs()[1]
        a = _fa(albedo)
        path = texture_path if texture_path is not None else ppm
        if path is not None:
            check(s.rth_scene_add_material_ppm(self.h, _fp(a), os.fsencode(path)), "add_material(texture file)")
        elif texture_bgr is not None:
            t = np.ascontiguousarray(texture_bgr, np.uint8)
            check(s.rth_scene_add_material(self.h, _fp(a), t.ctypes.data, t.shape[1], t.shape[0], t.strides[0]), "add_material")
        else:
            check(s.rth_scene_add_material(self.h, _fp(a), None, 0, 0, 0), "add_material")
        self._nmat = getattr(self, "_nmat", 0) + 1
        check(s.rth_scene_set_material_params(self.h, self._nmat - 1, roughness, metallic, illumination), "set_material_params")

    def add_mesh(self, mesh):
        check(libs()[1].rth_scene_add_mesh(self.h, mesh.h), "add_mesh")

    def add_mesh_instance(self, mesh, material, pose=(0, 0, 0, 0, 0, 0), scale=(1, 1, 1)):
        check(libs()[1].rth_scene_add_mesh_instance(self.h, mesh, material, _fp(_fa(pose)), _fp(_fa(scale))), "add_mesh_instance")

    def upload_to_device(self):
        check(libs()[1].rth_scene_upload_to_device(self.h), "Scene::upload_to_device")

    def update_mesh_instance(self, index, mesh, material, pose, scale=(1, 1, 1), stream=False):
        """stream=False: synchronising update (the reference's cudaMemcpy, Scene.cpp:67-74); a stream handle (or None for
        the default stream): ordered on that stream, no host wait."""
        if stream is False:
            check(libs()[1].rth_scene_update_mesh_instance(self.h, index, mesh, material, _fp(_fa(pose)), _fp(_fa(scale))),
                  "Scene::update_mesh_instance")
        else:
            check(libs()[1].rth_scene_update_mesh_instance_async(self.h, index, mesh, material, _fp(_fa(pose)), _fp(_fa(scale)), stream),
                  "Scene::update_mesh_instance(stream)")

    def refit_mesh(self, mesh_index, tris18, stream=None):
        """Scene::refit_mesh: the mesh deformed (same triangle count and order): new records, refitted bounds, no rebuild."""
        t = _fa(tris18).reshape(-1, 18)
        check(libs()[1].rth_scene_refit_mesh(self.h, mesh_index, _fp(t), t.shape[0], stream), "Scene::refit_mesh")

    def rebuild_mesh(self, mesh_index, tris18, stream=None):
        """Scene::rebuild_mesh: new triangles (at most as many as at upload): a new tree, built on the GPU in place."""
        t = _fa(tris18).reshape(-1, 18)
        check(libs()[1].rth_scene_rebuild_mesh(self.h, mesh_index, _fp(t), t.shape[0], stream), "Scene::rebuild_mesh")

    def debug_read(self, which, dtype):
        """tests: one of the device arrays of the uploaded scene (rt_scene_debug_read) as a numpy array of `dtype`."""
        n = C.c_size_t(0)
        check(libs()[0].rt_scene_debug_read(self.device_handle, which, None, 0, C.byref(n)), "rt_scene_debug_read")
        out = np.zeros(n.value, np.uint8)
        check(libs()[0].rt_scene_debug_read(self.device_handle, which, out.ctypes.data, n.value, C.byref(n)), "rt_scene_debug_read")
        return out.view(dtype)

    @property
    def device_handle(self):
        return libs()[1].rth_scene_device_handle(self.h)

    def mesh_flags(self, mesh_index):
        """rt_scene_mesh_flags: bit 0 = the mesh is traversed with the generic slab loop (an unordered or NaN child box)"""
        v = C.c_int32(0)
        check(libs()[0].rt_scene_mesh_flags(self.device_handle, mesh_index, C.byref(v)), "rt_scene_mesh_flags")
        return v.value

    def overlap_stats(self):
        """(frames that went through rt_render_overlapped, those that had to wait for the other stream)"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        check(libs()[0].rt_render_overlapped_stats(self.device_handle, C.byref(a), C.byref(b)), "rt_render_overlapped_stats")
        return a.value, b.value

    def view_stats(self):
        """rt_scene_view_stats: dict(launches=, fallbacks=, grows=, slot_frames=) of the scene's view records"""
        a, b, c, d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        check(libs()[0].rt_scene_view_stats(self.device_handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "rt_scene_view_stats")
        return dict(launches=a.value, fallbacks=b.value, grows=c.value, slot_frames=d.value)

    def view_cull_stats(self):
        """rt_scene_view_cull_stats: the culled leaf children per frame in the views the scene's last pre-pass wrote -- a list with one
        count per frame of that launch, empty when it wrote no culled views (RT_VIEW_CULL=0, a samples-only extension launch, none yet)"""
        n, out = C.c_int32(0), (C.c_uint64 * 32)()
        check(libs()[0].rt_scene_view_cull_stats(self.device_handle, C.byref(n), out), "rt_scene_view_cull_stats")
        return [int(out[k]) for k in range(n.value)]

    def dir_table_stats(self):
        """rt_scene_dir_table_stats: dict(launches=, skipped=, grows=, bytes=) -- launches that read a direction table, view launches
        that did not, times a slot's table was replaced by a larger one, bytes the tables hold now"""
        out = (C.c_uint64 * 4)()
        check(libs()[0].rt_scene_dir_table_stats(self.device_handle, out), "rt_scene_dir_table_stats")
        return dict(launches=out[0], skipped=out[1], grows=out[2], bytes=out[3])

    def reserve_views(self, frames_per_launch):
        """rt_scene_reserve_views: size the view pool for launches of up to that many frames (0: back to growing on demand)"""
        check(libs()[0].rt_scene_reserve_views(self.device_handle, frames_per_launch), "rt_scene_reserve_views")

    def memory(self):
        """rt_scene_memory: dict(records_bytes=, view_pool_bytes=, device_bytes=, view_slots=, view_slot_frames=)"""
        a, b, c, d, e = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_int32(0), C.c_int32(0)
        check(libs()[0].rt_scene_memory(self.device_handle, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)), "rt_scene_memory")
        return dict(records_bytes=a.value, view_pool_bytes=b.value, device_bytes=c.value, view_slots=d.value, view_slot_frames=e.value)

    LOOP_STATS = ("waves", "asm", "asm_posed", "cpp_octant", "cpp_generic", "deep", "retraced_lanes", "cpp_iters")     # RT_LOOP_* of include/rt_hip.h

    def loop_stats(self, camera, poses, d_imgs, pitch, stream=None):
        """rt_scene_loop_stats: renders the batch (poses[i] -> d_imgs[i]) through the instrumented copy of the production kernel and says
        which traversal loop the waves ran: dict of the RT_LOOP_* counts plus asm_loop_frac = casts on the hand-written loop / all casts."""
        n, P, ptrs = _pose_batch(poses, d_imgs)
        cams = (RtCameraParams * n)()
        for i in range(n):
            camera.set_pose(P[i])
            libs()[1].rth_camera_params(camera.h, C.addressof(cams[i]))
        out = (C.c_uint64 * 8)()
        check(libs()[0].rt_scene_loop_stats(self.device_handle, cams, ptrs, pitch, n, stream, out), "rt_scene_loop_stats")
        d = {k: int(out[i]) for i, k in enumerate(self.LOOP_STATS)}
        casts = d["asm"] + d["cpp_octant"] + d["cpp_generic"] + d["deep"]
        d["asm_loop_frac"] = round(d["asm"] / casts, 5) if casts else None
        return d

    RAY_OUTPUTS = _RAY_OUTPUTS                                          # the fields of RtRayHits

    def trace_rays(self, origins, directions, outputs=("t", "instance", "triangle"), stream=None, binning=None):
        """The reference's cast_ray (raycast.cu:21-142) on the caller's rays, closest hit, bit for bit (rt_trace_rays): dict of the
        wanted RAY_OUTPUTS -- t [...] float32 (HitInfo::min, the world DISTANCE to the hit, FLT_MAX on a miss; directions are not
        normalised), instance / triangle [...] int32 (-1 on a miss), location / normal [..., 3] float32 (raycast.cu:98-102 for the
        accepted hit, :115-122), uv [..., 2] float32 (TrianglePrimitive::point_inside), pops [...] int32 (node pops, :61).
        origins, directions: float32 [..., 3], contiguous, same shape.  torch tensors on the scene's (current) device: outputs
        are torch tensors allocated there and the call is enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t; default
        torch.cuda.current_stream()) without a synchronise.  Every tensor a query makes (outputs, offsets, workspace) is allocated
        with `stream` as the current stream, so the caching allocator hands its memory out again only in `stream`'s order, after the
        kernel that writes it.  numpy arrays: copied to the device and back, the call synchronises.  binning: sort the rays by direction
        octant on the device first (same results; None = TRACE_BINNING, see DESIGN.md "Ray queries")."""
        outputs = _check_outputs(outputs, self.RAY_OUTPUTS)

        def call(h, handle, ins, ptr, n, st, sync, ws, ws_bytes):
            hits = RtRayHits(*[ptr.get(k) for k in _RAY_OUTPUTS])
            check(h.rt_trace_rays(handle, ins[0], ins[1], n, C.byref(hits), ws, ws_bytes, st, sync), "rt_trace_rays")
        return _device_query(self, [("origins", origins), ("directions", directions)], outputs, call, stream,
                             scratch=_trace_workspace(binning))

    def occluded(self, origins, directions, tmax=None, stream=None, binning=None):
        """Occlusion (rt_occluded): cast_ray(ray, lighting_pass = true, light_distance = tmax) with the early return of
        raycast.cu:129-133 -- uint8 [...], 1 where the cast accepts a hit closer than tmax (None: FLT_MAX for every ray; a
        float32 array of the rays' leading shape otherwise).  Arguments and paths as in trace_rays."""
        def call(h, handle, ins, ptr, n, st, sync, ws, ws_bytes):
            check(h.rt_occluded(handle, ins[0], ins[1], ins[2], n, ptr["occluded"], ws, ws_bytes, st, sync), "rt_occluded")
        return _device_query(self, [("origins", origins), ("directions", directions), ("tmax", tmax)], ("occluded",), call, stream,
                             scratch=_trace_workspace(binning))["occluded"]

    POINT_OUTPUTS = _POINT_OUTPUTS                                      # the fields of RtPointHits

    def closest_points(self, points, max_distance=None, outputs=("distance", "instance", "triangle"), stream=None):
        """The nearest point of the scene's triangles to each of the caller's points (rt_closest_points; the rule, bit for bit a
        brute-force minimum over every instance and triangle, is in include/rt_hip.h): dict of the wanted POINT_OUTPUTS --
        distance [...] float32 (FLT_MAX on a miss), instance / triangle [...] int32 (-1 on a miss), point / normal [..., 3] float32
        (world position of the closest point, world face normal), barycentric [..., 2] float32 (weights of v1 and v2), uv [..., 2]
        float32, pops [...] int32 (interior nodes visited).  points: float32 [..., 3], contiguous.  max_distance: None (+inf) or
        float32 of the points' leading shape; a triangle farther than it is no candidate (inclusive), NaN or negative = a miss.
        torch tensors on the scene's (current) device: outputs are allocated there, with `stream` as the current stream as in
        trace_rays, and the call is enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t; default
        torch.cuda.current_stream()) without a synchronise.  numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.POINT_OUTPUTS)

        def call(h, handle, ins, ptr, n, st, sync):
            hits = RtPointHits(*[ptr.get(k) for k in _POINT_OUTPUTS])
            check(h.rt_closest_points(handle, ins[0], ins[1], n, C.byref(hits), st, sync), "rt_closest_points")
        return _device_query(self, [("points", points), ("max_distance", max_distance)], outputs, call, stream)

    CROSSING_OUTPUTS = _CROSSING_OUTPUTS                                # the fields of RtCrossings

    def count_crossings(self, origins, directions, tmax=None, outputs=("count", "winding"), stream=None):
        """Crossings of the scene's triangles along each of the caller's rays (rt_count_crossings; the rule, equal to a brute-force
        count over every instance and triangle, is in include/rt_hip.h): dict of the wanted CROSSING_OUTPUTS, each int32 of the rays'
        leading shape -- count (triangles crossed at 0 < t <= tmax, both faces), winding (+1 per crossing leaving a mesh wound
        counter-clockwise seen from outside, -1 per crossing entering it), pops (interior nodes visited).  origins / directions:
        float32 [..., 3], contiguous.  tmax: None (+inf) or float32 of the rays' leading shape, a ray parameter (with directions
        b - a and tmax 1, count is the crossings of the segment ab).  torch tensors: asynchronous on `stream` (default the current
        stream); numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.CROSSING_OUTPUTS)

        def call(h, handle, ins, ptr, n, st, sync):
            c = RtCrossings(*[ptr.get(k) for k in _CROSSING_OUTPUTS])
            check(h.rt_count_crossings(handle, ins[0], ins[1], ins[2], n, C.byref(c), st, sync), "rt_count_crossings")
        return _device_query(self, [("origins", origins), ("directions", directions), ("tmax", tmax)], outputs, call, stream)

    def winding_numbers(self, points, stream=None):
        """The winding number of each of the caller's points (rt_winding_numbers): int32 of the points' leading shape, the median of
        the windings along three fixed directions (include/rt_hip.h rule 6); nonzero = inside.  points: float32 [..., 3].  Paths as
        in count_crossings."""
        def call(h, handle, ins, ptr, n, st, sync):
            check(h.rt_winding_numbers(handle, ins[0], n, ptr["winding"], st, sync), "rt_winding_numbers")
        return _device_query(self, [("points", points)], ("winding",), call, stream)["winding"]

    def signed_distance(self, points, max_distance=None, stream=None):
        """Signed distance of each of the caller's points (rt_signed_distance): float32 of the points' leading shape, closest_points'
        distance (same points, same max_distance) negated where winding_numbers is not 0 -- so -0.0 and -FLT_MAX occur.  points:
        float32 [..., 3]; max_distance: None (+inf) or float32 of the points' leading shape.  Paths as in count_crossings."""
        def call(h, handle, ins, ptr, n, st, sync):
            check(h.rt_signed_distance(handle, ins[0], ins[1], n, ptr["sdf"], None, st, sync), "rt_signed_distance")
        return _device_query(self, [("points", points), ("max_distance", max_distance)], ("sdf",), call, stream)["sdf"]

    CROSSING_LIST_OUTPUTS = _CROSSING_LIST_OUTPUTS                      # the slot fields of RtCrossingList

    def list_crossings(self, origins, directions, tmax=None, max_hits=None, outputs=CROSSING_LIST_OUTPUTS, stream=None):
        """Every triangle each of the caller's rays crosses, sorted by (t, instance, triangle) (rt_crossing_offsets /
        rt_list_crossings; the pairs are exactly count_crossings' pairs, include/rt_hip.h rule 8).  Fields: t (float32, a ray
        parameter), instance / triangle (int32), sign (int8, +1 leaving a mesh wound counter-clockwise seen from outside), barycentric
        / uv ([2] float32), point ([3] float32, world).  origins / directions / tmax as in count_crossings.
        max_hits=None (CSR): dict of `offsets` (int64 [n + 1], ray j's hits at offsets[j]:offsets[j+1]), the wanted fields over all
        hits ([total], [total, 2], [total, 3]), `ray` (int32 [total], the flat index of each hit's ray) and `count` (int32 of the
        rays' leading shape).  On torch this makes exactly ONE host synchronisation (reading offsets[n] to size the outputs).
        max_hits=K >= 1: the first K hits of each ray, fields [..., K] / [..., K, 2|3] padded with t = inf, instance = triangle = -1,
        sign 0 and float 0, plus `count` (the full count, so count > K means truncated); on torch fully asynchronous on `stream`.
        numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.CROSSING_LIST_OUTPUTS)
        return _list_query(self, _CROSSING_LIST, [("origins", origins), ("directions", directions), ("tmax", tmax)],
                           _check_max_hits(max_hits), outputs, stream, per_query=("count",))

    NEARBY_LIST_OUTPUTS = _NEARBY_LIST_OUTPUTS                          # the slot fields of RtNearbyList

    def list_nearby(self, points, max_distance=None, max_hits=None, outputs=("distance", "instance", "triangle"), stream=None):
        """Every triangle within max_distance of each of the caller's points, sorted by (d2, instance, triangle) -- slot 0 is
        closest_points' winner (rt_nearby_offsets / rt_list_nearby, include/rt_hip.h rule 9).  Fields as closest_points gives them
        for each triangle: distance (float32), instance / triangle (int32), point / normal ([3] float32, world), barycentric / uv
        ([2] float32).  points / max_distance as in closest_points (inclusive; NaN or negative = no triangle).
        max_hits=None (CSR): dict of `offsets` (int64 [n + 1], point j's triangles at offsets[j]:offsets[j+1]), the wanted fields
        over all pairs ([total], [total, 2|3]), `point_index` (int32 [total], the flat index of each pair's point) and `count`
        (int32 of the points' leading shape, from the offsets); "pops" in outputs adds the interior nodes visited by the fill.  On
        torch this makes exactly ONE host synchronisation (reading offsets[n] to size the outputs).
        max_hits=K >= 1: the K nearest within the bound, fields [..., K] / [..., K, 2|3] padded with distance = FLT_MAX, instance =
        triangle = -1 and float 0; `count` (the full number, so count > K means truncated) and `pops` only when in outputs --
        without count the traversal prunes by the K-th distance (k-nearest), with the same rooms.  On torch fully asynchronous on
        `stream`.  max_distance and max_hits must not both be None (every triangle for every point).
        numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.NEARBY_LIST_OUTPUTS, extras=("count", "pops"))
        max_hits = _check_max_hits(max_hits)
        if max_distance is None and max_hits is None:
            raise ValueError("max_distance and max_hits are both None: that lists every triangle for every point")
        return _list_query(self, _NEARBY_LIST, [("points", points), ("max_distance", max_distance)], max_hits, outputs, stream)

    INTERSECT_COUNT_OUTPUTS = _INTERSECT_COUNT_OUTPUTS                  # the fields of RtIntersectCounts

    def count_intersecting(self, triangles, skip_instance=None, outputs=("count",), stream=None):
        """How many scene triangles each of the caller's triangles intersects (rt_count_intersecting; the rule, equal to a brute-force
        loop over every instance and triangle, is rule 10 of include/rt_hip.h): dict of the wanted INTERSECT_COUNT_OUTPUTS of the
        triangles' leading shape -- count (int32, the number of (instance, triangle) pairs), any (bool; wanted without count, the
        traversal stops at the first pair: the cheap collision check), pops (int32, interior nodes visited).  triangles: float32
        [..., 3, 3] world vertices, contiguous.  skip_instance: None or int32 of the leading shape, one instance per triangle whose pairs
        are never reported (-1 = none).  torch tensors: asynchronous on `stream` (default the current stream); numpy arrays: copied to
        the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.INTERSECT_COUNT_OUTPUTS)

        def call(h, handle, ins, ptr, n, st, sync):
            c = RtIntersectCounts(*[ptr.get(k) for k in _INTERSECT_COUNT_OUTPUTS])
            check(h.rt_count_intersecting(handle, ins[0], ins[1], n, C.byref(c), st, sync), "rt_count_intersecting")
        return _device_query(self, [("triangles", triangles), ("skip_instance", skip_instance)], outputs, call, stream,
                             **_TRIANGLE_INPUTS)

    INTERSECT_LIST_OUTPUTS = _INTERSECT_LIST_OUTPUTS                    # the slot fields of RtIntersectList

    def list_intersecting(self, triangles, skip_instance=None, max_hits=None, outputs=("instance", "triangle"), stream=None):
        """Every scene triangle each of the caller's triangles intersects, sorted by (instance, triangle) (rt_intersecting_offsets /
        rt_list_intersecting, include/rt_hip.h rule 10).  Fields: instance / triangle (int32), normal ([3] float32, the world face
        normal as closest_points gives it), segment ([2, 3] float32, world points of the first and the last counting segment test).
        triangles / skip_instance as in count_intersecting.
        max_hits=None (CSR): dict of `offsets` (int64 [n + 1], query j's pairs at offsets[j]:offsets[j+1]), the wanted fields over all
        pairs ([total], [total, 3], [total, 2, 3]), `query_index` (int32 [total], the flat index of each pair's query) and `count`
        (int32 of the leading shape, from the offsets); "pops" in outputs adds the interior nodes visited by the fill.  On torch this
        makes exactly ONE host synchronisation (reading offsets[n] to size the outputs).
        max_hits=K >= 1: the first K pairs of each query, fields [..., K] / [..., K, 3] / [..., K, 2, 3] padded with instance =
        triangle = -1 and float 0; `count` (the full number, so count > K means truncated) and `pops` only when in outputs -- without
        count the traversal ends after the instance of a full room's last key, with the same rooms.  On torch fully asynchronous on
        `stream`.  numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.INTERSECT_LIST_OUTPUTS, extras=("count", "pops"))
        return _list_query(self, _INTERSECT_LIST, [("triangles", triangles), ("skip_instance", skip_instance)],
                           _check_max_hits(max_hits), outputs, stream)

    BOX_COUNT_OUTPUTS = _BOX_COUNT_OUTPUTS                              # the fields of RtBoxCounts

    def count_in_boxes(self, boxes, outputs=("count",), stream=None):
        """How many scene triangles lie in or touch each of the caller's axis-aligned boxes (rt_count_in_boxes; the rule, equal to a
        brute-force loop over every instance and triangle, is rule 11 of include/rt_hip.h): dict of the wanted BOX_COUNT_OUTPUTS of
        the boxes' leading shape -- count (int32, the number of (instance, triangle) pairs), any (bool; wanted without count, the
        traversal stops at the first pair), pops (int32, interior nodes visited).  boxes: float32 [..., 2, 3] world, lo then hi,
        contiguous; a box with lo > hi on an axis or a NaN has no pairs.  torch tensors: asynchronous on `stream` (default the current
        stream); numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.BOX_COUNT_OUTPUTS)

        def call(h, handle, ins, ptr, n, st, sync):
            c = RtBoxCounts(*[ptr.get(k) for k in _BOX_COUNT_OUTPUTS])
            check(h.rt_count_in_boxes(handle, ins[0], n, C.byref(c), st, sync), "rt_count_in_boxes")
        return _device_query(self, [("boxes", boxes)], outputs, call, stream, **_BOX_INPUTS)

    BOX_LIST_OUTPUTS = _BOX_LIST_OUTPUTS                                # the slot fields of RtBoxList

    def list_in_boxes(self, boxes, max_hits=None, outputs=("instance", "triangle"), stream=None):
        """Every scene triangle that lies in or touches each of the caller's boxes, sorted by (instance, triangle) (rt_box_offsets /
        rt_list_in_boxes, include/rt_hip.h rule 11).  Fields: instance / triangle (int32).  boxes as in count_in_boxes.
        max_hits=None (CSR): dict of `offsets` (int64 [n + 1], box j's pairs at offsets[j]:offsets[j+1]), the wanted fields over all
        pairs ([total]), `query_index` (int32 [total], the flat index of each pair's box) and `count` (int32 of the leading shape, from
        the offsets); "pops" in outputs adds the interior nodes visited by the fill.  On torch this makes exactly ONE host
        synchronisation (reading offsets[n] to size the outputs).
        max_hits=K >= 1: the first K pairs of each box, fields [..., K] padded with -1; `count` (the full number, so count > K means
        truncated) and `pops` only when in outputs -- without count the traversal ends after the instance of a full room's last key,
        with the same rooms.  On torch fully asynchronous on `stream`.  numpy arrays: copied to the device and back, the call
        synchronises."""
        outputs = _check_outputs(outputs, self.BOX_LIST_OUTPUTS, extras=("count", "pops"))
        return _list_query(self, _BOX_LIST, [("boxes", boxes)], _check_max_hits(max_hits), outputs, stream)

    SECTION_COUNT_OUTPUTS = _SECTION_COUNT_OUTPUTS                      # the fields of RtSectionCounts

    def count_sections(self, planes, outputs=("count",), stream=None):
        """How many scene triangles each of the caller's planes cuts (rt_count_sections; the rule, equal to a brute-force loop over
        every instance and triangle, is rule 12 of include/rt_hip.h: a vertex with height >= 0 and a vertex with height < 0): dict of
        the wanted SECTION_COUNT_OUTPUTS of the planes' leading shape -- count (int32, the number of (instance, triangle) pairs), any
        (bool; wanted without count, the traversal stops at the first pair), pops (int32, interior nodes visited).  planes: float32
        [..., 2, 3] world, a point of the plane then its normal (any length; a zero normal has no pairs), contiguous.  torch tensors:
        asynchronous on `stream` (default the current stream); numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.SECTION_COUNT_OUTPUTS)

        def call(h, handle, ins, ptr, n, st, sync):
            c = RtSectionCounts(*[ptr.get(k) for k in _SECTION_COUNT_OUTPUTS])
            check(h.rt_count_sections(handle, ins[0], n, C.byref(c), st, sync), "rt_count_sections")
        return _device_query(self, [("planes", planes)], outputs, call, stream, **_PLANE_INPUTS)

    SECTION_LIST_OUTPUTS = _SECTION_LIST_OUTPUTS                        # the slot fields of RtSectionList

    def list_sections(self, planes, max_hits=None, outputs=("instance", "triangle", "segment"), stream=None):
        """Where each of the caller's planes cuts the scene: every cut triangle, sorted by (instance, triangle), with the segment of
        the cut (rt_section_offsets / rt_list_sections, include/rt_hip.h rule 12).  Fields: instance / triangle (int32), segment
        ([2, 3] float32, world: end 0 then end 1, running along cross(plane normal, face normal), so on a closed mesh one triangle's
        end 1 meets its neighbour's end 0, to rounding), normal ([3] float32, the world face normal as closest_points gives it).
        planes as in count_sections.
        max_hits=None (CSR): dict of `offsets` (int64 [n + 1], plane j's pairs at offsets[j]:offsets[j+1]), the wanted fields over all
        pairs ([total], [total, 2, 3], [total, 3]), `query_index` (int32 [total], the flat index of each pair's plane) and `count`
        (int32 of the leading shape, from the offsets); "pops" in outputs adds the interior nodes visited by the fill.  On torch this
        makes exactly ONE host synchronisation (reading offsets[n] to size the outputs).
        max_hits=K >= 1: the first K pairs of each plane, fields [..., K] / [..., K, 2, 3] / [..., K, 3] padded with instance =
        triangle = -1 and float 0; `count` (the full number, so count > K means truncated) and `pops` only when in outputs -- without
        count the traversal ends after the instance of a full room's greatest key, with the same rooms.  On torch fully asynchronous
        on `stream`.  numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.SECTION_LIST_OUTPUTS, extras=("count", "pops"))
        return _list_query(self, _SECTION_LIST, [("planes", planes)], _check_max_hits(max_hits), outputs, stream)

    REGION_COUNT_OUTPUTS = _REGION_COUNT_OUTPUTS                        # the fields of RtRegionCounts

    def count_in_regions(self, regions, outputs=("count",), stream=None):
        """How many scene triangles lie in or touch each of the caller's convex regions (rt_count_in_regions; the rule, equal to a
        brute-force loop over every instance and triangle, is rule 15 of include/rt_hip.h: rule 12's half-open classes on each of
        the K planes, then the triangle clipped by the planes in order): dict of the wanted REGION_COUNT_OUTPUTS of the regions'
        leading shape -- count (int32, the number of (instance, triangle) pairs), inside (int32, how many of them lie wholly
        inside), any (bool; wanted without count and inside, the traversal stops at the first pair), pops (int32, interior nodes
        visited).  regions: float32 [..., K, 2, 3] world, contiguous, 1 <= K <= REGION_MAX_PLANES read from the shape: per plane a
        point of it, then its normal pointing INTO the region (any length; a zero normal anywhere leaves the region without
        pairs).  The test is closed (touching counts) and decided in fp32 relative to each plane's point, so put the point on the
        region's face.  regions_from_boxes / regions_from_obbs / regions_from_frusta make common shapes.  torch tensors:
        asynchronous on `stream` (default the current stream); numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.REGION_COUNT_OUTPUTS)
        K = _region_planes(regions)

        def call(h, handle, ins, ptr, n, st, sync):
            c = RtRegionCounts(*[ptr.get(k) for k in _REGION_COUNT_OUTPUTS])
            check(h.rt_count_in_regions(handle, ins[0], n, K, C.byref(c), st, sync), "rt_count_in_regions")
        return _device_query(self, [("regions", regions)], outputs, call, stream, shape=(K, 2, 3))

    REGION_LIST_OUTPUTS = _REGION_LIST_OUTPUTS                          # the slot fields of RtRegionList

    def list_in_regions(self, regions, max_hits=None, outputs=("instance", "triangle", "inside"), stream=None):
        """Every scene triangle that lies in or touches each of the caller's convex regions, sorted by (instance, triangle)
        (rt_region_offsets / rt_list_in_regions, include/rt_hip.h rule 15).  Fields: instance / triangle (int32), inside (uint8, 1
        when the triangle lies wholly inside the region), normal ([3] float32, the world face normal as closest_points gives it).
        regions as in count_in_regions.
        max_hits=None (CSR): dict of `offsets` (int64 [n + 1], region j's pairs at offsets[j]:offsets[j+1]), the wanted fields over
        all pairs ([total], [total, 3]), `query_index` (int32 [total], the flat index of each pair's region) and `count` (int32 of
        the leading shape, from the offsets); "pops" in outputs adds the interior nodes visited by the fill.  On torch this makes
        exactly ONE host synchronisation (reading offsets[n] to size the outputs).
        max_hits=M >= 1: the first M pairs of each region, fields [..., M] / [..., M, 3] padded with instance = triangle = -1,
        inside = 0 and float 0; `count` (the full number, so count > M means truncated) and `pops` only when in outputs -- without
        count the traversal ends after the instance of a full room's greatest key, with the same rooms.  On torch fully
        asynchronous on `stream`.  numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.REGION_LIST_OUTPUTS, extras=("count", "pops"))
        return _list_query(self, _REGION_LIST[_region_planes(regions)], [("regions", regions)], _check_max_hits(max_hits), outputs, stream)

    GRID_OUTPUTS = ("occupied", "count")

    SEGMENT_OUTPUTS = _SEGMENT_OUTPUTS                                  # the fields of RtSegmentHits

    def closest_to_segments(self, segments, max_distance=None, outputs=("distance", "instance", "triangle", "parameter"), stream=None):
        """The nearest point of the scene's triangles to each of the caller's segments, and whether a capsule touches anything
        (rt_closest_to_segments; the rule, bit for bit a brute-force loop over every instance and triangle, is rule 13 of
        include/rt_hip.h): dict of the wanted SEGMENT_OUTPUTS of the segments' leading shape -- distance (float32, FLT_MAX on a miss),
        instance / triangle (int32, -1 on a miss), parameter (float32 in [0, 1]: where on the segment its nearest point lies),
        segment_point / point ([3] float32, world: the nearest pair, on the segment and on the triangle), normal ([3]), barycentric /
        uv ([2]) as closest_points gives them, crossings (int32, triangles the segment pierces: count_crossings with directions
        P1 - P0 and tmax 1), clearance (float32, 0 where crossings > 0, else distance), within (int32 0 / 1: a triangle within
        max_distance of the segment, or pierced by it -- the capsule overlap test; wanted alone or with pops, the distance traversal
        stops at the first triangle in reach), pops (int32, interior nodes visited by the distance traversal).  The point fields
        describe the nearest triangle even where the segment pierces another.  segments: float32 [..., 2, 3] world end points,
        contiguous.  max_distance: None (+inf) or float32 of the leading shape, the capsule's radius (inclusive; NaN or negative =
        nothing in reach).  torch tensors: asynchronous on `stream` (default the current stream); numpy arrays: copied to the device
        and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.SEGMENT_OUTPUTS)

        def call(h, handle, ins, ptr, n, st, sync):
            hits = RtSegmentHits(*[ptr.get(k) for k in _SEGMENT_OUTPUTS])
            check(h.rt_closest_to_segments(handle, ins[0], ins[1], n, C.byref(hits), st, sync), "rt_closest_to_segments")
        return _device_query(self, [("segments", segments), ("max_distance", max_distance)], outputs, call, stream, **_SEGMENT_INPUTS)

    SWEEP_OUTPUTS = _SWEEP_OUTPUTS                                      # the fields of RtSweepHits

    def sweep_spheres(self, segments, radius, outputs=("time", "instance", "triangle"), stream=None):
        """The first contact of a sphere whose centre moves from P0 to P1 with the scene: how far it can go, and what it touches there
        (rt_sweep_spheres; the rule, bit for bit a brute-force loop over every instance and triangle, is rule 16 of include/rt_hip.h):
        dict of the wanted SWEEP_OUTPUTS of the segments' leading shape -- time (float32 in [0, 1]: the centre stops at
        P0 + time * (P1 - P0); 0 where the sphere starts in contact; FLT_MAX on a miss), distance (float32: the centre's distance from
        the contact point, the radius up to rounding, less where it starts in contact; FLT_MAX on a miss), instance / triangle (int32,
        -1 on a miss), centre / point ([3] float32, world: the sphere's centre at contact and the contact point), normal ([3]: the
        face normal as closest_points gives it), contact_normal ([3]: the unit vector from point towards centre), barycentric / uv
        ([2]) of the contact point, hit (int32 0 / 1; wanted alone or with pops, the traversal stops at the first contact found), pops
        (int32, interior nodes visited).  A sphere that starts in contact reports the nearest triangle to P0, as
        closest_points(P0, max_distance=radius) does.  segments: float32 [..., 2, 3] world positions of the centre, contiguous.
        radius: float32 of the leading shape, required (inclusive; NaN or negative = no contact).  torch tensors: asynchronous on
        `stream` (default the current stream); numpy arrays: copied to the device and back, the call synchronises."""
        outputs = _check_outputs(outputs, self.SWEEP_OUTPUTS)
        if radius is None:
            raise ValueError("radius is required: float32 of the segments' leading shape")

        def call(h, handle, ins, ptr, n, st, sync):
            hits = RtSweepHits(*[ptr.get(k) for k in _SWEEP_OUTPUTS])
            check(h.rt_sweep_spheres(handle, ins[0], ins[1], n, C.byref(hits), st, sync), "rt_sweep_spheres")
        return _device_query(self, [("segments", segments), ("radius", radius)], outputs, call, stream, **_SEGMENT_INPUTS)

    TRIANGLE_HIT_OUTPUTS = _TRIANGLE_HIT_OUTPUTS                        # the fields of RtTriangleHits

    def closest_to_triangles(self, triangles, max_distance=None, skip_instance=None, outputs=("distance", "instance", "triangle"),
                             stream=None):
        """The nearest point of the scene's triangles to each of the caller's triangles, and whether it lies within a clearance
        (rt_closest_to_triangles; the rule, bit for bit a brute-force loop over every instance and triangle, is rule 14 of
        include/rt_hip.h): dict of the wanted TRIANGLE_HIT_OUTPUTS of the triangles' leading shape -- distance (float32, FLT_MAX on a
        miss), instance / triangle (int32, -1 on a miss), query_barycentric ([2] float32: the weights of the query's second and third
        vertex at its nearest point), query_point / point ([3] float32, world: the nearest pair, on the query triangle and on the
        scene triangle), normal ([3]), barycentric / uv ([2]) as closest_points gives them, intersections (int32, scene triangles the
        query triangle intersects: count_intersecting's count), clearance (float32, 0 where intersections > 0, else distance), within
        (int32 0 / 1: a triangle within max_distance of the query, or intersected by it; wanted alone or with pops, the distance
        traversal stops at the first triangle in reach), pops (int32, interior nodes visited by the distance traversal).  The point
        fields describe the nearest triangle even where the query intersects another.  triangles: float32 [..., 3, 3] world vertices,
        contiguous.  max_distance: None (+inf) or float32 of the leading shape (inclusive; NaN or negative = nothing in reach).
        skip_instance: None or int32 of the leading shape, one instance per triangle that contributes to nothing (-1 = none): an
        instance's own triangles with its index ask how close it is to everything else.  A large triangle prunes little: subdivide it
        first.  torch tensors: asynchronous on `stream` (default the current stream); numpy arrays: copied to the device and back, the
        call synchronises."""
        outputs = _check_outputs(outputs, self.TRIANGLE_HIT_OUTPUTS)

        def call(h, handle, ins, ptr, n, st, sync):
            hits = RtTriangleHits(*[ptr.get(k) for k in _TRIANGLE_HIT_OUTPUTS])
            check(h.rt_closest_to_triangles(handle, ins[0], ins[1], ins[2], n, C.byref(hits), st, sync), "rt_closest_to_triangles")
        return _device_query(self, [("triangles", triangles), ("max_distance", max_distance), ("skip_instance", skip_instance)], outputs,
                             call, stream, **_TRIANGLE_INPUTS)

    def occupancy_grid(self, origin, spacing, dims, outputs=("occupied",), stream=None, as_numpy=False):
        """count_in_boxes on the cells of a regular grid, which the kernel makes itself (rt_occupancy_grid): cell (ix, iy, iz) is the
        box from origin + i*spacing to origin + (i + 1)*spacing per axis in float32, so neighbouring cells share their faces exactly.
        origin, spacing: 3 floats; dims: (nx, ny, nz), each 0..2^24, at most 2^31 - 1 cells.  Dict of the wanted GRID_OUTPUTS, each
        [nz, ny, nx]: occupied (bool; wanted without count, a cell's traversal stops at its first triangle), count (int32) -- torch
        tensors on the current device, enqueued on `stream` (default the current torch stream) without a synchronise, or numpy
        arrays with as_numpy=True.  A negative spacing makes every cell an inverted box: all zeros."""
        outputs = _check_outputs(outputs, self.GRID_OUTPUTS)
        o, sp = (np.array(a, np.float32).reshape(-1) for a in (origin, spacing))
        d = np.array(dims).reshape(-1)
        if o.shape != (3,) or sp.shape != (3,) or d.shape != (3,) or d.dtype.kind not in "iu":
            raise ValueError("origin and spacing must be 3 floats and dims 3 ints, got %r, %r, %r" % (origin, spacing, dims))
        if (d < 0).any() or (d > 2 ** 24).any() or math.prod(int(x) for x in d) > 2 ** 31 - 1:
            raise ValueError("dims must be 0..2^24 each with at most 2^31 - 1 cells, got %r" % (tuple(int(x) for x in d),))
        d = d.astype(np.int32)
        shape = (int(d[2]), int(d[1]), int(d[0]))
        handle = self.device_handle
        with _staging(not as_numpy, stream) as sg:
            out = {k: sg.alloc(shape, _FIELDS[k][1]) for k in outputs}
            check(libs()[0].rt_occupancy_grid(handle, _fp(o), _fp(sp), d.ctypes.data_as(C.POINTER(C.c_int32)),
                                              sg.ptr(out["occupied"]) if "occupied" in out else None,
                                              sg.ptr(out["count"]) if "count" in out else None, sg.stream, sg.sync), "rt_occupancy_grid")
            return {k: sg.result(a) for k, a in out.items()}

    VISIBILITY_OUTPUTS = _VISIBILITY_OUTPUTS

    def visibility(self, instance, location, points, normal=None, bias=2.0 ** -10, outputs=("visible",), stream=None, as_numpy=False):
        """Visibility masks (rt_visibility; the rule is in include/rt_hip.h, "visibility masks"): which of `points` see the surface
        each pixel's ray hit.  instance [n, h, w] int32 and location [n, h, w, 3] float32 (normal [n, h, w, 3] too when "facing" is
        wanted) are G-buffer planes -- of Camera.render_gbuffer, Sensor.render_gbuffer, Sensor.render_rolling, or Scene.trace_rays
        reshaped -- as torch tensors on the scene's GPU or numpy arrays.  points: [K, 3] (the same for every frame) or [n, K, 3],
        world, 1 <= K <= 32, anything numpy converts to float32 or a torch tensor.  bias in [0, 1): the relative amount by which
        the ray from a point stops short of the surface (0 lets the surface shadow itself).  Returns a dict of the wanted
        VISIBILITY_OUTPUTS, int32 [n, h, w]: bit k of visible = points[k] sees the hit (no front face lies before it), of facing =
        the hit's front side is turned to points[k]; a miss is 0; `visible & facing` is "lit by" / "valid for".  Tensors for
        tensors, enqueued on `stream` (default the current torch stream) without a synchronise; numpy arrays for numpy arrays or
        with as_numpy=True.  Every ValueError is raised before a device call."""
        outputs, bias = _visibility_options(outputs, bias)
        facing = "facing" in outputs
        if facing and normal is None:
            raise ValueError("outputs with 'facing' need the normal plane")
        if instance is None or location is None:
            raise ValueError("instance and location are required")
        torch_in, lead, _n, dev = _query_inputs([("location", location), ("instance", instance)], ints=("instance",))
        if facing:                                                      # (a vector plane of its own: checked as a first input is)
            if _query_inputs([("normal", normal)])[0] != torch_in:
                raise ValueError("instance, location, normal must all be torch tensors or all numpy arrays")
            if tuple(normal.shape) != tuple(location.shape):
                raise ValueError("normal must have the shape %s, got %s" % (tuple(location.shape), tuple(normal.shape)))
        if len(lead) != 3 or min(lead) < 1:
            raise ValueError("instance must be [n, h, w] and location [n, h, w, 3], non-empty, got %s" % (tuple(location.shape),))
        n, h, w = (int(x) for x in lead)
        P = _visibility_points(points, n, keep_device=torch_in)
        with _staging(torch_in, stream, dev) as sg:
            ins = sg.inputs([instance, location, normal if facing else None])
            out = _visibility_launch(sg, self, dict(instance=ins[0], location=ins[1], normal=ins[2]), n, h, w, P, bias, outputs)
            res = {k: sg.result(a) for k, a in out.items()}
        if as_numpy and torch_in:
            res = {k: a.cpu().numpy() for k, a in res.items()}
        return res

    def info(self):
        b = C.c_size_t(0)
        d = C.c_int32(0)
        check(libs()[0].rt_scene_info(self.device_handle, C.byref(b), C.byref(d)), "rt_scene_info")
        return dict(device_bytes=b.value, max_stack=d.value)

    def close(self):
        if self.h:
            libs()[1].rth_scene_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _render_gbuffer(call, what, owner, scene, poses, outputs, image, stream, as_numpy, visibility=None):
    """Camera.render_gbuffer and Sensor.render_gbuffer: the argument checks, the staging and the cut into launches of RT_MAX_BATCH
    frames.  `call`: rth_camera_render_gbuffer or rth_sensor_render_gbuffer; owner: .h, .width, .height, .current_pose().
    visibility = (points, bias, mask outputs) (render_visibility): the launches also render the planes the masks are made from,
    rt_visibility follows them on the same stream, and the result holds the masks beside the planes `outputs` names (which may
    then be empty)."""
    outputs = tuple(outputs)
    if [o for o in outputs if o not in _GBUFFER_OUTPUTS] or len(set(outputs)) != len(outputs) or not (outputs or image or visibility):
        raise ValueError("outputs must be a subset of %s (non-empty unless image=True), nothing twice, got %r" % (_GBUFFER_OUTPUTS, outputs))
    wanted = outputs
    if visibility is not None:
        masks, bias = _visibility_options(visibility[2], visibility[1])
        needed = ("instance", "location") + (("normal",) if "facing" in masks else ())
        outputs = outputs + tuple(k for k in needed if k not in outputs)
    if poses is None:
        P = _fa(owner.current_pose()).reshape(1, 6)
    else:
        P = np.asarray(poses, np.float32)
        if P.ndim != 2 or P.shape[1] != 6 or P.shape[0] < 1:
            raise ValueError("poses must be None or a non-empty sequence of (x, y, z, yaw, pitch, roll), got shape %s" % (P.shape,))
        P = _fa(P)
    n, h, w = int(P.shape[0]), owner.height, owner.width
    if n * h * w > 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 1 pixels per call, got %d frames of %d x %d" % (n, w, h))
    if visibility is not None:
        points = _visibility_points(visibility[0], n)
    with _staging(not as_numpy, stream) as sg:
        out = {k: sg.alloc((n, h, w) + _FIELDS[k][0], _FIELDS[k][1]) for k in outputs}
        img = sg.alloc((n, h, w, 3), np.uint8) if image else None
        for first in range(0, n, RT_MAX_BATCH):
            m = min(RT_MAX_BATCH, n - first)
            at = {k: sg.ptr(a) for k, a in out.items()}
            at = {k: (v.value if isinstance(v, _vp) else int(v)) + first * h * w * math.prod(_FIELDS[k][0]) * 4 for k, v in at.items()}
            planes = RtGBuffer(*[at.get(k) for k in _GBUFFER_OUTPUTS])
            ptrs = None
            if image:
                base = sg.ptr(img)
                base = base.value if isinstance(base, _vp) else int(base)
                ptrs = (_vp * m)(*[base + (first + i) * h * w * 3 for i in range(m)])
            check(call(owner.h, scene.h, _fp(P[first:first + m]), m, C.byref(planes), ptrs, w * 3, sg.stream, sg.sync), what)
        res = {k: sg.result(out[k]) for k in wanted}
        if visibility is not None:
            staged = _visibility_launch(sg, scene, {k: sg.ptr(out[k]) for k in needed}, n, h, w, points, bias, masks)
            res.update({k: sg.result(a) for k, a in staged.items()})
        if image:
            res["image"] = sg.result(img)
        return res


def _rolling_args(owner, poses, axis, slice_pixels):
    """Sensor.render_rolling and Sensor.rolling_point_cloud: (poses float32 [n, slices, 6], axis number, slices), every ValueError of
    the rolling arguments -- before any device call"""
    if axis not in ROLLING_AXES:
        raise ValueError("axis must be 'x' (a slice is columns) or 'y' (rows), got %r" % (axis,))
    if isinstance(slice_pixels, bool) or int(slice_pixels) != slice_pixels or slice_pixels < 8 or slice_pixels % 8:
        raise ValueError("slice_pixels must be a positive multiple of 8 (slices are whole 8x8 tiles), got %r" % (slice_pixels,))
    ax = ROLLING_AXES[axis]
    slices = -(-(owner.height if ax else owner.width) // int(slice_pixels))
    P = np.asarray(poses, np.float32)
    if P.ndim != 3 or P.shape[2] != 6 or P.shape[0] < 1:
        raise ValueError("poses must be [frames, slices, 6] of (x, y, z, yaw, pitch, roll), got shape %s" % (P.shape,))
    if P.shape[1] != slices:
        raise ValueError("%d x %d with axis %r and slice_pixels %d has %d slices, poses has %d" % (owner.width, owner.height, axis, slice_pixels, slices, P.shape[1]))
    return _fa(P), ax, slices


def _point_cloud(call, what, owner, scene, poses, outputs, min_range, max_range, mask, stream, as_numpy, rolling=None):
    """Camera.point_cloud and Sensor.point_cloud: the argument checks -- all before any device call -- and, per group of RT_MAX_BATCH
    frames, the workspace, the offsets call, the one host read of the total, the exact allocation and the fill.  `call`:
    rth_camera_point_cloud_offsets or rth_sensor_point_cloud_offsets; owner: .h, .width, .height, .current_pose().
    rolling = (axis, slice_pixels) (Sensor.rolling_point_cloud): poses are [n, slices, 6], `call` is
    rth_sensor_point_cloud_offsets_rolling and the fill is the rolling one, which finds the poses in the workspace."""
    outputs = tuple(outputs)
    if not outputs or [o for o in outputs if o not in _CLOUD_OUTPUTS] or len(set(outputs)) != len(outputs):
        raise ValueError("outputs must be a non-empty subset of %s, nothing twice, got %r" % (_CLOUD_OUTPUTS, outputs))
    if rolling is not None:
        P, axis, slices = _rolling_args(owner, poses, *rolling)
    elif poses is None:
        P = _fa(owner.current_pose()).reshape(1, 6)
    else:
        P = np.asarray(poses, np.float32)
        if P.ndim != 2 or P.shape[1] != 6 or P.shape[0] < 1:
            raise ValueError("poses must be None or a non-empty sequence of (x, y, z, yaw, pitch, roll), got shape %s" % (P.shape,))
        P = _fa(P)
    n, h, w = int(P.shape[0]), owner.height, owner.width
    if n * h * w > 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 1 pixels per call, got %d frames of %d x %d" % (n, w, h))
    lo, hi = float(np.float32(min_range)), float(np.float32(max_range))
    if math.isnan(lo) or math.isnan(hi) or lo > hi:
        raise ValueError("min_range <= max_range must hold, neither a NaN, got %r, %r" % (min_range, max_range))
    torch_mask = mask is not None and type(mask).__module__.split(".")[0] == "torch"
    if mask is not None:
        if not torch_mask:
            mask = np.asarray(mask)
        if tuple(mask.shape) != (h, w) or str(mask.dtype).replace("torch.", "") not in ("bool", "uint8"):
            raise ValueError("mask must be bool or uint8 [%d, %d] (height, width), got %s %s" % (h, w, mask.dtype, tuple(mask.shape)))
    fields = 0
    for k in outputs:
        fields |= RT_CLOUD_BITS[k]
    hip, host = libs()
    with _staging(not as_numpy, stream) as sg:
        d_mask = None
        if mask is not None and as_numpy:
            m8 = mask.detach().cpu().numpy() if torch_mask else mask
            d_mask = sg.inputs([np.ascontiguousarray(m8.astype(np.uint8))])[0]
        elif mask is not None:
            keep_mask = (mask if torch_mask else sg.torch.from_numpy(np.ascontiguousarray(mask))).to(sg.dev).to(sg.torch.uint8).contiguous()
            d_mask = sg.ptr(keep_mask)
        groups, ends, base = [], [], 0                              # per group: its fields; its frames' end offsets, running on
        for first in range(0, n, RT_MAX_BATCH):
            m = min(RT_MAX_BATCH, n - first)
            if rolling is not None:
                ws_bytes = int(hip.rt_point_cloud_rolling_workspace_bytes(w, h, m, fields, slices))
            else:
                ws_bytes = int(hip.rt_point_cloud_workspace_bytes(w, h, m, fields))
            ws = sg.alloc((ws_bytes,), np.uint8)
            offsets = sg.alloc((m + 1,), np.int64)
            Pg = _fp(P[first:first + m])
            if rolling is not None:
                check(call(owner.h, scene.h, Pg, m, slices, axis, rolling[1], lo, hi, d_mask, fields, sg.ptr(offsets), sg.ptr(ws), ws_bytes,
                           sg.stream, sg.sync), what)
            else:
                check(call(owner.h, scene.h, Pg, m, lo, hi, d_mask, fields, sg.ptr(offsets), sg.ptr(ws), ws_bytes, sg.stream, sg.sync), what)
            total = sg.read_int64(offsets, m)                       # torch: the one host synchronisation per group, for the size of the outputs
            out = {k: sg.alloc((total,) + _CLOUD_FIELDS[k][0], _CLOUD_FIELDS[k][1]) for k in outputs}
            if total and rolling is not None:
                cloud = RtPointCloud(*[sg.ptr(out[k]) if k in out else None for k in _CLOUD_OUTPUTS])
                check(host.rth_point_cloud_fill_rolling(w, h, m, axis, rolling[1], fields, sg.ptr(ws), ws_bytes, total, C.byref(cloud), sg.stream,
                                                        sg.sync), "point_cloud_fill_rolling")
            elif total:
                cloud = RtPointCloud(*[sg.ptr(out[k]) if k in out else None for k in _CLOUD_OUTPUTS])
                check(host.rth_point_cloud_fill(w, h, Pg, m, fields, sg.ptr(ws), ws_bytes, total, C.byref(cloud), sg.stream, sg.sync),
                      "point_cloud_fill")
            got = {k: sg.result(a) for k, a in out.items()}
            if first and "frame" in got:
                got["frame"] = got["frame"] + first                 # (the call numbers its own frames from 0)
            groups.append(got)
            off = sg.result(offsets)
            ends.append(off[1:] + base)
            base += total
        if as_numpy:
            res = {k: groups[0][k] if len(groups) == 1 else np.concatenate([g[k] for g in groups]) for k in outputs}
            res["offsets"] = np.concatenate([np.zeros(1, np.int64)] + ends)
        else:
            torch = sg.torch
            res = {k: groups[0][k] if len(groups) == 1 else torch.cat([g[k] for g in groups]) for k in outputs}
            res["offsets"] = torch.cat([torch.zeros(1, dtype=torch.int64, device=sg.dev)] + ends)
        return res


_RENDER_VISIBILITY_DOC = """Visibility masks of this %s's frames: render_gbuffer for instance, location (normal for "facing") and whatever `gbuffer`
names -- one launch per RT_MAX_BATCH frames -- then rt_visibility on the same stream (the rule is in include/rt_hip.h, "visibility
masks"; Scene.visibility has the arguments).  points: [K, 3] world (every frame) or [n, K, 3], n = len(poses); a torch tensor is
copied to the host first.  Returns a dict of the masks named in `outputs` (int32 [n, h, w]), the `gbuffer` planes and, with
image=True, "image", as render_gbuffer returns them.  Every ValueError is raised before a device call."""
_POINT_CLOUD_DOC = """The point cloud of %s frames (rt_point_cloud_offsets%s + rt_point_cloud_fill; the rules are in include/rt_hip.h): the pixels
        whose ray hit something with min_range <= t <= max_range and, with a mask (bool or uint8 [height, width], numpy or torch,
        shared by all frames), mask != 0 -- packed in (frame, y, x) order.  poses: None = the current pose (one frame), or a sequence
        of any length of (x, y, z, yaw, pitch, roll).  Returns a dict of the wanted CLOUD_OUTPUTS [total](, k) -- range (t), pixel
        (y * width + x), frame, instance, triangle, position (world), local (apply_lre(pose, position): the sensor's own frame; local[:, 2]
        is the G-buffer's depth), normal, uv, each the G-buffer plane's bits -- plus offsets, int64 [frames + 1]: frame i's points are
        offsets[i]:offsets[i + 1].  torch tensors on the current device, enqueued on `stream` with one host read of the total per
        RT_MAX_BATCH frames -- or numpy arrays with as_numpy=True."""


class Camera:
    def __init__(self, width, height, K, D):
        self.width, self.height = int(width), int(height)
        self.h = libs()[1].rth_camera_create(self.width, self.height, _fp(_fa(K)), _fp(_fa(D)))
        if not self.h:
            raise RtError("camera creation failed")

    def set_pose(self, pose):
        libs()[1].rth_camera_set_pose(self.h, _fp(_fa(pose)))

    def set_stream(self, stream):
        libs()[1].rth_camera_set_stream(self.h, stream)

    def params(self):
        p = RtCameraParams()
        libs()[1].rth_camera_params(self.h, C.addressof(p))
        return p

    def current_pose(self):
        return list(self.params().camera_pose)

    def rays(self, as_numpy=False, stream=None):
        """(origins, directions) float32 [height, width, 3] of every pixel's primary ray, exactly as the render kernels make it
        (raycast.cu:156-188; rt_camera_rays): torch tensors on the current device, allocated and enqueued on `stream` (default the
        current torch stream) without a synchronise -- or numpy arrays with as_numpy=True."""
        p = self.params()
        shape = (self.height, self.width, 3)
        with _staging(not as_numpy, stream) as sg:
            o, d = sg.alloc(shape, np.float32), sg.alloc(shape, np.float32)
            check(libs()[0].rt_camera_rays(C.byref(p), sg.ptr(o), sg.ptr(d), sg.stream, sg.sync), "rt_camera_rays")
            return sg.result(o), sg.result(d)

    GBUFFER_OUTPUTS = _GBUFFER_OUTPUTS                                  # the fields of RtGBuffer

    def render_gbuffer(self, scene, poses=None, outputs=("t", "instance", "triangle"), image=False, stream=None, as_numpy=False):
        """G-buffer frames of this camera (rt_render_gbuffer; the rule is in include/rt_hip.h): what every pixel's primary ray hits, bit
        for bit what Scene.trace_rays gives for Camera.rays(), rendered by the primary kernel in one launch per RT_MAX_BATCH frames.
        poses: None = the camera's current pose (one frame), or a sequence of any length of (x, y, z, yaw, pitch, roll).  Returns a
        dict of the wanted GBUFFER_OUTPUTS -- t, depth [count, h, w] float32 (world distance to the hit; apply_lre(pose, location).z;
        FLT_MAX on a miss), instance, triangle [count, h, w] int32 (-1 on a miss), location, normal [count, h, w, 3] and uv
        [count, h, w, 2] float32 (0 on a miss) -- plus "image" [count, h, w, 3] uint8, the frames of render_scene, with image=True
        (`outputs` may then be empty).  torch tensors on the current device, allocated and enqueued on `stream` (a torch.cuda.Stream
        or a raw hipStream_t; default the current torch stream) without a synchronise -- or numpy arrays with as_numpy=True."""
        return _render_gbuffer(libs()[1].rth_camera_render_gbuffer, "Camera::render_gbuffer", self, scene, poses, outputs, image, stream, as_numpy)

    VISIBILITY_OUTPUTS = _VISIBILITY_OUTPUTS

    def render_visibility(self, scene, points, poses=None, bias=2.0 ** -10, outputs=("visible",), gbuffer=(), image=False, stream=None,
                          as_numpy=False):
        return _render_gbuffer(libs()[1].rth_camera_render_gbuffer, "Camera::render_gbuffer", self, scene, poses, gbuffer, image, stream, as_numpy,
                               visibility=(points, bias, outputs))
    render_visibility.__doc__ = _RENDER_VISIBILITY_DOC % "camera"

    CLOUD_OUTPUTS = _CLOUD_OUTPUTS                                      # the fields of RtPointCloud

    def point_cloud(self, scene, poses=None, outputs=("local", "range", "pixel"), min_range=0.0, max_range=math.inf, mask=None,
                    stream=None, as_numpy=False):
        return _point_cloud(libs()[1].rth_camera_point_cloud_offsets, "Camera::point_cloud_offsets", self, scene, poses, outputs, min_range,
                            max_range, mask, stream, as_numpy)
    point_cloud.__doc__ = _POINT_CLOUD_DOC % ("this camera's", "")

    def directions(self, as_numpy=False, stream=None):
        """float32 [height, width, 3]: the camera-space direction of every pixel (rt_camera_directions; +y the optical axis, +x image
        right, +z image up).  Sensor(camera.directions()) reproduces this camera bit for bit.  torch or numpy as rays()."""
        with _staging(not as_numpy, stream) as sg:
            d = sg.alloc((self.height, self.width, 3), np.float32)
            check(libs()[1].rth_camera_directions(self.h, sg.ptr(d), sg.stream, sg.sync), "Camera::directions")
            return sg.result(d)

    def render_scene(self, scene, d_img, pitch, synchronize=False):
        check(libs()[1].rth_camera_render_scene(self.h, scene.h, d_img, pitch, 1 if synchronize else 0), "Camera::render_scene")

    def prepared_render(self, scene, pose, d_img, pitch):
        """A zero-argument callable for `camera.pose = pose; camera.render_scene(scene, d_img, pitch)` -- the reference's own
        per-frame calls (kernel.cu:275-278) -- with the ctypes arguments built once."""
        host, cam_h, scene_h = libs()[1], self.h, scene.h
        P = _fa(pose)
        Pp, ptr = _fp(P), _vp(int(d_img))
        set_pose, render = host.rth_camera_set_pose, host.rth_camera_render_scene

        def call():
            set_pose(cam_h, Pp)
            rc = render(cam_h, scene_h, ptr, pitch, 0)
            if rc:
                check(rc, "Camera::render_scene")
        call._keep = (P,)
        return call

    def render_scene_stripes(self, scene, d_local, local_pitch, stripe_rows, rank, num_ranks, synchronize=False):
        check(libs()[1].rth_camera_render_scene_stripes(self.h, scene.h, d_local, local_pitch, stripe_rows, rank, num_ranks,
                                                        1 if synchronize else 0), "Camera::render_scene_stripes")

    def render_scene_tiled(self, scene, comm, d_img, pitch, synchronize=False, stripe_rows=16, root=0):
        """Camera::render_scene_tiled: every rank of `comm` calls this; the frame arrives in d_img on `root`."""
        check(libs()[1].rth_camera_render_scene_tiled(self.h, scene.h, comm.h, d_img, pitch, stripe_rows, root, 1 if synchronize else 0),
              "Camera::render_scene_tiled")

    def set_options(self, spp=1, bounces=0, lighting=0):
        libs()[1].rth_camera_set_options(self.h, spp, bounces, 1 if lighting else 0)

    def render_scene_ex(self, scene, d_img, pitch, d_total_pops=None, synchronize=False):
        check(libs()[1].rth_camera_render_scene_ex(self.h, scene.h, d_img, pitch, d_total_pops, 1 if synchronize else 0),
              "Camera::render_scene_ex")

    def render_scene_batch(self, scene, poses, d_imgs, pitch, synchronize=False):
        """frames along a camera path in one launch: poses[i] -> d_imgs[i] (device pointers)"""
        n, P, ptrs = _pose_batch(poses, d_imgs)
        check(libs()[1].rth_camera_render_scene_batch(self.h, scene.h, _fp(P), ptrs, pitch, n, 1 if synchronize else 0),
              "Camera::render_scene_batch")

    def prepared_batch(self, scene, poses, d_ptrs, pitch, stripes=None):
        """A zero-argument callable that issues one batched launch with pre-built ctypes arguments (the per-call Python
        overhead matters when a rank's share of a frame takes tens of microseconds).  stripes = (stripe_rows, rank,
        num_ranks) renders this rank's stripes, (stripe_rows, rank, num_ranks, first_frame) with the stripe owner rotating over
        the frames (frame i renders owner (rank + first_frame + i) % num_ranks), None renders whole frames."""
        n, P, ptrs = _pose_batch(poses, d_ptrs)
        host, cam_h, scene_h, Pp = libs()[1], self.h, scene.h, _fp(P)
        if stripes is None:
            fn = host.rth_camera_render_scene_batch

            def call():
                rc = fn(cam_h, scene_h, Pp, ptrs, pitch, n, 0)
                if rc:
                    check(rc, "Camera::render_scene_batch")
        elif len(stripes) == 4:
            fn = host.rth_camera_render_scene_stripes_batch_rotating
            sr, rk, nr, first = stripes

            def call():
                rc = fn(cam_h, scene_h, Pp, ptrs, pitch, n, sr, rk, nr, first, 0)
                if rc:
                    check(rc, "Camera::render_scene_stripes_batch (rotating owner)")
        else:
            fn = host.rth_camera_render_scene_stripes_batch
            sr, rk, nr = stripes

            def call():
                rc = fn(cam_h, scene_h, Pp, ptrs, pitch, n, sr, rk, nr, 0)
                if rc:
                    check(rc, "Camera::render_scene_stripes_batch")
        call._keep = (P, ptrs)
        return call

    def render_scene_stripes_batch(self, scene, poses, d_locals, local_pitch, stripe_rows, rank, num_ranks, synchronize=False, rotate_first=None):
        n, P, ptrs = _pose_batch(poses, d_locals)
        if rotate_first is not None:
            check(libs()[1].rth_camera_render_scene_stripes_batch_rotating(self.h, scene.h, _fp(P), ptrs, local_pitch, n, stripe_rows, rank,
                                                                           num_ranks, rotate_first, 1 if synchronize else 0),
                  "Camera::render_scene_stripes_batch (rotating owner)")
            return
        check(libs()[1].rth_camera_render_scene_stripes_batch(self.h, scene.h, _fp(P), ptrs, local_pitch, n, stripe_rows, rank,
                                                              num_ranks, 1 if synchronize else 0), "Camera::render_scene_stripes_batch")

    def close(self):
        if self.h:
            libs()[1].rth_camera_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sensor:
    """A sensor that is not the pinhole camera: one camera-space direction per pixel, [h, w, 3] float32, numpy or torch (+y the
    optical axis, +x image right, +z image up; any length; see "sensor frames" in include/rt_hip.h and the generators in
    sensors.py).  Holds a device-resident ray table; immutable, usable by any number of scenes, streams and threads."""

    def __init__(self, directions):
        d = directions.detach().cpu().numpy() if hasattr(directions, "detach") else np.asarray(directions)
        if d.ndim != 3 or d.shape[2] != 3 or d.shape[0] < 1 or d.shape[1] < 1 or d.dtype != np.float32:
            raise ValueError("directions must be float32 [height, width, 3], got %s %s" % (d.dtype, d.shape))
        d = np.ascontiguousarray(d)
        self.height, self.width = int(d.shape[0]), int(d.shape[1])
        self._pose = [0.0] * 6
        self.h = _vp()
        check(libs()[1].rth_sensor_create(_fp(d), self.width, self.height, C.byref(self.h)), "Sensor")

    def set_pose(self, pose):
        self._pose = [float(v) for v in _fa(pose).reshape(6)]

    def current_pose(self):
        return list(self._pose)

    def rays(self, pose=None, as_numpy=False, stream=None):
        """(origins, directions) float32 [height, width, 3] of every pixel's ray under `pose` (default: the set pose), as
        rt_ray_table_rays makes them: what render_gbuffer casts.  torch or numpy as Camera.rays()."""
        P = _fa(self._pose if pose is None else pose)
        if P.shape != (6,):
            raise ValueError("pose must be (x, y, z, yaw, pitch, roll), got shape %s" % (P.shape,))
        host = libs()[1]
        shape = (self.height, self.width, 3)
        with _staging(not as_numpy, stream) as sg:
            o, d = sg.alloc(shape, np.float32), sg.alloc(shape, np.float32)
            check(host.rth_sensor_rays(self.h, _fp(P), sg.ptr(o), sg.ptr(d), sg.stream, sg.sync), "Sensor::rays")
            return sg.result(o), sg.result(d)

    GBUFFER_OUTPUTS = _GBUFFER_OUTPUTS

    def render_gbuffer(self, scene, poses=None, outputs=("t", "instance", "triangle"), image=False, stream=None, as_numpy=False):
        """Camera.render_gbuffer for this sensor (rt_render_gbuffer_table): every plane but depth is, bit for bit, what
        Scene.trace_rays gives for rays(pose); "image" is the flat shade of that hit, the sky colour on a miss."""
        return _render_gbuffer(libs()[1].rth_sensor_render_gbuffer, "Sensor::render_gbuffer", self, scene, poses, outputs, image, stream, as_numpy)

    VISIBILITY_OUTPUTS = _VISIBILITY_OUTPUTS

    def render_visibility(self, scene, points, poses=None, bias=2.0 ** -10, outputs=("visible",), gbuffer=(), image=False, stream=None,
                          as_numpy=False):
        return _render_gbuffer(libs()[1].rth_sensor_render_gbuffer, "Sensor::render_gbuffer", self, scene, poses, gbuffer, image, stream, as_numpy,
                               visibility=(points, bias, outputs))
    render_visibility.__doc__ = _RENDER_VISIBILITY_DOC % "sensor"

    CLOUD_OUTPUTS = _CLOUD_OUTPUTS

    def point_cloud(self, scene, poses=None, outputs=("local", "range", "pixel"), min_range=0.0, max_range=math.inf, mask=None,
                    stream=None, as_numpy=False):
        return _point_cloud(libs()[1].rth_sensor_point_cloud_offsets, "Sensor::point_cloud_offsets", self, scene, poses, outputs, min_range,
                            max_range, mask, stream, as_numpy)
    point_cloud.__doc__ = _POINT_CLOUD_DOC % ("this sensor's", "_table")

    ROLLING_OUTPUTS = _GBUFFER_OUTPUTS + ("local",)

    def render_rolling(self, scene, poses, axis="x", slice_pixels=8, outputs=("t", "instance", "triangle"), image=False, stream=None,
                       as_numpy=False):
        """Rolling frames (rt_render_gbuffer_rolling, "rolling frames" in include/rt_hip.h): render_gbuffer with a pose per SLICE of
        slice_pixels columns (axis "x": a spinning lidar's revolution) or rows (axis "y": a rolling shutter) -- slice_pixels a
        multiple of 8, the last slice may be narrower.  poses: [n, slices, 6], slices = ceil(extent / slice_pixels); see
        sensors.rolling_poses.  outputs: any of ROLLING_OUTPUTS -- the G-buffer planes, each what Scene.trace_rays gives for
        rays(pose of the pixel's slice), plus "local" [n, h, w, 3]: the hit in the sensor's frame at the moment its slice was taken
        (the raw, motion-distorted scan; "location" is the de-skewed truth), local[..., 2] == depth.  n is cut into launches of
        RT_MAX_BATCH frames; always plain records (no view slot).  Every ValueError is raised before a device call."""
        outputs = tuple(outputs)
        if [o for o in outputs if o not in Sensor.ROLLING_OUTPUTS] or len(set(outputs)) != len(outputs) or not (outputs or image):
            raise ValueError("outputs must be a subset of %s (non-empty unless image=True), nothing twice, got %r" % (Sensor.ROLLING_OUTPUTS, outputs))
        P, ax, slices = _rolling_args(self, poses, axis, slice_pixels)
        n, h, w = int(P.shape[0]), self.height, self.width
        if n * h * w > 2 ** 31 - 1:
            raise ValueError("at most 2^31 - 1 pixels per call, got %d frames of %d x %d" % (n, w, h))
        hip, host = libs()
        kinds = dict(_FIELDS, local=((3,), np.float32))
        with _staging(not as_numpy, stream) as sg:
            out = {k: sg.alloc((n, h, w) + kinds[k][0], kinds[k][1]) for k in outputs}
            img = sg.alloc((n, h, w, 3), np.uint8) if image else None
            ws_bytes = int(hip.rt_rolling_workspace_bytes(min(n, RT_MAX_BATCH), slices))
            spaces = []                                                 # (one workspace per launch: each stays untouched until its render has run)
            for first in range(0, n, RT_MAX_BATCH):
                m = min(RT_MAX_BATCH, n - first)
                at = {k: sg.ptr(a) for k, a in out.items()}
                at = {k: (v.value if isinstance(v, _vp) else int(v)) + first * h * w * math.prod(kinds[k][0]) * 4 for k, v in at.items()}
                planes = RtGBuffer(*[at.get(k) for k in _GBUFFER_OUTPUTS])
                ptrs = None
                if image:
                    base = sg.ptr(img)
                    base = base.value if isinstance(base, _vp) else int(base)
                    ptrs = (_vp * m)(*[base + (first + i) * h * w * 3 for i in range(m)])
                spaces.append(sg.alloc((ws_bytes,), np.uint8))
                check(host.rth_sensor_render_rolling(self.h, scene.h, _fp(P[first:first + m]), m, slices, ax, int(slice_pixels), C.byref(planes),
                                                     at.get("local"), ptrs, w * 3, sg.ptr(spaces[-1]), ws_bytes, sg.stream, sg.sync),
                      "Sensor::render_rolling")
            res = {k: sg.result(a) for k, a in out.items()}
            if image:
                res["image"] = sg.result(img)
            return res

    def rolling_point_cloud(self, scene, poses, axis="x", slice_pixels=8, outputs=("local", "range", "pixel"), min_range=0.0,
                            max_range=math.inf, mask=None, stream=None, as_numpy=False):
        """point_cloud for rolling frames (rt_point_cloud_offsets_rolling + rt_point_cloud_fill_rolling): poses, axis and slice_pixels
        as render_rolling takes them, everything else as point_cloud.  `local` is in the sensor's frame at the moment each point's
        slice was taken -- the raw, motion-distorted scan a driver delivers -- `position` the de-skewed truth in the world."""
        return _point_cloud(libs()[1].rth_sensor_point_cloud_offsets_rolling, "Sensor::point_cloud_offsets_rolling", self, scene, poses, outputs,
                            min_range, max_range, mask, stream, as_numpy, rolling=(axis, slice_pixels))

    def close(self):
        if getattr(self, "h", None):
            libs()[1].rth_sensor_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RtComm: the RCCL communicator behind rt_gather / rt_all_to_all / rt_render_tiled (one process per GPU).
    Comm.unique_id() on one rank -> the 128 bytes travel to the others by the host's own means -> Comm(id, rank, n)."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        check(libs()[0].rt_comm_unique_id(buf), "rt_comm_unique_id")
        return bytes(buf)

    def __init__(self, unique_id, rank, num_ranks):
        self.h = _vp()
        self.rank, self.num_ranks = rank, num_ranks
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        check(libs()[0].rt_comm_init_rank(buf, rank, num_ranks, C.byref(self.h)), "rt_comm_init_rank")

    @classmethod
    def init_all(cls, devices):
        """rt_comm_init_all: one process drives every device; returns one Comm per entry of `devices` (rank i on devices[i]).
        Collectives of several of them issued from one thread must sit between group_start() and group_end()."""
        n = len(devices)
        handles = (_vp * n)()
        check(libs()[0].rt_comm_init_all((C.c_int32 * n)(*devices), n, handles), "rt_comm_init_all")
        out = []
        for r in range(n):
            c = cls.__new__(cls)
            c.h, c.rank, c.num_ranks = _vp(handles[r]), r, n
            out.append(c)
        return out

    def info(self):
        """(rank, num_ranks, device) as the RCCL communicator itself reports them (rt_comm_info)."""
        r, n, d = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        check(libs()[0].rt_comm_info(self.h, C.byref(r), C.byref(n), C.byref(d)), "rt_comm_info")
        return r.value, n.value, d.value

    @staticmethod
    def last_error():
        e = libs()[0].rt_comm_last_error()
        return e.decode(errors="replace") if e else ""

    @staticmethod
    def last_error_any():
        """The most recent RT_E_COMM text of ANY thread (rt_comm_last_error() is the calling thread's own): what a watchdog
        thread reports about a main thread stuck in a collective."""
        e = libs()[0].rt_comm_last_error_any()
        return e.decode(errors="replace") if e else ""

    @staticmethod
    def group_start():
        check(libs()[0].rt_group_start(), "rt_group_start")

    @staticmethod
    def group_end():
        check(libs()[0].rt_group_end(), "rt_group_end")

    def gather(self, d_send, nbytes, d_recv, root=0, stream=None):
        check(libs()[0].rt_gather(self.h, d_send, nbytes, d_recv, root, stream), "rt_gather")

    def all_to_all_plan(self, send_bytes, send_offsets, recv_bytes, recv_offsets):
        """The four size arrays of rt_all_to_all as ctypes arrays, for calls repeated with the same layout."""
        arr = lambda v: (C.c_size_t * self.num_ranks)(*[int(x) for x in v])
        return arr(send_bytes), arr(send_offsets), arr(recv_bytes), arr(recv_offsets)

    def all_to_all_planned(self, d_send, d_recv, plan, stream=None):
        rc = libs()[0].rt_all_to_all(self.h, d_send, plan[0], plan[1], d_recv, plan[2], plan[3], stream)
        if rc:
            check(rc, "rt_all_to_all")

    def all_to_all(self, d_send, send_bytes, send_offsets, d_recv, recv_bytes, recv_offsets, stream=None):
        self.all_to_all_planned(d_send, d_recv, self.all_to_all_plan(send_bytes, send_offsets, recv_bytes, recv_offsets), stream)

    def close(self):
        if self.h:
            libs()[0].rt_comm_destroy(self.h)
            self.h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """A device allocation made through the C-ABI (rt_malloc / rt_malloc_pitch)."""

    def __init__(self, nbytes=None, width_bytes=None, height=None):
        h = libs()[0]
        self.ptr = _vp()
        if nbytes is not None:
            check(h.rt_malloc(C.byref(self.ptr), nbytes), "rt_malloc")
            self.pitch, self.nbytes = None, nbytes
        else:
            pitch = C.c_size_t(0)
            check(h.rt_malloc_pitch(C.byref(self.ptr), C.byref(pitch), width_bytes, height), "rt_malloc_pitch")
            self.pitch, self.nbytes = pitch.value, pitch.value * height
        self.width_bytes, self.height = width_bytes, height

    def to_host(self, dtype=np.uint8):
        h = libs()[0]
        if self.pitch is None:
            out = np.zeros(self.nbytes // np.dtype(dtype).itemsize, dtype)
            check(h.rt_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes, None), "rt_memcpy_d2h")
            return out
        out = np.zeros((self.height, self.width_bytes), np.uint8)
        check(h.rt_memcpy2d_d2h(out.ctypes.data, self.width_bytes, self.ptr, self.pitch, self.width_bytes, self.height, None),
              "rt_memcpy2d_d2h")
        return out

    def free(self):
        if self.ptr:
            libs()[0].rt_free(self.ptr)
            self.ptr = _vp()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# Whether Scene.trace_rays / occluded sort the rays by direction octant before tracing when the caller does not say (binning=None).
# Off: tools/ray_query_bench.py measured the sort winning 1.4-1.6 x on shuffled and random rays but costing 11-36 % on camera rays in
# pixel order and 19 % on shadow rays from a frame's hits (DESIGN.md "Ray queries"); callers with incoherent rays pass binning=True.
TRACE_BINNING = False


def _trace_workspace(binning):
    """The scratch request of Scene.trace_rays / occluded to _device_query: (h, n) -> the bytes rt_trace_workspace_bytes wants when
    the rays are binned (binning=None: TRACE_BINNING as it is at the call), 0 otherwise"""
    if binning is None:
        binning = TRACE_BINNING
    return lambda h, n: h.rt_trace_workspace_bytes(n) if binning and n > 0 else 0


# name -> (trailing shape, dtype) of every field a query returns, per query or per list slot: the same in every struct that has it
# (but `inside`: a region's number of wholly-inside pairs here, a pair's flag in the region lists, which say so in their _ListKind)
_FIELDS = dict(
    t=((), np.float32), depth=((), np.float32), distance=((), np.float32), sdf=((), np.float32), instance=((), np.int32), triangle=((), np.int32),
    count=((), np.int32), winding=((), np.int32), pops=((), np.int32), sign=((), np.int8), occluded=((), np.uint8),
    any=((), np.bool_), occupied=((), np.bool_), barycentric=((2,), np.float32), uv=((2,), np.float32), location=((3,), np.float32),
    point=((3,), np.float32), normal=((3,), np.float32), segment=((2, 3), np.float32), parameter=((), np.float32),
    segment_point=((3,), np.float32), crossings=((), np.int32), clearance=((), np.float32), within=((), np.int32),
    query_barycentric=((2,), np.float32), query_point=((3,), np.float32), intersections=((), np.int32), inside=((), np.int32),
    time=((), np.float32), centre=((3,), np.float32), contact_normal=((3,), np.float32), hit=((), np.int32))


def _check_outputs(outputs, allowed, extras=()):
    """`outputs` as a tuple: a non-empty choice of `allowed`, plus any of `extras` (where there are extras, nothing twice)"""
    outputs = tuple(outputs)
    chosen = [o for o in outputs if o not in extras]
    if not chosen or [o for o in chosen if o not in allowed] or (extras and len(set(outputs)) != len(outputs)):
        raise ValueError("outputs must be a non-empty subset of %s%s, got %r"
                         % (allowed, ", optionally with " + " and ".join(extras) if extras else "", outputs))
    return outputs


def _check_max_hits(max_hits):
    """max_hits of the list queries: None (CSR) or the room per query as an int"""
    if max_hits is None:
        return None
    if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)) or not 1 <= int(max_hits) <= 2 ** 31 - 1:
        raise ValueError("max_hits must be None or an int in [1, 2^31 - 1], got %r" % (max_hits,))
    return int(max_hits)


def _query_inputs(inputs, shape=(3,), ints=()):
    """The argument checks of every query (_device_query, _list_query), before any device call -> (torch_in, leading shape, n,
    device).  inputs: (name, array) pairs, the first [..., *shape] (default [..., 3]), "directions" of the same shape, the others of
    the leading shape; None = not given.  Every input is float32 except those named in `ints`, which are int32."""
    given = [(k, a) for k, a in inputs if a is not None]
    torch_in = type(given[0][1]).__module__.split(".")[0] == "torch"
    if any((type(a).__module__.split(".")[0] == "torch") != torch_in for _k, a in given):
        raise ValueError("%s must all be torch tensors or all numpy arrays" % ", ".join(k for k, _a in given))
    if not torch_in and not all(isinstance(a, np.ndarray) for _k, a in given):
        raise ValueError("%s must be numpy arrays or torch tensors" % ", ".join(k for k, _a in given))
    for name, a in given:
        want = "int32" if name in ints else "float32"
        if str(a.dtype) not in (want, "torch." + want):
            raise ValueError("%s must be %s, got %s" % (name, want, a.dtype))
        contiguous = a.is_contiguous() if torch_in else a.flags["C_CONTIGUOUS"]
        if not contiguous:
            raise ValueError("%s must be contiguous" % name)
    first, a0 = given[0]
    nd = len(a0.shape) - len(shape)
    if nd < 0 or tuple(a0.shape[nd:]) != tuple(shape):
        raise ValueError("%s must have the shape [..., %s], got %s" % (first, ", ".join(str(x) for x in shape), tuple(a0.shape)))
    lead = tuple(a0.shape[:nd])
    for name, a in inputs[1:]:
        if a is None:
            continue
        want = tuple(a0.shape) if name == "directions" else lead
        if tuple(a.shape) != want:
            raise ValueError("%s must have the shape %s, got %s" % (name, want, tuple(a.shape)))
    n = math.prod(lead)
    if n > 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 1 queries per call, got %d" % n)
    dev = None
    if torch_in:
        import torch
        for name, a in given:
            if not a.is_cuda:
                raise ValueError("%s is on %s: torch inputs must be on the scene's GPU" % (name, a.device))
        dev = torch.device("cuda", torch.cuda.current_device())
        for name, a in given:
            if a.device != dev:
                raise ValueError("%s is on %s, the scene's device is %s" % (name, a.device, dev))
    return torch_in, lead, n, dev


def _staging(torch_form, stream, dev=None):
    """The staging of one "arrays in, arrays out" call (the queries, Camera.rays): a context manager in a torch and a numpy form with
    stream / sync (what the C-ABI call is given), inputs(arrays) -> device pointers (None stays None), alloc(shape, dtype, zero=False)
    -> an output or scratch array, ptr(array), read_int64(array, i) -> that element on the host, result(array) -> what the caller
    gets, and run_index / run_lengths on the result of a CSR offsets array.  Leaving it frees what it made, on every exit path."""
    return _TorchStaging(stream, dev) if torch_form else _HostStaging(stream)


class _TorchStaging:
    """Tensors in, tensors out, no host synchronisation but read_int64's.  `stream`: None (the current stream), a torch.cuda.Stream or
    a raw hipStream_t.  It is the current stream inside the context, so every tensor made here is allocated under the stream of the
    kernels that use it: the caching allocator reuses a freed tensor's memory in that stream's order only, so nothing has to be
    recorded on another stream and the caller may drop a result at any time."""
    sync = 0
    _dtypes = None                              # numpy type, as _FIELDS and the callers name it -> torch dtype; made by the first call

    def __init__(self, stream, dev):
        import torch
        self.torch = torch
        if self._dtypes is None:
            _TorchStaging._dtypes = {t: getattr(torch, np.dtype(t).name) for t in {dt for _tr, dt in _FIELDS.values()} | {np.int64}}
        self.dev = dev if dev is not None else torch.device("cuda", torch.cuda.current_device())
        ts = torch.cuda.current_stream() if stream is None else stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(stream)
        self.stream = ts.cuda_stream
        self._current = None if stream is None else torch.cuda.stream(ts)

    def __enter__(self):
        if self._current is not None:
            self._current.__enter__()
        return self

    def __exit__(self, *exc):
        if self._current is not None:
            self._current.__exit__(*exc)

    def inputs(self, arrays):
        return [None if a is None else a.data_ptr() for a in arrays]

    def alloc(self, shape, dtype, zero=False):
        make = self.torch.zeros if zero else self.torch.empty
        return make(shape, dtype=self._dtypes[dtype], device=self.dev)

    def ptr(self, a):
        return a.data_ptr()

    def read_int64(self, a, i):
        return int(a[i].item())

    def result(self, a):
        return a

    def run_index(self, offsets, total):
        torch = self.torch
        return torch.repeat_interleave(torch.arange(len(offsets) - 1, dtype=torch.int32, device=self.dev), offsets[1:] - offsets[:-1],
                                       output_size=total)

    def run_lengths(self, offsets):
        return (offsets[1:] - offsets[:-1]).to(self.torch.int32)


class _HostStaging:
    """numpy arrays in, numpy arrays out: inputs are copied to device buffers, the C-ABI call synchronises, results are copied back.
    An array here is (DeviceBuffer, shape, dtype)."""
    sync = 1

    def __init__(self, stream):
        self.stream, self._made = stream, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self._made:
            b.free()

    def _buffer(self, host=None, nbytes=0):
        """a device buffer of nbytes, or with the contents of the host array"""
        nbytes = nbytes if host is None else host.nbytes
        b = DeviceBuffer(nbytes=max(nbytes, 1))
        self._made.append(b)
        if nbytes and host is not None:
            check(libs()[0].rt_memcpy_h2d(b.ptr, host.ctypes.data, nbytes, self.stream), "rt_memcpy_h2d")
        return b

    def inputs(self, arrays):
        return [None if a is None else self._buffer(a).ptr for a in arrays]

    def alloc(self, shape, dtype, zero=False):
        dtype = np.dtype(dtype)
        if zero:
            return self._buffer(np.zeros(shape, dtype)), tuple(shape), dtype
        return self._buffer(nbytes=math.prod(shape) * dtype.itemsize), tuple(shape), dtype

    def ptr(self, a):
        return a[0].ptr

    def read_int64(self, a, i):
        v = np.zeros(1, np.int64)
        check(libs()[0].rt_memcpy_d2h(v.ctypes.data, a[0].ptr.value + 8 * i, 8, None), "rt_memcpy_d2h")
        return int(v[0])

    def result(self, a):
        b, shape, dtype = a
        size = math.prod(shape)
        return b.to_host(dtype)[:size].reshape(shape) if size else np.zeros(shape, dtype)

    def run_index(self, offsets, total):            # (total: what the torch form needs to stay asynchronous; np.repeat finds it)
        return np.repeat(np.arange(len(offsets) - 1, dtype=np.int32), np.diff(offsets))

    def run_lengths(self, offsets):
        return np.diff(offsets).astype(np.int32)


class _ListKind:
    """What _list_query needs of one list query: the slot fields in struct order, the key fields (always filled: the room keeps them),
    the struct (slot fields, then the per-query fields `tail`), the three C-ABI calls and the name of the per-slot query index of the
    CSR form"""

    def __init__(self, names, keys, struct, ws, offsets, fill, index, inputs=None, extra=(), types=None):
        self.names, self.keys, self.struct = names, keys, struct
        self.tail = tuple(f for f, _t in struct._fields_[len(names):])
        self.ws, self.offsets, self.fill, self.index = ws, offsets, fill, index
        self.inputs = inputs or {}              # _query_inputs' shape / ints when they are not the defaults
        self.extra = tuple(extra)               # integers the offsets and the fill call take after n (a region's plane count)
        self.types = dict(_FIELDS, **(types or {}))     # a slot field whose type is not the per-query field's of that name


def _list_query(scene, kind, inputs, max_hits, outputs, stream, per_query=None):
    """Scene.list_crossings / list_nearby / list_intersecting: every argument is checked before any device call (_query_inputs).
    inputs: (name, array) pairs in the C-ABI's order.  The key fields are always filled (the room keeps the keys, so the kernel inserts
    rather than selects); the ones not wanted are dropped.  per_query: the fields of kind.tail the kernel fills ([...] int32 each,
    returned); None: those named in outputs, `count` in fixed rooms only.  In CSR form `count` is taken from the offsets when the
    kernel does not fill it."""
    torch_in, lead, n, dev = _query_inputs(inputs, **kind.inputs)
    csr = max_hits is None
    if per_query is None:
        per_query = tuple(k for k in kind.tail if k in outputs and not (csr and k == "count"))
    h = libs()[0]
    handle = scene.device_handle
    fields = tuple(k for k in kind.names if k in outputs or k in kind.keys)
    with _staging(torch_in, stream, dev) as sg:
        ins = sg.inputs([a for _k, a in inputs])
        tail = {k: sg.alloc(lead, np.int32) for k in per_query}
        offsets = None
        if csr:
            offsets = sg.alloc((n + 1,), np.int64, zero=n == 0)     # (rt_*_offsets writes all n + 1 entries, or nothing when n is 0)
            ws_bytes = max(int(getattr(h, kind.ws)(n)), 1)
            ws = sg.alloc((ws_bytes,), np.uint8)
            check(getattr(h, kind.offsets)(handle, *ins, n, *kind.extra, sg.ptr(offsets), sg.ptr(ws), ws_bytes, sg.stream, sg.sync),
                  kind.offsets)
            rows = (sg.read_int64(offsets, n),)                     # torch: the one host synchronisation, for the size of the outputs
        else:
            rows = lead + (max_hits,)
        out = {k: sg.alloc(rows + kind.types[k][0], kind.types[k][1]) for k in fields}
        lst = kind.struct(*[sg.ptr(out[k]) if k in out else None for k in kind.names],
                          *[sg.ptr(tail[k]) if k in tail else None for k in kind.tail])
        check(getattr(h, kind.fill)(handle, *ins, n, *kind.extra, sg.ptr(offsets) if csr else None, 0 if csr else max_hits, C.byref(lst),
                                    sg.stream, sg.sync), kind.fill)
        res = {k: sg.result(out[k]) for k in kind.names if k in outputs}
        res.update({k: sg.result(a) for k, a in tail.items()})
        if csr:
            res["offsets"] = sg.result(offsets)
            res[kind.index] = sg.run_index(res["offsets"], rows[0])
            if "count" not in res:
                res["count"] = sg.run_lengths(res["offsets"]).reshape(lead)
        return res


_CROSSING_LIST = _ListKind(_CROSSING_LIST_OUTPUTS, ("t", "instance", "triangle"), RtCrossingList,
                           "rt_crossing_offsets_workspace_bytes", "rt_crossing_offsets", "rt_list_crossings", "ray")
_NEARBY_LIST = _ListKind(_NEARBY_LIST_OUTPUTS, ("distance", "instance", "triangle"), RtNearbyList,
                         "rt_nearby_offsets_workspace_bytes", "rt_nearby_offsets", "rt_list_nearby", "point_index")
_TRIANGLE_INPUTS = dict(shape=(3, 3), ints=("skip_instance",))
_INTERSECT_LIST = _ListKind(_INTERSECT_LIST_OUTPUTS, ("instance", "triangle"), RtIntersectList,
                            "rt_intersecting_offsets_workspace_bytes", "rt_intersecting_offsets", "rt_list_intersecting", "query_index",
                            inputs=_TRIANGLE_INPUTS)
_BOX_INPUTS = dict(shape=(2, 3))
_BOX_LIST = _ListKind(_BOX_LIST_OUTPUTS, ("instance", "triangle"), RtBoxList,
                      "rt_box_offsets_workspace_bytes", "rt_box_offsets", "rt_list_in_boxes", "query_index", inputs=_BOX_INPUTS)
_SEGMENT_INPUTS = dict(shape=(2, 3))                # (a box array's shape: P0 then P1)
_PLANE_INPUTS = dict(shape=(2, 3))                  # (a box array's shape: point then normal)
_SECTION_LIST = _ListKind(_SECTION_LIST_OUTPUTS, ("instance", "triangle"), RtSectionList,
                          "rt_section_offsets_workspace_bytes", "rt_section_offsets", "rt_list_sections", "query_index",
                          inputs=_PLANE_INPUTS)
REGION_MAX_PLANES = 8                               # RT_REGION_MAX_PLANES of include/rt_hip.h
# one kind per plane count: K is part of the input's shape and an argument of the calls; a slot's inside is a flag, a query's a number
_REGION_LIST = {K: _ListKind(_REGION_LIST_OUTPUTS, ("instance", "triangle"), RtRegionList,
                             "rt_region_offsets_workspace_bytes", "rt_region_offsets", "rt_list_in_regions", "query_index",
                             inputs=dict(shape=(K, 2, 3)), extra=(K,), types=dict(inside=((), np.uint8)))
                for K in range(1, REGION_MAX_PLANES + 1)}


def _region_planes(regions):
    """K of a regions array [..., K, 2, 3], checked before any device call (_query_inputs checks the rest)"""
    shape = tuple(getattr(regions, "shape", ()))
    if len(shape) < 3 or shape[-2:] != (2, 3) or not 1 <= shape[-3] <= REGION_MAX_PLANES:
        raise ValueError("regions must have the shape [..., K, 2, 3] with 1 <= K <= %d, got %s" % (REGION_MAX_PLANES, shape or type(regions)))
    return int(shape[-3])


def _device_query(scene, inputs, outs, call, stream, shape=(3,), ints=(), scratch=None):
    """Every query with one result per query (Scene.trace_rays / occluded / closest_points / count_crossings / winding_numbers /
    signed_distance / count_intersecting): every argument is checked before any device call (_query_inputs, which has the rules for
    inputs, shape and ints).  outs: names of _FIELDS.  call(h, handle, input pointers, output pointers by name, n, stream,
    synchronize) makes the C-ABI call; with scratch, (h, n) -> bytes, it is also given a workspace of that size (None when 0) and
    the size."""
    torch_in, lead, n, dev = _query_inputs(inputs, shape, ints)
    h = libs()[0]
    handle = scene.device_handle
    with _staging(torch_in, stream, dev) as sg:
        ins = sg.inputs([a for _k, a in inputs])
        out = {k: sg.alloc(lead + _FIELDS[k][0], _FIELDS[k][1]) for k in outs}
        ws = ()
        if scratch is not None:
            ws_bytes = scratch(h, n)
            workspace = sg.alloc((ws_bytes,), np.uint8) if ws_bytes else None
            ws = (None if workspace is None else sg.ptr(workspace), ws_bytes)
        call(h, handle, ins, {k: sg.ptr(a) for k, a in out.items()}, n, sg.stream, sg.sync, *ws)
        return {k: sg.result(a) for k, a in out.items()}


def _visibility_options(outputs, bias):
    """Scene.visibility and the render_visibility wrappers: (outputs as a tuple, bias as a float) or a ValueError"""
    outputs = _check_outputs(outputs, _VISIBILITY_OUTPUTS)
    if len(set(outputs)) != len(outputs):
        raise ValueError("outputs must not name a mask twice, got %r" % (outputs,))
    ok = isinstance(bias, (int, float, np.integer, np.floating)) and not isinstance(bias, bool)
    if not ok or not 0.0 <= float(np.float32(bias)) < 1.0:              # (as the C-ABI sees it: a float32; NaN fails both)
        raise ValueError("bias must be a number in [0, 1), got %r" % (bias,))
    return outputs, float(bias)


def _visibility_points(points, n, keep_device=False):
    """`points` as float32 [n, K, 3] with 1 <= K <= 32, from [K, 3] (every frame) or [n, K, 3]: a contiguous numpy array -- or, with
    keep_device, the caller's CUDA tensor in that shape.  Every ValueError before a device call."""
    is_torch = type(points).__module__.split(".")[0] == "torch"
    if is_torch:
        if str(points.dtype) != "torch.float32":
            raise ValueError("points must be float32, got %s" % points.dtype)
        P = points
    else:
        try:
            P = np.asarray(points, np.float32)
        except (TypeError, ValueError):
            raise ValueError("points must be [K, 3] or [n, K, 3] numbers, got %r" % (type(points),))
    shape = tuple(P.shape)
    if len(shape) not in (2, 3) or shape[-1] != 3 or not 1 <= shape[-2] <= 32 or (len(shape) == 3 and shape[0] != n):
        raise ValueError("points must be [K, 3] or [%d, K, 3] with 1 <= K <= 32, got %s" % (n, shape))
    K = int(shape[-2])
    if is_torch and keep_device and P.is_cuda:
        return P.detach().expand(n, K, 3)                               # (_visibility_launch makes it contiguous, on the call's stream)
    if is_torch:
        P = P.detach().cpu().numpy()
    return np.array(np.broadcast_to(P, (n, K, 3)), np.float32, order="C")      # (a copy of the caller's: writable, contiguous)


def _visibility_launch(sg, scene, planes, n, h, w, points, bias, outputs):
    """rth_scene_visibility on staged planes inside the staging `sg`: planes = the device pointers of instance, location and (for
    facing) normal, [n, h, w](x3); points [n, K, 3] as _visibility_points gives them.  -> the staged int32 masks by name."""
    if isinstance(points, np.ndarray):
        if sg.sync:
            d_points = sg.inputs([points])[0]
        else:                                                           # (made under the staging's stream, which orders its reuse)
            points = sg.torch.from_numpy(points).to(sg.dev)
            d_points = points.data_ptr()
    else:
        points = points.contiguous()
        d_points = points.data_ptr()
    out = {k: sg.alloc((n, h, w), np.int32) for k in outputs}
    masks = RtVisibility(*[sg.ptr(out[k]) if k in out else None for k in _VISIBILITY_OUTPUTS])
    check(libs()[1].rth_scene_visibility(scene.h, planes["instance"], planes["location"], planes.get("normal"), w, h, n, d_points,
                                         int(points.shape[1]), bias, C.byref(masks), sg.stream, sg.sync), "Scene::visibility")
    return out


def _xp(a):
    """numpy, or torch for a tensor: the region helpers use only what the two spell alike"""
    if type(a).__module__.split(".")[0] == "torch":
        import torch
        return torch
    return np


def _cross(xp, u, v):
    return xp.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _unit(xp, v):
    return v / xp.sqrt((v * v).sum(-1))[..., None]


def _plane(xp, point, normal):
    return xp.stack([point, normal], -2)


def regions_from_boxes(boxes):
    """World-aligned boxes [..., 2, 3] (lo then hi) as regions [..., 6, 2, 3] for Scene.count_in_regions / list_in_regions: the planes
    x-lo, x-hi, y-lo, y-hi, z-lo, z-hi, each with its point on its own face (the lo corner or the hi corner) and a unit normal
    pointing inward.  numpy in, numpy out; torch in, torch out.  Plain fp32 arithmetic, OUTSIDE the exact contract of rule 15: the
    region is what the planes say, and it is not rule 11's box test (which is decided relative to the box's first corner)."""
    xp = _xp(boxes)
    lo, hi = boxes[..., 0, :], boxes[..., 1, :]
    planes = []
    for a in range(3):
        e = xp.zeros_like(lo)
        e[..., a] = 1.0
        planes += [_plane(xp, lo, e), _plane(xp, hi, -e)]
    return xp.stack(planes, -3)


def regions_from_obbs(centers, axes, half_extents):
    """Oriented boxes as regions [..., 6, 2, 3]: centers [..., 3], axes [..., 3, 3] (row a is the box's a-th axis, a unit vector; the
    three orthogonal), half_extents [..., 3].  The planes come in pairs per axis, at center - h_a*axis_a with normal +axis_a and at
    center + h_a*axis_a with normal -axis_a, each point on its own face.  numpy in, numpy out; torch in, torch out.  Plain fp32
    arithmetic, outside the exact contract of rule 15."""
    xp = _xp(centers)
    planes = []
    for a in range(3):
        u = axes[..., a, :]
        d = half_extents[..., a][..., None] * u
        planes += [_plane(xp, centers - d, u), _plane(xp, centers + d, -u)]
    return xp.stack(planes, -3)


def regions_from_frusta(eyes, corners, near, far):
    """View frusta and selection pyramids as regions [..., 6, 2, 3]: eyes [..., 3]; corners [..., 4, 3], world points the four edges
    of the pyramid pass through, counter-clockwise seen from the eye; near and far, numbers or arrays of the leading shape.  Planes 0-3
    are the sides, each through the eye and two consecutive corner directions d_i = corner_i - eye (normal cross(d_(i+1), d_i),
    which points inward); planes 4 and 5 are the caps at the distances near and far along the normalised mean of the four unit
    directions, with normals along it and against it.  numpy in, numpy out; torch in, torch out.  Plain fp32 arithmetic, outside
    the exact contract of rule 15."""
    xp = _xp(eyes)
    d = [corners[..., i, :] - eyes for i in range(4)]
    planes = [_plane(xp, eyes, _cross(xp, d[(i + 1) % 4], d[i])) for i in range(4)]
    m = _unit(xp, _unit(xp, d[0]) + _unit(xp, d[1]) + _unit(xp, d[2]) + _unit(xp, d[3]))
    near, far = (x[..., None] if len(getattr(x, "shape", ())) else x for x in (near, far))
    planes += [_plane(xp, eyes + near * m, m), _plane(xp, eyes + far * m, -m)]
    out = xp.stack(planes, -3)
    return out.astype(np.float32) if xp is np else out.float()          # (a float64 near or far does not widen the result)


def render_debug(scene, camera):
    """One frame through rt_render_debug -> dict(img[h,w,3], hit_inst, hit_tri, pops, aabb, tris, inside)."""
    h = libs()[0]
    W, H = camera.width, camera.height
    img = DeviceBuffer(width_bytes=W * 3, height=H)
    names = ("hit_inst", "hit_tri", "pops", "aabb", "tris", "inside")
    bufs = [DeviceBuffer(nbytes=W * H * 4) for _ in names]
    planes = RtDebugPlanes(*[b.ptr for b in bufs])
    p = camera.params()
    check(h.rt_render_debug(scene.device_handle, C.byref(p), img.ptr, img.pitch, C.byref(planes), None, 1), "rt_render_debug")
    out = dict(img=img.to_host().reshape(H, W, 3))
    for n, b in zip(names, bufs):
        out[n] = b.to_host(np.int32).reshape(H, W)
        b.free()
    img.free()
    return out


def render_ids(scene, camera):
    """One frame through rt_render_ids (the PRODUCTION kernel plus its hit-id planes) -> dict(img, hit_inst, hit_tri)."""
    h = libs()[0]
    W, H = camera.width, camera.height
    img = DeviceBuffer(width_bytes=W * 3, height=H)
    inst, tri = DeviceBuffer(nbytes=W * H * 4), DeviceBuffer(nbytes=W * H * 4)
    p = camera.params()
    check(h.rt_render_ids(scene.device_handle, C.byref(p), img.ptr, img.pitch, inst.ptr, tri.ptr, None, 1), "rt_render_ids")
    out = dict(img=img.to_host().reshape(H, W, 3), hit_inst=inst.to_host(np.int32).reshape(H, W),
               hit_tri=tri.to_host(np.int32).reshape(H, W))
    for b in (img, inst, tri):
        b.free()
    return out


def render(scene, camera):
    """One frame through Camera::render_scene -> img[h,w,3] uint8 (uchar3 .x .y .z order)."""
    W, H = camera.width, camera.height
    img = DeviceBuffer(width_bytes=W * 3, height=H)
    camera.render_scene(scene, img.ptr, img.pitch, synchronize=True)
    out = img.to_host().reshape(H, W, 3)
    img.free()
    return out


def render_ex(scene, camera):
    """One extension frame (camera.set_options) -> dict(img[h,w,3], total_pops[h,w])."""
    W, H = camera.width, camera.height
    img = DeviceBuffer(width_bytes=W * 3, height=H)
    pops = DeviceBuffer(nbytes=W * H * 4)
    camera.render_scene_ex(scene, img.ptr, img.pitch, pops.ptr, synchronize=True)
    out = dict(img=img.to_host().reshape(H, W, 3), total_pops=pops.to_host(np.int32).reshape(H, W))
    img.free()
    pops.free()
    return out


def read_image(path):
    """PNG / baseline JPEG / binary PPM file -> [h, w, 3] uint8 B,G,R (the decoders behind Material::upload_texture)."""
    w, h = C.c_int32(0), C.c_int32(0)
    host = libs()[1]
    rc = host.rth_read_image_bgr(os.fsencode(path), None, 0, C.byref(w), C.byref(h))
    if rc:
        raise RtError("read_image(%s): %s" % (path, host.rth_last_error().decode()))
    out = np.empty((h.value, w.value, 3), np.uint8)
    check(host.rth_read_image_bgr(os.fsencode(path), out.ctypes.data, out.nbytes, C.byref(w), C.byref(h)), "read_image")
    return out


def write_png(path, img_bgr):
    """[h, w, 3] uint8 B,G,R image -> RGB PNG (host side of display_image's out.png)."""
    a = np.ascontiguousarray(img_bgr, np.uint8)
    check(libs()[1].rth_write_png_bgr(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0], a.strides[0]), "write_png")


class Timer:
    """hipEvent pair on a given stream (rt_timer_*)."""

    def __init__(self):
        self.h = _vp()
        check(libs()[0].rt_timer_create(C.byref(self.h)), "rt_timer_create")

    def start(self, stream=None):
        check(libs()[0].rt_timer_start(self.h, stream), "rt_timer_start")

    def stop(self, stream=None):
        check(libs()[0].rt_timer_stop(self.h, stream), "rt_timer_stop")

    def elapsed_ms(self):
        ms = C.c_float(0)
        check(libs()[0].rt_timer_elapsed_ms(self.h, C.byref(ms)), "rt_timer_elapsed_ms")
        return ms.value

    def close(self):
        if self.h:
            libs()[0].rt_timer_destroy(self.h)
            self.h = _vp()
