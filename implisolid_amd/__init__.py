"""implisolid_amd -- MI355X-native implicit-surface polygoniser (Python host side).

The product is the shared library ``implisolid_amd/lib/libimplisolid_mi355x.so`` (HIP, gfx950),
whose C ABI (``include/implisolid.h``) is a drop-in for ImpliSolid's ``mcc2.cpp`` interface.  This
module binds it with ctypes and mirrors the reference's JavaScript front-end calls for the same
path (``implisolid_main.js``: ``make_geometry`` :201-249, ``query_implicit_values`` :291-333,
``query_a_normal`` :335-368), so Python callers get the reference's behaviour.

There is no CPU fallback: if the library is missing or no GPU is present the calls raise.
"""
import ctypes
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libimplisolid_mi355x.so")
LIB_PATH = os.environ.get("IMPLISOLID_LIB") or LIB_PATH   # experiments: an alternative build

# every symbol declared in include/implisolid.h
ABI_SYMBOLS = [
    "build_geometry", "build_geometry_u", "get_v_size", "get_f_size", "get_f", "get_v", "finish_geometry",
    "get_f_ptr", "get_v_ptr", "set_object", "unset_object", "set_x", "unset_x", "calculate_implicit_values",
    "get_values_ptr", "get_values_size", "calculate_implicit_gradients", "get_gradients_ptr",
    "get_gradients_size", "get_pointset_ptr", "get_pointset_size", "about", "implisolid_last_error",
    "implisolid_set_error_mode", "implisolid_eval_points", "implisolid_program_info",
    "implisolid_slab_create", "implisolid_slab_destroy", "implisolid_slab_eval", "implisolid_slab_count",
    "implisolid_slab_emit", "implisolid_slab_emit_verts", "implisolid_slab_emit_faces", "implisolid_slab_counters", "implisolid_slab_counts", "implisolid_slab_grid",
    "implisolid_slab_verts", "implisolid_slab_faces", "implisolid_slab_field", "implisolid_slab_set_offsets",
    "implisolid_slab_download", "implisolid_slab_copy_counts", "implisolid_slab_read_field", "implisolid_set_pruning",
    "implisolid_parse_settings", "implisolid_slab_partition", "implisolid_slab_brick_stats",
    "implisolid_slab_set_timing", "implisolid_slab_kernel_times", "implisolid_jit_compile",
    "implisolid_slab_used_jit", "implisolid_set_jit", "implisolid_slab_stats", "implisolid_slab_read_signs",
    "implisolid_slab_read_fill",
    "implisolid_srand", "implisolid_rand", "implisolid_rand_skip",
    "implisolid_batch_create", "implisolid_batch_run", "implisolid_batch_info", "implisolid_batch_counts",
    "implisolid_batch_download", "implisolid_batch_destroy",
    "implisolid_slab_create_range", "implisolid_slab_balance", "implisolid_cuts_from_layer_work", "implisolid_set_devices",
    "implisolid_slab_copy_mesh", "implisolid_set_jit_bake", "implisolid_jit_wait", "implisolid_jit_stats",
    "implisolid_set_jit_max_modules", "implisolid_jit_modules",
    "implisolid_set_progress_callback", "implisolid_ob02_profile", "implisolid_last_build_stats",
    "implisolid_jit_compile_points", "implisolid_debug_libm", "implisolid_debug_cos", "implisolid_slab_stats_n",
    "implisolid_slab_kernel_times_each", "implisolid_debug_fold", "implisolid_debug_intervals",
    "implisolid_debug_eval_modes",
    "implisolid_ob02_create", "implisolid_ob02_destroy", "implisolid_ob02_load", "implisolid_ob02_resample",
    "implisolid_ob02_project", "implisolid_ob02_subdivide", "implisolid_ob02_counts", "implisolid_ob02_ranges",
    "implisolid_ob02_get_verts", "implisolid_ob02_set_verts", "implisolid_ob02_download",
    "implisolid_ob02_attach", "implisolid_ob02_stream", "implisolid_ob02_resample_async", "implisolid_ob02_project_async",
    "implisolid_ob02_unpack", "implisolid_ob02_halo",
    "get_n_size", "get_n_ptr", "get_n", "implisolid_normals_stats", "implisolid_eval_normals",
    "implisolid_slab_emit_normals", "implisolid_slab_normals", "implisolid_slab_download_normals",
    "implisolid_batch_has_normals", "implisolid_batch_download_normals",
    "implisolid_bounds", "implisolid_bounds_edges", "implisolid_fit_box", "implisolid_parse_fit_box",
    "implisolid_last_fit_box", "implisolid_debug_bounds_ms",
    "implisolid_slice", "implisolid_slice_copy", "implisolid_slice_coords", "implisolid_slice_loops",
    "implisolid_mass", "implisolid_mass_mids", "implisolid_mass_physical",
    "implisolid_raster", "implisolid_raster_coords",
    "implisolid_islands", "implisolid_islands_copy", "implisolid_debug_islands_ms",
    "implisolid_layer_distance", "implisolid_debug_layer_distance_ms",
    "implisolid_layer_hollow", "implisolid_hollow_wall2", "implisolid_debug_layer_hollow_ms",
    "implisolid_layer_supports", "implisolid_layer_supports_copy", "implisolid_debug_layer_supports_ms",
    "implisolid_layer_runs", "implisolid_layer_runs_copy", "implisolid_debug_layer_runs_ms",
    "implisolid_layer_bodies", "implisolid_layer_bodies_copy", "implisolid_debug_layer_bodies_ms",
    "implisolid_layer_cups", "implisolid_layer_cups_copy", "implisolid_debug_layer_cups_ms",
    "implisolid_raycast", "implisolid_ray_params", "implisolid_debug_raycast_ms",
    "implisolid_ray_spans", "implisolid_ray_spans_copy", "implisolid_debug_ray_spans_ms",
]

# implisolid_progress_callback (include/implisolid.h): verts, n_verts, faces, n_faces,
# progress_callback_id, shape_id, call_id, user
PROGRESS_CALLBACK = ctypes.CFUNCTYPE(None, ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p)

_lib = None


class ImplisolidError(RuntimeError):
    pass


def build(jobs=8):
    """Compile the HIP library in-tree (make -C implisolid_amd)."""
    import subprocess
    subprocess.run(["make", "-s", "-j%d" % jobs, "-C", _HERE], check=True)


def lib():
    """The loaded C ABI.  Raises if the HIP library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("implisolid_amd: %s is missing -- run implisolid_amd.build() (make -C implisolid_amd)" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    c_char_p, c_int, c_bool, c_void_p = ctypes.c_char_p, ctypes.c_int, ctypes.c_bool, ctypes.c_void_p
    fp = ctypes.POINTER(ctypes.c_float)
    ip = ctypes.POINTER(ctypes.c_int32)
    up = ctypes.POINTER(ctypes.c_uint32)
    sig = {
        "build_geometry": ([c_char_p, c_char_p], None),
        "build_geometry_u": ([c_char_p, c_char_p, c_char_p], None),
        "get_v_size": ([], c_int), "get_f_size": ([], c_int),
        "get_f": ([ip, c_int], None), "get_v": ([fp, c_int], None),
        "finish_geometry": ([], None), "get_f_ptr": ([], c_void_p), "get_v_ptr": ([], c_void_p),
        "set_object": ([c_char_p, c_bool], c_int), "unset_object": ([c_int], c_bool),
        "set_x": ([c_void_p, c_int], c_bool), "unset_x": ([], None),
        "calculate_implicit_values": ([], None), "get_values_ptr": ([], c_void_p), "get_values_size": ([], c_int),
        "calculate_implicit_gradients": ([c_bool], None), "get_gradients_ptr": ([], c_void_p),
        "get_gradients_size": ([], c_int), "get_pointset_ptr": ([c_char_p], c_void_p),
        "get_pointset_size": ([c_char_p], c_int), "about": ([], None),
        "implisolid_last_error": ([], c_char_p), "implisolid_set_error_mode": ([c_int], None),
        "implisolid_eval_points": ([fp, ctypes.c_int64, fp, fp], c_int),
        "implisolid_debug_libm": ([c_int, fp, fp, ctypes.c_int64, fp], c_int),
        "implisolid_debug_cos": ([ctypes.POINTER(ctypes.c_double), ctypes.c_int64, ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_debug_fold": ([fp, ctypes.c_int64, fp, ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_debug_intervals": ([c_char_p, c_int, c_int, fp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64, fp,
                                        ctypes.POINTER(ctypes.c_uint64)], c_int),
        "implisolid_debug_eval_modes": ([c_char_p, c_int, fp, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64, fp], c_int),
        "implisolid_ob02_create": ([c_char_p, c_char_p], c_void_p),
        "implisolid_ob02_destroy": ([c_void_p], None),
        "implisolid_ob02_load": ([c_void_p, c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64, ctypes.c_int64,
                                  ctypes.c_int64], c_int),
        "implisolid_ob02_resample": ([c_void_p], c_int),
        "implisolid_ob02_project": ([c_void_p], c_int),
        "implisolid_ob02_subdivide": ([c_void_p, ctypes.c_float], c_int),
        "implisolid_ob02_counts": ([c_void_p, ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_ob02_ranges": ([c_void_p, ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_ob02_get_verts": ([c_void_p, c_void_p], c_int),
        "implisolid_ob02_set_verts": ([c_void_p, c_void_p], c_int),
        "implisolid_ob02_download": ([c_void_p, fp, ip], c_int),
        "implisolid_ob02_attach": ([c_void_p, c_void_p, ctypes.c_int64, c_void_p, ctypes.c_int64, ctypes.c_int64,
                                    ctypes.c_int64, c_void_p], c_int),
        "implisolid_ob02_stream": ([c_void_p], c_void_p),
        "implisolid_ob02_resample_async": ([c_void_p], c_int),
        "implisolid_ob02_project_async": ([c_void_p], c_int),
        "implisolid_ob02_unpack": ([c_void_p, c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), c_int, c_int], c_int),
        "implisolid_ob02_halo": ([c_void_p, ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_program_info": ([c_char_p, c_int, ip, fp], c_int),
        "implisolid_slab_create": ([c_char_p, c_char_p, c_int, c_int], c_void_p),
        "implisolid_slab_destroy": ([c_void_p], None),
        "implisolid_slab_eval": ([c_void_p, c_void_p], c_int),
        "implisolid_slab_count": ([c_void_p, c_void_p], c_int),
        "implisolid_slab_emit": ([c_void_p, c_void_p, c_void_p], c_int),
        "implisolid_slab_emit_verts": ([c_void_p, c_void_p], c_int),
        "implisolid_slab_emit_faces": ([c_void_p, c_void_p, c_void_p, c_int, c_void_p], c_int),
        "implisolid_slab_counters": ([c_void_p], c_void_p),
        "implisolid_slab_counts": ([c_void_p, c_void_p, up], c_int),
        "implisolid_slab_grid": ([c_void_p, ip], c_int),
        "implisolid_slab_verts": ([c_void_p], c_void_p),
        "implisolid_slab_faces": ([c_void_p], c_void_p),
        "implisolid_slab_field": ([c_void_p], c_void_p),
        "implisolid_slab_set_offsets": ([c_void_p, ctypes.c_uint32, ctypes.c_uint32], c_int),
        "implisolid_slab_download": ([c_void_p, fp, ip, c_void_p], c_int),
        "implisolid_slab_copy_counts": ([c_void_p, c_void_p, c_void_p], c_int),
        "implisolid_slab_read_field": ([c_void_p, fp, ctypes.c_int64], ctypes.c_int64),
        "implisolid_set_pruning": ([c_int], None),
        "implisolid_parse_settings": ([c_char_p, fp, ip, fp], c_int),
        "implisolid_slab_partition": ([c_int, c_int, c_int, ip], c_int),
        "implisolid_slab_brick_stats": ([c_void_p, ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_slab_set_timing": ([c_void_p, c_int], c_int),
        "implisolid_slab_used_jit": ([c_void_p], c_int),
        "implisolid_slab_stats": ([c_void_p, ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_slab_read_signs": ([c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int64], ctypes.c_int64),
        "implisolid_slab_read_fill": ([c_void_p, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int64, ip], ctypes.c_int64),
        "implisolid_set_jit": ([c_int], None),
        "implisolid_jit_compile": ([c_char_p, ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)],
                                   ctypes.c_int64),
        "implisolid_slab_kernel_times": ([c_void_p, fp], c_int),
        "implisolid_slab_kernel_times_each": ([c_void_p, fp], c_int),
        "implisolid_slab_stats_n": ([c_void_p, ctypes.POINTER(ctypes.c_int64), c_int], c_int),
        "implisolid_srand": ([ctypes.c_uint], None),
        "implisolid_rand": ([], c_int),
        "implisolid_rand_skip": ([ctypes.c_uint64], None),
        "implisolid_batch_create": ([ctypes.POINTER(c_char_p), c_int, c_char_p, c_int], c_void_p),
        "implisolid_batch_run": ([c_void_p, c_void_p], c_int),
        "implisolid_batch_info": ([c_void_p, ip, ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_batch_counts": ([c_void_p, c_int, up], c_int),
        "implisolid_batch_download": ([c_void_p, c_int, fp, ip], c_int),
        "implisolid_batch_destroy": ([c_void_p], None),
        "implisolid_slab_create_range": ([c_char_p, c_char_p, c_int, c_int], c_void_p),
        "implisolid_slab_balance": ([c_char_p, c_char_p, c_int, ip], c_int),
        "implisolid_cuts_from_layer_work": ([ctypes.POINTER(ctypes.c_int64), c_int, ctypes.c_int64, c_int, c_int, ip], c_int),
        "implisolid_set_devices": ([ip, c_int], c_int),
        "implisolid_slab_copy_mesh": ([c_void_p, c_void_p, c_void_p, ctypes.c_int64, ctypes.c_int64, c_void_p], c_int),
        "implisolid_set_jit_bake": ([c_int], None),
        "implisolid_jit_wait": ([], None),
        "implisolid_jit_stats": ([ip, ctypes.POINTER(ctypes.c_double)], None),
        "implisolid_set_jit_max_modules": ([ctypes.c_int], None),
        "implisolid_jit_modules": ([ip], None),
        "implisolid_set_progress_callback": ([PROGRESS_CALLBACK, c_void_p], None),
        "implisolid_ob02_profile": ([c_int], None),
        "implisolid_jit_compile_points": ([c_char_p, ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)],
                                          ctypes.c_int64),
        "implisolid_last_build_stats": ([ctypes.POINTER(ctypes.c_double)], c_int),
        "get_n_size": ([], c_int), "get_n_ptr": ([], c_void_p), "get_n": ([fp, c_int], None),
        "implisolid_normals_stats": ([ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_eval_normals": ([fp, ctypes.c_int64, fp, ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_slab_emit_normals": ([c_void_p, c_void_p], c_int),
        "implisolid_slab_normals": ([c_void_p], c_void_p),
        "implisolid_slab_download_normals": ([c_void_p, fp, c_void_p], c_int),
        "implisolid_batch_has_normals": ([c_void_p], c_int),
        "implisolid_batch_download_normals": ([c_void_p, c_int, fp, ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_bounds": ([c_char_p, c_int, fp, c_int, fp, ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_bounds_edges": ([fp, c_int, fp], c_int),
        "implisolid_fit_box": ([fp, fp, c_int, c_int, fp], c_int),
        "implisolid_parse_fit_box": ([c_char_p, ip], c_int),
        "implisolid_last_fit_box": ([fp], c_int),
        "implisolid_debug_bounds_ms": ([c_int], ctypes.c_double),
        "implisolid_slice": ([c_char_p, c_int, fp, c_int, fp, c_int, ctypes.POINTER(ctypes.c_int64),
                              ctypes.POINTER(ctypes.c_int64)], ctypes.c_int64),
        "implisolid_slice_copy": ([fp, up], c_int),
        "implisolid_slice_coords": ([fp, c_int, fp, fp], c_int),
        "implisolid_slice_loops": ([up, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                    ctypes.POINTER(ctypes.c_uint8)], ctypes.c_int64),
        "implisolid_mass": ([c_char_p, c_int, fp, c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64),
                             ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_mass_mids": ([fp, c_int, fp], c_int),
        "implisolid_mass_physical": ([fp, c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_raster": ([c_char_p, c_int, fp, c_int, c_int, c_int, fp, c_int, ctypes.POINTER(ctypes.c_uint8),
                               ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_raster_coords": ([fp, c_int, c_int, c_int, fp, fp], c_int),
        "implisolid_islands": ([c_char_p, c_int, fp, c_int, c_int, c_int, fp, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int64),
                                ip, ctypes.POINTER(ctypes.c_int64)], ctypes.c_int64),
        "implisolid_islands_copy": ([ip], c_int),
        "implisolid_debug_islands_ms": ([c_int, ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_layer_distance": ([c_char_p, c_int, fp, c_int, c_int, c_int, fp, c_int, c_int, ctypes.c_int64, ip,
                                       ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_debug_layer_distance_ms": ([c_int, ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_layer_hollow": ([c_char_p, c_int, fp, c_int, c_int, c_int, fp, c_int, c_int, ctypes.POINTER(ctypes.c_int64), c_int,
                                     c_int, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int64),
                                     ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_hollow_wall2": ([ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_int64), c_int], c_int),
        "implisolid_debug_layer_hollow_ms": ([c_int, ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_layer_supports": ([c_char_p, c_int, fp, c_int, c_int, c_int, fp, c_int, c_int, ctypes.c_int64, c_int,
                                       ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                       ctypes.POINTER(ctypes.c_int64)], ctypes.c_int64),
        "implisolid_layer_supports_copy": ([ip], c_int),
        "implisolid_debug_layer_supports_ms": ([c_int, ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_layer_runs": ([c_char_p, c_int, fp, c_int, c_int, c_int, fp, c_int, c_int, ctypes.POINTER(ctypes.c_int64),
                                   ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)], ctypes.c_int64),
        "implisolid_layer_runs_copy": ([up, ctypes.POINTER(ctypes.c_uint8)], c_int),
        "implisolid_debug_layer_runs_ms": ([c_int, ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_layer_bodies": ([c_char_p, c_int, fp, c_int, c_int, c_int, fp, c_int, c_int, c_int, c_int, c_int,
                                     ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)], ctypes.c_int64),
        "implisolid_layer_bodies_copy": ([ctypes.POINTER(ctypes.c_int64), ip], c_int),
        "implisolid_debug_layer_bodies_ms": ([c_int, ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_layer_cups": ([c_char_p, c_int, fp, c_int, c_int, c_int, fp, c_int, c_int, c_int, c_int,
                                   ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)],
                                  ctypes.c_int64),
        "implisolid_layer_cups_copy": ([ctypes.POINTER(ctypes.c_int64), ip], c_int),
        "implisolid_debug_layer_cups_ms": ([c_int, ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_raycast": ([c_char_p, c_int, fp, fp, ctypes.c_int64, ctypes.c_float, ctypes.c_float, c_int, c_int, ip, fp,
                                fp, fp, ctypes.POINTER(ctypes.c_int64)], c_int),
        "implisolid_ray_params": ([ctypes.c_float, ctypes.c_float, c_int, fp], c_int),
        "implisolid_debug_raycast_ms": ([c_int, ctypes.POINTER(ctypes.c_double)], c_int),
        "implisolid_ray_spans": ([c_char_p, c_int, fp, fp, ctypes.c_int64, ctypes.c_float, ctypes.c_float, c_int, c_int, c_int,
                                  ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)], ctypes.c_int64),
        "implisolid_ray_spans_copy": ([ip, fp, fp, fp], c_int),
        "implisolid_debug_ray_spans_ms": ([c_int, ctypes.POINTER(ctypes.c_double)], c_int),
    }
    for name, (args, res) in sig.items():
        try:
            f = getattr(L, name)
        except AttributeError:
            # an older experimental build (IMPLISOLID_LIB, same-box A/B runs) lacks the newest entry
            # points: only its callers fail; the in-tree library exports every one (test_cpu)
            if os.environ.get("IMPLISOLID_LIB"):
                continue
            raise
        f.argtypes = args
        f.restype = res
    L.implisolid_set_error_mode(1)   # Python callers get exceptions instead of abort()
    _lib = L
    return L


def _s(x):
    if isinstance(x, (dict, list)):
        x = json.dumps(x)
    return x.encode() if isinstance(x, str) else x


def _check():
    err = lib().implisolid_last_error()
    if err:
        raise ImplisolidError(err.decode(errors="replace"))


def parse_settings(mc_settings):
    """Host-side mc-settings parse (no GPU): dict of the parsed values; raises on invalid input."""
    L = lib()
    box = (ctypes.c_float * 6)()
    ints = (ctypes.c_int32 * 7)()
    fl = (ctypes.c_float * 2)()
    if L.implisolid_parse_settings(_s(mc_settings), box, ints, fl) != 0:
        raise ImplisolidError(last_error())
    keys = ["resolution", "ignore_root_matrix", "overall_repeats", "vresampl_iters", "projection", "qem", "subdiv"]
    out = {k: int(v) for k, v in zip(keys, ints)}
    out["box"] = [np.float32(b) for b in box]
    out["vresampl_c"] = np.float32(fl[0])
    out["post_subdiv_noise"] = np.float32(fl[1])
    return out


def slab_partition(R, rank, nranks):
    """(z0, z1, halo): the cell layers a rank owns in the Z-slab decomposition."""
    out = (ctypes.c_int32 * 3)()
    if lib().implisolid_slab_partition(int(R), int(rank), int(nranks), out) != 0:
        raise ImplisolidError(last_error())
    return int(out[0]), int(out[1]), int(out[2])


def slab_balance(shape, mc_settings, nranks):
    """Balanced Z-slab cuts [1, ..., R + 3] (nranks + 1 cell-layer boundaries) from one interval
    pass of the whole grid on the current device; rank r owns layers [cuts[r], cuts[r + 1])."""
    out = (ctypes.c_int32 * (int(nranks) + 1))()
    if lib().implisolid_slab_balance(_s(shape), _s(mc_settings), int(nranks), out) != 0:
        raise ImplisolidError(last_error())
    return [int(x) for x in out]


def cuts_from_layer_work(listed, bricks_per_layer, R, nranks):
    """Host only: the balanced cuts from per-sample-layer listed-brick counts (R + 3 layers)."""
    a = np.ascontiguousarray(listed, dtype=np.int64)
    out = (ctypes.c_int32 * (int(nranks) + 1))()
    if lib().implisolid_cuts_from_layer_work(a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(a),
                                             int(bricks_per_layer), int(R), int(nranks), out) != 0:
        raise ImplisolidError(last_error())
    return [int(x) for x in out]


def set_devices(ids):
    """The HIP devices build_geometry's marching cubes runs on (balanced Z-slabs, slab r on
    ids[r]; a device may repeat).  None or one device: the current device only."""
    ids = list(ids or [])
    arr = (ctypes.c_int32 * max(1, len(ids)))(*ids)
    if lib().implisolid_set_devices(arr if ids else None, len(ids)) != 0:
        raise ImplisolidError(last_error())


def set_jit(mode):
    """Tree-kernel JIT mode for objects set from now on: False/0 off (interpreter), True/1 sync
    (compile before the first eval), 2 async (the library default: compile in the background, the
    interpreter meanwhile)."""
    lib().implisolid_set_jit(int(mode))


def set_jit_bake(mode):
    """Tree modules with the object's matrices baked in as literals: 0 never (one module per shape),
    1 every object, 2 (default) hot objects -- an object evaluated 4 times by the same engine gets its
    baked module (compiled in the background in async mode).  True / False mean 1 / 0."""
    lib().implisolid_set_jit_bake(int(mode))


def jit_wait():
    """Block until every scheduled tree-kernel compilation has finished."""
    lib().implisolid_jit_wait()


def jit_stats():
    out = (ctypes.c_int32 * 4)()
    secs = ctypes.c_double(0)
    lib().implisolid_jit_stats(out, ctypes.byref(secs))
    mods = (ctypes.c_int32 * 3)()
    lib().implisolid_jit_modules(mods)
    return {"mode": out[0], "bake": int(out[1]), "compiled": out[2], "disk_hits": out[3], "compile_s": secs.value,
            "modules": mods[0], "max_modules": mods[1], "evicted": mods[2]}


def set_jit_max_modules(n):
    """Bound the loaded tree modules (least recently requested unheld ones are unloaded past it)."""
    lib().implisolid_set_jit_max_modules(int(n))


def jit_compile(shape, points=False):
    """Host-only: (code-object bytes, compile seconds, generated source) of the shape's tree kernel
    module (points=True: its point module)."""
    L = lib()
    buf = ctypes.create_string_buffer(1 << 20)
    secs = ctypes.c_double(0)
    fn = L.implisolid_jit_compile_points if points else L.implisolid_jit_compile
    n = fn(_s(shape), buf, len(buf), ctypes.byref(secs))
    if n < 0:
        raise ImplisolidError(last_error())
    return int(n), float(secs.value), buf.value.decode()


def set_pruning(level):
    """Per-brick pruning level of the field evaluation: 0 off, 1 CSG operand pruning (field
    bit-identical), 2 (default) + sign-filled bricks (mesh bit-identical).  True means 2."""
    if level is True:
        level = 2
    lib().implisolid_set_pruning(int(level))


def srand(seed):
    """Seed the library's glibc-compatible rand() (the generator the subdivision noise draws from,
    randomize_verts basic_functions.hpp:551-557).  Host only."""
    lib().implisolid_srand(int(seed) & 0xFFFFFFFF)


def rand():
    return int(lib().implisolid_rand())


def rand_skip(n):
    """Discard n draws of the library's rand() (O(log n) jump-ahead)."""
    lib().implisolid_rand_skip(int(n))


def last_error():
    return lib().implisolid_last_error().decode(errors="replace")


# ---- mesh API (implisolid_main.js make_geometry :201-249) -----------------------------------------
def _with_normals(mc_settings, normals):
    """The settings as given, or (normals=True) a copy of them with "normals": {"enabled": 1} merged
    in: the caller's dict is never changed."""
    if not normals:
        return mc_settings
    d = json.loads(mc_settings.decode() if isinstance(mc_settings, bytes) else mc_settings) \
        if isinstance(mc_settings, (str, bytes)) else dict(mc_settings)
    d["normals"] = dict(d["normals"], enabled=1) if isinstance(d.get("normals"), dict) else {"enabled": 1}
    return d


def make_geometry(shape, mc_settings, normals=False):
    """Polygonise an MP5 shape; returns (verts float32 [V,3], faces int32 [F,3]) host copies, and with
    normals=True a third array, the per-vertex normals float32 [V,3] of the same build (the
    "normals" settings key, include/implisolid.h get_n_ptr)."""
    L = lib()
    L.finish_geometry()             # implisolid_main.js:214-217
    _VIEW_GEN[0] += 1   # earlier make_geometry_views arrays are stale from here on
    L.build_geometry(_s(shape), _s(_with_normals(mc_settings, normals)))
    _check()
    nv, nf = L.get_v_size(), L.get_f_size()
    v = np.empty((nv, 3), np.float32)
    f = np.empty((nf, 3), np.int32)
    if nv:
        L.get_v(v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nv)
    if nf:
        L.get_f(f.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), nf)
    if normals:
        nn = L.get_n_size()
        if nn != nv:
            raise ImplisolidError("make_geometry: %d normals for %d vertices" % (nn, nv))
        n = np.empty((nn, 3), np.float32)
        if nn:
            L.get_n(n.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nn)
    L.finish_geometry()
    return (v, f, n) if normals else (v, f)


def normals_stats():
    """[normals computed, rows that took the -42 branch (|grad| <= 1e-4 or not a number)] of the last build."""
    out = (ctypes.c_int64 * 2)()
    if lib().implisolid_normals_stats(out) != 0:
        raise ImplisolidError(last_error())
    return int(out[0]), int(out[1])


_VIEW_GEN = [0]   # build_geometry calls through make_geometry_views: the generation of its views


def make_geometry_views(shape, mc_settings, normals=False):
    """build_geometry as the reference's front end reads it (implisolid_main.js:227-237): the mesh is
    left in the library's result buffers (pinned host memory) and returned as read-only numpy views
    over get_v_ptr / get_f_ptr -- no copy.  The views are valid until the next build_geometry or
    finish_geometry (a larger next build frees the pinned buffers they point into): keep them with
    copy_geometry_views(v, f), which refuses stale views; views_current(v) tells whether a view
    still holds the last build's mesh.  normals=True: a third view, over get_n_ptr, with the same
    staleness rule."""
    L = lib()
    _VIEW_GEN[0] += 1
    L.finish_geometry()
    L.build_geometry(_s(shape), _s(_with_normals(mc_settings, normals)))
    _check()
    nv, nf = L.get_v_size(), L.get_f_size()
    v = np.ctypeslib.as_array(ctypes.cast(L.get_v_ptr(), ctypes.POINTER(ctypes.c_float)), shape=(nv, 3)) if nv \
        else np.zeros((0, 3), np.float32)
    f = np.ctypeslib.as_array(ctypes.cast(L.get_f_ptr(), ctypes.POINTER(ctypes.c_int32)), shape=(nf, 3)) if nf \
        else np.zeros((0, 3), np.int32)
    out = [v, f]
    if normals:
        nn = L.get_n_size()
        if nn != nv:
            raise ImplisolidError("make_geometry_views: %d normals for %d vertices" % (nn, nv))
        out.append(np.ctypeslib.as_array(ctypes.cast(L.get_n_ptr(), ctypes.POINTER(ctypes.c_float)), shape=(nn, 3)) if nn
                   else np.zeros((0, 3), np.float32))
    out = [a.view(_GeometryView) for a in out]
    for a in out:
        a.flags.writeable = False
        a._gen = _VIEW_GEN[0]
    return tuple(out)


class _GeometryView(np.ndarray):
    """A read-only numpy view into the library's result buffers (make_geometry_views), tagged with the
    build generation that made it."""
    _gen = -1

    def __array_finalize__(self, obj):
        self._gen = getattr(obj, "_gen", -1)


def views_current(a):
    """True while a make_geometry_views array still holds the last build's mesh."""
    return getattr(a, "_gen", -1) == _VIEW_GEN[0]


def copy_geometry_views(v, f):
    """Owned copies of make_geometry_views' arrays; raises if another build has replaced them."""
    if not (views_current(v) and views_current(f)):
        raise ImplisolidError("geometry views are stale: a later build_geometry replaced the mesh they point into")
    return np.array(v, dtype=np.float32, copy=True), np.array(f, dtype=np.int32, copy=True)


def make_geometry_progressive(shape, mc_settings, call_specs=None):
    """build_geometry_u with a progress hook (the reference's worker path, worker_api.js:315-345 and
    send_progress_update :399-416): returns (verts, faces, updates), updates = the intermediate
    meshes the library reported -- after marching cubes, after each repeat's vertex resampling and
    after each centroid projection -- as (verts, faces, progressCallback_id, shape_id, call_id)."""
    L = lib()
    updates = []

    def hook(vp, nv, fp_, nf, pid, sid, cid, user):
        v = np.ctypeslib.as_array(vp, shape=(nv * 3,)).copy().reshape(nv, 3) if nv else np.zeros((0, 3), np.float32)
        f = np.ctypeslib.as_array(fp_, shape=(nf * 3,)).copy().reshape(nf, 3) if nf else np.zeros((0, 3), np.int32)
        updates.append((v, f, int(pid), int(sid), int(cid)))

    cb = PROGRESS_CALLBACK(hook)
    L.finish_geometry()
    L.implisolid_set_progress_callback(cb, None)
    try:
        _VIEW_GEN[0] += 1
        L.build_geometry_u(_s(shape), _s(mc_settings), _s(call_specs if call_specs is not None else {}))
    finally:
        L.implisolid_set_progress_callback(PROGRESS_CALLBACK(), None)
    _check()
    nv, nf = L.get_v_size(), L.get_f_size()
    v = np.empty((nv, 3), np.float32)
    f = np.empty((nf, 3), np.int32)
    if nv:
        L.get_v(v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nv)
    if nf:
        L.get_f(f.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), nf)
    L.finish_geometry()
    return v, f, updates


OB02_STAGES = ("topology", "resample", "edge_fold", "project", "qem", "subdiv", "fetch")


def ob02_profile(on):
    """Per-stage wall times and evaluation counts of the OB02 steps for following builds (drains
    the stream at every stage boundary: for breakdowns, not for timing whole builds)."""
    lib().implisolid_ob02_profile(1 if on else 0)


def last_build_stats():
    """Diagnostics of the last build_geometry: bisection cap hits, projection evaluations and stage
    times (profiled builds), the last average edge length, faces and vertices."""
    out = (ctypes.c_double * 13)()
    if lib().implisolid_last_build_stats(out) != 0:
        raise ImplisolidError(last_error())
    d = {"bisection_cap_hits": int(out[0]), "projection_evals": int(out[1]), "avg_edge": float(out[2]),
         "faces": int(out[10]), "verts": int(out[11]), "jit_launches": int(out[12])}
    d["stage_ms"] = dict(zip(OB02_STAGES, [float(x) for x in out[3:10]]))
    return d


def get_pointset(name):
    L = lib()
    n = L.get_pointset_size(_s(name))
    p = L.get_pointset_ptr(_s(name))
    if not p or n <= 0:
        return None
    return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), shape=(n * 3,)).copy().reshape(n, 3)


# ---- direct evaluation (implisolid_main.js:291-368) ---------------------------------------------------
class ImplicitService:
    """set_object / set_x / calculate_implicit_values / calculate_implicit_gradients."""

    def __init__(self, shape, ignore_root_matrix=False):
        L = lib()
        self.id = L.set_object(_s(shape), bool(ignore_root_matrix))
        if self.id != 1:
            raise ImplisolidError(last_error() or "set_object failed")

    def close(self):
        if self.id:
            lib().unset_object(self.id)
            self.id = 0

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def eval(self, pts, gradient=False):
        """Any number of points (additive implisolid_eval_points; no 50k limit)."""
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        f = np.empty(p.shape[0], np.float32)
        g = np.empty((p.shape[0], 3), np.float32) if gradient else None
        fp = ctypes.POINTER(ctypes.c_float)
        rc = lib().implisolid_eval_points(p.ctypes.data_as(fp), p.shape[0], f.ctypes.data_as(fp),
                                          g.ctypes.data_as(fp) if gradient else None)
        if rc != 0:
            raise ImplisolidError(last_error())
        return (f, g) if gradient else f

    def normals(self, pts, return_problems=False):
        """Surface normals -g / |g| at any number of points (implisolid_eval_normals: the kernel of
        make_geometry(..., normals=True); rows with |g| <= 1e-4 or a non-finite g are -42 g).  With
        return_problems: (normals, the number of such rows)."""
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        out = np.empty((p.shape[0], 3), np.float32)
        bad = ctypes.c_int64(0)
        fp = ctypes.POINTER(ctypes.c_float)
        rc = lib().implisolid_eval_normals(p.ctypes.data_as(fp), p.shape[0], out.ctypes.data_as(fp), ctypes.byref(bad))
        if rc != 0:
            raise ImplisolidError(last_error())
        return (out, int(bad.value)) if return_problems else out

    def query_implicit_values(self, pts):
        """The reference call sequence set_x / calculate_implicit_values / get_values / unset_x."""
        L = lib()
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        if not L.set_x(p.ctypes.data_as(ctypes.c_void_p), p.shape[0]):
            raise ImplisolidError(last_error())
        try:
            L.calculate_implicit_values()
            _check()
            n = L.get_values_size()
            ptr = L.get_values_ptr()
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), shape=(n,)).copy() if n else np.zeros(0, np.float32)
        finally:
            L.unset_x()

    def query_normals(self, pts, normalize_and_invert=True):
        L = lib()
        p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        if not L.set_x(p.ctypes.data_as(ctypes.c_void_p), p.shape[0]):
            raise ImplisolidError(last_error())
        try:
            L.calculate_implicit_gradients(bool(normalize_and_invert))
            _check()
            n = L.get_gradients_size()
            ptr = L.get_gradients_ptr()
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_float)), shape=(n,)).copy().reshape(-1, 3)
        finally:
            L.unset_x()


def debug_libm(which, a, b=None):
    """Diagnostics: the device restatements of glibc sinf (0) / atanf (1) / atan2f (2: atan2f(a, b))."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    bb = np.ascontiguousarray(b, dtype=np.float32) if b is not None else None
    if bb is not None and bb.shape != a.shape:
        raise ValueError("debug_libm: a and b differ in shape")
    out = np.empty_like(a)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = lib().implisolid_debug_libm(int(which), a.ctypes.data_as(fp), bb.ctypes.data_as(fp) if bb is not None else None,
                                     a.size, out.ctypes.data_as(fp))
    if rc != 0:
        raise ImplisolidError(last_error())
    return out


def debug_cos(a):
    """Diagnostics: the device restatement of glibc's double cos (the screw gradient's) on a float64 array."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = lib().implisolid_debug_cos(a.ctypes.data_as(dp), a.size, out.ctypes.data_as(dp))
    if rc != 0:
        raise ImplisolidError(last_error())
    return out


def debug_fold(terms):
    """Diagnostics: the projection's edge-length fold (s = 0; s += e[k], float, in order) on the
    device, as build_geometry computes it; returns (sum, chunks taken from the chunk table)."""
    e = np.ascontiguousarray(terms, dtype=np.float32).reshape(-1)
    out = (ctypes.c_float * 1)()
    tc = ctypes.c_int64(0)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = lib().implisolid_debug_fold(e.ctypes.data_as(fp), e.size, out, ctypes.byref(tc))
    if rc != 0:
        raise ImplisolidError(last_error())
    return np.float32(out[0]), int(tc.value)


def debug_intervals(shape, boxes, variant=0, modes_in=None, ignore_root_matrix=False):
    """Diagnostics: the interval evaluator on boxes [n, 6] = {xlo, xhi, ylo, yhi, zlo, zhi} of the
    tree; variant 0 the interpreter, 1 the shape's JIT module, 2 the baked module.  modes_in: per box
    the modes word of an enclosing box.  Returns (iv float32[n, 2] = {lo, hi}, modes uint64[n])."""
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    n = b.shape[0]
    up64 = ctypes.POINTER(ctypes.c_uint64)
    mi = None
    if modes_in is not None:
        mi = np.ascontiguousarray(modes_in, np.uint64).reshape(-1)
        if mi.size != n:
            raise ValueError("debug_intervals: one modes word per box")
    iv = np.empty((n, 2), np.float32)
    mo = np.zeros(n, np.uint64)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = lib().implisolid_debug_intervals(_s(shape), int(bool(ignore_root_matrix)), int(variant), b.ctypes.data_as(fp),
                                          mi.ctypes.data_as(up64) if mi is not None else None, n,
                                          iv.ctypes.data_as(fp), mo.ctypes.data_as(up64))
    if rc != 0:
        raise ImplisolidError(last_error())
    return iv, mo


def _box6(box, what):
    b = np.ascontiguousarray(box, np.float32).reshape(-1)
    if b.size != 6:
        raise ValueError("%s: a box is six floats {xmin, xmax, ymin, ymax, zmin, zmax}" % what)
    return b


def bounds(shape, search_box, depth, ignore_root_matrix=False):
    """The axis-aligned bounds of the solid inside search_box {xmin, xmax, ymin, ymax, zmin, zmax},
    from the interval evaluator on a 2^depth-cell edge table (depth in [3, 10]; include/implisolid.h
    implisolid_bounds).  Returns (found, box float32[6], stats): found False means the solid is
    empty in the search box (box == search_box); stats = [boxes bounded, boxes skipped as inside the
    running bounds, longest list, reruns after a list overflow]."""
    fp = ctypes.POINTER(ctypes.c_float)
    sb = _box6(search_box, "bounds")
    out = np.empty(6, np.float32)
    stats = (ctypes.c_int64 * 4)()
    rc = lib().implisolid_bounds(_s(shape), int(bool(ignore_root_matrix)), sb.ctypes.data_as(fp), int(depth),
                                 out.ctypes.data_as(fp), stats)
    if rc < 0:
        raise ImplisolidError(last_error())
    return bool(rc), out, [int(v) for v in stats]


def bounds_edges(search_box, depth):
    """Host only: the edge table of bounds(), float32 [3, 2^depth + 1] (x, y, z rows)."""
    fp = ctypes.POINTER(ctypes.c_float)
    sb = _box6(search_box, "bounds_edges")
    if not 3 <= int(depth) <= 10:
        raise ImplisolidError("bounds_edges: depth must be in [3, 10]")
    out = np.empty((3, (1 << int(depth)) + 1), np.float32)
    if lib().implisolid_bounds_edges(sb.ctypes.data_as(fp), int(depth), out.ctypes.data_as(fp)) != 0:
        raise ImplisolidError(last_error())
    return out


def fit_box(search_box, bounds_box, resolution, margin=2):
    """Host only: the sampling box (float32[6]) that puts bounds_box on resolution - 2 margin cells
    with margin cells around it, clipped to search_box (implisolid_fit_box)."""
    fp = ctypes.POINTER(ctypes.c_float)
    sb, bb = _box6(search_box, "fit_box"), _box6(bounds_box, "fit_box")
    out = np.empty(6, np.float32)
    if lib().implisolid_fit_box(sb.ctypes.data_as(fp), bb.ctypes.data_as(fp), int(resolution), int(margin),
                                out.ctypes.data_as(fp)) != 0:
        raise ImplisolidError(last_error())
    return out


def _rect4(rect, what):
    r = np.ascontiguousarray(rect, np.float32).reshape(-1)
    if r.size != 4:
        raise ValueError("%s: a rect is four floats {xmin, xmax, ymin, ymax}" % what)
    return r


def _layer_args(what, rect, z, width, height, supersample):
    """What raster_layers, layer_islands, layer_distance, layer_hollow, layer_supports, layer_runs, layer_bodies and layer_cups do with their arguments first: (rect, z, W, H, s)."""
    r = _rect4(rect, what)
    zz = np.ascontiguousarray(z, np.float32).reshape(-1)
    W, H, s = int(width), int(height), int(supersample)
    if not (1 <= W <= 16384 and 1 <= H <= 16384):
        raise ImplisolidError("%s: width and height must be in [1, 16384]" % what)
    return r, zz, W, H, s


def slice_layers(shape, rect, resolution, z, ignore_root_matrix=False, return_stats=False):
    """The solid's outlines on the planes z = z[l], by marching squares on the GPU over `resolution`
    cells per axis of rect {xmin, xmax, ymin, ymax} (include/implisolid.h implisolid_slice).  Returns
    (segments float32 (S, 2, 2) = {start, end} x {x, y}, directed with the solid on their left,
    keys uint32 (S, 2) = {start, end} edge keys, layer_offsets int64 (L + 1,)), and with return_stats
    also [(layer, tile) pairs, tiles evaluated, samples evaluated, chunks]."""
    fp, up = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    r = _rect4(rect, "slice_layers")
    zz = np.ascontiguousarray(z, np.float32).reshape(-1)
    offs = np.zeros(zz.size + 1, np.int64)
    stats = (ctypes.c_int64 * 4)()
    n = lib().implisolid_slice(_s(shape), int(bool(ignore_root_matrix)), r.ctypes.data_as(fp), int(resolution),
                               zz.ctypes.data_as(fp), int(zz.size), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), stats)
    if n < 0:
        raise ImplisolidError(last_error())
    seg = np.empty((n, 2, 2), np.float32)
    keys = np.empty((n, 2), np.uint32)
    if lib().implisolid_slice_copy(seg.ctypes.data_as(fp), keys.ctypes.data_as(up)) != 0:
        raise ImplisolidError(last_error())
    if return_stats:
        return seg, keys, offs, [int(v) for v in stats]
    return seg, keys, offs


def slice_coords(rect, resolution):
    """Host only: the sample coordinates of slice_layers, (xs, ys) float32 (resolution + 1,) each."""
    fp = ctypes.POINTER(ctypes.c_float)
    r = _rect4(rect, "slice_coords")
    if not 1 <= int(resolution) <= 4096:
        raise ImplisolidError("slice_coords: resolution must be in [1, 4096]")
    xs, ys = np.empty(int(resolution) + 1, np.float32), np.empty(int(resolution) + 1, np.float32)
    if lib().implisolid_slice_coords(r.ctypes.data_as(fp), int(resolution), xs.ctypes.data_as(fp), ys.ctypes.data_as(fp)) != 0:
        raise ImplisolidError(last_error())
    return xs, ys


def slice_loops(keys):
    """Host only: one layer's keys uint32 (n, 2) chained into polylines (implisolid_slice_loops).
    Returns (order int64 (n,), loop_offsets int64 (polylines + 1,), closed bool (polylines,)): polyline p
    is the segments order[loop_offsets[p]:loop_offsets[p + 1]]; open chains first, then closed loops.
    Raises if a key starts two segments or ends two."""
    k = np.ascontiguousarray(keys, np.uint32).reshape(-1, 2)
    n = k.shape[0]
    ip64 = ctypes.POINTER(ctypes.c_int64)
    order = np.zeros(n, np.int64)
    offs = np.zeros(n + 1, np.int64)
    closed = np.zeros(max(n, 1), np.uint8)
    loops = lib().implisolid_slice_loops(k.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n, order.ctypes.data_as(ip64),
                                         offs.ctypes.data_as(ip64), closed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    if loops < 0:
        raise ImplisolidError(last_error())
    return order, offs[:loops + 1].copy(), closed[:loops].astype(bool)


def slice_polylines(shape, rect, resolution, z, ignore_root_matrix=False):
    """slice_layers chained: per layer a list of (points float32 (n, 2), closed).  A closed loop lists
    each vertex once (the last point joins the first); an open chain ends with its last segment's end."""
    seg, keys, offs = slice_layers(shape, rect, resolution, z, ignore_root_matrix)
    out = []
    for l in range(len(offs) - 1):
        s, k = seg[offs[l]:offs[l + 1]], keys[offs[l]:offs[l + 1]]
        order, lo, closed = slice_loops(k)
        lines = []
        for p in range(len(closed)):
            idx = order[lo[p]:lo[p + 1]]
            pts = s[idx, 0]
            if not closed[p]:
                pts = np.concatenate([pts, s[idx[-1:], 1]])
            lines.append((np.ascontiguousarray(pts), bool(closed[p])))
        out.append(lines)
    return out


def raster_layers(shape, rect, width, height, z, supersample=1, ignore_root_matrix=False, return_stats=False, want_cov=True):
    """The solid's layers z = z[l] as coverage images on the GPU: width x height pixels of rect {xmin,
    xmax, ymin, ymax}, supersample x supersample samples per pixel (include/implisolid.h
    implisolid_raster).  Returns (cov uint8 (L, H, W) = solid samples per pixel, 0 .. supersample^2, row 0
    at ymin; layer_sum int64 (L,)), and with return_stats also [(layer, tile) pairs, tiles evaluated,
    tiles filled whole, samples evaluated, chunks].  want_cov=False passes cov = NULL: cov is None and
    only the sums (and stats) are produced."""
    fp = ctypes.POINTER(ctypes.c_float)
    r, zz, W, H, s = _layer_args("raster_layers", rect, z, width, height, supersample)
    cov = np.empty((zz.size, H, W), np.uint8) if want_cov else None
    sums = np.zeros(zz.size, np.int64)
    stats = (ctypes.c_int64 * 5)()
    rc = lib().implisolid_raster(_s(shape), int(bool(ignore_root_matrix)), r.ctypes.data_as(fp), W, H, s,
                                 zz.ctypes.data_as(fp), int(zz.size),
                                 cov.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if want_cov else None,
                                 sums.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), stats)
    if rc != 0:
        raise ImplisolidError(last_error())
    if return_stats:
        return cov, sums, [int(v) for v in stats]
    return cov, sums


def raster_coords(rect, width, height, supersample):
    """Host only: the sample tables of raster_layers, (mx float32 (width * supersample,), my float32
    (height * supersample,))."""
    fp = ctypes.POINTER(ctypes.c_float)
    r = _rect4(rect, "raster_coords")
    W, H, s = int(width), int(height), int(supersample)
    if not (1 <= W <= 16384 and 1 <= H <= 16384) or s not in (1, 2, 4):
        raise ImplisolidError("raster_coords: width and height must be in [1, 16384], supersample 1, 2 or 4")
    mx, my = np.empty(W * s, np.float32), np.empty(H * s, np.float32)
    if lib().implisolid_raster_coords(r.ctypes.data_as(fp), W, H, s, mx.ctypes.data_as(fp), my.ctypes.data_as(fp)) != 0:
        raise ImplisolidError(last_error())
    return mx, my


COMP_DTYPE = np.dtype([(name, np.int32) for name in ("seed", "area", "below", "x0", "y0", "x1", "y1", "layer")])


def layer_islands(shape, rect, width, height, z, supersample=1, threshold=1, connectivity=8, ignore_root_matrix=False,
                  want_labels=False, return_stats=False):
    """The connected regions of the solid's layers z = z[l] on the GPU, and which of them are islands
    (include/implisolid.h implisolid_islands).  The images are raster_layers'; a pixel is solid iff its
    coverage >= threshold (1 .. supersample^2); connectivity is 4 or 8.  Returns (comp_offsets int64 (L + 1,):
    layer l's records are comps[comp_offsets[l]:comp_offsets[l + 1]], in increasing seed; comps, a structured
    array (COMP_DTYPE) of {seed = the smallest py * width + px, area, below = its pixels solid in layer l - 1
    (area for l = 0), x0, y0, x1, y1 = the inclusive bounding box, layer}), then with want_labels labels int32
    (L, H, W) = the pixel's seed or -1, and with return_stats [raster_layers' five figures, components, islands,
    solid pixels]."""
    fp, lp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    r, zz, W, H, s = _layer_args("layer_islands", rect, z, width, height, supersample)
    offs = np.zeros(zz.size + 1, np.int64)
    labels = np.empty((zz.size, H, W), np.int32) if want_labels else None
    stats = (ctypes.c_int64 * 8)()
    C = lib().implisolid_islands(_s(shape), int(bool(ignore_root_matrix)), r.ctypes.data_as(fp), W, H, s, zz.ctypes.data_as(fp),
                                 int(zz.size), int(threshold), int(connectivity), offs.ctypes.data_as(lp),
                                 labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if want_labels else None, stats)
    if C < 0:
        raise ImplisolidError(last_error())
    comps = np.empty(C, COMP_DTYPE)
    if lib().implisolid_islands_copy(comps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) != 0:
        raise ImplisolidError(last_error())
    out = (offs, comps)
    if want_labels:
        out += (labels,)
    if return_stats:
        out += ([int(v) for v in stats],)
    return out


def islands_of(comps):
    """Host only: the records of layer_islands() that are islands (below == 0)."""
    comps = np.asarray(comps)
    return comps[comps["below"] == 0]


def _pass_ms(query, n, enable):
    """implisolid_debug_<query>_ms: sets the timing switch and returns the last timed call's n figures as a tuple
    (n None: the entry returns its one figure itself)."""
    fn = getattr(lib(), "implisolid_debug_%s_ms" % query)
    if n is None:
        return float(fn(int(bool(enable))))
    ms = (ctypes.c_double * n)()
    fn(int(bool(enable)), ms)
    return tuple(float(v) for v in ms)


def islands_kernel_ms(enable=True):
    """Diagnostics: switch the event timing of layer_islands()'s kernels on or off; returns the last timed
    call's (raster passes, tile pass, merge pass, seed rows + scan, records + tally) ms, -1 before any."""
    return _pass_ms("islands", 5, enable)


DIST_DTYPE = np.dtype([(name, np.int64) for name in ("solid", "widest", "widest_at", "unsupported")])
DIST_NONE = 1 << 30


def layer_distance(shape, rect, width, height, z, supersample=1, threshold=1, reach2=0, ignore_root_matrix=False,
                   want_dist=True, return_stats=False):
    """The pixel distance field of the solid's layers z = z[l] on the GPU (include/implisolid.h
    implisolid_layer_distance).  The images are raster_layers'; a pixel is solid iff its coverage >= threshold
    (1 .. supersample^2).  Returns (dist int32 (L, H, W) = +D2 for a solid pixel and -D2 for an empty one, D2
    the exact squared distance in pixels to the nearest pixel of the layer of the other class, DIST_NONE
    where the layer has none -- or None with want_dist=False; records, a structured array (DIST_DTYPE) per
    layer of {solid = its solid pixels, widest = the largest D2 over them (0 without any), widest_at = the
    smallest py * width + px that attains it (-1 without any), unsupported = its solid pixels whose pixel in
    layer l - 1 has dist < -reach2 (0 for l = 0)}), and with return_stats [raster_layers' five figures, solid
    pixels, unsupported pixels, layers whose widest is DIST_NONE]."""
    fp, lp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    r, zz, W, H, s = _layer_args("layer_distance", rect, z, width, height, supersample)
    if not -(1 << 63) <= int(reach2) < (1 << 63):
        raise ImplisolidError("layer_distance: reach2 must be in [0, 2^30)")
    dist = np.empty((zz.size, H, W), np.int32) if want_dist else None
    records = np.zeros(zz.size, DIST_DTYPE)
    stats = (ctypes.c_int64 * 8)()
    rc = lib().implisolid_layer_distance(_s(shape), int(bool(ignore_root_matrix)), r.ctypes.data_as(fp), W, H, s,
                                         zz.ctypes.data_as(fp), int(zz.size), int(threshold), int(reach2),
                                         dist.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if want_dist else None,
                                         records.ctypes.data_as(lp), stats)
    if rc != 0:
        raise ImplisolidError(last_error())
    if return_stats:
        return dist, records, [int(v) for v in stats]
    return dist, records


def offset_mask(dist, r2):
    """Host only: a layer_distance() field grown or eroded by the disc of squared radius |r2| over pixel centres.
    r2 >= 0 grows: the pixels within sqrt(r2) of a solid pixel (dist >= -r2, and not -DIST_NONE: an empty layer
    stays empty), the dilation of the solid mask by that disc.  r2 < 0 erodes: the solid pixels farther than
    sqrt(-r2) from every empty one (dist > -r2), the erosion by the same disc."""
    dist = np.asarray(dist)
    r2 = int(r2)
    if r2 >= 0:
        return (dist >= -r2) & (dist != -DIST_NONE)
    return dist > -r2


def overhang_mask(dist, reach2):
    """Host only: the unsupported pixels of a layer_distance() stack (L, H, W): layer l's solid pixels whose pixel
    in layer l - 1 has dist < -reach2; layer 0 all False.  Its sums per layer are the records' unsupported."""
    dist = np.asarray(dist)
    out = np.zeros(dist.shape, bool)
    out[1:] = (dist[1:] > 0) & (dist[:-1] < -int(reach2))
    return out


def layer_distance_kernel_ms(enable=True):
    """Diagnostics: switch the event timing of layer_distance()'s kernels on or off; returns the last timed
    call's (raster passes, column pass, row pass + records) ms, -1 before any."""
    return _pass_ms("layer_distance", 3, enable)


HOLLOW_DTYPE = np.dtype([(name, np.int64) for name in ("solid", "core")])
HOLLOW_MAX_REACH = 1024


def hollow_wall2(wall_px, pitch_px):
    """Host only: layer_hollow()'s threshold table for a wall of wall_px pixels over layers pitch_px pixels apart
    (include/implisolid.h implisolid_hollow_wall2): int64 (R + 1,), wall2[j] = floor(wall^2 - (j pitch)^2) for every
    j with (j pitch)^2 <= wall^2 -- the digital ellipsoid whose in-plane radius is the wall."""
    w2 = np.empty(HOLLOW_MAX_REACH + 1, np.int64)
    R = lib().implisolid_hollow_wall2(float(wall_px), float(pitch_px), w2.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), int(w2.size))
    if R < 0:
        raise ImplisolidError(last_error())
    return w2[:R + 1].copy()


def layer_hollow(shape, rect, width, height, z, wall2, supersample=1, threshold=1, ends=3, ignore_root_matrix=False,
                 return_stats=False, want_out=True):
    """The solid's layers z = z[l] hollowed to a shell on the GPU (include/implisolid.h implisolid_layer_hollow).
    The images are raster_layers'; a pixel is solid iff its coverage >= threshold.  wall2 (reach + 1 entries,
    non-increasing, hollow_wall2() makes one) holds the squared in-plane radius of the structuring element at a
    layer offset of +-j: voxel (l, py, px) is core iff no empty voxel (m, q) has |m - l| <= reach and |q - p|^2 <=
    wall2[|m - l|].  ends: bit 0 / bit 1 make the layers in front of entry 0 / behind the last entry count as
    empty (a skin forms there); a clear bit means they do not exist.  Returns (out uint8 (L, H, W) = 0 for a core
    voxel and the coverage for every other -- or None with want_out=False; records, a structured array
    (HOLLOW_DTYPE) per layer of {solid, core} voxels), and with return_stats [raster_layers' five figures, solid
    voxels, core voxels, layers whose distance transform was computed]."""
    fp, lp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    r, zz, W, H, s = _layer_args("layer_hollow", rect, z, width, height, supersample)
    try:
        w2 = np.ascontiguousarray(wall2).reshape(-1)
        if w2.size < 1 or w2.dtype.kind not in "iu" or any(not -(1 << 63) <= int(v) < (1 << 63) for v in w2):
            raise OverflowError
        w2 = w2.astype(np.int64)
    except (OverflowError, TypeError, ValueError):
        raise ImplisolidError("layer_hollow: wall2 must be integers in [0, 2^30), one per layer offset 0 .. reach")
    out = np.empty((zz.size, H, W), np.uint8) if want_out else None
    records = np.zeros(zz.size, HOLLOW_DTYPE)
    stats = (ctypes.c_int64 * 8)()
    rc = lib().implisolid_layer_hollow(_s(shape), int(bool(ignore_root_matrix)), r.ctypes.data_as(fp), W, H, s,
                                       zz.ctypes.data_as(fp), int(zz.size), int(threshold), w2.ctypes.data_as(lp),
                                       min(int(w2.size) - 1, 1 << 30), int(ends),
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if want_out else None,
                                       records.ctypes.data_as(lp), stats)
    if rc != 0:
        raise ImplisolidError(last_error())
    if return_stats:
        return out, records, [int(v) for v in stats]
    return out, records


def layer_hollow_kernel_ms(enable=True):
    """Diagnostics: switch the event timing of layer_hollow()'s kernels on or off; returns the last timed call's
    (raster passes, ring copy + column pass, row pass, window pass) ms, -1 before any."""
    return _pass_ms("layer_hollow", 4, enable)


SUPPORT_DTYPE = np.dtype([(name, np.int32) for name in ("p", "depth", "foot", "load")])
SUPPORT_REC_DTYPE = np.dtype([(name, np.int64) for name in ("unsupported", "tips")])


def layer_supports(shape, rect, width, height, z, cell, supersample=1, threshold=1, reach2=0, ignore_root_matrix=False,
                   return_stats=False):
    """Support tips under the solid's layers z = z[l] on the GPU (include/implisolid.h implisolid_layer_supports):
    one tip per non-empty cell of a grid of cell x cell pixels laid over each layer's unsupported pixels --
    layer_distance()'s: solid, and dist < -reach2 at the same pixel of layer l - 1; none in layer 0.  Returns (tips,
    a structured array (SUPPORT_DTYPE) of {p = py * width + px of the cell's unsupported pixel with the largest
    dist, the smallest such p; depth = its dist (DIST_NONE in an all-solid layer); foot = the highest layer below
    whose pixel p is solid, -1 when the column reaches the plate; load = the cell's unsupported pixels}, by layer
    and within a layer by cell (py // cell) * ceil(width / cell) + px // cell; tip_offsets int64 (L + 1,): layer l's
    tips are tips[tip_offsets[l]:tip_offsets[l + 1]]; records, a structured array (SUPPORT_REC_DTYPE) per layer of
    {unsupported, tips}), and with return_stats also [raster_layers' five figures, unsupported pixels, tips, tips
    with foot == -1].  cell=1 lists the unsupported pixels themselves."""
    fp, lp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    r, zz, W, H, s = _layer_args("layer_supports", rect, z, width, height, supersample)
    if not -(1 << 63) <= int(reach2) < (1 << 63):
        raise ImplisolidError("layer_supports: reach2 must be in [0, 2^30)")
    if not 1 <= int(cell) <= 16384:
        raise ImplisolidError("layer_supports: cell must be in [1, 16384]")
    offs = np.zeros(zz.size + 1, np.int64)
    records = np.zeros(zz.size, SUPPORT_REC_DTYPE)
    stats = (ctypes.c_int64 * 8)()
    n = lib().implisolid_layer_supports(_s(shape), int(bool(ignore_root_matrix)), r.ctypes.data_as(fp), W, H, s, zz.ctypes.data_as(fp),
                                        int(zz.size), int(threshold), int(reach2), int(cell), offs.ctypes.data_as(lp),
                                        records.ctypes.data_as(lp), stats)
    if n < 0:
        raise ImplisolidError(last_error())
    tips = np.empty(n, SUPPORT_DTYPE)
    if lib().implisolid_layer_supports_copy(tips.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) != 0:
        raise ImplisolidError(last_error())
    if return_stats:
        return tips, offs, records, [int(v) for v in stats]
    return tips, offs, records


def supports_decode(tips, tip_offsets, width):
    """Host only: where layer_supports()'s tips are: (l, py, px), int64 (T,) each."""
    offs = np.asarray(tip_offsets, np.int64).reshape(-1)
    tips = np.asarray(tips)
    p = (tips["p"] if tips.dtype.names else tips.reshape(-1, 4)[:, 0]).astype(np.int64).reshape(-1)
    W = int(width)
    if W < 1 or offs.size < 1 or offs[0] != 0 or offs[-1] != p.size or (np.diff(offs) < 0).any() or (p < 0).any():
        raise ValueError("supports_decode: tip_offsets must run from 0 to len(tips) without decreasing, width >= 1")
    l = np.repeat(np.arange(offs.size - 1, dtype=np.int64), np.diff(offs))
    return l, p // W, p % W


def layer_supports_kernel_ms(enable=True):
    """Diagnostics: switch the event timing of layer_supports()'s kernels on or off; returns the last timed call's
    (raster passes, column + row passes, cell pass, count + scan + emit + top passes) ms, -1 before any."""
    return _pass_ms("layer_supports", 4, enable)


def layer_runs(shape, rect, width, height, z, supersample=1, threshold=0, ignore_root_matrix=False, return_stats=False):
    """The solid's layers z = z[l] as run-length streams on the GPU (include/implisolid.h implisolid_layer_runs).
    The images are raster_layers'; a pixel's value is its coverage (threshold 0, the grey mode) or coverage >=
    threshold as 0 / 1 (threshold in 1 .. supersample^2).  A layer is the row-major stream p = py * width + px;
    a run starts at p = 0 and wherever the value changes, across row ends too.  Returns (run_offsets int64
    (L + 1,): layer l's runs are [run_offsets[l], run_offsets[l + 1]); start uint32 (R,) = each run's first p, in
    increasing order within its layer; value uint8 (R,); layer_sum int64 (L,) = raster_layers' sums), and with
    return_stats also [raster_layers' five figures, runs, runs with value != 0]."""
    fp, lp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    r, zz, W, H, s = _layer_args("layer_runs", rect, z, width, height, supersample)
    offs = np.zeros(zz.size + 1, np.int64)
    sums = np.zeros(zz.size, np.int64)
    stats = (ctypes.c_int64 * 7)()
    n = lib().implisolid_layer_runs(_s(shape), int(bool(ignore_root_matrix)), r.ctypes.data_as(fp), W, H, s, zz.ctypes.data_as(fp),
                                    int(zz.size), int(threshold), offs.ctypes.data_as(lp), sums.ctypes.data_as(lp), stats)
    if n < 0:
        raise ImplisolidError(last_error())
    start = np.empty(n, np.uint32)
    value = np.empty(n, np.uint8)
    if lib().implisolid_layer_runs_copy(start.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                        value.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) != 0:
        raise ImplisolidError(last_error())
    if return_stats:
        return offs, start, value, sums, [int(v) for v in stats]
    return offs, start, value, sums


def run_lengths(run_offsets, start, layer_pixels):
    """Host only: the lengths int64 (R,) of layer_runs()'s runs: the next run's start minus the run's own, and
    layer_pixels (= width * height) minus the start for the last run of a layer."""
    offs = np.asarray(run_offsets, np.int64).reshape(-1)
    st = np.asarray(start).astype(np.int64).reshape(-1)
    if offs.size < 1 or offs[0] != 0 or offs[-1] != st.size or (np.diff(offs) < 1).any():
        raise ValueError("run_lengths: run_offsets must run from 0 to len(start) with a run in every layer at least")
    end = np.empty_like(st)
    end[:-1] = st[1:]
    end[offs[1:] - 1] = int(layer_pixels)
    return end - st


def runs_decode(run_offsets, start, value, width, height):
    """Host only: the images of layer_runs()'s runs, uint8 (L, height, width)."""
    W, H = int(width), int(height)
    offs = np.asarray(run_offsets, np.int64).reshape(-1)
    lengths = run_lengths(offs, start, W * H)
    if (lengths < 1).any() or (np.asarray(start)[offs[:-1]] != 0).any():
        raise ValueError("runs_decode: every layer's starts must begin at 0 and increase below width * height")
    return np.repeat(np.asarray(value, np.uint8).reshape(-1), lengths).reshape(offs.size - 1, H, W)


def layer_runs_kernel_ms(enable=True):
    """Diagnostics: switch the event timing of layer_runs()'s kernels on or off; returns the last timed call's
    (raster passes, count pass + scan, emit pass) ms, -1 before any."""
    return _pass_ms("layer_runs", 3, enable)


BODY_DTYPE = np.dtype([(name, np.int64) for name in ("seed", "volume", "x0", "y0", "l0", "x1", "y1", "l1")])
BODY_RUN_DTYPE = np.dtype([(name, np.int32) for name in ("start", "length", "body")])


def layer_bodies(shape, rect, width, height, z, supersample=1, threshold=1, target=1, connectivity=None, ignore_root_matrix=False,
                 want_runs=False, return_stats=False):
    """The bodies of the layer stack z = z[l] on the GPU: the connected components of its voxels through all layers
    (include/implisolid.h implisolid_layer_bodies).  The images are raster_layers'; target 1 takes the solid voxels
    (coverage >= threshold), target 0 the empty ones; connectivity is 6 or 26, and None means the dual pair: 26 for
    target 1, 6 for target 0.  Returns (run_offsets int64 (L + 1,): layer l's row runs are [run_offsets[l],
    run_offsets[l + 1]); bodies, a structured array (BODY_DTYPE) in increasing seed of {seed = the smallest l * W * H
    + py * W + px, volume, x0, y0, l0, x1, y1, l1 = the inclusive bounding box}), then with want_runs runs, a
    structured array (BODY_RUN_DTYPE) of {start = py * W + x0, length, body = the index of its body's record} per
    row run, and with return_stats [raster_layers' five figures, row runs, bodies, target voxels]."""
    fp, lp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    r, zz, W, H, s = _layer_args("layer_bodies", rect, z, width, height, supersample)
    if connectivity is None:
        connectivity = 26 if int(target) == 1 else 6
    offs = np.zeros(zz.size + 1, np.int64)
    stats = (ctypes.c_int64 * 8)()
    B = lib().implisolid_layer_bodies(_s(shape), int(bool(ignore_root_matrix)), r.ctypes.data_as(fp), W, H, s, zz.ctypes.data_as(fp),
                                      int(zz.size), int(threshold), int(target), int(connectivity), int(bool(want_runs)),
                                      offs.ctypes.data_as(lp), stats)
    if B < 0:
        raise ImplisolidError(last_error())
    bodies = np.empty(B, BODY_DTYPE)
    runs = np.empty(int(offs[-1]), BODY_RUN_DTYPE) if want_runs else None
    if lib().implisolid_layer_bodies_copy(bodies.ctypes.data_as(lp),
                                          runs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if want_runs else None) != 0:
        raise ImplisolidError(last_error())
    out = (offs, bodies)
    if want_runs:
        out += (runs,)
    if return_stats:
        out += ([int(v) for v in stats],)
    return out


def _body_rows(a, dtype, what):
    """records as a structured array of `dtype`: one already, or integers (n, fields)"""
    a = np.asarray(a)
    if a.dtype.names:
        if a.dtype.names != dtype.names:
            raise ValueError("%s: the records' fields must be %s" % (what, ", ".join(dtype.names)))
        return a.reshape(-1)
    return np.ascontiguousarray(a.reshape(-1, len(dtype.names)), dtype[0]).view(dtype).reshape(-1)


def _runs_decode(run_offsets, runs, width, height, dtype, what):
    """the label stack of row runs {start, length, label} (bodies_decode, cups_decode): the run's label on its voxels, -1 elsewhere"""
    W, H = int(width), int(height)
    offs = np.asarray(run_offsets, np.int64).reshape(-1)
    rr = _body_rows(runs, dtype, what)
    if offs.size < 2 or offs[0] != 0 or offs[-1] != rr.size or (np.diff(offs) < 0).any():
        raise ValueError("%s: run_offsets must run from 0 to len(runs) without decreasing" % what)
    start, length = rr["start"].astype(np.int64), rr["length"].astype(np.int64)
    if (length < 1).any() or (start < 0).any() or (start % W + length > W).any() or (start // W >= H).any():
        raise ValueError("%s: every run must lie inside one image row" % what)
    L = offs.size - 1
    first = start + np.repeat(np.arange(L, dtype=np.int64), np.diff(offs)) * (W * H)
    out = np.full(L * H * W, -1, np.int32)
    # every voxel of every run: its run's first key plus its position in the run
    at = np.repeat(first - np.concatenate(([0], np.cumsum(length)[:-1])), length) + np.arange(int(length.sum()), dtype=np.int64)
    out[at] = np.repeat(rr[dtype.names[2]], length)
    return out.reshape(L, H, W)


def bodies_decode(run_offsets, runs, width, height):
    """Host only: the label stack of layer_bodies()'s row runs, int32 (L, height, width): the voxel's body index,
    or -1 where the voxel is not of the target class."""
    return _runs_decode(run_offsets, runs, width, height, BODY_RUN_DTYPE, "bodies_decode")


def enclosed_voids(bodies, width, height, n_layers):
    """Host only: the records of layer_bodies() that touch no face of the stack (x0 > 0, y0 > 0, l0 > 0, x1 < width -
    1, y1 < height - 1, l1 < n_layers - 1).  Meant for target=0: the empty regions sealed on all sides."""
    b = _body_rows(bodies, BODY_DTYPE, "enclosed_voids")
    return b[(b["x0"] > 0) & (b["y0"] > 0) & (b["l0"] > 0) & (b["x1"] < int(width) - 1) & (b["y1"] < int(height) - 1)
             & (b["l1"] < int(n_layers) - 1)]


def floating_bodies(bodies):
    """Host only: the records of layer_bodies() that start above the first layer (l0 > 0).  Meant for target=1: the
    bodies that do not stand on the build plate."""
    b = _body_rows(bodies, BODY_DTYPE, "floating_bodies")
    return b[b["l0"] > 0]


def layer_bodies_kernel_ms(enable=True):
    """Diagnostics: switch the event timing of layer_bodies()'s kernels on or off; returns the last timed call's
    (raster passes, row-run count + scan + emit, link, finish) ms, -1 before any."""
    return _pass_ms("layer_bodies", 4, enable)


CUP_DTYPE = np.dtype([(name, np.int64) for name in ("seed", "area", "x0", "y0", "x1", "y1", "pocket")])
CUP_RUN_DTYPE = np.dtype([(name, np.int32) for name in ("start", "length", "cup")])


def layer_cups(shape, rect, width, height, z, supersample=1, threshold=1, connectivity=6, ignore_root_matrix=False, want_runs=False,
               return_stats=False):
    """The suction cups of the layer stack z = z[l] on the GPU (include/implisolid.h implisolid_layer_cups): per layer
    l the empty voxels (coverage < threshold) of layer l whose pocket -- their connected class among the empty voxels
    of layers 0 .. l, 6- or 26-connected -- reaches no pixel of the image frame.  The order of z is the print order;
    the plate below layer 0 and the film above layer l are closed.  The images are raster_layers'.  Returns
    (cup_offsets int64 (L + 1,): layer l's cups are [cup_offsets[l], cup_offsets[l + 1]); cups, a structured array
    (CUP_DTYPE) of {seed = the smallest py * W + px of the cup in its layer, area, x0, y0, x1, y1 = the inclusive box,
    pocket = the smallest key l' * W * H + py * W + px of the whole pocket}, layer by layer in increasing seed), then
    with want_runs run_offsets int64 (L + 1,) and runs, a structured array (CUP_RUN_DTYPE) of {start = py * W + x0,
    length, cup = the index of its cup's record} per cupped row run, and with return_stats [raster_layers' five
    figures, the empty row runs of the stack, cups, cupped voxels]."""
    fp, lp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    r, zz, W, H, s = _layer_args("layer_cups", rect, z, width, height, supersample)
    offs = np.zeros(zz.size + 1, np.int64)
    roffs = np.zeros(zz.size + 1, np.int64)
    stats = (ctypes.c_int64 * 8)()
    C = lib().implisolid_layer_cups(_s(shape), int(bool(ignore_root_matrix)), r.ctypes.data_as(fp), W, H, s, zz.ctypes.data_as(fp),
                                    int(zz.size), int(threshold), int(connectivity), int(bool(want_runs)), offs.ctypes.data_as(lp),
                                    roffs.ctypes.data_as(lp), stats)
    if C < 0:
        raise ImplisolidError(last_error())
    cups = np.empty(C, CUP_DTYPE)
    runs = np.empty(int(roffs[-1]), CUP_RUN_DTYPE) if want_runs else None
    if lib().implisolid_layer_cups_copy(cups.ctypes.data_as(lp),
                                        runs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if want_runs else None) != 0:
        raise ImplisolidError(last_error())
    out = (offs, cups)
    if want_runs:
        out += (roffs, runs)
    if return_stats:
        out += ([int(v) for v in stats],)
    return out


def cups_decode(run_offsets, runs, width, height):
    """Host only: the label stack of layer_cups()'s cupped row runs, int32 (L, height, width): the index of the
    voxel's cup, or -1 where the voxel lies in no cup."""
    return _runs_decode(run_offsets, runs, width, height, CUP_RUN_DTYPE, "cups_decode")


def cup_areas(cup_offsets, cups):
    """Host only: the sealed area of every layer, int64 (L,): the areas of layer_cups()'s records added up per layer."""
    offs = np.asarray(cup_offsets, np.int64).reshape(-1)
    c = _body_rows(cups, CUP_DTYPE, "cup_areas")
    if offs.size < 2 or offs[0] != 0 or offs[-1] != c.size or (np.diff(offs) < 0).any():
        raise ValueError("cup_areas: cup_offsets must run from 0 to len(cups) without decreasing")
    total = np.concatenate(([0], np.cumsum(c["area"].astype(np.int64))))
    return total[offs[1:]] - total[offs[:-1]]


def layer_cups_kernel_ms(enable=True):
    """Diagnostics: switch the event timing of layer_cups()'s kernels on or off; returns the last timed call's
    (raster passes, row-run count + scan + emit + frame, the layers' link + mark + head, finish) ms, -1 before any."""
    return _pass_ms("layer_cups", 4, enable)


def ray_params(t0, t1, steps):
    """Host only: the sample parameters of raycast(), float32 (steps + 1,): ts[k] = t0 + k * ((t1 - t0) /
    steps) in separately rounded float operations, ts[steps] = t1 (implisolid_ray_params)."""
    fp = ctypes.POINTER(ctypes.c_float)
    N = int(steps)
    if not 1 <= N <= 65536:
        raise ImplisolidError("ray_params: steps must be in [1, 65536]")
    ts = np.empty(N + 1, np.float32)
    if lib().implisolid_ray_params(float(np.float32(t0)), float(np.float32(t1)), N, ts.ctypes.data_as(fp)) != 0:
        raise ImplisolidError(last_error())
    return ts


def _rays(origins, dirs, what):
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ImplisolidError("%s: %d origins for %d directions" % (what, o.shape[0], d.shape[0]))
    return o, d


def raycast(shape, origins, dirs, t0, t1, steps, bisect=16, ignore_root_matrix=False, want_normals=True, return_stats=False):
    """Rays against the solid on the GPU (include/implisolid.h implisolid_raycast): per ray the first of
    the steps + 1 samples ray_params(t0, t1, steps) of p(t) = origin + t * dir that is solid, refined by
    `bisect` bisection rounds.  Returns (hit int32 (n,) = the sample's index, 0 for a ray that starts
    inside, -1 for a miss; t float32 (n,), t1 on a miss; f float32 (n,) = the field at the returned point;
    normals float32 (n, 3), zero rows on a miss, or None with want_normals=False), and with return_stats
    also [segments, segments skipped, segments evaluated, rays that hit, rays that start inside, chunks].
    ray_points(origins, dirs, t) gives the hit positions."""
    fp = ctypes.POINTER(ctypes.c_float)
    o, d = _rays(origins, dirs, "raycast")
    n = o.shape[0]
    hit = np.empty(n, np.int32)
    t = np.empty(n, np.float32)
    f = np.empty(n, np.float32)
    nrm = np.empty((n, 3), np.float32) if want_normals else None
    stats = (ctypes.c_int64 * 6)()
    rc = lib().implisolid_raycast(_s(shape), int(bool(ignore_root_matrix)), o.ctypes.data_as(fp), d.ctypes.data_as(fp), n,
                                  float(np.float32(t0)), float(np.float32(t1)), int(steps), int(bisect),
                                  hit.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), t.ctypes.data_as(fp), f.ctypes.data_as(fp),
                                  nrm.ctypes.data_as(fp) if want_normals else None, stats)
    if rc != 0:
        raise ImplisolidError(last_error())
    if return_stats:
        return hit, t, f, nrm, [int(v) for v in stats]
    return hit, t, f, nrm


def ray_points(origins, dirs, t):
    """Host only: p(t) = origin + t * dir per ray, float32 (n, 3), the product and the sum rounded to
    float32 separately as raycast() computes them (t: one parameter per ray, or a scalar)."""
    o, d = _rays(origins, dirs, "ray_points")
    tt = np.broadcast_to(np.asarray(t, np.float32).reshape(-1), (o.shape[0],))
    with np.errstate(all="ignore"):
        return np.add(o, np.multiply(tt[:, None], d, dtype=np.float32), dtype=np.float32)


def view_rays(eye, target, up, width, height, fov_y=None, ortho_height=None):
    """Host only: the rays of a width x height view from `eye` towards `target`, (origins, dirs) float32
    (height * width, 3) each, row-major with row 0 at the top, through the pixel centres; computed in
    float64 and rounded once.  fov_y (radians, the full vertical angle): a pinhole at eye, unit
    directions.  ortho_height (the view's height in world units): parallel rays along the view
    direction from the view plane through eye.  Exactly one of the two must be given."""
    if (fov_y is None) == (ortho_height is None):
        raise ValueError("view_rays: give exactly one of fov_y and ortho_height")
    W, H = int(width), int(height)
    if W < 1 or H < 1:
        raise ValueError("view_rays: width and height must be at least 1")
    e, tg, u = (np.asarray(v, np.float64).reshape(3) for v in (eye, target, up))
    fwd = tg - e
    right = np.cross(fwd, u)
    if not np.linalg.norm(fwd) > 0 or not np.linalg.norm(right) > 0:
        raise ValueError("view_rays: eye == target, or up is parallel to the view direction")
    fwd /= np.linalg.norm(fwd)
    right /= np.linalg.norm(right)
    upv = np.cross(right, fwd)
    half_h = np.tan(0.5 * float(fov_y)) if fov_y is not None else 0.5 * float(ortho_height)
    if not (np.isfinite(half_h) and half_h > 0):
        raise ValueError("view_rays: fov_y must be in (0, pi), ortho_height above 0")
    half_w = half_h * W / H
    x = (2.0 * (np.arange(W) + 0.5) / W - 1.0) * half_w
    y = (1.0 - 2.0 * (np.arange(H) + 0.5) / H) * half_h            # row 0 is the top row
    off = (y[:, None, None] * upv + x[None, :, None] * right).reshape(-1, 3)
    if fov_y is not None:
        d = fwd + off
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        o = np.broadcast_to(e, d.shape)
    else:
        o = e + off
        d = np.broadcast_to(fwd, o.shape)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def render_view(shape, eye, target, up, width, height, t0, t1, steps, bisect=16, fov_y=None, ortho_height=None,
                ignore_root_matrix=False, return_stats=False):
    """A depth-and-normal image of the solid without a mesh: raycast() over view_rays().  Returns (depth
    float32 (height, width) = the hit's ray parameter, the distance along the unit direction, NaN where
    the ray missed; normals float32 (height, width, 3); mask bool (height, width) = the ray hit), and
    with return_stats also raycast()'s stats."""
    o, d = view_rays(eye, target, up, width, height, fov_y=fov_y, ortho_height=ortho_height)
    hit, t, f, nrm, stats = raycast(shape, o, d, t0, t1, steps, bisect, ignore_root_matrix, True, True)
    H, W = int(height), int(width)
    mask = (hit >= 0).reshape(H, W)
    depth = np.where(mask, t.reshape(H, W), np.float32(np.nan)).astype(np.float32)
    out = (depth, nrm.reshape(H, W, 3), mask)
    return out + (stats,) if return_stats else out


def raycast_kernel_ms(enable=True):
    """Diagnostics: switch the event timing of raycast()'s kernels on or off; returns the last timed
    call's (march ms, finish ms), -1 before any."""
    return _pass_ms("raycast", 2, enable)


def ray_spans(shape, origins, dirs, t0, t1, steps, bisect=16, ignore_root_matrix=False, want_normals=False, return_stats=False):
    """Every solid span along each ray on the GPU (include/implisolid.h implisolid_ray_spans): the maximal
    runs of solid samples among the steps + 1 samples ray_params(t0, t1, steps) of p(t) = origin + t * dir,
    entries and exits refined by `bisect` bisection rounds.  Returns (offsets int64 (n + 1,): ray r's spans
    are rows offsets[r]:offsets[r + 1], in order along the ray; k int32 (S, 2) = {k_in, k_out}, the first
    solid sample and the first sample behind the span, steps + 1 where the ray ends inside; t float32 (S, 2)
    and f float32 (S, 2) = the parameter and the field at {entry, exit}, both on the solid side; normals
    float32 (S, 2, 3), or None without want_normals), and with return_stats also [segments, segments proved
    outside, proved solid, evaluated, spans, rays with a span, rays that start inside, chunks]."""
    fp = ctypes.POINTER(ctypes.c_float)
    o, d = _rays(origins, dirs, "ray_spans")
    n = o.shape[0]
    offs = np.zeros(n + 1, np.int64)
    stats = (ctypes.c_int64 * 8)()
    S = lib().implisolid_ray_spans(_s(shape), int(bool(ignore_root_matrix)), o.ctypes.data_as(fp), d.ctypes.data_as(fp), n,
                                   float(np.float32(t0)), float(np.float32(t1)), int(steps), int(bisect), int(bool(want_normals)),
                                   offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), stats)
    if S < 0:
        raise ImplisolidError(last_error())
    k = np.empty((S, 2), np.int32)
    t = np.empty((S, 2), np.float32)
    f = np.empty((S, 2), np.float32)
    nrm = np.empty((S, 2, 3), np.float32) if want_normals else None
    if lib().implisolid_ray_spans_copy(k.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), t.ctypes.data_as(fp), f.ctypes.data_as(fp),
                                       nrm.ctypes.data_as(fp) if want_normals else None) != 0:
        raise ImplisolidError(last_error())
    if return_stats:
        return offs, k, t, f, nrm, [int(v) for v in stats]
    return offs, k, t, f, nrm


def span_lengths(offsets, t, dirs):
    """Host only: per ray the solid length along it and its span count, (length float64 (n,), count int64
    (n,)), from ray_spans()'s offsets and t: the sum in span order of (float64(t_out) - float64(t_in)) * |d|,
    |d| in float64 (np.bincount with weights)."""
    offs = np.asarray(offsets, np.int64).reshape(-1)
    n = offs.size - 1
    tt = np.asarray(t, np.float32).reshape(-1, 2).astype(np.float64)
    d = np.asarray(dirs, np.float32).reshape(-1, 3).astype(np.float64)
    if n < 0 or d.shape[0] != n or tt.shape[0] != (offs[n] if n >= 0 else 0):
        raise ImplisolidError("span_lengths: offsets (n + 1,), t (offsets[n], 2) and dirs (n, 3) do not fit together")
    count = np.diff(offs)
    ray = np.repeat(np.arange(n), count)
    length = np.bincount(ray, weights=(tt[:, 1] - tt[:, 0]) * np.sqrt((d * d).sum(axis=1))[ray], minlength=n)
    return length.astype(np.float64), count.astype(np.int64)


def xray_view(shape, eye, target, up, width, height, t0, t1, steps, bisect=16, fov_y=None, ortho_height=None,
              ignore_root_matrix=False, return_stats=False):
    """An accumulated-thickness image of the solid without a mesh: ray_spans() over view_rays(), reduced by
    span_lengths().  Returns (thickness float64 (height, width) = the solid length along the pixel's ray,
    count int32 (height, width) = its spans), and with return_stats also ray_spans()'s stats."""
    o, d = view_rays(eye, target, up, width, height, fov_y=fov_y, ortho_height=ortho_height)
    offs, k, t, f, _, stats = ray_spans(shape, o, d, t0, t1, steps, bisect, ignore_root_matrix, False, True)
    length, count = span_lengths(offs, t, d)
    H, W = int(height), int(width)
    out = (length.reshape(H, W), count.astype(np.int32).reshape(H, W))
    return out + (stats,) if return_stats else out


def ray_spans_kernel_ms(enable=True):
    """Diagnostics: switch the event timing of ray_spans()'s kernels on or off; returns the last timed
    call's (march ms, scan + tally + emit ms, refine ms), -1 before any."""
    return _pass_ms("ray_spans", 3, enable)


def mass_mids(box, depth):
    """Host only: the sample table of mass_moments, float32 (3, 2^depth) (x, y, z rows):
    mid[k] = edge[k] + 0.5f * (edge[k + 1] - edge[k]) over bounds_edges(box, depth)."""
    fp = ctypes.POINTER(ctypes.c_float)
    b = _box6(box, "mass_mids")
    if not 3 <= int(depth) <= 10:
        raise ImplisolidError("mass_mids: depth must be in [3, 10]")
    out = np.empty((3, 1 << int(depth)), np.float32)
    if lib().implisolid_mass_mids(b.ctypes.data_as(fp), int(depth), out.ctypes.data_as(fp)) != 0:
        raise ImplisolidError(last_error())
    return out


def mass_moments(shape, box, depth, ignore_root_matrix=False, return_stats=False):
    """The integer moments of the solid cells of `shape` on the 2^depth-cell grid of box {xmin, xmax, ymin,
    ymax, zmin, zmax}, summed on the GPU (include/implisolid.h implisolid_mass).  Returns (moments
    uint64 (10,) = [n, Si, Sj, Sk, Sii, Sjj, Skk, Sij, Sjk, Sik], layer_cells int64 (N,)), and with
    return_stats also [boxes bounded, cells counted whole from solid boxes, samples evaluated, reruns
    after a list overflow]."""
    fp = ctypes.POINTER(ctypes.c_float)
    b = _box6(box, "mass_moments")
    if not 3 <= int(depth) <= 10:
        raise ImplisolidError("mass_moments: depth must be in [3, 10]")
    mom = np.zeros(10, np.uint64)
    layers = np.zeros(1 << int(depth), np.int64)
    stats = (ctypes.c_int64 * 4)()
    rc = lib().implisolid_mass(_s(shape), int(bool(ignore_root_matrix)), b.ctypes.data_as(fp), int(depth),
                               mom.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                               layers.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), stats)
    if rc < 0:
        raise ImplisolidError(last_error())
    if return_stats:
        return mom, layers, [int(v) for v in stats]
    return mom, layers


def mass_physical(box, depth, moments):
    """Host only: (empty, out float64 (10,) = [volume, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Iyz, Ixz]) from the
    integer moments (implisolid_mass_physical)."""
    b = _box6(box, "mass_physical")
    m = np.ascontiguousarray(moments, np.uint64).reshape(-1)
    if m.size != 10:
        raise ValueError("mass_physical: ten moments")
    out = np.zeros(10, np.float64)
    rc = lib().implisolid_mass_physical(b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(depth),
                                        m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if rc < 0:
        raise ImplisolidError(last_error())
    return rc == 0, out


def mass_properties(shape, box, depth, ignore_root_matrix=False):
    """Volume, centre of mass and inertia tensor (about the centre of mass, unit density) of the solid
    inside box, as the union of its solid cells on the 2^depth grid: dict(volume, centre (3,), inertia
    (3, 3), layer_area (N,), cells, moments, empty).  An empty solid gives zeros and empty = True."""
    mom, layers = mass_moments(shape, box, depth, ignore_root_matrix)
    empty, out = mass_physical(box, depth, mom)
    b = _box6(box, "mass_properties").astype(np.float64)
    N = float(1 << int(depth))
    dx, dy = (b[1] - b[0]) / N, (b[3] - b[2]) / N
    inertia = np.array([[out[4], out[7], out[9]], [out[7], out[5], out[8]], [out[9], out[8], out[6]]])
    return {"volume": float(out[0]), "centre": out[1:4].copy(), "inertia": inertia,
            "layer_area": layers.astype(np.float64) * dx * dy, "cells": int(mom[0]), "moments": mom, "empty": bool(empty)}


def parse_fit_box(mc_settings):
    """Host only: the "fit_box" settings key as a build reads it: dict(enabled, depth, margin)."""
    out = (ctypes.c_int32 * 3)()
    if lib().implisolid_parse_fit_box(_s(mc_settings), out) != 0:
        raise ImplisolidError(last_error())
    return {"enabled": int(out[0]), "depth": int(out[1]), "margin": int(out[2])}


def last_fit_box():
    """The box (float32[6]) the last build_geometry used if the "fit_box" key fitted it, else None."""
    out = np.empty(6, np.float32)
    return out if lib().implisolid_last_fit_box(out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == 1 else None


def debug_bounds_ms(enable=True):
    """Diagnostics: switch HIP-event timing of the bounds descent's level launches on or off; returns
    the last timed descent's milliseconds (-1.0: none yet)."""
    return _pass_ms("bounds", None, enable)


def debug_eval_modes(shape, pts, modes, ignore_root_matrix=False):
    """Diagnostics: the pruned point interpreter at pts [n, 3], each with its own modes word."""
    x = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    m = np.ascontiguousarray(modes, np.uint64).reshape(-1)
    if m.size != x.shape[0]:
        raise ValueError("debug_eval_modes: one modes word per point")
    out = np.empty(x.shape[0], np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = lib().implisolid_debug_eval_modes(_s(shape), int(bool(ignore_root_matrix)), x.ctypes.data_as(fp),
                                           m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), x.shape[0],
                                           out.ctypes.data_as(fp))
    if rc != 0:
        raise ImplisolidError(last_error())
    return out


def program_info(shape, ignore_root_matrix=False):
    """Host-only: compile an MP5 tree; returns (n_instr, depth, n_mats, inverse matrices [n,12])."""
    L = lib()
    info = (ctypes.c_int32 * 4)()
    mats = np.zeros((256, 12), np.float32)
    rc = L.implisolid_program_info(_s(shape), int(bool(ignore_root_matrix)), info,
                                   mats.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    if rc != 0:
        raise ImplisolidError(last_error())
    return info[0], info[1], info[2], mats[:info[2]].copy()


# ---- device slab pipeline (bench / multi-GPU) -----------------------------------------------------
class Slab:
    """One Z-slab of one object on the current device.  Stream = a hipStream_t handle (int)."""

    def __init__(self, shape, mc_settings, rank=0, nranks=1, cuts=None):
        """cuts: nranks + 1 cell-layer boundaries (slab_balance) -- rank r takes [cuts[r], cuts[r+1]);
        None: the equal-layer split (slab_partition)."""
        if cuts is not None:
            if len(cuts) != nranks + 1:
                raise ImplisolidError("Slab: cuts must hold nranks + 1 boundaries")
            self.h = lib().implisolid_slab_create_range(_s(shape), _s(mc_settings), int(cuts[rank]), int(cuts[rank + 1]))
        else:
            self.h = lib().implisolid_slab_create(_s(shape), _s(mc_settings), int(rank), int(nranks))
        if not self.h:
            raise ImplisolidError(last_error())
        g = (ctypes.c_int32 * 8)()
        lib().implisolid_slab_grid(self.h, g)
        self.R, self.res, self.cz0, self.cz1, self.cz_emit, self.fz0, self.fz1, self.depth = list(g)

    def _rc(self, rc):
        if rc != 0:
            raise ImplisolidError(last_error())

    def eval(self, stream=0):
        self._rc(lib().implisolid_slab_eval(self.h, ctypes.c_void_p(stream)))

    def count(self, stream=0):
        self._rc(lib().implisolid_slab_count(self.h, ctypes.c_void_p(stream)))

    def emit(self, d_offsets=0, stream=0):
        self._rc(lib().implisolid_slab_emit(self.h, ctypes.c_void_p(d_offsets or None), ctypes.c_void_p(stream)))

    def emit_verts(self, stream=0):
        """vertex pass alone (slab-local ids, no offsets needed)"""
        self._rc(lib().implisolid_slab_emit_verts(self.h, ctypes.c_void_p(stream)))

    def emit_faces(self, d_offsets=0, d_gathered=0, rank=0, stream=0):
        """face pass: offsets from device [Voff, Foff], or from every rank's gathered counts"""
        self._rc(lib().implisolid_slab_emit_faces(self.h, ctypes.c_void_p(d_offsets or None),
                                                  ctypes.c_void_p(d_gathered or None), int(rank),
                                                  ctypes.c_void_p(stream)))

    def counters_ptr(self):
        return lib().implisolid_slab_counters(self.h)

    def counts(self, stream=0):
        out = (ctypes.c_uint32 * 3)()
        self._rc(lib().implisolid_slab_counts(self.h, ctypes.c_void_p(stream), out))
        return int(out[0]), int(out[1]), bool(out[2])

    def copy_counts(self, d_dst, stream=0):
        """async: counters [own incl. halo, faces, active, halo] -> device uint32[4] at d_dst"""
        self._rc(lib().implisolid_slab_copy_counts(self.h, ctypes.c_void_p(d_dst), ctypes.c_void_p(stream)))

    def copy_mesh(self, d_verts, d_faces, nv, nf, stream=0):
        """async device-to-device copy of the emitted mesh into caller-owned device buffers"""
        self._rc(lib().implisolid_slab_copy_mesh(self.h, ctypes.c_void_p(d_verts or None), ctypes.c_void_p(d_faces or None),
                                                 int(nv), int(nf), ctypes.c_void_p(stream)))

    def set_offsets(self, voff, foff):
        self._rc(lib().implisolid_slab_set_offsets(self.h, int(voff), int(foff)))

    def download(self, nv, nf, stream=0):
        v = np.empty((nv, 3), np.float32)
        f = np.empty((nf, 3), np.int32)
        self._rc(lib().implisolid_slab_download(self.h, v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                f.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_void_p(stream)))
        return v, f

    def emit_normals(self, stream=0):
        """async, after emit / emit_verts: the normals of the slab's emitted vertices (device)"""
        self._rc(lib().implisolid_slab_emit_normals(self.h, ctypes.c_void_p(stream)))

    def normals_ptr(self):
        return lib().implisolid_slab_normals(self.h)

    def download_normals(self, nv, stream=0):
        """blocking host copy of the normals emit_normals wrote, float32 [nv, 3]"""
        n = np.empty((nv, 3), np.float32)
        self._rc(lib().implisolid_slab_download_normals(self.h, n.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                        ctypes.c_void_p(stream)))
        return n

    def run(self, stream=0):
        """eval + count + emit with the host-set offsets; returns (nv, nf) (blocking)."""
        self.eval(stream)
        self.count(stream)
        nv, nf, grew = self.counts(stream)
        self.emit(0, stream)
        nv, nf, of = self.counts(stream)
        if of:
            self.emit(0, stream)
            nv, nf, of = self.counts(stream)
            if of:
                raise ImplisolidError("slab output overflow")
        return nv, nf

    def verts_ptr(self):
        return lib().implisolid_slab_verts(self.h)

    def faces_ptr(self):
        return lib().implisolid_slab_faces(self.h)

    def field_ptr(self):
        return lib().implisolid_slab_field(self.h)

    KERNELS = ("brick_modes", "eval_field", "mc_count", "mc_scan", "mc_verts", "mc_faces")
    # one figure per kernel (Engine::kernel_times_each); names as in the rocprofv3 kernel trace
    EACH_KERNEL = ("impli_coarse_modes", "impli_brick_refine", "k_brick_fill", "impli_eval_bricks", "k_mc_count",
                   "k_unit_scan", "k_mc_cells", "k_mc_faces")

    def set_timing(self, on=True):
        self._rc(lib().implisolid_slab_set_timing(self.h, 1 if on else 0))

    def kernel_times(self):
        """ms per kernel of the last timed eval/count/emit (HIP events on the launch stream)."""
        out = (ctypes.c_float * 6)()
        self._rc(lib().implisolid_slab_kernel_times(self.h, out))
        return dict(zip(self.KERNELS, [float(x) for x in out]))

    def kernel_times_each(self):
        """ms per kernel (coarse, refine and fill split out of the brick pass) of the last timed calls."""
        out = (ctypes.c_float * 8)()
        self._rc(lib().implisolid_slab_kernel_times_each(self.h, out))
        return dict(zip(self.EACH_KERNEL, [float(x) for x in out]))

    def stats(self):
        """After count(): units, non-empty units, owned vertices, triangles, active cells, halo-owned,
        cells, mixed coarse boxes, halo-owned as the vertex pass reads it, unit parts."""
        out = (ctypes.c_int64 * 10)()
        n = lib().implisolid_slab_stats_n(self.h, out, 10)
        self._rc(-1 if n < 0 else 0)
        keys = ["units", "nonempty_units", "own", "tri", "act", "halo_own", "cells", "mixed_coarse_boxes",
                "halo_own_verts_pass", "unit_parts"]
        return dict(zip(keys, [int(x) for x in out]))

    def used_jit(self):
        return bool(lib().implisolid_slab_used_jit(self.h))

    def jit_module(self):
        """The tree kernels of the last eval: "interpreter", "shape" (JIT module per tree shape) or
        "baked" (the object's module with its matrices as literals)."""
        return ("interpreter", "shape", "baked")[lib().implisolid_slab_used_jit(self.h)]

    def brick_stats(self):
        """[bricks, mixed-sign bricks, sign-filled bricks] of the last eval."""
        out = (ctypes.c_int64 * 3)()
        self._rc(lib().implisolid_slab_brick_stats(self.h, out))
        return [int(x) for x in out]

    def read_fill(self):
        """Blocking host copy of the per-brick fill bytes of the last eval, shape (nbz, nby, nbx):
        class (bits 0-1) | 0x08 candidate | fill class << 4 | 0x80 claimed."""
        L = lib()
        dims = (ctypes.c_int32 * 3)()
        n = L.implisolid_slab_read_fill(self.h, None, 0, dims)
        _check()
        out = np.empty(n, np.uint8)
        L.implisolid_slab_read_fill(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n, dims)
        _check()
        return out.reshape(int(dims[2]), int(dims[1]), int(dims[0]))

    def read_signs(self):
        """Blocking host copy of the sample signs (1 where value < 0), shape (layers, n, n)."""
        L = lib()
        n = L.implisolid_slab_read_signs(self.h, None, 0)
        _check()
        out = np.empty(n, np.uint8)
        L.implisolid_slab_read_signs(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n)
        _check()
        n_side = self.R + 3
        return out.reshape(-1, n_side, n_side)

    def read_field(self):
        """Blocking host copy of the stored field samples, shape (layers, n, n)."""
        L = lib()
        n = L.implisolid_slab_read_field(self.h, None, 0)
        _check()
        out = np.empty(n, np.float32)
        L.implisolid_slab_read_field(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n)
        _check()
        n_side = self.R + 3          # samples 1 .. res-2 per axis, the sealed ring included
        return out.reshape(-1, n_side, n_side)

    def close(self):
        if self.h:
            lib().implisolid_slab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Ob02Shard:
    """The OB02 loop on one Z-slab shard (include/implisolid.h implisolid_ob02_*): load the whole MC
    mesh (device pointers) owning vertices [v0, v1); resample() / project() update the owned
    vertices; get_verts / set_verts move the current vertices to and from a device buffer for the
    exchange between steps (distributed.ob02_sharded drives the loop).  Every call blocks."""

    def __init__(self, shape, mc_settings):
        self.h = lib().implisolid_ob02_create(_s(shape), _s(mc_settings))
        if not self.h:
            raise ImplisolidError(last_error())

    def _rc(self, rc):
        if rc != 0:
            raise ImplisolidError(last_error())

    def load(self, d_verts, nv, d_faces, nf, v0, v1):
        self._rc(lib().implisolid_ob02_load(self.h, ctypes.c_void_p(d_verts), int(nv), ctypes.c_void_p(d_faces), int(nf),
                                            int(v0), int(v1)))

    def resample(self):
        self._rc(lib().implisolid_ob02_resample(self.h))

    def project(self):
        self._rc(lib().implisolid_ob02_project(self.h))

    def subdivide(self, amplitude):
        self._rc(lib().implisolid_ob02_subdivide(self.h, float(amplitude)))

    def counts(self):
        out = (ctypes.c_int64 * 2)()
        self._rc(lib().implisolid_ob02_counts(self.h, out))
        return int(out[0]), int(out[1])

    def ranges(self):
        """[v0, v1) owned vertices, [f0, f1) work faces, [c0, c1) centroid faces"""
        out = (ctypes.c_int64 * 6)()
        self._rc(lib().implisolid_ob02_ranges(self.h, out))
        return tuple(int(x) for x in out)

    # stream-ordered form (implisolid_ob02_attach ...): nothing below blocks the host
    def attach(self, d_verts, nv, d_faces, nf, v0, v1, after_stream=0):
        """The caller's device vertex array becomes the working one (updated in place; keep it alive);
        the handle's stream is ordered after `after_stream` by an event."""
        self._rc(lib().implisolid_ob02_attach(self.h, ctypes.c_void_p(d_verts), int(nv), ctypes.c_void_p(d_faces), int(nf),
                                              int(v0), int(v1), ctypes.c_void_p(after_stream)))

    def stream(self):
        """The handle's HIP stream (an int for torch.cuda.ExternalStream)."""
        return int(lib().implisolid_ob02_stream(self.h) or 0)

    def resample_async(self):
        self._rc(lib().implisolid_ob02_resample_async(self.h))

    def project_async(self):
        self._rc(lib().implisolid_ob02_project_async(self.h))

    def unpack(self, d_rows, row_len, voff, rank):
        """Copy every rank's row but `rank`'s (all-gathered owned ranges, equal rows of row_len floats)
        into the vertex array, on the handle's stream."""
        arr = (ctypes.c_int64 * len(voff))(*[int(x) for x in voff])
        self._rc(lib().implisolid_ob02_unpack(self.h, ctypes.c_void_p(d_rows), int(row_len), arr, len(voff) - 1, int(rank)))

    def halo(self):
        """[h0, h1): the vertices the next resampling reads."""
        out = (ctypes.c_int64 * 2)()
        self._rc(lib().implisolid_ob02_halo(self.h, out))
        return int(out[0]), int(out[1])

    def get_verts(self, d_dst):
        self._rc(lib().implisolid_ob02_get_verts(self.h, ctypes.c_void_p(d_dst)))

    def set_verts(self, d_src):
        self._rc(lib().implisolid_ob02_set_verts(self.h, ctypes.c_void_p(d_src)))

    def download(self):
        nv, nf = self.counts()
        v = np.empty((nv, 3), np.float32)
        f = np.empty((nf, 3), np.int32)
        self._rc(lib().implisolid_ob02_download(self.h, v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                f.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return v, f

    def close(self):
        if self.h:
            lib().implisolid_ob02_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """A stream of objects polygonised with one mc-settings dict (BASELINE config 5).  n_streams=0:
    merged launches (every stage once for all objects, interpreter kernels); n_streams >= 1: one
    hipGraph per object (JIT tree kernels) replayed over that many streams.  run() is async on
    `stream`; counts()/download() block.  With "normals": {"enabled": 1} in the settings (or
    normals=True, which merges the key into a copy of them) every run() also computes each object's
    per-vertex normals on the device, behind its face pass: normals(i), download(i, normals=True)."""

    def __init__(self, shapes, mc_settings, n_streams=4, normals=False):
        L = lib()
        enc = [_s(sh) for sh in shapes]
        arr = (ctypes.c_char_p * len(enc))(*enc)
        self.h = L.implisolid_batch_create(arr, len(enc), _s(_with_normals(mc_settings, normals)), int(n_streams))
        if not self.h:
            raise ImplisolidError(last_error() or "implisolid_batch_create failed")
        info = (ctypes.c_int32 * 4)()
        secs = ctypes.c_double(0)
        L.implisolid_batch_info(self.h, info, ctypes.byref(secs))
        self.n, self.n_streams, self.graphs, self.jit_seconds = int(info[0]), int(info[1]), bool(info[2]), secs.value
        self.merged = bool(info[3])
        # (an older experimental build, IMPLISOLID_LIB, has no such entry: its streams compute none)
        has = getattr(L, "implisolid_batch_has_normals", None)
        self.has_normals = bool(has(self.h)) if has else False

    def run(self, stream=None):
        if lib().implisolid_batch_run(self.h, stream) != 0:
            raise ImplisolidError(last_error())

    def counts(self, i):
        out = (ctypes.c_uint32 * 3)()
        if lib().implisolid_batch_counts(self.h, int(i), out) != 0:
            raise ImplisolidError(last_error())
        return int(out[0]), int(out[1]), bool(out[2])

    def download(self, i, normals=False):
        """(verts, faces) of object i's last run; with normals=True (verts, faces, normals)."""
        nv, nf, of = self.counts(i)
        v = np.empty((nv, 3), np.float32)
        f = np.empty((nf, 3), np.int32)
        if lib().implisolid_batch_download(self.h, int(i), v.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                           f.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) != 0:
            raise ImplisolidError(last_error())
        return (v, f, self.normals(i)) if normals else (v, f)

    def normals(self, i, return_problems=False):
        """Object i's per-vertex normals of the last run, float32 [nv, 3], the rows of download(i)'s
        vertices (rows with |g| <= 1e-4 or a non-finite g are -42 g); with return_problems: (normals,
        the number of such rows).  Raises for a batch created without the "normals" key."""
        if not self.has_normals:   # (the library says why; no vertex count is read for nothing)
            lib().implisolid_batch_download_normals(self.h, int(i), None, None)
            raise ImplisolidError(last_error() or "the batch computes no normals")
        nv = self.counts(i)[0]
        out = np.empty((nv, 3), np.float32)
        bad = ctypes.c_int64(0)
        if lib().implisolid_batch_download_normals(self.h, int(i), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                   ctypes.byref(bad)) != 0:
            raise ImplisolidError(last_error())
        return (out, int(bad.value)) if return_problems else out

    def close(self):
        if self.h:
            lib().implisolid_batch_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
