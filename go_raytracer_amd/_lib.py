"""ctypes binding of the C ABI in include/rt_abi.h (librt_amd.so).

The library is built in-tree (go_raytracer_amd/csrc/Makefile, or
``__graft_entry__.build()``).  There is no fallback: if the shared object is
missing, importing the binding raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_AMD_LIB") or os.path.join(_HERE, "librt_amd.so")  # env: dev A/B

RT_OK = 0
RT_ERR_INVALID = -1
RT_ERR_UNSUPPORTED = -2
RT_ERR_DEVICE = -3
RT_ERR_OOM = -4
RT_ERR_IO = -5

RT_TEX_SOLID, RT_TEX_CHECKER, RT_TEX_IMAGE, RT_TEX_NOISE = range(4)
RT_NOISE_PERLIN, RT_NOISE_MARBLE, RT_NOISE_TURBULENT = 1, 2, 3
(RT_MAT_LAMBERTIAN, RT_MAT_METAL, RT_MAT_DIELECTRIC, RT_MAT_DIFFUSE_LIGHT,
 RT_MAT_ISOTROPIC) = range(5)
(RT_NODE_LIST, RT_NODE_BVH, RT_NODE_SPHERE, RT_NODE_QUAD, RT_NODE_TRIANGLE,
 RT_NODE_TRANSLATE, RT_NODE_ROTATE_Y, RT_NODE_MEDIUM) = range(8)
RT_FLAG_PROFILE = 1
RT_FLAG_GATHER_RCCL = 2  # rt_render_multi: one RCCL ncclGather instead of peer copies
RT_FT_SPHERE, RT_FT_TRI, RT_FT_METAL, RT_FT_DIEL = 1, 2, 4, 8
RT_FT_MEDIA, RT_FT_CHECKER, RT_FT_IMAGE, RT_FT_NOISE = 16, 32, 64, 128
RT_FT_BOX = 256
RT_FT_ALL = 511
RT_MODE_AUTO, RT_MODE_WAVEFRONT, RT_MODE_FUSED = 0, 1, 2
RT_ACCUM_FEAT_GUIDES, RT_ACCUM_FEAT_EMIT = 1, 2  # rt_accum_set_features' plane groups
RT_ACCUM_FEAT_MEDIA = 4  # ... and the modifier that makes them first-event sums (with a scatter count)
RT_ACCUM_FEAT_SPEC = 8  # ... and the specular chains' normal, depth and bounces (not with MEDIA)

D3 = C.c_double * 3


class RtCamera(C.Structure):
    _fields_ = [
        ("aspect_ratio", C.c_double), ("width", C.c_int32),
        ("samples_per_pixel", C.c_int32), ("max_depth", C.c_int32),
        ("max_threads", C.c_int32), ("vertical_fov", C.c_double),
        ("defocus_angle", C.c_double), ("focus_distance", C.c_double),
        ("background", D3), ("max_contribution", C.c_double),
        ("look_from", D3), ("look_at", D3), ("vup", D3),
        ("positioned", C.c_int32), ("_pad", C.c_int32),
    ]


class RtCameraDerived(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("spp_sqrt", C.c_int32),
        ("max_depth", C.c_int32), ("pixel_samples_scale", C.c_double),
        ("recip_spp_sqrt", C.c_double), ("center", D3), ("pixel00", D3),
        ("delta_u", D3), ("delta_v", D3), ("defocus_u", D3), ("defocus_v", D3),
        ("defocus_angle", C.c_double), ("max_contribution", C.c_double),
        ("background", D3),
    ]


class RtSceneInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_spheres", "n_quads", "n_triangles", "n_world_prims", "n_media",
        "n_lights", "n_bvh_nodes", "bvh_depth", "max_leaf", "n_materials",
        "n_textures", "n_images", "n_perlins", "medium_draws")] + [
        ("device_bytes", C.c_int64), ("features", C.c_int32), ("bvh_builder", C.c_int32),
        ("tuned", C.c_int32), ("_pad", C.c_int32)]


class RtRenderOpts(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64), ("device", C.c_int32), ("rank", C.c_int32),
        ("nranks", C.c_int32), ("path_slots", C.c_int32), ("chunk", C.c_int32),
        ("flags", C.c_int32), ("mode", C.c_int32), ("stream", C.c_void_p),
        ("trace_pixel", C.c_int64), ("trace_sample", C.c_int32), ("trace_cap", C.c_int32),
        ("trace_out", C.c_void_p), ("progress_slices", C.c_int32), ("_pad3", C.c_int32),
    ]


class RtStats(C.Structure):
    _fields_ = [
        ("samples", C.c_uint64), ("segments", C.c_uint64),
        ("stack_pushes", C.c_uint64), ("extend_rays", C.c_uint64),
        ("shade_rays", C.c_uint64), ("ms_total", C.c_double),
        ("ms_extend", C.c_double), ("ms_shade", C.c_double),
        ("ms_other", C.c_double), ("n_extend_launches", C.c_int32),
        ("n_shade_launches", C.c_int32), ("iterations", C.c_int32),
        ("rows", C.c_int32), ("mode", C.c_int32), ("path_slots", C.c_int32),
        ("ms_fused", C.c_double),
        ("kernel_features", C.c_int32), ("scene_features", C.c_int32),
        ("tree_width", C.c_int32), ("lds_scene", C.c_int32),
        ("chunk_samples", C.c_int32), ("record_boxes", C.c_int32),
        ("overflow_samples", C.c_uint64),
        ("tuned", C.c_int32), ("chunk_records", C.c_int32),
    ]


class RtAov(C.Structure):  # rt_aov: feature buffers (any pointer may be NULL)
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p),
                ("material", C.c_void_p)]


class RtAovEmit(C.Structure):  # rt_aov_emit: the emission split (any pointer may be NULL)
    _fields_ = [("emission", C.c_void_p), ("surface_albedo", C.c_void_p),
                ("coverage", C.c_void_p)]


class RtAovMedia(C.Structure):  # rt_aov_media: the media mode's plane (may be NULL)
    _fields_ = [("scatter", C.c_void_p)]


class RtAovSpecOpts(C.Structure):  # rt_aov_spec_opts: the specular chains' limits (0 = defaults)
    _fields_ = [("max_bounces", C.c_int32), ("max_fuzz", C.c_float)]


class RtAovSpec(C.Structure):  # rt_aov_spec: the specular mode's plane (may be NULL)
    _fields_ = [("bounces", C.c_void_p)]


class RtDenoiseOpts(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("demodulate", C.c_int32),
                ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("_pad", C.c_int32)]


class RtDenoiseVarOpts(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("demodulate", C.c_int32),
                ("sigma_lum", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("_pad", C.c_int32)]


class RtFrame(C.Structure):  # rt_frame: one frame of rt_reproject (var and count may be NULL)
    _fields_ = [("rgb", C.c_void_p), ("var", C.c_void_p), ("count", C.c_void_p),
                ("normal", C.c_void_p), ("depth", C.c_void_p),
                ("count_scalar", C.c_float), ("_pad", C.c_int32)]


class RtReprojectOpts(C.Structure):  # rt_reproject_opts (0 = the library default)
    _fields_ = [("max_history", C.c_float), ("depth_tol", C.c_float),
                ("normal_tol", C.c_float), ("min_weight", C.c_float)]


class RtMomentsOpts(C.Structure):  # rt_moments_opts (0 = the library default; radius -1: no window)
    _fields_ = [("min_frames", C.c_float), ("radius", C.c_int32)]


class RtClipOpts(C.Structure):  # rt_clip_opts (0 = the library default)
    _fields_ = [("gamma", C.c_float)]


class RtSpecPlanes(C.Structure):  # rt_spec_planes: the chain lengths of rt_reproject_spec's two frames
    _fields_ = [("prev_bounces", C.c_void_p), ("cur_bounces", C.c_void_p)]


RT_REPROJECT_PLAIN, RT_REPROJECT_EMIT, RT_REPROJECT_LIGHT = 0, 1, 2
RT_PIPE_FILTER_NONE, RT_PIPE_FILTER_PLAIN, RT_PIPE_FILTER_VAR = 0, 1, 2


class RtPipelineOpts(C.Structure):  # rt_pipeline_opts (zeros in an option struct: the entries' defaults)
    _fields_ = [("temporal", C.c_int32), ("mode", C.c_int32), ("moments", C.c_int32), ("clip", C.c_int32),
                ("specular", C.c_int32), ("reproject", RtReprojectOpts), ("mopts", RtMomentsOpts),
                ("copts", RtClipOpts), ("filter", C.c_int32), ("split_emitters", C.c_int32),
                ("dopts", RtDenoiseOpts), ("vopts", RtDenoiseVarOpts)]


class RtPipelineInfo(C.Structure):  # rt_pipeline_info
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("device", C.c_int32), ("frames", C.c_int32),
                ("had_history", C.c_int32), ("_pad", C.c_int32), ("device_bytes", C.c_uint64),
                ("allocations", C.c_uint64)]


class RtAccumInfo(C.Structure):  # rt_accum_info
    _fields_ = [("passes", C.c_int32), ("max_passes", C.c_int32),
                ("samples_per_pixel", C.c_uint64), ("nonfinite_pixels", C.c_uint64),
                ("rms_std_error", C.c_double), ("mean_luminance", C.c_double),
                ("rel_error", C.c_double)]


class RtAdaptOpts(C.Structure):  # rt_adapt_opts
    _fields_ = [("rel_error", C.c_double), ("lum_floor", C.c_double),
                ("tile", C.c_int32), ("min_passes", C.c_int32)]


class RtAdaptInfo(C.Structure):  # rt_adapt_info
    _fields_ = [("active_pixels", C.c_uint64), ("total_samples", C.c_uint64),
                ("min_count", C.c_int32), ("max_count", C.c_int32),
                ("n_tiles", C.c_int32), ("active_tiles", C.c_int32)]


class RtTreeView(C.Structure):
    _fields_ = [
        ("nodes", C.c_void_p), ("n_nodes", C.c_int32),
        ("children", C.c_void_p), ("n_children", C.c_int32),
        ("tris", C.c_void_p), ("n_tris", C.c_int32),
        ("materials", C.c_void_p), ("n_materials", C.c_int32),
        ("textures", C.c_void_p), ("n_textures", C.c_int32),
        ("images", C.c_void_p), ("n_images", C.c_int32),
        ("perlins", C.c_void_p), ("n_perlins", C.c_int32),
    ]


class RtObjImage(C.Structure):
    _fields_ = [("name", C.c_char_p), ("rgb", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32)]


class RtObjOptions(C.Structure):  # LoadObjOptions objLoader.go:18-29
    _fields_ = [
        ("scale_factor", C.c_double), ("flip_yz", C.c_int32), ("debug", C.c_int32),
        ("ignore_normals", C.c_int32), ("center", C.c_int32), ("flip_faces", C.c_int32),
        ("default_material", C.c_int32), ("position", D3), ("ignore_mtl", C.c_int32),
        ("find_windows", C.c_int32), ("n_images", C.c_int32), ("_pad", C.c_int32),
        ("images", C.POINTER(RtObjImage)),
    ]


class RtObjInfo(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_int64), ("n_normals", C.c_int64), ("n_texcoords", C.c_int64),
        ("n_triangles", C.c_int64), ("n_lights", C.c_int64), ("n_materials", C.c_int32),
        ("default_material", C.c_int32), ("bounds_min", D3), ("bounds_max", D3), ("center", D3),
    ]


_P = C.c_void_p
_I = C.c_int
_DP = C.POINTER(C.c_double)

# name -> (restype, argtypes); every symbol declared in include/rt_abi.h
SIGNATURES = {
    "rt_last_error": (C.c_char_p, []),
    "rt_abi_version": (_I, []),
    "rt_tune_set": (_I, [C.c_char_p, C.c_char_p]),
    "rt_tune_get": (_I, [C.c_char_p, C.c_char_p, C.c_int32]),
    "rt_tune_list": (_I, [C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32)]),
    "rt_brute_shape": (_I, [C.POINTER(C.c_int32)]),
    "rt_tree_create": (_I, [C.POINTER(_P)]),
    "rt_tree_destroy": (_I, [_P]),
    "rt_tree_seed": (_I, [_P, C.c_uint64]),
    "rt_tree_rand": (C.c_double, [_P]),
    "rt_tree_rand_range": (C.c_double, [_P, C.c_double, C.c_double]),
    "rt_tree_randn": (_I, [_P, _I]),
    "rt_tex_solid": (_I, [_P, C.c_double, C.c_double, C.c_double]),
    "rt_tex_checker": (_I, [_P, C.c_double, _I, _I]),
    "rt_tex_image": (_I, [_P, C.c_void_p, _I, _I]),
    "rt_tex_noise": (_I, [_P, C.c_double, _I]),
    "rt_tex_noise_tables": (_I, [_P, C.c_double, _I, _DP, C.POINTER(C.c_int32)]),
    "rt_mat_lambertian": (_I, [_P, _I]),
    "rt_mat_metal": (_I, [_P, C.c_double, C.c_double, C.c_double, C.c_double]),
    "rt_mat_dielectric": (_I, [_P, C.c_double]),
    "rt_mat_diffuse_light": (_I, [_P, _I]),
    "rt_mat_isotropic": (_I, [_P, _I]),
    "rt_new_list": (_I, [_P]),
    "rt_list_add": (_I, [_P, _I, _I]),
    "rt_build_bvh": (_I, [_P, _I]),
    "rt_new_sphere": (_I, [_P, D3, C.c_double, _I]),
    "rt_new_motion_sphere": (_I, [_P, D3, D3, C.c_double, _I]),
    "rt_new_quad": (_I, [_P, D3, D3, D3, _I]),
    "rt_new_box": (_I, [_P, D3, D3, _I]),
    "rt_new_triangle": (_I, [_P, _DP, _DP, _DP, _I]),
    "rt_new_triangles": (_I, [_P, _I, _DP, _DP, _DP, C.POINTER(C.c_int32)]),
    "rt_translate": (_I, [_P, _I, D3]),
    "rt_rotate_y": (_I, [_P, _I, C.c_double]),
    "rt_constant_medium": (_I, [_P, _I, C.c_double, _I]),
    "rt_obj_default_options": (_I, [C.POINTER(RtObjOptions)]),
    "rt_load_obj": (_I, [_P, C.c_char_p, C.POINTER(RtObjOptions), C.POINTER(_I), C.POINTER(_I),
                         C.POINTER(RtObjInfo)]),
    "rt_load_obj_memory": (_I, [_P, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p,
                                C.POINTER(RtObjOptions), C.POINTER(_I), C.POINTER(_I),
                                C.POINTER(RtObjInfo)]),
    "rt_tree_get_view": (_I, [_P, C.POINTER(RtTreeView)]),
    "rt_camera_derive": (_I, [C.POINTER(RtCamera), C.POINTER(RtCameraDerived)]),
    "rt_scene_create": (_I, [_P, _I, _I, C.POINTER(_P)]),
    "rt_scene_destroy": (_I, [_P]),
    "rt_scene_info_get": (_I, [_P, C.POINTER(RtSceneInfo)]),
    "rt_scene_export_bvh": (_I, [_P, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p,
                                 C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]),
    "rt_scene_export_bvh8": (_I, [_P, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p,
                                  C.POINTER(C.c_int32)]),
    "rt_scene_export_qbvh": (_I, [_P, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p,
                                  C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]),
    "rt_scene_export_records": (_I, [_P, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rt_scene_export_prim_bounds": (_I, [_P, C.c_void_p, C.POINTER(C.c_int32)]),
    "rt_bvh_build_boxes": (_I, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32),
                                C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rt_scene_lean_light": (_I, [_P, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int32)]),
    "rt_scene_plan_light": (_I, [_P, _I, C.POINTER(C.c_int32)]),
    "rt_scene_lean_emitter": (_I, [_P, C.POINTER(C.c_int32)]),
    "rt_scene_plan_early": (_I, [_P, _I, C.POINTER(C.c_int32)]),
    "rt_scene_plan_cost": (_I, [_P, _I, C.POINTER(C.c_int32)]),
    "rt_render": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_void_p,
                       C.POINTER(RtStats)]),
    "rt_render_device": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_void_p,
                              C.POINTER(RtStats)]),
    "rt_render_multi": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts),
                             C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(RtStats)]),
    "rt_render_multi_device": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts),
                                    C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                    C.POINTER(RtStats)]),
    "rt_quantize": (_I, [C.c_void_p, C.c_int64, C.c_void_p]),
    "rt_format_ppm": (C.c_int64, [C.c_void_p, _I, _I, C.c_void_p, C.c_int64]),
    "rt_progress": (_I, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "rt_quantize_device": (_I, [C.c_void_p, C.c_int64, C.c_void_p, _I, C.c_void_p]),
    "rt_format_ppm_device": (C.c_int64, [C.c_void_p, _I, _I, C.c_void_p, C.c_int64, _I,
                                         C.c_void_p]),
    "rt_render_aov": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_int32,
                           C.POINTER(RtAov), C.POINTER(RtStats)]),
    "rt_render_aov_device": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_int32,
                                  C.POINTER(RtAov), C.POINTER(RtStats)]),
    "rt_denoise": (_I, [C.c_void_p, C.POINTER(RtAov), _I, _I, C.POINTER(RtDenoiseOpts),
                        C.c_void_p]),
    "rt_denoise_device": (_I, [C.c_void_p, C.POINTER(RtAov), _I, _I, C.POINTER(RtDenoiseOpts),
                               C.c_void_p, _I, C.c_void_p]),
    "rt_denoise_var": (_I, [C.c_void_p, C.c_void_p, C.POINTER(RtAov), _I, _I,
                            C.POINTER(RtDenoiseVarOpts), C.c_void_p, C.c_void_p]),
    "rt_denoise_var_device": (_I, [C.c_void_p, C.c_void_p, C.POINTER(RtAov), _I, _I,
                                   C.POINTER(RtDenoiseVarOpts), C.c_void_p, C.c_void_p, _I,
                                   C.c_void_p]),
    "rt_render_aov_emit": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_int32,
                                C.POINTER(RtAov), C.POINTER(RtAovEmit), C.POINTER(RtStats)]),
    "rt_render_aov_emit_device": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_int32,
                                       C.POINTER(RtAov), C.POINTER(RtAovEmit),
                                       C.POINTER(RtStats)]),
    "rt_render_aov_media": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_int32,
                                 C.POINTER(RtAov), C.POINTER(RtAovEmit), C.POINTER(RtAovMedia),
                                 C.POINTER(RtStats)]),
    "rt_render_aov_media_device": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_int32,
                                        C.POINTER(RtAov), C.POINTER(RtAovEmit), C.POINTER(RtAovMedia),
                                        C.POINTER(RtStats)]),
    "rt_render_aov_spec": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_int32,
                                C.POINTER(RtAovSpecOpts), C.POINTER(RtAov), C.POINTER(RtAovSpec),
                                C.POINTER(RtStats)]),
    "rt_render_aov_spec_device": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_int32,
                                       C.POINTER(RtAovSpecOpts), C.POINTER(RtAov), C.POINTER(RtAovSpec),
                                       C.POINTER(RtStats)]),
    "rt_denoise_emit": (_I, [C.c_void_p, C.POINTER(RtAov), C.POINTER(RtAovEmit), _I, _I,
                             C.POINTER(RtDenoiseOpts), C.c_void_p]),
    "rt_denoise_emit_device": (_I, [C.c_void_p, C.POINTER(RtAov), C.POINTER(RtAovEmit), _I, _I,
                                    C.POINTER(RtDenoiseOpts), C.c_void_p, _I, C.c_void_p]),
    "rt_denoise_var_emit": (_I, [C.c_void_p, C.c_void_p, C.POINTER(RtAov), C.POINTER(RtAovEmit),
                                 _I, _I, C.POINTER(RtDenoiseVarOpts), C.c_void_p, C.c_void_p]),
    "rt_denoise_var_emit_device": (_I, [C.c_void_p, C.c_void_p, C.POINTER(RtAov),
                                        C.POINTER(RtAovEmit), _I, _I,
                                        C.POINTER(RtDenoiseVarOpts), C.c_void_p, C.c_void_p, _I,
                                        C.c_void_p]),
    "rt_accum_create": (_I, [_P, C.POINTER(RtCamera), C.POINTER(RtRenderOpts), C.c_int32,
                             C.POINTER(_P)]),
    "rt_accum_destroy": (_I, [_P]),
    "rt_accum_reset": (_I, [_P]),
    "rt_accum_add": (_I, [_P, C.c_uint64, C.POINTER(RtStats)]),
    "rt_accum_resolve": (_I, [_P, C.c_void_p, C.c_void_p]),
    "rt_accum_resolve_device": (_I, [_P, C.c_void_p, C.c_void_p]),
    "rt_accum_info_get": (_I, [_P, C.POINTER(RtAccumInfo)]),
    "rt_accum_select": (_I, [_P, C.POINTER(RtAdaptOpts), C.POINTER(C.c_uint64)]),
    "rt_accum_set_active": (_I, [_P, C.c_void_p, C.POINTER(C.c_uint64)]),
    "rt_accum_add_active": (_I, [_P, C.c_uint64, C.POINTER(RtStats)]),
    "rt_accum_counts": (_I, [_P, C.c_void_p]),
    "rt_accum_counts_device": (_I, [_P, C.c_void_p]),
    "rt_accum_tile_error": (_I, [_P, C.POINTER(RtAdaptOpts), C.c_void_p, C.POINTER(C.c_int32),
                                C.POINTER(C.c_int32)]),
    "rt_accum_adapt_info": (_I, [_P, C.POINTER(RtAdaptInfo)]),
    "rt_accum_set_features": (_I, [_P, C.c_uint32]),
    "rt_accum_get_features": (_I, [_P, C.POINTER(C.c_uint32)]),
    "rt_accum_resolve_aov": (_I, [_P, C.POINTER(RtAov), C.POINTER(RtAovEmit)]),
    "rt_accum_resolve_aov_device": (_I, [_P, C.POINTER(RtAov), C.POINTER(RtAovEmit)]),
    "rt_accum_resolve_aov_media": (_I, [_P, C.POINTER(RtAov), C.POINTER(RtAovEmit), C.POINTER(RtAovMedia)]),
    "rt_accum_resolve_aov_media_device": (_I, [_P, C.POINTER(RtAov), C.POINTER(RtAovEmit),
                                               C.POINTER(RtAovMedia)]),
    "rt_reproject": (_I, [C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtCamera),
                          C.POINTER(RtFrame), _I, _I, C.POINTER(RtReprojectOpts),
                          C.POINTER(RtFrame)]),
    "rt_reproject_device": (_I, [C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtCamera),
                                 C.POINTER(RtFrame), _I, _I, C.POINTER(RtReprojectOpts),
                                 C.POINTER(RtFrame), _I, C.c_void_p]),
    "rt_reproject_emit": (_I, [C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                               C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit), _I, _I,
                               C.POINTER(RtReprojectOpts), C.POINTER(RtFrame)]),
    "rt_reproject_emit_device": (_I, [C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                      C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                      _I, _I, C.POINTER(RtReprojectOpts), C.POINTER(RtFrame), _I,
                                      C.c_void_p]),
    "rt_reproject_light": (_I, [C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit), _I, _I,
                                C.POINTER(RtReprojectOpts), C.POINTER(RtFrame), C.POINTER(RtAovEmit)]),
    "rt_reproject_light_device": (_I, [C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                       C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                       _I, _I, C.POINTER(RtReprojectOpts), C.POINTER(RtFrame),
                                       C.POINTER(RtAovEmit), _I, C.c_void_p]),
    "rt_reproject_moments": (_I, [_I, C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                  C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtFrame),
                                  C.POINTER(RtAovEmit), _I, _I, C.POINTER(RtReprojectOpts),
                                  C.POINTER(RtMomentsOpts), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                  C.c_void_p]),
    "rt_reproject_moments_device": (_I, [_I, C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                         C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtFrame),
                                         C.POINTER(RtAovEmit), _I, _I, C.POINTER(RtReprojectOpts),
                                         C.POINTER(RtMomentsOpts), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                         C.c_void_p, _I, C.c_void_p]),
    "rt_reproject_clip": (_I, [_I, C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                               C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtFrame),
                               C.POINTER(RtAovEmit), _I, _I, C.POINTER(RtReprojectOpts),
                               C.POINTER(RtMomentsOpts), C.POINTER(RtClipOpts), C.POINTER(RtFrame),
                               C.POINTER(RtAovEmit), C.c_void_p]),
    "rt_reproject_clip_device": (_I, [_I, C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                      C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtFrame),
                                      C.POINTER(RtAovEmit), _I, _I, C.POINTER(RtReprojectOpts),
                                      C.POINTER(RtMomentsOpts), C.POINTER(RtClipOpts), C.POINTER(RtFrame),
                                      C.POINTER(RtAovEmit), C.c_void_p, _I, C.c_void_p]),
    "rt_reproject_spec": (_I, [_I, C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                               C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtFrame),
                               C.POINTER(RtAovEmit), _I, _I, C.POINTER(RtReprojectOpts),
                               C.POINTER(RtMomentsOpts), C.POINTER(RtClipOpts), C.POINTER(RtSpecPlanes),
                               C.POINTER(RtFrame), C.POINTER(RtAovEmit), C.c_void_p]),
    "rt_reproject_spec_device": (_I, [_I, C.POINTER(RtCamera), C.POINTER(RtFrame), C.POINTER(RtAovEmit),
                                      C.c_void_p, C.POINTER(RtCamera), C.POINTER(RtFrame),
                                      C.POINTER(RtAovEmit), _I, _I, C.POINTER(RtReprojectOpts),
                                      C.POINTER(RtMomentsOpts), C.POINTER(RtClipOpts), C.POINTER(RtSpecPlanes),
                                      C.POINTER(RtFrame), C.POINTER(RtAovEmit), C.c_void_p, _I, C.c_void_p]),
    "rt_accum_set_features_spec": (_I, [_P, C.c_uint32, C.POINTER(RtAovSpecOpts)]),
    "rt_accum_resolve_aov_spec": (_I, [_P, C.POINTER(RtAov), C.POINTER(RtAovSpec)]),
    "rt_accum_resolve_aov_spec_device": (_I, [_P, C.POINTER(RtAov), C.POINTER(RtAovSpec)]),
    "rt_pipeline_create": (_I, [C.POINTER(RtPipelineOpts), C.POINTER(_P)]),
    "rt_pipeline_destroy": (_I, [_P]),
    "rt_pipeline_reset": (_I, [_P]),
    "rt_pipeline_push": (_I, [_P, _P]),
    "rt_pipeline_image": (_I, [_P, C.c_void_p]),
    "rt_pipeline_ppm": (C.c_int64, [_P, C.c_void_p, C.c_int64]),
    "rt_pipeline_planes_device": (_I, [_P, C.POINTER(RtFrame), C.POINTER(RtAovEmit), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_void_p)]),
    "rt_pipeline_info_get": (_I, [_P, C.POINTER(RtPipelineInfo)]),
    "rt_accum_add_shares": (_I, [C.POINTER(_P), C.c_int32, C.c_uint64, C.POINTER(RtStats)]),
    "rt_pipeline_push_shares": (_I, [_P, C.POINTER(_P), C.c_int32]),
    "rt_demo_scene": (_I, [_P, C.c_char_p, C.c_char_p, C.POINTER(RtCamera), C.POINTER(_I),
                           C.POINTER(_I)]),
    "rt_demo_scene_name": (_I, [_I, C.POINTER(C.c_char_p)]),
    "rt_substitute_mesh_obj": (C.c_int64, [_I, _I, C.c_void_p, C.c_int64]),
    "rt_device_count": (_I, []),
}

_lib = None


def lib():
    """Load librt_amd.so (raises OSError if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} not built: run `make -C go_raytracer_amd/csrc` "
                          "or __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("RT_AMD_LIB") and not hasattr(L, name):
                continue  # dev A/B against an older build that predates the symbol
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rt error {code}: {msg}")
        self.code = code


def check(rc):
    """Raise RtError for a negative status, else return rc (a handle or RT_OK)."""
    if rc < 0:
        raise RtError(rc, lib().rt_last_error().decode(errors="replace"))
    return rc
