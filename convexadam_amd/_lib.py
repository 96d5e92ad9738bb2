"""ctypes binding of libconvexadam_hip.so and the one call path into it.

One table per public header: SIGNATURES (include/convexadam_hip.h), PREP_SIGNATURES (convexadam_prep.h), FIELD_SIGNATURES
(convexadam_field.h), AFFINE_SIGNATURES (convexadam_affine.h); lib() types all four when it loads the library.  SOFT_SIGNATURES
(convexadam_soft.h) is typed by soft_lib(), on the first call of convexadam_amd.confidence, as strictly and by name, and SIM_SIGNATURES
(convexadam_sim.h) by sim_lib(), on the first call of convexadam_amd.similarity, and SPLINE_SIGNATURES (convexadam_spline.h) by
spline_lib(), on the first call of convexadam_amd.spline.  Every entry point that takes a stream is entered through call(), every scratch
buffer comes from scratch().

The HIP library IS the product: there is no CPU or PyTorch fallback.  If the shared object is
missing (not built) or an operator is called with tensors that do not live on a HIP device, the call
fails loudly.  PyTorch is used only for device memory, streams and dtype conversion.
"""
import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CONVEXADAM_HIP_LIB") or os.path.join(_HERE, "csrc", "libconvexadam_hip.so")     # (override: race-stress build)

ABI_VERSION = 2          # CVX_ABI_VERSION of include/convexadam_hip.h this binding was written against
CVX_OK, CVX_ERR_INVALID_ARG, CVX_ERR_WORKSPACE, CVX_ERR_LAUNCH, CVX_ERR_UNSUPPORTED = 0, -1, -2, -3, -4
CVX_PREP_CLAMP, CVX_PREP_POSITIVE = 1, 2          # flags of cvx_prep_stats_f32 (include/convexadam_prep.h)


class CvxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libconvexadam_hip error %d: %s" % (code, msg))
        self.code = code


class Smoother(C.Structure):
    """struct cvx_smoother (include/convexadam_hip.h)."""
    _fields_ = [("kind", C.c_int), ("n_boxes", C.c_int), ("box_k", C.c_int * 4), ("gauss_w", C.c_float * 5)]


class CorrOpts(C.Structure):
    """struct cvx_corr_opts (include/convexadam_hip.h)."""
    _fields_ = [("cost", C.c_int), ("n_box", C.c_int), ("fast", C.c_int), ("f16", C.c_int)]


class PairParams(C.Structure):
    """struct cvx_pair_params (include/convexadam_hip.h)."""
    _fields_ = [("H", C.c_int), ("W", C.c_int), ("D", C.c_int), ("mind_r", C.c_int), ("mind_d", C.c_int),
                ("lambda_weight", C.c_float), ("grid_sp", C.c_int), ("disp_hw", C.c_int), ("selected_niter", C.c_int),
                ("selected_smooth", C.c_int), ("grid_sp_adam", C.c_int), ("ic", C.c_int), ("n_feat", C.c_int),
                ("cost_scale", C.c_float), ("cost", C.c_int), ("n_box", C.c_int), ("n_spline_pools", C.c_int), ("corr_fast", C.c_int),
                ("fp16_storage", C.c_int), ("ctx", C.c_void_p), ("adam_fast", C.c_int), ("reserved_", C.c_int * 3)]


class StageParams(C.Structure):
    """struct cvx_convex_stage_params (include/convexadam_hip.h)."""
    _fields_ = [("C", C.c_int), ("h", C.c_int), ("w", C.c_int), ("d", C.c_int), ("disp_hw", C.c_int), ("grid_sp", C.c_int),
                ("ic_iters", C.c_int), ("H", C.c_int), ("W", C.c_int), ("D", C.c_int), ("ctx", C.c_void_p), ("reserved_", C.c_int * 4)]


_vp, _i, _f, _sz, _i64, _ll, _d = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_int64, C.c_longlong, C.c_double

# the arguments every cvx_adam_run_* entry point starts with (F2 .. snapshots); a smoother / mode, then workspace, its size and the stream follow
_ADAM_HEAD = [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _f, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]

# name -> (restype, argtypes); this table is also what tests/test_abi.py checks against the header
SIGNATURES = {
    "cvx_version": (_i, []),
    "cvx_last_error": (C.c_char_p, []),
    "cvx_device_count": (_i, []),
    "cvx_context_create": (_vp, []),
    "cvx_context_destroy": (None, [_vp]),
    "cvx_context_bind": (_vp, [_vp]),
    "cvx_context_set_option": (_i, [_vp, C.c_char_p, C.c_longlong]),
    "cvx_context_get_option": (C.c_longlong, [_vp, C.c_char_p]),
    "cvx_context_set_adam_sqrt_table": (_i, [_vp, _vp, _vp]),
    "cvx_context_set_mind_exp_table": (_i, [_vp, _vp, C.c_uint, C.c_uint, _vp]),
    "cvx_set_adam_sqrt_table": (_i, [_vp]),
    "cvx_set_mind_exp_table": (_i, [_vp, C.c_uint, C.c_uint]),
    "cvx_expf_f32": (_i, [_vp, _vp, _sz, _vp]),
    "cvx_set_option": (_i, [C.c_char_p, C.c_longlong]),
    "cvx_box_tile_sync_errors": (_i, [_i]),
    "cvx_get_option": (C.c_longlong, [C.c_char_p]),
    "cvx_affine_base_host": (None, [_i, _vp]),
    "cvx_disp_mesh_host": (None, [_i, _vp]),
    "cvx_disp_mesh_f32": (_i, [_i, _vp, _vp]),
    "cvx_affine_base_f32": (_i, [_i, _vp, _vp]),
    "cvx_mindssc_workspace_bytes": (_sz, [_i] * 5),
    "cvx_mindssc_f32": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "cvx_mindssc_pooled_scratch_bytes": (_sz, [_i] * 7),
    "cvx_mindssc_pooled_f32": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "cvx_avgpool_f32": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "cvx_round_f16_f32": (_i, [_vp, _i64, _vp]),
    "cvx_pack_field_f64": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "cvx_box_smooth_workspace_bytes": (_sz, [_i] * 5),
    "cvx_box_smooth_f32": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "cvx_box_grow_f32": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "cvx_mask_erode_f32": (_i, [_vp, _i, _i, _i, _f, _vp, _vp]),
    "cvx_gather_f32": (_i, [_vp, _vp, _i64, _vp, _vp]),
    "cvx_select_f32": (_i, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "cvx_label_histogram_i64": (_i, [_vp, _i64, _i, _vp, _vp]),
    "cvx_label_weights_host": (_i, [_vp, _vp, _i, _vp, _vp]),
    "cvx_label_features_f32": (_i, [_vp, _i64, _i, _vp, _vp, _f, _vp, _vp]),
    "cvx_label_features_pooled_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp, _i, _vp, _vp]),
    "cvx_correlate_workspace_bytes": (_sz, [_i] * 5),
    "cvx_correlate_ex_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cvx_correlate_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "cvx_coupled_convex_workspace_bytes": (_sz, [_i] * 4),
    "cvx_coupled_convex_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "cvx_coupled_convex_masked_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "cvx_coupled_convex_f16": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "cvx_inverse_consistency_workspace_bytes": (_sz, [_i] * 3),
    "cvx_inverse_consistency_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cvx_resize_trilinear_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "cvx_grid_sample_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp]),
    "cvx_adam_workspace_bytes": (_sz, [_i] * 4),
    "cvx_adam_run_f32": (_i, _ADAM_HEAD + [_vp, _sz, _vp]),
    "cvx_smooth_workspace_bytes": (_sz, [_i] * 4),
    "cvx_smooth_f32": (_i, [_vp, _i, _i, _i, _i, C.POINTER(Smoother), _i, _vp, _vp, _sz, _vp]),
    "cvx_adam_run_smoother_f32": (_i, _ADAM_HEAD + [C.POINTER(Smoother), _vp, _sz, _vp]),
    "cvx_adam_run_ex_f32": (_i, _ADAM_HEAD + [C.POINTER(Smoother), _i, _vp, _sz, _vp]),
    "cvx_adam_run_fast_f32": (_i, _ADAM_HEAD + [_vp, _sz, _vp]),
    "cvx_adam_run_fast_all_f32": (_i, _ADAM_HEAD + [_vp, _sz, _vp]),
    "cvx_adam_run_mode_f32": (_i, _ADAM_HEAD + [C.POINTER(Smoother), _i, _vp, _sz, _vp]),
    "cvx_const_div_make": (_i, [_f, _i, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "cvx_const_div_enumerate": (_i, [_f, _f]),
    "cvx_const_div_mismatches": (C.c_longlong, [_f, _i, _i, _i, C.POINTER(C.c_uint)]),
    "cvx_smooth_fast_f32": (_i, [_vp, _i, _i, _i, C.POINTER(Smoother), _i, _vp, _vp]),
    "cvx_box3_fast_f32": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "cvx_register_pair_workspace_bytes": (_sz, [C.POINTER(PairParams)]),
    "cvx_register_pair_f32": (_i, [_vp, _vp, _vp, _vp, C.POINTER(PairParams), _vp, _vp, _vp, _sz, _vp]),
    "cvx_register_label_pair_workspace_bytes": (_sz, [C.POINTER(PairParams)]),
    "cvx_register_label_pair_f32": (_i, [_vp, _vp, _vp, _vp, _f, C.POINTER(PairParams), _vp, _vp, _vp, _sz, _vp]),
    "cvx_register_pair_snapshots_workspace_bytes": (_sz, [_vp, _i, _vp, _i]),
    "cvx_register_pair_snapshots_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _sz, _vp]),
    "cvx_register_pairs_f32": (_i, [_i, _vp, _vp, _vp, _vp, C.POINTER(PairParams), _vp, _vp, _vp, _sz, _i, _vp]),
    "cvx_last_pair_profile": (_i, [_vp, _vp, _i]),
    "cvx_set_profiling": (None, [_i]),
    "cvx_jacobian_det_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "cvx_jacobian_stats_f64": (_i, [_vp, _i64, _vp, _vp]),
    "cvx_warp_labels_nearest_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "cvx_label_overlap_i64": (_i, [_vp, _vp, _i64, _i, _vp, _vp]),
    "cvx_map_coordinates_linear_f64": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "cvx_feature_transform_workspace_bytes": (_sz, [_i, _i, _i]),
    "cvx_feature_transform_i32": (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "cvx_feature_flat_index_i64": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "cvx_label_mask_f32": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "cvx_label_mask_scaled_f32": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp]),
    "cvx_edt_sqdist_i32": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "cvx_surface_hist_i64": (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "cvx_hist_order_stats_i64": (_i, [_vp, _i, _i64, _i64, _vp, _vp]),
    "cvx_hist_percentile_neighbours_i64": (_i, [_vp, _i, _f, _vp, _vp]),
    "cvx_surface_hist_batch_i64": (_i, [_vp, _i, _i64, _i, _vp, _vp, _vp]),
    "cvx_hist_percentile_neighbours_batch_i64": (_i, [_vp, _i, _i, _f, _vp, _vp]),
    "cvx_edt_squared_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "cvx_edt_squared_i32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "cvx_edt_squared_labels_i32": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _sz, _vp]),
    "cvx_label_bits_bytes": (_sz, [_i, _i, _i, _i]),
    "cvx_label_bits_u64": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "cvx_surface_distance_hist_i64": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i64, _vp, _i, _i, _vp]),
    "cvx_surface_distance_hist_bits_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "cvx_surface_distance_hist_bits_i64": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i64, _vp, _i, _i, _vp, _sz, _vp]),
    "cvx_tps_fit_workspace_bytes": (_sz, [_i, _i]),
    "cvx_tps_fit_f32": (_i, [_vp, _vp, _i, _i, _f, _vp, _vp, _sz, _vp]),
    "cvx_tps_eval_f32": (_i, [_vp, _i64, _vp, _vp, _i, _i, _vp, _vp]),
    "cvx_tps_dense_f32": (_i, [_i, _i, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "cvx_resize_trilinear_ac_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _vp]),
    "cvx_rigid_lts_workspace_bytes": (_sz, [_i64]),
    "cvx_rigid_lts_f32": (_i, [_vp, _i, _vp, _i, _i64, _i, _vp, _vp, _vp, _sz, _vp]),
    "cvx_affine_warp_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "cvx_threshold_pool_mask_u8": (_i, [_vp, _i, _i, _i, _f, _i, _vp, _vp]),
    "cvx_label_centroids_i64": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "cvx_rigid_samples_workspace_bytes": (_sz, [_i] * 6),
    "cvx_rigid_samples_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cvx_convex_stage_workspace_bytes": (_sz, [C.POINTER(StageParams)]),
    "cvx_convex_stage_f32": (_i, [_vp, _vp, _vp, _vp, C.POINTER(StageParams), _vp, _vp, _vp, _sz, _vp]),
    "cvx_ssim3d_workspace_bytes": (_sz, [_i] * 6),
    "cvx_ssim3d_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cvx_resample_linear_f64": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, C.c_double, _vp]),
    "cvx_field_to_grid_f64": (_i, [_vp, _i, _i64, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "cvx_field_mean_workspace_bytes": (_sz, [_i] * 3),
    "cvx_field_mean_f64": (_i, [_vp, _i, C.c_longlong, C.c_longlong, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cvx_crop_field_half_f32": (_i, [_vp, _i64, _i64, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "cvx_ranksum_critical_u2": (_i, [_i, C.c_double, C.POINTER(C.c_int)]),
    "cvx_ranksum_better_f64": (_i, [_vp, _vp, C.c_double, C.c_double, _i, _i, _i, _i, _vp, _vp, _vp]),
}

# include/convexadam_prep.h (tests/test_abi.py compares each side header with its own table)
PREP_SIGNATURES = {
    "cvx_prep_stats_workspace_bytes": (_sz, [_ll]),
    "cvx_prep_stats_f32": (_i, [_vp, _ll, _i, _f, _f, _i, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    "cvx_prep_normalise_f32": (_i, [_vp, _ll, _vp, C.POINTER(C.c_float), _i, _vp, _vp]),
    "cvx_prep_nonzero_mask_workspace_bytes": (_sz, [_i, _i, _i]),
    "cvx_prep_nonzero_mask_u8": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, C.POINTER(C.c_int), _vp, _sz, _vp]),
    "cvx_prep_mask_bbox_i32": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
}

_FIELD = [_vp, _i, _i64, _i64]          # a field operand: pointer, elements are double, component stride, voxel stride

# include/convexadam_field.h
FIELD_SIGNATURES = {
    "cvx_field_invert_f64": (_i, _FIELD + [_i, _i, _i, _i, _d] + _FIELD + [_vp, _vp, _vp, _vp]),
    "cvx_field_compose_f64": (_i, _FIELD + _FIELD + [_i, _i, _i] + _FIELD + [_vp]),
}

# include/convexadam_affine.h
AFFINE_SIGNATURES = {
    "cvx_affine_lts_workspace_bytes": (_sz, [_i64]),
    "cvx_affine_lts_f32": (_i, [_vp, _i, _vp, _i, _i64, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "cvx_affine_field_f64": (_i, [_vp, _i, _i, _i] + _FIELD + _FIELD + [_vp]),
}

# include/convexadam_soft.h (typed by soft_lib() below, not at load)
SOFT_SIGNATURES = {
    "cvx_soft_stats_workspace_bytes": (_sz, [_i] * 4),
    "cvx_soft_stats_f32": (_i, [_vp, _i, _vp, _f, _f, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
}

# include/convexadam_sim.h (typed by sim_lib() below, not at load)
SIM_SIGNATURES = {
    "cvx_sim_range_f32": (_i, [_vp, _vp] + _FIELD + [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "cvx_joint_hist_f32": (_i, [_vp, _vp] + _FIELD + [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "cvx_joint_hist_lds_bytes": (_i, [_i, _i]),
}

# include/convexadam_spline.h (typed by spline_lib() below, not at load)
SPLINE_SIGNATURES = {
    "cvx_spline_prefilter_f64": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "cvx_map_coordinates_cubic_f64": (_i, [_vp] + _FIELD + [_i, _i, _i, _vp, _vp]),
    "cvx_resample_cubic_f64": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i, _vp, _d, _vp]),
}

_REBUILD = "rebuild with `python -m convexadam_amd.csrc.build`"
_lib = None
_soft_typed = None          # the handle soft_lib() has typed SOFT_SIGNATURES on
_sim_typed = None           # the handle sim_lib() has typed SIM_SIGNATURES on
_spline_typed = None        # the handle spline_lib() has typed SPLINE_SIGNATURES on
_lock = threading.Lock()


def bind(L, table):
    """Types the entry points of a name -> (restype, argtypes) table on the handle L; a handle that lacks one is refused by name (there is
    no fallback)."""
    for name, (res, args) in table.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise RuntimeError("%s lacks the entry point %s: %s" % (LIB_PATH, name, _REBUILD)) from None
        fn.restype = res
        fn.argtypes = args
    return L


def _typed(L):
    """The handle L with the entry points of all four headers typed and its ABI version checked."""
    for table in (SIGNATURES, PREP_SIGNATURES, FIELD_SIGNATURES, AFFINE_SIGNATURES):
        bind(L, table)
    if L.cvx_version() != ABI_VERSION:
        raise RuntimeError("%s reports ABI version %d, this binding needs %d (struct layouts differ): %s"
                           % (LIB_PATH, L.cvx_version(), ABI_VERSION, _REBUILD))
    return L


def lib():
    """Loads the HIP library (raises if it has not been built or lacks a declared entry point -- never falls back)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError("%s not found: build it with `python -m convexadam_amd.csrc.build` "
                                       "(there is no CPU fallback)" % LIB_PATH)
                _lib = _typed(C.CDLL(LIB_PATH))
    return _lib


def soft_lib():
    """lib() with the entry points of include/convexadam_soft.h typed as well: a library that lacks one is refused by name, as at load.
    (Not part of _typed(): tests/test_call_path.py loads stand-in handles that hold the four tables above and nothing else.)"""
    global _soft_typed
    L = lib()
    if _soft_typed is not L:
        _soft_typed = bind(L, SOFT_SIGNATURES)
    return L


def sim_lib():
    """lib() with the entry points of include/convexadam_sim.h typed as well, exactly as soft_lib() does it (and for its reason)."""
    global _sim_typed
    L = lib()
    if _sim_typed is not L:
        _sim_typed = bind(L, SIM_SIGNATURES)
    return L


def spline_lib():
    """lib() with the entry points of include/convexadam_spline.h typed as well, exactly as soft_lib() does it (and for its reason)."""
    global _spline_typed
    L = lib()
    if _spline_typed is not L:
        _spline_typed = bind(L, SPLINE_SIGNATURES)
    return L


def _last_error():
    return lib().cvx_last_error().decode("utf-8", "replace")


def check(rc):
    if rc != CVX_OK:
        raise CvxError(rc, _last_error())


def require_device_tensor(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if t.device.type != "cuda":
        raise RuntimeError("%s lives on %s: the convexadam_amd operators run only on a HIP (ROCm 'cuda') device; "
                           "there is no CPU path" % (name, t.device))
    return t


def _shape(t, name):
    """The shape of a tensor, read from its metadata only (the callers' checks answer before any device is touched)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    return tuple(int(s) for s in t.shape)


def f32c(t):
    """float32, contiguous view/copy of a device tensor."""
    return t.detach().to(torch.float32).contiguous()


def field_operand(t, grid=None, name="field", strict=False, planar=None, f32=False):
    """A displacement field as the kernels read it (a field operand of include/convexadam_field.h) ->
    (contiguous tensor, (H, W, D), component stride, voxel stride, is_f64), strides in elements.

    t       (H, W, D, 3) or (3, H, W, D) tensor; float32 and float64 are read as they are, every other dtype as float64 (f32=True: all as
            float32, cropfield's rule)
    grid    the (H, W, D) the field must live on; None reads it from the shape, where (3, 3, 3, 3) is (H, W, D, 3), what convex_adam_pt
            returns -- or, with strict=True, is refused like every shape that does not say which layout it is
    planar  True / False: the caller knows the layout to be (3, H, W, D) / (H, W, D, 3); None: the shape says, (H, W, D, 3) first"""
    t = t.detach()
    s = tuple(int(n) for n in t.shape)
    if len(s) != 4 and (grid is None or strict):
        raise ValueError("%s must be (H, W, D, 3) or (3, H, W, D), got %s" % (name, s))
    if grid is None:
        if s[0] != 3 and s[-1] != 3 and not strict:
            raise ValueError("%s must be (H, W, D, 3) or (3, H, W, D), got %s" % (name, s))
        if strict and (s[0] == 3) == (s[-1] == 3):
            raise ValueError("a field of shape %s does not say which of its layouts it is: pass field_grid" % (s,))
        grid = s[:3] if s[-1] == 3 else s[1:]
    grid = tuple(int(n) for n in grid)
    if s == grid + (3,) and not planar:
        cs, vs = 1, 3
    elif s == (3,) + grid and planar is not False:
        cs, vs = grid[0] * grid[1] * grid[2], 1
    else:
        raise ValueError("field must be (H, W, D, 3) or (3, H, W, D) on the grid (z, y, x) = %s, got %s" % (grid, s))
    if f32:
        t = t.to(torch.float32)
    elif t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)                                  # integers (and half floats) are computed in float64
    return t.contiguous(), grid, cs, vs, int(t.dtype == torch.float64)


def field_operand_from(f, name, device):
    """field_operand of a device tensor (read in place), or of an (H, W, D, 3) array, image or host tensor uploaded to `device` (None: the
    current one) as float64 -> field_operand's tuple + (came from the host,)"""
    if isinstance(f, torch.Tensor) and f.is_cuda:
        return field_operand(f, name=name) + (False,)
    from .convex_adam_utils import validate_image          # (at call time: convex_adam_utils imports this module)
    t = validate_image(f)
    if t.dim() != 4 or t.shape[-1] != 3:
        raise ValueError("%s must be (H, W, D, 3), got %s" % (name, tuple(t.shape)))
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    return field_operand(t.to(dev, torch.float64), name=name) + (True,)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_tls = threading.local()


def workspace(nbytes, device):
    """Grow-only scratch buffer per (thread, device, stream): the library never allocates.  Per THREAD as well (round 5): two Python
    threads calling the drop-in API on the same stream interleave their launches (ctypes releases the GIL inside the C call); with a
    shared scratch buffer one pair's kernels would run between the other's on the same memory.  Every other piece of a call's data --
    inputs, outputs, optimiser state -- already belongs to the call; the buffers of a thread are freed with the thread."""
    ws = getattr(_tls, "workspaces", None)
    if ws is None:
        ws = _tls.workspaces = {}
    key = (str(device), stream_ptr(device).value or 0)          # (the stream call() hands to the library; the null stream is 0)
    buf = ws.get(key)
    if buf is None or buf.numel() < nbytes:
        ws[key] = buf = torch.empty(int(nbytes * 1.05) + 4096, dtype=torch.uint8, device=device)
    return buf


def release_workspaces():
    """Drops the calling thread's scratch buffers."""
    if getattr(_tls, "workspaces", None):
        _tls.workspaces.clear()


def scratch(dev, query_name, *query_args, required=False, otherwise="", size=None):
    """(pointer, nbytes) of the calling thread's scratch buffer for the current stream of `dev`, sized by the library's query
    `query_name(*query_args)`: the only caller of a *_workspace_bytes / *_scratch_bytes query on the way to a launch and the only caller
    of workspace().  nbytes is the query's value, unchanged; the pointer is never null (a query that answers 0 still gets a buffer), so
    a launcher that refuses a size of 0 refuses it for the size and nothing else.  required=True: 0 means that the library refused the
    query's arguments -> CvxError(CVX_ERR_INVALID_ARG) with cvx_last_error's text, or `otherwise` where that is empty.  The pair goes
    directly in front of the stream in most entry points: call(dev, name, ..., *scratch(dev, query, ...)).  size=f is for the one
    entry point whose workspace the library has no query for (cvx_register_pairs_f32: n_streams slots of the single pair's size): nbytes
    is then f(the query's value), the caller's own arithmetic."""
    nbytes = getattr(lib(), query_name)(*query_args)
    if required and nbytes == 0:
        raise CvxError(CVX_ERR_INVALID_ARG, _last_error() or otherwise)
    if size is not None:
        nbytes = size(nbytes)
    return ptr(workspace(nbytes, dev)), nbytes


def call(dev, name, *args):
    """The one way into an entry point that takes a stream (all of them take it last): runs lib().name(*args, current stream of `dev`)
    with `dev` as the current device and raises CvxError on a status other than CVX_OK.  `dev` is the device the operands live on, never
    simply the current one; where it already is the current one (or names no index) the guard is skipped.  Adds no synchronisation and
    no allocation.  The host-only entry points (*_host, cvx_const_div_*, the option, table and profiling setters, cvx_last_*) take no
    stream and are called on lib() directly."""
    fn = getattr(lib(), name)
    index = torch.device(dev).index
    if index is None or index == torch.cuda.current_device():
        return check(fn(*args, stream_ptr(dev)))
    with torch.cuda.device(index):
        check(fn(*args, stream_ptr(dev)))
