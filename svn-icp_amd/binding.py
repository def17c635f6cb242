"""ctypes binding of libsvnicp_hip.so (C ABI: include/svnicp_hip.h).  No torch types cross it."""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB_PATH = os.path.join(_HERE, "libsvnicp_hip.so")
_HEADER = os.path.join(_ROOT, "include", "svnicp_hip.h")


class SvnIcpError(RuntimeError):
    pass


class Params(C.Structure):
    """struct svnicp_params (include/svnicp_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("mode", C.c_int32), ("iterations", C.c_int32),
                ("knn_count", C.c_int32), ("lr", C.c_double), ("max_dist", C.c_double),
                ("convergence_threshold", C.c_double), ("check_early_stop", C.c_int32),
                ("svn_full_grad", C.c_int32), ("optimizer", C.c_int32), ("record_trace", C.c_int32)]


class SegParamsStruct(C.Structure):
    """struct svnicp_seg_params (include/svnicp_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("n_scan", C.c_int32), ("horizon_scan", C.c_int32), ("ground_scan_ind", C.c_int32),
                ("ang_res_x", C.c_float), ("ang_res_y", C.c_float), ("ang_bottom", C.c_float), ("min_range", C.c_float),
                ("mount_angle", C.c_float), ("segment_theta", C.c_float), ("valid_point_num", C.c_int32),
                ("valid_line_num", C.c_int32)]


class VisibilityOptStruct(C.Structure):
    """struct svnicp_visibility_opt (include/svnicp_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("window_rows", C.c_int32), ("window_cols", C.c_int32), ("margin_abs", C.c_float),
                ("margin_rel", C.c_float), ("max_range", C.c_float)]


class VisibilityStatsStruct(C.Structure):
    """struct svnicp_visibility_stats (include/svnicp_hip.h)."""
    _fields_ = [("pixels_filled", C.c_int64), ("points_tested", C.c_int64), ("points_removed", C.c_int64),
                ("voxels_emptied", C.c_int64)]


class EvalStruct(C.Structure):
    """struct svnicp_eval (include/svnicp_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("has_normals", C.c_int32), ("rows", C.c_int64), ("evaluated", C.c_int64),
                ("inliers", C.c_int64), ("plane_inliers", C.c_int64), ("sum_d2", C.c_double), ("sum_r2", C.c_double),
                ("fitness", C.c_double), ("inlier_rmse", C.c_double), ("plane_rmse", C.c_double), ("R", C.c_double * 9),
                ("t", C.c_double * 3)]


class InformationStruct(C.Structure):
    """struct svnicp_information (include/svnicp_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("form", C.c_int32), ("pairs", C.c_int64), ("rank", C.c_int32), ("reserved", C.c_int32),
                ("huber_delta", C.c_double), ("eig_floor_ratio", C.c_double), ("max_corr_dist", C.c_double), ("sum_w", C.c_double),
                ("sum_wr2", C.c_double), ("sigma2", C.c_double), ("H", C.c_double * 36), ("b", C.c_double * 6),
                ("eigval", C.c_double * 6), ("eigvec", C.c_double * 36), ("eig_t", C.c_double * 3), ("vec_t", C.c_double * 9),
                ("eig_r", C.c_double * 3), ("vec_r", C.c_double * 9), ("step", C.c_double * 6), ("cov", C.c_double * 36),
                ("R", C.c_double * 9), ("t", C.c_double * 3)]


INFO_POINT, INFO_PLANE = 0, 1   # SVNICP_INFO_POINT, SVNICP_INFO_PLANE
INFO_GICP = 3                   # SVNICP_INFO_GICP (2 is not a form)
MODES_MAX = 32                  # SVNICP_MODES_MAX
SCORE_AS_SOLVED, SCORE_POINT, SCORE_PLANE, SCORE_GICP = -1, 0, 1, 2   # SVNICP_SCORE_*


class ScoreObjectiveStruct(C.Structure):
    """struct svnicp_score_objective (include/svnicp_hip.h)."""
    _fields_ = [("struct_size", C.c_size_t), ("form", C.c_int), ("max_corr_dist", C.c_double), ("huber_delta", C.c_double),
                ("epsilon", C.c_double)]


class ModesOptStruct(C.Structure):
    """struct svnicp_modes_opt (include/svnicp_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("max_modes", C.c_int32), ("link_trans", C.c_double), ("link_rot", C.c_double),
                ("particles6xP", C.POINTER(C.c_double)), ("P", C.c_int32), ("reserved", C.c_int32), ("weightsP", C.POINTER(C.c_double))]


class ModesStruct(C.Structure):
    """struct svnicp_modes (include/svnicp_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("particles", C.c_int32), ("nonfinite", C.c_int32), ("n_modes", C.c_int32),
                ("n_reported", C.c_int32), ("has_scores", C.c_int32), ("label", C.c_int32 * MODES_MAX), ("count", C.c_int32 * MODES_MAX),
                ("best", C.c_int32 * MODES_MAX), ("mass", C.c_double * MODES_MAX), ("cost_min", C.c_double * MODES_MAX),
                ("cost_mean", C.c_double * MODES_MAX), ("mean", C.c_double * (6 * MODES_MAX)), ("cov", C.c_double * (36 * MODES_MAX)),
                ("R", C.c_double * (9 * MODES_MAX)), ("t", C.c_double * (3 * MODES_MAX))]


MAP_SEARCH_MAX_LEVELS, MAP_SEARCH_MAX_KEEP = 8, 1024   # SVNICP_MAP_SEARCH_MAX_LEVELS, SVNICP_MAP_SEARCH_MAX_KEEP


class MapSearchOptStruct(C.Structure):
    """struct svnicp_map_search_opt (include/svnicp_hip.h)."""
    _fields_ = [("extent", C.c_double * 6), ("step", C.c_double * 6), ("levels", C.c_int), ("keep", C.c_int),
                ("max_corr_dist", C.c_double)]


class MapSearchStruct(C.Structure):
    """struct svnicp_map_search (include/svnicp_hip.h)."""
    _fields_ = [("levels", C.c_int), ("active_axes", C.c_int), ("nodes_scored", C.c_int64),
                ("level_count", C.c_int64 * MAP_SEARCH_MAX_LEVELS), ("level_kept", C.c_int32 * MAP_SEARCH_MAX_LEVELS),
                ("fine_step", C.c_double * 6), ("best_lattice", C.c_int32 * 6), ("best_correction", C.c_double * 6),
                ("best_pose", C.c_double * 12), ("best_record", C.c_double * 4), ("zero_record", C.c_double * 4)]


def library_path() -> str:
    return _LIB_PATH


def declared_symbols() -> list[str]:
    """Every function name include/svnicp_hip.h declares (used by the symbol-export test)."""
    txt = open(_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(svnicp_[a-z0-9_]+)\s*\(", txt)))


_lib = None


def load_library():
    """dlopen libsvnicp_hip.so; raises SvnIcpError (never falls back) when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise SvnIcpError(f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch wheels bundle their own libamdhip64; if the system HIP runtime gets loaded first (through
    # this library), a later `import torch` binds to it and torch.cuda reports "No HIP GPUs".  Import
    # torch first so that the whole process shares ONE runtime (torch is only plumbing here: device
    # memory, streams, torch.distributed — the library itself has no torch dependency).
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover
        pass
    try:
        L = C.CDLL(_LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise SvnIcpError(f"cannot load {_LIB_PATH}: {e}") from e
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    vp = C.c_void_p
    L.svnicp_abi_version.restype = C.c_int
    L.svnicp_last_error.restype = C.c_char_p
    L.svnicp_last_error.argtypes = [vp]
    L.svnicp_create.argtypes = [C.POINTER(Params), C.c_int, dp, C.c_int, C.POINTER(vp)]
    L.svnicp_destroy.argtypes = [vp]
    L.svnicp_destroy.restype = None
    L.svnicp_set_stream.argtypes = [vp, vp]
    L.svnicp_synchronize.argtypes = [vp]
    L.svnicp_set_clouds.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.c_int]
    L.svnicp_set_particles.argtypes = [vp, dp, C.c_int]
    L.svnicp_set_source.argtypes = [vp, vp, C.c_int64, C.c_int]
    L.svnicp_set_target.argtypes = [vp, vp, C.c_int64, C.c_int]
    L.svnicp_map_create.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int64, C.POINTER(vp)]
    L.svnicp_map_destroy.argtypes = [vp]
    L.svnicp_map_destroy.restype = None
    L.svnicp_map_last_error.argtypes = [vp]
    L.svnicp_map_last_error.restype = C.c_char_p
    L.svnicp_map_clear.argtypes = [vp]
    L.svnicp_map_size.argtypes = [vp, C.POINTER(C.c_int64)]
    L.svnicp_map_add_cloud.argtypes = [vp, vp, C.c_int64, C.c_int, dp, dp]
    L.svnicp_map_query.argtypes = [vp, dp, C.c_double, C.POINTER(C.c_int64)]
    L.svnicp_map_points_devptr.argtypes = [vp]
    L.svnicp_map_points_devptr.restype = vp
    L.svnicp_map_download.argtypes = [vp, dp, C.c_int64, C.POINTER(C.c_int64)]
    L.svnicp_map_query_normals.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    L.svnicp_map_normals_devptr.argtypes = [vp]
    L.svnicp_map_normals_devptr.restype = vp
    L.svnicp_map_download_normals.argtypes = [vp, dp, C.c_int64, C.POINTER(C.c_int64)]
    L.svnicp_map_clear_seen_through.argtypes = [vp, vp, C.c_int64, C.c_int, dp, dp, C.POINTER(SegParamsStruct),
                                                C.POINTER(VisibilityOptStruct), C.POINTER(VisibilityStatsStruct)]
    L.svnicp_map_score_poses.argtypes = [vp, vp, C.c_int64, C.c_int, vp, C.c_int64, C.c_int, C.c_double, dp]
    L.svnicp_map_scores_devptr.argtypes = [vp]
    L.svnicp_map_scores_devptr.restype = vp
    L.svnicp_map_search_poses.argtypes = [vp, vp, C.c_int64, C.c_int, dp, dp, C.POINTER(MapSearchOptStruct), C.POINTER(MapSearchStruct)]
    L.svnicp_map_search_top.argtypes = [vp, C.c_int, ip, dp, dp, dp, C.POINTER(C.c_int)]
    L.svnicp_map_search_level.argtypes = [vp, C.c_int, C.c_int64, ip, dp, dp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int)]
    L.svnicp_prep_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.svnicp_prep_destroy.argtypes = [vp]
    L.svnicp_prep_destroy.restype = None
    L.svnicp_prep_last_error.argtypes = [vp]
    L.svnicp_prep_last_error.restype = C.c_char_p
    L.svnicp_prep_scan.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double, dp, C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.svnicp_map_skipped_points.argtypes = [vp, C.POINTER(C.c_int64)]
    L.svnicp_map_table_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    for name in ("svnicp_prep_cropped_devptr", "svnicp_prep_map_cloud_devptr", "svnicp_prep_source_devptr", "svnicp_prep_source_f32_devptr"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = vp
    L.svnicp_prep_download.argtypes = [vp, C.c_int, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.svnicp_prep_scan_deskew.argtypes = [vp, vp, vp, C.c_int, C.c_int64, C.c_int, dp, C.c_int, C.c_double, C.c_double, C.c_double, dp,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.svnicp_prep_deskewed_devptr.argtypes = [vp]
    L.svnicp_prep_deskewed_devptr.restype = vp
    L.svnicp_prep_download_deskewed.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.svnicp_seg_default_params.argtypes = [C.c_int, C.POINTER(SegParamsStruct)]
    L.svnicp_prep_segment.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(SegParamsStruct), C.POINTER(C.c_int64)]
    for name in ("svnicp_prep_segmented_devptr", "svnicp_prep_segmented_index_devptr"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = vp
    L.svnicp_prep_download_segmented.argtypes = [vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.svnicp_prep_download_seg_images.argtypes = [vp, vp, vp, vp, vp, C.c_int64]
    L.svnicp_set_initial_mean.argtypes = [vp, dp, dp]
    L.svnicp_set_k.argtypes = [vp, C.c_int]
    L.svnicp_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.svnicp_set_max_dist.argtypes = [vp, C.c_double]
    L.svnicp_align.argtypes = [vp]
    L.svnicp_align_async.argtypes = [vp]
    for n in ("transformation", "distribution", "cov_matrix", "particles", "particle_weight", "runtime",
              "candidate_dist2", "gpu_ms"):
        getattr(L, "svnicp_get_" + n).argtypes = [vp, dp]
    L.svnicp_get_particle_history.argtypes = [vp, fp]
    L.svnicp_get_candidates.argtypes = [vp, ip]
    L.svnicp_get_trace.argtypes = [vp, ip, dp, dp, dp, dp, dp]
    L.svnicp_get_knn_fallbacks.argtypes = [vp, C.POINTER(C.c_int)]
    L.svnicp_get_knn_survivors.argtypes = [vp, ip]
    L.svnicp_get_knn_fallback_rows.argtypes = [vp, ip, C.c_int, C.POINTER(C.c_int)]
    L.svnicp_get_ambiguous_steps.argtypes = [vp, C.POINTER(C.c_int)]
    L.svnicp_get_ambiguous_pairs.argtypes = [vp, C.POINTER(C.c_int64)]
    L.svnicp_get_iterations_run.argtypes = [vp, C.POINTER(C.c_int)]
    L.svnicp_set_profile.argtypes = [vp, C.c_int]
    L.svnicp_get_kernel_ms.argtypes = [vp, dp, ip]
    L.svnicp_set_shard.argtypes = [vp, C.c_int, C.c_int]
    L.svnicp_set_row_shard.argtypes = [vp, C.c_int, C.c_int, C.c_int64]
    L.svnicp_rank_sums_devptr.argtypes = [vp]
    L.svnicp_rank_sums_devptr.restype = vp
    L.svnicp_align_begin.argtypes = [vp]
    L.svnicp_stage_candidates.argtypes = [vp, C.c_int64, C.c_int64]
    L.svnicp_build_candidate_table.argtypes = [vp]
    L.svnicp_iter_accumulate.argtypes = [vp, C.c_int]
    L.svnicp_iter_update.argtypes = [vp, C.c_int]
    L.svnicp_finish.argtypes = [vp]
    L.svnicp_stopped.argtypes = [vp]
    L.svnicp_candidates_devptr.argtypes = [vp]
    L.svnicp_candidates_devptr.restype = vp
    L.svnicp_sums_devptr.argtypes = [vp]
    L.svnicp_sums_devptr.restype = vp
    L.svnicp_total_pose_devptr.argtypes = [vp]
    L.svnicp_total_pose_devptr.restype = vp
    for name in ("svnicp_plane_record_devptr", "svnicp_plane_stats_devptr"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = vp
    L.svnicp_get_stage_b_grid.argtypes = [vp, C.POINTER(C.c_int)]
    L.svnicp_set_minibatch.argtypes = [vp, C.c_int, C.c_uint64]
    L.svnicp_set_minibatch_indices.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int]
    L.svnicp_get_minibatch_indices.argtypes = [vp, ip]
    L.svnicp_get_minibatch_candidates.argtypes = [vp, ip]
    L.svnicp_get_minibatch_rows.argtypes = [vp, C.POINTER(C.c_int64)]
    L.svnicp_set_residual.argtypes = [vp, C.c_int, C.c_double, C.c_int]
    L.svnicp_set_pose_prior.argtypes = [vp, dp, dp]
    L.svnicp_get_pose_prior.argtypes = [vp, C.POINTER(C.c_int), dp, dp]
    L.svnicp_particle_pose_devptr.argtypes = [vp, C.c_int]
    L.svnicp_particle_pose_devptr.restype = vp
    L.svnicp_set_target_normals.argtypes = [vp, vp, C.c_int64, C.c_int]
    L.svnicp_get_target_normals.argtypes = [vp, dp]
    L.svnicp_get_plane_stats.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    L.svnicp_set_residual_gicp.argtypes = [vp, C.c_double, C.c_int, C.c_double]
    L.svnicp_set_source_normals.argtypes = [vp, vp, C.c_int64, C.c_int]
    L.svnicp_get_source_normals.argtypes = [vp, dp]
    L.svnicp_get_gicp_stats.argtypes = [vp, dp, C.POINTER(C.c_int64)]
    L.svnicp_evaluate.argtypes = [vp, dp, dp, C.c_double, C.POINTER(EvalStruct)]
    for name in ("svnicp_eval_index_devptr", "svnicp_eval_dist2_devptr"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = vp
    L.svnicp_get_eval_pairs.argtypes = [vp, ip, dp]
    L.svnicp_eval_information.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.POINTER(InformationStruct)]
    L.svnicp_eval_information_gicp.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.POINTER(InformationStruct)]
    L.svnicp_information_solve.argtypes = [C.POINTER(InformationStruct)]
    L.svnicp_score_particles.argtypes = [vp, C.c_double, dp, dp]
    L.svnicp_set_particle_weighting.argtypes = [vp, C.c_int, C.c_double, C.c_double]
    L.svnicp_get_particle_scores.argtypes = [vp, dp, dp]
    L.svnicp_score_particles_objective.argtypes = [vp, C.POINTER(ScoreObjectiveStruct), dp, dp]
    L.svnicp_set_particle_weighting_objective.argtypes = [vp, C.c_int, C.POINTER(ScoreObjectiveStruct), C.c_double]
    L.svnicp_get_score_objective.argtypes = [vp, C.POINTER(ScoreObjectiveStruct)]
    L.svnicp_particle_modes.argtypes = [vp, C.POINTER(ModesOptStruct), C.POINTER(ModesStruct)]
    L.svnicp_get_mode_labels.argtypes = [vp, ip]
    for name in declared_symbols():
        getattr(L, name)  # AttributeError here = the header declares a symbol the library does not export
    _lib = L
    return L


def abi_version() -> int:
    return int(load_library().svnicp_abi_version())
