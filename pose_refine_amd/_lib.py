"""ctypes binding of the C ABI (include/pose_refine.h) -> pose_refine_amd/lib/libpose_refine_hip.so.

The shared library is built in-tree by ``pose_refine_amd.build`` (hipcc --offload-arch=gfx950).
There is no fallback of any kind: a missing library raises ImportError-like RuntimeError, a missing
GPU makes every device entry point fail with PR_ERR_NO_DEVICE (raised as PoseRefineError).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (PR_LIB_PATH: same-box A/B runs of kernel variants, tools/ab_libs.sh -- the product is the in-tree library)
LIB_PATH = os.environ.get("PR_LIB_PATH") or os.path.join(_HERE, "lib", "libpose_refine_hip.so")

PR_OK = 0
PR_ERR_NO_DEVICE, PR_ERR_HIP, PR_ERR_INVALID, PR_ERR_IO, PR_ERR_NOMEM, PR_ERR_COMM = -1, -2, -3, -4, -5, -6
SCENE_PROJ, SCENE_NN, SCENE_PROJ_CROP, SCENE_GRID = 0, 1, 2, 3
GRID_NONE, GRID_MAX_CELLS = 0xFFFFFFFF, 1 << 26          # PR_GRID_NONE, PR_GRID_MAX_CELLS
COMM_ID_BYTES = 128
SOLVE_HOST, SOLVE_DEVICE = 0, 1

KDNODE = np.dtype([("parent", "<i4"), ("child1", "<i4"), ("child2", "<i4"), ("split_v", "<f4"),
                   ("bbox", "<f4", (6,)), ("split_dim", "<i4"), ("left", "<i4"), ("right", "<i4")])
RESULT = np.dtype([("T", "<f4", (16,)), ("inlier_rmse", "<f4"), ("fitness", "<f4")])
# pr_pose_score: render-and-compare counts of one hypothesis (pr_score_poses)
SCORE = np.dtype([("visible", "<u4"), ("inlier", "<u4"), ("occluded", "<u4"), ("violation", "<u4"), ("missing", "<u4"),
                  ("reserved", "<u4"), ("abs_err_sum", "<u8")])
# pr_pose_contour: depth-edge agreement of one hypothesis with the scene (pr_score_contours)
CONTOUR = np.dtype([("contour", "<u4"), ("hit", "<u4"), ("occluded", "<u4"), ("miss", "<u4"), ("reserved", "<u4", (2,)), ("dist_sum", "<u8")])
CONTOUR_MAX_RADIUS = 32                  # PR_CONTOUR_MAX_RADIUS
# pr_contour_fit: the silhouette of one hypothesis against the scene's nearest-edge map (pr_contour_information)
CONTOUR_FIT = np.dtype([("contour", "<u4"), ("used", "<u4"), ("occluded", "<u4"), ("miss", "<u4"), ("reserved", "<u4", (2,)), ("sum_d2", "<u8")])
EDGE_NONE = 0xFFFFFFFF                   # PR_EDGE_NONE
# pr_pose_normal: surface-normal agreement of one hypothesis with the scene on its inlier pixels (pr_score_normals)
NORMAL = np.dtype([("tested", "<u4"), ("agree", "<u4"), ("disagree", "<u4"), ("no_render_normal", "<u4"), ("no_scene_normal", "<u4"), ("reserved", "<u4", (3,))])
NORMAL_MAX_STEP = 8                      # PR_NORMAL_MAX_STEP
# pr_pose_visible / pr_frame_explained: what a hypothesis keeps once the batch is composed, and what the set explains (pr_compose_detections)
VISIBLE = np.dtype([("owned", "<u4"), ("owned_inlier", "<u4"), ("owned_occluded", "<u4"), ("owned_violation", "<u4"), ("owned_missing", "<u4"),
                    ("reserved", "<u4", (3,))])
FRAME = np.dtype([("window", "<u4"), ("measured", "<u4"), ("covered", "<u4"), ("explained", "<u4"), ("in_front", "<u4"), ("behind", "<u4"),
                  ("unmeasured", "<u4"), ("reserved", "<u4")])
COMPOSE_NONE, COMPOSE_MAX_POSES = 0xFFFF, 65535      # PR_COMPOSE_NONE, PR_COMPOSE_MAX_POSES
# pr_pose_cover / pr_cover_frame: what a hypothesis adds to the pixels the better ones claim, and what the detections claim together (pr_score_cover)
COVER = np.dtype([("support", "<u4"), ("fresh", "<u4"), ("state", "<u4"), ("position", "<u4")])
COVER_FRAME = np.dtype([("claimed", "<u4"), ("n_selected", "<u4"), ("reserved", "<u4", (2,))])
COVER_NOT_IN_ORDER, COVER_EMPTY, COVER_ACCEPTED, COVER_REJECTED, COVER_STATE_MASK = 0, 1, 2, 3, 0xFF      # PR_COVER_*
COVER_REASON_THRESHOLD, COVER_REASON_CAP, COVER_NO_POSITION = 0x100, 0x200, 0xFFFFFFFF
# pr_pose_dist: the displacement of the model's points between two poses, minimised over the symmetry candidates (pr_pose_distance)
POSE_DIST = np.dtype([("disp_sum_q16", "<u8"), ("max_disp_sq", "<f4"), ("max_proj_sq", "<f4"), ("sym_sum", "<u2"), ("sym_disp", "<u2"),
                      ("sym_proj", "<u2"), ("reserved", "<u2"), ("n_points", "<u4"), ("reserved2", "<u4")])
POSE_DIST_MAX_SYMS, POSE_DIST_MAX_POSES, POSE_DIST_MAX_POINTS = 64, 4096, 1 << 24     # PR_POSE_DIST_MAX_SYMS, _MAX_POSES, _MAX_POINTS
# pr_vsd_counts: the visible surfaces of an estimate and a truth against the scene frame, counted (pr_pose_vsd)
VSD_MAX_TAUS = 12                        # PR_VSD_MAX_TAUS
VSD = np.dtype([("visib_gt", "<u4"), ("visib_est", "<u4"), ("inter", "<u4"), ("uni", "<u4"), ("far", "<u4", (VSD_MAX_TAUS,))])
# pr_pair_solid: the shared pixels and the shared depth intervals of two hypotheses (pr_pose_penetration)
PENETRATION_MAX_POSES = 1024             # PR_PENETRATION_MAX_POSES
PAIR_SOLID = np.dtype([("both", "<u4"), ("inter", "<u4"), ("max_mm", "<u4"), ("reserved", "<u4"), ("sum_mm", "<u8")])
assert PAIR_SOLID.itemsize == 24
# pr_pose_info / pr_pose_eig: the float64 information matrix of a hypothesis about a centre, and its Jacobi eigen-decomposition (pr_icp_information)
POSE_INFO = np.dtype([("n_points", "<u4"), ("n_valid", "<u4"), ("n_zero_weight", "<u4"), ("reserved", "<u4"), ("c", "<f4", (3,)), ("rho", "<f4"),
                      ("H", "<f8", (21,)), ("g", "<f8", (6,)), ("sum_w", "<f8"), ("sum_wr2", "<f8"), ("sum_r2", "<f8")])
POSE_EIG = np.dtype([("lambda", "<f8", (6,)), ("V", "<f8", (6, 6)), ("sweeps", "<u4"), ("reserved", "<u4")])
INFO_MAX_SWEEPS = 16                     # PR_INFO_MAX_SWEEPS
assert POSE_INFO.itemsize == 272 and POSE_EIG.itemsize == 344
# pr_ppf_entry / pr_ppf_peak: an ordered model pair in its bucket, a peak of a scene reference's accumulator (pr_ppf_model_build_dev, pr_ppf_vote)
PPF_ENTRY = np.dtype([("pair", "<u4"), ("cos_m", "<f4"), ("sin_m", "<f4")])
PPF_PEAK = np.dtype([("votes", "<u4"), ("model_ref", "<u2"), ("alpha_bin", "<u2"), ("scene_ref", "<u4"), ("n_pairs", "<u4")])
PPF_MAX_DIST_BINS, PPF_MAX_ANGLE_BINS, PPF_MAX_ALPHA_BINS, PPF_MAX_KEYS = 64, 32, 64, 1 << 21        # PR_PPF_MAX_*
PPF_MAX_MODEL_POINTS, PPF_MAX_SCENE_POINTS, PPF_MAX_CELLS, PPF_MAX_PEAKS, PPF_MAX_STRIDE = 2048, 16384, 32768, 4, 256
assert PPF_ENTRY.itemsize == 12 and PPF_PEAK.itemsize == 16
POSE_DIST_CHUNK = 256                    # PR_POSE_DIST_CHUNK (pr_tuning.h; the library reports its own as option "pose_dist_chunk")
assert KDNODE.itemsize == 52 and RESULT.itemsize == 72 and SCORE.itemsize == 32 and CONTOUR.itemsize == 32
assert COVER.itemsize == 16 and COVER_FRAME.itemsize == 16 and CONTOUR_FIT.itemsize == 32
assert NORMAL.itemsize == 32 and VISIBLE.itemsize == 32 and FRAME.itemsize == 32 and POSE_DIST.itemsize == 32 and VSD.itemsize == 64


class PoseRefineError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"pose_refine error {code}: {msg}")
        self.code = code


class Roi(C.Structure):
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("width", C.c_int), ("height", C.c_int)]


class Criteria(C.Structure):
    _fields_ = [("relative_fitness", C.c_float), ("relative_rmse", C.c_float), ("max_iteration", C.c_int)]


class PyramidLevel(C.Structure):
    """pr_pyramid_level: one level of a coarse-to-fine schedule (pr_refine_pyramid): the cloud stride and the ICP criteria run on it."""
    _fields_ = [("stride", C.c_uint32), ("crit", Criteria)]


PYRAMID_MAX_LEVELS, PYRAMID_MAX_STRIDE = 4, 16          # PR_PYRAMID_MAX_LEVELS, PR_PYRAMID_MAX_STRIDE
ROBUST_NONE, ROBUST_HUBER, ROBUST_TUKEY, ROBUST_CAUCHY = 0, 1, 2, 3      # PR_ROBUST_*


class RobustDesc(C.Structure):
    """pr_robust: an M-estimator weight on the ICP residual (pr_robust_describe fills it: inv_c is computed there, once)."""
    _fields_ = [("kind", C.c_uint32), ("c", C.c_float), ("inv_c", C.c_float), ("reserved", C.c_uint32)]


class PPFParams(C.Structure):
    """pr_ppf_params: the point-pair-feature descriptor (pr_ppf_describe fills it: the bin edges and centres are computed there, once)."""
    _fields_ = [("diameter", C.c_float), ("dist_step", C.c_float), ("inv_dist_step", C.c_float), ("n_dist", C.c_uint32), ("n_angle", C.c_uint32),
                ("n_alpha", C.c_uint32), ("n_keys", C.c_uint32), ("flip_model_normals", C.c_uint32), ("cos_edge", C.c_float * 33),
                ("alpha_edge", C.c_float * 33), ("alpha_cos", C.c_double * 64), ("alpha_sin", C.c_double * 64)]


assert C.sizeof(PPFParams) == 1320
PPF_MAX_MODELS = 32                      # PR_PPF_MAX_MODELS


class PPFModelDesc(C.Structure):
    """pr_ppf_model: one model of pr_ppf_vote_multi's table (the descriptor and the sample on the host, the pair table on the device)."""
    _fields_ = [("params", C.c_void_p), ("offsets_dev", C.c_void_p), ("entries_dev", C.c_void_p), ("points_host", C.c_void_p), ("normals_host", C.c_void_p),
                ("n_model", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(PPFModelDesc) == 48


# pr_plane: one dominant plane of a frame (pr_scene_planes_dev / _host); pr_plane_params: what pr_plane_describe fills
PLANE = np.dtype([("normal", "<f4", (3,)), ("offset_mm", "<f4"), ("candidate", "<u4"), ("support", "<u4"), ("labelled", "<u4"), ("behind", "<u4"),
                  ("rms_mm", "<f4"), ("reserved", "<u4", (3,))])
PLANE_MAX_SAMPLES, PLANE_MAX_CANDIDATES, PLANE_MAX_PLANES, PLANE_BEHIND, PLANE_NO_DEPTH = 65536, 4096, 4, 254, 255        # PR_PLANE_*
assert PLANE.itemsize == 48


class PlaneParamsDesc(C.Structure):
    """pr_plane_params: the sample, the support and label tests and the number of planes of a peel (pr_plane_describe checks and fills it)."""
    _fields_ = [("stride", C.c_uint32), ("cand_stride", C.c_uint32), ("tau_mm", C.c_float), ("label_tau_mm", C.c_float), ("cos_min", C.c_float),
                ("min_support", C.c_uint32), ("n_planes", C.c_uint32), ("drop_behind", C.c_uint32)]


assert C.sizeof(PlaneParamsDesc) == 32


# pr_segment: one depth-connected component of a frame (pr_scene_segments_dev / _host); pr_segment_params: what pr_segment_describe fills
SEGMENT = np.dtype([("root", "<u4"), ("pixels", "<u4"), ("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2"), ("depth_min", "<u4"), ("depth_max", "<u4"),
                    ("sum_x", "<u8"), ("sum_y", "<u8"), ("sum_depth", "<u8"), ("reserved", "<u8", (2,))])
SEGMENT_MAX, SEGMENT_MAX_ROOTS, SEGMENT_DROPPED = 4096, 65536, 65535        # PR_SEGMENT_*
assert SEGMENT.itemsize == 64


class SegmentParamsDesc(C.Structure):
    """pr_segment_params: the link threshold, the smallest component kept and the number of segments of a call (pr_segment_describe checks and fills it)."""
    _fields_ = [("jump_mm", C.c_uint32), ("min_pixels", C.c_uint32), ("max_segments", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(SegmentParamsDesc) == 16


# pr_depth_filter_params: what pr_depth_filter_describe fills; pr_depth_filter_counts: the pixels per flag code of a pr_depth_filter_dev / _host call
DEPTH_FUSE_MAX, DEPTH_FILTER_MAX_RADIUS = 8, 2                              # PR_DEPTH_FUSE_MAX, PR_DEPTH_FILTER_MAX_RADIUS
DEPTH_UNMEASURED, DEPTH_KEPT, DEPTH_SMOOTHED, DEPTH_GATED, DEPTH_FLYING, DEPTH_FILLED = range(6)      # PR_DEPTH_*: a pixel's flag


class DepthFilterParamsDesc(C.Structure):
    """pr_depth_filter_params: the range gate, the tolerance, the support a pixel needs, the window and the fill threshold (pr_depth_filter_describe checks and fills it)."""
    _fields_ = [("min_mm", C.c_uint32), ("max_mm", C.c_uint32), ("tol_mm", C.c_uint32), ("tol_permille", C.c_uint32), ("fly_min_support", C.c_uint32),
                ("radius", C.c_uint32), ("fill_min", C.c_uint32), ("reserved", C.c_uint32)]


class DepthFilterCounts(C.Structure):
    """pr_depth_filter_counts: n[c] = the pixels whose flag is c."""
    _fields_ = [("n", C.c_uint32 * 6), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(DepthFilterParamsDesc) == 32 and C.sizeof(DepthFilterCounts) == 32


# pr_reproject_source: one source of a pr_depth_reproject_* call; pr_reproject_params: what pr_reproject_describe fills; pr_reproject_counts: what became of the samples
REPROJECT_MAX_SOURCES, REPROJECT_MAX_RADIUS = 8, 2                          # PR_REPROJECT_MAX_SOURCES, PR_REPROJECT_MAX_RADIUS
SRC_DEPTH_U16, SRC_DEPTH_I32, SRC_CLOUD = range(3)                          # PR_SRC_*: a source's kind
REPROJECT_HIDDEN, REPROJECT_NONE = 254, 255                                 # PR_REPROJECT_*: the source image's codes beside a source index


class ReprojectSourceDesc(C.Structure):
    """pr_reproject_source: a depth frame of another camera or a bare cloud, and its rigid transform into the target camera."""
    _fields_ = [("data", C.c_void_p), ("n_points", C.c_uint64), ("kind", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("reserved", C.c_uint32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("T", C.c_float * 16)]


class ReprojectParamsDesc(C.Structure):
    """pr_reproject_params: the footprint, the gate on the reprojected depth, the tolerance and the visibility window (pr_reproject_describe checks and fills it)."""
    _fields_ = [("splat", C.c_uint32), ("min_mm", C.c_uint32), ("max_mm", C.c_uint32), ("tol_mm", C.c_uint32), ("tol_permille", C.c_uint32),
                ("occl_radius", C.c_uint32), ("occl_min_front", C.c_uint32), ("reserved", C.c_uint32)]


class ReprojectSourceCounts(C.Structure):
    """One source's entry of pr_reproject_counts."""
    _fields_ = [("samples", C.c_uint32), ("invalid", C.c_uint32), ("range", C.c_uint32), ("outside", C.c_uint32), ("drawn", C.c_uint32), ("won", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class ReprojectCounts(C.Structure):
    """pr_reproject_counts: per source what became of its samples and the pixels it won; per frame the covered, hidden and kept pixels."""
    _fields_ = [("source", ReprojectSourceCounts * 8), ("covered", C.c_uint32), ("hidden", C.c_uint32), ("kept", C.c_uint32), ("reserved", C.c_uint32 * 5)]


assert C.sizeof(ReprojectSourceDesc) == 112 and C.sizeof(ReprojectParamsDesc) == 32 and C.sizeof(ReprojectCounts) == 288


# pr_cloud_params: what pr_cloud_describe fills; pr_cloud_counts: the points of a pr_cloud_normals_* call per outcome
KNN_MAX_K, KNN_NONE = 32, 0xFFFFFFFF                                        # PR_KNN_MAX_K, PR_KNN_NONE


class CloudParamsDesc(C.Structure):
    """pr_cloud_params: the neighbourhood (k, max_radius and its square), when a point gets no normal, and the viewpoint normals face (pr_cloud_describe checks and fills it)."""
    _fields_ = [("k", C.c_uint32), ("min_neighbours", C.c_uint32), ("max_radius", C.c_float), ("r2", C.c_float), ("line_ratio", C.c_float),
                ("viewpoint", C.c_float * 3)]


class CloudCounts(C.Structure):
    """pr_cloud_counts: the points, those with a normal, those with too few neighbours, the degenerate ones."""
    _fields_ = [("points", C.c_uint32), ("with_normal", C.c_uint32), ("too_few", C.c_uint32), ("degenerate", C.c_uint32)]


assert C.sizeof(CloudParamsDesc) == 32 and C.sizeof(CloudCounts) == 16


class MeshRef(C.Structure):
    """pr_mesh_ref: one mesh of a mixed batch (pr_*_multi)."""
    _fields_ = [("tris_dev", C.c_void_p), ("n_tris", C.c_size_t)]


class SceneProjDesc(C.Structure):
    _fields_ = [("width", C.c_uint64), ("height", C.c_uint64), ("max_dist_diff", C.c_float), ("K", C.c_float * 9),
                ("pcd", C.c_void_p), ("normal", C.c_void_p)]


class SceneProjCropDesc(C.Structure):
    _fields_ = [("view", SceneProjDesc), ("tl_x", C.c_uint32), ("tl_y", C.c_uint32)]


SCENE_NN_CAM_MAGIC = 0x4d414350          # PR_SCENE_NN_CAM_MAGIC: the camera hint of a pr_scene_nn is read only with it


class SceneNNDesc(C.Structure):
    _fields_ = [("max_dist_diff", C.c_float), ("pcd", C.c_void_p), ("normal", C.c_void_p), ("nodes", C.c_void_p),
                ("n_points", C.c_uint32), ("n_nodes", C.c_uint32),
                ("cam_fx", C.c_float), ("cam_fy", C.c_float), ("cam_cx", C.c_float), ("cam_cy", C.c_float), ("cam_w", C.c_uint32), ("cam_h", C.c_uint32), ("cam_magic", C.c_uint32)]


class SceneGridDesc(C.Structure):
    """pr_scene_grid: a closest-point grid over the scene's volume (pr_scene_grid_describe fills the geometry, pr_scene_grid_build_dev the arrays)."""
    _fields_ = [("origin", C.c_float * 3), ("cell", C.c_float), ("inv_cell", C.c_float), ("dim", C.c_uint32 * 3), ("max_dist_diff", C.c_float),
                ("reach", C.c_float), ("n_points", C.c_uint32), ("cell_point", C.c_void_p), ("rec", C.c_void_p)]


class NNRecordsCounts(C.Structure):
    """pr_nn_records_counts: how many elements the arrays of pr_debug_nn_records hold."""
    _fields_ = [("n_nodes", C.c_uint32), ("n_points", C.c_uint32), ("n_wide", C.c_uint32), ("grid_w", C.c_uint32), ("grid_h", C.c_uint32),
                ("grid_usable", C.c_uint32), ("grid_cells", C.c_uint64)]


NN_RECORDS_FIELDS = ("topo", "bmin", "bmax", "rec64", "rec32", "desc", "pts", "info", "wide", "cell_idx", "grid")


class NNRecordsOut(C.Structure):
    """pr_nn_records_out: host arrays pr_debug_nn_records fills (NULL: skipped)."""
    _fields_ = [(f, C.c_void_p) for f in NN_RECORDS_FIELDS]


# name -> (restype, argtypes); this table is also what tests/test_cabi_symbols.py checks against the header
_vp, _sz, _u32, _i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
SIGNATURES = {
    "pr_last_error": (C.c_char_p, []),
    "pr_version": (C.c_char_p, []),
    "pr_abi_version": (_i32, []),
    "pr_device_count": (_i32, []),
    "pr_init": (_i32, [_i32]),
    "pr_set_device": (_i32, [_i32]),
    "pr_thread_context": (_i32, [_i32]),
    "pr_shutdown": (_i32, []),
    "pr_sync": (_i32, []),
    "pr_malloc": (_i32, [C.POINTER(_vp), _sz]),
    "pr_free": (_i32, [_vp]),
    "pr_memcpy_h2d": (_i32, [_vp, _vp, _sz]),
    "pr_memcpy_d2h": (_i32, [_vp, _vp, _sz]),
    "pr_memcpy_d2d": (_i32, [_vp, _vp, _sz]),
    "pr_fill_i32": (_i32, [_vp, _sz, C.c_int32]),
    "pr_invalidate": (_i32, [_vp, _sz]),
    "pr_scene_proj_crop_dev": (_i32, [_vp, _vp, _sz, _sz, Roi, _vp, _vp]),
    "pr_mesh_count": (_i32, [C.c_char_p, C.POINTER(_sz), C.POINTER(_sz)]),
    "pr_mesh_load": (_i32, [C.c_char_p, _vp, _sz, C.POINTER(_sz), _vp, _sz, C.POINTER(_sz), _vp, _vp, _vp]),
    "pr_ply_count": (_i32, [C.c_char_p, C.POINTER(_sz), C.POINTER(_sz)]),
    "pr_ply_load": (_i32, [C.c_char_p, _vp, _sz, C.POINTER(_sz)]),
    "pr_compute_proj": (None, [_vp, _i32, _i32, C.c_float, C.c_float, _vp]),
    "pr_get_normal": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "pr_scene_proj_prepare": (_i32, [_vp, _i32, _vp, _sz, _sz, _vp, _vp]),
    "pr_scene_proj_prepare_dev": (_i32, [_vp, _i32, _vp, _sz, _sz, _vp, _vp]),
    "pr_raw2depth_mask": (_i32, [_vp, _sz, _vp, _vp]),
    "pr_scene_nn_prepare": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _sz, C.POINTER(_u32), C.POINTER(_u32)]),
    "pr_kdtree_build_dev": (_i32, [_vp, _vp, _sz, _i32, _vp, _sz, C.POINTER(_u32)]),
    "pr_scene_nn_prepare_dev": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _sz, C.POINTER(_u32), C.POINTER(_u32)]),
    "pr_kdtree_build": (_i32, [_vp, _vp, _sz, _i32, _vp, _sz, C.POINTER(_u32)]),
    "pr_solve_666": (None, [_vp, _vp, _vp]),
    "pr_mat4_mul": (None, [_vp, _vp, _vp]),
    "pr_render": (_i32, [_vp, _sz, _vp, _sz, _sz, _sz, _vp, Roi, _vp]),
    "pr_render_to_host": (_i32, [_vp, _sz, _vp, _sz, _sz, _sz, _vp, Roi, _vp]),
    "pr_depth2cloud_i32": (_i32, [_vp, _u32, _u32, _vp, _u32, _u32, _u32, C.POINTER(_vp), C.POINTER(_u32)]),
    "pr_depth2cloud_u16": (_i32, [_vp, _u32, _u32, _vp, _u32, _u32, _u32, C.POINTER(_vp), C.POINTER(_u32)]),
    "pr_icp_proj": (_i32, [_vp, _u32, _vp, Criteria, _vp]),
    "pr_icp_nn": (_i32, [_vp, _u32, _vp, Criteria, _vp]),
    "pr_icp_grid": (_i32, [_vp, _u32, _vp, Criteria, _vp]),
    "pr_scene_grid_describe": (_i32, [_vp, _vp, C.c_float, C.c_float, C.c_float, _vp]),
    "pr_scene_grid_build_dev": (_i32, [_vp, _vp, _vp, _vp]),
    "pr_icp_batch": (_i32, [_vp, _vp, _u32, _i32, _vp, Criteria, _vp]),
    "pr_robust_describe": (_i32, [_u32, C.c_float, _vp]),
    "pr_icp_batch_robust": (_i32, [_vp, _vp, _u32, _i32, _vp, Criteria, _vp, _vp]),
    "pr_refine_pyramid_robust": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, _vp, _u32, Roi, _vp, _vp, _vp, _vp, _u32]),
    "pr_refine_pyramid_robust_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, _vp, _u32, Roi, _vp, _vp, _vp, _vp, _u32]),
    "pr_debug_robust_terms": (_i32, [_vp, _u32, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    "pr_icp_information": (_i32, [_vp, _vp, _u32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_debug_icp_information": (_i32, [_vp, _vp, _u32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "pr_pose_information": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, Roi, _vp, _vp, C.c_float, _vp, _vp, _vp]),
    "pr_pose_information_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, Roi, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_info_covariance": (_i32, [_vp, _vp, C.c_double, C.c_double, _vp, C.POINTER(_u32), C.POINTER(C.c_double)]),
    "pr_refine_batch": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, Criteria, _vp, _vp]),
    "pr_refine_batch_dev": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, Criteria, _vp, _vp]),
    "pr_refine_submit": (_i32, [_i32, _vp, _sz, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, Criteria, _vp, _vp, _vp]),
    "pr_refine_batch_roi": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, Criteria, Roi, _vp, _vp]),
    "pr_refine_submit_roi": (_i32, [_i32, _vp, _sz, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, Criteria, Roi, _vp, _vp, _vp]),
    "pr_refine_wait": (_i32, [_i32]),
    "pr_score_poses": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, _vp]),
    "pr_refined_poses": (None, [_vp, _vp, _u32, _vp]),
    "pr_render_multi": (_i32, [_vp, _u32, _vp, _vp, _sz, _sz, _sz, _vp, Roi, _vp]),
    "pr_refine_batch_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, Criteria, Roi, _vp, _vp]),
    "pr_refine_pyramid": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, _vp, _u32, Roi, _vp, _vp, _vp]),
    "pr_refine_pyramid_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, _vp, _u32, Roi, _vp, _vp, _vp]),
    "pr_score_poses_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, _vp]),
    "pr_score_overlap": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, _vp, _vp]),
    "pr_score_overlap_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, _vp, _vp]),
    "pr_select_greedy": (_i32, [_vp, _u32, _vp, _u32, _u32, _u32, _vp, C.POINTER(_u32)]),
    "pr_score_cover": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, C.POINTER(_u32)]),
    "pr_score_cover_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, C.POINTER(_u32)]),
    "pr_select_cover_host": (_i32, [_vp, _u32, _sz, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "pr_scene_edge_distance_dev": (_i32, [_vp, _i32, _u32, _u32, C.c_int32, _u32, _vp]),
    "pr_score_contours": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "pr_score_contours_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "pr_scene_edge_nearest_dev": (_i32, [_vp, _i32, _u32, _u32, C.c_int32, _u32, _vp]),
    "pr_contour_information": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_float, _vp, _vp, _vp]),
    "pr_contour_information_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pr_info_combine": (_i32, [_vp, C.c_double, _vp, C.c_double, _vp]),
    "pr_info_eig": (_i32, [_vp, _vp]),
    "pr_info_step": (_i32, [_vp, _vp, C.c_double, _vp, _vp, _vp, C.POINTER(_u32)]),
    "pr_score_normals": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, _vp, _u32, C.c_int32, C.c_float, _vp, _vp, _vp]),
    "pr_score_normals_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, _vp, _u32, C.c_int32, C.c_float, _vp, _vp, _vp]),
    "pr_compose_detections": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "pr_compose_detections_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, Roi, _vp, _i32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "pr_pose_distance": (_i32, [_vp, _u32, _vp, _u32, _vp, _u32, _i32, _vp, _u32, _vp, _vp]),
    "pr_cluster_greedy": (_i32, [_vp, _u32, _vp, _u32, C.c_float, _vp, C.POINTER(_u32), _vp]),
    "pr_ppf_describe": (_i32, [C.c_float, C.c_float, _u32, _u32, _i32, _vp]),
    "pr_ppf_model_sample": (_i32, [_vp, _sz, C.c_float, _i32, _vp, _vp, C.POINTER(_u32)]),
    "pr_ppf_model_build_dev": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "pr_ppf_scene_points_dev": (_i32, [_vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "pr_ppf_vote": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "pr_ppf_peak_pose": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "pr_ppf_vote_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "pr_plane_describe": (_i32, [_u32, _u32, C.c_float, C.c_float, C.c_float, _u32, _u32, _i32, _vp]),
    "pr_plane_from_moments": (_i32, [_vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double), _vp]),
    "pr_scene_planes_dev": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u32)]),
    "pr_scene_planes_host": (_i32, [_vp, _vp, _vp, _i32, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u32)]),
    "pr_segment_describe": (_i32, [_u32, _u32, _u32, _vp]),
    "pr_scene_segments_dev": (_i32, [_vp, _i32, _sz, _sz, _vp, _vp, _vp, _vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "pr_scene_segments_host": (_i32, [_vp, _i32, _sz, _sz, _vp, _vp, _vp, _vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "pr_segment_depth_dev": (_i32, [_vp, _vp, _i32, _sz, _vp, _u32, _vp]),
    "pr_segment_roi": (_i32, [_vp, _sz, _sz, _u32, C.POINTER(Roi)]),
    "pr_depth_filter_describe": (_i32, [_u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp]),
    "pr_depth_fuse_dev": (_i32, [_vp, _u32, _i32, _sz, _u32, _vp, _vp]),
    "pr_depth_fuse_host": (_i32, [_vp, _u32, _i32, _sz, _u32, _vp, _vp]),
    "pr_depth_filter_dev": (_i32, [_vp, _i32, _sz, _sz, _vp, _vp, _vp, _vp]),
    "pr_depth_filter_host": (_i32, [_vp, _i32, _sz, _sz, _vp, _vp, _vp, _vp]),
    "pr_reproject_describe": (_i32, [_u32, _u32, _u32, _u32, _u32, _u32, _u32, _vp]),
    "pr_depth_reproject_dev": (_i32, [_vp, _u32, _sz, _sz, C.c_float, C.c_float, C.c_float, C.c_float, _i32, _vp, _vp, _vp, _vp]),
    "pr_depth_reproject_host": (_i32, [_vp, _u32, _sz, _sz, C.c_float, C.c_float, C.c_float, C.c_float, _i32, _vp, _vp, _vp, _vp]),
    "pr_cloud_describe": (_i32, [_u32, C.c_float, _u32, C.c_float, _vp, _vp]),
    "pr_cloud_knn_dev": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "pr_cloud_normals_dev": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "pr_scene_nn_from_cloud_dev": (_i32, [_vp, _sz, _i32, _vp, _vp, _vp, _sz, C.POINTER(_u32), _vp]),
    "pr_cloud_knn_host": (_i32, [_vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "pr_cloud_normals_host": (_i32, [_vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp]),
    "pr_ppf_cloud_points_dev": (_i32, [_vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "pr_pose_vsd": (_i32, [_vp, _sz, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, C.c_float, _vp, _u32, _vp]),
    "pr_pose_vsd_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp, _i32, _vp, C.c_float, _vp, _u32, _vp]),
    "pr_render_span": (_i32, [_vp, _sz, _vp, _sz, _sz, _sz, _vp, Roi, _vp, _vp]),
    "pr_pose_penetration": (_i32, [_vp, _sz, _vp, _u32, _u32, _u32, _vp, C.c_int32, _vp]),
    "pr_pose_penetration_multi": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _vp, C.c_int32, _vp]),
    "pr_select_disjoint": (_i32, [_vp, _u32, _vp, _u32, _u32, _u32, _vp, C.POINTER(_u32)]),
    "pr_comm_id": (_i32, [_vp]),
    "pr_comm_init_rank": (_i32, [_vp, _i32, _i32]),
    "pr_comm_init_all": (_i32, [_i32]),
    "pr_comm_rank": (_i32, [C.POINTER(_i32), C.POINTER(_i32)]),
    "pr_comm_destroy": (_i32, []),
    "pr_gather_results": (_i32, [_vp, _u32, _u32, _i32, _vp]),
    "pr_shard_range": (None, [_u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "pr_set_option": (_i32, [C.c_char_p, _i32]),
    "pr_get_option": (_i32, [C.c_char_p, C.POINTER(_i32)]),
    "pr_nn_counters": (_i32, [_vp, _u32]),
    "pr_profile_reset": (_i32, []),
    "pr_profile_read": (_i32, [C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pr_gather_profile": (_i32, [C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "pr_profile_launches": (_i32, [_vp, _u32, C.POINTER(_u32)]),
    "pr_profile_nn": (_i32, [_vp, C.POINTER(C.c_uint64)]),
    "pr_debug_contrib29": (_i32, [_vp, _u32, _i32, _vp, _vp, _i32, _vp]),
    "pr_debug_pose_iteration": (_i32, [_vp, _vp, _u32, Criteria, _u32, _i32, _vp, _vp, _vp]),
    "pr_debug_trace_sums": (_i32, [_vp, _u32, _u32]),
    "pr_debug_mesh_order": (_i32, [_vp, _sz, _vp]),
    "pr_debug_mesh_fingerprint": (_i32, [_vp, _sz, C.POINTER(C.c_uint64)]),
    "pr_debug_tight_box": (_i32, [_vp, _sz, _vp, _vp, _u32, _u32, Roi, _vp, _vp]),
    "pr_debug_box_layout": (_i32, [_vp, _u32, _u32, _i32, _vp, _vp, _sz, _vp, _vp]),
    "pr_debug_nn_records": (_i32, [_vp, _u32, _u32, _vp, C.POINTER(NNRecordsCounts), C.POINTER(NNRecordsOut)]),
    "pr_stats": (_i32, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
}

_lib = None


def load():
    """Load (once) the in-tree shared library and bind every entry point of the header."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -m pose_refine_amd.build` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int):
    if rc != PR_OK:
        raise PoseRefineError(rc, load().pr_last_error().decode(errors="replace"))


def ptr(a: np.ndarray) -> int:
    return a.ctypes.data
