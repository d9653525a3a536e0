"""ctypes binding of the C ABI (include/orbfe.h) -- plumbing for tests and bench.py.

The product is liborbfe.so (HIP, gfx950).  This module never computes anything
itself and has no CPU fallback: if the library is missing or no GPU is present
the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liborbfe.so")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5

EXPORTS = [
    "orbfe_build_id", "orbfe_set_pattern", "orbfe_get_pattern", "orbfe_blur_ride_from", "orbfe_set_input_retained",
    "orbfe_abi_version", "orbfe_last_error", "orbfe_create", "orbfe_destroy", "orbfe_levels",
    "orbfe_keypoint_capacity", "orbfe_get_tables", "orbfe_level_size", "orbfe_extract",
    "orbfe_stereo_frame", "orbfe_rgbd_frame", "orbfe_rgbd_frame_u16", "orbfe_fetch_pyramid", "orbfe_enqueue_extract",
    "orbfe_enqueue_stereo", "orbfe_synchronize", "orbfe_fetch_image", "orbfe_fetch_counts",
    "orbfe_device_buffers", "orbfe_fetch_candidates", "orbfe_hamming_matrix",
    "orbfe_set_profiling", "orbfe_stage_name", "orbfe_stage_times", "orbfe_set_streams", "orbfe_quadtree_kernel", "orbfe_quadtree_plan",
    "orbfe_features_in_area", "orbfe_features_in_area_batch", "orbfe_three_maxima", "orbfe_search_by_projection_last", "orbfe_is_in_frustum",
    "orbfe_search_by_projection_points", "orbfe_search_by_projection_kf", "orbfe_search_for_initialization",
    "orbfe_vocab_load", "orbfe_bow_transform", "orbfe_bow_maps", "orbfe_search_by_bow", "orbfe_search_by_bow_kf",  # bound in orbslam2_amd/bow.py
    "orbfe_search_for_triangulation", "orbfe_fuse", "orbfe_search_by_projection_sim3", "orbfe_fuse_sim3", "orbfe_search_by_sim3", "orbfe_kfdb_clear", "orbfe_kfdb_add", "orbfe_kfdb_erase", "orbfe_kfdb_size", "orbfe_kfdb_score", "orbfe_detect_reloc_candidates", "orbfe_detect_loop_candidates",
    "orbfe_pose_optimization", "orbfe_pose_optimization_batch", "orbfe_enqueue_pose_optimization", "orbfe_set_input_format", "orbfe_fetch_batch_async", "orbfe_set_rectification", "orbfe_set_distortion", "orbfe_undistort_keypoints", "orbfe_fetch_keys_un", "orbfe_image_bounds",
    "orbfe_png_last_error", "orbfe_png_info", "orbfe_png_decode", "orbfe_png_decode_batch",
    "orbfe_get_camera", "orbfe_assign_features_to_grid", "orbfe_set_profiling_interval", "orbfe_stereo_batch", "orbfe_device_count", "orbfe_vocab_bytes",
    "orbfe_get_packed_layout", "orbfe_fetch_batch_packed", "orbfe_expand_packed", "orbfe_enqueue_rgbd", "orbfe_stereo_batch_packed",
    "orbfe_enqueue_search_by_projection_last", "orbfe_enqueue_is_in_frustum", "orbfe_enqueue_search_by_projection_points", "orbfe_device_keys_un",
    "orbfe_enqueue_compute_bow", "orbfe_enqueue_search_by_bow", "orbfe_enqueue_search_by_bow_batch",
    "orbfe_enqueue_search_by_projection_kf", "orbfe_enqueue_search_by_projection_kf_batch",
    "orbfe_enqueue_search_for_triangulation",
    "orbfe_enqueue_keyframe_grid", "orbfe_enqueue_fuse", "orbfe_enqueue_fuse_sim3",
    "orbfe_enqueue_search_by_sim3", "orbfe_enqueue_search_by_projection_sim3", "orbfe_enqueue_optimize_sim3", "orbfe_optimize_sim3",
    "orbfe_enqueue_sim3_ransac_batch", "orbfe_enqueue_sim3_ransac_select", "orbfe_sim3_ransac",
    "orbfe_enqueue_pnp_ransac_batch", "orbfe_enqueue_pnp_ransac_select", "orbfe_pnp_ransac",
    "orbfe_enqueue_search_by_bow_kf", "orbfe_enqueue_search_by_bow_kf_batch",
    "orbfe_enqueue_update_map_points",
    "orbfe_enqueue_local_bundle_adjustment", "orbfe_local_bundle_adjustment",
    "orbfe_essential_graph_plan_size", "orbfe_essential_graph_plan", "orbfe_enqueue_optimize_essential_graph", "orbfe_optimize_essential_graph",
    "orbfe_enqueue_triangulate_pairs",
    "orbfe_enqueue_find_homography_fundamental", "orbfe_find_homography_fundamental",
    "orbfe_enqueue_reconstruct_initial", "orbfe_reconstruct_initial",
]
NUM_STAGES = 8
STAGE_NAMES = ["ingest", "pyramid", "blur", "fast", "octree", "describe", "stereo_match", "stereo_median"]  # orbfe_stage_name()


class Params(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("patch_size", C.c_int32),
                ("half_patch_size", C.c_int32), ("edge_threshold", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("bf", C.c_float), ("device", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("max_images", C.c_int32)]


class FrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("keys_un", C.c_void_p), ("u_right", C.c_void_p), ("descriptors", C.c_void_p),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("device_slot_plus1", C.c_int32), ("keyframe", C.c_int32)]


class PackedLayout(C.Structure):
    """orbfe_packed_layout (include/orbfe.h): byte offsets of the arrays inside a packed result block."""
    _fields_ = [("n_images_out", C.c_int32), ("capacity", C.c_int32), ("nlevels", C.c_int32), ("n_pairs", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("counts_off", C.c_size_t), ("level_counts_off", C.c_size_t), ("xy_off", C.c_size_t), ("angle_off", C.c_size_t),
                ("response_off", C.c_size_t), ("desc_off", C.c_size_t), ("u_right_off", C.c_size_t), ("depth_off", C.c_size_t), ("bytes", C.c_size_t)]


class BowKeyframe(C.Structure):
    """orbfe_bow_keyframe (include/orbfe.h): one candidate keyframe of enqueue_search_by_bow_batch, either keyframe of
    enqueue_search_by_bow_kf / _batch; device pointers."""
    _fields_ = [("nodes", C.c_void_p), ("off", C.c_void_p), ("feat", C.c_void_p), ("valid", C.c_void_p), ("desc", C.c_void_p),
                ("angle", C.c_void_p), ("pos", C.c_void_p), ("nnodes", C.c_int32), ("n", C.c_int32)]


class TriKeyframe(C.Structure):
    """orbfe_tri_keyframe (include/orbfe.h): one keyframe of enqueue_search_for_triangulation, device pointers."""
    _fields_ = [("nodes", C.c_void_p), ("off", C.c_void_p), ("feat", C.c_void_p), ("keys_un", C.c_void_p), ("u_right", C.c_void_p),
                ("has_mp", C.c_void_p), ("desc", C.c_void_p), ("nnodes", C.c_int32), ("n", C.c_int32)]


assert C.sizeof(TriKeyframe) == 64


class GridKeyframe(C.Structure):
    """orbfe_grid_keyframe (include/orbfe.h): the keyframe of enqueue_fuse / enqueue_fuse_sim3 and the Sim3 matchers, device pointers; cell_off / cell_idx as
    enqueue_keyframe_grid wrote them, the bounds the frame's floats."""
    _fields_ = [("keys_un", C.c_void_p), ("u_right", C.c_void_p), ("desc", C.c_void_p), ("cell_off", C.c_void_p), ("cell_idx", C.c_void_p),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("n", C.c_int32), ("keyframe", C.c_int32)]


assert C.sizeof(GridKeyframe) == 64


class Sim3OptParams(C.Structure):
    """orbfe_sim3_opt_params (include/orbfe.h): Optimizer's sim3Iterations, additionalIterations, additionalIterationsNoOutliers and
    minimumInliersBeforeFail; the reference's values are the defaults."""
    _fields_ = [("iterations", C.c_int32), ("more_iterations_outliers", C.c_int32), ("more_iterations_clean", C.c_int32), ("min_inliers", C.c_int32)]

    def __init__(self, iterations=5, more_iterations_outliers=10, more_iterations_clean=5, min_inliers=10):
        super().__init__(iterations, more_iterations_outliers, more_iterations_clean, min_inliers)


SIM3_OPT_LDS_SLOTS = 2048  # ORBFE_SIM3_OPT_LDS_SLOTS


class Sim3RansacCandidate(C.Structure):
    """orbfe_sim3_ransac_candidate (include/orbfe.h): one candidate keyframe of enqueue_sim3_ransac_batch, device pointers; an ARRAY of
    these records lives in HBM.  pairs / n_pairs: row c of enqueue_search_by_bow_kf_batch's d_pairs and &d_nmatches[c]."""
    _fields_ = [("keys_un", C.c_void_p), ("pos", C.c_void_p), ("valid", C.c_void_p), ("T2w", C.c_void_p), ("pairs", C.c_void_p), ("n_pairs", C.c_void_p),
                ("draws", C.c_void_p), ("n", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(Sim3RansacCandidate) == 64
# orbfe_sim3_hypothesis: one iteration's mnInliersi, ms12i, mR12i (row-major), mt12i
SIM3_HYP_DTYPE = np.dtype([("n_inliers", "<i4"), ("s12", "<f4"), ("R12", "<f4", (9,)), ("t12", "<f4", (3,)), ("pad", "<i4", (2,))])
assert SIM3_HYP_DTYPE.itemsize == 64
SIM3_RANSAC_LDS_SLOTS = 1024  # ORBFE_SIM3_RANSAC_LDS_SLOTS


class PnPCandidate(C.Structure):
    """orbfe_pnp_candidate (include/orbfe.h): one candidate keyframe of enqueue_pnp_ransac_batch, device pointers; an ARRAY of these
    records lives in HBM.  f_match: row c of enqueue_search_by_bow_batch's d_f_match; draws: [max_its][4] raw rand() values."""
    _fields_ = [("f_match", C.c_void_p), ("pos", C.c_void_p), ("valid", C.c_void_p), ("draws", C.c_void_p), ("n", C.c_int32), ("reserved", C.c_int32 * 7)]


assert C.sizeof(PnPCandidate) == 64
# orbfe_pnp_hypothesis / orbfe_pnp_refined: one iteration of PnPsolver::iterate; Refine() on a record holder's inliers
PNP_HYP_DTYPE = np.dtype([("n_inliers", "<i4"), ("best_k", "<i4"), ("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("pad", "<i4", (2,))])
PNP_REFINED_DTYPE = np.dtype([("ok", "<i4"), ("n_inliers", "<i4"), ("Tcw", "<f4", (12,)), ("pad", "<i4", (2,))])
assert PNP_HYP_DTYPE.itemsize == 64 and PNP_REFINED_DTYPE.itemsize == 64
PNP_RANSAC_LDS_SLOTS = 1024  # ORBFE_PNP_RANSAC_LDS_SLOTS
PNP_EVENT, PNP_EXHAUSTED = 0, 1  # ORBFE_PNP_EVENT, ORBFE_PNP_EXHAUSTED


class ObsKeyframe(C.Structure):
    """orbfe_obs_keyframe (include/orbfe.h): one keyframe as enqueue_update_map_points reads it, device pointers; an ARRAY of these
    records lives in HBM (the keyframe directory), Ow and bad patched on the stream as the map changes."""
    _fields_ = [("desc", C.c_void_p), ("keys_un", C.c_void_p), ("Ow", C.c_float * 3), ("n", C.c_int32), ("bad", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(ObsKeyframe) == 40
OBS_KF_DTYPE = np.dtype([("desc", "<u8"), ("keys_un", "<u8"), ("Ow", "<f4", 3), ("n", "<i4"), ("bad", "<i4"), ("reserved", "<i4")])  # the same, as a numpy record
assert OBS_KF_DTYPE.itemsize == 40
MP_DESCRIPTOR, MP_NORMAL_DEPTH = 1, 2  # ORBFE_MP_*


class BaKeyframe(C.Structure):
    """orbfe_ba_keyframe (include/orbfe.h): one keyframe as enqueue_local_bundle_adjustment reads it, device pointers; an ARRAY of
    these records lives in HBM."""
    _fields_ = [("keys_un", C.c_void_p), ("u_right", C.c_void_p), ("n", C.c_int32), ("reserved", C.c_int32 * 3)]


class LbaInfo(C.Structure):
    """orbfe_lba_info (include/orbfe.h): edges built, active free keyframes and points, per optimize() the iterations run and the
    system solves tried, the robust chi2 at entry and after either round, the last lambda."""
    _fields_ = [("n_mono", C.c_int32), ("n_stereo", C.c_int32), ("n_free", C.c_int32), ("n_points", C.c_int32),
                ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2),
                ("chi2_start", C.c_double), ("chi2_first", C.c_double), ("chi2_second", C.c_double), ("lambda_last", C.c_double)]


assert C.sizeof(BaKeyframe) == 32 and C.sizeof(LbaInfo) == 64
LBA_INFO_DTYPE = np.dtype([("n_mono", "<i4"), ("n_stereo", "<i4"), ("n_free", "<i4"), ("n_points", "<i4"), ("iterations", "<i4", 2), ("trials", "<i4", 2),
                           ("chi2_start", "<f8"), ("chi2_first", "<f8"), ("chi2_second", "<f8"), ("lambda_last", "<f8")])  # the same, as a numpy record
assert LBA_INFO_DTYPE.itemsize == 64
BA_SKIP, BA_LOCAL, BA_LOCAL_HELD, BA_FIXED = 0, 1, 2, 3  # ORBFE_BA_*
BA_CODE_LEVEL1, BA_CODE_ERASE, BA_CODE_SKIPPED, BA_CODE_FAULTY = 1, 2, 4, 8  # bits of d_edge_code
LBA_LDS_KEYFRAMES = 21  # ORBFE_LBA_LDS_KEYFRAMES

# orbfe_essential_plan_header and orbfe_essential_graph_info (include/orbfe.h): Optimizer::OptimizeEssentialGraph
ESSENTIAL_PLAN_MAGIC = 0x31504745
ESSENTIAL_PLAN_HEADER_DTYPE = np.dtype([(k, "<i4") for k in (
    "magic", "n_kfs", "fixed_kf", "n_edges", "n_free", "n_lblocks", "n_slot_edges", "n_updates", "blob_bytes", "off_order", "off_pos", "off_colptr",
    "off_rowidx", "off_edge_slots", "off_slot_ptr", "off_slot_edges", "off_upd_ptr", "off_upd")] + [("reserved", "<i4", 2)])
assert ESSENTIAL_PLAN_HEADER_DTYPE.itemsize == 80
EG_INFO_DTYPE = np.dtype([("iterations", "<i4"), ("trials", "<i4"), ("n_active_edges", "<i4"), ("n_lblocks", "<i4"), ("chi2_start", "<f8"),
                          ("chi2_end", "<f8"), ("lambda_last", "<f8"), ("in_lds", "<i4"), ("reserved", "<i4")])
assert EG_INFO_DTYPE.itemsize == 48
EG_EDGE_INDEX, EG_EDGE_SIM3 = 1, 2
EG_LDS_DOUBLES = 16064  # ORBFE_EG_LDS_DOUBLES
EG_LAMBDA_INIT = float(np.float32(1.0e-16))  # Optimizer::mInitialLambda


class NewpointKeyframe(C.Structure):
    """orbfe_newpoint_keyframe (include/orbfe.h): one keyframe of enqueue_triangulate_pairs; device pointers (has_mp is written) and the
    host scalars of the keyframe: Tcw (3x4, row major), GetCameraCenter() and the camera."""
    _fields_ = [("keys_un", C.c_void_p), ("keys", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p), ("cos_stereo", C.c_void_p),
                ("has_mp", C.c_void_p), ("Tcw", C.c_float * 12), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float), ("n", C.c_int32)]


assert C.sizeof(NewpointKeyframe) == 136
GRID_CELLS = 64 * 48  # FRAME_GRID_COLS * FRAME_GRID_ROWS: cell_off holds GRID_CELLS + 1 entries


class RelocCandidate(C.Structure):
    """orbfe_reloc_candidate (include/orbfe.h): one candidate keyframe of enqueue_search_by_projection_kf_batch, device pointers."""
    _fields_ = [("Tcw", C.c_void_p), ("pos", C.c_void_p), ("desc", C.c_void_p), ("valid", C.c_void_p), ("angle", C.c_void_p),
                ("max_distance", C.c_void_p), ("min_distance", C.c_void_p), ("cur_point", C.c_void_p), ("outlier", C.c_void_p),
                ("n", C.c_int32), ("th", C.c_float), ("orb_dist", C.c_int32), ("reserved", C.c_int32)]


PACK_STEREO, PACK_LEFT_ONLY, PACK_DIRECT = 1, 2, 4

TP_DTYPE = np.dtype([("in_view", "<i4"), ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("level", "<i4"), ("view_cos", "<f4")])


class OrbfeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("orbfe error %d: %s" % (code, msg))
        self.code = code


_lib = None


def build_id() -> str:
    """orbfe_build_id(): sha256 over the sources and flags liborbfe.so was built from."""
    return load().orbfe_build_id().decode()


def load():
    """Load liborbfe.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("liborbfe.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "or `make -C orbslam2_amd/csrc`")
    # PyTorch-ROCm bundles its own libamdhip64.so.7; two HIP runtimes in one process make the second one
    # see no GPU.  Importing torch first makes its copy the process-wide runtime that liborbfe.so binds to.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.orbfe_abi_version.restype = C.c_int
    L.orbfe_build_id.restype = C.c_char_p
    L.orbfe_set_pattern.restype = C.c_int; L.orbfe_set_pattern.argtypes = [vp, vp]
    L.orbfe_get_pattern.restype = C.c_int; L.orbfe_get_pattern.argtypes = [vp, vp]
    L.orbfe_blur_ride_from.restype = C.c_int; L.orbfe_blur_ride_from.argtypes = [vp, C.c_int]
    L.orbfe_set_input_retained.restype = C.c_int; L.orbfe_set_input_retained.argtypes = [vp, C.c_int]
    L.orbfe_last_error.restype = C.c_char_p; L.orbfe_last_error.argtypes = [vp]
    L.orbfe_create.restype = C.c_int; L.orbfe_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.orbfe_destroy.restype = None; L.orbfe_destroy.argtypes = [vp]
    L.orbfe_levels.restype = C.c_int; L.orbfe_levels.argtypes = [vp]
    L.orbfe_keypoint_capacity.restype = C.c_int; L.orbfe_keypoint_capacity.argtypes = [vp]
    L.orbfe_get_tables.restype = C.c_int; L.orbfe_get_tables.argtypes = [vp] + [vp] * 6
    L.orbfe_level_size.restype = C.c_int; L.orbfe_level_size.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.orbfe_extract.restype = C.c_int
    L.orbfe_extract.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.orbfe_stereo_frame.restype = C.c_int
    L.orbfe_stereo_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, vp, vp, C.POINTER(C.c_int),
                                     vp, vp, C.POINTER(C.c_int), vp, vp, C.c_int]
    L.orbfe_rgbd_frame.restype = C.c_int
    L.orbfe_rgbd_frame.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t, vp, vp, C.POINTER(C.c_int), vp, vp, C.c_int]
    L.orbfe_rgbd_frame_u16.restype = C.c_int
    L.orbfe_rgbd_frame_u16.argtypes = [vp, vp, vp, C.c_float, C.c_int, C.c_int, C.c_size_t, C.c_size_t, vp, vp, C.POINTER(C.c_int), vp, vp, C.c_int]
    L.orbfe_fetch_pyramid.restype = C.c_int
    L.orbfe_fetch_pyramid.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t]
    L.orbfe_enqueue_extract.restype = C.c_int; L.orbfe_enqueue_extract.argtypes = [vp, vp, C.c_int, vp]
    L.orbfe_enqueue_stereo.restype = C.c_int; L.orbfe_enqueue_stereo.argtypes = [vp, vp, C.c_int, vp]
    L.orbfe_synchronize.restype = C.c_int; L.orbfe_synchronize.argtypes = [vp, vp]
    L.orbfe_fetch_image.restype = C.c_int
    L.orbfe_fetch_image.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.orbfe_fetch_counts.restype = C.c_int; L.orbfe_fetch_counts.argtypes = [vp, vp, C.c_int]
    L.orbfe_device_buffers.restype = C.c_int; L.orbfe_device_buffers.argtypes = [vp] + [C.POINTER(vp)] * 5
    L.orbfe_fetch_candidates.restype = C.c_int
    L.orbfe_fetch_candidates.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.orbfe_hamming_matrix.restype = C.c_int
    L.orbfe_hamming_matrix.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp]
    L.orbfe_set_profiling.restype = C.c_int; L.orbfe_set_profiling.argtypes = [vp, C.c_int]
    L.orbfe_stage_name.restype = C.c_char_p; L.orbfe_stage_name.argtypes = [C.c_int]
    L.orbfe_stage_times.restype = C.c_int; L.orbfe_stage_times.argtypes = [vp, vp, C.POINTER(C.c_int), C.c_int]
    L.orbfe_set_streams.restype = C.c_int; L.orbfe_set_streams.argtypes = [vp, C.c_int]
    L.orbfe_quadtree_kernel.restype = C.c_int; L.orbfe_quadtree_kernel.argtypes = [vp]
    L.orbfe_quadtree_plan.restype = C.c_int; L.orbfe_quadtree_plan.argtypes = [vp]
    fvp, ip = C.POINTER(FrameView), C.POINTER(C.c_int)
    L.orbfe_features_in_area.restype = C.c_int
    L.orbfe_features_in_area.argtypes = [vp, fvp, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, vp, C.c_int, ip]
    L.orbfe_features_in_area_batch.restype = C.c_int
    L.orbfe_features_in_area_batch.argtypes = [vp, fvp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int]
    L.orbfe_three_maxima.restype = C.c_int; L.orbfe_three_maxima.argtypes = [vp, C.c_int, ip, ip, ip]
    L.orbfe_search_by_projection_last.restype = C.c_int
    L.orbfe_search_by_projection_last.argtypes = [vp, fvp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_int, C.c_int, vp, ip]
    L.orbfe_is_in_frustum.restype = C.c_int
    L.orbfe_is_in_frustum.argtypes = [vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, vp, vp, vp, vp, C.c_float, vp]
    L.orbfe_search_by_projection_points.restype = C.c_int
    L.orbfe_search_by_projection_points.argtypes = [vp, fvp, C.c_int, vp, vp, vp, vp, C.c_float, C.c_float, vp, ip]
    L.orbfe_search_by_projection_kf.restype = C.c_int
    L.orbfe_search_by_projection_kf.argtypes = [vp, fvp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_int, C.c_int, vp, ip]
    L.orbfe_fuse.restype = C.c_int
    L.orbfe_fuse.argtypes = [vp, fvp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, vp, ip]
    L.orbfe_search_by_projection_sim3.restype = C.c_int
    L.orbfe_search_by_projection_sim3.argtypes = [vp, fvp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_float, vp, ip]
    L.orbfe_fuse_sim3.restype = C.c_int
    L.orbfe_fuse_sim3.argtypes = [vp, fvp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, vp, ip]
    L.orbfe_search_by_sim3.restype = C.c_int
    L.orbfe_search_by_sim3.argtypes = [vp] + [fvp, vp, vp, vp, vp, vp, vp] * 2 + [C.c_float, vp, vp, C.c_float, vp, ip]
    L.orbfe_set_distortion.restype = C.c_int
    L.orbfe_set_distortion.argtypes = [vp, vp, C.c_int]
    L.orbfe_undistort_keypoints.restype = C.c_int
    L.orbfe_undistort_keypoints.argtypes = [vp, vp, C.c_int, vp]
    L.orbfe_fetch_keys_un.restype = C.c_int
    L.orbfe_fetch_keys_un.argtypes = [vp, C.c_int, vp, C.c_int, ip]
    L.orbfe_image_bounds.restype = C.c_int
    L.orbfe_image_bounds.argtypes = [vp, vp]
    L.orbfe_fetch_batch_async.restype = C.c_int
    L.orbfe_fetch_batch_async.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.orbfe_get_packed_layout.restype = C.c_int
    L.orbfe_get_packed_layout.argtypes = [vp, C.c_int, C.c_int, C.POINTER(PackedLayout)]
    L.orbfe_fetch_batch_packed.restype = C.c_int
    L.orbfe_fetch_batch_packed.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, vp]
    L.orbfe_expand_packed.restype = C.c_int
    L.orbfe_expand_packed.argtypes = [vp, vp, C.POINTER(PackedLayout), C.c_int, vp, C.c_int, ip]
    L.orbfe_enqueue_rgbd.restype = C.c_int
    L.orbfe_enqueue_rgbd.argtypes = [vp, vp, vp, C.c_int, C.c_float, C.c_int, vp]
    L.orbfe_set_rectification.restype = C.c_int
    L.orbfe_set_rectification.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int]
    L.orbfe_set_input_format.restype = C.c_int
    L.orbfe_set_input_format.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.orbfe_pose_optimization.restype = C.c_int
    L.orbfe_pose_optimization.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, ip]
    L.orbfe_pose_optimization_batch.restype = C.c_int
    L.orbfe_pose_optimization_batch.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_enqueue_pose_optimization.restype = C.c_int
    L.orbfe_enqueue_pose_optimization.argtypes = [vp, C.c_int] + [vp] * 8 + [C.c_int, vp]
    L.orbfe_search_for_initialization.restype = C.c_int
    L.orbfe_search_for_initialization.argtypes = [vp, fvp, fvp, vp, C.c_int, C.c_float, C.c_int, vp, ip]
    L.orbfe_enqueue_search_by_projection_last.restype = C.c_int
    L.orbfe_enqueue_search_by_projection_last.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 7 + [C.c_float, C.c_int, C.c_int] + [vp] * 6
    L.orbfe_enqueue_is_in_frustum.restype = C.c_int
    L.orbfe_enqueue_is_in_frustum.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_float, vp, vp]
    L.orbfe_enqueue_search_by_projection_points.restype = C.c_int
    L.orbfe_enqueue_search_by_projection_points.argtypes = [vp, C.c_int, vp, C.c_int] + [vp] * 5 + [C.c_float, C.c_float] + [vp] * 6
    L.orbfe_device_keys_un.restype = C.c_int
    L.orbfe_device_keys_un.argtypes = [vp, C.c_int, C.POINTER(vp), vp]
    L.orbfe_enqueue_compute_bow.restype = C.c_int
    L.orbfe_enqueue_compute_bow.argtypes = [vp, C.c_int, C.c_int] + [vp] * 12
    L.orbfe_enqueue_search_by_bow.restype = C.c_int
    L.orbfe_enqueue_search_by_bow.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp] + [vp] * 4 + [C.c_float, C.c_int] + [vp] * 6
    L.orbfe_enqueue_search_by_bow_batch.restype = C.c_int
    L.orbfe_enqueue_search_by_bow_batch.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int] + [vp] * 4 + [C.c_float, C.c_int] + [vp] * 6
    L.orbfe_enqueue_search_by_projection_kf.restype = C.c_int
    L.orbfe_enqueue_search_by_projection_kf.argtypes = [vp, C.c_int, vp, vp, C.c_int] + [vp] * 8 + [C.c_float, C.c_int, C.c_int, C.c_int] + [vp] * 6
    L.orbfe_enqueue_search_by_projection_kf_batch.restype = C.c_int
    L.orbfe_enqueue_search_by_projection_kf_batch.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int] + [vp] * 6
    L.orbfe_enqueue_search_for_triangulation.restype = C.c_int
    L.orbfe_enqueue_search_for_triangulation.argtypes = [vp, C.POINTER(TriKeyframe), C.POINTER(TriKeyframe), vp, vp, vp] + [C.c_float] * 4 + \
        [C.c_int, C.c_int] + [vp] * 5
    L.orbfe_enqueue_keyframe_grid.restype = C.c_int
    L.orbfe_enqueue_keyframe_grid.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    for fn in (L.orbfe_enqueue_fuse, L.orbfe_enqueue_fuse_sim3):
        fn.restype = C.c_int
        fn.argtypes = [vp, C.POINTER(GridKeyframe), vp, C.c_int, vp, C.c_int] + [vp] * 6 + [C.c_float] + [vp] * 4
    L.orbfe_enqueue_optimize_sim3.restype = C.c_int
    L.orbfe_enqueue_optimize_sim3.argtypes = ([vp] + [C.POINTER(GridKeyframe), vp, vp, vp] * 2 + [C.c_float, vp, vp, C.c_float, C.c_int, C.POINTER(Sim3OptParams)]
                                              + [vp] * 6)
    L.orbfe_optimize_sim3.restype = C.c_int
    L.orbfe_optimize_sim3.argtypes = [vp] + [vp, C.c_int, vp, vp, vp] * 2 + [C.c_float, vp, vp, C.c_float, C.c_int, C.POINTER(Sim3OptParams), vp, vp, vp, ip]
    L.orbfe_enqueue_sim3_ransac_batch.restype = C.c_int
    L.orbfe_enqueue_sim3_ransac_batch.argtypes = [vp, C.POINTER(GridKeyframe), vp, vp, vp, vp] + [C.c_int] * 6 + [vp] * 11
    L.orbfe_enqueue_sim3_ransac_select.restype = C.c_int
    L.orbfe_enqueue_sim3_ransac_select.argtypes = [vp, vp] + [C.c_int] * 4 + [vp] + [C.c_int] * 3 + [vp] * 9
    L.orbfe_enqueue_pnp_ransac_batch.restype = C.c_int
    L.orbfe_enqueue_pnp_ransac_batch.argtypes = [vp, C.c_int, vp] + [C.c_int] * 6 + [C.c_float] * 2 + [vp] * 14
    L.orbfe_enqueue_pnp_ransac_select.restype = C.c_int
    L.orbfe_enqueue_pnp_ransac_select.argtypes = [vp] + [C.c_int] * 6 + [vp] * 13
    L.orbfe_pnp_ransac.restype = C.c_int
    L.orbfe_pnp_ransac.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int, vp] + [C.c_int] * 4 + [C.c_float] * 2 + [vp, ip, ip] + [vp] * 7 + [ip, ip]
    L.orbfe_sim3_ransac.restype = C.c_int
    L.orbfe_sim3_ransac.argtypes = [vp] + [vp, C.c_int, vp, vp, vp] * 2 + [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, ip, ip, vp, vp, vp, vp, vp, ip]
    L.orbfe_enqueue_search_by_sim3.restype = C.c_int
    L.orbfe_enqueue_search_by_sim3.argtypes = [vp] + [C.POINTER(GridKeyframe)] + [vp] * 6 + [C.POINTER(GridKeyframe)] + [vp] * 6 + [C.c_float, vp, vp, C.c_float] + [vp] * 4
    L.orbfe_enqueue_search_by_projection_sim3.restype = C.c_int
    L.orbfe_enqueue_search_by_projection_sim3.argtypes = [vp, C.POINTER(GridKeyframe), vp, C.c_int, vp, C.c_int] + [vp] * 7 + [C.c_float] + [vp] * 5
    L.orbfe_enqueue_search_by_bow_kf.restype = C.c_int
    L.orbfe_enqueue_search_by_bow_kf.argtypes = [vp, C.POINTER(BowKeyframe), C.POINTER(BowKeyframe), C.c_float, C.c_int] + [vp] * 5
    L.orbfe_enqueue_search_by_bow_kf_batch.restype = C.c_int
    L.orbfe_enqueue_search_by_bow_kf_batch.argtypes = [vp, C.POINTER(BowKeyframe), vp, C.c_int, C.c_int, C.c_float, C.c_int] + [vp] * 5
    L.orbfe_enqueue_triangulate_pairs.restype = C.c_int
    L.orbfe_enqueue_triangulate_pairs.argtypes = [vp, vp, vp, C.c_float, C.c_float, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp]
    L.orbfe_enqueue_find_homography_fundamental.restype = C.c_int
    L.orbfe_enqueue_find_homography_fundamental.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, C.c_float] + [vp] * 10
    L.orbfe_find_homography_fundamental.restype = C.c_int
    L.orbfe_find_homography_fundamental.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_float] + [vp] * 9
    L.orbfe_enqueue_reconstruct_initial.restype = C.c_int
    L.orbfe_enqueue_reconstruct_initial.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int] + [vp] * 7 + [C.c_float, C.c_int, C.c_int] + [vp] * 14
    L.orbfe_reconstruct_initial.restype = C.c_int
    L.orbfe_reconstruct_initial.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int] + [vp] * 7 + [C.c_float, C.c_float, C.c_int, C.c_int] + [vp] * 13
    L.orbfe_enqueue_update_map_points.restype = C.c_int
    L.orbfe_enqueue_update_map_points.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int] + [vp] * 8
    L.orbfe_enqueue_local_bundle_adjustment.restype = C.c_int
    L.orbfe_enqueue_local_bundle_adjustment.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 9
    L.orbfe_local_bundle_adjustment.restype = C.c_int
    L.orbfe_local_bundle_adjustment.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, ip, C.POINTER(LbaInfo)]
    L.orbfe_essential_graph_plan_size.restype = C.c_int
    L.orbfe_essential_graph_plan_size.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_size_t)]
    L.orbfe_essential_graph_plan.restype = C.c_int
    L.orbfe_essential_graph_plan.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.orbfe_enqueue_optimize_essential_graph.restype = C.c_int
    L.orbfe_enqueue_optimize_essential_graph.argtypes = [vp, C.c_int, C.c_int] + [vp] * 8 + [C.c_int, vp, vp, C.c_int, C.c_int, C.c_double, vp, vp, vp, C.c_int] + [vp] * 7
    L.orbfe_optimize_essential_graph.restype = C.c_int
    L.orbfe_optimize_essential_graph.argtypes = [vp, C.c_int, C.c_int] + [vp] * 8 + [C.c_int, C.c_int, C.c_int, C.c_double, vp, vp, vp, C.c_int] + [vp] * 6
    _lib = L
    return L


def essential_graph_plan(n_kfs, fixed_kf, edge_i, edge_j, capacity=None):
    """orbfe_essential_graph_plan (include/orbfe.h): the host-only planner of optimize_essential_graph; needs no GPU.  Returns the blob as
    int32 words (its first 20 are an ESSENTIAL_PLAN_HEADER_DTYPE record).  capacity: bytes offered instead of what the size query says
    (an OrbfeError with ERR_CAPACITY when too few)."""
    L = load()
    ei = np.ascontiguousarray(edge_i, np.int32); ej = np.ascontiguousarray(edge_j, np.int32)
    assert ei.shape == ej.shape and ei.ndim == 1
    n = C.c_size_t()
    pe = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    rc = L.orbfe_essential_graph_plan_size(int(n_kfs), int(fixed_kf), pe(ei), pe(ej), len(ei), C.byref(n))
    if rc != OK:
        raise OrbfeError(rc, "orbfe_essential_graph_plan_size refused n_kfs = %d, fixed_kf = %d" % (n_kfs, fixed_kf))
    cap = n.value if capacity is None else int(capacity)
    blob = np.zeros(max(cap // 4, 1), np.int32)
    rc = L.orbfe_essential_graph_plan(int(n_kfs), int(fixed_kf), pe(ei), pe(ej), len(ei), blob.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    if rc != OK:
        raise OrbfeError(rc, "orbfe_essential_graph_plan: %d bytes offered, %d needed" % (cap, n.value))
    return blob[: n.value // 4]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pnp_iteration_table(capacity, probability=0.99, min_inliers=10, max_its=300, epsilon=0.5):
    """ORB_SLAM2::PnPRansacIterationTable (orbslam2_amd/host/PnPsolver.h): d_its_for_n of enqueue_pnp_ransac_batch, mRansacMaxIts after
    PnPsolver::SetRansacParameters for every N in [0, capacity]; 0 where N < mRansacMinInliers (iterate's bNoMore exit).  The defaults
    are Tracking::Relocalization's."""
    import math
    f32 = np.float32
    out = np.zeros(capacity + 1, np.int32)
    for N in range(capacity + 1):
        n_min = max(int(f32(N) * f32(epsilon)), min_inliers, 4)
        if N < n_min:
            continue
        eps = max(f32(epsilon), f32(n_min) / f32(N))
        n = 1.0
        if n_min != N:
            den = math.log(1 - math.pow(float(eps), 3.0))
            n = math.ceil(math.log(1 - probability) / den) if den != 0 else math.inf
        out[N] = max(1, min(max_its if not n < max_its else int(n), max_its))
    return out


def sim3_iteration_table(max_pairs, probability=0.99, min_inliers=20, max_its=300):
    """ORB_SLAM2::Sim3RansacIterationTable (orbslam2_amd/host/Sim3Solver.h): d_its_for_n of enqueue_sim3_ransac_batch, mRansacMaxIts after
    Sim3Solver::SetRansacParameters for every N in [0, max_pairs]; 0 below min_inliers (iterate's bNoMore exit)."""
    import math
    out = np.zeros(max_pairs + 1, np.int32)
    for N in range(min_inliers, max_pairs + 1):
        n = 1.0
        if N != min_inliers:
            den = math.log(1 - math.pow(float(np.float32(min_inliers) / np.float32(N)), 3))
            n = math.ceil(math.log(1 - probability) / den) if den != 0 else math.inf
        out[N] = max(1, min(max_its if not n < max_its else int(n), max_its))
    return out


def reconstruct_accept(model, cos_parallax, min_parallax):
    """ORB_SLAM2::ReconstructAccept (orbslam2_amd/host/Initializer.h): the parallax test of ReconstructF / ReconstructH on the chosen
    hypothesis's cosine, the one comparison enqueue_reconstruct_initial leaves to the host.  2.0 stands for nGood == 0."""
    f32 = np.float32
    parallax = f32(0) if cos_parallax == 2.0 else f32(np.float64(f32(np.arccos(f32(cos_parallax))) * f32(180)) / np.float64(np.pi))
    return bool(parallax >= f32(min_parallax)) if model == 0 else bool(parallax > f32(min_parallax))


class Context:
    """One device context = one ORBextractor pair / one camera model (include/orbfe.h)."""

    def __init__(self, width, height, nfeatures=2000, scale_factor=1.2, nlevels=8, ini_th_fast=20,
                 min_th_fast=7, patch_size=31, half_patch_size=15, edge_threshold=19,
                 fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, bf=386.1448, device=0, max_images=2):
        self.L = load()
        self.params = Params(nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast, patch_size,
                             half_patch_size, edge_threshold, fx, fy, cx, cy, bf, device, width, height, max_images)
        h = C.c_void_p()
        rc = self.L.orbfe_create(C.byref(self.params), C.byref(h))
        if rc != OK:
            raise OrbfeError(rc, self.L.orbfe_last_error(None).decode())
        self.h = h
        self.width, self.height = width, height
        self.nlevels = nlevels
        self.capacity = self.L.orbfe_keypoint_capacity(self.h)
        self.max_images = max_images

    def close(self):
        if getattr(self, "h", None):
            self.L.orbfe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != OK:
            raise OrbfeError(rc, self.L.orbfe_last_error(self.h).decode())

    # ---- tables (ORBextractor getters) ----
    def tables(self):
        n = self.nlevels
        sc, isc, s2, is2 = (np.zeros(n, np.float32) for _ in range(4))
        feats = np.zeros(n, np.int32)
        umax = np.zeros(self.params.half_patch_size + 1, np.int32)
        self._check(self.L.orbfe_get_tables(self.h, _p(sc), _p(isc), _p(s2), _p(is2), _p(feats), _p(umax)))
        return dict(scale=sc, inv_scale=isc, sigma2=s2, inv_sigma2=is2, features_per_level=feats, umax=umax)

    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        self._check(self.L.orbfe_level_size(self.h, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def blur_ride_from(self, n_images):
        """First pyramid level whose blur rides in FAST's launch for a batch of n_images (nlevels: none)."""
        r = self.L.orbfe_blur_ride_from(self.h, n_images)
        if r < 0:
            raise OrbfeError(r, "orbfe_blur_ride_from")
        return r

    def set_input_retained(self, retained=True):
        """Promise that the images of an enqueue_* call stay valid until the next one (orbfe_fetch_pyramid's level 0 then reads them in place)."""
        self._check(self.L.orbfe_set_input_retained(self.h, int(bool(retained))))

    def set_pattern(self, pattern):
        """Replace the context's copy of the 256 x (x0, y0, x1, y1) rBRIEF tests (ORBextractor::pattern, src/ORBextractor.cc:442-444)."""
        pat = np.ascontiguousarray(np.asarray(pattern, dtype=np.int32).reshape(1024))
        self._check(self.L.orbfe_set_pattern(self.h, _p(pat)))

    def pattern(self):
        pat = np.zeros(1024, np.int32)
        self._check(self.L.orbfe_get_pattern(self.h, _p(pat)))
        return pat.reshape(256, 4)

    # ---- host-image entry points ----
    @staticmethod
    def _rows(a, dtype):
        """Row-strided views (a cv::Mat ROI) go through as they are; anything else is made contiguous.  HxWxC colour
        images (orbfe_set_input_format) must have packed pixels."""
        a = np.asarray(a, dtype)
        if a.ndim == 2 and a.strides[1] == a.itemsize and a.strides[0] >= a.shape[1] * a.itemsize:
            return a
        if a.ndim == 3 and a.strides[2] == a.itemsize and a.strides[1] == a.shape[2] * a.itemsize and a.strides[0] >= a.shape[1] * a.strides[1]:
            return a
        return np.ascontiguousarray(a)

    def set_distortion(self, dist):
        """mDistCoef = k1 k2 p1 p2 [k3] (src/Tracking.cc:67-78); empty: no distortion."""
        d = np.ascontiguousarray(dist, np.float32)
        self._check(self.L.orbfe_set_distortion(self.h, _p(d) if len(d) else None, len(d)))

    def undistort_keypoints(self, kps):
        k = np.ascontiguousarray(kps, KP_DTYPE); out = np.zeros(max(len(k), 1), KP_DTYPE)
        self._check(self.L.orbfe_undistort_keypoints(self.h, _p(k), len(k), _p(out)))
        return out[: len(k)].copy()

    def fetch_keys_un(self, image=0):
        cap = self.capacity
        out = np.zeros(cap, KP_DTYPE); n = C.c_int()
        self._check(self.L.orbfe_fetch_keys_un(self.h, image, _p(out), cap, C.byref(n)))
        return out[: n.value].copy()

    def image_bounds(self):
        b = np.zeros(4, np.float32)
        self._check(self.L.orbfe_image_bounds(self.h, _p(b)))
        return b

    def set_rectification(self, side, map_x=None, map_y=None, src_size=None):
        """cv::remap(raw, map1, map2, INTER_LINEAR) in front of the pipeline (stereo_euroc.cc:136-137); None clears."""
        if map_x is None:
            self._check(self.L.orbfe_set_rectification(self.h, side, None, None, 0, 0))
            return
        mx = np.ascontiguousarray(map_x, np.float32); my = np.ascontiguousarray(map_y, np.float32)
        assert mx.shape == my.shape
        sw, sh = src_size if src_size is not None else (mx.shape[1], mx.shape[0])
        self._check(self.L.orbfe_set_rectification(self.h, side, _p(mx), _p(my), sw, sh))

    def set_input_format(self, channels=1, rgb=True, legacy_weights=False):
        """cv::cvtColor(..., COLOR_{RGB,BGR}[A]2GRAY) of Tracking::GrabImage* folded into ingest (src/Tracking.cc:269-294)."""
        self._check(self.L.orbfe_set_input_format(self.h, channels, int(rgb), int(legacy_weights)))

    def extract(self, img: np.ndarray):
        img = self._rows(img, np.uint8)
        cap = self.capacity
        kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int()
        self._check(self.L.orbfe_extract(self.h, _p(img), img.shape[1], img.shape[0], img.strides[0], _p(kps), _p(desc), cap, C.byref(n)))
        return kps[: n.value].copy(), desc[: n.value].copy()

    def stereo_frame(self, left: np.ndarray, right: np.ndarray):
        left = self._rows(left, np.uint8); right = self._rows(right, np.uint8)
        assert left.shape == right.shape
        if left.strides[0] != right.strides[0]:
            left = np.ascontiguousarray(left); right = np.ascontiguousarray(right)
        cap = self.capacity
        kl = np.zeros(cap, KP_DTYPE); dl = np.zeros((cap, 32), np.uint8)
        kr = np.zeros(cap, KP_DTYPE); dr = np.zeros((cap, 32), np.uint8)
        ur = np.zeros(cap, np.float32); dp = np.zeros(cap, np.float32)
        nl, nr = C.c_int(), C.c_int()
        self._check(self.L.orbfe_stereo_frame(self.h, _p(left), _p(right), left.shape[1], left.shape[0], left.strides[0],
                                              _p(kl), _p(dl), C.byref(nl), _p(kr), _p(dr), C.byref(nr), _p(ur), _p(dp), cap))
        a, b = nl.value, nr.value
        return dict(kps_left=kl[:a].copy(), desc_left=dl[:a].copy(), kps_right=kr[:b].copy(), desc_right=dr[:b].copy(),
                    u_right=ur[:a].copy(), depth=dp[:a].copy())

    def rgbd_frame(self, gray: np.ndarray, depth_img: np.ndarray, depth_map_factor: float = 1.0):
        """depth_img float32: the CV_32F map of Frame::Frame(rgbd).  depth_img uint16: the raw sensor map, converted
        with Tracking's mDepthMapFactor (src/Tracking.cc:323-324) on the device."""
        raw = np.asarray(depth_img).dtype == np.uint16
        gray = self._rows(gray, np.uint8); depth_img = self._rows(depth_img, np.uint16 if raw else np.float32)
        cap = self.capacity
        k = np.zeros(cap, KP_DTYPE); d = np.zeros((cap, 32), np.uint8)
        ur = np.zeros(cap, np.float32); dp = np.zeros(cap, np.float32)
        n = C.c_int()
        if raw:
            self._check(self.L.orbfe_rgbd_frame_u16(self.h, _p(gray), _p(depth_img), float(depth_map_factor), gray.shape[1], gray.shape[0],
                                                    gray.strides[0], depth_img.strides[0], _p(k), _p(d), C.byref(n), _p(ur), _p(dp), cap))
        else:
            self._check(self.L.orbfe_rgbd_frame(self.h, _p(gray), _p(depth_img), gray.shape[1], gray.shape[0], gray.strides[0],
                                                depth_img.strides[0], _p(k), _p(d), C.byref(n), _p(ur), _p(dp), cap))
        m = n.value
        return dict(kps=k[:m].copy(), desc=d[:m].copy(), u_right=ur[:m].copy(), depth=dp[:m].copy())

    # ---- taps ----
    def fetch_pyramid(self, image, level, blurred=False):
        w, h = self.level_size(level)
        out = np.zeros((h, w), np.uint8)
        self._check(self.L.orbfe_fetch_pyramid(self.h, image, level, int(blurred), _p(out), out.strides[0]))
        return out

    def fetch_candidates(self, image, level):
        w, h = self.level_size(level)
        cap = max(16, (w * h) // 4 + 16)
        xs, ys, sc = (np.zeros(cap, np.int32) for _ in range(3))
        n = C.c_int()
        self._check(self.L.orbfe_fetch_candidates(self.h, image, level, _p(xs), _p(ys), _p(sc), cap, C.byref(n)))
        return xs[: n.value].copy(), ys[: n.value].copy(), sc[: n.value].copy()

    # ---- device-resident batched path ----
    def enqueue_extract(self, d_ptr: int, n_images: int, stream: int = 0):
        self._check(self.L.orbfe_enqueue_extract(self.h, C.c_void_p(d_ptr), n_images, C.c_void_p(stream)))

    def enqueue_stereo(self, d_ptr: int, n_pairs: int, stream: int = 0):
        self._check(self.L.orbfe_enqueue_stereo(self.h, C.c_void_p(d_ptr), n_pairs, C.c_void_p(stream)))

    def synchronize(self, stream: int = 0):
        self._check(self.L.orbfe_synchronize(self.h, C.c_void_p(stream)))

    def fetch_batch_async(self, n_images, kps_ptr, desc_ptr, counts_ptr, u_right_ptr, depth_ptr, stream=0):
        """Raw-pointer form (pinned host buffers owned by the caller); see include/orbfe.h."""
        self._check(self.L.orbfe_fetch_batch_async(self.h, n_images, C.c_void_p(kps_ptr), C.c_void_p(desc_ptr), C.c_void_p(counts_ptr),
                                                   C.c_void_p(u_right_ptr), C.c_void_p(depth_ptr), C.c_void_p(stream)))

    def packed_layout(self, n_images, flags=0):
        lay = PackedLayout()
        self._check(self.L.orbfe_get_packed_layout(self.h, n_images, flags, C.byref(lay)))
        return lay

    def fetch_batch_packed(self, n_images, flags, host_ptr, host_bytes, stream=0):
        """Raw-pointer form: one small gather kernel + ONE device-to-host copy of the packed block (include/orbfe.h)."""
        self._check(self.L.orbfe_fetch_batch_packed(self.h, n_images, flags, C.c_void_p(host_ptr), host_bytes, C.c_void_p(stream)))

    def expand_packed(self, block, lay, out_image):
        """cv::KeyPoint records (+ views of descriptors / uRight / depth) of one out image of a fetched block (numpy uint8 array)."""
        k = np.zeros(lay.capacity, KP_DTYPE)
        n = C.c_int()
        self._check(self.L.orbfe_expand_packed(self.h, _p(block), C.byref(lay), out_image, _p(k), lay.capacity, C.byref(n)))
        m, cap = n.value, lay.capacity
        out = dict(kps=k[:m].copy(), desc=block[lay.desc_off + out_image * cap * 32: lay.desc_off + (out_image * cap + m) * 32].reshape(m, 32).copy())
        slot = out_image * (2 if lay.flags & PACK_LEFT_ONLY else 1)
        if (lay.flags & PACK_STEREO) and slot % 2 == 0:
            pr = slot // 2
            out["u_right"] = block[lay.u_right_off + pr * cap * 4: lay.u_right_off + (pr * cap + m) * 4].view(np.float32).copy()
            out["depth"] = block[lay.depth_off + pr * cap * 4: lay.depth_off + (pr * cap + m) * 4].view(np.float32).copy()
        return out

    def fetch_packed(self, n_images, flags=0, stream=0):
        """Blocking convenience for tests: (block, layout) of the latest batched call's results."""
        lay = self.packed_layout(n_images, flags)
        block = np.zeros(lay.bytes, np.uint8)
        self.fetch_batch_packed(n_images, flags, block.ctypes.data, lay.bytes, stream)
        self.synchronize(stream)
        return block, lay

    def enqueue_rgbd(self, gray_ptr, depth_ptr, n_images, depth_is_u16=False, depth_map_factor=1.0, stream=0):
        self._check(self.L.orbfe_enqueue_rgbd(self.h, C.c_void_p(gray_ptr), C.c_void_p(depth_ptr), 1 if depth_is_u16 else 0, depth_map_factor, n_images, C.c_void_p(stream)))

    def fetch_counts(self, n_images):
        c = np.zeros(n_images, np.int32)
        self._check(self.L.orbfe_fetch_counts(self.h, _p(c), n_images))
        return c

    def fetch_image(self, image, stereo=False):
        cap = self.capacity
        k = np.zeros(cap, KP_DTYPE); d = np.zeros((cap, 32), np.uint8)
        ur = np.zeros(cap, np.float32); dp = np.zeros(cap, np.float32)
        n = C.c_int()
        self._check(self.L.orbfe_fetch_image(self.h, image, _p(k), _p(d), _p(ur) if stereo else None,
                                             _p(dp) if stereo else None, cap, C.byref(n)))
        m = n.value
        out = dict(kps=k[:m].copy(), desc=d[:m].copy())
        if stereo:
            out.update(u_right=ur[:m].copy(), depth=dp[:m].copy())
        return out

    def quadtree_kernel(self) -> int:
        return int(self.L.orbfe_quadtree_kernel(self.h))

    def quadtree_plan(self) -> int:
        """0 / 1: bucket-pyramid kernel with node tables in LDS / HBM; 2 / 3: generic kernel with node tables in LDS / HBM"""
        rc = int(self.L.orbfe_quadtree_plan(self.h))
        if rc < 0:
            self._check(rc)
        return rc

    def set_streams(self, groups: int):
        self._check(self.L.orbfe_set_streams(self.h, groups))

    def set_profiling(self, mode):
        """0/False = off, 1/True = events at every stage boundary, 2 + k = only around stage k."""
        self._check(self.L.orbfe_set_profiling(self.h, int(mode)))

    def set_profiling_interval(self, every: int):
        self.L.orbfe_set_profiling_interval.restype = C.c_int
        self.L.orbfe_set_profiling_interval.argtypes = [C.c_void_p, C.c_int]
        self._check(self.L.orbfe_set_profiling_interval(self.h, int(every)))

    def stage_times(self, reset=True):
        """{stage: total ms} over the recorded enqueue calls, and the number of calls."""
        ms = np.zeros(NUM_STAGES, np.float32)
        calls = C.c_int()
        self._check(self.L.orbfe_stage_times(self.h, _p(ms), C.byref(calls), int(reset)))
        names = [self.L.orbfe_stage_name(i).decode() for i in range(NUM_STAGES)]
        return dict(zip(names, ms.tolist())), calls.value

    # ---- Tracking-thread matchers (flattened inputs; see include/orbfe.h) ----
    def _view(self, keys_un, u_right, desc, bounds, device_slot=None, keyframe=False):
        """orbfe_frame_view over host arrays; device_slot = k makes the matchers read image slot k of the latest extraction call
        in HBM instead of uploading the arrays (the host copies are still needed by the host-side accept rules); keyframe: the
        view is a KeyFrame's (windows and the in-image test use the integer-truncated bounds, include/orbfe.h)."""
        k = np.ascontiguousarray(keys_un, KP_DTYPE); d = np.ascontiguousarray(desc, np.uint8)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        fv = FrameView(len(k), _p(k), None if ur is None else _p(ur), _p(d), *[float(b) for b in bounds],
                       0 if device_slot is None else device_slot + 1, 1 if keyframe else 0)
        fv._keep = (k, d, ur)
        return fv

    def features_in_area_batch(self, view, x, y, r, min_level=None, max_level=None):
        """List of index arrays, one per query (Frame::GetFeaturesInArea order)."""
        x = np.ascontiguousarray(x, np.float32); y = np.ascontiguousarray(y, np.float32); r = np.ascontiguousarray(r, np.float32)
        nq = len(x)
        lo = None if min_level is None else np.ascontiguousarray(min_level, np.int32)
        hi = None if max_level is None else np.ascontiguousarray(max_level, np.int32)
        off = np.zeros(nq + 1, np.int32); cap = max(view.n * max(nq, 1), 1)
        out = np.zeros(cap, np.int32)
        self._check(self.L.orbfe_features_in_area_batch(self.h, C.byref(view), nq, _p(x), _p(y), _p(r), None if lo is None else _p(lo),
                                                        None if hi is None else _p(hi), _p(off), _p(out), cap))
        return [out[off[i]:off[i + 1]].copy() for i in range(nq)]

    def features_in_area(self, view, x, y, r, min_level=-1, max_level=-1):
        out = np.zeros(max(view.n, 1), np.int32); n = C.c_int()
        self._check(self.L.orbfe_features_in_area(self.h, C.byref(view), x, y, r, min_level, max_level, _p(out), len(out), C.byref(n)))
        return out[: n.value].copy()

    def search_by_projection_last(self, view, Tcw_cur, Tcw_last, last_pos, last_desc, last_valid, last_obs, last_octave, last_angle,
                                  cur_has_obs, th, mono, check_ori):
        tc = np.ascontiguousarray(Tcw_cur, np.float32); tl = np.ascontiguousarray(Tcw_last, np.float32)
        lp = np.ascontiguousarray(last_pos, np.float32); ld = np.ascontiguousarray(last_desc, np.uint8)
        lv = np.ascontiguousarray(last_valid, np.int32); lo = np.ascontiguousarray(last_obs, np.int32)
        loc = np.ascontiguousarray(last_octave, np.int32); la = np.ascontiguousarray(last_angle, np.float32)
        ho = None if cur_has_obs is None else np.ascontiguousarray(cur_has_obs, np.uint8)
        out = np.zeros(max(view.n, 1), np.int32); nm = C.c_int()
        self._check(self.L.orbfe_search_by_projection_last(self.h, C.byref(view), _p(tc), _p(tl), len(lv), _p(lp), _p(ld), _p(lv), _p(lo),
                                                           _p(loc), _p(la), None if ho is None else _p(ho), th, int(mono), int(check_ori),
                                                           _p(out), C.byref(nm)))
        return out[: view.n].copy(), nm.value

    def is_in_frustum(self, Tcw, bounds, pos, normal, max_distance, min_distance, viewing_cos_limit):
        tc = np.ascontiguousarray(Tcw, np.float32); pos = np.ascontiguousarray(pos, np.float32); nr = np.ascontiguousarray(normal, np.float32)
        mx = np.ascontiguousarray(max_distance, np.float32); mn = np.ascontiguousarray(min_distance, np.float32)
        out = np.zeros(len(pos), TP_DTYPE)
        self._check(self.L.orbfe_is_in_frustum(self.h, _p(tc), bounds[0], bounds[1], bounds[2], bounds[3], len(pos), _p(pos), _p(nr), _p(mx),
                                               _p(mn), viewing_cos_limit, _p(out)))
        return out

    def search_by_projection_points(self, view, pts, pt_desc, pt_obs, cur_has_obs, th, nnratio):
        pts = np.ascontiguousarray(pts, TP_DTYPE); pd = np.ascontiguousarray(pt_desc, np.uint8); po = np.ascontiguousarray(pt_obs, np.int32)
        ho = None if cur_has_obs is None else np.ascontiguousarray(cur_has_obs, np.uint8)
        out = np.zeros(max(view.n, 1), np.int32); nm = C.c_int()
        self._check(self.L.orbfe_search_by_projection_points(self.h, C.byref(view), len(pts), _p(pts), _p(pd), _p(po),
                                                             None if ho is None else _p(ho), th, nnratio, _p(out), C.byref(nm)))
        return out[: view.n].copy(), nm.value

    # ---- the same on device-resident data, asynchronous (integer device pointers and a stream; see include/orbfe.h) ----
    def enqueue_search_by_projection_last(self, slot, bounds, d_Tcw_cur, d_Tcw_last, n_last, d_last_pos, d_last_desc, d_last_valid, d_last_obs,
                                          d_last_octave, d_last_angle, d_cur_has_obs, th, mono, check_ori, d_cur_match, d_nmatches, d_status,
                                          d_has_point=0, d_Xw=0, stream=0):
        b = np.ascontiguousarray(bounds, np.float32)
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_search_by_projection_last(
            self.h, slot, _p(b), v(d_Tcw_cur), v(d_Tcw_last), n_last, v(d_last_pos), v(d_last_desc), v(d_last_valid), v(d_last_obs), v(d_last_octave),
            v(d_last_angle), v(d_cur_has_obs or None), th, int(mono), int(check_ori), v(d_cur_match), v(d_nmatches), v(d_status),
            v(d_has_point or None), v(d_Xw or None), v(stream or None)))

    def enqueue_is_in_frustum(self, d_Tcw, bounds, n, d_pos, d_normal, d_max_distance, d_min_distance, viewing_cos_limit, d_out, stream=0):
        """d_out: n orbfe_track_point records (TP_DTYPE, 24 bytes each)."""
        b = np.ascontiguousarray(bounds, np.float32)
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_is_in_frustum(self.h, v(d_Tcw), _p(b), n, v(d_pos), v(d_normal), v(d_max_distance), v(d_min_distance),
                                                       viewing_cos_limit, v(d_out), v(stream or None)))

    def enqueue_search_by_projection_points(self, slot, bounds, n_pts, d_pts, d_pt_desc, d_pt_obs, d_pt_pos, d_cur_has_obs, th, nnratio,
                                            d_cur_match, d_nmatches, d_status, d_has_point=0, d_Xw=0, stream=0):
        b = np.ascontiguousarray(bounds, np.float32)
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_search_by_projection_points(
            self.h, slot, _p(b), n_pts, v(d_pts), v(d_pt_desc), v(d_pt_obs), v(d_pt_pos or None), v(d_cur_has_obs or None), th, nnratio,
            v(d_cur_match), v(d_nmatches), v(d_status), v(d_has_point or None), v(d_Xw or None), v(stream or None)))

    def enqueue_search_by_projection_kf(self, slot, bounds, d_Tcw, n_kf, d_kf_pos, d_kf_desc, d_kf_valid, d_kf_angle, d_kf_max_distance,
                                        d_kf_min_distance, d_cur_point, d_outlier, th, orb_dist, check_ori, exclude_held, d_cur_match,
                                        d_nmatches, d_status, d_has_point=0, d_Xw=0, stream=0):
        """SearchByProjection(CurrentFrame, KeyFrame, sAlreadyFound, th, ORBdist) on image slot `slot`, asynchronous: d_cur_point
        (int32[capacity], in/out) is the keyframe index whose map point each keypoint holds; see include/orbfe.h."""
        b = np.ascontiguousarray(bounds, np.float32)
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_search_by_projection_kf(
            self.h, slot, _p(b), v(d_Tcw or None), n_kf, v(d_kf_pos or None), v(d_kf_desc or None), v(d_kf_valid or None), v(d_kf_angle or None),
            v(d_kf_max_distance or None), v(d_kf_min_distance or None), v(d_cur_point or None), v(d_outlier or None), th, int(orb_dist),
            int(check_ori), int(exclude_held), v(d_cur_match or None), v(d_nmatches or None), v(d_status or None), v(d_has_point or None),
            v(d_Xw or None), v(stream or None)))

    def enqueue_search_by_projection_kf_batch(self, slot, bounds, d_cands, n_cands, max_n_kf, check_ori, exclude_held, d_cur_match, d_nmatches,
                                              d_status, d_has_point=0, d_Xw=0, stream=0):
        """enqueue_search_by_projection_kf for n_cands candidates at once (Relocalization): d_cands is a device array of
        RelocCandidate records, max_n_kf an upper bound of their n; the outputs hold one row per candidate."""
        b = np.ascontiguousarray(bounds, np.float32)
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_search_by_projection_kf_batch(
            self.h, slot, _p(b), v(d_cands or None), n_cands, max_n_kf, int(check_ori), int(exclude_held), v(d_cur_match or None),
            v(d_nmatches or None), v(d_status or None), v(d_has_point or None), v(d_Xw or None), v(stream or None)))

    def device_keys_un(self, slot, stream=0) -> int:
        """Device pointer to mvKeysUn of image slot `slot` (orbfe_keypoint records) for enqueue_pose_optimization."""
        out = C.c_void_p()
        self._check(self.L.orbfe_device_keys_un(self.h, slot, C.byref(out), C.c_void_p(stream or None)))
        return out.value or 0

    def enqueue_compute_bow(self, slot, level, d_words, d_word_w, d_n_words, d_nodes, d_node_off, d_node_feat, d_n_nodes, d_status,
                            d_word_id=0, d_weight=0, d_node_id=0, stream=0):
        """Frame::ComputeFboW of image slot `slot` (needs bow.vocab_load): fBow and fBow2 as device arrays of `capacity` entries
        (d_node_off: capacity + 1), the counts and the status as one int32 each; the per-feature arrays are optional."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_compute_bow(
            self.h, slot, level, v(d_word_id or None), v(d_weight or None), v(d_node_id or None), v(d_words), v(d_word_w), v(d_n_words),
            v(d_nodes), v(d_node_off), v(d_node_feat), v(d_n_nodes), v(d_status), v(stream or None)))

    def enqueue_search_by_bow(self, slot, d_kf_nodes, d_kf_off, d_kf_feat, kf_nnodes, d_kf_valid, d_kf_desc, d_kf_angle, n_kf,
                              d_f_nodes, d_f_off, d_f_feat, d_f_n_nodes, nnratio, check_ori, d_f_match, d_nmatches, d_status,
                              d_kf_pos=0, d_has_point=0, d_Xw=0, stream=0):
        """ORBmatcher::SearchByFboW(KeyFrame*, Frame&) against image slot `slot`, whose feature vector enqueue_compute_bow wrote."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_search_by_bow(
            self.h, slot, v(d_kf_nodes or None), v(d_kf_off or None), v(d_kf_feat or None), kf_nnodes, v(d_kf_valid or None), v(d_kf_desc or None),
            v(d_kf_angle or None), n_kf, v(d_kf_pos or None), v(d_f_nodes), v(d_f_off), v(d_f_feat), v(d_f_n_nodes), nnratio, int(check_ori),
            v(d_f_match), v(d_nmatches), v(d_status), v(d_has_point or None), v(d_Xw or None), v(stream or None)))

    def enqueue_search_by_bow_batch(self, slot, d_kfs, n_kfs, max_kf_nnodes, d_f_nodes, d_f_off, d_f_feat, d_f_n_nodes, nnratio, check_ori,
                                    d_f_match, d_nmatches, d_status, d_has_point=0, d_Xw=0, stream=0):
        """enqueue_search_by_bow against n_kfs keyframes at once (Relocalization): d_kfs is a device array of BowKeyframe records,
        max_kf_nnodes an upper bound of their nnodes; the outputs hold one row per keyframe."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_search_by_bow_batch(
            self.h, slot, v(d_kfs or None), n_kfs, max_kf_nnodes, v(d_f_nodes), v(d_f_off), v(d_f_feat), v(d_f_n_nodes), nnratio, int(check_ori),
            v(d_f_match), v(d_nmatches), v(d_status), v(d_has_point or None), v(d_Xw or None), v(stream or None)))

    def enqueue_search_by_bow_kf(self, kf1, kf2, nnratio, check_ori, d_match12, d_nmatches, d_status, d_pairs=0, stream=0):
        """ORBmatcher::SearchByFboW(KeyFrame*, KeyFrame*) on two device-resident keyframes (BowKeyframe records on the host, device
        pointers inside; None passes as a NULL record), asynchronous on `stream`: d_match12[kf1.n], the optional d_pairs[2 * kf1.n]
        ((idx1, idx2) in ascending idx1), the count and the status as one int32 each."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_search_by_bow_kf(
            self.h, None if kf1 is None else C.byref(kf1), None if kf2 is None else C.byref(kf2), nnratio, int(check_ori),
            v(d_match12 or None), v(d_pairs or None), v(d_nmatches or None), v(d_status or None), v(stream or None)))

    def enqueue_search_by_bow_kf_batch(self, kf1, d_kfs, n_kfs, max_kf_n, nnratio, check_ori, d_match12, d_nmatches, d_status, d_pairs=0, stream=0):
        """enqueue_search_by_bow_kf of kf1 against n_kfs keyframes at once (LoopClosing::ComputeSim3): d_kfs is a device array of
        BowKeyframe records, max_kf_n an upper bound of their n; the outputs hold one row per candidate (d_match12[n_kfs][kf1.n],
        d_pairs[n_kfs][2 * kf1.n], d_nmatches[n_kfs], d_status[n_kfs])."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_search_by_bow_kf_batch(
            self.h, None if kf1 is None else C.byref(kf1), v(d_kfs or None), n_kfs, max_kf_n, nnratio, int(check_ori),
            v(d_match12 or None), v(d_pairs or None), v(d_nmatches or None), v(d_status or None), v(stream or None)))

    def enqueue_search_for_triangulation(self, kf1, kf2, F12, Cw1, T2w, fx2, fy2, cx2, cy2, only_stereo, check_ori,
                                         d_match12, d_nmatches, d_status, d_pairs=0, stream=0):
        """ORBmatcher::SearchForTriangulation on two device-resident keyframes (TriKeyframe records on the host, device pointers inside),
        asynchronous on `stream`.  F12 (3x3), Cw1 (3), T2w (3x4) are host arrays read before the call returns.  One call per neighbour:
        kf1.has_mp changes on the stream between two calls (CreateNewMapPoints adds points in between): enqueue_triangulate_pairs sets it,
        or the caller patches it."""
        v = C.c_void_p
        f = np.ascontiguousarray(F12, np.float32); c = np.ascontiguousarray(Cw1, np.float32); t = np.ascontiguousarray(T2w, np.float32)
        assert f.size == 9 and c.size == 3 and t.size == 12
        self._check(self.L.orbfe_enqueue_search_for_triangulation(
            self.h, C.byref(kf1), C.byref(kf2), _p(f), _p(c), _p(t), fx2, fy2, cx2, cy2, int(only_stereo), int(check_ori),
            v(d_match12 or None), v(d_pairs or None), v(d_nmatches or None), v(d_status or None), v(stream or None)))

    def enqueue_keyframe_grid(self, d_keys_un, n, bounds, d_cell_off, d_cell_idx, stream=0):
        """Frame::AssignFeaturesToGrid for a keyframe's n device-resident keypoints: d_cell_off (int32[GRID_CELLS + 1]) and d_cell_idx
        (int32[n]) are arrays the caller keeps for the keyframe's life (GridKeyframe.cell_off / cell_idx); bounds: the frame's floats."""
        b = np.ascontiguousarray(bounds, np.float32)
        assert b.size == 4
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_keyframe_grid(self.h, v(d_keys_un or None), n, _p(b), v(d_cell_off or None), v(d_cell_idx or None),
                                                       v(stream or None)))

    def _enqueue_fuse(self, fn, kf, pose, n_pts, d_pt_index, n_rows, d_pos, d_normal, d_max_distance, d_min_distance, d_pt_desc, d_pt_valid, th,
                      d_best_idx, d_n_fused, d_status, stream):
        v = C.c_void_p
        t = np.ascontiguousarray(pose, np.float32)
        assert t.size >= 12
        self._check(fn(self.h, C.byref(kf), _p(t), n_pts, v(d_pt_index or None), n_rows, v(d_pos or None), v(d_normal or None),
                       v(d_max_distance or None), v(d_min_distance or None), v(d_pt_desc or None), v(d_pt_valid or None), th, v(d_best_idx or None),
                       v(d_n_fused or None), v(d_status or None), v(stream or None)))

    def enqueue_fuse(self, kf, Tcw, n_pts, d_pt_index, n_rows, d_pos, d_normal, d_max_distance, d_min_distance, d_pt_desc, d_pt_valid, th,
                     d_best_idx, d_n_fused, d_status, stream=0):
        """Search part of ORBmatcher::Fuse(pKF, vpMapPoints, th) on a device-resident keyframe (a GridKeyframe record on the host, device
        pointers inside), asynchronous on `stream`.  Tcw (3x4) is a host array read before the call returns.  The map points are a table
        of n_rows rows in HBM; query q reads row d_pt_index[q] (0: row q) and its own d_pt_valid[q].  One call per target keyframe: the
        caller patches d_pt_valid (and descriptor rows that MapPoint::Replace recomputed) on the stream between two calls."""
        self._enqueue_fuse(self.L.orbfe_enqueue_fuse, kf, Tcw, n_pts, d_pt_index, n_rows, d_pos, d_normal, d_max_distance, d_min_distance, d_pt_desc,
                           d_pt_valid, th, d_best_idx, d_n_fused, d_status, stream)

    def enqueue_fuse_sim3(self, kf, Scw, n_pts, d_pt_index, n_rows, d_pos, d_normal, d_max_distance, d_min_distance, d_pt_desc, d_pt_valid, th,
                          d_best_idx, d_n_fused, d_status, stream=0):
        """The same for ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) of LoopClosing::SearchAndFuse: Scw = [sR | s t] (3x4, host)."""
        self._enqueue_fuse(self.L.orbfe_enqueue_fuse_sim3, kf, Scw, n_pts, d_pt_index, n_rows, d_pos, d_normal, d_max_distance, d_min_distance,
                           d_pt_desc, d_pt_valid, th, d_best_idx, d_n_fused, d_status, stream)

    def enqueue_update_map_points(self, d_kfs, n_kfs, n_upd, d_row, n_rows, d_obs_off, d_obs_kf, d_obs_idx, n_obs, d_ref, what, d_pos, d_normal,
                                  d_max_distance, d_min_distance, d_pt_desc, d_best, d_status, stream=0):
        """MapPoint::ComputeDistinctiveDescriptors (what & MP_DESCRIPTOR) and MapPoint::UpdateNormalAndDepth (what & MP_NORMAL_DEPTH) for
        n_upd rows of the map-point table in HBM, asynchronous on `stream`.  d_kfs: device array of n_kfs ObsKeyframe records; update q
        rewrites row d_row[q] (0: row q) from the observations d_obs_off[q] .. d_obs_off[q + 1] - 1 of d_obs_kf / d_obs_idx, given in
        the order of the reference's mObservations; d_ref[q] is the position of mpRefKF's entry inside that list.  d_best (0: not
        wanted) receives the list position of the chosen descriptor, or -1.  Every argument but the counts is a raw device pointer."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_update_map_points(
            self.h, v(d_kfs or None), n_kfs, n_upd, v(d_row or None), n_rows, v(d_obs_off or None), v(d_obs_kf or None), v(d_obs_idx or None), n_obs,
            v(d_ref or None), what, v(d_pos or None), v(d_normal or None), v(d_max_distance or None), v(d_min_distance or None), v(d_pt_desc or None),
            v(d_best or None), v(d_status or None), v(stream or None)))

    def enqueue_triangulate_pairs(self, kf1, kf2, mbf, ratio_factor, d_pairs, d_npairs, max_pairs, d_code, d_x3d, d_new, d_nnew, d_status,
                                  d_pos=0, n_rows=0, d_rows_used=0, patch_has_mp=1, stream=0):
        """The triangulation stage of LocalMapping::CreateNewMapPoints for the pairs enqueue_search_for_triangulation left in HBM
        (d_pairs, and d_npairs read on the device; max_pairs bounds it), asynchronous on `stream`.  kf1 / kf2: NewpointKeyframe records on
        the host (None passes as a NULL record).  d_code[max_pairs] (uint8; a point is created iff <= 2), d_x3d[max_pairs][3],
        d_new[3 * max_pairs] = (idx1, idx2, row) of the created pairs in pair order, d_nnew[1], d_status[1]; with d_pos the positions
        are appended to the table from row *d_rows_used on (a device counter, advanced); patch_has_mp sets has_mp of both keyframes."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_triangulate_pairs(
            self.h, None if kf1 is None else C.byref(kf1), None if kf2 is None else C.byref(kf2), mbf, ratio_factor, v(d_pairs or None),
            v(d_npairs or None), max_pairs, v(d_code or None), v(d_x3d or None), v(d_new or None), v(d_nnew or None), v(d_pos or None), n_rows,
            v(d_rows_used or None), int(patch_has_mp), v(d_status or None), v(stream or None)))

    def enqueue_find_homography_fundamental(self, d_keys1_un, n1, d_keys2_un, n2, d_pairs, n_matches, d_sets, iterations, norm1, norm2, sigma,
                                            d_H21, d_F21, d_score, d_best, d_status, d_inliers_h=0, d_inliers_f=0, d_ninliers=0, d_all_scores=0,
                                            stream=0):
        """Initializer::FindHomography + FindFundamental for one frame pair, every hypothesis of both models, asynchronous on `stream`.
        d_pairs[n_matches][2] = mvMatches12, d_sets[iterations][8] = mvSets; norm1 / norm2 = (meanX, meanY, sX, sY) of Normalize on the
        host (four floats each, None passes as NULL), read before the call returns.  d_H21[9], d_F21[9], d_score[2], d_best[2] (the
        winning iteration or -1), d_status[1]; optional d_inliers_h / d_inliers_f[n_matches], d_ninliers[2], d_all_scores[2][iterations].
        The per-hypothesis scratch is the context's: queue the calls of one context on one stream."""
        v = C.c_void_p
        nm = [None if n is None else (C.c_float * 4)(*[float(x) for x in n]) for n in (norm1, norm2)]
        self._check(self.L.orbfe_enqueue_find_homography_fundamental(
            self.h, v(d_keys1_un or None), n1, v(d_keys2_un or None), n2, v(d_pairs or None), n_matches, v(d_sets or None), iterations, nm[0], nm[1],
            sigma, v(d_H21 or None), v(d_F21 or None), v(d_score or None), v(d_best or None), v(d_inliers_h or None), v(d_inliers_f or None),
            v(d_ninliers or None), v(d_all_scores or None), v(d_status or None), v(stream or None)))

    def find_homography_fundamental(self, keys1_un, keys2_un, matches12, sets, sigma=1.0):
        """The same from host arrays, synchronous: keys*_un KP_DTYPE arrays, matches12 int32[n1] (vMatches12, < 0 = none), sets
        int32[iterations][8].  Returns dict(H21, F21 (3x3, zeros without a winner), score[2], best[2], inliers_h, inliers_f (uint8[N]),
        ninliers[2], all_scores[2][iterations], n_matches)."""
        k1, k2 = np.ascontiguousarray(keys1_un, KP_DTYPE), np.ascontiguousarray(keys2_un, KP_DTYPE)
        m = np.ascontiguousarray(matches12, np.int32)
        st = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
        assert len(m) == len(k1)
        H, F = np.zeros(9, np.float32), np.zeros(9, np.float32)
        score, best, nin = np.zeros(2, np.float32), np.zeros(2, np.int32), np.zeros(2, np.int32)
        ih, jf = np.zeros(max(len(k1), 1), np.uint8), np.zeros(max(len(k1), 1), np.uint8)
        scores = np.zeros((2, len(st)), np.float32)
        n = C.c_int32(0)
        self._check(self.L.orbfe_find_homography_fundamental(self.h, _p(k1), len(k1), _p(k2), len(k2), _p(m), _p(st), len(st), sigma, _p(H), _p(F),
                                                             _p(score), _p(best), _p(ih), _p(jf), _p(nin), _p(scores), C.byref(n)))
        return dict(H21=H.reshape(3, 3), F21=F.reshape(3, 3), score=score, best=best, inliers_h=ih[:n.value], inliers_f=jf[:n.value], ninliers=nin,
                    all_scores=scores, n_matches=n.value)

    def enqueue_reconstruct_initial(self, d_keys1_un, n1, d_keys2_un, n2, d_pairs, n_matches, d_H21, d_F21, d_score, d_best, d_inliers_h, d_inliers_f, K,
                                    sigma, d_model, d_hyp_R, d_hyp_t, d_ngood, d_cos_parallax, d_result, d_choice, d_R21, d_t21, d_p3d, d_triangulated,
                                    d_status, d_codes=0, min_triangulated=50, model=-1, stream=0):
        """Initializer::ReconstructF / ReconstructH (with DecomposeE and CheckRT) on the outputs of enqueue_find_homography_fundamental
        where they lie in HBM, asynchronous on `stream`.  K = (fx, fy, cx, cy) on the host (None passes as NULL), read before the call
        returns; model -1 takes the RH decision on the device, 0 / 1 force H / F.  d_model[1], d_hyp_R[8][9], d_hyp_t[8][3], d_ngood[8],
        d_cos_parallax[8], d_result[1] (0 chosen, 1 no RANSAC winner, 2 the singular-value test, 3 the count rules refuse), d_choice[1],
        d_R21[9], d_t21[3], d_p3d[n1][3], d_triangulated[n1], d_status[1]; optional d_codes[8][n_matches].  The parallax test stays
        with the caller: reconstruct_accept(model, cos_parallax[choice], min_parallax).  The scratch is the context's: queue the calls
        of one context on one stream."""
        v = C.c_void_p
        k = None if K is None else (C.c_float * 4)(*[float(x) for x in K])
        self._check(self.L.orbfe_enqueue_reconstruct_initial(
            self.h, v(d_keys1_un or None), n1, v(d_keys2_un or None), n2, v(d_pairs or None), n_matches, v(d_H21 or None), v(d_F21 or None),
            v(d_score or None), v(d_best or None), v(d_inliers_h or None), v(d_inliers_f or None), k, sigma, min_triangulated, model, v(d_model or None),
            v(d_hyp_R or None), v(d_hyp_t or None), v(d_ngood or None), v(d_cos_parallax or None), v(d_result or None), v(d_choice or None),
            v(d_R21 or None), v(d_t21 or None), v(d_p3d or None), v(d_triangulated or None), v(d_codes or None), v(d_status or None), v(stream or None)))

    def reconstruct_initial(self, keys1_un, keys2_un, pairs, H21, F21, score, best, inliers_h, inliers_f, K, sigma=1.0, min_parallax=1.0,
                            min_triangulated=50, model=-1, codes=True):
        """The same from host arrays, synchronous: pairs int32[N][2] (mvMatches12) and the RANSAC call's outputs.  Returns dict(ok (the
        reference's bool, the parallax test applied with min_parallax), model, hyp_R[8][9], hyp_t[8][3] (zeros where untouched), ngood[8],
        cos_parallax[8], result, choice, R21 (3x3), t21 (zeros without a choice), p3d[n1][3], triangulated[n1], codes[8][N] or None)."""
        k1, k2 = np.ascontiguousarray(keys1_un, KP_DTYPE), np.ascontiguousarray(keys2_un, KP_DTYPE)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        f32 = lambda a, n: np.ascontiguousarray(a, np.float32).reshape(n)
        H, F, sc, bs = f32(H21, 9), f32(F21, 9), f32(score, 2), np.ascontiguousarray(best, np.int32).reshape(2)
        ih, jf = np.ascontiguousarray(inliers_h, np.uint8), np.ascontiguousarray(inliers_f, np.uint8)
        assert len(ih) == len(pr) and len(jf) == len(pr)
        kk = f32(K, 4)
        hyp_R, hyp_t, R21, t21 = np.zeros((8, 9), np.float32), np.zeros((8, 3), np.float32), np.zeros(9, np.float32), np.zeros(3, np.float32)
        ngood, cosp = np.zeros(8, np.int32), np.zeros(8, np.float32)
        p3d, tri = np.zeros((max(len(k1), 1), 3), np.float32), np.zeros(max(len(k1), 1), np.uint8)
        cd = np.zeros((8, len(pr)), np.uint8) if codes else None
        m, res, ch, ok = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int(0)
        self._check(self.L.orbfe_reconstruct_initial(self.h, _p(k1), len(k1), _p(k2), len(k2), _p(pr), len(pr), _p(H), _p(F), _p(sc), _p(bs), _p(ih), _p(jf), _p(kk),
                                                     sigma, min_parallax, min_triangulated, model, C.byref(m), _p(hyp_R), _p(hyp_t), _p(ngood), _p(cosp), C.byref(res),
                                                     C.byref(ch), _p(R21), _p(t21), _p(p3d), _p(tri), None if cd is None else _p(cd), C.byref(ok)))
        return dict(ok=bool(ok.value), model=m.value, hyp_R=hyp_R, hyp_t=hyp_t, ngood=ngood, cos_parallax=cosp, result=res.value, choice=ch.value,
                    R21=R21.reshape(3, 3), t21=t21, p3d=p3d[:len(k1)], triangulated=tri[:len(k1)], codes=cd)

    def enqueue_search_by_sim3(self, kf1, T1w, d_pts1, kf2, T2w, d_pts2, s12, R12, t12, th, d_match12, d_n_found, d_status, stream=0):
        """ORBmatcher::SearchBySim3 on two device-resident keyframes (GridKeyframe records on the host, device pointers inside),
        asynchronous on `stream`.  d_pts = (d_pos, d_max_distance, d_min_distance, d_pt_desc, d_valid), one entry per keypoint slot, as
        search_by_sim3's pts.  T1w, T2w (3x4), R12 (3x3) and t12 (3) are host arrays read before the call returns.  d_match12 holds
        kf1.n entries.  The one-way results live in the context's scratch: queue the calls of one context on one stream."""
        v = C.c_void_p
        t1 = np.ascontiguousarray(T1w, np.float32); t2 = np.ascontiguousarray(T2w, np.float32)
        R = np.ascontiguousarray(R12, np.float32); t = np.ascontiguousarray(t12, np.float32)
        assert t1.size >= 12 and t2.size >= 12 and R.size == 9 and t.size == 3 and len(d_pts1) == 5 and len(d_pts2) == 5
        self._check(self.L.orbfe_enqueue_search_by_sim3(self.h, C.byref(kf1), _p(t1), *[v(x or None) for x in d_pts1], C.byref(kf2), _p(t2),
                                                        *[v(x or None) for x in d_pts2], float(s12), _p(R), _p(t), th, v(d_match12 or None),
                                                        v(d_n_found or None), v(d_status or None), v(stream or None)))

    def enqueue_optimize_sim3(self, kf1, T1w, d_pos1, d_valid1, kf2, T2w, d_pos2, d_valid2, s12, R12, t12, th2, fix_scale, d_match12, d_S12,
                              d_n_inliers, d_status, d_prior12=0, params=None, stream=0):
        """Optimizer::OptimizeSim3 on two device-resident keyframes (GridKeyframe records on the host; only keys_un and n are read),
        asynchronous on `stream`.  d_pos / d_valid: the map point's position and pMP && !isBad() per keypoint slot; d_match12 (int32
        [kf1.n], in/out) is what enqueue_search_by_sim3 wrote, d_prior12 (optional) the RANSAC inliers' matches as slots of kf2; T1w,
        T2w (3x4), R12 (3x3), t12 (3) are host arrays read before the call returns.  d_S12 receives 8 doubles (qx qy qz qw tx ty tz s).
        params: a Sim3OptParams or None for the reference's values.  Queue the calls of one context on one stream."""
        v = C.c_void_p
        t1 = np.ascontiguousarray(T1w, np.float32); t2 = np.ascontiguousarray(T2w, np.float32)
        R = np.ascontiguousarray(R12, np.float32); t = np.ascontiguousarray(t12, np.float32)
        assert t1.size >= 12 and t2.size >= 12 and R.size == 9 and t.size == 3
        self._check(self.L.orbfe_enqueue_optimize_sim3(self.h, C.byref(kf1), _p(t1), v(d_pos1 or None), v(d_valid1 or None), C.byref(kf2), _p(t2),
                                                       v(d_pos2 or None), v(d_valid2 or None), float(s12), _p(R), _p(t), float(th2), int(fix_scale),
                                                       None if params is None else C.byref(params), v(d_prior12 or None), v(d_match12 or None),
                                                       v(d_S12 or None), v(d_n_inliers or None), v(d_status or None), v(stream or None)))

    def enqueue_local_bundle_adjustment(self, d_kfs, d_role, n_kfs, max_free_kfs, d_Tcw, n_pts, d_row, n_rows, d_obs_off, d_obs_kf, d_obs_idx, n_obs,
                                        d_pos, d_obs_kfs, d_edge_code, d_edge_chi2, d_erase, d_n_erase, d_info, d_status, stream=0):
        """Optimizer::LocalBundleAdjustment on device-resident keyframes and the map-point table (include/orbfe.h), asynchronous on
        `stream`.  d_kfs: a device array of BaKeyframe; d_role: uint8[n_kfs] of BA_*; max_free_kfs: a host bound on the BA_LOCAL ones;
        the point list, rows and CSR are enqueue_update_map_points'; d_Tcw float32[n_kfs][16] and d_pos are rewritten in place;
        d_obs_kfs (0: none) is the ObsKeyframe directory whose Ow is patched; d_info receives one LBA_INFO_DTYPE record.  Every
        argument is a device address.  Queue the calls of one context on one stream."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_local_bundle_adjustment(
            self.h, v(d_kfs or None), v(d_role or None), n_kfs, max_free_kfs, v(d_Tcw or None), n_pts, v(d_row or None), n_rows, v(d_obs_off or None),
            v(d_obs_kf or None), v(d_obs_idx or None), n_obs, *[v(x or None) for x in (d_pos, d_obs_kfs, d_edge_code, d_edge_chi2, d_erase, d_n_erase,
                                                                                       d_info, d_status, stream)]))

    def local_bundle_adjustment(self, keyframes, role, Tcw, row, n_rows, obs_off, obs_kf, obs_idx, pos):
        """The same from host arrays, synchronous.  keyframes: a sequence of (keys_un KP_DTYPE[n], u_right float32[n]); row may be None.
        Returns a dict: Tcw float32[n_kfs][16], pos float32[n_rows][3], Ow float32[n_kfs][3] (NaN rows for keyframes that were not
        rewritten), edge_code uint8[n_obs], edge_chi2 float64[n_obs], erase int32[n_erase][2], info (an LBA_INFO_DTYPE record), status
        (0, or ERR_INVALID / ERR_CAPACITY as the device set it: the outputs are written all the same, so this form does not raise then)."""
        ks = [np.ascontiguousarray(k, KP_DTYPE) for k, _ in keyframes]
        us = [np.ascontiguousarray(u, np.float32) for _, u in keyframes]
        n_kfs = len(ks)
        assert all(len(k) == len(u) for k, u in zip(ks, us))
        kp = (C.c_void_p * max(n_kfs, 1))(*[k.ctypes.data if k.size else None for k in ks])
        up = (C.c_void_p * max(n_kfs, 1))(*[u.ctypes.data if u.size else None for u in us])
        kn = np.array([len(k) for k in ks], np.int32)
        ro = np.ascontiguousarray(role, np.uint8)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16).copy()
        po = np.ascontiguousarray(pos, np.float32).reshape(-1, 3).copy()
        off = np.ascontiguousarray(obs_off, np.int32); okf = np.ascontiguousarray(obs_kf, np.int32); oidx = np.ascontiguousarray(obs_idx, np.int32)
        rw = None if row is None else np.ascontiguousarray(row, np.int32)
        n_pts, n_obs = max(len(off) - 1, 0), len(okf)
        assert len(ro) == n_kfs and len(T) == n_kfs and len(oidx) == n_obs and len(po) == n_rows and (rw is None or len(rw) == n_pts)
        Ow = np.full((n_kfs, 3), np.nan, np.float32)
        code = np.zeros(n_obs, np.uint8); chi = np.zeros(n_obs, np.float64); erase = np.zeros((n_obs, 2), np.int32)
        n_erase = C.c_int(); info = LbaInfo()
        ptr = lambda a: _p(a) if a is not None and a.size else None
        rc = self.L.orbfe_local_bundle_adjustment(self.h, kp, up, ptr(kn), ptr(ro), n_kfs, ptr(T), n_pts, ptr(rw), n_rows, ptr(off), ptr(okf), ptr(oidx),
                                                  n_obs, ptr(po), ptr(Ow), ptr(code), ptr(chi), ptr(erase), C.byref(n_erase), C.byref(info))
        if rc not in (OK, ERR_INVALID, ERR_CAPACITY):   # the asserts above leave the call itself nothing to refuse: these two are the device's
            self._check(rc)
        return dict(Tcw=T, pos=po, Ow=Ow, edge_code=code, edge_chi2=chi, erase=erase[:n_erase.value].copy(),
                    info=np.frombuffer(bytes(info), LBA_INFO_DTYPE)[0], status=rc)

    def enqueue_optimize_essential_graph(self, n_kfs, fixed_kf, d_Tcw, d_corrected, d_has_corrected, d_noncorrected, d_has_noncorrected, d_edge_i, d_edge_j,
                                         d_edge_kind, n_edges, d_plan, plan_header, iterations, fix_scale, lambda_init, d_pos, d_pt_ref, d_pt_valid, n_pts,
                                         d_obs_kfs, d_edge_code, d_pt_code, d_sim3_out, d_info, d_status, stream=0):
        """Optimizer::OptimizeEssentialGraph on device-resident keyframes and the position column (include/orbfe.h), asynchronous on
        `stream`.  d_plan: essential_graph_plan()'s blob in HBM; plan_header: the blob itself or its first 20 words, on the host.  Every
        other d_ argument is a device address (0: none, where the header allows it); d_info receives one EG_INFO_DTYPE record."""
        v = C.c_void_p
        hdr = np.ascontiguousarray(np.asarray(plan_header).view(np.int32).reshape(-1)[:20])
        self._check(self.L.orbfe_enqueue_optimize_essential_graph(
            self.h, n_kfs, fixed_kf, *[v(x or None) for x in (d_Tcw, d_corrected, d_has_corrected, d_noncorrected, d_has_noncorrected, d_edge_i, d_edge_j,
                                                             d_edge_kind)], n_edges, v(d_plan or None), _p(hdr), int(iterations), int(fix_scale),
            float(lambda_init), v(d_pos or None), v(d_pt_ref or None), v(d_pt_valid or None), n_pts,
            *[v(x or None) for x in (d_obs_kfs, d_edge_code, d_pt_code, d_sim3_out, d_info, d_status, stream)]))

    def optimize_essential_graph(self, fixed_kf, Tcw, edge_i, edge_j, edge_kind, corrected=None, has_corrected=None, noncorrected=None,
                                 has_noncorrected=None, iterations=20, fix_scale=False, lambda_init=EG_LAMBDA_INIT, pos=None, pt_ref=None, pt_valid=None):
        """The same from host arrays, synchronous (it plans, uploads, enqueues and downloads).  Returns a dict: Tcw float32[n_kfs][16],
        pos float32[n_pts][3], Ow float32[n_kfs][3], sim3 float64[n_kfs][8] (the final estimates), edge_code uint8[n_edges], pt_code
        uint8[n_pts], info (an EG_INFO_DTYPE record), status (0 or ERR_INVALID, as the device set it)."""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16).copy()
        n_kfs = len(T)
        ei = np.ascontiguousarray(edge_i, np.int32); ej = np.ascontiguousarray(edge_j, np.int32); ek = np.ascontiguousarray(edge_kind, np.uint8)
        assert len(ei) == len(ej) == len(ek)
        tab = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).reshape(n_kfs, 8)
        flg = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8).reshape(n_kfs)
        co, hc, no, hn = tab(corrected), flg(has_corrected), tab(noncorrected), flg(has_noncorrected)
        po = np.zeros((0, 3), np.float32) if pos is None else np.ascontiguousarray(pos, np.float32).reshape(-1, 3).copy()
        n_pts = len(po)
        pr = np.zeros(0, np.int32) if pt_ref is None else np.ascontiguousarray(pt_ref, np.int32)
        pv = np.zeros(0, np.uint8) if pt_valid is None else np.ascontiguousarray(pt_valid, np.uint8)
        assert len(pr) == n_pts and len(pv) == n_pts
        Ow = np.zeros((n_kfs, 3), np.float32); sim3 = np.zeros((n_kfs, 8), np.float64)
        ecode = np.zeros(len(ei), np.uint8); pcode = np.zeros(n_pts, np.uint8)
        info = np.zeros(1, EG_INFO_DTYPE); status = np.zeros(1, np.int32)
        ptr = lambda a: _p(a) if a is not None and a.size else None
        self._check(self.L.orbfe_optimize_essential_graph(
            self.h, n_kfs, int(fixed_kf), ptr(T), ptr(co), ptr(hc), ptr(no), ptr(hn), ptr(ei), ptr(ej), ptr(ek), len(ei), int(iterations), int(fix_scale),
            float(lambda_init), ptr(po), ptr(pr), ptr(pv), n_pts, ptr(Ow), ptr(ecode), ptr(pcode), ptr(sim3), ptr(info), ptr(status)))
        return dict(Tcw=T, pos=po, Ow=Ow, sim3=sim3, edge_code=ecode, pt_code=pcode, info=info[0], status=int(status[0]))

    def enqueue_sim3_ransac_batch(self, kf1, T1w, d_pos1, d_valid1, d_cands, n_cands, max_pairs, max_kf_n, fix_scale, min_inliers, max_its, d_its_for_n,
                                  d_n_corr, d_n_its, d_corr, d_sets, d_hyp, d_inlier_bits, d_events, d_n_events, d_status, stream=0):
        """Sim3Solver for all candidates of LoopClosing::ComputeSim3 in one call (include/orbfe.h), asynchronous on `stream`.  kf1: a
        GridKeyframe record on the host (keys_un and n are read), T1w a host 3x4; d_cands: a device array of Sim3RansacCandidate;
        d_its_for_n: sim3_iteration_table() in HBM.  Every output is a device address; d_sets may be 0."""
        v = C.c_void_p
        t1 = np.ascontiguousarray(T1w, np.float32)
        assert t1.size >= 12
        self._check(self.L.orbfe_enqueue_sim3_ransac_batch(
            self.h, C.byref(kf1) if kf1 is not None else None, _p(t1), v(d_pos1 or None), v(d_valid1 or None), v(d_cands or None), n_cands, max_pairs, max_kf_n,
            int(fix_scale), min_inliers, max_its, *[v(x or None) for x in (d_its_for_n, d_n_corr, d_n_its, d_corr, d_sets, d_hyp, d_inlier_bits, d_events,
                                                                           d_n_events, d_status, stream)]))

    def enqueue_sim3_ransac_select(self, d_cands, n_cands, c, k, kf1_n, d_valid1, max_pairs, max_kf_n, max_its, d_n_corr, d_n_its, d_corr, d_inlier_bits,
                                   d_prior12, d_valid1_round, d_valid2_round, d_status, stream=0):
        """What the round of candidate c at iteration k hands to enqueue_search_by_sim3 and enqueue_optimize_sim3, written on `stream`
        from the rows enqueue_sim3_ransac_batch left in HBM: d_prior12, d_valid1_round [kf1_n], d_valid2_round [max_kf_n]."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_sim3_ransac_select(
            self.h, v(d_cands or None), n_cands, c, k, kf1_n, v(d_valid1 or None), max_pairs, max_kf_n, max_its,
            *[v(x or None) for x in (d_n_corr, d_n_its, d_corr, d_inlier_bits, d_prior12, d_valid1_round, d_valid2_round, d_status, stream)]))

    def sim3_ransac(self, keys_un1, T1w, pos1, valid1, keys_un2, T2w, pos2, valid2, pairs, draws, fix_scale, min_inliers, max_its, its_for_n):
        """enqueue_sim3_ransac_batch from host arrays for one candidate, synchronous; max_pairs = max(len(pairs), 1).  Returns a dict of
        the candidate's rows.  Raises OrbfeError (ERR_INVALID) for what only the device can see."""
        k1 = np.ascontiguousarray(keys_un1, KP_DTYPE); k2 = np.ascontiguousarray(keys_un2, KP_DTYPE)
        t1 = np.ascontiguousarray(T1w, np.float32); t2 = np.ascontiguousarray(T2w, np.float32)
        p1 = np.ascontiguousarray(pos1, np.float32); p2 = np.ascontiguousarray(pos2, np.float32)
        v1 = np.ascontiguousarray(valid1, np.int32); v2 = np.ascontiguousarray(valid2, np.int32)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2); dr = np.ascontiguousarray(draws, np.uint32)
        tab = np.ascontiguousarray(its_for_n, np.int32)
        assert t1.size >= 12 and t2.size >= 12 and dr.size >= 3 * max_its and tab.size >= len(pr) + 1
        mp = max(len(pr), 1)
        out = dict(corr=np.zeros((mp, 2), np.int32), sets=np.zeros((max_its, 3), np.int32), hyp=np.zeros(max_its, SIM3_HYP_DTYPE),
                   bits=np.zeros((max_its, (mp + 31) // 32), np.uint32), events=np.zeros(max_its, np.int32))
        n_corr, n_its, n_ev = C.c_int(), C.c_int(), C.c_int()
        ptr = lambda a: _p(a) if a.size else None
        self._check(self.L.orbfe_sim3_ransac(self.h, ptr(k1), len(k1), _p(t1), ptr(p1), ptr(v1), ptr(k2), len(k2), _p(t2), ptr(p2), ptr(v2), ptr(pr), len(pr),
                                             _p(dr), int(fix_scale), min_inliers, max_its, _p(tab), C.byref(n_corr), C.byref(n_its), _p(out["corr"]),
                                             _p(out["sets"]), _p(out["hyp"]), _p(out["bits"]), _p(out["events"]), C.byref(n_ev)))
        out.update(n_corr=n_corr.value, n_its=n_its.value, n_events=n_ev.value, status=0)
        return out

    def enqueue_pnp_ransac_batch(self, slot, d_cands, n_cands, max_kf_n, min_inliers, max_its, n_iterations, epsilon, th2, d_its_for_n, d_n_corr, d_n_its,
                                 d_corr, d_sets, d_hyp, d_inlier_bits, d_refined, d_refined_bits, d_events, d_n_events, d_exhausted, d_status, min_set=4, stream=0):
        """PnPsolver for all candidates of Tracking::Relocalization in one call (include/orbfe.h), asynchronous on `stream`.  The frame is
        image slot `slot`; d_cands: a device array of PnPCandidate; d_its_for_n: pnp_iteration_table(capacity) in HBM.  Every output is a
        device address; d_sets may be 0."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_pnp_ransac_batch(
            self.h, slot, v(d_cands or None), n_cands, max_kf_n, min_set, min_inliers, max_its, n_iterations, float(epsilon), float(th2),
            *[v(x or None) for x in (d_its_for_n, d_n_corr, d_n_its, d_corr, d_sets, d_hyp, d_inlier_bits, d_refined, d_refined_bits, d_events, d_n_events,
                                     d_exhausted, d_status, stream)]))

    def enqueue_pnp_ransac_select(self, slot, n_cands, c, which, k, max_its, d_n_corr, d_n_its, d_corr, d_hyp, d_inlier_bits, d_refined, d_refined_bits,
                                  d_exhausted, d_Tcw_row, d_cur_point_row, d_has_point_row, d_status, stream=0):
        """What candidate c's first pose optimisation reads, written on `stream` from the rows enqueue_pnp_ransac_batch left in HBM:
        which = PNP_EVENT: the refined pose and inliers of iteration k's record holder; PNP_EXHAUSTED: the best hypothesis's."""
        v = C.c_void_p
        self._check(self.L.orbfe_enqueue_pnp_ransac_select(
            self.h, slot, n_cands, c, which, k, max_its,
            *[v(x or None) for x in (d_n_corr, d_n_its, d_corr, d_hyp, d_inlier_bits, d_refined, d_refined_bits, d_exhausted, d_Tcw_row, d_cur_point_row,
                                     d_has_point_row, d_status, stream)]))

    def pnp_ransac(self, keys_un, f_match, pos, valid, draws, min_inliers, max_its, n_iterations, epsilon, th2, its_for_n, min_set=4):
        """enqueue_pnp_ransac_batch from host arrays for one candidate, synchronous; capacity = max(len(keys_un), 1).  Returns a dict of
        the candidate's rows.  Raises OrbfeError (ERR_INVALID) for what only the device can see."""
        k = np.ascontiguousarray(keys_un, KP_DTYPE); fm = np.ascontiguousarray(f_match, np.int32)
        p = np.ascontiguousarray(pos, np.float32); va = np.ascontiguousarray(valid, np.int32)
        dr = np.ascontiguousarray(draws, np.uint32); tab = np.ascontiguousarray(its_for_n, np.int32)
        assert len(fm) == len(k) and p.size == 3 * len(va) and dr.size >= 4 * max_its and tab.size >= len(k) + 1
        cap = max(len(k), 1)
        words = (cap + 31) // 32
        out = dict(corr=np.zeros((cap, 2), np.int32), sets=np.zeros((max_its, 4), np.int32), hyp=np.zeros(max_its, PNP_HYP_DTYPE),
                   bits=np.zeros((max_its, words), np.uint32), refined=np.zeros(max_its, PNP_REFINED_DTYPE),
                   refined_bits=np.zeros((max_its, words), np.uint32), events=np.zeros(max_its, np.int32))
        n_corr, n_its, n_ev, exh = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        ptr = lambda a: _p(a) if a.size else None
        self._check(self.L.orbfe_pnp_ransac(self.h, ptr(k), len(k), ptr(fm), ptr(p), ptr(va), len(va), _p(dr), min_set, min_inliers, max_its, n_iterations,
                                            float(epsilon), float(th2), _p(tab), C.byref(n_corr), C.byref(n_its), _p(out["corr"]), _p(out["sets"]), _p(out["hyp"]),
                                            _p(out["bits"]), _p(out["refined"]), _p(out["refined_bits"]), _p(out["events"]), C.byref(n_ev), C.byref(exh)))
        out.update(n_corr=n_corr.value, n_its=n_its.value, n_events=n_ev.value, exhausted=exh.value, status=0)
        return out

    def optimize_sim3(self, keys_un1, T1w, pos1, valid1, keys_un2, T2w, pos2, valid2, s12, R12, t12, th2, fix_scale, match12, prior12=None,
                      params=None):
        """The same from host arrays, synchronous.  Returns (S12 float64[8], match12 int32[n1], n_inliers).  Raises OrbfeError
        (ERR_INVALID) for what only the device can see -- an entry outside [-1, n2), an octave outside the context's levels."""
        k1 = np.ascontiguousarray(keys_un1, KP_DTYPE); k2 = np.ascontiguousarray(keys_un2, KP_DTYPE)
        t1 = np.ascontiguousarray(T1w, np.float32); t2 = np.ascontiguousarray(T2w, np.float32)
        p1 = np.ascontiguousarray(pos1, np.float32); p2 = np.ascontiguousarray(pos2, np.float32)
        v1 = np.ascontiguousarray(valid1, np.int32); v2 = np.ascontiguousarray(valid2, np.int32)
        R = np.ascontiguousarray(R12, np.float32); t = np.ascontiguousarray(t12, np.float32)
        m = np.ascontiguousarray(match12, np.int32).copy()
        pr = None if prior12 is None else np.ascontiguousarray(prior12, np.int32)
        assert t1.size >= 12 and t2.size >= 12 and R.size == 9 and t.size == 3 and len(m) == len(k1) and (pr is None or len(pr) == len(k1))
        S = np.zeros(8, np.float64); n = C.c_int()
        ptr = lambda a: _p(a) if a.size else None
        self._check(self.L.orbfe_optimize_sim3(self.h, ptr(k1), len(k1), _p(t1), ptr(p1), ptr(v1), ptr(k2), len(k2), _p(t2), ptr(p2), ptr(v2), float(s12),
                                               _p(R), _p(t), float(th2), int(fix_scale), None if params is None else C.byref(params),
                                               None if pr is None else ptr(pr), ptr(m), _p(S), C.byref(n)))
        return S, m, n.value

    def enqueue_search_by_projection_sim3(self, kf, Scw, n_pts, d_pt_index, n_rows, d_pos, d_normal, d_max_distance, d_min_distance, d_pt_desc,
                                          d_pt_valid, d_kf_matched, th, d_pt_match, d_kf_match, d_nmatches, d_status, stream=0):
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) of LoopClosing::ComputeSim3 on a device-resident keyframe,
        asynchronous on `stream`.  The point table, the index list and the per-query validity are enqueue_fuse_sim3's; d_kf_matched
        (uint8[kf.n], 0: none) marks the keypoints matched on entry.  d_pt_match[n_pts] and d_kf_match[kf.n] are exact inverses.  Uses
        the context's query scratch: queue the calls of one context on one stream."""
        v = C.c_void_p
        t = np.ascontiguousarray(Scw, np.float32)
        assert t.size >= 12
        self._check(self.L.orbfe_enqueue_search_by_projection_sim3(
            self.h, C.byref(kf), _p(t), n_pts, v(d_pt_index or None), n_rows, v(d_pos or None), v(d_normal or None), v(d_max_distance or None),
            v(d_min_distance or None), v(d_pt_desc or None), v(d_pt_valid or None), v(d_kf_matched or None), th, v(d_pt_match or None),
            v(d_kf_match or None), v(d_nmatches or None), v(d_status or None), v(stream or None)))

    def search_by_projection_kf(self, view, Tcw_cur, kf_pos, kf_desc, kf_valid, kf_angle, kf_max_distance, kf_min_distance, cur_has_point,
                                th, orb_dist, check_ori):
        tc = np.ascontiguousarray(Tcw_cur, np.float32); kp = np.ascontiguousarray(kf_pos, np.float32)
        kd = np.ascontiguousarray(kf_desc, np.uint8); kv = np.ascontiguousarray(kf_valid, np.int32); ka = np.ascontiguousarray(kf_angle, np.float32)
        kmx = np.ascontiguousarray(kf_max_distance, np.float32); kmn = np.ascontiguousarray(kf_min_distance, np.float32)
        hp = None if cur_has_point is None else np.ascontiguousarray(cur_has_point, np.uint8)
        out = np.zeros(max(view.n, 1), np.int32); nm = C.c_int()
        self._check(self.L.orbfe_search_by_projection_kf(self.h, C.byref(view), _p(tc), len(kv), _p(kp), _p(kd), _p(kv), _p(ka), _p(kmx), _p(kmn),
                                                         None if hp is None else _p(hp), th, orb_dist, int(check_ori), _p(out), C.byref(nm)))
        return out[: view.n].copy(), nm.value

    def fuse(self, view, Tcw, pos, normal, max_distance, min_distance, pt_desc, pt_valid, th):
        """Search part of ORBmatcher::Fuse(KeyFrame*, vpMapPoints, th): best keypoint per map point (-1: none), and the count."""
        t = np.ascontiguousarray(Tcw, np.float32); p = np.ascontiguousarray(pos, np.float32); nrm = np.ascontiguousarray(normal, np.float32)
        mx = np.ascontiguousarray(max_distance, np.float32); mn = np.ascontiguousarray(min_distance, np.float32)
        d = np.ascontiguousarray(pt_desc, np.uint8); ok = np.ascontiguousarray(pt_valid, np.int32)
        out = np.zeros(max(len(ok), 1), np.int32); nf = C.c_int()
        self._check(self.L.orbfe_fuse(self.h, C.byref(view), _p(t), len(ok), _p(p), _p(nrm), _p(mx), _p(mn), _p(d), _p(ok), th, _p(out), C.byref(nf)))
        return out[: len(ok)].copy(), nf.value

    def sim3_projection(self, mode, view, Scw, pos, normal, max_distance, min_distance, pt_desc, pt_valid, kf_matched, th):
        """mode 0: SearchByProjection(KeyFrame*, Scw, ...); mode 1: search part of Fuse(KeyFrame*, Scw, ...): (match per point, count)."""
        t = np.ascontiguousarray(Scw, np.float32); p = np.ascontiguousarray(pos, np.float32); nrm = np.ascontiguousarray(normal, np.float32)
        mx = np.ascontiguousarray(max_distance, np.float32); mn = np.ascontiguousarray(min_distance, np.float32)
        d = np.ascontiguousarray(pt_desc, np.uint8); ok = np.ascontiguousarray(pt_valid, np.int32)
        out = np.zeros(max(len(ok), 1), np.int32); nf = C.c_int()
        if mode == 0:
            km = None if kf_matched is None else np.ascontiguousarray(kf_matched, np.uint8)
            self._check(self.L.orbfe_search_by_projection_sim3(self.h, C.byref(view), _p(t), len(ok), _p(p), _p(nrm), _p(mx), _p(mn), _p(d), _p(ok),
                                                               None if km is None else _p(km), th, _p(out), C.byref(nf)))
        else:
            self._check(self.L.orbfe_fuse_sim3(self.h, C.byref(view), _p(t), len(ok), _p(p), _p(nrm), _p(mx), _p(mn), _p(d), _p(ok), th, _p(out), C.byref(nf)))
        return out[: len(ok)].copy(), nf.value

    def search_by_sim3(self, view1, T1w, pts1, view2, T2w, pts2, s12, R12, t12, th):
        """ORBmatcher::SearchBySim3; pts = (pos, max_distance, min_distance, desc, valid) per keypoint slot.  (match12, count)."""
        def prep(T, pts):
            pos, mx, mn, d, ok = pts
            return (np.ascontiguousarray(T, np.float32), np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(mx, np.float32),
                    np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(d, np.uint8), np.ascontiguousarray(ok, np.int32))
        a, b = prep(T1w, pts1), prep(T2w, pts2)
        R = np.ascontiguousarray(R12, np.float32); t = np.ascontiguousarray(t12, np.float32)
        out = np.zeros(max(view1.n, 1), np.int32); nf = C.c_int()
        self._check(self.L.orbfe_search_by_sim3(self.h, C.byref(view1), *[_p(x) for x in a], C.byref(view2), *[_p(x) for x in b],
                                                float(s12), _p(R), _p(t), th, _p(out), C.byref(nf)))
        return out[: view1.n].copy(), nf.value

    def pose_optimization(self, Tcw, keys_un, u_right, has_point, Xw, outlier=None):
        """Optimizer::PoseOptimization (src/Optimizer.cc:283-495).  Returns (Tcw 4x4 float32, outlier uint8[N], n_inliers)."""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(4, 4).copy()
        k = np.ascontiguousarray(keys_un, KP_DTYPE); ur = np.ascontiguousarray(u_right, np.float32)
        hp = np.ascontiguousarray(has_point, np.uint8); X = np.ascontiguousarray(Xw, np.float32)
        out = np.zeros(max(len(k), 1), np.uint8) if outlier is None else np.ascontiguousarray(outlier, np.uint8).copy()
        n = C.c_int()
        self._check(self.L.orbfe_pose_optimization(self.h, _p(T), len(k), _p(k), _p(ur), _p(hp), _p(X), _p(out), C.byref(n)))
        return T, out[: len(k)].copy(), n.value

    def pose_optimization_batch(self, Tcw, offsets, keys_un, u_right, has_point, Xw, outlier=None):
        """One problem per slice offsets[k]:offsets[k+1].  Returns (Tcw [P,4,4], outlier, n_inliers int32[P])."""
        off = np.ascontiguousarray(offsets, np.int32); P = len(off) - 1
        T = np.ascontiguousarray(Tcw, np.float32).reshape(P, 4, 4).copy()
        k = np.ascontiguousarray(keys_un, KP_DTYPE); ur = np.ascontiguousarray(u_right, np.float32)
        hp = np.ascontiguousarray(has_point, np.uint8); X = np.ascontiguousarray(Xw, np.float32)
        out = np.zeros(max(len(k), 1), np.uint8) if outlier is None else np.ascontiguousarray(outlier, np.uint8).copy()
        n = np.zeros(max(P, 1), np.int32)
        self._check(self.L.orbfe_pose_optimization_batch(self.h, P, _p(off), _p(T), _p(k), _p(ur), _p(hp), _p(X), _p(out), _p(n)))
        return T, out[: len(k)].copy(), n[:P].copy()

    def search_for_initialization(self, view1, view2, prev_matched, window_size, nnratio, check_ori):
        pm = np.ascontiguousarray(prev_matched, np.float32).copy()
        out = np.zeros(max(view1.n, 1), np.int32); nm = C.c_int()
        self._check(self.L.orbfe_search_for_initialization(self.h, C.byref(view1), C.byref(view2), _p(pm), window_size, nnratio,
                                                           int(check_ori), _p(out), C.byref(nm)))
        return out[: view1.n].copy(), pm, nm.value

    def hamming_matrix(self, a: np.ndarray, b: np.ndarray):
        a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
        out = np.zeros((len(a), len(b)), np.int32)
        self._check(self.L.orbfe_hamming_matrix(self.h, _p(a), len(a), _p(b), len(b), _p(out)))
        return out


# ---- PNG input (orbfe_png_*): no context, no GPU ----
def png_info(data: bytes):
    """(width, height, channels, bit_depth) cv::imread(..., IMREAD_UNCHANGED) would return for this PNG file."""
    L = load()
    buf = np.frombuffer(data, np.uint8)
    w, h, ch, bd = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    rc = L.orbfe_png_info(_p(buf), len(buf), C.byref(w), C.byref(h), C.byref(ch), C.byref(bd))
    if rc != OK:
        L.orbfe_png_last_error.restype = C.c_char_p
        raise OrbfeError(rc, L.orbfe_png_last_error().decode())
    return w.value, h.value, ch.value, bd.value


def png_decode(data: bytes) -> np.ndarray:
    """cv::imread(path, IMREAD_UNCHANGED) of a PNG file held in memory: HxW or HxWxC array, uint8 or uint16."""
    L = load()
    w, h, ch, bd = png_info(data)
    out = np.zeros((h, w, ch), np.uint16 if bd == 16 else np.uint8)
    buf = np.frombuffer(data, np.uint8)
    L.orbfe_png_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t] + [C.POINTER(C.c_int)] * 4
    rc = L.orbfe_png_decode(_p(buf), len(buf), _p(out), out.nbytes, 0, None, None, None, None)
    if rc != OK:
        L.orbfe_png_last_error.restype = C.c_char_p
        raise OrbfeError(rc, L.orbfe_png_last_error().decode())
    return out[:, :, 0] if ch == 1 else out


def png_decode_batch(files, width, height, channels=1, bit_depth=8, threads=0, out=None) -> np.ndarray:
    """n PNG files of one geometry -> [n, H, W(, C)] array (optionally a caller buffer, e.g. pinned memory)."""
    L = load()
    n = len(files)
    shape = (n, height, width) if channels == 1 else (n, height, width, channels)
    if out is None:
        out = np.zeros(shape, np.uint16 if bit_depth == 16 else np.uint8)
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    sizes = (C.c_size_t * max(n, 1))(*[len(b) for b in bufs])
    L.orbfe_png_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t] + [C.c_int] * 5
    rc = L.orbfe_png_decode_batch(ptrs, sizes, n, _p(out), out.nbytes // max(n, 1), width, height, channels, bit_depth, threads)
    if rc != OK:
        L.orbfe_png_last_error.restype = C.c_char_p
        raise OrbfeError(rc, L.orbfe_png_last_error().decode())
    return out
