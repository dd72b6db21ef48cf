"""Python binding of libslamit_hip.so (the C-ABI of include/slamit.h) — used by tests and bench.py.

The classes keep the reference's names and argument meaning:
  ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)   include/ORBextractor.h:50-57
  ORBmatcher.DescriptorDistance / best2 / TH_LOW / TH_HIGH              include/ORBmatcher.h:41-89
  Optimizer.LocalBundleAdjustment                                        include/Optimizer.h:45
There is NO CPU fallback: if the library is missing or no GPU is usable every call raises.
"""
import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SLAMIT_LIB", os.path.join(HERE, "libslamit_hip.so"))  # override only for diagnostic builds

KP_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
     ("octave", "<i4"), ("class_id", "<i4")]
)

MAX_ITS = 32


class SlamitError(RuntimeError):
    pass


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("max_batch", C.c_int32)]


class BaProblem(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_pt", C.c_int32), ("n_edge", C.c_int32),
                ("kf_pose", C.c_void_p), ("kf_fixed", C.c_void_p), ("kf_intr", C.c_void_p),
                ("pt_xyz", C.c_void_p), ("edge_kf", C.c_void_p), ("edge_pt", C.c_void_p),
                ("edge_uv", C.c_void_p), ("edge_inv_sigma2", C.c_void_p),
                ("edge_ur", C.c_void_p), ("kf_bf", C.c_void_p)]   # stereo observations: both NULL for a monocular window


class BaOpts(C.Structure):
    _fields_ = [("its_robust", C.c_int32), ("its_final", C.c_int32), ("huber_delta", C.c_double),
                ("chi2_gate", C.c_double), ("stop", C.c_void_p),
                ("huber_delta_stereo", C.c_double), ("chi2_gate_stereo", C.c_double)]   # 0: the reference's sqrt(7.815) / 7.815


class BaStats(C.Structure):
    _fields_ = [("n_its", C.c_int32 * 2), ("chi2", (C.c_double * MAX_ITS) * 2),
                ("lambda_", (C.c_double * MAX_ITS) * 2), ("trials", (C.c_int32 * MAX_ITS) * 2),
                ("chi2_init", C.c_double * 2)]


class BaResult(C.Structure):
    _fields_ = [("kf_pose", C.c_void_p), ("pt_xyz", C.c_void_p), ("edge_chi2", C.c_void_p),
                ("edge_outlier", C.c_void_p), ("edge_stage1_outlier", C.c_void_p), ("stats", C.c_void_p)]


class FrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("kp_xy", C.c_void_p), ("kp_octave", C.c_void_p), ("desc", C.c_void_p),
                ("kp_taken", C.c_void_p), ("min_x", C.c_float), ("min_y", C.c_float), ("inv_w", C.c_float),
                ("inv_h", C.c_float)]


class SearchQueries(C.Structure):
    _fields_ = [("m", C.c_int32), ("uvr", C.c_void_p), ("level_min", C.c_void_p), ("level_max", C.c_void_p),
                ("desc", C.c_void_p), ("valid", C.c_void_p), ("takes", C.c_void_p)]


class SearchRule(C.Structure):
    _fields_ = [("th_dist", C.c_int32), ("use_ratio", C.c_int32), ("nnratio", C.c_float), ("chi2_gate", C.c_float),
                ("inv_level_sigma2", C.c_float * 16), ("mode", C.c_int32)]


SEARCH_ER_NONE, SEARCH_ER_RADIUS, SEARCH_ER_CHI2 = 0, 1, 2   # SLAMIT_SEARCH_ER_*


class SearchStereo(C.Structure):
    _fields_ = [("er_mode", C.c_int32), ("chi2_gate_stereo", C.c_float), ("kp_ur", C.c_void_p), ("q_ur", C.c_void_p),
                ("q_ur_stride", C.c_int32)]


class SearchStereoDev(C.Structure):
    _fields_ = [("er_mode", C.c_int32), ("chi2_gate_stereo", C.c_float), ("d_kp_ur", C.c_void_p), ("d_q_ur", C.c_void_p),
                ("q_ur_stride", C.c_int32)]


def _search_rule(th_dist, use_ratio, nnratio, chi2_gate=0.0, inv_level_sigma2=None, mode=0):
    sig = [1.0] * 16
    if inv_level_sigma2 is not None:
        for i, v in enumerate(list(inv_level_sigma2)[:16]):
            sig[i] = float(v)
    return SearchRule(int(th_dist), int(bool(use_ratio)), float(nnratio), float(chi2_gate), (C.c_float * 16)(*sig), int(mode))


class BowGroups(C.Structure):
    _fields_ = [("n_groups", C.c_int32), ("q_ptr", C.c_void_p), ("q_idx", C.c_void_p), ("c_ptr", C.c_void_p), ("c_idx", C.c_void_p)]


class BowRule(C.Structure):
    _fields_ = [("mode", C.c_int32), ("th", C.c_int32), ("th_inclusive", C.c_int32), ("nnratio", C.c_float),
                ("F12", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float), ("kp1_xy", C.c_void_p), ("kp2_xy", C.c_void_p),
                ("kp2_octave", C.c_void_p), ("scale_factor", C.c_float * 16), ("level_sigma2", C.c_float * 16)]


class Sim3Problem(C.Structure):
    _fields_ = [("n", C.c_int32), ("p1", C.c_void_p), ("p2", C.c_void_p), ("obs1", C.c_void_p), ("obs2", C.c_void_p),
                ("inv_sigma2_1", C.c_void_p), ("inv_sigma2_2", C.c_void_p), ("intr1", C.c_double * 4), ("intr2", C.c_double * 4),
                ("r12", C.c_double * 9), ("t12", C.c_double * 3), ("s12", C.c_double), ("th2", C.c_double), ("fix_scale", C.c_int32)]


class Sim3Result(C.Structure):
    _fields_ = [("r12", C.c_double * 9), ("t12", C.c_double * 3), ("s12", C.c_double), ("inlier", C.c_void_p), ("n_inliers", C.c_int32),
                ("n_its", C.c_int32 * 2), ("chi2", C.c_double * 2)]


class Sim3RansacProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("x1", C.c_void_p), ("x2", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p),
                ("intr1", C.c_float * 4), ("intr2", C.c_float * 4), ("fix_scale", C.c_int32), ("n_hyp", C.c_int32), ("triples", C.c_void_p)]


class Sim3RansacResult(C.Structure):
    _fields_ = [("t12", C.c_void_p), ("n_inliers", C.c_void_p), ("inlier_bits", C.c_void_p)]


SIM3_RANSAC_MAX_N, SIM3_RANSAC_MAX_HYP = 8192, 1024   # SLAMIT_SIM3_RANSAC_MAX_N / _MAX_HYP


class PnpProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("p3d", C.c_void_p), ("p2d", C.c_void_p), ("max_err", C.c_void_p), ("intr", C.c_double * 4),
                ("n_hyp", C.c_int32), ("quads", C.c_void_p)]


class PnpResult(C.Structure):
    _fields_ = [("pose", C.c_void_p), ("n_inliers", C.c_void_p), ("inlier_bits", C.c_void_p)]


class PnpRefineProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("p3d", C.c_void_p), ("p2d", C.c_void_p), ("max_err", C.c_void_p), ("intr", C.c_double * 4),
                ("subset_bits", C.c_void_p)]


class PnpRefineResult(C.Structure):
    _fields_ = [("pose", C.c_double * 12), ("n_inliers", C.c_int32), ("inlier_bits", C.c_void_p)]


PNP_MAX_N, PNP_MAX_HYP = 8192, 1024   # SLAMIT_PNP_MAX_N / _MAX_HYP


class InitProblem(C.Structure):
    _fields_ = [("n1", C.c_int32), ("keys1", C.c_void_p), ("n2", C.c_int32), ("keys2", C.c_void_p), ("n", C.c_int32), ("matches", C.c_void_p),
                ("sigma", C.c_float), ("n_hyp", C.c_int32), ("sets", C.c_void_p)]


class InitResult(C.Structure):
    _fields_ = [("model", C.c_void_p), ("score", C.c_void_p), ("n_inliers", C.c_void_p), ("inlier_bits", C.c_void_p)]


class InitReconstructProblem(C.Structure):
    _fields_ = [("n1", C.c_int32), ("keys1", C.c_void_p), ("n2", C.c_int32), ("keys2", C.c_void_p), ("n", C.c_int32), ("matches", C.c_void_p),
                ("sigma", C.c_float), ("kind", C.c_int32), ("model", C.c_float * 9), ("K", C.c_float * 9), ("subset_bits", C.c_void_p)]


class InitReconstructResult(C.Structure):
    _fields_ = [("decomposable", C.c_int32), ("n_motions", C.c_int32), ("R", C.c_float * 72), ("t", C.c_float * 24), ("n_good", C.c_int32 * 8),
                ("cos_sel", C.c_float * 8), ("status", C.c_void_p), ("points", C.c_void_p), ("good_bits", C.c_void_p)]


INIT_MAX_N, INIT_MAX_HYP, INIT_H, INIT_F = 8192, 1024, 0, 1   # SLAMIT_INIT_MAX_N / _MAX_HYP / _H / _F


class TriangulateProblem(C.Structure):
    _fields_ = [("Tcw1", C.c_float * 12), ("Tcw2", C.c_float * 12), ("intr1", C.c_float * 6), ("intr2", C.c_float * 6), ("n", C.c_int32),
                ("n_levels", C.c_int32), ("kp1_xy", C.c_void_p), ("kp2_xy", C.c_void_p), ("octave1", C.c_void_p), ("octave2", C.c_void_p),
                ("scale_factors1", C.c_void_p), ("level_sigma2_1", C.c_void_p), ("scale_factors2", C.c_void_p), ("level_sigma2_2", C.c_void_p),
                ("ratio_factor", C.c_float)]


class TriangulateResult(C.Structure):
    _fields_ = [("status", C.c_void_p), ("x3d", C.c_void_p), ("n_accepted", C.c_int32)]


class TriangulateStereo(C.Structure):   # struct slamit_triangulate_stereo
    _fields_ = [("ur1", C.c_void_p), ("ur2", C.c_void_p), ("depth1", C.c_void_p), ("depth2", C.c_void_p), ("raw1_xy", C.c_void_p),
                ("raw2_xy", C.c_void_p), ("mb1", C.c_float), ("mb2", C.c_float), ("bf", C.c_float)]


class BowStereo(C.Structure):
    _fields_ = [("ur1", C.c_void_p), ("ur2", C.c_void_p), ("only_stereo", C.c_int32)]


TRIANGULATE_MAX_N, MAX_LEVELS = 8192, 16   # SLAMIT_TRIANGULATE_MAX_N, SLAMIT_MAX_LEVELS


class FrustumFrame(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("bf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("view_cos_limit", C.c_float), ("log_scale_factor", C.c_float), ("th", C.c_float), ("n_levels", C.c_int32),
                ("scale_factors", C.c_float * 16)]


class FrustumProblem(C.Structure):
    _fields_ = [("frame", FrustumFrame), ("n", C.c_int32), ("pos", C.c_void_p), ("normal", C.c_void_p), ("max_dist", C.c_void_p),
                ("min_dist", C.c_void_p), ("skip", C.c_void_p)]


class FrustumResult(C.Structure):
    _fields_ = [("status", C.c_void_p), ("proj", C.c_void_p), ("view_cos", C.c_void_p), ("level", C.c_void_p), ("uvr", C.c_void_p),
                ("level_min", C.c_void_p), ("level_max", C.c_void_p), ("valid", C.c_void_p), ("n_in_view", C.c_int32)]


class FrustumBatchRec(C.Structure):
    _fields_ = [("nframes", C.c_int32), ("q_cap", C.c_int32), ("d_frames", C.c_void_p), ("d_m", C.c_void_p), ("d_pos", C.c_void_p),
                ("d_normal", C.c_void_p), ("d_max_dist", C.c_void_p), ("d_min_dist", C.c_void_p), ("d_skip", C.c_void_p), ("d_uvr", C.c_void_p),
                ("d_level_min", C.c_void_p), ("d_level_max", C.c_void_p), ("d_valid", C.c_void_p), ("d_status", C.c_void_p),
                ("d_proj", C.c_void_p), ("d_view_cos", C.c_void_p), ("d_level", C.c_void_p), ("d_n_in_view", C.c_void_p)]


FRUSTUM_MAX_N = 65536   # SLAMIT_FRUSTUM_MAX_N
FRUSTUM_FRAME_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                                ("bf", "<f4"), ("min_x", "<f4"), ("max_x", "<f4"), ("min_y", "<f4"), ("max_y", "<f4"), ("view_cos_limit", "<f4"),
                                ("log_scale_factor", "<f4"), ("th", "<f4"), ("n_levels", "<i4"), ("scale_factors", "<f4", 16)])   # slamit_frustum_frame


class ProjectCamera(C.Structure):
    _fields_ = [("form", C.c_int32), ("R", C.c_float * 9), ("t", C.c_float * 3), ("O", C.c_float * 3), ("R2", C.c_float * 9), ("t2", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float),
                ("min_y", C.c_float), ("max_y", C.c_float), ("log_scale_factor", C.c_float), ("th", C.c_float), ("n_levels", C.c_int32),
                ("scale_factors", C.c_float * 16), ("direction", C.c_int32)]


class ProjectProblem(C.Structure):
    _fields_ = [("camera", ProjectCamera), ("n", C.c_int32), ("pos", C.c_void_p), ("normal", C.c_void_p), ("max_dist", C.c_void_p),
                ("min_dist", C.c_void_p), ("octave", C.c_void_p), ("skip", C.c_void_p)]


class ProjectResult(C.Structure):
    _fields_ = [("status", C.c_void_p), ("proj", C.c_void_p), ("level", C.c_void_p), ("uvr", C.c_void_p), ("level_min", C.c_void_p),
                ("level_max", C.c_void_p), ("valid", C.c_void_p), ("n_valid", C.c_int32)]


class ProjectBatchRec(C.Structure):
    _fields_ = [("nframes", C.c_int32), ("q_cap", C.c_int32), ("d_cameras", C.c_void_p), ("d_m", C.c_void_p), ("d_pos", C.c_void_p),
                ("d_normal", C.c_void_p), ("d_max_dist", C.c_void_p), ("d_min_dist", C.c_void_p), ("d_octave", C.c_void_p), ("d_skip", C.c_void_p),
                ("d_uvr", C.c_void_p), ("d_level_min", C.c_void_p), ("d_level_max", C.c_void_p), ("d_valid", C.c_void_p), ("d_status", C.c_void_p),
                ("d_proj", C.c_void_p), ("d_level", C.c_void_p), ("d_n_valid", C.c_void_p)]


class RotationBatch(C.Structure):
    _fields_ = [("nframes", C.c_int32), ("kp_cap", C.c_int32), ("q_cap", C.c_int32), ("d_n", C.c_void_p), ("d_kps_un", C.c_void_p),
                ("d_m", C.c_void_p), ("d_match_kp", C.c_void_p), ("d_qangle", C.c_void_p), ("d_kp_query", C.c_void_p), ("d_nmatches", C.c_void_p),
                ("d_bins", C.c_void_p)]


class PyramidLevel(C.Structure):
    _fields_ = [("plane", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("stride", C.c_size_t), ("frame_stride", C.c_size_t)]


class PyramidView(C.Structure):
    _fields_ = [("nlevels", C.c_int32), ("nframes", C.c_int32), ("level", PyramidLevel * 16)]


class StereoBatch(C.Structure):
    _fields_ = [("nframes", C.c_int32), ("cap_left", C.c_int32), ("cap_right", C.c_int32), ("reserved", C.c_int32), ("left", PyramidView),
                ("right", PyramidView), ("d_kps_left", C.c_void_p), ("d_desc_left", C.c_void_p), ("d_n_left", C.c_void_p),
                ("d_kps_right", C.c_void_p), ("d_desc_right", C.c_void_p), ("d_n_right", C.c_void_p), ("d_mb", C.c_void_p), ("d_mbf", C.c_void_p),
                ("d_scale", C.c_void_p), ("d_inv_scale", C.c_void_p), ("d_workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("d_u_right", C.c_void_p), ("d_depth", C.c_void_p), ("d_status", C.c_void_p), ("d_best_r", C.c_void_p), ("d_ham_dist", C.c_void_p),
                ("d_sad_dist", C.c_void_p), ("d_n_matched", C.c_void_p)]


STEREO_MAX_KP = 8191   # SLAMIT_STEREO_MAX_KP
STEREO_STATUS = ("matched", "no_candidate", "no_descriptor", "right_window", "edge_shift", "delta", "disparity", "median", "departure")


class DepthPlane(C.Structure):   # slamit_depth_plane
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_size_t), ("width", C.c_int32), ("height", C.c_int32), ("type", C.c_int32), ("factor", C.c_float)]


class RgbdProblem(C.Structure):
    _fields_ = [("plane", DepthPlane), ("mbf", C.c_float), ("n", C.c_int32), ("kps", C.c_void_p), ("kps_un", C.c_void_p)]


class RgbdResult(C.Structure):
    _fields_ = [("u_right", C.c_void_p), ("depth", C.c_void_p), ("status", C.c_void_p)]


class RgbdBatchRec(C.Structure):
    _fields_ = [("nframes", C.c_int32), ("cap", C.c_int32), ("d_planes", C.c_void_p), ("d_mbf", C.c_void_p), ("d_kps", C.c_void_p),
                ("d_kps_un", C.c_void_p), ("d_n", C.c_void_p), ("d_u_right", C.c_void_p), ("d_depth", C.c_void_p), ("d_status", C.c_void_p)]


class UnprojectFrame(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float),
                ("Rwc", C.c_float * 9), ("Ow", C.c_float * 3), ("th_depth", C.c_float), ("min_points", C.c_int32), ("mode", C.c_int32),
                ("ctor", C.c_int32), ("n_levels", C.c_int32), ("scale_factors", C.c_float * 16)]


class UnprojectCounts(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_candidates", "n_close", "n_visited", "n_created", "n_total", "n_map")]


class UnprojectProblem(C.Structure):
    _fields_ = [("frame", UnprojectFrame), ("n", C.c_int32), ("kps_un", C.c_void_p), ("depth", C.c_void_p), ("tracked", C.c_void_p)]


class UnprojectResult(C.Structure):
    _fields_ = [("status", C.c_void_p), ("order", C.c_void_p), ("pos", C.c_void_p), ("normal", C.c_void_p), ("max_dist", C.c_void_p),
                ("min_dist", C.c_void_p), ("counts", UnprojectCounts)]


class UnprojectBatchRec(C.Structure):
    _fields_ = [("nframes", C.c_int32), ("cap", C.c_int32), ("d_frames", C.c_void_p), ("d_n", C.c_void_p), ("d_kps_un", C.c_void_p),
                ("d_depth", C.c_void_p), ("d_tracked", C.c_void_p), ("d_pos", C.c_void_p), ("d_octave", C.c_void_p), ("d_skip", C.c_void_p),
                ("d_normal", C.c_void_p), ("d_max_dist", C.c_void_p), ("d_min_dist", C.c_void_p), ("d_status", C.c_void_p), ("d_order", C.c_void_p),
                ("d_counts", C.c_void_p)]


class MapIndexRec(C.Structure):   # struct slamit_map_index
    _fields_ = [("n_kf", C.c_int32), ("n_mp", C.c_int32), ("obs_ptr", C.c_void_p), ("obs_kf", C.c_void_p), ("mp_bad", C.c_void_p),
                ("kf_bad", C.c_void_p), ("kf_mp_ptr", C.c_void_p), ("kf_mp", C.c_void_p), ("kf_best", C.c_void_p), ("kf_child_ptr", C.c_void_p),
                ("kf_child", C.c_void_p), ("kf_parent", C.c_void_p), ("mp_pos", C.c_void_p), ("mp_normal", C.c_void_p),
                ("mp_max_dist", C.c_void_p), ("mp_min_dist", C.c_void_p)]


class LocalMapBatchRec(C.Structure):   # struct slamit_local_map_batch_rec
    _fields_ = [("nframes", C.c_int32), ("n_maps", C.c_int32), ("kp_cap", C.c_int32), ("seen_cap", C.c_int32), ("kf_cap", C.c_int32),
                ("q_cap", C.c_int32), ("vote_cap", C.c_int32), ("mp_cap", C.c_int32), ("maps", C.POINTER(MapIndexRec)), ("d_frame_map", C.c_void_p),
                ("d_n", C.c_void_p), ("d_frame_mp", C.c_void_p), ("d_n_seen", C.c_void_p), ("d_frame_seen", C.c_void_p), ("d_votes", C.c_void_p),
                ("d_local_kf", C.c_void_p), ("d_n_local_kf", C.c_void_p), ("d_ref_kf", C.c_void_p), ("d_local_mp", C.c_void_p),
                ("d_n_local_mp", C.c_void_p), ("d_pos", C.c_void_p), ("d_normal", C.c_void_p), ("d_max_dist", C.c_void_p),
                ("d_min_dist", C.c_void_p), ("d_skip", C.c_void_p), ("d_m", C.c_void_p), ("d_status", C.c_void_p), ("d_workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


# SLAMIT_LOCAL_MAP_*: the status bits, then MAX_KF, MAX_ROW, MIN_KF_CAP, MAX_MAPS, BEST
LOCAL_MAP_STATUS = {"BAD_SLOT": 1, "KF_OVERFLOW": 2, "MP_OVERFLOW": 4, "ROW_CUT": 8}
LOCAL_MAP_MAX_KF, LOCAL_MAP_MAX_ROW, LOCAL_MAP_MIN_KF_CAP, LOCAL_MAP_MAX_MAPS, LOCAL_MAP_BEST = 65535, 65536, 83, 8, 10
# slamit_map_index: the tables and their element types, in the record's order
MAP_INDEX_TABLES = (("obs_ptr", np.int32), ("obs_kf", np.int32), ("mp_bad", np.uint8), ("kf_bad", np.uint8), ("kf_mp_ptr", np.int32),
                    ("kf_mp", np.int32), ("kf_best", np.int32), ("kf_child_ptr", np.int32), ("kf_child", np.int32), ("kf_parent", np.int32),
                    ("mp_pos", np.float32), ("mp_normal", np.float32), ("mp_max_dist", np.float32), ("mp_min_dist", np.float32))


class CovisIndexRec(C.Structure):   # struct slamit_covis_index
    _fields_ = [("row_cap", C.c_int32), ("origin_kf", C.c_int32), ("obs_octave", C.c_void_p), ("obs_weight", C.c_void_p), ("mp_nobs", C.c_void_p),
                ("kf_octave", C.c_void_p), ("kf_depth", C.c_void_p), ("kf_th_depth", C.c_void_p), ("kf_not_erase", C.c_void_p), ("cw_kf", C.c_void_p),
                ("cw_w", C.c_void_p), ("cw_n", C.c_void_p), ("ord_kf", C.c_void_p), ("ord_w", C.c_void_p), ("ord_n", C.c_void_p), ("kf_best", C.c_void_p)]


class CovisBatchRec(C.Structure):   # struct slamit_covis_batch_rec
    _fields_ = [("nitems", C.c_int32), ("n_maps", C.c_int32), ("count_cap", C.c_int32), ("reserved", C.c_int32), ("maps", C.POINTER(MapIndexRec)),
                ("covis", C.POINTER(CovisIndexRec)), ("item_map", C.POINTER(C.c_int32)), ("d_kf", C.c_void_p), ("d_first", C.c_void_p),
                ("d_counts", C.c_void_p), ("d_n_counted", C.c_void_p), ("d_n_listed", C.c_void_p), ("d_parent", C.c_void_p), ("d_status", C.c_void_p)]


class CullingBatchRec(C.Structure):   # struct slamit_culling_batch_rec
    _fields_ = [("nprob", C.c_int32), ("n_maps", C.c_int32), ("cand_cap", C.c_int32), ("mp_cap", C.c_int32), ("maps", C.POINTER(MapIndexRec)),
                ("covis", C.POINTER(CovisIndexRec)), ("d_prob_map", C.c_void_p), ("d_kf", C.c_void_p), ("d_monocular", C.c_void_p),
                ("d_verdict", C.c_void_p), ("d_n_mps", C.c_void_p), ("d_n_redundant", C.c_void_p), ("d_n_cand", C.c_void_p),
                ("d_mp_turned_bad", C.c_void_p), ("d_status", C.c_void_p)]


# SLAMIT_COVIS_*: the status bits, MAX_ROW, TH, and the verdicts (the index is the value)
COVIS_STATUS = {"NO_OBSERVER": 1, "ROW_OVERFLOW": 2, "BAD_SLOT": 4}
COVIS_MAX_ROW, COVIS_TH = 1024, 15
COVIS_VERDICTS = ("kept", "culled", "to_be_erased", "origin")
# slamit_covis_index: the columns and graph rows and their element types, in the record's order
COVIS_INDEX_TABLES = (("obs_octave", np.uint8), ("obs_weight", np.uint8), ("mp_nobs", np.int32), ("kf_octave", np.uint8), ("kf_depth", np.float32),
                      ("kf_th_depth", np.float32), ("kf_not_erase", np.uint8), ("cw_kf", np.int32), ("cw_w", np.int32), ("cw_n", np.int32),
                      ("ord_kf", np.int32), ("ord_w", np.int32), ("ord_n", np.int32), ("kf_best", np.int32))
COVIS_GRAPH = ("cw_kf", "cw_w", "cw_n", "ord_kf", "ord_w", "ord_n", "kf_best")   # what UpdateConnections rewrites


class PointIndexRec(C.Structure):   # struct slamit_point_index
    _fields_ = [("n_levels", C.c_int32), ("reserved", C.c_int32), ("scale_factors", C.c_float * 16), ("obs_idx", C.c_void_p), ("obs_octave", C.c_void_p),
                ("kf_octave", C.c_void_p), ("kf_center", C.c_void_p), ("kf_desc", C.c_void_p), ("mp_ref_kf", C.c_void_p), ("mp_nobs", C.c_void_p),
                ("mp_found", C.c_void_p), ("mp_visible", C.c_void_p), ("mp_first_kf", C.c_void_p), ("mp_normal", C.c_void_p), ("mp_max_dist", C.c_void_p),
                ("mp_min_dist", C.c_void_p), ("mp_desc", C.c_void_p)]


class PointsBatchRec(C.Structure):   # struct slamit_points_batch_rec
    _fields_ = [("nitems", C.c_int32), ("n_maps", C.c_int32), ("cap", C.c_int32), ("reserved", C.c_int32), ("maps", C.POINTER(MapIndexRec)),
                ("pts", C.POINTER(PointIndexRec)), ("d_item_map", C.c_void_p), ("d_n", C.c_void_p), ("d_what", C.c_void_p), ("d_points", C.c_void_p),
                ("d_status", C.c_void_p)]


class PointCullingBatchRec(C.Structure):   # struct slamit_point_culling_batch_rec
    _fields_ = [("nlists", C.c_int32), ("n_maps", C.c_int32), ("cap", C.c_int32), ("reserved", C.c_int32), ("maps", C.POINTER(MapIndexRec)),
                ("pts", C.POINTER(PointIndexRec)), ("d_list_map", C.c_void_p), ("d_cur_id", C.c_void_p), ("d_monocular", C.c_void_p), ("d_n", C.c_void_p),
                ("d_recent", C.c_void_p), ("d_verdict", C.c_void_p), ("d_kept", C.c_void_p), ("d_n_kept", C.c_void_p), ("d_status", C.c_void_p)]


# SLAMIT_UPKEEP_*: the status bits, the ceilings, `what`, and the verdicts (the index is the value)
UPKEEP_STATUS = {"REF_NOT_OBSERVER": 1, "NO_REF": 2, "REF_NO_KP": 4, "OCTAVE": 8, "DESC_OVERFLOW": 16, "OBS_OVERFLOW": 32, "BAD_SLOT": 64}
UPKEEP_MAX_OBS, UPKEEP_MAX_POINTS, UPKEEP_MAX_RECENT, DISTINCTIVE_MAX = 512, 65536, 65536, 128
UPKEEP_NORMAL, UPKEEP_DESC = 1, 2
UPKEEP_VERDICTS = ("kept", "was_bad", "low_ratio", "few_obs", "aged")
# slamit_point_index: the columns and their element types, in the record's order; the last four are rewritten
POINT_INDEX_TABLES = (("obs_idx", np.int32), ("obs_octave", np.uint8), ("kf_octave", np.uint8), ("kf_center", np.float32), ("kf_desc", np.uint8),
                      ("mp_ref_kf", np.int32), ("mp_nobs", np.int32), ("mp_found", np.int32), ("mp_visible", np.int32), ("mp_first_kf", np.int32),
                      ("mp_normal", np.float32), ("mp_max_dist", np.float32), ("mp_min_dist", np.float32), ("mp_desc", np.uint8))
POINT_PLANES = ("mp_normal", "mp_max_dist", "mp_min_dist", "mp_desc")   # what update_points rewrites


class EditIndexRec(C.Structure):   # struct slamit_edit_index
    _fields_ = [("obs_idx", C.c_void_p), ("obs_octave", C.c_void_p), ("obs_weight", C.c_void_p), ("mp_bad", C.c_void_p), ("mp_nobs", C.c_void_p),
                ("mp_ref_kf", C.c_void_p), ("kf_mp", C.c_void_p), ("obs_ptr_out", C.c_void_p), ("obs_kf_out", C.c_void_p), ("obs_idx_out", C.c_void_p),
                ("obs_octave_out", C.c_void_p), ("obs_weight_out", C.c_void_p), ("obs_cap_out", C.c_int32), ("reserved", C.c_int32)]


class MapEditBatchRec(C.Structure):   # struct slamit_map_edit_batch_rec
    _fields_ = [("n_maps", C.c_int32), ("cap", C.c_int32), ("mp_cap", C.c_int32), ("kfmp_cap", C.c_int32), ("maps", C.POINTER(MapIndexRec)),
                ("edit", C.POINTER(EditIndexRec)), ("d_edits", C.c_void_p), ("d_n", C.c_void_p), ("d_status_mp", C.c_void_p), ("d_touched", C.c_void_p),
                ("d_n_touched", C.c_void_p), ("d_n_obs_out", C.c_void_p), ("d_status", C.c_void_p), ("d_workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


# SLAMIT_EDIT_*: the kinds, the flag, the status bits, the ceilings; struct slamit_map_edit as a numpy record
EDIT_ADD_OBS, EDIT_ERASE_OBS, EDIT_SET_BAD, EDIT_MATCH = 1, 2, 3, 1
EDIT_STATUS = {"REF_END": 1, "EDIT_OVERFLOW": 2, "OBS_OVERFLOW": 4, "BAD_SLOT": 8, "TABLE_OVERFLOW": 16}
EDIT_MAX_PER_POINT, EDIT_MAX_EDITS = 64, 1 << 20
EDIT_DTYPE = np.dtype([("kind", "<i4"), ("flags", "<i4"), ("mp", "<i4"), ("kf", "<i4"), ("idx", "<i4"), ("octave", "u1"), ("weight", "u1"), ("pad", "u1", 2)])
# slamit_edit_index: the columns read, the arrays rewritten in place, the observation table written out of place
EDIT_INDEX_COLUMNS = (("obs_idx", np.int32), ("obs_octave", np.uint8), ("obs_weight", np.uint8))
EDIT_INDEX_INPLACE = (("mp_bad", np.uint8), ("mp_nobs", np.int32), ("mp_ref_kf", np.int32), ("kf_mp", np.int32))
EDIT_INDEX_OUT = (("obs_kf_out", np.int32), ("obs_idx_out", np.int32), ("obs_octave_out", np.uint8), ("obs_weight_out", np.uint8))


class ReplaceIndexRec(C.Structure):   # struct slamit_replace_index
    _fields_ = [("obs_idx", C.c_void_p), ("obs_octave", C.c_void_p), ("obs_weight", C.c_void_p), ("mp_bad", C.c_void_p), ("mp_nobs", C.c_void_p),
                ("mp_found", C.c_void_p), ("mp_visible", C.c_void_p), ("mp_replaced", C.c_void_p), ("kf_mp", C.c_void_p), ("obs_ptr_out", C.c_void_p),
                ("obs_kf_out", C.c_void_p), ("obs_idx_out", C.c_void_p), ("obs_octave_out", C.c_void_p), ("obs_weight_out", C.c_void_p),
                ("obs_cap_out", C.c_int32), ("reserved", C.c_int32)]


class MapReplaceBatchRec(C.Structure):   # struct slamit_map_replace_batch_rec
    _fields_ = [("n_maps", C.c_int32), ("cap", C.c_int32), ("mp_cap", C.c_int32), ("kfmp_cap", C.c_int32), ("maps", C.POINTER(MapIndexRec)),
                ("index", C.POINTER(ReplaceIndexRec)), ("d_ops", C.c_void_p), ("d_n", C.c_void_p), ("d_moved", C.c_void_p), ("d_erased", C.c_void_p),
                ("d_touched", C.c_void_p), ("d_n_touched", C.c_void_p), ("d_n_obs_out", C.c_void_p), ("d_status", C.c_void_p), ("d_workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


class MapFuseBatchRec(C.Structure):   # struct slamit_map_fuse_batch_rec
    _fields_ = [("n_maps", C.c_int32), ("cap", C.c_int32), ("mp_cap", C.c_int32), ("kfmp_cap", C.c_int32), ("maps", C.POINTER(MapIndexRec)),
                ("index", C.POINTER(ReplaceIndexRec)), ("d_ops", C.c_void_p), ("d_n", C.c_void_p), ("d_outcome", C.c_void_p), ("d_moved", C.c_void_p),
                ("d_erased", C.c_void_p), ("d_touched", C.c_void_p), ("d_n_touched", C.c_void_p), ("d_n_fused", C.c_void_p), ("d_n_obs_out", C.c_void_p),
                ("d_status", C.c_void_p), ("d_workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


class FuseListBatchRec(C.Structure):   # struct slamit_fuse_list_batch_rec
    _fields_ = [("nframes", C.c_int32), ("n_maps", C.c_int32), ("kp_cap", C.c_int32), ("q_cap", C.c_int32), ("cap", C.c_int32), ("reserved", C.c_int32),
                ("d_m", C.c_void_p), ("d_match_kp", C.c_void_p), ("d_query_point", C.c_void_p), ("d_kps_un", C.c_void_p), ("d_kp_ur", C.c_void_p),
                ("d_frame_map", C.c_void_p), ("d_frame_kf", C.c_void_p), ("d_base", C.c_void_p), ("d_ops", C.c_void_p), ("d_n", C.c_void_p), ("d_status", C.c_void_p)]


class CheckReplacedBatchRec(C.Structure):   # struct slamit_check_replaced_batch_rec
    _fields_ = [("nframes", C.c_int32), ("n_maps", C.c_int32), ("cap", C.c_int32), ("reserved", C.c_int32), ("n_mp", C.POINTER(C.c_int32)),
                ("d_mp_replaced", C.POINTER(C.c_void_p)), ("d_frame_map", C.c_void_p), ("d_n", C.c_void_p), ("d_frame_mp", C.c_void_p), ("d_status", C.c_void_p)]


# SLAMIT_REPLACE_*: the kinds, the status bits, the ceilings; struct slamit_map_replace as a numpy record
REPLACE_REPLACE, REPLACE_ADD_OBS = 1, 2
REPLACE_STATUS = {"OP_OVERFLOW": 1, "OBS_OVERFLOW": 2, "TABLE_OVERFLOW": 4, "BAD_SLOT": 8}
REPLACE_REFUSED = 1 | 2 | 4   # with one of these nothing was written but the status (and n_obs_out for TABLE_OVERFLOW)
REPLACE_MAX_OPS, REPLACE_MAX_PER_POINT, CHECK_REPLACED_MAX_N = 16384, 64, 65536
REPLACE_DTYPE = np.dtype([("kind", "<i4"), ("a", "<i4"), ("b", "<i4"), ("idx", "<i4"), ("octave", "u1"), ("weight", "u1"), ("pad", "u1", 2)])
# SLAMIT_FUSE_*: the third kind of a fuse list, its outcomes, the status bits (REPLACE's values) and the ceiling
FUSE_FUSE = 3
FUSE_OUT = {"PLAIN": 0, "NOMATCH": 1, "SKIP_BAD": 2, "SKIP_IN_KF": 3, "ADDED": 4, "OCCUPANT_BAD": 5, "P_REPLACED": 6, "Q_REPLACED": 7}
FUSE_STATUS = {"OBS_OVERFLOW": 2, "TABLE_OVERFLOW": 4, "BAD_SLOT": 8}
FUSE_REFUSED = 2 | 4   # with one of these nothing was written but the status (and n_obs_out for TABLE_OVERFLOW)
FUSE_MAX_OPS = 16384
# slamit_replace_index: the columns read and the table written are the edit index's; the arrays rewritten in place
REPLACE_INDEX_INPLACE = (("mp_bad", np.uint8), ("mp_nobs", np.int32), ("mp_found", np.int32), ("mp_visible", np.int32), ("mp_replaced", np.int32), ("kf_mp", np.int32))


class TreeIndexRec(C.Structure):   # struct slamit_tree_index
    _fields_ = [("row_cap", C.c_int32), ("origin_kf", C.c_int32), ("kf_not_erase", C.c_void_p), ("kf_bad", C.c_void_p), ("kf_parent", C.c_void_p),
                ("kf_to_be_erased", C.c_void_p), ("cw_kf", C.c_void_p), ("cw_w", C.c_void_p), ("cw_n", C.c_void_p), ("ord_kf", C.c_void_p), ("ord_w", C.c_void_p),
                ("ord_n", C.c_void_p), ("kf_best", C.c_void_p), ("child_ptr_out", C.c_void_p), ("child_out", C.c_void_p), ("child_cap_out", C.c_int32),
                ("reserved", C.c_int32)]


class KfEraseBatchRec(C.Structure):   # struct slamit_kf_erase_batch_rec
    _fields_ = [("n_maps", C.c_int32), ("cap", C.c_int32), ("kf_cap", C.c_int32), ("row_cap", C.c_int32), ("child_cap", C.c_int32), ("edit_cap", C.c_int32),
                ("maps", C.POINTER(MapIndexRec)), ("tree", C.POINTER(TreeIndexRec)), ("d_ops", C.c_void_p), ("d_n", C.c_void_p), ("d_op_status", C.c_void_p),
                ("d_edits", C.c_void_p), ("d_n_edits_out", C.c_void_p), ("d_n_child_out", C.c_void_p), ("d_status", C.c_void_p), ("d_workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


# SLAMIT_KF_ERASE_*: the kinds, the status bits, the ceilings; struct slamit_kf_op as a numpy record
KF_ERASE_SET_PARENT, KF_ERASE_SET_BAD = 1, 2
KF_ERASE_STATUS = {"ORIGIN": 1, "NOT_ERASE": 2, "NO_PARENT": 4, "BAD_SLOT": 8, "ROW_OVERFLOW": 16, "CHILD_OVERFLOW": 32, "EDIT_OVERFLOW": 64}
KF_ERASE_REFUSED = 32 | 64   # with one of these nothing was written but the two needs and the status
KF_ERASE_MAX_OPS, KF_ERASE_MAX_CHILD = 1024, 1024
KF_OP_DTYPE = np.dtype([("kind", "<i4"), ("kf", "<i4"), ("parent", "<i4"), ("reserved", "<i4")])
# slamit_tree_index: the column read, the arrays rewritten in place (the last seven are the covis record's graph)
TREE_INDEX_INPLACE = (("kf_bad", np.uint8), ("kf_parent", np.int32), ("kf_to_be_erased", np.uint8), ("cw_kf", np.int32), ("cw_w", np.int32), ("cw_n", np.int32),
                      ("ord_kf", np.int32), ("ord_w", np.int32), ("ord_n", np.int32), ("kf_best", np.int32))


# slamit_grow_index: the appendable arrays and their element types, in the record's order (after kf_cap, mp_cap, kfmp_cap, reserved)
GROW_INDEX_ARRAYS = (("kf_mp_ptr", np.int32), ("kf_mp", np.int32), ("kf_octave", np.uint8), ("kf_desc", np.uint8), ("kf_depth", np.float32), ("kf_bad", np.uint8),
                     ("kf_parent", np.int32), ("kf_to_be_erased", np.uint8), ("kf_not_erase", np.uint8), ("kf_th_depth", np.float32), ("kf_best", np.int32),
                     ("cw_n", np.int32), ("ord_n", np.int32), ("kf_child_ptr", np.int32), ("kf_center", np.float32), ("mp_pos", np.float32),
                     ("mp_normal", np.float32), ("mp_max_dist", np.float32), ("mp_min_dist", np.float32), ("mp_bad", np.uint8), ("mp_nobs", np.int32),
                     ("mp_ref_kf", np.int32), ("mp_found", np.int32), ("mp_visible", np.int32), ("mp_first_kf", np.int32), ("mp_replaced", np.int32),
                     ("mp_desc", np.uint8), ("obs_ptr", np.int32))


class GrowIndexRec(C.Structure):   # struct slamit_grow_index
    _fields_ = [("kf_cap", C.c_int32), ("mp_cap", C.c_int32), ("kfmp_cap", C.c_int32), ("reserved", C.c_int32)] + [(k, C.c_void_p) for k, _ in GROW_INDEX_ARRAYS]


class GrowFrameRec(C.Structure):   # struct slamit_grow_frame
    _fields_ = [("n_kp", C.c_int32), ("th_depth", C.c_float), ("frame_mp", C.c_void_p), ("octave", C.c_void_p), ("desc", C.c_void_p), ("depth", C.c_void_p),
                ("uright", C.c_void_p), ("Tcw", C.c_void_p)]


class MapGrowBatchRec(C.Structure):   # struct slamit_map_grow_batch_rec
    _fields_ = [("n_maps", C.c_int32), ("cap", C.c_int32), ("n_frames", C.c_int32), ("cand_cap", C.c_int32), ("edit_cap", C.c_int32), ("recent_cap", C.c_int32),
                ("mp_cap", C.c_int32), ("reserved", C.c_int32), ("maps", C.POINTER(MapIndexRec)), ("grow", C.POINTER(GrowIndexRec)), ("frames", C.POINTER(GrowFrameRec)),
                ("d_ops", C.c_void_p), ("d_n", C.c_void_p), ("d_cand_status", C.c_void_p), ("d_cand_x3d", C.c_void_p), ("d_op_status", C.c_void_p),
                ("d_edits", C.c_void_p), ("d_n_edits_out", C.c_void_p), ("d_recent", C.c_void_p), ("d_n_recent", C.c_void_p), ("d_n_new", C.c_void_p),
                ("d_need", C.c_void_p), ("d_status", C.c_void_p), ("d_workspace", C.c_void_p), ("workspace_bytes", C.c_size_t)]


# SLAMIT_GROW_*: the kinds, the flag, the op codes, the status bits per map, the ceilings; struct slamit_grow_op as a numpy record
GROW_NEW_KF, GROW_NEW_POINT, GROW_ASSOCIATE, GROW_RECENT = 1, 2, 3, 1
GROW_OP_REJECTED, GROW_OP_BAD = -1, -2
GROW_STATUS = {"KF_OVERFLOW": 1, "MP_OVERFLOW": 2, "KFMP_OVERFLOW": 4, "EDIT_OVERFLOW": 8, "RECENT_OVERFLOW": 16, "KP_OVERFLOW": 32, "OPS_OVERFLOW": 64, "BAD_SLOT": 128}
GROW_REFUSED = 127   # with one of these nothing was written but the needs and the status
GROW_MAX_OPS, GROW_MAX_FRAMES, GROW_NEEDS = 65536, 16, 5
GROW_OP_DTYPE = np.dtype([("kind", "<i4"), ("flags", "<i4"), ("kf", "<i4"), ("src", "<i4"), ("kf_id", "<i4"), ("cand", "<i4"), ("kf_a", "<i4"), ("idx_a", "<i4"),
                          ("kf_b", "<i4"), ("idx_b", "<i4"), ("weight_a", "u1"), ("weight_b", "u1"), ("pad", "u1", 2), ("pos", "<f4", 3)])


DEPTH_TYPES = ("f32", "u16")   # SLAMIT_DEPTH_*: the index is the type
DEPTH_PLANE_DTYPE = np.dtype([("data", "<u8"), ("pitch", "<u8"), ("width", "<i4"), ("height", "<i4"), ("type", "<i4"), ("factor", "<f4")])   # slamit_depth_plane
RGBD_STATUS = ("no_depth", "depth", "outside")
UNPROJECT_MODES = ("CLOSEST", "ALL")   # SLAMIT_UNPROJECT_*
UNPROJECT_CTORS = ("FRAME", "KEYFRAME")   # SLAMIT_UNPROJECT_CTOR_*
UNPROJECT_STATUS = ("no_depth", "beyond", "tracked", "created", "octave")
UNPROJECT_COUNTS = ("n_candidates", "n_close", "n_visited", "n_created", "n_total", "n_map")   # slamit_unproject_counts
UNPROJECT_FRAME_DTYPE = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("invfx", "<f4"), ("invfy", "<f4"), ("Rwc", "<f4", 9),
                                  ("Ow", "<f4", 3), ("th_depth", "<f4"), ("min_points", "<i4"), ("mode", "<i4"), ("ctor", "<i4"), ("n_levels", "<i4"),
                                  ("scale_factors", "<f4", 16)])   # slamit_unproject_frame


PROJECT_MAX_N = 65536   # SLAMIT_PROJECT_MAX_N
PROJECT_FORMS = ("LAST_FRAME", "RELOC", "FUSE", "SIM3_PROJ", "SIM3_FUSE", "SIM3_PAIR")   # SLAMIT_PROJECT_*: the index is the form
PROJECT_CAMERA_DTYPE = np.dtype([("form", "<i4"), ("R", "<f4", 9), ("t", "<f4", 3), ("O", "<f4", 3), ("R2", "<f4", 9), ("t2", "<f4", 3), ("fx", "<f4"),
                                 ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("min_x", "<f4"), ("max_x", "<f4"), ("min_y", "<f4"), ("max_y", "<f4"),
                                 ("log_scale_factor", "<f4"), ("th", "<f4"), ("n_levels", "<i4"), ("scale_factors", "<f4", 16),
                                 ("direction", "<i4")])   # slamit_project_camera


class VocDesc(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32), ("n_nodes", C.c_int32),
                ("parent", C.c_void_p), ("is_leaf", C.c_void_p), ("desc", C.c_void_p), ("weight", C.c_void_p)]


VOC_MAX_K, VOC_MAX_L, VOC_MAX_FEATURES = 20, 10, 8191   # SLAMIT_VOC_MAX_K / _MAX_L / _MAX_FEATURES


class SearchBatch(C.Structure):
    _fields_ = [("nframes", C.c_int32), ("kp_cap", C.c_int32), ("q_cap", C.c_int32), ("d_n", C.c_void_p),
                ("d_kps_un", C.c_void_p), ("d_desc", C.c_void_p), ("d_kp_taken", C.c_void_p), ("min_x", C.c_float),
                ("min_y", C.c_float), ("inv_w", C.c_float), ("inv_h", C.c_float), ("d_m", C.c_void_p), ("d_uvr", C.c_void_p),
                ("d_level_min", C.c_void_p), ("d_level_max", C.c_void_p), ("d_qdesc", C.c_void_p), ("d_valid", C.c_void_p),
                ("d_takes", C.c_void_p)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k1", C.c_float),
                ("k2", C.c_float), ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float)]


class BaProfile(C.Structure):
    _fields_ = [("phase_ms", C.c_double * 5), ("slots", C.c_int32), ("nwin", C.c_int32), ("schur_exec_mflop", C.c_double)]


POSE_MAX_N, SIM3_MAX_N = 65536, 65536   # SLAMIT_POSE_MAX_N, SLAMIT_SIM3_MAX_N
FRAME_MAX_KP, HAMMING_MAX_TRAIN, BOW_MAX_GROUP = 30000, 65535, 2048   # SLAMIT_FRAME_MAX_KP, SLAMIT_HAMMING_MAX_TRAIN, SLAMIT_BOW_MAX_GROUP
BA_PHASES = ("linearize", "schur", "solve", "update", "residuals")   # slamit_ba_profile_out.phase_ms


class PoseProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("pose", C.c_void_p), ("intr", C.c_void_p), ("xw", C.c_void_p),
                ("uv", C.c_void_p), ("inv_sigma2", C.c_void_p), ("ur", C.c_void_p), ("bf", C.c_double)]   # stereo: right-image columns (< 0: monocular) and Frame::mbf


class PoseResult(C.Structure):
    _fields_ = [("pose", C.c_void_p), ("outlier", C.c_void_p), ("n_inliers", C.c_int32),
                ("n_its", C.c_int32 * 4), ("chi2", C.c_double * 4)]


EG_NORMAL, EG_LOOP_CONNECTION = 0, 1
EG_MAX_KF, EG_MAX_EDGES, EG_MAX_ITS, EG_MAX_TRIALS, EG_MAX_POINTS = 1024, 65536, 32, 320, 1 << 24


class EgGraph(C.Structure):   # struct slamit_eg_graph
    _fields_ = [("n_kf", C.c_int32), ("row_cap", C.c_int32), ("loop_kf", C.c_int32), ("cur_kf", C.c_int32), ("min_feat", C.c_int32), ("reserved", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("kf_bad", "kf_id", "kf_parent", "child_ptr", "child_kf", "loop_ptr", "loop_kf_list", "ord_kf", "ord_w", "ord_n",
                                          "conn_ptr", "conn_kf")]


class EgProblem(C.Structure):   # struct slamit_eg_problem
    _fields_ = [("n_kf", C.c_int32), ("n_edge", C.c_int32), ("n_pt", C.c_int32), ("n_free", C.c_int32), ("fix_scale", C.c_int32), ("max_its", C.c_int32),
                ("lambda_init", C.c_double)] + \
               [(k, C.c_void_p) for k in ("scw_r", "scw_t", "scw_s", "snc_r", "snc_t", "snc_s", "fixed", "bad", "edge_v0", "edge_v1", "edge_kind", "inc_ptr",
                                          "inc_edge", "pt_pos", "pt_ref", "pt_bad")]


class EgStats(C.Structure):   # struct slamit_eg_stats
    _fields_ = [("n_its", C.c_int32), ("n_trials", C.c_int32), ("n_free", C.c_int32), ("status", C.c_int32), ("chi2_init", C.c_double),
                ("chi2", C.c_double * EG_MAX_ITS), ("lambda", C.c_double * EG_MAX_ITS), ("trials", C.c_int32 * EG_MAX_ITS),
                ("trial_chi2", C.c_double * EG_MAX_TRIALS), ("trial_rho", C.c_double * EG_MAX_TRIALS)]


class EgResult(C.Structure):   # struct slamit_eg_result
    _fields_ = [(k, C.c_void_p) for k in ("sim3_r", "sim3_t", "sim3_s", "pose", "pt_pos", "touched", "n_touched", "stats")]


_lib = None

EXPORTS = [
    "slamit_essential_plan", "slamit_essential_graph", "slamit_essential_graph_workspace", "slamit_essential_graph_dev",
    "slamit_orb_create", "slamit_orb_destroy", "slamit_orb_tables", "slamit_orb_max_keypoints",
    "slamit_orb_extract", "slamit_orb_extract_batch", "slamit_orb_extract_batch_dev", "slamit_orb_level",
    "slamit_orb_debug_candidates", "slamit_orb_debug_octree_path", "slamit_orb_debug_blurred", "slamit_orb_profile", "slamit_hamming_best2", "slamit_hamming_best2_batch_dev",
    "slamit_hamming_matrix", "slamit_distinctive_batch", "slamit_guided_search", "slamit_guided_search_workspace", "slamit_guided_search_batch_dev", "slamit_guided_search_stereo", "slamit_guided_search_stereo_batch_dev", "slamit_bow_search", "slamit_voc_create", "slamit_voc_load_text", "slamit_voc_destroy", "slamit_voc_info",
    "slamit_voc_transform", "slamit_voc_transform_workspace", "slamit_voc_transform_batch_dev",
    "slamit_kfdb_create", "slamit_kfdb_destroy", "slamit_kfdb_clear", "slamit_kfdb_info", "slamit_kfdb_add", "slamit_kfdb_add_dev", "slamit_kfdb_erase",
    "slamit_kfdb_query", "slamit_kfdb_query_batch_dev", "slamit_undistort_points", "slamit_frame_finish",
    "slamit_frame_finish_batch_dev", "slamit_ba_create", "slamit_ba_create_ex", "slamit_ba_destroy", "slamit_ba_solve",
    "slamit_ba_solve_batch", "slamit_ba_profile", "slamit_ba_profile_read", "slamit_pose_optimize", "slamit_pose_optimize_batch", "slamit_sim3_optimize", "slamit_sim3_optimize_batch", "slamit_sim3_ransac", "slamit_sim3_ransac_batch", "slamit_pnp_ransac", "slamit_pnp_ransac_batch", "slamit_pnp_refine_batch", "slamit_init_hyp", "slamit_init_hyp_batch", "slamit_init_reconstruct", "slamit_init_reconstruct_batch", "slamit_init_best_hypothesis", "slamit_init_choose_h", "slamit_init_parallax_deg", "slamit_init_pick_f", "slamit_init_pick_h", "slamit_triangulate", "slamit_triangulate_batch", "slamit_triangulate_stereo", "slamit_triangulate_stereo_batch", "slamit_bow_search_stereo", "slamit_frustum", "slamit_frustum_batch", "slamit_frustum_batch_dev", "slamit_project", "slamit_project_batch", "slamit_project_batch_dev", "slamit_project_batch_stereo", "slamit_project_batch_dev_stereo", "slamit_rotation_check_batch_dev", "slamit_orb_pyramid_view", "slamit_stereo_match_workspace", "slamit_stereo_match_batch_dev", "slamit_stereo_match", "slamit_rgbd_depth", "slamit_rgbd_depth_batch", "slamit_rgbd_depth_batch_dev", "slamit_unproject_closest", "slamit_unproject_closest_batch", "slamit_unproject_closest_batch_dev", "slamit_local_keyframes", "slamit_local_points", "slamit_local_map_workspace", "slamit_local_map_batch_dev", "slamit_update_connections", "slamit_update_connections_batch_dev", "slamit_keyframe_culling", "slamit_keyframe_culling_batch_dev", "slamit_update_points", "slamit_update_points_batch_dev", "slamit_map_point_culling", "slamit_map_point_culling_batch_dev", "slamit_map_edit_apply", "slamit_map_edit_workspace", "slamit_map_edit_batch_dev", "slamit_map_replace_apply", "slamit_map_replace_workspace", "slamit_map_replace_batch_dev", "slamit_check_replaced", "slamit_check_replaced_batch_dev", "slamit_map_fuse_apply", "slamit_map_fuse_workspace", "slamit_map_fuse_batch_dev", "slamit_fuse_list_batch_dev", "slamit_kf_erase_apply", "slamit_kf_erase_workspace", "slamit_kf_erase_batch_dev", "slamit_map_grow_apply", "slamit_map_grow_workspace", "slamit_map_grow_batch_dev", "slamit_last_error", "slamit_version", "slamit_device_count", "slamit_set_device", "slamit_release_thread_scratch",
]


def lib():
    """Loads the HIP library; raises (never falls back) when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SlamitError(
                "libslamit_hip.so is not built: run `python -m weiner_slamit_v2_amd.build` "
                "(there is no CPU fallback)")
        # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.so.7 /
        # libhsa-runtime64; if ours loaded /opt/rocm's copy first, torch.cuda would later find
        # "No HIP GPUs".  Importing torch first makes our DT_NEEDED resolve to the copy torch
        # already mapped (same SONAME).  Pure C/C++ users link /opt/rocm and never see this.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
        L.slamit_orb_create.argtypes = [C.POINTER(OrbParams), i32, C.POINTER(vp)]
        L.slamit_orb_destroy.argtypes = [vp]
        L.slamit_orb_destroy.restype = None
        L.slamit_orb_tables.argtypes = [vp] + [vp] * 5
        L.slamit_orb_max_keypoints.argtypes = [vp]
        L.slamit_orb_extract.argtypes = [vp, vp, sz, vp, vp, i32, vp]
        L.slamit_orb_extract_batch.argtypes = [vp, vp, sz, sz, i32, vp, vp, i32, vp]
        L.slamit_orb_extract_batch_dev.argtypes = [vp, vp, sz, sz, i32, vp, vp, i32, vp, vp]
        L.slamit_orb_level.argtypes = [vp, i32, i32, vp, sz, vp, vp]
        L.slamit_orb_debug_blurred.argtypes = [vp, i32, i32, vp, sz, vp, vp]
        L.slamit_orb_profile.argtypes = [vp, i32, vp, vp, i32]
        L.slamit_orb_debug_candidates.argtypes = [vp, i32, i32, vp, i32, vp]
        if hasattr(L, "slamit_orb_debug_octree_path"):   # absent from earlier libraries loaded through SLAMIT_LIB for A/B runs
            L.slamit_orb_debug_octree_path.argtypes = [vp, i32, i32, vp]
        L.slamit_hamming_best2.argtypes = [vp, i32, vp, i32, vp, vp, vp]
        L.slamit_hamming_best2_batch_dev.argtypes = [vp, vp, sz, vp, vp, sz, i32, i32, vp, vp, vp, sz, i32, vp]
        L.slamit_hamming_matrix.argtypes = [vp, i32, vp, i32, vp]
        L.slamit_distinctive_batch.argtypes = [vp, vp, i32, vp, vp]
        L.slamit_guided_search.argtypes = [i32, C.POINTER(FrameView), C.POINTER(SearchQueries), C.POINTER(SearchRule),
                                           vp, vp, vp, vp, vp, vp]
        L.slamit_guided_search_workspace.argtypes = [i32, i32]
        L.slamit_guided_search_workspace.restype = sz
        L.slamit_guided_search_batch_dev.argtypes = [i32, C.POINTER(SearchBatch), C.POINTER(SearchRule), vp, vp, vp, vp, sz, vp]
        L.slamit_guided_search_stereo.argtypes = [i32, C.POINTER(FrameView), C.POINTER(SearchQueries), C.POINTER(SearchRule),
                                                  C.POINTER(SearchStereo), vp, vp, vp, vp, vp, vp]
        L.slamit_guided_search_stereo_batch_dev.argtypes = [i32, C.POINTER(SearchBatch), C.POINTER(SearchRule), C.POINTER(SearchStereoDev),
                                                            vp, vp, vp, vp, sz, vp]
        f32 = C.c_float
        L.slamit_sim3_optimize_batch.argtypes = [i32, i32, C.POINTER(Sim3Problem), C.POINTER(Sim3Result)]
        L.slamit_sim3_optimize.argtypes = [i32, C.POINTER(Sim3Problem), C.POINTER(Sim3Result)]
        L.slamit_sim3_ransac_batch.argtypes = [i32, i32, C.POINTER(Sim3RansacProblem), C.POINTER(Sim3RansacResult)]
        L.slamit_sim3_ransac.argtypes = [i32, C.POINTER(Sim3RansacProblem), C.POINTER(Sim3RansacResult)]
        L.slamit_pnp_ransac_batch.argtypes = [i32, i32, C.POINTER(PnpProblem), C.POINTER(PnpResult)]
        L.slamit_pnp_ransac.argtypes = [i32, C.POINTER(PnpProblem), C.POINTER(PnpResult)]
        L.slamit_pnp_refine_batch.argtypes = [i32, i32, C.POINTER(PnpRefineProblem), C.POINTER(PnpRefineResult)]
        L.slamit_init_hyp_batch.argtypes = [i32, i32, C.POINTER(InitProblem), C.POINTER(InitResult)]
        L.slamit_init_hyp.argtypes = [i32, C.POINTER(InitProblem), C.POINTER(InitResult)]
        L.slamit_init_reconstruct_batch.argtypes = [i32, i32, C.POINTER(InitReconstructProblem), C.POINTER(InitReconstructResult)]
        L.slamit_init_reconstruct.argtypes = [i32, C.POINTER(InitReconstructProblem), C.POINTER(InitReconstructResult)]
        L.slamit_init_best_hypothesis.argtypes = [i32, vp]
        L.slamit_init_choose_h.argtypes = [f32, f32]
        L.slamit_init_parallax_deg.argtypes = [i32, f32]
        L.slamit_init_parallax_deg.restype = f32
        L.slamit_init_pick_f.argtypes = [vp, vp, i32, f32, i32]
        L.slamit_init_pick_h.argtypes = [vp, vp, i32, f32, i32]
        L.slamit_triangulate_batch.argtypes = [i32, i32, C.POINTER(TriangulateProblem), C.POINTER(TriangulateResult)]
        L.slamit_triangulate.argtypes = [i32, C.POINTER(TriangulateProblem), C.POINTER(TriangulateResult)]
        L.slamit_triangulate_stereo_batch.argtypes = [i32, i32, C.POINTER(TriangulateProblem), C.POINTER(C.POINTER(TriangulateStereo)), C.POINTER(TriangulateResult), C.POINTER(vp)]
        L.slamit_triangulate_stereo.argtypes = [i32, C.POINTER(TriangulateProblem), C.POINTER(TriangulateStereo), C.POINTER(TriangulateResult), vp]
        L.slamit_frustum_batch.argtypes = [i32, i32, C.POINTER(FrustumProblem), C.POINTER(FrustumResult)]
        L.slamit_frustum.argtypes = [i32, C.POINTER(FrustumProblem), C.POINTER(FrustumResult)]
        L.slamit_frustum_batch_dev.argtypes = [i32, C.POINTER(FrustumBatchRec), vp]
        L.slamit_project_batch.argtypes = [i32, i32, C.POINTER(ProjectProblem), C.POINTER(ProjectResult)]
        L.slamit_project.argtypes = [i32, C.POINTER(ProjectProblem), C.POINTER(ProjectResult)]
        L.slamit_project_batch_dev.argtypes = [i32, C.POINTER(ProjectBatchRec), vp]
        L.slamit_project_batch_stereo.argtypes = [i32, i32, C.POINTER(ProjectProblem), C.POINTER(ProjectResult), vp, vp]
        L.slamit_project_batch_dev_stereo.argtypes = [i32, C.POINTER(ProjectBatchRec), vp, vp, vp]
        L.slamit_rotation_check_batch_dev.argtypes = [i32, C.POINTER(RotationBatch), vp]
        L.slamit_orb_pyramid_view.argtypes = [vp, C.POINTER(PyramidView)]
        L.slamit_stereo_match_workspace.argtypes = [i32, i32]
        L.slamit_stereo_match_workspace.restype = sz
        L.slamit_stereo_match_batch_dev.argtypes = [i32, C.POINTER(StereoBatch), vp]
        L.slamit_stereo_match.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, i32, f32, f32] + [vp] * 7
        L.slamit_rgbd_depth_batch.argtypes = [i32, i32, C.POINTER(RgbdProblem), C.POINTER(RgbdResult)]
        L.slamit_rgbd_depth.argtypes = [i32, C.POINTER(RgbdProblem), C.POINTER(RgbdResult)]
        L.slamit_rgbd_depth_batch_dev.argtypes = [i32, C.POINTER(RgbdBatchRec), vp]
        L.slamit_unproject_closest_batch.argtypes = [i32, i32, C.POINTER(UnprojectProblem), C.POINTER(UnprojectResult)]
        L.slamit_unproject_closest.argtypes = [i32, C.POINTER(UnprojectProblem), C.POINTER(UnprojectResult)]
        L.slamit_unproject_closest_batch_dev.argtypes = [i32, C.POINTER(UnprojectBatchRec), vp]
        L.slamit_local_keyframes.argtypes = [i32, C.POINTER(MapIndexRec), i32, vp, vp, i32, vp, vp, vp, vp]
        L.slamit_local_points.argtypes = [i32, C.POINTER(MapIndexRec), i32, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp]
        L.slamit_local_map_workspace.argtypes = [i32, i32, i32]
        L.slamit_local_map_workspace.restype = sz
        L.slamit_local_map_batch_dev.argtypes = [i32, C.POINTER(LocalMapBatchRec), vp]
        L.slamit_update_connections.argtypes = [i32, C.POINTER(MapIndexRec), C.POINTER(CovisIndexRec), i32, i32, vp, vp, vp, vp, vp]
        L.slamit_update_connections_batch_dev.argtypes = [i32, C.POINTER(CovisBatchRec), vp]
        L.slamit_keyframe_culling.argtypes = [i32, C.POINTER(MapIndexRec), C.POINTER(CovisIndexRec), i32, i32, vp, vp, vp, vp, vp, vp]
        L.slamit_keyframe_culling_batch_dev.argtypes = [i32, C.POINTER(CullingBatchRec), vp]
        L.slamit_update_points.argtypes = [i32, C.POINTER(MapIndexRec), C.POINTER(PointIndexRec), i32, vp, i32, vp]
        L.slamit_update_points_batch_dev.argtypes = [i32, C.POINTER(PointsBatchRec), vp]
        L.slamit_map_point_culling.argtypes = [i32, C.POINTER(MapIndexRec), C.POINTER(PointIndexRec), i32, i32, i32, vp, vp, vp, vp, vp]
        L.slamit_map_point_culling_batch_dev.argtypes = [i32, C.POINTER(PointCullingBatchRec), vp]
        L.slamit_map_edit_apply.argtypes = [i32, C.POINTER(MapIndexRec), C.POINTER(EditIndexRec), i32, vp, vp, vp, vp, vp, vp]
        L.slamit_map_edit_workspace.argtypes = [i32, i32, i32, i32]
        L.slamit_map_edit_workspace.restype = sz
        L.slamit_map_edit_batch_dev.argtypes = [i32, C.POINTER(MapEditBatchRec), vp]
        L.slamit_map_replace_apply.argtypes = [i32, C.POINTER(MapIndexRec), C.POINTER(ReplaceIndexRec), i32, vp, vp, vp, vp, vp, vp, vp]
        L.slamit_map_replace_workspace.argtypes = [i32, i32, i32, i32]
        L.slamit_map_replace_workspace.restype = sz
        L.slamit_map_replace_batch_dev.argtypes = [i32, C.POINTER(MapReplaceBatchRec), vp]
        L.slamit_map_fuse_apply.argtypes = [i32, C.POINTER(MapIndexRec), C.POINTER(ReplaceIndexRec), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.slamit_map_fuse_workspace.argtypes = [i32, i32, i32, i32]
        L.slamit_map_fuse_workspace.restype = sz
        L.slamit_map_fuse_batch_dev.argtypes = [i32, C.POINTER(MapFuseBatchRec), vp]
        L.slamit_fuse_list_batch_dev.argtypes = [i32, C.POINTER(FuseListBatchRec), vp]
        L.slamit_check_replaced.argtypes = [i32, i32, vp, i32, vp, vp]
        L.slamit_check_replaced_batch_dev.argtypes = [i32, C.POINTER(CheckReplacedBatchRec), vp]
        L.slamit_kf_erase_apply.argtypes = [i32, C.POINTER(MapIndexRec), C.POINTER(TreeIndexRec), i32, vp, vp, i32, vp, vp, vp, vp]
        L.slamit_kf_erase_workspace.argtypes = [i32, i32, i32, i32, i32]
        L.slamit_kf_erase_workspace.restype = sz
        L.slamit_kf_erase_batch_dev.argtypes = [i32, C.POINTER(KfEraseBatchRec), vp]
        L.slamit_map_grow_apply.argtypes = [i32, C.POINTER(MapIndexRec), C.POINTER(GrowIndexRec), i32, C.POINTER(GrowFrameRec), i32, vp, i32, vp, vp, vp, i32, vp, vp, i32,
                                            vp, vp, vp, vp, vp]
        L.slamit_map_grow_workspace.argtypes = [i32, i32]
        L.slamit_map_grow_workspace.restype = sz
        L.slamit_map_grow_batch_dev.argtypes = [i32, C.POINTER(MapGrowBatchRec), vp]
        L.slamit_bow_search.argtypes = [i32, vp, i32, vp, vp, i32, vp, C.POINTER(BowGroups), C.POINTER(BowRule), vp, vp, vp]
        L.slamit_bow_search_stereo.argtypes = [i32, vp, i32, vp, vp, i32, vp, C.POINTER(BowGroups), C.POINTER(BowRule), C.POINTER(BowStereo), vp, vp, vp]
        L.slamit_voc_create.argtypes = [C.POINTER(VocDesc), i32, C.POINTER(vp)]
        L.slamit_voc_load_text.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
        L.slamit_voc_destroy.argtypes = [vp]
        L.slamit_voc_destroy.restype = None
        L.slamit_voc_info.argtypes = [vp, vp, vp, vp, vp]
        L.slamit_voc_transform.argtypes = [vp, vp, i32, i32] + [vp] * 9
        L.slamit_voc_transform_workspace.argtypes = [i32, i32]
        L.slamit_voc_transform_workspace.restype = sz
        L.slamit_voc_transform_batch_dev.argtypes = [vp, vp, vp, i32, i32, i32] + [vp] * 9 + [vp, sz, vp]
        L.slamit_kfdb_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
        L.slamit_kfdb_destroy.argtypes = [vp]
        L.slamit_kfdb_destroy.restype = None
        L.slamit_kfdb_clear.argtypes = [vp]
        L.slamit_kfdb_info.argtypes = [vp, vp, vp, vp]
        L.slamit_kfdb_add.argtypes = [vp, vp, vp, i32, vp]
        L.slamit_kfdb_add_dev.argtypes = [vp, vp, vp, vp, vp, vp]
        L.slamit_kfdb_erase.argtypes = [vp, i32]
        L.slamit_kfdb_query.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
        L.slamit_kfdb_query_batch_dev.argtypes = [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
        L.slamit_undistort_points.argtypes = [i32, C.POINTER(Camera), vp, i32, vp]
        L.slamit_frame_finish.argtypes = [i32, C.POINTER(Camera), vp, i32, f32, f32, f32, f32, vp, vp, vp]
        L.slamit_frame_finish_batch_dev.argtypes = [i32, C.POINTER(Camera), vp, vp, i32, i32, f32, f32, f32, f32, vp, vp, vp, vp]
        if hasattr(L, "slamit_ba_create"):
            L.slamit_ba_create.argtypes = [i32, i32, i32, i32, i32, C.POINTER(vp)]
            if hasattr(L, "slamit_ba_create_ex"):
                L.slamit_ba_create_ex.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
            L.slamit_ba_destroy.argtypes = [vp]
            L.slamit_ba_destroy.restype = None
            L.slamit_ba_solve.argtypes = [vp, C.POINTER(BaProblem), C.POINTER(BaOpts), C.POINTER(BaResult)]
            L.slamit_ba_solve_batch.argtypes = [vp, i32, C.POINTER(BaProblem), C.POINTER(BaOpts), C.POINTER(BaResult)]
            if hasattr(L, "slamit_ba_profile"):   # absent from round-2 libraries loaded through SLAMIT_LIB for A/B runs
                L.slamit_ba_profile.argtypes = [vp, i32]
                L.slamit_ba_profile_read.argtypes = [vp, C.POINTER(BaProfile)]
        if hasattr(L, "slamit_pose_optimize_batch"):
            L.slamit_pose_optimize_batch.argtypes = [i32, i32, C.POINTER(PoseProblem), C.POINTER(PoseResult)]
            L.slamit_pose_optimize.argtypes = [i32, C.POINTER(PoseProblem), C.POINTER(PoseResult)]
        if hasattr(L, "slamit_essential_graph"):   # absent from earlier libraries loaded through SLAMIT_LIB for A/B runs
            L.slamit_essential_plan.argtypes = [C.POINTER(EgGraph), i32, vp, vp, vp, vp, vp, vp]
            L.slamit_essential_graph.argtypes = [i32, C.POINTER(EgProblem), C.POINTER(EgResult)]
            L.slamit_essential_graph_workspace.argtypes = [i32, i32, i32, i32]
            L.slamit_essential_graph_workspace.restype = sz
            L.slamit_essential_graph_dev.argtypes = [i32, C.POINTER(EgProblem), C.POINTER(EgResult), vp, sz, vp]
        L.slamit_last_error.restype = C.c_char_p
        L.slamit_version.restype = C.c_char_p
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise SlamitError("%s failed (%d): %s" % (what, rc, lib().slamit_last_error().decode()))


def device_count():
    return lib().slamit_device_count()


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class ORBextractor:
    """ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) on one GPU.

    Frame geometry is bound lazily on the first image (the reference accepts any cv::Mat; the
    device workspace is sized per geometry and re-created if it changes)."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7,
                 device=0, max_batch=1):
        self.params = (int(nfeatures), float(scaleFactor), int(nlevels), int(iniThFAST), int(minThFAST))
        self.device = device
        self.max_batch = max_batch
        self._h = None
        self._geom = None

    # -- handle management --
    def _bind(self, width, height, batch=1):
        if self._h is not None and self._geom == (width, height) and batch <= self.max_batch:
            return
        self.close()
        self.max_batch = max(self.max_batch, batch)
        p = OrbParams(self.params[0], self.params[1], self.params[2], self.params[3], self.params[4],
                      width, height, self.max_batch)
        h = C.c_void_p()
        _check(lib().slamit_orb_create(C.byref(p), self.device, C.byref(h)), "slamit_orb_create")
        self._h = h
        self._geom = (width, height)
        self.max_keypoints = lib().slamit_orb_max_keypoints(h)

    def close(self):
        if self._h is not None:
            lib().slamit_orb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- getters of the reference class --
    def GetLevels(self):
        return self.params[2]

    def GetScaleFactor(self):
        return self.params[1]

    def _tables(self):
        if self._h is None:
            self._bind(640, 480)
        n = self.params[2]
        out = [np.zeros(n, np.float32) for _ in range(4)] + [np.zeros(n, np.int32)]
        _check(lib().slamit_orb_tables(self._h, *[_np_ptr(a) for a in out]), "slamit_orb_tables")
        return out

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def features_per_level(self):
        return self._tables()[4]

    # -- operator() --
    def __call__(self, image, mask=None):
        """image: uint8 (H, W) numpy array. Returns (keypoints[KP_DTYPE], descriptors[n,32])."""
        image = np.asarray(image)
        if image.size == 0:
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        assert image.dtype == np.uint8 and image.ndim == 2, "CV_8UC1 expected (ORBextractor.cc:1075)"
        k, d = self.extract_batch(image[None])
        return k[0], d[0]

    def extract_batch(self, frames):
        """frames: uint8 (B, H, W) host array -> lists of per-frame keypoints / descriptors."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        b, hh, ww = frames.shape
        self._bind(ww, hh, b)
        cap = self.max_keypoints
        kps = np.zeros((b, cap), KP_DTYPE)
        desc = np.zeros((b, cap, 32), np.uint8)
        n = np.zeros(b, np.int32)
        _check(lib().slamit_orb_extract_batch(self._h, _np_ptr(frames), ww, ww * hh, b, _np_ptr(kps), _np_ptr(desc),
                                              cap, _np_ptr(n)), "slamit_orb_extract_batch")
        return [kps[i, :n[i]].copy() for i in range(b)], [desc[i, :n[i]].copy() for i in range(b)]

    def extract_batch_dev(self, d_frames, d_kps, d_desc, d_n, stream=None):
        """torch uint8 CUDA tensor (B,H,W) -> fills d_kps (B,cap,7 float32 view), d_desc (B,cap,32), d_n (B)."""
        b, hh, ww = d_frames.shape
        self._bind(ww, hh, b)
        cap = d_kps.shape[1]
        _check(lib().slamit_orb_extract_batch_dev(
            self._h, d_frames.data_ptr(), d_frames.stride(1), d_frames.stride(0), b, d_kps.data_ptr(),
            d_desc.data_ptr(), cap, d_n.data_ptr(), stream), "slamit_orb_extract_batch_dev")

    STAGES = ("resize", "fast", "octree", "angle", "blur", "describe")

    def profile(self, enable):
        """Returns {stage: (total_ms, calls)} accumulated since the last call; sets recording."""
        ms = np.zeros(6, np.float32)
        calls = np.zeros(6, np.int32)
        _check(lib().slamit_orb_profile(self._h, int(enable), _np_ptr(ms), _np_ptr(calls), 6), "slamit_orb_profile")
        return {s: (float(ms[i]), int(calls[i])) for i, s in enumerate(self.STAGES)}

    def level(self, frame, level):
        """mvImagePyramid[level] of `frame` of the last call, padded plane (h+38, w+38)."""
        w, h = C.c_int(), C.c_int()
        _check(lib().slamit_orb_level(self._h, frame, level, None, 0, C.byref(w), C.byref(h)), "slamit_orb_level")
        out = np.zeros((h.value + 38, w.value + 38), np.uint8)
        _check(lib().slamit_orb_level(self._h, frame, level, _np_ptr(out), out.size, C.byref(w), C.byref(h)),
               "slamit_orb_level")
        return out

    def pyramid_view(self):
        """slamit_pyramid_view of the last extract call: where its planes lie in HBM (valid until the next call)."""
        v = PyramidView()
        if self._h is None:
            raise SlamitError("slamit_orb_pyramid_view failed (-4): no extract call yet")
        _check(lib().slamit_orb_pyramid_view(self._h, C.byref(v)), "slamit_orb_pyramid_view")
        return v

    def blurred(self, frame, level):
        """The blurred level (h, w) the descriptors of `frame` of the last call were sampled from."""
        w, h = C.c_int(), C.c_int()
        _check(lib().slamit_orb_debug_blurred(self._h, frame, level, None, 0, C.byref(w), C.byref(h)), "slamit_orb_debug_blurred")
        out = np.zeros((h.value, w.value), np.uint8)
        _check(lib().slamit_orb_debug_blurred(self._h, frame, level, _np_ptr(out), out.size, C.byref(w), C.byref(h)),
               "slamit_orb_debug_blurred")
        return out

    def debug_candidates(self, frame, level):
        n = C.c_int()
        _check(lib().slamit_orb_debug_candidates(self._h, frame, level, None, 0, C.byref(n)), "debug_candidates")
        out = np.zeros((max(n.value, 1), 3), np.int32)
        _check(lib().slamit_orb_debug_candidates(self._h, frame, level, _np_ptr(out), n.value, C.byref(n)),
               "debug_candidates")
        return out[:n.value]

    def debug_octree_path(self, frame, level):
        """(passes served from the path table, whether the workgroup left it and walked the keys) of the last call's octree pass."""
        w = C.c_int()
        _check(lib().slamit_orb_debug_octree_path(self._h, frame, level, C.byref(w)), "debug_octree_path")
        return w.value & 0xFF, bool(w.value & 0x100)


GRID_COLS, GRID_ROWS = 64, 48   # FRAME_GRID_COLS / FRAME_GRID_ROWS (include/Frame.h:40-41)


class Frame:
    """The part of ORB_SLAM2::Frame's constructor that follows the extractor (src/Frame.cc:84-117): image bounds,
    UndistortKeyPoints, AssignFeaturesToGrid.  cam9 = fx fy cx cy k1 k2 p1 p2 k3."""

    @staticmethod
    def undistort_points(cam9, xy, device=0):
        cam = Camera(*[float(v) for v in cam9])
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.zeros_like(xy)
        _check(lib().slamit_undistort_points(device, C.byref(cam), _np_ptr(xy), len(xy), _np_ptr(out)), "slamit_undistort_points")
        return out

    @staticmethod
    def ComputeImageBounds(cam9, cols, rows, device=0):
        """(mnMinX, mnMaxX, mnMinY, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv), Frame.cc:561-590, :113-118."""
        f32 = np.float32
        if f32(cam9[4]) != 0:
            m = Frame.undistort_points(cam9, [[0, 0], [cols, 0], [0, rows], [cols, rows]], device)
            b = (min(m[0, 0], m[2, 0]), max(m[1, 0], m[3, 0]), min(m[0, 1], m[1, 1]), max(m[2, 1], m[3, 1]))
        else:
            b = (f32(0), f32(cols), f32(0), f32(rows))
        b = tuple(f32(v) for v in b)
        return b + (f32(GRID_COLS) / f32(b[1] - b[0]), f32(GRID_ROWS) / f32(b[3] - b[2]))

    @staticmethod
    def finish(cam9, kps, min_x, min_y, inv_w, inv_h, device=0):
        """UndistortKeyPoints + AssignFeaturesToGrid: (mvKeysUn, cell_start[3073], cell_items)."""
        cam = Camera(*[float(v) for v in cam9])
        kps = np.ascontiguousarray(kps)
        n = len(kps)
        un = np.zeros(max(n, 1), KP_DTYPE)
        start, items = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int32), np.zeros(max(n, 1), np.int32)
        _check(lib().slamit_frame_finish(device, C.byref(cam), _np_ptr(kps), n, float(min_x), float(min_y), float(inv_w),
                                         float(inv_h), _np_ptr(un), _np_ptr(start), _np_ptr(items)), "slamit_frame_finish")
        return un[:n], start, items[:start[-1]]

    @staticmethod
    def finish_batch_dev(cam9, d_kps, d_n, min_x, min_y, inv_w, inv_h, d_kps_un, d_cell_start, d_cell_items, device=0, stream=None):
        """torch tensors in the extractor's layout: d_kps (B, cap, 7) float32 view of cv::KeyPoint records."""
        cam = Camera(*[float(v) for v in cam9])
        b, cap = d_kps.shape[0], d_kps.shape[1]
        _check(lib().slamit_frame_finish_batch_dev(device, C.byref(cam), d_kps.data_ptr(), d_n.data_ptr(), cap, b, float(min_x),
                                                   float(min_y), float(inv_w), float(inv_h), d_kps_un.data_ptr(),
                                                   d_cell_start.data_ptr(), d_cell_items.data_ptr(), stream),
               "slamit_frame_finish_batch_dev")


class ORBmatcher:
    TH_HIGH = 100      # ORBmatcher.cc:37
    TH_LOW = 50        # :38
    HISTO_LENGTH = 30  # :39

    def __init__(self, nnratio=0.6, checkOri=True):
        self.mfNNratio = nnratio
        self.mbCheckOrientation = checkOri

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8).reshape(1, 32)
        b = np.ascontiguousarray(b, np.uint8).reshape(1, 32)
        return int(ORBmatcher.distance_matrix(a, b)[0, 0])

    @staticmethod
    def distance_matrix(q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        out = np.zeros((len(q), len(t)), np.uint16)
        _check(lib().slamit_hamming_matrix(_np_ptr(q), len(q), _np_ptr(t), len(t), _np_ptr(out)), "slamit_hamming_matrix")
        return out

    @staticmethod
    def best2(q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        idx, best, second = (np.zeros(len(q), np.int32) for _ in range(3))
        _check(lib().slamit_hamming_best2(_np_ptr(q), len(q), _np_ptr(t), len(t), _np_ptr(idx), _np_ptr(best),
                                          _np_ptr(second)), "slamit_hamming_best2")
        return idx, best, second

    @staticmethod
    def distinctive(desc, offsets):
        """MapPoint::ComputeDistinctiveDescriptors, batched: returns (best row per point, its median)."""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        offsets = np.ascontiguousarray(offsets, np.int32)
        n = len(offsets) - 1
        idx, med = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        _check(lib().slamit_distinctive_batch(_np_ptr(desc), _np_ptr(offsets), n, _np_ptr(idx), _np_ptr(med)),
               "slamit_distinctive_batch")
        return idx[:n], med[:n]

    @staticmethod
    def guided_search(frame, queries, th_dist=100, use_ratio=True, nnratio=0.8, device=0, chi2_gate=0.0, inv_level_sigma2=None, mode=0,
                      stereo=None):
        """The loop body of ORBmatcher::SearchByProjection (ORBmatcher.cc:47-131, :1332-1474) for all
        queries in order: window query over the frame grid, best/second Hamming, accept, mark taken.
        frame: dict kp_xy (n,2) f32, kp_octave (n) i32, desc (n,32) u8, kp_taken (n) u8, min_x, min_y,
        inv_w, inv_h.  queries: dict uvr (m,3) f32, level_min, level_max (m) i32, desc (m,32) u8,
        optional valid / takes (m) u8.  stereo: None (the monocular call), or a dict er_mode (SEARCH_ER_*), kp_ur (n) f32 = mvuRight,
        q_ur f32 with query q at q_ur[q * q_ur_stride], q_ur_stride = 1, chi2_gate_stereo = 7.8: the right-image gate of
        slamit_guided_search_stereo.  Returns (match_kp[m], nmatches, out4[m,4])."""
        f = dict(kp_xy=np.ascontiguousarray(frame["kp_xy"], np.float32).reshape(-1, 2),
                 kp_octave=np.ascontiguousarray(frame["kp_octave"], np.int32),
                 desc=np.ascontiguousarray(frame["desc"], np.uint8).reshape(-1, 32),
                 kp_taken=np.ascontiguousarray(frame["kp_taken"], np.uint8))
        uvr = np.ascontiguousarray(queries["uvr"], np.float32).reshape(-1, 3)
        m, n = len(uvr), len(f["kp_xy"])
        q = dict(level_min=np.ascontiguousarray(queries["level_min"], np.int32),
                 level_max=np.ascontiguousarray(queries["level_max"], np.int32),
                 desc=np.ascontiguousarray(queries["desc"], np.uint8).reshape(-1, 32),
                 valid=np.ascontiguousarray(queries.get("valid", np.ones(m)), np.uint8),
                 takes=np.ascontiguousarray(queries.get("takes", np.ones(m)), np.uint8))
        for k, a in list(f.items())[1:]:
            if len(a) != n:
                raise SlamitError("guided_search: frame[%s] has %d rows, expected %d" % (k, len(a), n))
        for k, a in q.items():
            if len(a) != m:
                raise SlamitError("guided_search: queries[%s] has %d rows, expected %d" % (k, len(a), m))
        fv = FrameView(n, _np_ptr(f["kp_xy"]), _np_ptr(f["kp_octave"]), _np_ptr(f["desc"]), _np_ptr(f["kp_taken"]),
                       frame["min_x"], frame["min_y"], frame["inv_w"], frame["inv_h"])
        sq = SearchQueries(m, _np_ptr(uvr), _np_ptr(q["level_min"]), _np_ptr(q["level_max"]), _np_ptr(q["desc"]),
                           _np_ptr(q["valid"]), _np_ptr(q["takes"]))
        rule = _search_rule(th_dist, use_ratio, nnratio, chi2_gate, inv_level_sigma2, mode)
        match = np.full(max(m, 1), -1, np.int32)
        out4 = np.zeros((4, max(m, 1)), np.int32)
        nm = C.c_int32(0)
        if stereo is not None:
            stride = int(stereo.get("q_ur_stride", 1))
            kur = np.ascontiguousarray(stereo["kp_ur"], np.float32).reshape(-1) if stereo.get("kp_ur") is not None else None
            qur = np.ascontiguousarray(stereo["q_ur"], np.float32).reshape(-1) if stereo.get("q_ur") is not None else None
            if int(stereo["er_mode"]) != SEARCH_ER_NONE:
                if kur is not None and len(kur) != n:
                    raise SlamitError("guided_search: stereo[kp_ur] has %d entries, expected %d" % (len(kur), n))
                if qur is not None and stride >= 1 and m and len(qur) < (m - 1) * stride + 1:
                    raise SlamitError("guided_search: stereo[q_ur] has %d entries, %d queries of stride %d" % (len(qur), m, stride))
            st = SearchStereo(int(stereo["er_mode"]), float(stereo.get("chi2_gate_stereo", 7.8)), _np_ptr(kur) if kur is not None and len(kur) else None,
                              _np_ptr(qur) if qur is not None and len(qur) else None, stride)
            _check(lib().slamit_guided_search_stereo(device, C.byref(fv), C.byref(sq), C.byref(rule), C.byref(st), _np_ptr(match), C.byref(nm),
                                                     _np_ptr(out4[0]), _np_ptr(out4[1]), _np_ptr(out4[2]), _np_ptr(out4[3])),
                   "slamit_guided_search_stereo")
            return match[:m], nm.value, out4[:, :m].T.copy()
        _check(lib().slamit_guided_search(device, C.byref(fv), C.byref(sq), C.byref(rule), _np_ptr(match), C.byref(nm),
                                          _np_ptr(out4[0]), _np_ptr(out4[1]), _np_ptr(out4[2]), _np_ptr(out4[3])),
               "slamit_guided_search")
        return match[:m], nm.value, out4[:, :m].T.copy()

    @staticmethod
    def guided_search_batch_dev(t, bounds, th_dist=100, use_ratio=True, nnratio=0.8, device=0, stream=None, chi2_gate=0.0,
                                inv_level_sigma2=None, stereo=None):
        """Batched device form.  t: dict of torch CUDA tensors n (B) i32, kps_un (B, kp_cap, 7) f32 view of cv::KeyPoint,
        desc (B, kp_cap, 32) u8, kp_taken (B, kp_cap) u8, m (B) i32, uvr (B, q_cap, 3) f32, level_min / level_max
        (B, q_cap) i32, qdesc (B, q_cap, 32) u8, valid / takes (B, q_cap) u8, match_kp (B, q_cap) i32, nmatches (B) i32,
        out4 (B, q_cap, 4) i32 or None, workspace (bytes,) u8.  bounds = (min_x, min_y, inv_w, inv_h).  stereo: None, or a dict
        er_mode, kp_ur (B, kp_cap) f32 tensor, q_ur f32 tensor whose element (f * q_cap + q) * q_ur_stride is query q of frame f (it
        may be a view into frustum_batch_dev's proj at offset 2, with q_ur_stride = 3), q_ur_stride = 1, chi2_gate_stereo = 7.8."""
        b, kp_cap, q_cap = t["kps_un"].shape[0], t["kps_un"].shape[1], t["uvr"].shape[1]
        sb = SearchBatch(b, kp_cap, q_cap, t["n"].data_ptr(), t["kps_un"].data_ptr(), t["desc"].data_ptr(), t["kp_taken"].data_ptr(),
                         float(bounds[0]), float(bounds[1]), float(bounds[2]), float(bounds[3]), t["m"].data_ptr(), t["uvr"].data_ptr(),
                         t["level_min"].data_ptr(), t["level_max"].data_ptr(), t["qdesc"].data_ptr(), t["valid"].data_ptr(),
                         t["takes"].data_ptr())
        rule = _search_rule(th_dist, use_ratio, nnratio, chi2_gate, inv_level_sigma2)
        out4 = t.get("out4")
        if stereo is not None:
            st = SearchStereoDev(int(stereo["er_mode"]), float(stereo.get("chi2_gate_stereo", 7.8)),
                                 stereo["kp_ur"].data_ptr() if stereo.get("kp_ur") is not None else None,
                                 stereo["q_ur"].data_ptr() if stereo.get("q_ur") is not None else None, int(stereo.get("q_ur_stride", 1)))
            _check(lib().slamit_guided_search_stereo_batch_dev(device, C.byref(sb), C.byref(rule), C.byref(st), t["match_kp"].data_ptr(),
                                                               t["nmatches"].data_ptr(), out4.data_ptr() if out4 is not None else None,
                                                               t["workspace"].data_ptr(), t["workspace"].numel(), stream),
                   "slamit_guided_search_stereo_batch_dev")
            return
        _check(lib().slamit_guided_search_batch_dev(device, C.byref(sb), C.byref(rule), t["match_kp"].data_ptr(), t["nmatches"].data_ptr(),
                                                    out4.data_ptr() if out4 is not None else None, t["workspace"].data_ptr(),
                                                    t["workspace"].numel(), stream), "slamit_guided_search_batch_dev")

    @staticmethod
    def guided_search_workspace(nframes, q_cap):
        return int(lib().slamit_guided_search_workspace(nframes, q_cap))

    @staticmethod
    def rotation_check_batch_dev(t, device=0, stream=None):
        """The rotation-consistency check of SearchByProjection(CurrentFrame, LastFrame, ...) (ORBmatcher.cc:1430-1471) on what
        guided_search_batch_dev left on the device.  t: its tensors n (B) i32, kps_un (B, kp_cap, 7) f32, m (B) i32, match_kp
        (B, q_cap) i32, nmatches (B) i32 (updated in place), plus qangle (B, q_cap) f32 (the query keypoints' angles) and the outputs
        kp_query (B, kp_cap) i32 (the query that owns each keypoint, or -1) and bins (B, 3) i32.  Asynchronous on `stream`."""
        b, kp_cap, q_cap = t["kps_un"].shape[0], t["kps_un"].shape[1], t["match_kp"].shape[1]
        for key, count in (("n", b), ("m", b), ("nmatches", b), ("bins", 3 * b), ("match_kp", b * q_cap), ("qangle", b * q_cap), ("kp_query", b * kp_cap)):
            if t[key].numel() != count or not t[key].is_contiguous():
                raise SlamitError("rotation_check_batch_dev: %s is not a contiguous array of %d entries" % (key, count))
        rec = RotationBatch(b, kp_cap, q_cap, t["n"].data_ptr(), t["kps_un"].data_ptr(), t["m"].data_ptr(), t["match_kp"].data_ptr(),
                            t["qangle"].data_ptr(), t["kp_query"].data_ptr(), t["nmatches"].data_ptr(), t["bins"].data_ptr())
        _check(lib().slamit_rotation_check_batch_dev(device, C.byref(rec), stream), "slamit_rotation_check_batch_dev")

    @staticmethod
    def search_for_initialization(f1, prev_xy, f2, window=100, nnratio=0.9, th_low=50, device=0):
        """ORBmatcher::SearchForInitialization's matching loop (ORBmatcher.cc:409-474) as guided-search mode 1: queries =
        F1's level-0 keypoints at vbPrevMatched, window `window`, level [0, 0].  Returns (vnMatches12, nmatches, accepted-at-turn)."""
        o1 = np.ascontiguousarray(f1["kp_octave"], np.int32)
        n1 = len(o1)
        pv = np.ascontiguousarray(prev_xy, np.float32).reshape(-1, 2)
        q = dict(uvr=np.concatenate([pv, np.full((n1, 1), float(window), np.float32)], 1), level_min=np.zeros(n1, np.int32),
                 level_max=np.zeros(n1, np.int32), desc=f1["desc"], valid=(o1 <= 0).astype(np.uint8), takes=np.zeros(n1, np.uint8))
        frame = dict(f2, kp_taken=np.zeros(len(np.asarray(f2["kp_octave"])), np.uint8))
        m12, nm, out4 = ORBmatcher.guided_search(frame, q, th_low, False, nnratio, device=device, mode=1)
        return m12, nm, out4[:, 1].copy()   # the level slot carries the keypoint accepted at the query's own turn

    @staticmethod
    def bow_search(side1, side2, groups, mode=0, th=50, th_inclusive=True, nnratio=0.6, epi=None, device=0, stereo=None):
        """The matching loops of SearchByBoW (mode 0; ORBmatcher.cc:161-290, 526-657) and SearchForTriangulation (mode 1;
        :659-826) over vocabulary-node groups.  side1 / side2: dicts with desc (n, 32), optional valid (n) and, for mode 1,
        kp_xy (n, 2) (+ kp_octave on side 2); groups: dict q_ptr, q_idx, c_ptr, c_idx (CSR per common node); epi (mode 1):
        dict F12 (9, row-major), ex, ey, scale_factor (16), level_sigma2 (16).  Returns (match12, dist12, nmatches)
        before the rotation-histogram filter.  stereo (mode 1 only): dict ur1 (n1), ur2 (n2) = mvuRight of the two keyframes and
        only_stereo = bOnlyStereo; None is the monocular search."""
        d1 = np.ascontiguousarray(side1["desc"], np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(side2["desc"], np.uint8).reshape(-1, 32)
        n1, n2 = len(d1), len(d2)
        v1 = None if side1.get("valid") is None else np.ascontiguousarray(side1["valid"], np.uint8)
        v2 = None if side2.get("valid") is None else np.ascontiguousarray(side2["valid"], np.uint8)
        qp, qi, cp, ci = (np.ascontiguousarray(groups[k], np.int32) for k in ("q_ptr", "q_idx", "c_ptr", "c_idx"))
        g = BowGroups(len(qp) - 1, qp.ctypes.data, qi.ctypes.data, cp.ctypes.data, ci.ctypes.data)
        rule = BowRule()
        rule.mode, rule.th, rule.th_inclusive, rule.nnratio = int(mode), int(th), int(bool(th_inclusive)), float(nnratio)
        keep = []
        if mode == 1:
            k1 = np.ascontiguousarray(side1["kp_xy"], np.float32).reshape(-1, 2)
            k2 = np.ascontiguousarray(side2["kp_xy"], np.float32).reshape(-1, 2)
            o2 = np.ascontiguousarray(side2["kp_octave"], np.int32)
            keep = [k1, k2, o2]
            rule.F12 = (C.c_float * 9)(*[float(v) for v in np.asarray(epi["F12"], np.float32).reshape(9)])
            rule.ex, rule.ey = float(np.float32(epi["ex"])), float(np.float32(epi["ey"]))
            rule.kp1_xy, rule.kp2_xy, rule.kp2_octave = k1.ctypes.data, k2.ctypes.data, o2.ctypes.data
            rule.scale_factor = (C.c_float * 16)(*[float(v) for v in list(epi["scale_factor"])[:16] + [1.0] * (16 - len(epi["scale_factor"]))])
            rule.level_sigma2 = (C.c_float * 16)(*[float(v) for v in list(epi["level_sigma2"])[:16] + [1.0] * (16 - len(epi["level_sigma2"]))])
        m12, dd = np.full(max(n1, 1), -1, np.int32), np.full(max(n1, 1), 256, np.int32)
        nm = C.c_int32(0)
        if stereo is None:
            _check(lib().slamit_bow_search(device, _np_ptr(d1), n1, _np_ptr(v1) if v1 is not None else None, _np_ptr(d2), n2,
                                           _np_ptr(v2) if v2 is not None else None, C.byref(g), C.byref(rule), _np_ptr(m12),
                                           _np_ptr(dd), C.byref(nm)), "slamit_bow_search")
        else:
            u1, u2 = np.ascontiguousarray(stereo["ur1"], np.float32).reshape(-1), np.ascontiguousarray(stereo["ur2"], np.float32).reshape(-1)
            if len(u1) != n1 or len(u2) != n2:
                raise SlamitError("bow_search: stereo ur1 / ur2 do not have n1 / n2 entries")
            st = BowStereo(u1.ctypes.data if n1 else None, u2.ctypes.data if n2 else None, int(bool(stereo.get("only_stereo", False))))
            _check(lib().slamit_bow_search_stereo(device, _np_ptr(d1), n1, _np_ptr(v1) if v1 is not None else None, _np_ptr(d2), n2,
                                                  _np_ptr(v2) if v2 is not None else None, C.byref(g), C.byref(rule), C.byref(st),
                                                  _np_ptr(m12), _np_ptr(dd), C.byref(nm)), "slamit_bow_search_stereo")
        del keep
        return m12[:n1], dd[:n1], nm.value

    def match(self, q, t, th=None):
        """All-pairs match with the reference's acceptance rule: best <= th and best < nnratio*second
        (ORBmatcher.cc:1430-1436 style). Returns query indices and their matched train indices."""
        th = self.TH_LOW if th is None else th
        idx, best, second = self.best2(q, t)
        ok = (best <= th) & (best.astype(np.float32) < np.float32(self.mfNNratio) * second.astype(np.float32))
        return np.nonzero(ok)[0], idx[ok]

    @staticmethod
    def best2_batch_dev(d_q, d_nq, d_t, d_nt, d_idx, d_best, d_second, max_n, device=0, stream=None):
        """torch tensors: d_q/d_t (P, cap, 32) uint8, d_nq/d_nt (P) int32, outputs (P, cap) int32."""
        p = d_q.shape[0]
        _check(lib().slamit_hamming_best2_batch_dev(
            d_q.data_ptr(), d_nq.data_ptr(), d_q.stride(0), d_t.data_ptr(), d_nt.data_ptr(), d_t.stride(0), p, max_n,
            d_idx.data_ptr(), d_best.data_ptr(), d_second.data_ptr(), d_idx.stride(0), device, stream),
            "slamit_hamming_best2_batch_dev")


class ORBVocabulary:
    """ORBVocabulary (include/ORBVocabulary.h: DBoW2's TemplatedVocabulary over ORB descriptors) on one GPU: the transform of
    Frame::ComputeBoW / KeyFrame::ComputeBoW.  Node and word ids are the reference's (text-file order)."""

    def __init__(self, handle, device):
        self._h, self.device = handle, device

    @classmethod
    def from_arrays(cls, k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0, device=0):
        """Entry i of the arrays is node i + 1 (0 = root): parent (n) i32, is_leaf (n) u8, desc (n, 32) u8, weight (n) f64."""
        parent = np.ascontiguousarray(parent, np.int32)
        n = len(parent)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        weight = np.ascontiguousarray(weight, np.float64)
        if len(is_leaf) != n or len(desc) != n or len(weight) != n:
            raise SlamitError("ORBVocabulary.from_arrays: parent / is_leaf / desc / weight do not have the same length")
        d = VocDesc(int(k), int(L), int(scoring), int(weighting), n, parent.ctypes.data, is_leaf.ctypes.data, desc.ctypes.data,
                    weight.ctypes.data)
        h = C.c_void_p()
        _check(lib().slamit_voc_create(C.byref(d), device, C.byref(h)), "slamit_voc_create")
        return cls(h, device)

    @classmethod
    def load_text(cls, path, device=0):
        """TemplatedVocabulary::loadFromTextFile."""
        h = C.c_void_p()
        _check(lib().slamit_voc_load_text(os.fsencode(path), device, C.byref(h)), "slamit_voc_load_text")
        return cls(h, device)

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().slamit_voc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """{"k", "L", "n_nodes" (without the root), "n_words"}."""
        v = [C.c_int32() for _ in range(4)]
        _check(lib().slamit_voc_info(self._h, *[C.byref(x) for x in v]), "slamit_voc_info")
        return dict(zip(("k", "L", "n_nodes", "n_words"), (x.value for x in v)))

    def transform(self, desc, levelsup=4, bow=True, fv=True):
        """One frame's descriptors (n, 32) u8 -> dict: word_id (n; -1 = stopped word), node_id (n); with bow: bow_word, bow_value
        (the BowVector: unique word ids ascending, normalised values); with fv: fv_node, fv_ptr, fv_items (the FeatureVector as
        CSR: features of node j are fv_items[fv_ptr[j]:fv_ptr[j + 1]])."""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        m = max(n, 1)
        word, node = np.zeros(m, np.int32), np.zeros(m, np.int32)
        bn, fn = C.c_int32(0), C.c_int32(0)
        bw, bv = np.zeros(m, np.int32), np.zeros(m, np.float64)
        fnode, fptr, fitems = np.zeros(m, np.int32), np.zeros(m + 1, np.int32), np.zeros(m, np.int32)
        _check(lib().slamit_voc_transform(
            self._h, _np_ptr(desc), n, int(levelsup), _np_ptr(word), _np_ptr(node),
            C.byref(bn) if bow else None, _np_ptr(bw) if bow else None, _np_ptr(bv) if bow else None,
            C.byref(fn) if fv else None, _np_ptr(fnode) if fv else None, _np_ptr(fptr) if fv else None,
            _np_ptr(fitems) if fv else None), "slamit_voc_transform")
        out = {"word_id": word[:n], "node_id": node[:n]}
        if bow:
            out.update(bow_word=bw[:bn.value].copy(), bow_value=bv[:bn.value].copy())
        if fv:
            out.update(fv_node=fnode[:fn.value].copy(), fv_ptr=fptr[:fn.value + 1].copy(), fv_items=fitems[:fptr[fn.value]].copy())
        return out

    @staticmethod
    def transform_workspace(nframes, cap):
        return int(lib().slamit_voc_transform_workspace(nframes, cap))

    def transform_batch_dev(self, t, levelsup=4, stream=None):
        """Batched device form.  t: dict of torch CUDA tensors desc (B, cap, 32) u8 and n (B) i32 as extract_batch_dev writes them,
        word_id / node_id (B, cap) i32, workspace (bytes,) u8, and optionally (as a whole) bow_n (B) i32, bow_word (B, cap) i32,
        bow_value (B, cap) f64 and / or fv_n (B) i32, fv_node (B, cap) i32, fv_ptr (B, cap + 1) i32, fv_items (B, cap) i32.
        Asynchronous; a frame whose n lies outside [0, cap] gets bow_n = fv_n = -1."""
        b, cap = t["desc"].shape[0], t["desc"].shape[1]
        opt = [t[k].data_ptr() if t.get(k) is not None else None
               for k in ("bow_n", "bow_word", "bow_value", "fv_n", "fv_node", "fv_ptr", "fv_items")]
        _check(lib().slamit_voc_transform_batch_dev(
            self._h, t["desc"].data_ptr(), t["n"].data_ptr(), cap, b, int(levelsup), t["word_id"].data_ptr(), t["node_id"].data_ptr(),
            *opt, t["workspace"].data_ptr(), t["workspace"].numel(), stream), "slamit_voc_transform_batch_dev")

    @staticmethod
    def groups(fv1, fv2):
        """The vocabulary nodes two FeatureVectors share, ascending -- what the lower_bound walk of SearchByBoW visits
        (ORBmatcher.cc:178-270) -- as the groups dict ORBmatcher.bow_search takes.  fv1 / fv2: dicts with fv_node, fv_ptr, fv_items."""
        n1, n2 = np.asarray(fv1["fv_node"]), np.asarray(fv2["fv_node"])
        _, i1, i2 = np.intersect1d(n1, n2, assume_unique=True, return_indices=True)
        g = {"q_ptr": [0], "q_idx": [], "c_ptr": [0], "c_idx": []}
        for a, b in zip(i1, i2):
            g["q_idx"].extend(fv1["fv_items"][fv1["fv_ptr"][a]:fv1["fv_ptr"][a + 1]])
            g["c_idx"].extend(fv2["fv_items"][fv2["fv_ptr"][b]:fv2["fv_ptr"][b + 1]])
            g["q_ptr"].append(len(g["q_idx"]))
            g["c_ptr"].append(len(g["c_idx"]))
        return {k: np.asarray(v, np.int32) for k, v in g.items()}


def _min_common_words(max_common):
    """int minCommonWords = maxCommonWords*0.8f (KeyFrameDatabase.cc:129, :254): the product in float, truncated."""
    return int(np.float32(max_common) * np.float32(0.8))


class KeyFrameDatabase:
    """KeyFrameDatabase (include/KeyFrameDatabase.h) on one GPU.  Keyframes are slots; the device holds their BowVectors and compares
    a query with all of them (query), the rest of DetectLoopCandidates / DetectRelocalizationCandidates is host logic in the
    reference's order over the per-slot members the reference keeps in KeyFrame (mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery,
    mnRelocWords, mRelocScore: self.state, reset when a slot is added; the two scores start at 0.0f, which the reference leaves
    uninitialised)."""

    STATE_DTYPE = np.dtype([("mnLoopQuery", "<i8"), ("mnLoopWords", "<i4"), ("mLoopScore", "<f4"),
                            ("mnRelocQuery", "<i8"), ("mnRelocWords", "<i4"), ("mRelocScore", "<f4")])

    def __init__(self, max_kf, max_words, device=0):
        h = C.c_void_p()
        _check(lib().slamit_kfdb_create(int(max_kf), int(max_words), device, C.byref(h)), "slamit_kfdb_create")
        self._h, self.device, self.max_kf, self.max_words = h, device, int(max_kf), int(max_words)
        self.state = np.zeros(self.max_kf, self.STATE_DTYPE)
        self._next_loop_id = 1

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().slamit_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """{"max_kf", "max_words", "n_live"}."""
        v = [C.c_int32() for _ in range(3)]
        _check(lib().slamit_kfdb_info(self._h, *[C.byref(x) for x in v]), "slamit_kfdb_info")
        return dict(zip(("max_kf", "max_words", "n_live"), (x.value for x in v)))

    def add(self, bow_word, bow_value):
        """A keyframe's BowVector (word ids strictly ascending, values) -> its slot, the lowest free one."""
        w, v = np.ascontiguousarray(bow_word, np.int32), np.ascontiguousarray(bow_value, np.float64)
        if len(w) != len(v):
            raise SlamitError("KeyFrameDatabase.add: bow_word and bow_value do not have the same length")
        s = C.c_int32(-1)
        _check(lib().slamit_kfdb_add(self._h, _np_ptr(w), _np_ptr(v), len(w), C.byref(s)), "slamit_kfdb_add")
        self.state[s.value] = 0
        return s.value

    def add_dev(self, bow_n, bow_word, bow_value, stream=None):
        """The same from torch CUDA tensors as transform_batch_dev wrote one frame: bow_n (1,) i32, bow_word (cap,) i32, bow_value
        (cap,) f64.  Asynchronous."""
        s = C.c_int32(-1)
        _check(lib().slamit_kfdb_add_dev(self._h, bow_n.data_ptr(), bow_word.data_ptr(), bow_value.data_ptr(), stream, C.byref(s)),
               "slamit_kfdb_add_dev")
        self.state[s.value] = 0
        return s.value

    def erase(self, slot):
        _check(lib().slamit_kfdb_erase(self._h, int(slot)), "slamit_kfdb_erase")

    def clear(self):
        _check(lib().slamit_kfdb_clear(self._h), "slamit_kfdb_clear")

    def query(self, bow_word, bow_value):
        """-> (common i32, first_word i32, seq i64, score f64), max_kf entries each, by slot (slamit.h)."""
        w, v = np.ascontiguousarray(bow_word, np.int32), np.ascontiguousarray(bow_value, np.float64)
        if len(w) != len(v):
            raise SlamitError("KeyFrameDatabase.query: bow_word and bow_value do not have the same length")
        common, first = np.zeros(self.max_kf, np.int32), np.zeros(self.max_kf, np.int32)
        seq, score = np.zeros(self.max_kf, np.int64), np.zeros(self.max_kf, np.float64)
        _check(lib().slamit_kfdb_query(self._h, _np_ptr(w), _np_ptr(v), len(w), _np_ptr(common), _np_ptr(first), _np_ptr(seq), _np_ptr(score)),
               "slamit_kfdb_query")
        return common, first, seq, score

    def query_batch_dev(self, t, stream=None):
        """t: dict of torch CUDA tensors bow_n (nq) i32, bow_word (nq, cap) i32, bow_value (nq, cap) f64 and the outputs common,
        first_word (nq, max_kf) i32, score (nq, max_kf) f64.  Asynchronous."""
        nq, cap = t["bow_word"].shape[0], t["bow_word"].shape[1]
        _check(lib().slamit_kfdb_query_batch_dev(self._h, t["bow_n"].data_ptr(), t["bow_word"].data_ptr(), t["bow_value"].data_ptr(), cap, nq,
                                                 t["common"].data_ptr(), t["first_word"].data_ptr(), t["score"].data_ptr(), stream),
               "slamit_kfdb_query_batch_dev")

    def _sharing(self, query_bow):
        """The slots that share a word with the query, in the order the reference's walk over the inverted file first meets them
        (KeyFrameDatabase.cc:94-112, :219-237): by (first shared word, position in that word's list)."""
        common, first, seq, score = self.query(*query_bow)
        slots = np.flatnonzero(common >= 1)
        return slots[np.lexsort((seq[slots], first[slots]))].tolist(), common, score

    @staticmethod
    def _retain(acc, min_to_retain):
        out, seen = [], set()
        for a, s in acc:                                                    # :191-202, :313-325
            if a > min_to_retain and s not in seen:
                out.append(s)
                seen.add(s)
        return out

    def DetectLoopCandidates(self, query_bow, connected_slots, neighbours, min_score, query_id=None):
        """KeyFrameDatabase::DetectLoopCandidates (:84-206).  query_bow = (bow_word, bow_value) of pKF, connected_slots the slots of
        pKF->GetConnectedKeyFrames(), neighbours[slot] the slots of GetBestCovisibilityKeyFrames(10) of that keyframe in its order,
        query_id pKF->mnId (default: a fresh one).  -> the candidates' slots in the reference's order."""
        if query_id is None:
            query_id, self._next_loop_id = self._next_loop_id, self._next_loop_id + 1
        st, f32 = self.state, np.float32
        min_score = f32(min_score)
        connected = set(int(s) for s in connected_slots)
        order, common, score = self._sharing(query_bow)
        sharing = []
        for s in order:
            if st["mnLoopQuery"][s] != query_id:                            # :101
                if s not in connected:                                      # :104-108
                    st["mnLoopQuery"][s] = query_id
                    st["mnLoopWords"][s] = common[s]
                    sharing.append(s)
                else:
                    st["mnLoopWords"][s] = 1                                # :103 at every meeting, :110 after it
            else:
                st["mnLoopWords"][s] += common[s]                           # :110 alone
        if not sharing:
            return []
        min_common = _min_common_words(max(int(st["mnLoopWords"][s]) for s in sharing))   # :121-129
        scored = []
        for s in sharing:                                                   # :134-148
            if st["mnLoopWords"][s] > min_common:
                si = f32(score[s])                                          # :142 float si = score()
                st["mLoopScore"][s] = si
                if si >= min_score:
                    scored.append((si, s))
        if not scored:
            return []
        acc, best_acc = [], min_score                                       # :154
        for si, s in scored:                                                # :157-182
            best, a, best_s = si, si, s
            for s2 in neighbours[s]:
                if st["mnLoopQuery"][s2] == query_id and st["mnLoopWords"][s2] > min_common:
                    a = f32(a + st["mLoopScore"][s2])
                    if st["mLoopScore"][s2] > best:
                        best_s, best = s2, st["mLoopScore"][s2]
            acc.append((a, best_s))
            if a > best_acc:
                best_acc = a
        return self._retain(acc, f32(f32(0.75) * best_acc))                 # :185

    def DetectRelocalizationCandidates(self, query_bow, query_id, neighbours):
        """KeyFrameDatabase::DetectRelocalizationCandidates (:208-328); query_id is F->mnId.  A neighbour counts when it shares any
        word with this query (:292); its mRelocScore is this query's only if it also passed minCommonWords, else what an earlier
        query left in self.state."""
        st, f32 = self.state, np.float32
        order, common, score = self._sharing(query_bow)
        sharing = []
        for s in order:
            if st["mnRelocQuery"][s] != query_id:                           # :227-234
                st["mnRelocQuery"][s] = query_id
                st["mnRelocWords"][s] = common[s]
                sharing.append(s)
            else:
                st["mnRelocWords"][s] += common[s]
        if not sharing:
            return []
        min_common = _min_common_words(max(int(st["mnRelocWords"][s]) for s in sharing))   # :247-254
        scored = []
        for s in sharing:                                                   # :261-272
            if st["mnRelocWords"][s] > min_common:
                si = f32(score[s])
                st["mRelocScore"][s] = si
                scored.append((si, s))
        if not scored:
            return []
        acc, best_acc = [], f32(0)                                          # :278
        for si, s in scored:                                                # :281-306
            best, a, best_s = si, si, s
            for s2 in neighbours[s]:
                if st["mnRelocQuery"][s2] != query_id:
                    continue
                a = f32(a + st["mRelocScore"][s2])
                if st["mRelocScore"][s2] > best:
                    best_s, best = s2, st["mRelocScore"][s2]
            acc.append((a, best_s))
            if a > best_acc:
                best_acc = a
        return self._retain(acc, f32(f32(0.75) * best_acc))                 # :309


def _ba_problem(arrs):
    keep = {}
    for k, dt in (("kf_pose", np.float64), ("kf_fixed", np.uint8), ("kf_intr", np.float64), ("pt_xyz", np.float64),
                  ("edge_kf", np.int32), ("edge_pt", np.int32), ("edge_uv", np.float64), ("edge_inv_sigma2", np.float64)):
        keep[k] = np.ascontiguousarray(arrs[k], dtype=dt)
    stereo = arrs.get("edge_ur") is not None
    if stereo:   # right-image columns (negative: a monocular edge) and the keyframes' baseline x fx
        keep["edge_ur"] = np.ascontiguousarray(arrs["edge_ur"], dtype=np.float64)
        keep["kf_bf"] = np.ascontiguousarray(arrs["kf_bf"], dtype=np.float64)
        if len(keep["edge_ur"]) != len(keep["edge_kf"]) or len(keep["kf_bf"]) != len(keep["kf_fixed"]):
            raise SlamitError("edge_ur / kf_bf do not match the window's edges / keyframes")
    p = BaProblem(len(keep["kf_fixed"]), len(keep["pt_xyz"]), len(keep["edge_kf"]),
                  *[keep[k].ctypes.data for k in ("kf_pose", "kf_fixed", "kf_intr", "pt_xyz", "edge_kf", "edge_pt",
                                                   "edge_uv", "edge_inv_sigma2")],
                  keep["edge_ur"].ctypes.data if stereo else None, keep["kf_bf"].ctypes.data if stereo else None)
    return p, keep


HUBER_MONO = float(np.float32(np.sqrt(5.991)))  # Optimizer.cc:569 stores sqrt(5.991) in a float
HUBER_STEREO = float(np.float32(np.sqrt(7.815)))  # Optimizer.cc:570


class Optimizer:
    """Optimizer::LocalBundleAdjustment on POD inputs (the KeyFrame/MapPoint gathering of
    Optimizer.cc:456-504 stays with the caller)."""

    MAX_FREE_KF = 341   # SLAMIT_BA_MAX_FREE_KF

    def __init__(self, max_kf=64, max_pt=4096, max_edge=262144, max_batch=1, device=0, max_free_kf=None):
        """max_free_kf: size the reduced system for that many free keyframes apart from max_kf, which then counts free and fixed
        ones together (slamit_ba_create_ex; up to MAX_FREE_KF).  None: slamit_ba_create, max_kf <= 85 keyframes of either kind."""
        h = C.c_void_p()
        if max_free_kf is None:
            _check(lib().slamit_ba_create(max_kf, max_pt, max_edge, max_batch, device, C.byref(h)), "slamit_ba_create")
        else:
            _check(lib().slamit_ba_create_ex(max_kf, max_free_kf, max_pt, max_edge, max_batch, device, C.byref(h)), "slamit_ba_create_ex")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None:
            lib().slamit_ba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def profile(self, on=True):
        """Per-phase timing of the following solves (slamit_ba_profile): events between the phases of every LM slot."""
        _check(lib().slamit_ba_profile(self._h, 1 if on else 0), "slamit_ba_profile")

    def profile_read(self):
        """Phase sums of the last profiled solve: {"phase_ms": {linearize, schur, solve, update, residuals}, "slots", "nwin",
        "schur_exec_mflop"} — the analogue of g2o's G2OBatchStatistics."""
        o = BaProfile()
        _check(lib().slamit_ba_profile_read(self._h, C.byref(o)), "slamit_ba_profile_read")
        return {"phase_ms": dict(zip(BA_PHASES, [float(v) for v in o.phase_ms])), "slots": int(o.slots), "nwin": int(o.nwin),
                "schur_exec_mflop": float(o.schur_exec_mflop)}

    @staticmethod
    def _result(n_kf, n_pt, n_e):
        # (np.empty: the call writes every element of every output or fails; zero-filling 210 KB per window was 4 ms of a 17-ms batch of 64)
        out = {"kf_pose": np.empty((n_kf, 12)), "pt_xyz": np.empty((n_pt, 3)), "edge_chi2": np.empty(n_e),
               "edge_outlier": np.empty(n_e, np.uint8), "edge_stage1_outlier": np.empty(n_e, np.uint8)}
        st = BaStats()
        r = BaResult(out["kf_pose"].ctypes.data, out["pt_xyz"].ctypes.data, out["edge_chi2"].ctypes.data,
                     out["edge_outlier"].ctypes.data, out["edge_stage1_outlier"].ctypes.data, C.addressof(st))
        return r, out, st

    @staticmethod
    def _stats(st):
        n = list(st.n_its)
        return {"n_its": n, "chi2": [st.chi2[s][:n[s]] for s in range(2)],
                "lambda": [st.lambda_[s][:n[s]] for s in range(2)],
                "trials": [st.trials[s][:n[s]] for s in range(2)], "chi2_init": list(st.chi2_init)}

    def LocalBundleAdjustment(self, problem, its_robust=5, its_final=10, huber_delta=HUBER_MONO, chi2_gate=5.991,
                              stop=None, huber_delta_stereo=HUBER_STEREO, chi2_gate_stereo=7.815):
        p, keep = _ba_problem(problem)
        o = BaOpts(its_robust, its_final, huber_delta, chi2_gate, stop.ctypes.data if stop is not None else None,
                   huber_delta_stereo, chi2_gate_stereo)
        r, out, st = self._result(p.n_kf, p.n_pt, p.n_edge)
        _check(lib().slamit_ba_solve(self._h, C.byref(p), C.byref(o), C.byref(r)), "slamit_ba_solve")
        out["stats"] = self._stats(st)
        return out

    @staticmethod
    def OptimizeSim3(problems, device=0):
        """Optimizer::OptimizeSim3 for one problem dict or a list of them (synth.synth_sim3 layout: p1, p2, obs1, obs2,
        inv_sigma2_1, inv_sigma2_2, intr1, intr2, r12, t12, s12, th2, fix_scale).  Returns dict(s) with r12 (3, 3), t12, s12,
        inlier flags, n_inliers, n_its[2], chi2[2]."""
        single = isinstance(problems, dict)
        plist = [problems] if single else list(problems)
        m = len(plist)
        P = (Sim3Problem * m)()
        R = (Sim3Result * m)()
        keep, flags = [], []
        for i, pr in enumerate(plist):
            k = {key: np.ascontiguousarray(pr[key], np.float64) for key in ("p1", "p2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")}
            q = P[i]
            q.n = len(k["inv_sigma2_1"])
            for key, a in k.items():
                setattr(q, key, a.ctypes.data)
            q.intr1 = (C.c_double * 4)(*[float(v) for v in pr["intr1"]])
            q.intr2 = (C.c_double * 4)(*[float(v) for v in pr["intr2"]])
            q.r12 = (C.c_double * 9)(*[float(v) for v in np.asarray(pr["r12"]).reshape(9)])
            q.t12 = (C.c_double * 3)(*[float(v) for v in pr["t12"]])
            q.s12, q.th2, q.fix_scale = float(pr["s12"]), float(pr["th2"]), int(pr["fix_scale"])
            fl = np.zeros(max(q.n, 1), np.uint8)
            R[i].inlier = fl.ctypes.data
            keep.append(k)
            flags.append(fl)
        _check(lib().slamit_sim3_optimize_batch(device, m, P, R), "slamit_sim3_optimize_batch")
        outs = [{"r12": np.array(R[i].r12[:]).reshape(3, 3), "t12": np.array(R[i].t12[:]), "s12": R[i].s12, "inlier": flags[i][:P[i].n].copy(),
                 "n_inliers": R[i].n_inliers, "n_its": list(R[i].n_its), "chi2": list(R[i].chi2)} for i in range(m)]
        del keep
        return outs[0] if single else outs

    @staticmethod
    def PoseOptimization(problems, device=0):
        """Optimizer::PoseOptimization for one problem dict or a list of them (synth.synth_pose layout):
        returns dict(s) with pose (12), outlier flags, n_inliers, n_its[4], chi2[4]."""
        single = isinstance(problems, dict)
        plist = [problems] if single else list(problems)
        n = len(plist)
        P = (PoseProblem * n)()
        R = (PoseResult * n)()
        keep, outs = [], []
        for i, pr in enumerate(plist):
            k = {key: np.ascontiguousarray(pr[key], np.float64) for key in ("pose", "intr", "xw", "uv", "inv_sigma2")}
            m = len(k["inv_sigma2"])
            if pr.get("ur") is not None:
                k["ur"] = np.ascontiguousarray(pr["ur"], np.float64)
                if len(k["ur"]) != m:
                    raise SlamitError("ur does not match the correspondences")
            P[i] = PoseProblem(m, *[k[key].ctypes.data for key in ("pose", "intr", "xw", "uv", "inv_sigma2")],
                               k["ur"].ctypes.data if "ur" in k else None, float(pr.get("bf", 0.0)))
            o = {"pose": np.zeros(12), "outlier": np.zeros(max(m, 1), np.uint8)}
            R[i] = PoseResult(o["pose"].ctypes.data, o["outlier"].ctypes.data, 0)
            keep.append(k)
            outs.append((o, m))
        _check(lib().slamit_pose_optimize_batch(device, n, P, R), "slamit_pose_optimize_batch")
        res = [{"pose": o["pose"], "outlier": o["outlier"][:m].copy(), "n_inliers": R[i].n_inliers,
                "n_its": list(R[i].n_its), "chi2": list(R[i].chi2)} for i, (o, m) in enumerate(outs)]
        return res[0] if single else res

    def LocalBundleAdjustmentBatch(self, problems, its_robust=5, its_final=10, huber_delta=HUBER_MONO,
                                   chi2_gate=5.991, huber_delta_stereo=HUBER_STEREO, chi2_gate_stereo=7.815):
        n = len(problems)
        P = (BaProblem * n)()
        R = (BaResult * n)()
        keeps, outs, sts = [], [], []
        for i, prob in enumerate(problems):
            P[i], keep = _ba_problem(prob)
            keeps.append(keep)
            R[i], out, st = self._result(P[i].n_kf, P[i].n_pt, P[i].n_edge)
            outs.append(out)
            sts.append(st)
        o = BaOpts(its_robust, its_final, huber_delta, chi2_gate, None, huber_delta_stereo, chi2_gate_stereo)
        _check(lib().slamit_ba_solve_batch(self._h, n, P, C.byref(o), R), "slamit_ba_solve_batch")
        for out, st in zip(outs, sts):
            out["stats"] = self._stats(st)
        return outs


class Sim3Solver:
    """Sim3Solver (include/Sim3Solver.h) on POD inputs: the constructor's gathering (Sim3Solver.cc:62-103) stays with the caller,
    who hands over a problem dict in the layout of slamit_sim3_ransac_problem (synth.synth_sim3_ransac): x1, x2 (n, 3) float32,
    max_err1, max_err2 (n) -- see max_error() --, intr1, intr2, fix_scale.  The hypotheses run on the device in one call
    (evaluate), iterate()'s sequential acceptance scan (:183-200) runs here over the device's counts.  `rand_int(lo, hi)` stands
    for DUtils::Random::RandomInt; all mRansacMaxIts triples are drawn when the parameters are set."""

    def __init__(self, problem, rand_int=None, device=0):
        self.problem = problem
        self.N = len(np.asarray(problem["max_err1"]))
        self.device = device
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.best = None            # index of the hypothesis that holds the running best
        self.counts = None          # device results, filled by the first iterate()
        self.accepted = -1          # index of the hypothesis iterate() returned
        if rand_int is None:
            rs = np.random.RandomState(0)
            rand_int = lambda lo, hi: int(rs.randint(lo, hi + 1))   # noqa: E731
        self.rand_int = rand_int
        self.SetRansacParameters()

    @staticmethod
    def max_error(sigma2):
        """mvnMaxError (Sim3Solver.h:78-79) is a vector<size_t>: 9.210 * sigma2 is truncated to an integer before err < max."""
        return np.floor(9.210 * np.asarray(sigma2, np.float32).astype(np.float64)).astype(np.float32)

    @staticmethod
    def ransac_iterations(N, probability, minInliers, maxIterations):
        """mRansacMaxIts of SetRansacParameters (:114-138): float epsilon, ceil(log / log), the minInliers == N case, the clamp."""
        with np.errstate(divide="ignore", invalid="ignore"):
            eps = np.float32(minInliers) / np.float32(N)
            if minInliers == N:
                nit = 1
            else:
                eps3 = math.pow(float(eps), 3)   # pow(float, int) promotes to double
                v = np.ceil(np.log(1 - probability) / np.log(np.float64(1) - eps3))
                nit = int(np.clip(v, -2 ** 31, 2 ** 31 - 1)) if np.isfinite(v) else -2 ** 31   # (int) of an unrepresentable double on x86-64
        return max(1, min(nit, maxIterations))

    @staticmethod
    def sample_triples(N, count, rand_int):
        """The sampler of iterate() (:163-177), with its quirk: the slot overwritten is vAvailableIndices[idx] -- indexed by the
        VALUE drawn, not by the position randi -- so a value can be drawn twice inside a triple."""
        out = np.zeros((count, 3), np.int32)
        for h in range(count):
            avail, size = list(range(N)), N   # a value drawn may lie past the shrunken end: the store then lands in a popped slot
            for i in range(3):
                randi = rand_int(0, size - 1)
                idx = avail[randi]
                out[h, i] = idx
                avail[idx] = avail[size - 1]
                size -= 1
        return out

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.mRansacProb, self.mRansacMinInliers = probability, minInliers
        self.mRansacMaxIts = self.ransac_iterations(self.N, probability, minInliers, maxIterations)
        self.mnIterations = 0
        self.counts = None
        self.triples = self.sample_triples(self.N, min(self.mRansacMaxIts, SIM3_RANSAC_MAX_HYP), self.rand_int) if self.N >= max(minInliers, 3) else np.zeros((0, 3), np.int32)

    @staticmethod
    def evaluate(problems, device=0, want_bits=True):
        """Raw per-hypothesis results of one problem dict (with "triples" (n_hyp, 3)) or a list of them, in ONE device call:
        dict(s) with t12 (n_hyp, 13) float32 = R12 row-major, t12, s12; n_inliers (n_hyp); inlier_bits (n_hyp, (n + 31) // 32)."""
        single = isinstance(problems, dict)
        plist = [problems] if single else list(problems)
        m = len(plist)
        P = (Sim3RansacProblem * m)()
        R = (Sim3RansacResult * m)()
        keep, outs = [], []
        for i, pr in enumerate(plist):
            k = {"x1": np.ascontiguousarray(pr["x1"], np.float32).reshape(-1, 3), "x2": np.ascontiguousarray(pr["x2"], np.float32).reshape(-1, 3),
                 "max_err1": np.ascontiguousarray(pr["max_err1"], np.float32), "max_err2": np.ascontiguousarray(pr["max_err2"], np.float32),
                 "triples": np.ascontiguousarray(pr["triples"], np.int32).reshape(-1, 3)}
            n, nh = len(k["max_err1"]), len(k["triples"])
            if len(k["x1"]) != n or len(k["x2"]) != n or len(k["max_err2"]) != n:
                raise SlamitError("Sim3Solver.evaluate: x1 / x2 / max_err arrays do not have the same length")
            q = P[i]
            q.n, q.n_hyp, q.fix_scale = n, nh, int(pr["fix_scale"])
            for key, a in k.items():
                setattr(q, key, a.ctypes.data)
            q.intr1 = (C.c_float * 4)(*[float(v) for v in pr["intr1"]])
            q.intr2 = (C.c_float * 4)(*[float(v) for v in pr["intr2"]])
            o = {"t12": np.zeros((nh, 13), np.float32), "n_inliers": np.zeros(nh, np.int32)}
            R[i].t12, R[i].n_inliers = o["t12"].ctypes.data, o["n_inliers"].ctypes.data
            if want_bits:
                o["inlier_bits"] = np.zeros((nh, (n + 31) // 32), np.uint32)
                R[i].inlier_bits = o["inlier_bits"].ctypes.data
            keep.append(k)
            outs.append(o)
        _check(lib().slamit_sim3_ransac_batch(device, m, P, R), "slamit_sim3_ransac_batch")
        del keep
        return outs[0] if single else outs

    @staticmethod
    def EvaluateAll(solvers, device=0):
        """Every candidate's hypotheses in one launch (what LoopClosing::ComputeSim3 costs)."""
        todo = [s for s in solvers if s.counts is None]
        res = Sim3Solver.evaluate([dict(s.problem, triples=s.triples) for s in todo], device) if todo else []
        for s, r in zip(todo, res):
            s.t12, s.counts, s.bits = r["t12"], r["n_inliers"], r["inlier_bits"]

    def flags(self, h):
        """mvbInliersi of hypothesis h as a bool array (N)."""
        b = np.unpackbits(self.bits[h].view(np.uint8), bitorder="little")[:self.N]
        return b.astype(bool)

    @staticmethod
    def scan(counts, first, nIterations, mnIterations, mRansacMaxIts, mnBestInliers, mRansacMinInliers):
        """The loop of iterate() (:158-204) over counts[first:]: -> (accepted index or -1, best index or -1 if never updated,
        mnBestInliers, mnIterations, bNoMore).  The best is replaced on >=, the return is on a strict >."""
        best, k, cur = -1, first, 0
        while mnIterations < mRansacMaxIts and cur < nIterations:
            cur += 1
            mnIterations += 1
            c = int(counts[k])
            k += 1
            if c >= mnBestInliers:
                mnBestInliers, best = c, k - 1
                if c > mRansacMinInliers:
                    return k - 1, best, mnBestInliers, mnIterations, False
        return -1, best, mnBestInliers, mnIterations, mnIterations >= mRansacMaxIts

    def iterate(self, nIterations):
        """-> (T12 (4, 4) float32 or None, bNoMore, vbInliers (N) bool, nInliers)."""
        vb = np.zeros(self.N, bool)
        if self.N < self.mRansacMinInliers or self.N < 3:   # (the reference cannot sample three of fewer than three either)
            return None, True, vb, 0
        if self.counts is None:
            Sim3Solver.EvaluateAll([self], self.device)
        acc, best, self.mnBestInliers, self.mnIterations, no_more = self.scan(
            self.counts, self.mnIterations, nIterations, self.mnIterations, self.mRansacMaxIts, self.mnBestInliers, self.mRansacMinInliers)
        if best >= 0:
            self.best = best
        if acc < 0:
            return None, no_more, vb, 0
        self.accepted = acc
        return self.T12(acc), False, self.flags(acc), int(self.counts[acc])

    def find(self):
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n

    def T12(self, h):
        """mT12i of hypothesis h: [s R | t; 0 0 0 1] in float32."""
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = self.t12[h, 12] * self.t12[h, :9].reshape(3, 3)
        T[:3, 3] = self.t12[h, 9:12]
        return T

    def GetEstimatedRotation(self):
        return self.t12[self.best, :9].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return self.t12[self.best, 9:12].copy()

    def GetEstimatedScale(self):
        return float(self.t12[self.best, 12])


class PnPsolver:
    """PnPsolver (include/PnPsolver.h) on POD inputs: the constructor's gathering (PnPsolver.cc:67-118) stays with the caller, who
    hands over a problem dict in the layout of slamit_pnp_problem (synth.synth_pnp): p3d (n, 3), p2d (n, 2) float32, sigma2 (n)
    -- or max_err (n) directly --, intr (fu fv uc vc).  The hypotheses run on the device in one call (ransac), Refine() of every
    hypothesis the scan can record as best in a second one (refine); iterate()'s sequential scan (:190-263) runs here over both
    result sets.  `rand_int(lo, hi)` stands for DUtils::Random::RandomInt; all mRansacMaxIts quadruples are drawn when the
    parameters are set, so the process RNG is consumed in another order than in the reference."""

    def __init__(self, problem, rand_int=None, device=0):
        self.problem = dict(problem)
        self.N = len(np.asarray(problem["p3d"]).reshape(-1, 3))
        self.device = device
        if rand_int is None:
            rs = np.random.RandomState(0)
            rand_int = lambda lo, hi: int(rs.randint(lo, hi + 1))   # noqa: E731
        self.rand_int = rand_int
        self.SetRansacParameters(_draw=False)   # the constructor's default parameters (:117) take nothing from the RNG: the first iterate() draws

    @staticmethod
    def ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon):
        """SetRansacParameters (:137-160) -> (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon): the truncated float product, the two
        clamps, the epsilon update in float, pow(epsilon, 3) (3 although the set is 4), the == N case, the final clamp."""
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            eps = np.float32(epsilon)
            nmin = int(np.float32(N) * eps)
            nmin = max(nmin, minInliers, minSet)
            ratio = np.float32(nmin) / np.float32(N)
            if eps < ratio:
                eps = ratio
            if nmin == N:
                nit = 1
            else:
                v = np.ceil(np.log(np.float64(1) - np.float64(probability)) / np.log(np.float64(1) - np.float64(eps) ** 3))
                nit = int(v) if np.isfinite(v) and abs(v) < 2 ** 31 else -2 ** 31   # (int) of an unrepresentable double on x86-64
        return nmin, max(1, min(nit, maxIterations)), eps

    @staticmethod
    def sample_quads(N, count, rand_int):
        """The sampler of iterate() (:196-209), with its quirk: the slot overwritten is vAvailableIndices[idx] -- indexed by the
        VALUE drawn, not by the position randi -- so a value can be drawn twice inside a quadruple."""
        out = np.zeros((count, 4), np.int32)
        for h in range(count):
            avail, size = list(range(N)), N   # a value drawn may lie past the shrunken end: the store then lands in a popped slot
            for i in range(4):
                randi = rand_int(0, size - 1)
                idx = avail[randi]
                out[h, i] = idx
                avail[idx] = avail[size - 1]
                size -= 1
        return out

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991, _draw=True):
        if minSet != 4:
            raise SlamitError("PnPsolver.SetRansacParameters: minSet must be 4 (SLAMIT_ERR_ARG): the device solves four-point sets only")
        self.mRansacProb = probability
        self.mRansacMinInliers, self.mRansacMaxIts, self.mRansacEpsilon = self.ransac_parameters(self.N, probability, minInliers, maxIterations, minSet, epsilon)
        if "sigma2" in self.problem:
            self.problem["max_err"] = (np.asarray(self.problem["sigma2"], np.float32) * np.float32(th2)).astype(np.float32)   # mvMaxError: a float product
        self.mnIterations, self.mnBestInliers, self.best, self.accepted = 0, 0, -1, -1
        draw = self.mRansacMaxIts if _draw and self.N >= self.mRansacMinInliers else 0
        self.quads = self.sample_quads(self.N, draw, self.rand_int)
        w = (self.N + 31) // 32
        self.pose, self.counts, self.bits = np.zeros((0, 12)), np.zeros(0, np.int32), np.zeros((0, w), np.uint32)
        self.refined = {}   # recorded best -> dict(pose, n_inliers, inlier_bits)

    # ---- the two device calls ----
    @staticmethod
    def _arrays(pr, what):
        k = {"p3d": np.ascontiguousarray(pr["p3d"], np.float32).reshape(-1, 3), "p2d": np.ascontiguousarray(pr["p2d"], np.float32).reshape(-1, 2),
             "max_err": np.ascontiguousarray(pr["max_err"], np.float32).reshape(-1)}
        n = len(k["max_err"])
        if len(k["p3d"]) != n or len(k["p2d"]) != n:
            raise SlamitError("PnPsolver.%s: p3d / p2d / max_err do not have the same length" % what)
        return k, n

    @staticmethod
    def ransac(problems, device=0, want_bits=True):
        """Raw per-hypothesis results of one problem dict (with "quads" (n_hyp, 4)) or a list of them, in ONE device call: dict(s)
        with pose (n_hyp, 12) float64 = mRi row-major, mti; n_inliers (n_hyp); inlier_bits (n_hyp, (n + 31) // 32)."""
        single = isinstance(problems, dict)
        plist = [problems] if single else list(problems)
        m = len(plist)
        P, R = (PnpProblem * m)(), (PnpResult * m)()
        keep, outs = [], []
        for i, pr in enumerate(plist):
            k, n = PnPsolver._arrays(pr, "ransac")
            k["quads"] = np.ascontiguousarray(pr["quads"], np.int32).reshape(-1, 4)
            nh = len(k["quads"])
            q = P[i]
            q.n, q.n_hyp = n, nh
            for key, a in k.items():
                setattr(q, key, a.ctypes.data)
            q.intr = (C.c_double * 4)(*[float(v) for v in pr["intr"]])
            o = {"pose": np.zeros((nh, 12), np.float64), "n_inliers": np.zeros(nh, np.int32)}
            R[i].pose, R[i].n_inliers = o["pose"].ctypes.data, o["n_inliers"].ctypes.data
            if want_bits:
                o["inlier_bits"] = np.zeros((nh, (n + 31) // 32), np.uint32)
                R[i].inlier_bits = o["inlier_bits"].ctypes.data
            keep.append(k)
            outs.append(o)
        _check(lib().slamit_pnp_ransac_batch(device, m, P, R), "slamit_pnp_ransac_batch")
        del keep
        return outs[0] if single else outs

    @staticmethod
    def refine(problems, device=0):
        """Refine() (:268-313) of one problem dict or a list of them in ONE device call.  Each carries "subset_bits" ((n + 31) // 32
        uint32, e.g. a row of ransac()'s inlier_bits) or "subset" (n bool).  -> dict(s) pose (12) float64, n_inliers, inlier_bits."""
        single = isinstance(problems, dict)
        plist = [problems] if single else list(problems)
        m = len(plist)
        P, R = (PnpRefineProblem * m)(), (PnpRefineResult * m)()
        keep, outs = [], []
        for i, pr in enumerate(plist):
            k, n = PnPsolver._arrays(pr, "refine")
            if "subset_bits" in pr:
                k["subset_bits"] = np.ascontiguousarray(pr["subset_bits"], np.uint32).reshape(-1)
            else:
                f = np.zeros(((n + 31) // 32) * 32, np.uint8)
                f[:n] = np.asarray(pr["subset"], bool).reshape(-1)
                k["subset_bits"] = np.packbits(f, bitorder="little").view(np.uint32)
            if len(k["subset_bits"]) != (n + 31) // 32:
                raise SlamitError("PnPsolver.refine: the subset does not have (n + 31) // 32 words")
            q = P[i]
            q.n = n
            for key, a in k.items():
                setattr(q, key, a.ctypes.data)
            q.intr = (C.c_double * 4)(*[float(v) for v in pr["intr"]])
            o = {"inlier_bits": np.zeros((n + 31) // 32, np.uint32)}
            R[i].inlier_bits = o["inlier_bits"].ctypes.data
            keep.append(k)
            outs.append(o)
        _check(lib().slamit_pnp_refine_batch(device, m, P, R), "slamit_pnp_refine_batch")
        for i, o in enumerate(outs):
            o["pose"], o["n_inliers"] = np.array(R[i].pose, np.float64), int(R[i].n_inliers)
        del keep
        return outs[0] if single else outs

    @staticmethod
    def records(counts, minInliers, best=0):
        """The hypotheses iterate() records as best (:217-232): the strict prefix maxima among counts >= minInliers."""
        out = []
        for h, c in enumerate(counts):
            if c >= minInliers and c > best:
                best = int(c)
                out.append(h)
        return out

    @staticmethod
    def EvaluateAll(solvers, device=0):
        """Everything the next iterate() of every solver can need, in two launches: the hypotheses drawn and not yet evaluated, then
        Refine() of every hypothesis those scans can record as best (what Tracking::Relocalization costs for all its candidates)."""
        for s in solvers:
            if len(s.quads) < s.mRansacMaxIts and s.N >= s.mRansacMinInliers:   # parameters set by the constructor alone: draw now
                s.quads = np.vstack([s.quads, PnPsolver.sample_quads(s.N, s.mRansacMaxIts - len(s.quads), s.rand_int)])
        todo = [s for s in solvers if len(s.counts) < len(s.quads)]
        first = [len(s.counts) for s in todo]
        for lo in range(0, max([len(s.quads) - f for s, f in zip(todo, first)] + [0]), PNP_MAX_HYP):
            part = [(s, s.quads[f + lo:f + lo + PNP_MAX_HYP]) for s, f in zip(todo, first) if f + lo < len(s.quads)]
            res = PnPsolver.ransac([dict(s.problem, quads=q) for s, q in part], device)
            for (s, _), r in zip(part, res):
                s.pose, s.counts, s.bits = np.vstack([s.pose, r["pose"]]), np.concatenate([s.counts, r["n_inliers"]]), np.vstack([s.bits, r["inlier_bits"]])
        jobs = []
        for s in solvers:
            for h in PnPsolver.records(s.counts[s.mnIterations:], s.mRansacMinInliers, s.mnBestInliers):
                if s.mnIterations + h not in s.refined:
                    jobs.append((s, s.mnIterations + h))
        if jobs:
            res = PnPsolver.refine([dict(s.problem, subset_bits=s.bits[h]) for s, h in jobs], device)
            for (s, h), r in zip(jobs, res):
                s.refined[h] = r

    def flags(self, bits):
        b = np.unpackbits(np.ascontiguousarray(bits, np.uint32).view(np.uint8), bitorder="little")[:self.N]
        return b.astype(bool)

    @staticmethod
    def Tcw(pose):
        """[R | t; 0 0 0 1] in float32, converted from the double pose as :225-231 does."""
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = np.asarray(pose[:9], np.float64).reshape(3, 3).astype(np.float32)
        T[:3, 3] = np.asarray(pose[9:12], np.float64).astype(np.float32)
        return T

    def iterate(self, nIterations):
        """-> (Tcw (4, 4) float32 or None, bNoMore, vbInliers (N) bool, nInliers).  self.accepted is the hypothesis whose refined
        (self.kind == "refined") or own (self.kind == "best", the bNoMore tail) pose was returned."""
        vb = np.zeros(self.N, bool)
        self.kind = None
        if self.N < self.mRansacMinInliers:
            return None, True, vb, 0
        need = self.mnIterations + max(self.mRansacMaxIts - self.mnIterations, nIterations)
        if need > len(self.quads):   # a call after bNoMore (or maxIts < nIterations): its further hypotheses, in a call of their own
            self.quads = np.vstack([self.quads, self.sample_quads(self.N, need - len(self.quads), self.rand_int)])
        PnPsolver.EvaluateAll([self], self.device)
        cur = 0
        while self.mnIterations < self.mRansacMaxIts or cur < nIterations:
            cur += 1
            h = self.mnIterations
            self.mnIterations += 1
            if self.counts[h] >= self.mRansacMinInliers:
                if self.counts[h] > self.mnBestInliers:
                    self.mnBestInliers, self.best = int(self.counts[h]), h
                r = self.refined[self.best]           # Refine() on an unchanged best gives the same (failing) answer again
                if r["n_inliers"] > self.mRansacMinInliers:
                    self.accepted, self.kind = self.best, "refined"
                    return self.Tcw(r["pose"]), False, self.flags(r["inlier_bits"]), int(r["n_inliers"])
        if self.mnIterations >= self.mRansacMaxIts and self.mnBestInliers >= self.mRansacMinInliers:
            self.accepted, self.kind = self.best, "best"
            return self.Tcw(self.pose[self.best]), True, self.flags(self.bits[self.best]), self.mnBestInliers
        return None, self.mnIterations >= self.mRansacMaxIts, vb, 0

    def find(self):
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n


def _init_frames(pr, q):
    """keys1 / keys2 / matches of a problem dict into the record q; -> (arrays kept alive, n)."""
    k = {"keys1": np.ascontiguousarray(pr["keys1"], np.float32).reshape(-1, 2), "keys2": np.ascontiguousarray(pr["keys2"], np.float32).reshape(-1, 2),
         "matches": np.ascontiguousarray(pr["matches"], np.int32).reshape(-1, 2)}
    q.n1, q.n2, q.n = len(k["keys1"]), len(k["keys2"]), len(k["matches"])
    q.sigma = float(pr.get("sigma", 1.0))
    for key, a in k.items():
        setattr(q, key, a.ctypes.data)
    return k, int(q.n)


def init_hypotheses(problems, device=0, want_bits=True):
    """FindHomography's and FindFundamental's loop bodies (Initializer.cc:133-232) for one problem dict or a list of them in ONE
    device call.  A problem has keys1 (n1, 2), keys2 (n2, 2) float32, matches (n, 2) int32 (index into keys1, into keys2), sigma and
    sets (n_hyp, 8) int32 indices into the matches.  -> dict(s) model (2, n_hyp, 9) float32 (row 0 the H21i, row 1 the F21i), score
    (2, n_hyp) float32, n_inliers (2, n_hyp), inlier_bits (2, n_hyp, (n + 31) // 32)."""
    single = isinstance(problems, dict)
    plist = [problems] if single else list(problems)
    m = len(plist)
    P, R = (InitProblem * m)(), (InitResult * m)()
    keep, outs = [], []
    for i, pr in enumerate(plist):
        k, n = _init_frames(pr, P[i])
        k["sets"] = np.ascontiguousarray(pr["sets"], np.int32).reshape(-1, 8)
        nh = len(k["sets"])
        P[i].n_hyp, P[i].sets = nh, k["sets"].ctypes.data
        o = {"model": np.zeros((2, nh, 9), np.float32), "score": np.zeros((2, nh), np.float32), "n_inliers": np.zeros((2, nh), np.int32)}
        R[i].model, R[i].score, R[i].n_inliers = o["model"].ctypes.data, o["score"].ctypes.data, o["n_inliers"].ctypes.data
        if want_bits:
            o["inlier_bits"] = np.zeros((2, nh, (n + 31) // 32), np.uint32)
            R[i].inlier_bits = o["inlier_bits"].ctypes.data
        keep.append(k)
        outs.append(o)
    _check(lib().slamit_init_hyp_batch(device, m, P, R), "slamit_init_hyp_batch")
    del keep
    return outs[0] if single else outs


def init_reconstruct(problems, device=0):
    """ReconstructH's eight motions or ReconstructF's four with CheckRT for each (Initializer.cc:479-916) for one problem dict or a
    list of them in ONE device call.  A problem has keys1, keys2, matches, sigma as for init_hypotheses, kind (INIT_H / INIT_F), model
    (9), K (3, 3) and subset_bits ((n + 31) // 32 uint32, a row of inlier_bits) or subset (n bool).  -> dict(s) decomposable, R (m, 9),
    t (m, 3), n_good (m), cos_sel (m), status (m, n) uint8, points (m, n, 3), good_bits (m, words) with m = 8 or 4."""
    single = isinstance(problems, dict)
    plist = [problems] if single else list(problems)
    m = len(plist)
    P, R = (InitReconstructProblem * m)(), (InitReconstructResult * m)()
    keep, outs = [], []
    for i, pr in enumerate(plist):
        k, n = _init_frames(pr, P[i])
        if "subset_bits" in pr:
            k["subset_bits"] = np.ascontiguousarray(pr["subset_bits"], np.uint32).reshape(-1)
        else:
            f = np.zeros(((n + 31) // 32) * 32, np.uint8)
            f[:n] = np.asarray(pr["subset"], bool).reshape(-1)
            k["subset_bits"] = np.packbits(f, bitorder="little").view(np.uint32)
        if len(k["subset_bits"]) != (n + 31) // 32:
            raise SlamitError("init_reconstruct: the subset does not have (n + 31) // 32 words")
        kind = int(pr["kind"])
        nm = 8 if kind == INIT_H else 4
        P[i].kind, P[i].subset_bits = kind, k["subset_bits"].ctypes.data
        P[i].model = (C.c_float * 9)(*[float(v) for v in np.asarray(pr["model"], np.float32).reshape(9)])
        P[i].K = (C.c_float * 9)(*[float(v) for v in np.asarray(pr["K"], np.float32).reshape(9)])
        o = {"status": np.zeros((nm, n), np.uint8), "points": np.zeros((nm, n, 3), np.float32), "good_bits": np.zeros((nm, (n + 31) // 32), np.uint32)}
        R[i].status, R[i].points, R[i].good_bits = o["status"].ctypes.data, o["points"].ctypes.data, o["good_bits"].ctypes.data
        keep.append(k)
        outs.append(o)
    _check(lib().slamit_init_reconstruct_batch(device, m, P, R), "slamit_init_reconstruct_batch")
    for i, o in enumerate(outs):
        nm = int(R[i].n_motions)
        o["decomposable"] = int(R[i].decomposable)
        o["R"] = np.array(R[i].R, np.float32)[:9 * nm].reshape(nm, 9)
        o["t"] = np.array(R[i].t, np.float32)[:3 * nm].reshape(nm, 3)
        o["n_good"] = np.array(R[i].n_good, np.int32)[:nm]
        o["cos_sel"] = np.array(R[i].cos_sel, np.float32)[:nm]
    del keep
    return outs[0] if single else outs


def init_select(hyp, reco=None, min_parallax=1.0, min_triangulated=50):
    """The host scans (csrc/two_view.h through the library).  With `hyp` alone: -> dict(best_h, best_f, SH, SF, kind) -- the strict >
    first-best of each model and RH > 0.40.  With the result `reco` of init_reconstruct on the kept hypothesis and its inlier count
    n_inliers in `hyp["N"]`: adds parallax (m) in degrees and motion (the winner, -1 = rejected)."""
    L = lib()
    sel = {}
    for r, name in ((0, "h"), (1, "f")):
        sc = np.ascontiguousarray(hyp["score"][r], np.float32)
        sel["best_" + name] = int(L.slamit_init_best_hypothesis(len(sc), sc.ctypes.data))
    sel["SH"] = np.float32(hyp["score"][0][sel["best_h"]]) if sel["best_h"] >= 0 else np.float32(0)
    sel["SF"] = np.float32(hyp["score"][1][sel["best_f"]]) if sel["best_f"] >= 0 else np.float32(0)
    sel["kind"] = INIT_H if L.slamit_init_choose_h(float(sel["SH"]), float(sel["SF"])) else INIT_F
    if reco is not None:
        ng = np.ascontiguousarray(reco["n_good"], np.int32)
        par = np.array([L.slamit_init_parallax_deg(int(g), float(c)) for g, c in zip(ng, reco["cos_sel"])], np.float32)
        pick = L.slamit_init_pick_h if len(ng) == 8 else L.slamit_init_pick_f
        sel["parallax"] = par
        sel["motion"] = int(pick(ng.ctypes.data, par.ctypes.data, int(hyp["N"]), float(min_parallax), int(min_triangulated))) if reco["decomposable"] else -1
    return sel


class Initializer:
    """Initializer (include/Initializer.h) on POD inputs: keys1 (n1, 2) = the reference frame's mvKeysUn, K (3, 3), sigma, iterations.
    Initialize(keys2, vMatches12) with vMatches12 (n1) int (-1 = unmatched) -> (ok, R21 (3, 3), t21 (3), vP3D (n1, 3), vbTriangulated
    (n1) bool) and leaves kind, motion and the raw device results in self.last.  `rand_int(lo, hi)` stands for
    DUtils::Random::RandomInt.  InitializeAll runs a list of (initializer, keys2, vMatches12) in two device calls."""

    def __init__(self, keys1, K, sigma=1.0, iterations=200, rand_int=None, device=0):
        self.keys1 = np.ascontiguousarray(keys1, np.float32).reshape(-1, 2)
        self.K = np.ascontiguousarray(K, np.float32).reshape(3, 3)
        self.sigma, self.iterations, self.device = float(sigma), int(iterations), device
        if rand_int is None:
            rs = np.random.RandomState(0)
            rand_int = lambda lo, hi: int(rs.randint(lo, hi + 1))   # noqa: E731
        self.rand_int = rand_int
        self.last = None

    @staticmethod
    def sample_sets(N, count, rand_int):
        """The sampler of Initialize (:91-106): eight draws without replacement per set."""
        out = np.zeros((count, 8), np.int32)
        for it in range(count):
            avail = list(range(N))
            for j in range(8):
                randi = rand_int(0, len(avail) - 1)
                out[it, j] = avail[randi]
                avail[randi] = avail[-1]
                avail.pop()
        return out

    def _problem(self, keys2, vMatches12, sets=None):
        vm = np.asarray(vMatches12, np.int64).reshape(-1)
        i1 = np.flatnonzero(vm >= 0)
        matches = np.stack([i1, vm[i1]], axis=1).astype(np.int32)
        if sets is None:
            sets = self.sample_sets(len(matches), self.iterations, self.rand_int)
        return {"keys1": self.keys1, "keys2": np.ascontiguousarray(keys2, np.float32).reshape(-1, 2), "matches": matches, "sigma": self.sigma,
                "sets": sets, "K": self.K}

    @staticmethod
    def InitializeAll(jobs, device=0, sets=None):
        """jobs: (initializer, keys2, vMatches12).  Two device calls for all of them; -> the list of Initialize results."""
        probs = [ini._problem(k2, vm, None if sets is None else sets[j]) for j, (ini, k2, vm) in enumerate(jobs)]
        hyps = init_hypotheses(probs, device)
        recos_in = []
        for pr, hy in zip(probs, hyps):
            sel = init_select(hy)
            kind = sel["kind"]
            b = sel["best_h"] if kind == INIT_H else sel["best_f"]
            n = len(pr["matches"])
            bits = hy["inlier_bits"][kind][b] if b >= 0 else np.zeros((n + 31) // 32, np.uint32)   # no score above 0: an empty model and no inliers
            model = hy["model"][kind][b] if b >= 0 else np.zeros(9, np.float32)
            hy["N"] = int(hy["n_inliers"][kind][b]) if b >= 0 else 0
            hy["sel"] = sel
            recos_in.append(dict(pr, kind=kind, model=model, subset_bits=bits))
        recos = init_reconstruct(recos_in, device)
        outs = []
        for (ini, _, _), pr, hy, rc in zip(jobs, probs, hyps, recos):
            sel = dict(hy["sel"], **init_select(hy, rc))
            n1 = len(ini.keys1)
            R21, t21 = np.zeros((3, 3), np.float32), np.zeros(3, np.float32)
            vP3D, vbT = np.zeros((n1, 3), np.float32), np.zeros(n1, bool)
            mo = sel["motion"]
            if mo >= 0:
                R21, t21 = rc["R"][mo].reshape(3, 3).copy(), rc["t"][mo].copy()
                i1 = pr["matches"][:, 0]
                counted = rc["status"][mo] == 0
                vP3D[i1[counted]] = rc["points"][mo][counted]
                n = len(i1)
                good = np.unpackbits(rc["good_bits"][mo].view(np.uint8), bitorder="little")[:n].astype(bool)
                vbT[i1[good]] = True
            ini.last = {"problem": pr, "hyp": hy, "reco": rc, "sel": sel, "kind": sel["kind"], "motion": mo}
            outs.append((mo >= 0, R21, t21, vP3D, vbT))
        return outs

    def Initialize(self, keys2, vMatches12, sets=None):
        return Initializer.InitializeAll([(self, keys2, vMatches12)], self.device, None if sets is None else [sets])[0]


_TRI_STEREO_ARRAYS = ("ur1", "ur2", "depth1", "depth2", "raw1_xy", "raw2_xy")
_TRI_STEREO_SCALARS = ("mb1", "mb2", "bf")


def triangulate_batch(problems, device=0):
    """LocalMapping::CreateNewMapPoints' per-pair body (LocalMapping.cc:348-483, monocular) for a list of (current keyframe, neighbour)
    problems in ONE device call.  Each problem is a dict in the layout of slamit_triangulate_problem (synth.synth_triangulation):
    Tcw1, Tcw2 (12) float32, intr1, intr2 (fx fy cx cy invfx invfy), kp1_xy, kp2_xy (n, 2), octave1, octave2 (n), n_levels,
    scale_factors1/2 and level_sigma2_1/2 (n_levels), ratio_factor.  -> a list of dicts: status (n) uint8 (0 accepted, else the first
    gate that rejected the pair), x3d (n, 3) float32, n_accepted, source (n) uint8 (0 no point, 1 triangulated, 2 / 3 UnprojectStereo
    of keyframe 1 / 2).  A problem that also holds the stereo keys ur1, ur2, depth1, depth2 (n), raw1_xy, raw2_xy (n, 2), mb1, mb2, bf
    (synth.synth_triangulation_stereo) takes the stereo branches (:335-465, status 9 = UnprojectStereo of a depth <= 0); all of the
    keys or none."""
    plist = list(problems)
    m = len(plist)
    P = (TriangulateProblem * m)()
    R = (TriangulateResult * m)()
    T = (C.POINTER(TriangulateStereo) * m)()
    SRC = (C.c_void_p * m)()
    keep, outs = [], []
    for i, pr in enumerate(plist):
        k = {"kp1_xy": np.ascontiguousarray(pr["kp1_xy"], np.float32).reshape(-1, 2), "kp2_xy": np.ascontiguousarray(pr["kp2_xy"], np.float32).reshape(-1, 2),
             "octave1": np.ascontiguousarray(pr["octave1"], np.int32).reshape(-1), "octave2": np.ascontiguousarray(pr["octave2"], np.int32).reshape(-1)}
        n, nl = len(k["octave1"]), int(pr["n_levels"])
        if len(k["kp1_xy"]) != n or len(k["kp2_xy"]) != n or len(k["octave2"]) != n:
            raise SlamitError("triangulate: kp1_xy / kp2_xy / octave1 / octave2 do not have the same length")
        for key in ("scale_factors1", "level_sigma2_1", "scale_factors2", "level_sigma2_2"):
            k[key] = np.ascontiguousarray(pr[key], np.float32).reshape(-1)
            if len(k[key]) != nl:
                raise SlamitError("triangulate: %s does not have n_levels entries" % key)
        q = P[i]
        for key in ("Tcw1", "Tcw2", "intr1", "intr2"):
            a = np.asarray(pr[key], np.float32).reshape(-1)
            if len(a) != (12 if key[0] == "T" else 6):
                raise SlamitError("triangulate: %s has %d entries" % (key, len(a)))
            setattr(q, key, (C.c_float * len(a))(*[float(v) for v in a]))
        q.n, q.n_levels, q.ratio_factor = n, nl, float(pr["ratio_factor"])
        for key, a in k.items():
            setattr(q, key, a.ctypes.data)
        have = [key in pr for key in _TRI_STEREO_ARRAYS + _TRI_STEREO_SCALARS]
        if any(have):
            if not all(have):
                raise SlamitError("triangulate: a stereo problem needs all of " + " ".join(_TRI_STEREO_ARRAYS + _TRI_STEREO_SCALARS))
            t = TriangulateStereo()
            for key in _TRI_STEREO_ARRAYS:
                a = np.ascontiguousarray(pr[key], np.float32).reshape(-1)
                if len(a) != (2 * n if key[:3] == "raw" else n):
                    raise SlamitError("triangulate: %s has %d entries" % (key, len(a)))
                k[key] = a
                setattr(t, key, a.ctypes.data)
            t.mb1, t.mb2, t.bf = float(pr["mb1"]), float(pr["mb2"]), float(pr["bf"])
            k["stereo record"] = t
            T[i] = C.pointer(t)
        o = {"status": np.zeros(n, np.uint8), "x3d": np.zeros((n, 3), np.float32), "source": np.zeros(n, np.uint8)}
        R[i].status, R[i].x3d = o["status"].ctypes.data, o["x3d"].ctypes.data
        SRC[i] = o["source"].ctypes.data
        keep.append(k)
        outs.append(o)
    _check(lib().slamit_triangulate_stereo_batch(device, m, P, T, R, SRC), "slamit_triangulate_stereo_batch")
    del keep
    for i, o in enumerate(outs):
        o["n_accepted"] = int(R[i].n_accepted)
    return outs


def triangulate(problem, device=0):
    """One (current keyframe, neighbour) problem: triangulate_batch([problem])[0]."""
    return triangulate_batch([problem], device)[0]


_FRUSTUM_SCALARS = ("fx", "fy", "cx", "cy", "bf", "min_x", "max_x", "min_y", "max_y", "view_cos_limit", "log_scale_factor", "th")


def frustum_frame_record(pr):
    """The slamit_frustum_frame of a problem dict as a one-element numpy record array (FRUSTUM_FRAME_DTYPE): what frustum_batch_dev's
    d_frames holds per frame."""
    rec = np.zeros(1, FRUSTUM_FRAME_DTYPE)
    for key, k in (("Rcw", 9), ("tcw", 3), ("Ow", 3)):
        a = np.asarray(pr[key], np.float32).reshape(-1)
        if len(a) != k:
            raise SlamitError("frustum: %s has %d entries" % (key, len(a)))
        rec[key][0] = a
    for key in _FRUSTUM_SCALARS:
        rec[key][0] = np.float32(pr[key])
    sf = np.asarray(pr["scale_factors"], np.float32).reshape(-1)
    nl = int(pr["n_levels"])
    if len(sf) != nl:
        raise SlamitError("frustum: scale_factors does not have n_levels entries")
    rec["n_levels"][0] = nl
    rec["scale_factors"][0, :min(nl, 16)] = sf[:16]
    return rec


def frustum_batch(problems, device=0):
    """Tracking::SearchLocalPoints' visibility pass (Frame::isInFrustum + MapPoint::PredictScale, Frame.cc:389-445, MapPoint.cc:391-400)
    and the queries of the SearchByProjection that follows, for a list of frames in ONE device call.  Each problem is a dict in the
    layout of slamit_frustum_problem (synth.synth_frustum): Rcw (9), tcw, Ow (3), fx fy cx cy bf, min_x max_x min_y max_y,
    view_cos_limit, log_scale_factor, th, n_levels, scale_factors (n_levels), pos, normal (n, 3), max_dist, min_dist (n) float32, skip
    (n) uint8.  -> a list of dicts: status (n) uint8 (0 in view, else the first test that rejected the point; 7 = the level outside
    the table, the stated departure), proj (n, 3) = u, v, uR, view_cos (n), level (n), and the guided search's query arrays uvr
    (n, 3), level_min, level_max (n), valid (n); n_in_view."""
    plist = list(problems)
    m = len(plist)
    P = (FrustumProblem * m)()
    R = (FrustumResult * m)()
    keep, outs = [], []
    for i, pr in enumerate(plist):
        k = {"pos": np.ascontiguousarray(pr["pos"], np.float32).reshape(-1, 3), "normal": np.ascontiguousarray(pr["normal"], np.float32).reshape(-1, 3),
             "max_dist": np.ascontiguousarray(pr["max_dist"], np.float32).reshape(-1), "min_dist": np.ascontiguousarray(pr["min_dist"], np.float32).reshape(-1),
             "skip": np.ascontiguousarray(pr["skip"], np.uint8).reshape(-1)}
        n = len(k["skip"])
        if any(len(a) != n for a in k.values()):
            raise SlamitError("frustum: pos / normal / max_dist / min_dist / skip do not have the same length")
        rec = frustum_frame_record(pr)
        C.memmove(C.byref(P[i].frame), rec.ctypes.data, C.sizeof(FrustumFrame))
        P[i].n = n
        for key, a in k.items():
            setattr(P[i], key, a.ctypes.data)
        o = {"status": np.zeros(n, np.uint8), "proj": np.zeros((n, 3), np.float32), "view_cos": np.zeros(n, np.float32), "level": np.zeros(n, np.int32),
             "uvr": np.zeros((n, 3), np.float32), "level_min": np.zeros(n, np.int32), "level_max": np.zeros(n, np.int32), "valid": np.zeros(n, np.uint8)}
        for key, a in o.items():
            setattr(R[i], key, a.ctypes.data)
        keep.append(k)
        outs.append(o)
    _check(lib().slamit_frustum_batch(device, m, P, R), "slamit_frustum_batch")
    del keep
    for i, o in enumerate(outs):
        o["n_in_view"] = int(R[i].n_in_view)
    return outs


def frustum(problem, device=0):
    """One frame: frustum_batch([problem])[0]."""
    return frustum_batch([problem], device)[0]


def frustum_batch_dev(t, device=0, stream=None):
    """The resident form.  t: dict of torch CUDA tensors frames (B, 44) f32 (rows of FRUSTUM_FRAME_DTYPE viewed as float32), m (B) i32,
    pos / normal (B, 3, q_cap) f32 PLANES, max_dist / min_dist (B, q_cap) f32, skip (B, q_cap) u8, and the outputs uvr (B, q_cap, 3)
    f32, level_min / level_max (B, q_cap) i32, valid (B, q_cap) u8 -- the tensors guided_search_batch_dev reads -- plus optionally
    status (B, q_cap) u8, proj (B, q_cap, 3) f32, view_cos (B, q_cap) f32, level (B, q_cap) i32, n_in_view (B) i32.
    Asynchronous on `stream`."""
    b, q_cap = t["pos"].shape[0], t["pos"].shape[2]
    if t["frames"].numel() * t["frames"].element_size() != b * C.sizeof(FrustumFrame):
        raise SlamitError("frustum_batch_dev: frames does not hold one slamit_frustum_frame per frame")
    for key, per in (("pos", 3), ("normal", 3), ("max_dist", 1), ("min_dist", 1), ("skip", 1), ("uvr", 3), ("level_min", 1), ("level_max", 1), ("valid", 1),
                     ("status", 1), ("proj", 3), ("view_cos", 1), ("level", 1)):
        if t.get(key) is not None and (t[key].numel() != b * q_cap * per or not t[key].is_contiguous()):
            raise SlamitError("frustum_batch_dev: %s is not a contiguous (B, q_cap) array" % key)
    for key in ("m", "n_in_view"):
        if t.get(key) is not None and t[key].numel() != b:
            raise SlamitError("frustum_batch_dev: %s does not have one entry per frame" % key)

    def opt(key):
        return t[key].data_ptr() if t.get(key) is not None else None

    rec = FrustumBatchRec(b, q_cap, t["frames"].data_ptr(), t["m"].data_ptr(), t["pos"].data_ptr(), t["normal"].data_ptr(), t["max_dist"].data_ptr(),
                          t["min_dist"].data_ptr(), t["skip"].data_ptr(), t["uvr"].data_ptr(), t["level_min"].data_ptr(), t["level_max"].data_ptr(),
                          t["valid"].data_ptr(), opt("status"), opt("proj"), opt("view_cos"), opt("level"), opt("n_in_view"))
    _check(lib().slamit_frustum_batch_dev(device, C.byref(rec), stream), "slamit_frustum_batch_dev")


_PROJECT_SCALARS = ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "log_scale_factor", "th")


def project_camera_record(pr):
    """The slamit_project_camera of a problem dict as a one-element numpy record array (PROJECT_CAMERA_DTYPE): what
    project_batch_dev's d_cameras holds per frame.  form is an index into PROJECT_FORMS or one of its names; R2 / t2 (SIM3_PAIR) and
    direction (LAST_FRAME) default to zero."""
    rec = np.zeros(1, PROJECT_CAMERA_DTYPE)
    form = pr["form"]
    rec["form"][0] = PROJECT_FORMS.index(form) if isinstance(form, str) else int(form)
    for key, k in (("R", 9), ("t", 3), ("O", 3), ("R2", 9), ("t2", 3)):
        if key in ("R2", "t2") and pr.get(key) is None:
            continue
        a = np.asarray(pr[key], np.float32).reshape(-1)
        if len(a) != k:
            raise SlamitError("project: %s has %d entries" % (key, len(a)))
        rec[key][0] = a
    for key in _PROJECT_SCALARS:
        rec[key][0] = np.float32(pr[key])
    sf = np.asarray(pr["scale_factors"], np.float32).reshape(-1)
    nl = int(pr["n_levels"])
    if len(sf) != nl:
        raise SlamitError("project: scale_factors does not have n_levels entries")
    rec["n_levels"][0] = nl
    rec["scale_factors"][0, :min(nl, 16)] = sf[:16]
    rec["direction"][0] = int(pr.get("direction", 0))
    return rec


def project_batch(problems, device=0, bf=None):
    """The projection loops in front of the guided search of six ORBmatcher drivers (csrc/project.h) for a list of
    cameras in ONE device call; the problems may differ in form.  Each problem is a dict in the layout of slamit_project_problem
    (synth.synth_project): the camera's fields (project_camera_record), pos (n, 3) float32, skip (n) uint8 and, where the form reads
    them (None otherwise), normal (n, 3), max_dist, min_dist (n) float32, octave (n) int32.  -> a list of dicts: status (n) uint8
    (0 accepted, else the first test that rejected the point; 7 = the level outside the table), proj (n, 2) = u, v, level (n), the
    guided search's query arrays uvr (n, 3), level_min, level_max (n), valid (n); n_valid.  bf: None, or one mbf per problem: every
    result then also holds ur (n) = u - bf * invz for the accepted points, zero otherwise (slamit_project_batch_stereo; forms
    LAST_FRAME and FUSE are the ones whose search reads it)."""
    plist = list(problems)
    m = len(plist)
    if bf is not None:
        bf = np.ascontiguousarray(np.atleast_1d(bf), np.float32)
        if len(bf) != m:
            raise SlamitError("project: bf does not have one entry per problem")
    P = (ProjectProblem * m)()
    R = (ProjectResult * m)()
    keep, outs = [], []
    for i, pr in enumerate(plist):
        k = {"pos": np.ascontiguousarray(pr["pos"], np.float32).reshape(-1, 3), "skip": np.ascontiguousarray(pr["skip"], np.uint8).reshape(-1)}
        for key, dt, shape in (("normal", np.float32, (-1, 3)), ("max_dist", np.float32, (-1,)), ("min_dist", np.float32, (-1,)), ("octave", np.int32, (-1,))):
            if pr.get(key) is not None:
                k[key] = np.ascontiguousarray(pr[key], dt).reshape(shape)
        n = len(k["skip"])
        if any(len(a) != n for a in k.values()):
            raise SlamitError("project: pos / normal / max_dist / min_dist / octave / skip do not have the same length")
        rec = project_camera_record(pr)
        C.memmove(C.byref(P[i].camera), rec.ctypes.data, C.sizeof(ProjectCamera))
        P[i].n = n
        for key, a in k.items():
            setattr(P[i], key, a.ctypes.data)
        o = {"status": np.zeros(n, np.uint8), "proj": np.zeros((n, 2), np.float32), "level": np.zeros(n, np.int32), "uvr": np.zeros((n, 3), np.float32),
             "level_min": np.zeros(n, np.int32), "level_max": np.zeros(n, np.int32), "valid": np.zeros(n, np.uint8)}
        for key, a in o.items():
            setattr(R[i], key, a.ctypes.data)
        keep.append(k)
        outs.append(o)
    if bf is not None:
        urp = (C.c_void_p * max(m, 1))()
        for i, o in enumerate(outs):
            o["ur"] = np.zeros(len(o["status"]), np.float32)
            urp[i] = o["ur"].ctypes.data if len(o["ur"]) else None
        _check(lib().slamit_project_batch_stereo(device, m, P, R, bf.ctypes.data, C.cast(urp, C.c_void_p)), "slamit_project_batch_stereo")
    else:
        _check(lib().slamit_project_batch(device, m, P, R), "slamit_project_batch")
    del keep
    for i, o in enumerate(outs):
        o["n_valid"] = int(R[i].n_valid)
    return outs


def project(problem, device=0, bf=None):
    """One camera: project_batch([problem])[0]; bf: its mbf, for the ur output."""
    return project_batch([problem], device, None if bf is None else [bf])[0]


def project_batch_dev(t, device=0, stream=None):
    """The resident form.  t: dict of torch CUDA tensors cameras (B, 56) f32 (rows of PROJECT_CAMERA_DTYPE viewed as float32), m (B)
    i32, pos / normal (B, 3, q_cap) f32 PLANES, max_dist / min_dist (B, q_cap) f32, octave (B, q_cap) i32, skip (B, q_cap) u8, and the
    outputs uvr (B, q_cap, 3) f32, level_min / level_max (B, q_cap) i32, valid (B, q_cap) u8 -- the tensors guided_search_batch_dev
    reads -- plus optionally status (B, q_cap) u8, proj (B, q_cap, 2) f32, level (B, q_cap) i32, n_valid (B) i32.  With bf (B) f32 and
    ur (B, q_cap) f32 both present, ur is written as well (slamit_project_batch_dev_stereo): guided_search_batch_dev's q_ur, stride 1.
    Asynchronous on `stream`."""
    b, q_cap = t["pos"].shape[0], t["pos"].shape[2]
    if t["cameras"].numel() * t["cameras"].element_size() != b * C.sizeof(ProjectCamera):
        raise SlamitError("project_batch_dev: cameras does not hold one slamit_project_camera per frame")
    for key, per in (("pos", 3), ("normal", 3), ("max_dist", 1), ("min_dist", 1), ("octave", 1), ("skip", 1), ("uvr", 3), ("level_min", 1),
                     ("level_max", 1), ("valid", 1), ("status", 1), ("proj", 2), ("level", 1), ("ur", 1)):
        if t.get(key) is not None and (t[key].numel() != b * q_cap * per or not t[key].is_contiguous()):
            raise SlamitError("project_batch_dev: %s is not a contiguous (B, q_cap) array" % key)
    for key in ("m", "n_valid", "bf"):
        if t.get(key) is not None and t[key].numel() != b:
            raise SlamitError("project_batch_dev: %s does not have one entry per frame" % key)

    def opt(key):
        return t[key].data_ptr() if t.get(key) is not None else None

    rec = ProjectBatchRec(b, q_cap, t["cameras"].data_ptr(), t["m"].data_ptr(), t["pos"].data_ptr(), t["normal"].data_ptr(), t["max_dist"].data_ptr(),
                          t["min_dist"].data_ptr(), t["octave"].data_ptr(), t["skip"].data_ptr(), t["uvr"].data_ptr(), t["level_min"].data_ptr(),
                          t["level_max"].data_ptr(), t["valid"].data_ptr(), opt("status"), opt("proj"), opt("level"), opt("n_valid"))
    if t.get("bf") is not None or t.get("ur") is not None:
        _check(lib().slamit_project_batch_dev_stereo(device, C.byref(rec), opt("bf"), opt("ur"), stream), "slamit_project_batch_dev_stereo")
        return
    _check(lib().slamit_project_batch_dev(device, C.byref(rec), stream), "slamit_project_batch_dev")


# ---- Frame::ComputeStereoMatches ------------------------------------------------------------------------------------------------

_STEREO_OUT = (("u_right", np.float32), ("depth", np.float32), ("status", np.uint8), ("best_r", np.int32), ("ham_dist", np.int32), ("sad_dist", np.int32))


def stereo_match(ext_left, ext_right, kps_left, desc_left, kps_right, desc_right, mb, mbf, frame=0):
    """Frame::ComputeStereoMatches on frame `frame` of the two extractors' last calls; keypoints (KP_DTYPE) and descriptors (n, 32)
    from the host, as the reference's Frame holds them.  -> dict u_right, depth (mvuRight, mvDepth), status, best_r, ham_dist,
    sad_dist (n_left each) and n_matched."""
    for e in (ext_left, ext_right):
        if e._h is None:
            raise SlamitError("stereo_match failed (-4): an extractor has no extract call yet")
    kl, kr = np.ascontiguousarray(kps_left, KP_DTYPE), np.ascontiguousarray(kps_right, KP_DTYPE)
    dl, dr = np.ascontiguousarray(desc_left, np.uint8).reshape(-1, 32), np.ascontiguousarray(desc_right, np.uint8).reshape(-1, 32)
    if len(dl) != len(kl) or len(dr) != len(kr):
        raise SlamitError("stereo_match: one descriptor row per keypoint")
    n = len(kl)
    out = {k: np.zeros(n, t) for k, t in _STEREO_OUT}
    nm = C.c_int32(0)
    _check(lib().slamit_stereo_match(ext_left._h, ext_right._h, frame, _np_ptr(kl), _np_ptr(dl), n, _np_ptr(kr), _np_ptr(dr), len(kr), float(mb),
                                     float(mbf), *[_np_ptr(out[k]) for k, _ in _STEREO_OUT], C.byref(nm)), "slamit_stereo_match")
    out["n_matched"] = int(nm.value)
    return out


def stereo_planes_view(planes):
    """slamit_pyramid_view over the caller's own planes: a list, one torch uint8 CUDA tensor (B, h, w) per level; rows and frames
    may be strided, pixels of a row are adjacent."""
    v = PyramidView()
    v.nlevels, v.nframes = len(planes), int(planes[0].shape[0]) if planes else 0
    if len(planes) > MAX_LEVELS:
        raise SlamitError("stereo_planes_view: more than SLAMIT_MAX_LEVELS levels")
    for l, p in enumerate(planes):
        if p.dim() != 3 or p.element_size() != 1 or (p.shape[2] > 1 and p.stride(2) != 1) or p.shape[0] != v.nframes:
            raise SlamitError("stereo_planes_view: level %d is not a (B, h, w) byte tensor with adjacent pixels" % l)
        v.level[l] = PyramidLevel(p.data_ptr(), int(p.shape[2]), int(p.shape[1]), int(p.stride(1)), int(p.stride(0)))
    return v


def stereo_match_workspace(nframes, cap_right):
    return int(lib().slamit_stereo_match_workspace(nframes, cap_right))


def stereo_match_batch_dev(t, device=0, stream=None):
    """The resident form.  t: dict with left / right: a PyramidView (ORBextractor.pyramid_view()) or a list of per-level torch
    tensors (stereo_planes_view); torch CUDA tensors kps_left (B, cap_l, 7) f32 rows of KP_DTYPE, desc_left (B, cap_l, 32) u8,
    n_left (B) i32, the same for right, mb / mbf (B) f32, scale / inv_scale (16) f32, workspace (u8, stereo_match_workspace bytes)
    and the outputs u_right / depth (B, cap_l) f32, status (B, cap_l) u8, best_r / ham_dist / sad_dist (B, cap_l) i32, n_matched (B)
    i32.  Asynchronous on `stream`."""
    views = [v if isinstance(v, PyramidView) else stereo_planes_view(v) for v in (t["left"], t["right"])]
    b, cap_l, cap_r = t["n_left"].numel(), t["kps_left"].shape[1], t["kps_right"].shape[1]
    for side, cap in (("left", cap_l), ("right", cap_r)):
        k, d = t["kps_" + side], t["desc_" + side]
        if k.numel() * k.element_size() != b * cap * KP_DTYPE.itemsize or d.numel() != b * cap * 32 or not k.is_contiguous() or not d.is_contiguous():
            raise SlamitError("stereo_match_batch_dev: %s keypoints / descriptors are not contiguous (B, cap) arrays" % side)
    for key, _ in _STEREO_OUT:
        if t[key].numel() != b * cap_l or not t[key].is_contiguous():
            raise SlamitError("stereo_match_batch_dev: %s is not a contiguous (B, cap_left) array" % key)
    for key in ("n_right", "mb", "mbf", "n_matched"):
        if t[key].numel() != b:
            raise SlamitError("stereo_match_batch_dev: %s does not have one entry per frame" % key)
    for key in ("scale", "inv_scale"):
        if t[key].numel() != MAX_LEVELS or t[key].element_size() != 4:
            raise SlamitError("stereo_match_batch_dev: %s does not hold SLAMIT_MAX_LEVELS floats" % key)
    ws = t.get("workspace")
    rec = StereoBatch(b, cap_l, cap_r, 0, views[0], views[1], t["kps_left"].data_ptr(), t["desc_left"].data_ptr(), t["n_left"].data_ptr(),
                      t["kps_right"].data_ptr(), t["desc_right"].data_ptr(), t["n_right"].data_ptr(), t["mb"].data_ptr(), t["mbf"].data_ptr(),
                      t["scale"].data_ptr(), t["inv_scale"].data_ptr(), ws.data_ptr() if ws is not None else None,
                      ws.numel() * ws.element_size() if ws is not None else 0, t["u_right"].data_ptr(), t["depth"].data_ptr(), t["status"].data_ptr(),
                      t["best_r"].data_ptr(), t["ham_dist"].data_ptr(), t["sad_dist"].data_ptr(), t["n_matched"].data_ptr())
    _check(lib().slamit_stereo_match_batch_dev(device, C.byref(rec), stream), "slamit_stereo_match_batch_dev")


# ---- Frame::ComputeStereoFromRGBD and the closest-point walk (csrc/unproject.h) ------------------------------

def rgbd_depth_batch(problems, device=0):
    """Frame::ComputeStereoFromRGBD (Frame.cc:766-787) for a list of frames in ONE device call.  Each problem is a dict
    (synth.synth_rgbd): plane, a 2-D numpy array of uint16 or float32 whose rows may be strided (a view of a wider array), factor
    (mDepthMapFactor), mbf, kps and kps_un (KP_DTYPE).  -> a list of dicts u_right, depth (mvuRight, mvDepth) float32 and status uint8
    (RGBD_STATUS: 2 = the truncated row or column lies outside the plane, the stated departure)."""
    plist = list(problems)
    m = len(plist)
    P = (RgbdProblem * max(m, 1))()
    R = (RgbdResult * max(m, 1))()
    keep, outs = [], []
    for i, pr in enumerate(plist):
        plane = pr["plane"]
        if plane.ndim != 2 or plane.dtype not in (np.uint16, np.float32) or (plane.shape[1] > 1 and plane.strides[1] != plane.itemsize):
            raise SlamitError("rgbd_depth: plane is not a 2-D uint16 / float32 array with adjacent pixels")
        k = {"kps": np.ascontiguousarray(pr["kps"], KP_DTYPE), "kps_un": np.ascontiguousarray(pr["kps_un"], KP_DTYPE)}
        n = len(k["kps"])
        if len(k["kps_un"]) != n:
            raise SlamitError("rgbd_depth: kps and kps_un do not have the same length")
        P[i].plane = DepthPlane(plane.ctypes.data, plane.strides[0] if plane.shape[0] > 1 else plane.shape[1] * plane.itemsize, plane.shape[1],
                                plane.shape[0], 1 if plane.dtype == np.uint16 else 0, float(pr["factor"]))
        P[i].mbf, P[i].n, P[i].kps, P[i].kps_un = float(pr["mbf"]), n, k["kps"].ctypes.data, k["kps_un"].ctypes.data
        o = {"u_right": np.zeros(n, np.float32), "depth": np.zeros(n, np.float32), "status": np.zeros(n, np.uint8)}
        for key, a in o.items():
            setattr(R[i], key, a.ctypes.data)
        keep.append((k, plane))
        outs.append(o)
    _check(lib().slamit_rgbd_depth_batch(device, m, P, R), "slamit_rgbd_depth_batch")
    del keep
    return outs


def rgbd_depth(problem, device=0):
    """One frame: rgbd_depth_batch([problem])[0]."""
    return rgbd_depth_batch([problem], device)[0]


def rgbd_depth_batch_dev(t, device=0, stream=None):
    """The resident form.  t: dict of torch CUDA tensors planes (B, 8) i32 (rows of DEPTH_PLANE_DTYPE viewed as int32; data is a
    device pointer), mbf (B) f32, kps / kps_un (B, cap, 7) f32 rows of KP_DTYPE, n (B) i32 and the outputs u_right / depth (B, cap)
    f32, optionally status (B, cap) u8.  Asynchronous on `stream`."""
    b, cap = t["n"].numel(), t["kps"].shape[1]
    if t["planes"].numel() * t["planes"].element_size() != b * C.sizeof(DepthPlane):
        raise SlamitError("rgbd_depth_batch_dev: planes does not hold one slamit_depth_plane per frame")
    for key in ("kps", "kps_un"):
        if t[key].numel() * t[key].element_size() != b * cap * KP_DTYPE.itemsize or not t[key].is_contiguous():
            raise SlamitError("rgbd_depth_batch_dev: %s is not a contiguous (B, cap) keypoint array" % key)
    for key in ("u_right", "depth", "status"):
        if t.get(key) is not None and (t[key].numel() != b * cap or not t[key].is_contiguous()):
            raise SlamitError("rgbd_depth_batch_dev: %s is not a contiguous (B, cap) array" % key)
    if t["mbf"].numel() != b:
        raise SlamitError("rgbd_depth_batch_dev: mbf does not have one entry per frame")
    rec = RgbdBatchRec(b, cap, t["planes"].data_ptr(), t["mbf"].data_ptr(), t["kps"].data_ptr(), t["kps_un"].data_ptr(), t["n"].data_ptr(),
                       t["u_right"].data_ptr(), t["depth"].data_ptr(), t["status"].data_ptr() if t.get("status") is not None else None)
    _check(lib().slamit_rgbd_depth_batch_dev(device, C.byref(rec), stream), "slamit_rgbd_depth_batch_dev")


_UNPROJECT_SCALARS = ("fx", "fy", "cx", "cy", "invfx", "invfy", "th_depth")


def unproject_frame_record(pr):
    """The slamit_unproject_frame of a problem dict as a one-element numpy record array (UNPROJECT_FRAME_DTYPE): what
    unproject_closest_batch_dev's d_frames holds per frame.  mode / ctor are indices into UNPROJECT_MODES / UNPROJECT_CTORS or names."""
    rec = np.zeros(1, UNPROJECT_FRAME_DTYPE)
    for key, k in (("Rwc", 9), ("Ow", 3)):
        a = np.asarray(pr[key], np.float32).reshape(-1)
        if len(a) != k:
            raise SlamitError("unproject: %s has %d entries" % (key, len(a)))
        rec[key][0] = a
    for key in _UNPROJECT_SCALARS:
        rec[key][0] = np.float32(pr[key])
    mode, ctor = pr.get("mode", 0), pr.get("ctor", 0)
    rec["mode"][0] = UNPROJECT_MODES.index(mode) if isinstance(mode, str) else int(mode)
    rec["ctor"][0] = UNPROJECT_CTORS.index(ctor) if isinstance(ctor, str) else int(ctor)
    rec["min_points"][0] = int(pr.get("min_points", 100))
    sf = np.asarray(pr["scale_factors"], np.float32).reshape(-1)
    nl = int(pr["n_levels"])
    if 1 <= nl <= 16 and len(sf) != nl:   # an n_levels outside the table goes to the library, which refuses it
        raise SlamitError("unproject: scale_factors does not have n_levels entries")
    rec["n_levels"][0] = nl
    rec["scale_factors"][0, :min(len(sf), 16)] = sf[:16]
    return rec


def unproject_closest_batch(problems, device=0):
    """The closest-point walk of Tracking::UpdateLastFrame / CreateNewKeyFrame / StereoInitialization with Frame::UnprojectStereo and
    the new points' constructor (csrc/unproject.h) for a list of frames in ONE device call.  Each problem is a
    dict in the layout of slamit_unproject_problem (synth.synth_unproject): the frame's fields (unproject_frame_record), kps_un
    (KP_DTYPE), depth (n) float32, tracked (n) uint8 (None in mode ALL).  -> a list of dicts: status (n) uint8 (UNPROJECT_STATUS),
    order (n) int32 (the keypoint at walk position j, -1 from n_visited on), pos, normal (n, 3), max_dist, min_dist (n) float32 --
    written for status 3, zero elsewhere -- and the six counters of UNPROJECT_COUNTS."""
    plist = list(problems)
    m = len(plist)
    P = (UnprojectProblem * max(m, 1))()
    R = (UnprojectResult * max(m, 1))()
    keep, outs = [], []
    for i, pr in enumerate(plist):
        k = {"kps_un": np.ascontiguousarray(pr["kps_un"], KP_DTYPE), "depth": np.ascontiguousarray(pr["depth"], np.float32).reshape(-1)}
        if pr.get("tracked") is not None:
            k["tracked"] = np.ascontiguousarray(pr["tracked"], np.uint8).reshape(-1)
        n = len(k["depth"])
        if any(len(a) != n for a in k.values()):
            raise SlamitError("unproject: kps_un / depth / tracked do not have the same length")
        rec = unproject_frame_record(pr)
        C.memmove(C.byref(P[i].frame), rec.ctypes.data, C.sizeof(UnprojectFrame))
        P[i].n = n
        for key, a in k.items():
            setattr(P[i], key, a.ctypes.data)
        o = {"status": np.zeros(n, np.uint8), "order": np.zeros(n, np.int32), "pos": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32),
             "max_dist": np.zeros(n, np.float32), "min_dist": np.zeros(n, np.float32)}
        for key, a in o.items():
            setattr(R[i], key, a.ctypes.data)
        keep.append(k)
        outs.append(o)
    _check(lib().slamit_unproject_closest_batch(device, m, P, R), "slamit_unproject_closest_batch")
    del keep
    for i, o in enumerate(outs):
        for key in UNPROJECT_COUNTS:
            o[key] = int(getattr(R[i].counts, key))
    return outs


def unproject_closest(problem, device=0):
    """One frame: unproject_closest_batch([problem])[0]."""
    return unproject_closest_batch([problem], device)[0]


def unproject_closest_batch_dev(t, device=0, stream=None):
    """The resident form, merged in place into project_batch_dev's LAST_FRAME arrays.  t: dict of torch CUDA tensors frames (B, 39)
    f32 (rows of UNPROJECT_FRAME_DTYPE viewed as float32), n (B) i32, kps_un (B, cap, 7) f32 rows of KP_DTYPE, depth (B, cap) f32,
    tracked (B, cap) u8 and, in / out, pos (B, 3, cap) f32 PLANES, octave (B, cap) i32, skip (B, cap) u8, optionally normal
    (B, 3, cap), max_dist, min_dist (B, cap) f32 -- written only where a point is created -- plus the optional outputs status (B, cap)
    u8, order (B, cap) i32, counts (B, 6) i32.  Asynchronous on `stream`."""
    b, cap = t["pos"].shape[0], t["pos"].shape[2]
    if t["frames"].numel() * t["frames"].element_size() != b * C.sizeof(UnprojectFrame):
        raise SlamitError("unproject_closest_batch_dev: frames does not hold one slamit_unproject_frame per frame")
    if t["kps_un"].numel() * t["kps_un"].element_size() != b * cap * KP_DTYPE.itemsize or not t["kps_un"].is_contiguous():
        raise SlamitError("unproject_closest_batch_dev: kps_un is not a contiguous (B, cap) keypoint array")
    for key, per in (("depth", 1), ("tracked", 1), ("pos", 3), ("octave", 1), ("skip", 1), ("normal", 3), ("max_dist", 1), ("min_dist", 1), ("status", 1),
                     ("order", 1)):
        if t.get(key) is not None and (t[key].numel() != b * cap * per or not t[key].is_contiguous()):
            raise SlamitError("unproject_closest_batch_dev: %s is not a contiguous (B, cap) array" % key)
    if t["n"].numel() != b or (t.get("counts") is not None and t["counts"].numel() != 6 * b):
        raise SlamitError("unproject_closest_batch_dev: n / counts do not have one entry per frame")

    def opt(key):
        return t[key].data_ptr() if t.get(key) is not None else None

    rec = UnprojectBatchRec(b, cap, t["frames"].data_ptr(), t["n"].data_ptr(), t["kps_un"].data_ptr(), t["depth"].data_ptr(), t["tracked"].data_ptr(),
                            t["pos"].data_ptr(), t["octave"].data_ptr(), t["skip"].data_ptr(), opt("normal"), opt("max_dist"), opt("min_dist"),
                            opt("status"), opt("order"), opt("counts"))
    _check(lib().slamit_unproject_closest_batch_dev(device, C.byref(rec), stream), "slamit_unproject_closest_batch_dev")


def _map_index_host(tables):
    """A map's tables (dict in the layout of slamit_map_index; a missing table is NULL) as a MapIndexRec of host pointers and the arrays
    that keep them alive."""
    keep = {}
    rec = MapIndexRec(int(tables["n_kf"]), int(tables["n_mp"]))
    for key, dt in MAP_INDEX_TABLES:
        if tables.get(key) is not None:
            keep[key] = np.ascontiguousarray(tables[key], dt).reshape(-1)
            setattr(rec, key, keep[key].ctypes.data)
    return rec, keep


def local_keyframes(tables, frame_mp, local_kf=(), ref_kf=-1, kf_cap=128, device=0):
    """Tracking::UpdateLocalKeyFrames (Tracking.cc:1512-1626) for one frame over a map's tables (dict in the layout of slamit_map_index:
    n_kf, n_mp, obs_ptr, obs_kf, mp_bad, kf_bad, kf_best (n_kf, 10), kf_child_ptr, kf_child, kf_parent; every id a slot, -1 = none).
    frame_mp: mvpMapPoints as slots; local_kf / ref_kf: the list and the reference keyframe as they stand (they survive a frame in
    which no keyframe gets a vote).  -> dict(votes (n_kf), frame_mp (bad points set to -1), local_kf (the list), n_local_kf (the
    size needed: above kf_cap the list is cut), ref_kf, status).  Voted keyframes in ascending slot order, children as given."""
    rec, keep = _map_index_host(tables)
    mp = np.array(frame_mp, np.int32).reshape(-1)
    lk = np.full(max(int(kf_cap), 0), -1, np.int32)
    cur = np.asarray(local_kf, np.int32).reshape(-1)
    if len(cur) > len(lk):
        raise SlamitError("local_keyframes: the list as it stands does not fit kf_cap")
    lk[:len(cur)] = cur
    votes = np.zeros(max(rec.n_kf, 0), np.int32)
    nlk, ref, st = np.array([len(cur)], np.int32), np.array([ref_kf], np.int32), np.zeros(1, np.int32)
    _check(lib().slamit_local_keyframes(device, C.byref(rec), len(mp), _np_ptr(mp), _np_ptr(votes), int(kf_cap), _np_ptr(lk), _np_ptr(nlk),
                                        _np_ptr(ref), _np_ptr(st)), "slamit_local_keyframes")
    del keep
    return {"votes": votes, "frame_mp": mp, "local_kf": lk[:min(int(nlk[0]), len(lk))].copy(), "n_local_kf": int(nlk[0]), "ref_kf": int(ref[0]),
            "status": int(st[0])}


def local_points(tables, frame_mp, local_kf, frame_seen=(), q_cap=4096, fill=-1, device=0):
    """Tracking::UpdateLocalPoints (Tracking.cc:1477-1509) for a keyframe list, with the skip flags of SearchLocalPoints (:1412-1437), over a
    map's tables (n_kf, n_mp, mp_bad, kf_mp_ptr, kf_mp).  frame_mp: the list local_keyframes cleaned; frame_seen: slots already seen
    this frame.  -> dict(local_mp (q_cap) int32 and skip (q_cap) uint8, entries past min(n_local_mp, q_cap) left at `fill` / 0xff,
    n_local_mp (the number needed), status)."""
    rec, keep = _map_index_host(tables)
    mp = np.ascontiguousarray(frame_mp, np.int32).reshape(-1)
    seen = np.ascontiguousarray(frame_seen, np.int32).reshape(-1)
    lk = np.ascontiguousarray(local_kf, np.int32).reshape(-1)
    out = np.full(max(int(q_cap), 0), fill, np.int32)
    skip = np.full(max(int(q_cap), 0), 0xff, np.uint8)
    nmp, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
    _check(lib().slamit_local_points(device, C.byref(rec), len(mp), _np_ptr(mp), len(seen), _np_ptr(seen) if len(seen) else None, len(lk), _np_ptr(lk),
                                     int(q_cap), _np_ptr(out), _np_ptr(skip), _np_ptr(nmp), _np_ptr(st)), "slamit_local_points")
    del keep
    return {"local_mp": out, "skip": skip, "n_local_mp": int(nmp[0]), "status": int(st[0])}


class MapIndex:
    """A map's tables uploaded once (the resident form's slamit_map_index): MapIndex(tables).rec holds the device pointers.  Nothing here
    is per frame.  Where the map changes which keyframe observes which point, map_edit_batch_dev rewrites the tables in HBM through an
    EditIndex beside this record; new keyframes and new points are appended by map_grow_batch_dev into buffers with room (GrowIndexRec
    names them); any other change is a table the caller uploads again."""

    def __init__(self, tables, device=0):
        import torch

        self.n_kf, self.n_mp, self.device = int(tables["n_kf"]), int(tables["n_mp"]), device
        self.t = {}
        self.rec = MapIndexRec(self.n_kf, self.n_mp)
        for key, dt in MAP_INDEX_TABLES:
            a = np.ascontiguousarray(tables[key], dt).reshape(-1)
            # an empty table still needs an address: the resident form refuses NULL
            self.t[key] = torch.from_numpy(a if len(a) else np.zeros(1, dt)).to("cuda:%d" % device)
            setattr(self.rec, key, self.t[key].data_ptr())


def local_map_workspace(nframes, mp_cap, kf_cap):
    return int(lib().slamit_local_map_workspace(nframes, mp_cap, kf_cap))


def local_map_batch_dev(maps, t, device=0, stream=None):
    """Tracking::UpdateLocalMap for a batch of frames, resident.  maps: a list of MapIndex; t: dict of torch CUDA tensors frame_map (B) i32,
    n (B) i32, frame_mp (B, kp_cap) i32 in / out, optionally n_seen (B) and frame_seen (B, seen_cap) i32, votes (B, vote_cap) i32,
    local_kf (B, kf_cap) i32 / n_local_kf (B) / ref_kf (B) in / out, local_mp (B, q_cap) i32, n_local_mp (B) i32, and the tensors
    frustum_batch_dev reads: pos / normal (B, 3, q_cap) f32, max_dist / min_dist (B, q_cap) f32, skip (B, q_cap) u8, m (B) i32; status (B)
    i32; workspace: uint8, local_map_workspace(B, mp_cap, kf_cap) bytes with mp_cap = t["mp_cap"] >= every map's n_mp.
    Asynchronous on `stream`."""
    b, kp_cap = t["frame_mp"].shape
    q_cap, kf_cap, vote_cap = t["local_mp"].shape[1], t["local_kf"].shape[1], t["votes"].shape[1]
    for key, per in (("frame_mp", kp_cap), ("votes", vote_cap), ("local_kf", kf_cap), ("local_mp", q_cap), ("pos", 3 * q_cap), ("normal", 3 * q_cap),
                     ("max_dist", q_cap), ("min_dist", q_cap), ("skip", q_cap), ("frame_map", 1), ("n", 1), ("n_local_kf", 1), ("ref_kf", 1),
                     ("n_local_mp", 1), ("m", 1), ("status", 1)):
        if t[key].numel() != b * per or not t[key].is_contiguous():
            raise SlamitError("local_map_batch_dev: %s is not a contiguous array of %d entries per frame" % (key, per))
    seen_cap = 0
    if t.get("frame_seen") is not None:
        seen_cap = t["frame_seen"].shape[1]
        if t["frame_seen"].numel() != b * seen_cap or not t["frame_seen"].is_contiguous() or t["n_seen"].numel() != b:
            raise SlamitError("local_map_batch_dev: frame_seen / n_seen do not hold one row per frame")
    M = (MapIndexRec * max(len(maps), 1))()
    for i, mi in enumerate(maps):
        M[i] = mi.rec
    ws = t["workspace"]
    rec = LocalMapBatchRec(b, len(maps), kp_cap, seen_cap, kf_cap, q_cap, vote_cap, int(t["mp_cap"]), M, t["frame_map"].data_ptr(), t["n"].data_ptr(),
                           t["frame_mp"].data_ptr(), t["n_seen"].data_ptr() if seen_cap or t.get("frame_seen") is not None else None,
                           t["frame_seen"].data_ptr() if t.get("frame_seen") is not None else None, t["votes"].data_ptr(), t["local_kf"].data_ptr(),
                           t["n_local_kf"].data_ptr(), t["ref_kf"].data_ptr(), t["local_mp"].data_ptr(), t["n_local_mp"].data_ptr(),
                           t["pos"].data_ptr(), t["normal"].data_ptr(), t["max_dist"].data_ptr(), t["min_dist"].data_ptr(), t["skip"].data_ptr(),
                           t["m"].data_ptr(), t["status"].data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    _check(lib().slamit_local_map_batch_dev(device, C.byref(rec), stream), "slamit_local_map_batch_dev")


def _covis_index_host(covis, copy_graph=False):
    """A map's covisibility columns and graph rows (dict in the layout of slamit_covis_index; a missing table is NULL) as a CovisIndexRec of
    host pointers and the arrays that keep them alive.  copy_graph: the graph rows are copies, for a call that rewrites them."""
    keep = {}
    rec = CovisIndexRec(int(covis["row_cap"]), int(covis["origin_kf"]))
    for key, dt in COVIS_INDEX_TABLES:
        if covis.get(key) is not None:
            keep[key] = (np.array if copy_graph and key in COVIS_GRAPH else np.ascontiguousarray)(covis[key], dt).reshape(-1)
            setattr(rec, key, keep[key].ctypes.data)
    return rec, keep


def update_connections(tables, covis, k, first_connection=False, parent=-1, device=0):
    """KeyFrame::UpdateConnections (KeyFrame.cc:296-386) for keyframe k over a map's tables (slamit_map_index: n_kf, n_mp, obs_ptr, obs_kf,
    mp_bad, kf_mp_ptr, kf_mp) and its graph (dict in the layout of slamit_covis_index: row_cap, origin_kf, cw_kf / cw_w (n_kf, row_cap), cw_n,
    ord_kf / ord_w, ord_n, optionally kf_best (n_kf, 10)).  The caller's arrays are not modified.  -> dict(counts (n_kf), n_counted,
    n_listed, parent (as given unless the list was written), status, and the seven graph arrays after the call)."""
    rec, keep = _map_index_host(tables)
    xrec, xkeep = _covis_index_host(covis, copy_graph=True)
    n_kf = max(rec.n_kf, 0)
    counts = np.zeros(n_kf, np.int32)
    nc, nl, par, st = np.zeros(1, np.int32), np.zeros(1, np.int32), np.array([parent], np.int32), np.zeros(1, np.int32)
    _check(lib().slamit_update_connections(device, C.byref(rec), C.byref(xrec), int(k), int(bool(first_connection)), _np_ptr(counts), _np_ptr(nc),
                                           _np_ptr(nl), _np_ptr(par), _np_ptr(st)), "slamit_update_connections")
    out = {"counts": counts, "n_counted": int(nc[0]), "n_listed": int(nl[0]), "parent": int(par[0]), "status": int(st[0])}
    for key in COVIS_GRAPH:
        if key in xkeep:
            out[key] = xkeep[key].reshape(np.shape(covis[key]))
    del keep
    return out


def keyframe_culling(tables, covis, c, monocular, verdict=None, n_mps=None, n_redundant=None, mp_turned_bad=None, device=0):
    """LocalMapping::KeyFrameCulling (LocalMapping.cc:686-752) for current keyframe c over a map's tables and the columns of
    slamit_covis_index (obs_octave, obs_weight, mp_nobs, kf_octave, kf_depth / kf_th_depth unless monocular, kf_not_erase, ord_kf, ord_n).
    verdict / n_mps / n_redundant (row_cap) and mp_turned_bad (n_mp) may be given as the arrays to write into (copies are returned).
    -> dict(verdict, n_mps, n_redundant: the first n_cand written; n_cand; mp_turned_bad: bytes set to 1; status).  Nothing is applied."""
    rec, keep = _map_index_host(tables)
    xrec, xkeep = _covis_index_host(covis)
    cap, n_mp = max(xrec.row_cap, 0), max(rec.n_mp, 0)
    arr = lambda a, n, dt: np.zeros(n, dt) if a is None else np.array(a, dt).reshape(-1)
    v, nm, nr, tb = arr(verdict, cap, np.uint8), arr(n_mps, cap, np.int32), arr(n_redundant, cap, np.int32), arr(mp_turned_bad, n_mp, np.uint8)
    if len(v) != cap or len(nm) != cap or len(nr) != cap or len(tb) != n_mp:
        raise SlamitError("keyframe_culling: verdict / n_mps / n_redundant hold row_cap entries, mp_turned_bad n_mp")
    ncand, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
    _check(lib().slamit_keyframe_culling(device, C.byref(rec), C.byref(xrec), int(c), int(bool(monocular)), _np_ptr(v), _np_ptr(nm), _np_ptr(nr),
                                         _np_ptr(ncand), _np_ptr(tb) if n_mp else None, _np_ptr(st)), "slamit_keyframe_culling")
    del keep, xkeep
    return {"verdict": v, "n_mps": nm, "n_redundant": nr, "n_cand": int(ncand[0]), "mp_turned_bad": tb, "status": int(st[0])}


class CovisIndex:
    """A map's covisibility columns and graph rows uploaded once, beside a MapIndex (the resident forms' slamit_covis_index):
    CovisIndex(covis, map_index).rec holds the device pointers, .t the tensors (cw_* / ord_* are rewritten in place by
    update_connections_batch_dev).  With share_best the record's kf_best IS map_index's kf_best tensor, so local_map_batch_dev reads the
    refreshed rows with no copy; otherwise covis["kf_best"] is uploaded (None: no kf_best rows are kept)."""

    def __init__(self, covis, map_index, share_best=True):
        import torch

        self.row_cap, self.device = int(covis["row_cap"]), map_index.device
        self.t = {}
        self.rec = CovisIndexRec(self.row_cap, int(covis["origin_kf"]))
        for key, dt in COVIS_INDEX_TABLES:
            if key == "kf_best" and share_best:
                self.t[key] = map_index.t["kf_best"]
            elif covis.get(key) is None:
                continue
            else:
                a = np.ascontiguousarray(covis[key], dt).reshape(-1)
                self.t[key] = torch.from_numpy(a if len(a) else np.zeros(1, dt)).to("cuda:%d" % self.device)
            setattr(self.rec, key, self.t[key].data_ptr())


def _covis_records(maps, covis):
    M, X = (MapIndexRec * max(len(maps), 1))(), (CovisIndexRec * max(len(maps), 1))()
    if len(maps) != len(covis):
        raise SlamitError("covis: one CovisIndex per MapIndex")
    for i, (mi, ci) in enumerate(zip(maps, covis)):
        M[i], X[i] = mi.rec, ci.rec
    return M, X


def _rows(t, what, specs, b):
    for key, per in specs:
        if t[key].numel() != b * per or not t[key].is_contiguous():
            raise SlamitError("%s: %s is not a contiguous array of %d entries per row" % (what, key, per))


def update_connections_batch_dev(maps, covis, item_map, t, device=0, stream=None):
    """KeyFrame::UpdateConnections for one keyframe of each of len(item_map) DIFFERENT maps, resident.  maps / covis: lists of MapIndex /
    CovisIndex; item_map: host list, item i works on maps[item_map[i]]; t: dict of torch CUDA tensors kf (B) i32, first (B) i32, counts
    (B, count_cap) i32, n_counted (B), n_listed (B), parent (B) in / out, status (B).  The graph rows of the CovisIndex tensors (and the
    kf_best rows they share with the MapIndex) are rewritten in place.  Asynchronous on `stream`."""
    b = len(item_map)
    count_cap = t["counts"].shape[1] if t["counts"].dim() == 2 else 0
    _rows(t, "update_connections_batch_dev", (("counts", count_cap), ("kf", 1), ("first", 1), ("n_counted", 1), ("n_listed", 1), ("parent", 1), ("status", 1)), b)
    M, X = _covis_records(maps, covis)
    im = (C.c_int32 * max(b, 1))(*[int(m) for m in item_map])
    rec = CovisBatchRec(b, len(maps), count_cap, 0, M, X, im, t["kf"].data_ptr(), t["first"].data_ptr(), t["counts"].data_ptr(), t["n_counted"].data_ptr(),
                        t["n_listed"].data_ptr(), t["parent"].data_ptr(), t["status"].data_ptr())
    _check(lib().slamit_update_connections_batch_dev(device, C.byref(rec), stream), "slamit_update_connections_batch_dev")


def keyframe_culling_batch_dev(maps, covis, t, device=0, stream=None):
    """LocalMapping::KeyFrameCulling for a batch of current keyframes, resident.  t: dict of torch CUDA tensors prob_map (B) i32, kf (B) i32,
    monocular (B) i32, verdict (B, cand_cap) u8 / n_mps / n_redundant (B, cand_cap) i32 in / out, n_cand (B) i32, mp_turned_bad (B, mp_cap) u8
    in / out, status (B) i32; cand_cap >= every row_cap, mp_cap >= every n_mp.  Asynchronous on `stream`."""
    b, cand_cap = t["verdict"].shape
    mp_cap = t["mp_turned_bad"].shape[1]
    _rows(t, "keyframe_culling_batch_dev", (("verdict", cand_cap), ("n_mps", cand_cap), ("n_redundant", cand_cap), ("mp_turned_bad", mp_cap), ("prob_map", 1),
                                             ("kf", 1), ("monocular", 1), ("n_cand", 1), ("status", 1)), b)
    M, X = _covis_records(maps, covis)
    rec = CullingBatchRec(b, len(maps), cand_cap, mp_cap, M, X, t["prob_map"].data_ptr(), t["kf"].data_ptr(), t["monocular"].data_ptr(),
                          t["verdict"].data_ptr(), t["n_mps"].data_ptr(), t["n_redundant"].data_ptr(), t["n_cand"].data_ptr(),
                          t["mp_turned_bad"].data_ptr(), t["status"].data_ptr())
    _check(lib().slamit_keyframe_culling_batch_dev(device, C.byref(rec), stream), "slamit_keyframe_culling_batch_dev")


def _point_index_host(pts, copy_planes=False):
    """A map's point columns (dict in the layout of slamit_point_index: n_levels, scale_factors and the tables; a missing table is NULL) as a
    PointIndexRec of host pointers and the arrays that keep them alive.  copy_planes: the in / out planes are copies, for a call that rewrites them."""
    keep = {}
    rec = PointIndexRec(int(pts["n_levels"]), 0)
    sf = np.asarray(pts["scale_factors"], np.float32).reshape(-1)[:16]
    rec.scale_factors[:len(sf)] = sf.tolist()
    for key, dt in POINT_INDEX_TABLES:
        if pts.get(key) is not None:
            keep[key] = (np.array if copy_planes and key in POINT_PLANES else np.ascontiguousarray)(pts[key], dt).reshape(-1)
            setattr(rec, key, keep[key].ctypes.data)
    return rec, keep


def update_points(tables, pts, points, what=UPKEEP_NORMAL | UPKEEP_DESC, device=0):
    """MapPoint::UpdateNormalAndDepth (what & 1) and ::ComputeDistinctiveDescriptors (what & 2) (MapPoint.cc:248-377) for the listed points
    over a map's tables (slamit_map_index: n_kf, n_mp, obs_ptr, obs_kf, mp_bad, kf_bad, kf_mp_ptr, mp_pos) and its point columns (dict in the
    layout of slamit_point_index).  The caller's arrays are not modified.  -> dict(status (n), mp_normal (n_mp, 3), mp_max_dist, mp_min_dist
    (n_mp), mp_desc (n_mp, 32) after the call, where given)."""
    rec, keep = _map_index_host(tables)
    xrec, xkeep = _point_index_host(pts, copy_planes=True)
    lst = np.ascontiguousarray(points, np.int32).reshape(-1)
    st = np.zeros(len(lst), np.int32)
    _check(lib().slamit_update_points(device, C.byref(rec), C.byref(xrec), len(lst), _np_ptr(lst) if len(lst) else None, int(what),
                                      _np_ptr(st) if len(lst) else None), "slamit_update_points")
    out = {"status": st}
    for key in POINT_PLANES:
        if key in xkeep:
            out[key] = xkeep[key].reshape(np.shape(pts[key]))
    del keep
    return out


def map_point_culling(tables, pts, cur_id, monocular, recent, verdict=None, kept=None, device=0):
    """LocalMapping::MapPointCulling (LocalMapping.cc:184-219) for a recent list over a map's mp_bad and the columns mp_nobs, mp_found,
    mp_visible, mp_first_kf.  verdict / kept (n) may be given as the arrays to write into (copies are returned).  -> dict(verdict (n) uint8,
    kept (n) int32 of which the first n_kept are written, n_kept, status).  Nothing is applied."""
    rec, keep = _map_index_host(tables)
    xrec, xkeep = _point_index_host(pts)
    lst = np.ascontiguousarray(recent, np.int32).reshape(-1)
    n = len(lst)
    v = np.zeros(n, np.uint8) if verdict is None else np.array(verdict, np.uint8).reshape(-1)
    kp = np.full(n, -1, np.int32) if kept is None else np.array(kept, np.int32).reshape(-1)
    if len(v) != n or len(kp) != n:
        raise SlamitError("map_point_culling: verdict and kept hold one entry per entry of the list")
    nk, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
    ptr = lambda a: _np_ptr(a) if n else None
    _check(lib().slamit_map_point_culling(device, C.byref(rec), C.byref(xrec), int(cur_id), int(bool(monocular)), n, ptr(lst), ptr(v), ptr(kp),
                                          _np_ptr(nk), _np_ptr(st)), "slamit_map_point_culling")
    del keep, xkeep
    return {"verdict": v, "kept": kp, "n_kept": int(nk[0]), "status": int(st[0])}


class PointIndex:
    """A map's point columns uploaded once, beside a MapIndex (the resident forms' slamit_point_index): PointIndex(pts, map_index).rec holds
    the device pointers, .t the tensors.  mp_normal, mp_max_dist and mp_min_dist ARE map_index's tensors of the same names, so
    update_points_batch_dev rewrites the planes local_map_batch_dev gathers, with no copy; mp_desc is uploaded from pts."""

    def __init__(self, pts, map_index):
        import torch

        self.device = map_index.device
        self.t = {}
        self.rec = PointIndexRec(int(pts["n_levels"]), 0)
        sf = np.asarray(pts["scale_factors"], np.float32).reshape(-1)[:16]
        self.rec.scale_factors[:len(sf)] = sf.tolist()
        for key, dt in POINT_INDEX_TABLES:
            if key in ("mp_normal", "mp_max_dist", "mp_min_dist"):
                self.t[key] = map_index.t[key]
            else:
                a = np.ascontiguousarray(pts[key], dt).reshape(-1)
                self.t[key] = torch.from_numpy(a if len(a) else np.zeros(32, dt)).to("cuda:%d" % self.device)
            setattr(self.rec, key, self.t[key].data_ptr())


def _point_records(maps, pts):
    M, X = (MapIndexRec * max(len(maps), 1))(), (PointIndexRec * max(len(maps), 1))()
    if len(maps) != len(pts):
        raise SlamitError("upkeep: one PointIndex per MapIndex")
    for i, (mi, pi) in enumerate(zip(maps, pts)):
        M[i], X[i] = mi.rec, pi.rec
    return M, X


def update_points_batch_dev(maps, pts, t, device=0, stream=None):
    """UpdateNormalAndDepth / ComputeDistinctiveDescriptors for a batch of point lists, resident.  maps / pts: lists of MapIndex / PointIndex;
    t: dict of torch CUDA tensors item_map (B) i32, n (B) i32, what (B) i32, points (B, cap) i32, status (B, cap) i32 out.  The planes of the
    PointIndex tensors (shared with the MapIndex) are rewritten in place.  Asynchronous on `stream`."""
    b, cap = t["points"].shape
    _rows(t, "update_points_batch_dev", (("points", cap), ("status", cap), ("item_map", 1), ("n", 1), ("what", 1)), b)
    M, X = _point_records(maps, pts)
    rec = PointsBatchRec(b, len(maps), cap, 0, M, X, t["item_map"].data_ptr(), t["n"].data_ptr(), t["what"].data_ptr(), t["points"].data_ptr(),
                         t["status"].data_ptr())
    _check(lib().slamit_update_points_batch_dev(device, C.byref(rec), stream), "slamit_update_points_batch_dev")


def map_point_culling_batch_dev(maps, pts, t, device=0, stream=None):
    """LocalMapping::MapPointCulling for a batch of recent lists, resident.  t: dict of torch CUDA tensors list_map (B) i32, cur_id (B) i32,
    monocular (B) i32, n (B) i32, recent (B, cap) i32, verdict (B, cap) u8 / kept (B, cap) i32 in / out, n_kept (B) i32, status (B) i32.
    Asynchronous on `stream`."""
    b, cap = t["recent"].shape
    _rows(t, "map_point_culling_batch_dev", (("recent", cap), ("verdict", cap), ("kept", cap), ("list_map", 1), ("cur_id", 1), ("monocular", 1), ("n", 1),
                                              ("n_kept", 1), ("status", 1)), b)
    M, X = _point_records(maps, pts)
    rec = PointCullingBatchRec(b, len(maps), cap, 0, M, X, t["list_map"].data_ptr(), t["cur_id"].data_ptr(), t["monocular"].data_ptr(), t["n"].data_ptr(),
                               t["recent"].data_ptr(), t["verdict"].data_ptr(), t["kept"].data_ptr(), t["n_kept"].data_ptr(), t["status"].data_ptr())
    _check(lib().slamit_map_point_culling_batch_dev(device, C.byref(rec), stream), "slamit_map_point_culling_batch_dev")


def edit_records(edits):
    """Edits as an array of slamit_map_edit: an EDIT_DTYPE array as it is, else rows (kind, flags, mp, kf, idx, octave, weight)."""
    if isinstance(edits, np.ndarray) and edits.dtype == EDIT_DTYPE:
        return np.ascontiguousarray(edits).reshape(-1)
    rows = list(edits)
    out = np.zeros(len(rows), EDIT_DTYPE)
    for i, r in enumerate(rows):
        out[i] = tuple(int(v) for v in r) + ((0, 0),)
    return out


def map_edit(tables, edit, edits, obs_cap_out=None, fill=None, device=0):
    """MapPoint::AddObservation / ::EraseObservation / ::SetBadFlag with the keyframes' side (MapPoint.cc:104-174, KeyFrame.cc:215-243) for
    a list of edits applied as if sequentially, over a map's tables (slamit_map_index: n_kf, n_mp, obs_ptr, obs_kf, kf_mp_ptr, kf_mp,
    mp_bad) and its edit columns (dict: obs_idx, obs_octave, obs_weight beside obs_kf; mp_nobs, mp_ref_kf; mp_bad / kf_mp where they are
    not taken from `tables`).  edits: edit_records().  The caller's arrays are not modified.  obs_cap_out: the room of the new table
    (default: the old table plus one entry per edit).  fill: optional dict of prefilled output arrays (obs_ptr_out, obs_kf_out, obs_idx_out,
    obs_octave_out, obs_weight_out, status_mp, touched, n_touched), copied.  -> dict: obs_ptr, obs_kf, mp_bad, kf_mp (what MapIndex /
    _map_index_host take in place of the old ones: dict(tables, **{k: out[k] for k in ("obs_ptr", "obs_kf", "mp_bad", "kf_mp")})),
    obs_idx, obs_octave, obs_weight, mp_nobs, mp_ref_kf, status_mp (n_mp), touched (the first n_touched of it), n_touched, n_obs_out,
    status, and `raw`: the output arrays in full.  With EDIT_STATUS["TABLE_OVERFLOW"] the tables returned are the old ones."""
    rec, keep = _map_index_host(tables)
    n_mp = max(rec.n_mp, 0)
    ed = edit_records(edits)
    src = dict(edit)
    for key in ("mp_bad", "kf_mp"):
        src.setdefault(key, tables.get(key))
    n_obs = int(np.asarray(tables["obs_ptr"]).reshape(-1)[-1]) if tables.get("obs_ptr") is not None and len(np.asarray(tables["obs_ptr"]).reshape(-1)) else 0
    cap = n_obs + len(ed) if obs_cap_out is None else int(obs_cap_out)
    fill = fill or {}
    xrec, xkeep = EditIndexRec(), {}
    for key, dt in EDIT_INDEX_COLUMNS:
        if src.get(key) is not None:
            xkeep[key] = np.ascontiguousarray(src[key], dt).reshape(-1)
            setattr(xrec, key, xkeep[key].ctypes.data)
    for key, dt in EDIT_INDEX_INPLACE:
        if src.get(key) is not None:
            xkeep[key] = np.array(src[key], dt).reshape(-1)
            setattr(xrec, key, xkeep[key].ctypes.data)
    for key, dt, count in (("obs_ptr_out", np.int32, n_mp + 1),) + tuple((k, d, max(cap, 0)) for k, d in EDIT_INDEX_OUT):
        xkeep[key] = np.zeros(count, dt) if fill.get(key) is None else np.array(fill[key], dt).reshape(-1)
        if len(xkeep[key]) != count:
            raise SlamitError("map_edit: fill[%s] does not hold %d entries" % (key, count))
        setattr(xrec, key, xkeep[key].ctypes.data if count else None)
    xrec.obs_cap_out = cap
    st_mp = np.zeros(n_mp, np.int32) if fill.get("status_mp") is None else np.array(fill["status_mp"], np.int32).reshape(-1)
    tch = np.full(n_mp, -1, np.int32) if fill.get("touched") is None else np.array(fill["touched"], np.int32).reshape(-1)
    if len(st_mp) != n_mp or len(tch) != n_mp:
        raise SlamitError("map_edit: status_mp and touched hold n_mp entries")
    nt, no, st = np.array([fill.get("n_touched", 0)], np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    _check(lib().slamit_map_edit_apply(device, C.byref(rec), C.byref(xrec), len(ed), _np_ptr(ed) if len(ed) else None, _np_ptr(st_mp) if n_mp else None,
                                       _np_ptr(tch) if n_mp else None, _np_ptr(nt), _np_ptr(no), _np_ptr(st)), "slamit_map_edit_apply")
    del keep
    status, need = int(st[0]), int(no[0])
    out = {"status": status, "n_obs_out": need, "n_touched": int(nt[0]), "status_mp": st_mp, "raw": dict(xkeep, status_mp=st_mp, touched=tch)}
    if status & EDIT_STATUS["TABLE_OVERFLOW"]:
        out.update(obs_ptr=np.array(tables["obs_ptr"], np.int32).reshape(-1), obs_kf=np.array(tables["obs_kf"], np.int32).reshape(-1), touched=tch[:0])
        for key, _ in EDIT_INDEX_COLUMNS:
            out[key] = xkeep[key].copy()
    else:
        out.update(obs_ptr=xkeep["obs_ptr_out"], obs_kf=xkeep["obs_kf_out"][:need], touched=tch[:int(nt[0])])
        for key, _ in EDIT_INDEX_COLUMNS:
            out[key] = xkeep[key + "_out"][:need]
    for key, _ in EDIT_INDEX_INPLACE:
        out[key] = xkeep.get(key)
    return out


class EditIndex:
    """The arrays map_edit_batch_dev reads and writes beside a MapIndex (the resident form's slamit_edit_index), with TWO buffer sets for
    the observation table.  EditIndex(edit, map_index, obs_cap, covis=None, points=None): obs_idx / obs_octave / obs_weight and mp_nobs /
    mp_ref_kf are uploaded from `edit` unless a CovisIndex / PointIndex is given, whose tensors are then used (and whose records follow
    every swap); mp_bad and kf_mp ARE map_index's tensors, rewritten in place.  obs_cap: entries each buffer set of the table holds.
    .rec reads the current set and writes the other; after map_edit_batch_dev has run, swap() makes the written set the current one in
    map_index.rec (and the covis / points records) and the old one the next target, so every reader takes the new table unchanged."""

    def __init__(self, edit, map_index, obs_cap, covis=None, points=None):
        import torch

        self.map_index, self.covis, self.points, self.device, self.obs_cap = map_index, covis, points, map_index.device, int(obs_cap)
        dev = "cuda:%d" % self.device
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1) if np.size(a) else np.zeros(1, dt)).to(dev)
        room = lambda t: torch.cat([t, torch.zeros(max(self.obs_cap, 1) - t.numel(), dtype=t.dtype, device=dev)]) if t.numel() < max(self.obs_cap, 1) else t
        cur = {"obs_ptr": map_index.t["obs_ptr"], "obs_kf": room(map_index.t["obs_kf"])}
        cur["obs_idx"] = room(points.t["obs_idx"] if points is not None else up(edit["obs_idx"], np.int32))
        cur["obs_octave"] = room(covis.t["obs_octave"] if covis is not None else points.t["obs_octave"] if points is not None else up(edit["obs_octave"], np.uint8))
        cur["obs_weight"] = room(covis.t["obs_weight"] if covis is not None else up(edit["obs_weight"], np.uint8))
        self.sets = [cur, {k: torch.zeros_like(v) for k, v in cur.items()}]
        self.t = {"mp_bad": map_index.t["mp_bad"], "kf_mp": map_index.t["kf_mp"]}
        self.t["mp_nobs"] = covis.t["mp_nobs"] if covis is not None else points.t["mp_nobs"] if points is not None else up(edit["mp_nobs"], np.int32)
        self.t["mp_ref_kf"] = points.t["mp_ref_kf"] if points is not None else up(edit["mp_ref_kf"], np.int32)
        if covis is not None and points is not None:   # one memory for what both records name
            points.t["mp_nobs"] = self.t["mp_nobs"]
            points.rec.mp_nobs = self.t["mp_nobs"].data_ptr()
        self.rec = EditIndexRec()
        self.followers = []   # called after every repointing: a ReplaceIndex over the same buffer sets
        self._point()

    def _point(self):
        cur, nxt = self.sets
        mi = self.map_index
        mi.t["obs_ptr"], mi.t["obs_kf"] = cur["obs_ptr"], cur["obs_kf"]
        mi.rec.obs_ptr, mi.rec.obs_kf = cur["obs_ptr"].data_ptr(), cur["obs_kf"].data_ptr()
        for idx, keys in ((self.covis, ("obs_octave", "obs_weight")), (self.points, ("obs_idx", "obs_octave"))):
            if idx is not None:
                for key in keys:
                    idx.t[key] = cur[key]
                    setattr(idx.rec, key, cur[key].data_ptr())
        for key in ("obs_idx", "obs_octave", "obs_weight"):
            setattr(self.rec, key, cur[key].data_ptr())
        for key in ("mp_bad", "mp_nobs", "mp_ref_kf", "kf_mp"):
            setattr(self.rec, key, self.t[key].data_ptr())
        self.rec.obs_ptr_out = nxt["obs_ptr"].data_ptr()
        for key in ("obs_kf", "obs_idx", "obs_octave", "obs_weight"):
            setattr(self.rec, key + "_out", nxt[key].data_ptr())
        self.rec.obs_cap_out = self.obs_cap
        for follow in self.followers:
            follow()

    def swap(self):
        """The table the last call wrote becomes the one every record reads; no copy, no synchronisation."""
        self.sets.reverse()
        self._point()


def map_edit_workspace(n_maps, cap, mp_cap, kfmp_cap):
    return int(lib().slamit_map_edit_workspace(n_maps, cap, mp_cap, kfmp_cap))


def map_edit_batch_dev(maps, edit, t, device=0, stream=None):
    """One edit list per map, resident.  maps / edit: lists of MapIndex / EditIndex; t: dict of torch CUDA tensors edits (B, cap, 24) u8 (the
    bytes of EDIT_DTYPE records), n (B) i32, status_mp (B, mp_cap) i32, touched (B, mp_cap) i32 in / out, n_touched (B), n_obs_out (B),
    status (B) i32, workspace: uint8, map_edit_workspace(B, cap, mp_cap, kfmp_cap) bytes with kfmp_cap = t["kfmp_cap"] >= every map's
    number of kf_mp entries.  The new tables are written into each EditIndex's other buffer set: call swap() on each before the next
    reader is ENQUEUED (the swap is host bookkeeping; the stream orders the work).  Asynchronous on `stream`."""
    b, cap = t["edits"].shape[0], t["edits"].shape[1]
    mp_cap = t["status_mp"].shape[1]
    if len(maps) != b or len(edit) != b:
        raise SlamitError("map_edit_batch_dev: one MapIndex, one EditIndex and one list per map")
    _rows(t, "map_edit_batch_dev", (("edits", cap * EDIT_DTYPE.itemsize), ("status_mp", mp_cap), ("touched", mp_cap), ("n", 1), ("n_touched", 1), ("n_obs_out", 1),
                                    ("status", 1)), b)
    M, X = (MapIndexRec * max(b, 1))(), (EditIndexRec * max(b, 1))()
    for i, (mi, ei) in enumerate(zip(maps, edit)):
        M[i], X[i] = mi.rec, ei.rec
    ws = t["workspace"]
    rec = MapEditBatchRec(b, cap, mp_cap, int(t["kfmp_cap"]), M, X, t["edits"].data_ptr(), t["n"].data_ptr(), t["status_mp"].data_ptr(), t["touched"].data_ptr(),
                          t["n_touched"].data_ptr(), t["n_obs_out"].data_ptr(), t["status"].data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    _check(lib().slamit_map_edit_batch_dev(device, C.byref(rec), stream), "slamit_map_edit_batch_dev")


def replace_records(ops):
    """Ops as an array of slamit_map_replace: a REPLACE_DTYPE array as it is, else rows (kind, a, b, idx, octave, weight)."""
    if isinstance(ops, np.ndarray) and ops.dtype == REPLACE_DTYPE:
        return np.ascontiguousarray(ops).reshape(-1)
    rows = list(ops)
    out = np.zeros(len(rows), REPLACE_DTYPE)
    for i, r in enumerate(rows):
        out[i] = tuple(int(v) for v in r) + ((0, 0),)
    return out


def map_replace(tables, index, ops, obs_cap_out=None, fill=None, device=0):
    """MapPoint::Replace with Fuse's add pair for a list of ops: the arguments and the result are stated at _map_list_apply."""
    return _map_list_apply(False, tables, index, ops, obs_cap_out, fill, device)


def map_fuse(tables, cols, ops, obs_cap_out=None, fill=None, device=0):
    """The tail of ORBmatcher::Fuse (ORBmatcher.cc:853, :955-975) for a list of ops applied as if sequentially: map_replace's arguments
    and result, with ops of kind FUSE_FUSE (a = P, b = the keyframe, idx = the matched keypoint or -1, octave, weight) beside the other
    two, obs_cap_out defaulting to the old table plus one entry per ADD_OBS and FUSE op, `outcome` among the prefilled outputs, and in
    the result outcome (FUSE_OUT per op) and n_fused (the reference's return value).  With a bit of FUSE_REFUSED in status the tables
    returned are the old ones."""
    return _map_list_apply(True, tables, cols, ops, obs_cap_out, fill, device)


def _map_list_apply(fuse, tables, index, ops, obs_cap_out, fill, device):
    """MapPoint::Replace (MapPoint.cc:183-221) with Fuse's AddObservation + AddMapPoint for a list of ops applied as if sequentially, over
    a map's tables (slamit_map_index: n_kf, n_mp, obs_ptr, obs_kf, kf_mp_ptr, kf_mp, mp_bad) and the columns beside them (dict: obs_idx,
    obs_octave, obs_weight; mp_nobs, mp_found, mp_visible, mp_replaced; mp_bad / kf_mp where they are not taken from `tables`).  ops:
    replace_records().  The caller's arrays are not modified.  obs_cap_out: the room of the new table (default: the old table plus one
    entry per ADD_OBS op, which always suffices).  fill: optional dict of prefilled outputs (obs_ptr_out, obs_kf_out, obs_idx_out,
    obs_octave_out, obs_weight_out, moved, erased, touched, n_touched, n_obs_out), copied.  -> dict: obs_ptr, obs_kf, mp_bad, kf_mp (what
    MapIndex / _map_index_host take in place of the old ones), obs_idx, obs_octave, obs_weight, mp_nobs, mp_found, mp_visible,
    mp_replaced, moved, erased (per op), touched (the first n_touched of it), n_touched, n_obs_out, status, and `raw`: the output arrays
    in full.  With a bit of REPLACE_REFUSED in status the tables returned are the old ones."""
    rec, keep = _map_index_host(tables)
    n_mp = max(rec.n_mp, 0)
    ed = replace_records(ops)
    src = dict(index)
    for key in ("mp_bad", "kf_mp"):
        src.setdefault(key, tables.get(key))
    n_obs = int(np.asarray(tables["obs_ptr"]).reshape(-1)[-1]) if tables.get("obs_ptr") is not None and len(np.asarray(tables["obs_ptr"]).reshape(-1)) else 0
    cap = n_obs + int(np.count_nonzero((ed["kind"] == REPLACE_ADD_OBS) | (fuse & (ed["kind"] == FUSE_FUSE)))) if obs_cap_out is None else int(obs_cap_out)
    name = "map_fuse" if fuse else "map_replace"
    fill = fill or {}
    xrec, xkeep = ReplaceIndexRec(), {}
    for key, dt in EDIT_INDEX_COLUMNS:
        if src.get(key) is not None:
            xkeep[key] = np.ascontiguousarray(src[key], dt).reshape(-1)
            setattr(xrec, key, xkeep[key].ctypes.data)
    for key, dt in REPLACE_INDEX_INPLACE:
        if src.get(key) is not None:
            xkeep[key] = np.array(src[key], dt).reshape(-1)
            setattr(xrec, key, xkeep[key].ctypes.data)
    for key, dt, count in (("obs_ptr_out", np.int32, n_mp + 1),) + tuple((k, d, max(cap, 0)) for k, d in EDIT_INDEX_OUT):
        xkeep[key] = np.zeros(count, dt) if fill.get(key) is None else np.array(fill[key], dt).reshape(-1)
        if len(xkeep[key]) != count:
            raise SlamitError("%s: fill[%s] does not hold %d entries" % (name, key, count))
        setattr(xrec, key, xkeep[key].ctypes.data if count else None)
    xrec.obs_cap_out = cap
    per_op = {key: np.zeros(len(ed), np.int32) if fill.get(key) is None else np.array(fill[key], np.int32).reshape(-1) for key in ("moved", "erased") + (("outcome",) if fuse else ())}
    tch = np.full(n_mp, -1, np.int32) if fill.get("touched") is None else np.array(fill["touched"], np.int32).reshape(-1)
    if len(tch) != n_mp or any(len(v) != len(ed) for v in per_op.values()):
        raise SlamitError("%s: moved and erased hold one entry per op, touched n_mp entries" % name)
    nt, no, st = np.array([fill.get("n_touched", 0)], np.int32), np.array([fill.get("n_obs_out", 0)], np.int32), np.zeros(1, np.int32)
    nf = np.array([fill.get("n_fused", 0)], np.int32)
    some = lambda a: _np_ptr(a) if len(a) else None
    if fuse:
        _check(lib().slamit_map_fuse_apply(device, C.byref(rec), C.byref(xrec), len(ed), some(ed), some(per_op["outcome"]), some(per_op["moved"]),
                                           some(per_op["erased"]), some(tch), _np_ptr(nt), _np_ptr(nf), _np_ptr(no), _np_ptr(st)), "slamit_map_fuse_apply")
    else:
        _check(lib().slamit_map_replace_apply(device, C.byref(rec), C.byref(xrec), len(ed), some(ed), some(per_op["moved"]), some(per_op["erased"]), some(tch),
                                              _np_ptr(nt), _np_ptr(no), _np_ptr(st)), "slamit_map_replace_apply")
    del keep
    status, need = int(st[0]), int(no[0])
    out = {"status": status, "n_obs_out": need, "n_touched": int(nt[0]), "moved": per_op["moved"], "erased": per_op["erased"],
           "raw": dict(xkeep, touched=tch, n_touched=int(nt[0]), n_obs_out=need, **per_op)}
    if fuse:
        out.update(outcome=per_op["outcome"], n_fused=int(nf[0]))
        out["raw"]["n_fused"] = int(nf[0])
    if status & REPLACE_REFUSED:
        out.update(obs_ptr=np.array(tables["obs_ptr"], np.int32).reshape(-1), obs_kf=np.array(tables["obs_kf"], np.int32).reshape(-1), touched=tch[:0])
        for key, _ in EDIT_INDEX_COLUMNS:
            out[key] = xkeep[key].copy()
    else:
        out.update(obs_ptr=xkeep["obs_ptr_out"], obs_kf=xkeep["obs_kf_out"][:need], touched=tch[:int(nt[0])])
        for key, _ in EDIT_INDEX_COLUMNS:
            out[key] = xkeep[key + "_out"][:need]
    for key, _ in REPLACE_INDEX_INPLACE:
        out[key] = xkeep.get(key)
    return out


class ReplaceIndex:
    """The arrays map_replace_batch_dev reads and writes beside a MapIndex (the resident form's slamit_replace_index).  ReplaceIndex(
    edit_index, cols) SHARES the EditIndex's two buffer sets of the observation table and its in-place tensors, so one swap() of the
    EditIndex repoints this record with every other.  mp_found / mp_visible are the PointIndex's tensors where the EditIndex has one,
    else uploaded from cols; mp_replaced is uploaded from cols (default: -1 everywhere) and kept in .t for check_replaced_batch_dev."""

    def __init__(self, edit_index, cols=None):
        import torch

        cols = cols or {}
        self.edit_index, self.device = edit_index, edit_index.device
        dev = "cuda:%d" % self.device
        n_mp = max(int(edit_index.map_index.rec.n_mp), 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32).reshape(-1) if np.size(a) else np.zeros(1, np.int32)).to(dev)
        pts = edit_index.points
        self.t = {"mp_found": pts.t["mp_found"] if pts is not None else up(cols["mp_found"]),
                  "mp_visible": pts.t["mp_visible"] if pts is not None else up(cols["mp_visible"]),
                  "mp_replaced": up(cols["mp_replaced"] if cols.get("mp_replaced") is not None else np.full(max(n_mp, 1), -1, np.int32))}
        self.rec = ReplaceIndexRec()
        edit_index.followers.append(self._point)
        self._point()

    def _point(self):
        e = self.edit_index.rec
        for key in ("obs_idx", "obs_octave", "obs_weight", "mp_bad", "mp_nobs", "kf_mp", "obs_ptr_out", "obs_kf_out", "obs_idx_out", "obs_octave_out", "obs_weight_out",
                    "obs_cap_out"):
            setattr(self.rec, key, getattr(e, key))
        for key in ("mp_found", "mp_visible", "mp_replaced"):
            setattr(self.rec, key, self.t[key].data_ptr())


def map_replace_workspace(n_maps, cap, mp_cap, kfmp_cap):
    return int(lib().slamit_map_replace_workspace(n_maps, cap, mp_cap, kfmp_cap))


def map_replace_batch_dev(maps, index, t, device=0, stream=None):
    """One op list per map, resident.  maps / index: lists of MapIndex / ReplaceIndex; t: dict of torch CUDA tensors ops (B, cap, 20) u8 (the
    bytes of REPLACE_DTYPE records), n (B) i32, moved (B, cap) / erased (B, cap) / touched (B, mp_cap) i32 in / out, n_touched (B),
    n_obs_out (B), status (B) i32, workspace: uint8, map_replace_workspace(B, cap, mp_cap, kfmp_cap) bytes with kfmp_cap = t["kfmp_cap"]
    >= every map's number of kf_mp entries.  The new tables are written into each EditIndex's other buffer set: where status has no bit of
    REPLACE_REFUSED, call swap() on the EditIndex before the next reader is ENQUEUED.  Asynchronous on `stream`."""
    b, cap = t["ops"].shape[0], t["ops"].shape[1]
    mp_cap = t["touched"].shape[1]
    if len(maps) != b or len(index) != b:
        raise SlamitError("map_replace_batch_dev: one MapIndex, one ReplaceIndex and one list per map")
    _rows(t, "map_replace_batch_dev", (("ops", cap * REPLACE_DTYPE.itemsize), ("moved", cap), ("erased", cap), ("touched", mp_cap), ("n", 1), ("n_touched", 1),
                                       ("n_obs_out", 1), ("status", 1)), b)
    M, X = (MapIndexRec * max(b, 1))(), (ReplaceIndexRec * max(b, 1))()
    for i, (mi, ri) in enumerate(zip(maps, index)):
        M[i], X[i] = mi.rec, ri.rec
    ws = t["workspace"]
    rec = MapReplaceBatchRec(b, cap, mp_cap, int(t["kfmp_cap"]), M, X, t["ops"].data_ptr(), t["n"].data_ptr(), t["moved"].data_ptr(), t["erased"].data_ptr(),
                             t["touched"].data_ptr(), t["n_touched"].data_ptr(), t["n_obs_out"].data_ptr(), t["status"].data_ptr(), ws.data_ptr(),
                             ws.numel() * ws.element_size())
    _check(lib().slamit_map_replace_batch_dev(device, C.byref(rec), stream), "slamit_map_replace_batch_dev")


def map_fuse_workspace(n_maps, cap, mp_cap, kfmp_cap):
    return int(lib().slamit_map_fuse_workspace(n_maps, cap, mp_cap, kfmp_cap))


def map_fuse_batch_dev(maps, index, t, device=0, stream=None):
    """One fuse list per map, resident: map_replace_batch_dev's arguments, the lists holding FUSE ops too, with outcome (B, cap) and n_fused
    (B) i32 in / out beside the others and workspace of map_fuse_workspace(B, cap, mp_cap, kfmp_cap) bytes.  Where status has no bit of
    FUSE_REFUSED, call swap() on the EditIndex before the next reader is ENQUEUED.  Asynchronous on `stream`."""
    b, cap = t["ops"].shape[0], t["ops"].shape[1]
    mp_cap = t["touched"].shape[1]
    if len(maps) != b or len(index) != b:
        raise SlamitError("map_fuse_batch_dev: one MapIndex, one ReplaceIndex and one list per map")
    _rows(t, "map_fuse_batch_dev", (("ops", cap * REPLACE_DTYPE.itemsize), ("outcome", cap), ("moved", cap), ("erased", cap), ("touched", mp_cap), ("n", 1),
                                    ("n_touched", 1), ("n_fused", 1), ("n_obs_out", 1), ("status", 1)), b)
    M, X = (MapIndexRec * max(b, 1))(), (ReplaceIndexRec * max(b, 1))()
    for i, (mi, ri) in enumerate(zip(maps, index)):
        M[i], X[i] = mi.rec, ri.rec
    ws = t["workspace"]
    rec = MapFuseBatchRec(b, cap, mp_cap, int(t["kfmp_cap"]), M, X, t["ops"].data_ptr(), t["n"].data_ptr(), t["outcome"].data_ptr(), t["moved"].data_ptr(),
                          t["erased"].data_ptr(), t["touched"].data_ptr(), t["n_touched"].data_ptr(), t["n_fused"].data_ptr(), t["n_obs_out"].data_ptr(),
                          t["status"].data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    _check(lib().slamit_map_fuse_batch_dev(device, C.byref(rec), stream), "slamit_map_fuse_batch_dev")


def fuse_list_batch_dev(t, n_maps, device=0, stream=None):
    """The FUSE ops of a guided search into the lists map_fuse_batch_dev reads, resident.  t: dict of torch CUDA tensors match_kp (F, q_cap)
    i32 and m (F) i32 as the search left them, query_point (F, q_cap) i32, kps_un (F, kp_cap, 28) u8 or (F, kp_cap, 7) f32 (slamit_kp records), kp_ur (F, kp_cap)
    f32 or None, frame_map / frame_kf / base (F) i32, and the outputs ops (n_maps, cap, 20) u8, n (n_maps) i32, list_status (F) i32.
    Asynchronous on `stream`."""
    f, q_cap = t["match_kp"].shape[0], t["match_kp"].shape[1]
    kp_cap, cap = t["kps_un"].shape[1], t["ops"].shape[1]
    if t["ops"].shape[0] != n_maps or t["n"].numel() < n_maps:
        raise SlamitError("fuse_list_batch_dev: one list and one length per map")
    if t["kps_un"].numel() * t["kps_un"].element_size() != f * kp_cap * 28 or not t["kps_un"].is_contiguous():
        raise SlamitError("fuse_list_batch_dev: kps_un does not hold kp_cap slamit_kp records per target")
    _rows(t, "fuse_list_batch_dev", (("match_kp", q_cap), ("query_point", q_cap), ("m", 1), ("frame_map", 1), ("frame_kf", 1), ("base", 1),
                                     ("list_status", 1)), f)
    ur = t.get("kp_ur")
    if ur is not None and (not ur.is_contiguous() or ur.numel() < f * kp_cap):
        raise SlamitError("fuse_list_batch_dev: kp_ur holds one float per keypoint")
    rec = FuseListBatchRec(f, n_maps, kp_cap, q_cap, cap, 0, t["m"].data_ptr(), t["match_kp"].data_ptr(), t["query_point"].data_ptr(), t["kps_un"].data_ptr(),
                           ur.data_ptr() if ur is not None else None, t["frame_map"].data_ptr(), t["frame_kf"].data_ptr(), t["base"].data_ptr(),
                           t["ops"].data_ptr(), t["n"].data_ptr(), t["list_status"].data_ptr())
    _check(lib().slamit_fuse_list_batch_dev(device, C.byref(rec), stream), "slamit_fuse_list_batch_dev")


def check_replaced(mp_replaced, frame_mp, device=0):
    """Tracking::CheckReplacedInLastFrame (Tracking.cc:959-974): every entry p >= 0 of a frame's point list with mp_replaced[p] >= 0
    becomes mp_replaced[p], one hop.  -> (the list, status).  The caller's arrays are not modified."""
    rep = np.ascontiguousarray(mp_replaced, np.int32).reshape(-1)
    lst = np.array(frame_mp, np.int32).reshape(-1)
    st = np.zeros(1, np.int32)
    _check(lib().slamit_check_replaced(device, len(rep), _np_ptr(rep) if len(rep) else None, len(lst), _np_ptr(lst) if len(lst) else None, _np_ptr(st)),
           "slamit_check_replaced")
    return lst, int(st[0])


def check_replaced_batch_dev(replaced, t, n_mp=None, device=0, stream=None):
    """The same for a batch of frames, resident.  replaced: one mp_replaced tensor per map (ReplaceIndex.t["mp_replaced"]); n_mp: the
    maps' point counts (default: the tensors' lengths); t: dict of torch CUDA tensors frame_map (F) i32, n (F) i32, frame_mp (F, cap) i32
    in / out, status (F) i32.  Asynchronous on `stream`."""
    f, cap = t["frame_mp"].shape
    _rows(t, "check_replaced_batch_dev", (("frame_mp", cap), ("frame_map", 1), ("n", 1), ("status", 1)), f)
    nm = len(replaced)
    counts = (C.c_int32 * max(nm, 1))(*[int(r.numel()) if n_mp is None else int(n_mp[i]) for i, r in enumerate(replaced)])
    ptrs = (C.c_void_p * max(nm, 1))(*[r.data_ptr() for r in replaced])
    rec = CheckReplacedBatchRec(f, nm, cap, 0, counts, ptrs, t["frame_map"].data_ptr(), t["n"].data_ptr(), t["frame_mp"].data_ptr(), t["status"].data_ptr())
    _check(lib().slamit_check_replaced_batch_dev(device, C.byref(rec), stream), "slamit_check_replaced_batch_dev")


def kf_op_records(ops):
    """Ops as an array of slamit_kf_op: a KF_OP_DTYPE array as it is, else rows (kind, kf) or (kind, kf, parent)."""
    if isinstance(ops, np.ndarray) and ops.dtype == KF_OP_DTYPE:
        return np.ascontiguousarray(ops).reshape(-1)
    rows = list(ops)
    out = np.zeros(len(rows), KF_OP_DTYPE)
    for i, r in enumerate(rows):
        r = tuple(int(v) for v in r)
        out[i] = (r + (-1,))[:3] + (0,)
    return out


def kf_erase(tables, tree, ops, child_cap_out=None, edit_cap=None, fill=None, device=0):
    """KeyFrame::SetBadFlag's graph rows and spanning tree (KeyFrame.cc:460-552, with EraseConnection and ChangeParent) for a list of
    keyframe ops applied as if sequentially, over a map's tables (slamit_map_index: n_kf, n_mp, kf_mp_ptr, kf_mp, kf_child_ptr, kf_child,
    kf_bad, kf_parent) and the arrays beside them (dict: row_cap, origin_kf, kf_not_erase, kf_to_be_erased, cw_kf / cw_w (n_kf, row_cap),
    cw_n, ord_kf / ord_w, ord_n, optionally kf_best (n_kf, 10); kf_bad / kf_parent where they are not taken from `tables`).  ops:
    kf_op_records().  The caller's arrays are not modified.  child_cap_out: the room of the new children table (default: the old table
    plus one entry per op and per child of a SET_BAD keyframe); edit_cap: the room of the emitted list (default: k's keypoints summed over the
    SET_BAD ops).  fill: optional dict of prefilled outputs (child_ptr_out, child_out, op_status, edits), copied.  -> dict:
    kf_child_ptr, kf_child, kf_bad, kf_parent (what MapIndex / _map_index_host take in place of the old ones), kf_to_be_erased, the
    seven graph arrays, op_status, edits (EDIT_DTYPE, the first n_edits_out of them), n_edits_out, n_child_out, status, and `raw`: the
    output arrays in full.  With a bit of KF_ERASE_REFUSED in status the tables returned are the old ones."""
    rec, keep = _map_index_host(tables)
    n_kf = max(rec.n_kf, 0)
    ed = kf_op_records(ops)
    src = dict(tree)
    for key in ("kf_bad", "kf_parent"):
        src.setdefault(key, tables.get(key))
    cptr = np.asarray(tables["kf_child_ptr"], np.int64).reshape(-1) if tables.get("kf_child_ptr") is not None else np.zeros(1, np.int64)
    kptr = np.asarray(tables["kf_mp_ptr"], np.int64).reshape(-1) if tables.get("kf_mp_ptr") is not None else np.zeros(1, np.int64)
    inside = [int(k) for k in ed["kf"][ed["kind"] == KF_ERASE_SET_BAD] if 0 <= k < len(cptr) - 1]
    if child_cap_out is None:
        child_cap_out = int(cptr[-1]) + len(ed) + sum(int(cptr[k + 1] - cptr[k]) for k in inside)
    if edit_cap is None:
        edit_cap = sum(int(kptr[k + 1] - kptr[k]) for k in inside if k < len(kptr) - 1)
    child_cap_out, edit_cap = int(child_cap_out), int(edit_cap)
    fill = fill or {}
    xrec, xkeep = TreeIndexRec(int(tree["row_cap"]), int(tree["origin_kf"])), {}
    if src.get("kf_not_erase") is not None:
        xkeep["kf_not_erase"] = np.ascontiguousarray(src["kf_not_erase"], np.uint8).reshape(-1)
        xrec.kf_not_erase = xkeep["kf_not_erase"].ctypes.data
    for key, dt in TREE_INDEX_INPLACE:
        if src.get(key) is not None:
            xkeep[key] = np.array(src[key], dt).reshape(-1)
            setattr(xrec, key, xkeep[key].ctypes.data)
    for key, count in (("child_ptr_out", n_kf + 1), ("child_out", max(child_cap_out, 0))):
        xkeep[key] = np.zeros(count, np.int32) if fill.get(key) is None else np.array(fill[key], np.int32).reshape(-1)
        if len(xkeep[key]) != count:
            raise SlamitError("kf_erase: fill[%s] does not hold %d entries" % (key, count))
        setattr(xrec, key, xkeep[key].ctypes.data if count else None)
    xrec.child_cap_out = child_cap_out
    ost = np.zeros(len(ed), np.int32) if fill.get("op_status") is None else np.array(fill["op_status"], np.int32).reshape(-1)
    edits = np.zeros(max(edit_cap, 0), EDIT_DTYPE) if fill.get("edits") is None else np.array(fill["edits"], EDIT_DTYPE).reshape(-1)
    if len(ost) != len(ed) or len(edits) != max(edit_cap, 0):
        raise SlamitError("kf_erase: op_status holds one entry per op, edits edit_cap entries")
    ne, nc, st = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    some = lambda a: _np_ptr(a) if len(a) else None
    _check(lib().slamit_kf_erase_apply(device, C.byref(rec), C.byref(xrec), len(ed), some(ed), some(ost), edit_cap, some(edits), _np_ptr(ne), _np_ptr(nc),
                                       _np_ptr(st)), "slamit_kf_erase_apply")
    del keep
    status, n_edits, need = int(st[0]), int(ne[0]), int(nc[0])
    out = {"status": status, "n_edits_out": n_edits, "n_child_out": need, "op_status": ost, "raw": dict(xkeep, op_status=ost, edits=edits)}
    if status & KF_ERASE_REFUSED:
        out.update(kf_child_ptr=np.array(tables["kf_child_ptr"], np.int32).reshape(-1), kf_child=np.array(tables["kf_child"], np.int32).reshape(-1), edits=edits[:0])
    else:
        out.update(kf_child_ptr=xkeep["child_ptr_out"], kf_child=xkeep["child_out"][:need], edits=edits[:n_edits])
    for key, _ in TREE_INDEX_INPLACE:
        out[key] = xkeep[key].reshape(np.shape(src[key])) if key in xkeep else None
    return out


class TreeIndex:
    """The arrays kf_erase_batch_dev reads and writes beside a MapIndex (the resident form's slamit_tree_index), with TWO buffer sets for
    the children table.  TreeIndex(tree, map_index, covis, child_cap): kf_bad and kf_parent ARE map_index's tensors and the seven graph
    arrays (kf_best included, where the CovisIndex has one) the CovisIndex's, all rewritten in place; kf_not_erase is the CovisIndex's
    column; kf_to_be_erased is uploaded from tree (default: zeros) and kept in .t.  child_cap: entries each buffer set of the table holds.
    .rec reads the current set and writes the other; after kf_erase_batch_dev has run without a bit of KF_ERASE_REFUSED, swap() makes the
    written set the current one in map_index.rec, so every reader takes the new table unchanged."""

    def __init__(self, tree, map_index, covis, child_cap):
        import torch

        tree = tree or {}
        self.map_index, self.covis, self.device, self.child_cap = map_index, covis, map_index.device, int(child_cap)
        dev = "cuda:%d" % self.device
        n_kf = max(map_index.n_kf, 0)
        room = lambda t: torch.cat([t, torch.zeros(max(self.child_cap, 1) - t.numel(), dtype=t.dtype, device=dev)]) if t.numel() < max(self.child_cap, 1) else t
        cur = {"kf_child_ptr": map_index.t["kf_child_ptr"], "kf_child": room(map_index.t["kf_child"])}
        self.sets = [cur, {k: torch.zeros_like(v) for k, v in cur.items()}]
        tbe = np.ascontiguousarray(tree["kf_to_be_erased"], np.uint8).reshape(-1) if tree.get("kf_to_be_erased") is not None else np.zeros(max(n_kf, 1), np.uint8)
        self.t = {"kf_to_be_erased": torch.from_numpy(tbe if len(tbe) else np.zeros(1, np.uint8)).to(dev)}
        self.rec = TreeIndexRec(covis.row_cap, int(covis.rec.origin_kf))
        self._point()

    def _point(self):
        cur, nxt = self.sets
        mi, ci = self.map_index, self.covis
        mi.t["kf_child_ptr"], mi.t["kf_child"] = cur["kf_child_ptr"], cur["kf_child"]
        mi.rec.kf_child_ptr, mi.rec.kf_child = cur["kf_child_ptr"].data_ptr(), cur["kf_child"].data_ptr()
        self.rec.kf_not_erase = ci.t["kf_not_erase"].data_ptr()
        self.rec.kf_bad, self.rec.kf_parent = mi.t["kf_bad"].data_ptr(), mi.t["kf_parent"].data_ptr()
        self.rec.kf_to_be_erased = self.t["kf_to_be_erased"].data_ptr()
        for key in COVIS_GRAPH:
            setattr(self.rec, key, ci.t[key].data_ptr() if key in ci.t else None)
        self.rec.child_ptr_out, self.rec.child_out, self.rec.child_cap_out = nxt["kf_child_ptr"].data_ptr(), nxt["kf_child"].data_ptr(), self.child_cap

    def swap(self):
        """The children table the last call wrote becomes the one every record reads; no copy, no synchronisation."""
        self.sets.reverse()
        self._point()


def kf_erase_workspace(n_maps, cap, kf_cap, row_cap, child_cap):
    return int(lib().slamit_kf_erase_workspace(n_maps, cap, kf_cap, row_cap, child_cap))


def kf_erase_batch_dev(maps, tree, t, device=0, stream=None):
    """One op list per map, resident.  maps / tree: lists of MapIndex / TreeIndex; t: dict of torch CUDA tensors ops (B, cap, 16) u8 (the
    bytes of KF_OP_DTYPE records; an int32 tensor (B, cap, 4) is the same memory), n (B) i32, op_status (B, cap) i32 in / out, edits (B,
    edit_cap, 24) u8 in / out (what map_edit_batch_dev takes as its edits, with n_edits_out as its n), n_edits_out (B), n_child_out (B),
    status (B) i32, workspace: uint8, kf_erase_workspace(B, cap, kf_cap, row_cap, child_cap) bytes with kf_cap = t["kf_cap"] >= every
    n_kf, row_cap = t["row_cap"] >= every map's, child_cap = t["child_cap"] >= every map's children entries.  The new children tables are
    written into each TreeIndex's other buffer set: where status has no bit of KF_ERASE_REFUSED, call swap() on the TreeIndex before the
    next reader is ENQUEUED.  Asynchronous on `stream`."""
    b, cap = t["ops"].shape[0], t["ops"].shape[1]
    edit_cap = t["edits"].shape[1]
    if len(maps) != b or len(tree) != b:
        raise SlamitError("kf_erase_batch_dev: one MapIndex, one TreeIndex and one list per map")
    _rows(t, "kf_erase_batch_dev", (("op_status", cap), ("n", 1), ("n_edits_out", 1), ("n_child_out", 1), ("status", 1)), b)
    for key, per in (("ops", cap * KF_OP_DTYPE.itemsize), ("edits", edit_cap * EDIT_DTYPE.itemsize)):
        if t[key].numel() * t[key].element_size() != b * per or not t[key].is_contiguous():
            raise SlamitError("kf_erase_batch_dev: %s is not a contiguous array of %d bytes per map" % (key, per))
    M, X = (MapIndexRec * max(b, 1))(), (TreeIndexRec * max(b, 1))()
    for i, (mi, ti) in enumerate(zip(maps, tree)):
        M[i], X[i] = mi.rec, ti.rec
    ws = t["workspace"]
    rec = KfEraseBatchRec(b, cap, int(t["kf_cap"]), int(t["row_cap"]), int(t["child_cap"]), edit_cap, M, X, t["ops"].data_ptr(), t["n"].data_ptr(),
                          t["op_status"].data_ptr(), t["edits"].data_ptr(), t["n_edits_out"].data_ptr(), t["n_child_out"].data_ptr(), t["status"].data_ptr(),
                          ws.data_ptr(), ws.numel() * ws.element_size())
    _check(lib().slamit_kf_erase_batch_dev(device, C.byref(rec), stream), "slamit_kf_erase_batch_dev")


# ---- map growth: new keyframes, new map points, ProcessNewKeyFrame's association loop -----------------------------------------------
def grow_op_records(ops):
    """A list of dicts (the fields of GROW_OP_DTYPE; those left out are 0, kf_b and cand -1) as slamit_grow_op records."""
    out = np.zeros(len(ops), GROW_OP_DTYPE)
    out["kf_b"], out["cand"] = -1, -1
    for i, e in enumerate(ops):
        for k, v in e.items():
            out[i][k] = v
    return out


def grow_index_rec(tensors, kf_cap, mp_cap, kfmp_cap):
    """slamit_grow_index over a dict of torch CUDA tensors under the names of GROW_INDEX_ARRAYS, each with room for kf_cap keyframes,
    mp_cap points and kfmp_cap keypoints (kf_depth and kf_th_depth may be left out together).  The tensors are the memory the other
    records of the map point to; the caller keeps them alive."""
    rec = GrowIndexRec(int(kf_cap), int(mp_cap), int(kfmp_cap), 0)
    room = {"kf_mp_ptr": kf_cap + 1, "kf_child_ptr": kf_cap + 1, "obs_ptr": mp_cap + 1, "kf_mp": kfmp_cap, "kf_octave": kfmp_cap, "kf_desc": 32 * kfmp_cap,
            "kf_depth": kfmp_cap, "kf_best": LOCAL_MAP_BEST * kf_cap, "kf_center": 3 * kf_cap, "mp_pos": 3 * mp_cap, "mp_normal": 3 * mp_cap, "mp_desc": 32 * mp_cap}
    for key, dt in GROW_INDEX_ARRAYS:
        t = tensors.get(key)
        if t is None:
            if key in ("kf_depth", "kf_th_depth"):
                continue
            raise SlamitError("grow_index_rec: no %s" % key)
        need = room.get(key, kf_cap if key.startswith(("kf_", "cw_", "ord_")) else mp_cap)
        if not t.is_cuda or not t.is_contiguous() or t.element_size() != np.dtype(dt).itemsize or t.numel() < need:
            raise SlamitError("grow_index_rec: %s is not a contiguous CUDA tensor of at least %d %s" % (key, need, np.dtype(dt).name))
        setattr(rec, key, t.data_ptr())
    return rec


def grow_frame_rec(frame):
    """slamit_grow_frame over a dict of torch CUDA tensors frame_mp (n_kp) i32, octave (n_kp) u8, desc (n_kp, 32) u8, Tcw (12) f32 and
    optionally depth, uright (n_kp) f32, with th_depth a float.  The caller keeps the tensors alive."""
    n_kp = int(frame["frame_mp"].numel())
    rec = GrowFrameRec(n_kp, float(frame.get("th_depth", 0.0)))
    for key, per in (("frame_mp", 1), ("octave", 1), ("desc", 32), ("depth", 1), ("uright", 1)):
        t = frame.get(key)
        if t is None:
            if key in ("depth", "uright"):
                continue
            raise SlamitError("grow_frame_rec: no %s" % key)
        if t.numel() != n_kp * per or not t.is_contiguous():
            raise SlamitError("grow_frame_rec: %s does not hold %d entries per keypoint" % (key, per))
        setattr(rec, key, t.data_ptr())
    if frame["Tcw"].numel() != 12:
        raise SlamitError("grow_frame_rec: Tcw holds 12 floats")
    rec.Tcw = frame["Tcw"].data_ptr()
    return rec


def map_grow(tables, cols, ops, frames, cands=None, recent=(), caps=None, fill=None, device=0):
    """New keyframes, new map points and ProcessNewKeyFrame's association loop for a list of ops applied as if sequentially, over a map's
    tables and column records, host form (for parity and tests: it stages every table both ways).  tables / cols: dicts that together hold
    n_kf, n_mp, obs_kf and the arrays of GROW_INDEX_ARRAYS (the dicts MapIndex, CovisIndex, PointIndex, EditIndex, ReplaceIndex and
    TreeIndex take; kf_depth and kf_th_depth may be None together).  ops: grow_op_records().  frames: a list of dicts frame_mp, octave, desc,
    Tcw, th_depth and optionally depth, uright (numpy).  cands: dict status (u8), x3d (n, 3) f32, or None.  recent: the recent list so far.
    caps: dict kf_cap, mp_cap, kfmp_cap, edit_cap, recent_cap (default: what the gate needs).  fill: optional dict of prefilled arrays, each
    at its capacity, under the names of GROW_INDEX_ARRAYS, op_status, edits (bytes) and recent: what lies past the tables and the counts.
    The caller's arrays are not modified.  -> dict: the grown arrays under their names, cut to n_kf / n_mp as they now stand (what the index
    classes take in place of the old ones), n_kf, n_mp, op_status, edits (the first n_edits_out, EDIT_DTYPE), recent (the first n_recent),
    n_new, need, status, and raw: every array in full."""
    ops = np.ascontiguousarray(ops, GROW_OP_DTYPE).reshape(-1)
    src = dict(tables)
    src.update(cols or {})
    n_kf, n_mp = int(src["n_kf"]), int(src["n_mp"])
    n_new_kf, P = int((ops["kind"] == GROW_NEW_KF).sum()), int((ops["kind"] == GROW_NEW_POINT).sum())
    kp = lambda kind: sum(len(frames[s]["frame_mp"]) for s in ops["src"][ops["kind"] == kind] if 0 <= s < len(frames))
    end = int(np.asarray(src["kf_mp_ptr"]).reshape(-1)[n_kf]) if src.get("kf_mp_ptr") is not None and len(np.asarray(src["kf_mp_ptr"]).reshape(-1)) > n_kf else 0
    c = {"kf_cap": n_kf + n_new_kf, "mp_cap": n_mp + P, "kfmp_cap": end + kp(GROW_NEW_KF), "edit_cap": 2 * P + kp(GROW_ASSOCIATE),
         "recent_cap": len(recent) + int(((ops["kind"] == GROW_NEW_POINT) & (ops["flags"] & GROW_RECENT != 0)).sum()) + kp(GROW_ASSOCIATE)}
    c.update(caps or {})
    fill = fill or {}
    room = {"kf_mp_ptr": c["kf_cap"] + 1, "kf_child_ptr": c["kf_cap"] + 1, "obs_ptr": c["mp_cap"] + 1, "kf_mp": c["kfmp_cap"], "kf_octave": c["kfmp_cap"],
            "kf_desc": 32 * c["kfmp_cap"], "kf_depth": c["kfmp_cap"], "kf_best": LOCAL_MAP_BEST * c["kf_cap"], "kf_center": 3 * c["kf_cap"], "mp_pos": 3 * c["mp_cap"],
            "mp_normal": 3 * c["mp_cap"], "mp_desc": 32 * c["mp_cap"]}

    def held(key, dt, count, front):
        a = np.array(fill[key], dt).reshape(-1) if fill.get(key) is not None else np.zeros(max(count, 0), dt)
        if len(a) != count:
            raise SlamitError("map_grow: fill[%s] does not hold %d entries" % (key, count))
        if front is not None:
            f = np.ascontiguousarray(front, dt).reshape(-1)
            if len(f) > count:
                raise SlamitError("map_grow: %s holds more than its capacity" % key)
            a[:len(f)] = f
        return a

    raw, rec = {}, GrowIndexRec(c["kf_cap"], c["mp_cap"], c["kfmp_cap"], 0)
    for key, dt in GROW_INDEX_ARRAYS:
        if src.get(key) is None:
            continue
        raw[key] = held(key, dt, room.get(key, c["kf_cap"] if key.startswith(("kf_", "cw_", "ord_")) else c["mp_cap"]), src[key])
        setattr(rec, key, _np_ptr(raw[key]))
    obs_kf = np.ascontiguousarray(src["obs_kf"], np.int32).reshape(-1) if src.get("obs_kf") is not None else np.zeros(0, np.int32)
    mrec = MapIndexRec(n_kf, n_mp)
    mrec.obs_kf = _np_ptr(obs_kf) if len(obs_kf) else None
    F, keep = (GrowFrameRec * max(len(frames), 1))(), []
    for i, f in enumerate(frames):
        n_kp = len(f["frame_mp"])
        F[i].n_kp, F[i].th_depth = n_kp, float(f.get("th_depth", 0.0))
        for key, dt, per in (("frame_mp", np.int32, 1), ("octave", np.uint8, 1), ("desc", np.uint8, 32), ("depth", np.float32, 1), ("uright", np.float32, 1), ("Tcw", np.float32, 0)):
            if f.get(key) is None:
                continue
            a = np.ascontiguousarray(f[key], dt).reshape(-1)
            if len(a) != (n_kp * per if per else 12):
                raise SlamitError("map_grow: a frame's %s does not hold its entries" % key)
            keep.append(a if len(a) else np.zeros(1, dt))
            setattr(F[i], key, _np_ptr(keep[-1]))
    cs = np.ascontiguousarray(cands["status"], np.uint8).reshape(-1) if cands else np.zeros(0, np.uint8)
    cx = np.ascontiguousarray(cands["x3d"], np.float32).reshape(-1) if cands else np.zeros(0, np.float32)
    if len(cx) != 3 * len(cs):
        raise SlamitError("map_grow: cands x3d holds three floats per status")
    ost = held("op_status", np.int32, len(ops), None)
    edits = held("edits", np.uint8, c["edit_cap"] * EDIT_DTYPE.itemsize, None)
    rct = held("recent", np.int32, c["recent_cap"], np.asarray(recent, np.int32) if len(recent) <= c["recent_cap"] else None)
    ne, nn = np.array([int(fill.get("n_edits_out", 0))], np.int32), np.array([int(fill.get("n_new", 0))], np.int32)   # left as they are by a refused call
    nr, need, st = np.array([len(recent)], np.int32), np.zeros(GROW_NEEDS, np.int32), np.zeros(1, np.int32)
    some = lambda a: _np_ptr(a) if len(a) else None
    _check(lib().slamit_map_grow_apply(device, C.byref(mrec), C.byref(rec), len(frames), F, len(ops), some(ops), len(cs), some(cs), some(cx), some(ost), c["edit_cap"],
                                       some(edits), _np_ptr(ne), c["recent_cap"], some(rct), _np_ptr(nr), _np_ptr(nn), _np_ptr(need), _np_ptr(st)), "slamit_map_grow_apply")
    out = {"raw": dict(raw, op_status=ost, edits=edits, recent=rct), "status": int(st[0]), "need": need.tolist(), "n_new": int(nn[0]), "n_edits_out": int(ne[0]),
           "n_recent": int(nr[0]), "op_status": ost, "caps": c}
    grown = not out["status"] & GROW_REFUSED
    out["n_kf"], out["n_mp"] = n_kf + (n_new_kf if grown else 0), n_mp + (P if grown else 0)
    cut = {"kf_mp_ptr": out["n_kf"] + 1, "kf_child_ptr": out["n_kf"] + 1, "obs_ptr": out["n_mp"] + 1, "kf_best": LOCAL_MAP_BEST * out["n_kf"], "kf_center": 3 * out["n_kf"],
           "mp_pos": 3 * out["n_mp"], "mp_normal": 3 * out["n_mp"], "mp_desc": 32 * out["n_mp"]}
    n_kfmp = int(raw["kf_mp_ptr"][out["n_kf"]])
    for key, _ in GROW_INDEX_ARRAYS:
        if key in raw:
            k = cut.get(key, n_kfmp * (32 if key == "kf_desc" else 1) if key in ("kf_mp", "kf_octave", "kf_desc", "kf_depth") else
                        out["n_kf"] if key.startswith(("kf_", "cw_", "ord_")) else out["n_mp"])
            out[key] = raw[key][:k]
    out["edits"] = edits[:out["n_edits_out"] * EDIT_DTYPE.itemsize].view(EDIT_DTYPE) if grown else edits[:0].view(EDIT_DTYPE)
    out["recent"] = rct[:out["n_recent"]]
    return out


class GrowIndex:
    """The index classes of one map re-housed in buffers with room, and the record map_grow_batch_dev takes (the resident form's
    slamit_grow_index).  GrowIndex(map_index, covis=, points=, edit=, replace=, tree=, kf_cap=, mp_cap=, kfmp_cap=): every tensor the
    records share that grows with the keyframes, the points or the keypoints -- the MapIndex's tables, the CovisIndex's columns and graph
    rows, the PointIndex's columns, the in-place tensors of the EditIndex / ReplaceIndex / TreeIndex and the pointer arrays of BOTH buffer
    sets of the EditIndex and the TreeIndex -- is copied once into a tensor that holds kf_cap keyframes, mp_cap points or kfmp_cap keypoints
    (zeros behind what it held), a tensor two records shared stays one tensor, and all records are repointed.  covis, points, edit (built
    with that covis and those points) and tree are required: between them they hold every array a new keyframe or point needs; without
    replace, mp_replaced is kept here.  The PointIndex's kf_octave becomes the CovisIndex's tensor.  The observation and children tables
    keep the room their EditIndex / TreeIndex were given.  .rec is built from the tensors as they stand (after any swap()).  After
    map_grow_batch_dev has run without a bit of GROW_REFUSED, grown(n_new_kf, n_point_ops) advances n_kf / n_mp of the map record, the one
    every sibling call reads them from: host bookkeeping with what the caller listed, no synchronisation."""

    def __init__(self, map_index, covis=None, points=None, edit=None, replace=None, tree=None, kf_cap=0, mp_cap=0, kfmp_cap=0):
        import torch

        if covis is None or points is None or edit is None or tree is None:
            raise SlamitError("GrowIndex: covis, points, edit and tree hold arrays a new keyframe or point needs: all four are required")
        if edit.covis is not covis or edit.points is not points or edit.map_index is not map_index or tree.map_index is not map_index or tree.covis is not covis:
            raise SlamitError("GrowIndex: the EditIndex and the TreeIndex must have been built over this MapIndex, CovisIndex and PointIndex")
        mi = map_index
        self.map_index, self.covis, self.points, self.edit, self.replace, self.tree = mi, covis, points, edit, replace, tree
        self.kf_cap, self.mp_cap, self.kfmp_cap, self.device = int(kf_cap), int(mp_cap), int(kfmp_cap), mi.device
        n_kfmp = int(mi.t["kf_mp_ptr"][mi.rec.n_kf]) if mi.rec.n_kf else 0     # read once, when the index is set up
        if self.kf_cap < mi.rec.n_kf or self.mp_cap < mi.rec.n_mp or self.kfmp_cap < n_kfmp:
            raise SlamitError("GrowIndex: a capacity below what the map holds")
        rc, K, P, E = covis.row_cap, self.kf_cap, self.mp_cap, self.kfmp_cap
        points.t["kf_octave"] = covis.t["kf_octave"]
        self.t = {} if replace is not None else {"mp_replaced": torch.full((max(mi.rec.n_mp, 1),), -1, dtype=torch.int32, device="cuda:%d" % self.device)}
        rooms = [(mi.t, {"kf_bad": K, "kf_parent": K, "kf_best": LOCAL_MAP_BEST * K, "kf_mp_ptr": K + 1, "kf_mp": E, "mp_bad": P, "mp_pos": 3 * P, "mp_normal": 3 * P,
                         "mp_max_dist": P, "mp_min_dist": P}),
                 (covis.t, {"kf_octave": E, "kf_depth": E, "kf_th_depth": K, "kf_not_erase": K, "cw_kf": K * rc, "cw_w": K * rc, "cw_n": K, "ord_kf": K * rc, "ord_w": K * rc,
                            "ord_n": K, "kf_best": LOCAL_MAP_BEST * K, "mp_nobs": P}),
                 (points.t, {"kf_octave": E, "kf_center": 3 * K, "kf_desc": 32 * E, "mp_ref_kf": P, "mp_nobs": P, "mp_found": P, "mp_visible": P, "mp_first_kf": P,
                             "mp_normal": 3 * P, "mp_max_dist": P, "mp_min_dist": P, "mp_desc": 32 * P}),
                 (edit.t, {"mp_bad": P, "mp_nobs": P, "mp_ref_kf": P, "kf_mp": E}), (edit.sets[0], {"obs_ptr": P + 1}), (edit.sets[1], {"obs_ptr": P + 1}),
                 (tree.t, {"kf_to_be_erased": K}), (tree.sets[0], {"kf_child_ptr": K + 1}), (tree.sets[1], {"kf_child_ptr": K + 1}), (self.t, {"mp_replaced": P})]
        if replace is not None:
            rooms.append((replace.t, {"mp_found": P, "mp_visible": P, "mp_replaced": P}))
        housed = {}                                                      # the old tensor's address -> its new house: what two records shared stays one tensor

        def house(t, count):
            key = (t.data_ptr(), t.dtype)
            if key not in housed:
                new = torch.zeros(max(count, 1), dtype=t.dtype, device=t.device)   # a table longer than its room is an empty one's padding
                new[:min(t.numel(), count)] = t.reshape(-1)[:count]
                housed[key] = new
            if housed[key].numel() < count:
                raise SlamitError("GrowIndex: one tensor is named with two different rooms")
            return housed[key]

        for d, room in rooms:
            for key, count in room.items():
                if key in d:
                    d[key] = house(d[key], count)
        for idx, tables in ((mi, MAP_INDEX_TABLES), (covis, COVIS_INDEX_TABLES), (points, POINT_INDEX_TABLES)):
            for key, _ in tables:
                if key in idx.t:
                    setattr(idx.rec, key, idx.t[key].data_ptr())
        edit._point()                                                    # its followers (a ReplaceIndex) repoint with it
        if replace is not None:
            replace._point()
        tree._point()

    @property
    def rec(self):
        mi, ci, pi = self.map_index.t, self.covis.t, self.points.t
        t = {k: mi[k] for k in ("kf_mp_ptr", "kf_mp", "kf_bad", "kf_parent", "kf_best", "kf_child_ptr", "mp_pos", "mp_normal", "mp_max_dist", "mp_min_dist", "mp_bad", "obs_ptr")}
        t.update({k: ci[k] for k in ("kf_octave", "kf_depth", "kf_th_depth", "kf_not_erase", "cw_n", "ord_n", "mp_nobs") if k in ci})
        t.update({k: pi[k] for k in ("kf_desc", "kf_center", "mp_ref_kf", "mp_found", "mp_visible", "mp_first_kf", "mp_desc")})
        t["kf_to_be_erased"] = self.tree.t["kf_to_be_erased"]
        t["mp_replaced"] = (self.replace.t if self.replace is not None else self.t)["mp_replaced"]
        return grow_index_rec(t, self.kf_cap, self.mp_cap, self.kfmp_cap)

    def grown(self, n_new_kf, n_point_ops):
        mi = self.map_index
        mi.n_kf, mi.n_mp = mi.n_kf + int(n_new_kf), mi.n_mp + int(n_point_ops)
        if mi.n_kf > self.kf_cap or mi.n_mp > self.mp_cap:
            raise SlamitError("GrowIndex.grown: past the capacity")
        mi.rec.n_kf, mi.rec.n_mp = mi.n_kf, mi.n_mp


def map_grow_workspace(n_maps, mp_cap):
    return int(lib().slamit_map_grow_workspace(n_maps, mp_cap))


def map_grow_batch_dev(map_recs, grow_recs, frame_recs, t, device=0, stream=None):
    """One op list per map, resident: new keyframes, new points and the association loop appended to tables with room.  map_recs: a list of
    MapIndex (any object with .rec, as the sibling calls take) or of bare MapIndexRec; grow_recs: a list of GrowIndexRec (grow_index_rec); frame_recs: a list of GrowFrameRec
    (grow_frame_rec), at most GROW_MAX_FRAMES.  t: dict of torch CUDA tensors ops (B, cap, 56) u8 (the bytes of GROW_OP_DTYPE records), n (B)
    i32, cand_status (B, cand_cap) u8, cand_x3d (B, cand_cap, 3) f32, op_status (B, cap) i32 in / out, edits (B, edit_cap, 24) u8 in / out
    (what map_edit_batch_dev takes as its edits, with n_edits_out as its n), n_edits_out (B) i32, recent (B, recent_cap) i32 and n_recent (B)
    i32 in / out (what map_point_culling_batch_dev takes), n_new (B) i32, need (B, GROW_NEEDS) i32, status (B) i32, workspace: uint8,
    map_grow_workspace(B, mp_cap) bytes with mp_cap = t["mp_cap"] >= every grow record's mp_cap.  Where status has no bit of
    GROW_REFUSED the caller advances n_kf / n_mp of its records by the NEW_KF ops and by the NEW_POINT ops it listed.  Asynchronous on
    `stream`."""
    b, cap = t["ops"].shape[0], t["ops"].shape[1]
    edit_cap, recent_cap, cand_cap = t["edits"].shape[1], t["recent"].shape[1], t["cand_status"].shape[1]
    if len(map_recs) != b or len(grow_recs) != b:
        raise SlamitError("map_grow_batch_dev: one MapIndexRec, one GrowIndexRec and one list per map")
    _rows(t, "map_grow_batch_dev", (("op_status", cap), ("n", 1), ("n_edits_out", 1), ("recent", recent_cap), ("n_recent", 1), ("n_new", 1), ("need", GROW_NEEDS),
                                    ("status", 1), ("cand_status", cand_cap), ("cand_x3d", 3 * cand_cap)), b)
    for key, per in (("ops", cap * GROW_OP_DTYPE.itemsize), ("edits", edit_cap * EDIT_DTYPE.itemsize)):
        if t[key].numel() * t[key].element_size() != b * per or not t[key].is_contiguous():
            raise SlamitError("map_grow_batch_dev: %s is not a contiguous array of %d bytes per map" % (key, per))
    M, X, F = (MapIndexRec * max(b, 1))(), (GrowIndexRec * max(b, 1))(), (GrowFrameRec * max(len(frame_recs), 1))()
    for i, (mr, gr) in enumerate(zip(map_recs, grow_recs)):
        M[i], X[i] = getattr(mr, "rec", mr), getattr(gr, "rec", gr)     # MapIndex and its like, as the sibling calls take them, or the bare records
    for i, fr in enumerate(frame_recs):
        F[i] = fr
    ws = t["workspace"]
    rec = MapGrowBatchRec(b, cap, len(frame_recs), cand_cap, edit_cap, recent_cap, int(t["mp_cap"]), 0, M, X, F, t["ops"].data_ptr(), t["n"].data_ptr(),
                          t["cand_status"].data_ptr(), t["cand_x3d"].data_ptr(), t["op_status"].data_ptr(), t["edits"].data_ptr(), t["n_edits_out"].data_ptr(),
                          t["recent"].data_ptr(), t["n_recent"].data_ptr(), t["n_new"].data_ptr(), t["need"].data_ptr(), t["status"].data_ptr(),
                          ws.data_ptr(), ws.numel() * ws.element_size())
    _check(lib().slamit_map_grow_batch_dev(device, C.byref(rec), stream), "slamit_map_grow_batch_dev")


# ---- essential-graph optimisation (Optimizer::OptimizeEssentialGraph) -----------------------------------------------------------
_EG_GRAPH_ARRAYS = (("kf_bad", np.uint8), ("kf_id", np.int32), ("kf_parent", np.int32), ("child_ptr", np.int32), ("child_kf", np.int32),
                    ("loop_ptr", np.int32), ("loop_kf_list", np.int32), ("ord_kf", np.int32), ("ord_w", np.int32), ("ord_n", np.int32),
                    ("conn_ptr", np.int32), ("conn_kf", np.int32))
_EG_PROBLEM_ARRAYS = (("scw_r", np.float64), ("scw_t", np.float64), ("scw_s", np.float64), ("snc_r", np.float64), ("snc_t", np.float64),
                      ("snc_s", np.float64), ("fixed", np.uint8), ("bad", np.uint8), ("edge_v0", np.int32), ("edge_v1", np.int32),
                      ("edge_kind", np.int32), ("inc_ptr", np.int32), ("inc_edge", np.int32), ("pt_pos", np.float32), ("pt_ref", np.int32),
                      ("pt_bad", np.uint8))


def essential_plan(graph, edge_cap=None):
    """The edge list of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:847-983) from slot-numbered tables: `graph` holds the
    fields of slamit_eg_graph (synth.synth_essential makes one).  Host only.  Returns edge_v0, edge_v1, edge_kind in the reference's
    insertion order and inc_ptr, inc_edge, the incidence lists slamit_essential_graph_dev needs."""
    n = int(graph["n_kf"])
    keep = {k: np.ascontiguousarray(graph[k], dt) for k, dt in _EG_GRAPH_ARRAYS}
    g = EgGraph(n, int(graph["row_cap"]), int(graph["loop_kf"]), int(graph["cur_kf"]), int(graph.get("min_feat", 100)), 0,
                *[_np_ptr(keep[k]) if keep[k].size else None for k, _ in _EG_GRAPH_ARRAYS])
    if edge_cap is None:
        edge_cap = int(keep["conn_kf"].size + keep["loop_kf_list"].size + keep["ord_n"].sum() + n)
    v0, v1, kind = (np.zeros(max(edge_cap, 1), np.int32) for _ in range(3))
    inc_ptr, inc_edge = np.zeros(n + 1, np.int32), np.zeros(2 * max(edge_cap, 1), np.int32)
    ne = C.c_int32(0)
    _check(lib().slamit_essential_plan(C.byref(g), edge_cap, _np_ptr(v0), _np_ptr(v1), _np_ptr(kind), C.byref(ne), _np_ptr(inc_ptr), _np_ptr(inc_edge)),
           "slamit_essential_plan")
    e = ne.value
    return dict(edge_v0=v0[:e].copy(), edge_v1=v1[:e].copy(), edge_kind=kind[:e].copy(), inc_ptr=inc_ptr, inc_edge=inc_edge[:2 * e].copy())


def _eg_stats(st):
    n, q = int(st.n_its), min(int(st.n_trials), EG_MAX_TRIALS)
    return dict(n_its=n, n_trials=int(st.n_trials), n_free=int(st.n_free), chi2_init=float(st.chi2_init), chi2=np.array(st.chi2[:n]),
                lam=np.array(getattr(st, "lambda")[:n]), trials=np.array(st.trials[:n], np.int32), trial_chi2=np.array(st.trial_chi2[:q]),
                trial_rho=np.array(st.trial_rho[:q]))


def essential_graph(prob, device=0):
    """Optimizer::OptimizeEssentialGraph on host arrays: `prob` holds the fields of slamit_eg_problem (the edges as essential_plan
    returns them; inc_ptr / inc_edge optional).  Returns sim3_r (n_kf, 9), sim3_t, sim3_s, pose (n_kf, 12), points (n_pt, 3) f32, touched
    (the good points, ascending) and the LM record (n_its, chi2, lam, trials per iteration; trial_chi2, trial_rho per trial)."""
    n, ne = int(prob["n_kf"]), len(prob["edge_v0"])
    keep = {k: np.ascontiguousarray(prob[k], dt) for k, dt in _EG_PROBLEM_ARRAYS if prob.get(k) is not None}
    npt = len(keep["pt_ref"]) if "pt_ref" in keep else 0
    p = EgProblem(n, ne, npt, 0, int(prob["fix_scale"]), int(prob.get("max_its", 20)), float(prob.get("lambda_init", 1e-16)),
                  *[_np_ptr(keep[k]) if k in keep and keep[k].size else None for k, _ in _EG_PROBLEM_ARRAYS])
    out = dict(sim3_r=np.zeros((n, 9)), sim3_t=np.zeros((n, 3)), sim3_s=np.zeros(n), pose=np.zeros((n, 12)), points=np.zeros((npt, 3), np.float32),
               touched=np.zeros(npt, np.int32))
    nt, st = np.zeros(1, np.int32), EgStats()
    r = EgResult(*[_np_ptr(out[k]) if out[k].size else None for k in ("sim3_r", "sim3_t", "sim3_s", "pose", "points", "touched")], _np_ptr(nt),
                 C.cast(C.byref(st), C.c_void_p))
    _check(lib().slamit_essential_graph(device, C.byref(p), C.byref(r)), "slamit_essential_graph")
    out["touched"] = out["touched"][:int(nt[0])]
    out.update(_eg_stats(st))
    return out


def essential_graph_workspace(n_free, n_kf, n_edge, n_pt):
    return int(lib().slamit_essential_graph_workspace(n_free, n_kf, n_edge, n_pt))


def essential_graph_dev(t, n_free, fix_scale, max_its=20, lambda_init=1e-16, device=0, stream=None):
    """The same, resident.  t: dict of torch CUDA tensors -- the arrays of slamit_eg_problem (inc_ptr and inc_edge required) and of
    slamit_eg_result (sim3_r, sim3_t, sim3_s, pose f64; points f32; touched, n_touched i32; stats: uint8 of ctypes.sizeof(EgStats)) and
    workspace (uint8, essential_graph_workspace(...) bytes, 256-byte aligned).  n_free: the keyframes neither fixed nor bad.  Waits on
    `stream` once per LM trial; the result is complete on return (the stream's later work may go on reading it there)."""
    n, ne, npt = t["scw_s"].shape[0], t["edge_v0"].shape[0], t["pt_ref"].shape[0]
    ptr = lambda k: t[k].data_ptr() if t[k].numel() else None
    p = EgProblem(n, ne, npt, int(n_free), int(fix_scale), int(max_its), float(lambda_init), *[ptr(k) for k, _ in _EG_PROBLEM_ARRAYS])
    r = EgResult(*[ptr(k) for k in ("sim3_r", "sim3_t", "sim3_s", "pose", "points", "touched", "n_touched", "stats")])
    ws = t["workspace"]
    _check(lib().slamit_essential_graph_dev(device, C.byref(p), C.byref(r), ws.data_ptr(), ws.numel() * ws.element_size(), stream),
           "slamit_essential_graph_dev")


def eg_stats_from_bytes(buf):
    """The LM record out of the bytes of a slamit_eg_stats (essential_graph_dev's `stats` tensor, copied to the host)."""
    return _eg_stats(EgStats.from_buffer_copy(bytes(buf)))
