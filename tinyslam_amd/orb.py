"""Host-side mirror of the reference's `tinyslam::orb` module over the C ABI (include/tinyorb.h).

Same names and argument meaning as src/orb.rs: `OrbConfig` (orb.rs:40-45), `OrbProgram` with
`init` (107), `write_input_image` (567), `set_threshold` (585), `extract_corners` (469),
`read_corners` (559), `read_descriptors` (563), and the POD records `CornerData` (10-17) /
`CornerDescriptor` (19-23).  Where the reference panics this raises `OrbError`.

There is no CPU fallback: if libtinyorb.so is missing or no HIP device is present, loading
or `init()` raises.
"""
import ctypes
import importlib.util
import os
from dataclasses import dataclass, field

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TINYORB_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libtinyorb.so")  # TINYORB_LIB: A/B of two builds on one box

ORB_OK, ORB_EINVAL, ORB_EHIP, ORB_ECAPACITY, ORB_ESTATE = 0, 1, 2, 3, 4
ORB_PLANE_GRAY, ORB_PLANE_BLUR = 0, 1
ORB_KERNEL_COUNT = 25
ORB_FLAG_STAGED = 1
ORB_FLAG_DOUBLE_OUTPUT = 2
ORB_FLAG_NMS = 4
ORB_FLAG_INTENDED = 8
ORB_FLAG_INPUT_Y8 = 16
ORB_FLAG_SINGLE_BLOCKING_WAIT = 32  # orb_extract_corners: bounded spin, then sleep until the completion interrupt
ORB_OOB_ZERO, ORB_OOB_CLAMP, ORB_OOB_UMIN = 0, 1, 2  # OrbOptions.oob_policy
OOB_POLICIES = {"zero": ORB_OOB_ZERO, "clamp": ORB_OOB_CLAMP, "umin": ORB_OOB_UMIN}
# OrbOptions.fp_contract (CRD-13): which stages' products and sums the adapter's shader compiler fuses, and its reduction order
ORB_FP_CONTRACT_LUMINANCE, ORB_FP_CONTRACT_BLUR, ORB_FP_CONTRACT_ROTATION, ORB_FP_CONTRACT_ALL, ORB_FP_LAST_TERM_FIRST = 1, 2, 4, 7, 8
TRANSPORT_RECORD_WORDS = 10  # ORB_TRANSPORT_RECORD_BYTES / 4
SYN_GRADIENT, SYN_BLOBS, SYN_WEDGES, SYN_NOISE = 1, 2, 4, 8
SYN_ALL = 15

# orb.rs:10-17 / orb.rs:19-23 as numpy record layouts (16 B / 32 B)
CORNER_DTYPE = np.dtype([("x", "<u4"), ("y", "<u4"), ("angle", "<u4"), ("octave", "<u4")])
MATCH_DTYPE = np.dtype([("index", "<u4"), ("distance", "<u2"), ("second", "<u2")])
ORB_MATCH_NONE = 0xFFFFFFFF
DESCRIPTOR_DTYPE = np.dtype([("bits", "u1", (32,))])
# csrc/orb_kernels_front.h BlurCol, the fractions as bit patterns (OrbProgram.blur_col_table)
BLUR_COL_DTYPE = np.dtype([("a0", "<u2"), ("a1", "<u2"), ("b0", "<u2"), ("b1", "<u2"), ("fa", "<u4"), ("fb", "<u4"), ("f2", "<u4"), ("pad", "<u4")])
# geometric verification (orb_verify_consecutive): OrbPairModel (64 B) and its status codes
VERIFY_MODEL_DTYPE = np.dtype([("h", "<f4", (9,)), ("candidates", "<u4"), ("inliers", "<u4"), ("hypothesis", "<u4"),
                               ("status", "<u4"), ("reserved", "<u4", (3,))])
ORB_VERIFY_OK, ORB_VERIFY_FEW, ORB_VERIFY_DEGENERATE, ORB_VERIFY_MINIMAL = 0, 1, 2, 3
ORB_VERIFY_MAX_HYPOTHESES = 4096
# guided matching (orb_match_guided): where a pair's model comes from, and the flag of OrbGuideParams
ORB_GUIDE_VERIFIED, ORB_GUIDE_IDENTITY, ORB_GUIDE_HOST = 0, 1, 2
ORB_GUIDE_SCALE_RADIUS = 1
# epipolar-band guided matching (orb_match_epipolar): where a pair's F comes from, and the flag of OrbBandParams
ORB_BAND_VERIFIED, ORB_BAND_HOST = 0, 1
ORB_BAND_SCALE = 1
# relative pose and triangulation (orb_pose_consecutive): OrbPairPose (64 B), OrbPoint (16 B), status and flags
POSE_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("inliers", "<u4"), ("good", "<u4"), ("second", "<u4"), ("status", "<u4")])
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("flags", "<u4")])
ORB_POSE_OK, ORB_POSE_NOMODEL, ORB_POSE_FEW, ORB_POSE_AMBIGUOUS, ORB_POSE_LOW_PARALLAX = 0, 1, 2, 3, 4
ORB_POINT_GOOD, ORB_POINT_PARALLAX = 1, 2
# trajectory and map in one frame and one unit (orb_trajectory_consecutive): OrbFramePose (80 B), its status,
# the flag of OrbTrajectoryParams
FRAME_POSE_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4"), ("step", "<f4"), ("origin", "<u4"),
                             ("shared", "<u4"), ("consistent", "<u4"), ("status", "<u4"), ("reserved", "<u4", (2,))])
ORB_TRAJ_CHAINED, ORB_TRAJ_START, ORB_TRAJ_RESTART_FEW, ORB_TRAJ_RESTART_SPREAD, ORB_TRAJ_LOST, ORB_TRAJ_ORIGIN = 0, 1, 2, 3, 4, 5
ORB_TRAJ_NEED_PARALLAX = 1
# absolute pose from the previous pair's map points (orb_localize_consecutive): OrbFrameFix (80 B), its status
FIX_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("step", "<f4"), ("candidates", "<u4"), ("inliers", "<u4"),
                      ("hypothesis", "<u4"), ("status", "<u4"), ("reserved", "<u4", (3,))])
ORB_LOCALIZE_OK, ORB_LOCALIZE_NOMAP, ORB_LOCALIZE_FEW, ORB_LOCALIZE_DEGENERATE, ORB_LOCALIZE_MINIMAL = 0, 1, 2, 3, 4
# one multi-view map point per landmark (orb_landmarks_consecutive): OrbLandmark (32 B), OrbLandmarkRow (16 B)
LANDMARK_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("flags", "<u4"), ("views", "<u2"), ("inliers", "<u2"),
                           ("origin", "<u4"), ("tail_index", "<u4"), ("reserved", "<u4", (1,))])
LANDMARK_ROW_DTYPE = np.dtype([("landmarks", "<u4"), ("good", "<u4"), ("longest", "<u4"), ("origin", "<u4")])
ORB_LANDMARK_NO_ORIGIN = 0xFFFFFFFF
# a trajectory carried across LOST frames (orb_bridge_consecutive): OrbBridgePose (96 B), its status
BRIDGE_POSE_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4"), ("gain", "<f4"), ("root", "<u4"), ("anchor", "<u4"),
                              ("candidates", "<u4"), ("inliers", "<u4"), ("hypothesis", "<u4"), ("shared", "<u4"), ("consistent", "<u4"),
                              ("fix", "<u4"), ("status", "<u4"), ("reserved", "<u4", (1,))])
ORB_BRIDGE_COPIED, ORB_BRIDGE_MOVED, ORB_BRIDGE_FIXED, ORB_BRIDGE_JOINED, ORB_BRIDGE_UNFIXED = 0, 1, 2, 3, 4
# poses and landmarks refined by reprojection (orb_adjust_consecutive): OrbAdjustedPose (64 B), its status
ADJUSTED_POSE_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("cost_before", "<f4"), ("cost_after", "<f4"),
                                ("observations", "<u4"), ("status", "<u4")])
ORB_ADJUST_HELD, ORB_ADJUST_REFINED, ORB_ADJUST_FEW, ORB_ADJUST_FAILED = 0, 1, 2, 3
# feature tracks and keyframes (orb_track_consecutive): the link source, OrbTrack (16 B), OrbTrackFrame (32 B)
ORB_TRACK_VERIFIED, ORB_TRACK_GUIDED, ORB_TRACK_MATCHED = 0, 1, 2
TRACK_DTYPE = np.dtype([("prev", "<u4"), ("next", "<u4"), ("head_index", "<u4"), ("head_frame", "<u2"), ("tail_frame", "<u2")])
TRACK_FRAME_DTYPE = np.dtype([("keypoints", "<u4"), ("links_in", "<u4"), ("links_out", "<u4"), ("keyframe", "<u4"),
                              ("ref_keyframe", "<u4"), ("shared", "<u4"), ("reserved", "<u4", (2,))])
# loop candidates by descriptor-signature overlap (orb_place_frames): OrbPlaceCandidate (8 B), OrbPlaceRow (96 B),
# the flag of OrbPlaceParams, the mark of a database entry in a row, and the two capacities
PLACE_CANDIDATE_DTYPE = np.dtype([("frame", "<u4"), ("score", "<u4")])
PLACE_ROW_DTYPE = np.dtype([("keypoints", "<u4"), ("bits_set", "<u4"), ("eligible", "<u4"), ("candidates", "<u4"), ("n", "<u4"),
                            ("reserved", "<u4", (3,)), ("best", PLACE_CANDIDATE_DTYPE, (8,))])
ORB_PLACE_KEYFRAMES = 1
ORB_PLACE_DB = 0x80000000
ORB_PLACE_SIG_BYTES_MAX = 65536
ORB_PLACE_DB_MAX = 1024
# matching and verification of caller-listed frame pairs (orb_match_pairs, orb_verify_pairs): OrbFramePair (8 B),
# the pairs a call takes per frame of max_batch, and the two models of orb_verify_pairs
FRAME_PAIR_DTYPE = np.dtype([("query", "<u4"), ("target", "<u4")])
ORB_PAIRS_PER_FRAME = 4
ORB_PAIRS_HOMOGRAPHY = 0
ORB_PAIRS_EPIPOLAR = 1
# a listed query's pose from its target's landmarks (orb_loop_pairs): OrbLoopFix (128 B); status ORB_LOCALIZE_*
LOOP_FIX_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("step", "<f4"), ("pose_r", "<f4", (9,)), ("pose_t", "<f4", (3,)),
                           ("origin", "<u4"), ("query_origin", "<u4"), ("candidates", "<u4"), ("inliers", "<u4"), ("hypothesis", "<u4"),
                           ("status", "<u4"), ("reserved", "<u4", (1,))])
ORB_LOOP_NO_ORIGIN = 0xFFFFFFFF
# pose-graph correction from the loop fixes (orb_graph_pairs): OrbGraphPose (64 B) and its status, OrbGraphEdge
# (16 B) and its verdict, the flag of OrbGraphParams
GRAPH_POSE_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("cost_before", "<f4"), ("cost_after", "<f4"), ("loops", "<u4"),
                             ("status", "<u4")])
GRAPH_EDGE_DTYPE = np.dtype([("verdict", "<u4"), ("cost_before", "<f4"), ("cost_after", "<f4"), ("origin", "<u4")])
ORB_GRAPH_HELD, ORB_GRAPH_UNCHANGED, ORB_GRAPH_REFINED, ORB_GRAPH_STALLED, ORB_GRAPH_FAILED, ORB_GRAPH_INVALID = 0, 1, 2, 3, 4, 5
(ORB_GRAPH_EDGE_USED, ORB_GRAPH_EDGE_STATUS, ORB_GRAPH_EDGE_FEW, ORB_GRAPH_EDGE_RANGE, ORB_GRAPH_EDGE_SEGMENT, ORB_GRAPH_EDGE_NONFINITE,
 ORB_GRAPH_EDGE_SEGMENT_INVALID) = 0, 1, 2, 3, 4, 5, 6
ORB_GRAPH_USE_MINIMAL = 1
# trajectory segments joined through loop fixes (orb_join_pairs): OrbJoinPose (64 B) and its status,
# OrbJoinSegment (64 B) and its status, OrbJoinLink (32 B) and its verdict, the flag of OrbJoinParams
JOIN_POSE_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4"), ("gain", "<f4"), ("root", "<u4"), ("status", "<u4")])
JOIN_SEGMENT_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("sigma", "<f4"), ("root", "<u4"), ("link", "<u4"), ("status", "<u4")])
JOIN_LINK_DTYPE = np.dtype([("verdict", "<u4"), ("origin", "<u4"), ("query_origin", "<u4"), ("shared", "<u4"), ("consistent", "<u4"),
                            ("gamma", "<f4"), ("chosen", "<u4"), ("reserved", "<u4")])
ORB_JOIN_COPIED, ORB_JOIN_MOVED = 0, 1
ORB_JOIN_SEGMENT_NONE, ORB_JOIN_SEGMENT_ROOT, ORB_JOIN_SEGMENT_LINKED = 0, 1, 2
(ORB_JOIN_LINK_HOLDS, ORB_JOIN_LINK_STATUS, ORB_JOIN_LINK_FEW, ORB_JOIN_LINK_RANGE, ORB_JOIN_LINK_SAME, ORB_JOIN_LINK_FORWARD,
 ORB_JOIN_LINK_NONFINITE, ORB_JOIN_LINK_RATIO_FEW, ORB_JOIN_LINK_RATIO_SPREAD) = 0, 1, 2, 3, 4, 5, 6, 7, 8
ORB_JOIN_USE_MINIMAL = 1
ORB_JOIN_NO_LINK = 0xFFFFFFFF
# corrected poses and landmarks in one root frame (orb_remap_frames): OrbRemapPose (64 B) and its status bits,
# OrbRemapRow (16 B), the source flags of OrbRemapParams; the landmarks come back as LANDMARK_DTYPE
REMAP_POSE_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4"), ("gain", "<f4"), ("root", "<u4"), ("status", "<u4")])
REMAP_ROW_DTYPE = np.dtype([("good", "<u4"), ("moved", "<u4"), ("dropped", "<u4"), ("root", "<u4")])
ORB_REMAP_GRAPH, ORB_REMAP_JOIN = 1, 2
ORB_REMAP_FROM_GRAPH, ORB_REMAP_MOVED = 1, 2
# a keyframe store that outlives a batch (orb_keyframes_*, orb_match_keyframes, orb_localize_keyframes):
# OrbKeyframe (96 B) and its status, OrbMapPoint (16 B), OrbKeyframeEntry (16 B), OrbKeyframePair (8 B), OrbKeyframeFix (128 B:
# LOOP_FIX_DTYPE with the slot where the query's origin is there)
KEYFRAME_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4"), ("keypoints", "<u4"), ("points", "<u4"), ("frame", "<u4"),
                           ("origin", "<u4"), ("user", "<u4", (2,)), ("status", "<u4"), ("reserved", "<u4", (4,))])
MAP_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("key", "<u4")])
KEYFRAME_ENTRY_DTYPE = np.dtype([("frame", "<u4"), ("slot", "<u4"), ("user", "<u4", (2,))])
KEYFRAME_PAIR_DTYPE = np.dtype([("query", "<u4"), ("slot", "<u4")])
KEYFRAME_FIX_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("step", "<f4"), ("pose_r", "<f4", (9,)), ("pose_t", "<f4", (3,)),
                               ("origin", "<u4"), ("slot", "<u4"), ("candidates", "<u4"), ("inliers", "<u4"), ("hypothesis", "<u4"),
                               ("status", "<u4"), ("reserved", "<u4", (1,))])
ORB_KEYFRAME_SLOTS_MAX = 1024
ORB_KEYFRAME_NONE = 0xFFFFFFFF
ORB_KEYFRAME_EMPTY, ORB_KEYFRAME_STORED, ORB_KEYFRAME_NOMAP = 0, 1, 2
# a batch's path and landmarks in the stored map (orb_anchor_frames): OrbAnchorPose (64 B) and its status,
# OrbAnchorSegment (96 B) and its status, OrbAnchorLink (32 B) and its verdict, OrbAnchorRow (32 B), the flag of OrbAnchorParams; the
# landmarks come back as LANDMARK_DTYPE
ANCHOR_POSE_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("scale", "<f4"), ("gain", "<f4"), ("slot", "<u4"), ("status", "<u4")])
ANCHOR_SEGMENT_DTYPE = np.dtype([("r", "<f4", (9,)), ("t", "<f4", (3,)), ("gamma", "<f4"), ("slot", "<u4"), ("link", "<u4"), ("map_origin", "<u4"),
                                 ("map_frame", "<u4"), ("user", "<u4", (2,)), ("status", "<u4"), ("reserved", "<u4", (4,))])
ANCHOR_LINK_DTYPE = np.dtype([("verdict", "<u4"), ("query_origin", "<u4"), ("slot", "<u4"), ("shared", "<u4"), ("consistent", "<u4"),
                              ("gamma", "<f4"), ("chosen", "<u4"), ("reserved", "<u4")])
ANCHOR_ROW_DTYPE = np.dtype([("good", "<u4"), ("moved", "<u4"), ("dropped", "<u4"), ("origin", "<u4"), ("slot", "<u4"), ("map_origin", "<u4"),
                             ("reserved", "<u4", (2,))])
ORB_ANCHOR_FREE, ORB_ANCHOR_ANCHORED = 0, 1
ORB_ANCHOR_SEGMENT_NONE, ORB_ANCHOR_SEGMENT_FREE, ORB_ANCHOR_SEGMENT_ANCHORED = 0, 1, 2
(ORB_ANCHOR_LINK_HOLDS, ORB_ANCHOR_LINK_STATUS, ORB_ANCHOR_LINK_FEW, ORB_ANCHOR_LINK_RANGE, ORB_ANCHOR_LINK_NONFINITE, ORB_ANCHOR_LINK_RATIO_FEW,
 ORB_ANCHOR_LINK_RATIO_SPREAD) = 0, 1, 2, 3, 4, 5, 6
ORB_ANCHOR_USE_MINIMAL = 1
ORB_ANCHOR_NONE = 0xFFFFFFFF

# Names every build of libtinyorb.so must export (checked by tests against include/tinyorb.h).
EXPORTS = [
    "orb_abi_version", "orb_pipeline", "orb_last_error", "orb_kernel_name", "orb_program_create", "orb_program_destroy",
    "orb_write_input_image", "orb_set_threshold", "orb_extract_corners", "orb_read_corners",
    "orb_read_descriptors", "orb_extract_batch_device", "orb_extract_batch_host", "orb_batch_sync",
    "orb_batch_counts", "orb_batch_read", "orb_batch_select_output", "orb_batch_device_buffers", "orb_level_size",
    "orb_debug_read_plane", "orb_debug_f32_to_f16", "orb_debug_angle_code", "orb_debug_rot_table", "orb_debug_blur_col_table", "orb_profile_enable",
    "orb_profile_reset", "orb_profile_get", "orb_synth_frames_device", "orb_copy_to_host", "orb_debug_stamps",
    "orb_match_consecutive", "orb_match_read", "orb_corner_level0_xy",
    "orb_batch_read_all", "orb_batch_compact_device", "orb_host_alloc", "orb_host_free", "orb_stream_sync",
    "orb_program_stream", "orb_pipeline_note", "orb_batch_pack", "orb_batch_fetch",
    "orb_batch_pack_transport", "orb_unpack_transport",
    "orb_node_create", "orb_node_destroy", "orb_node_last_error", "orb_node_device_count", "orb_node_program",
    "orb_node_shard", "orb_node_extract_batch", "orb_node_extract_batch_host", "orb_node_collate",
    "orb_node_read_collated", "orb_node_collate_begin", "orb_node_collate_end", "orb_node_pending",
    "orb_extract_batch_pinned", "orb_upload_sync", "orb_node_exchange_backend", "orb_node_rccl_pairs",
    "orb_write_input_image_pinned", "orb_node_set_results", "orb_node_shard_result",
    "orb_verify_consecutive", "orb_verify_read", "orb_match_guided", "orb_match_guided_read",
    "orb_track_consecutive", "orb_track_read", "orb_track_frames", "orb_verify_epipolar", "orb_verify_epipolar_read",
    "orb_match_epipolar", "orb_match_epipolar_read", "orb_pose_consecutive", "orb_pose_read",
    "orb_trajectory_consecutive", "orb_trajectory_read", "orb_debug_pose_buffers", "orb_debug_frame_buffer",
    "orb_localize_consecutive", "orb_localize_read",
    "orb_landmarks_consecutive", "orb_landmarks_read",
    "orb_bridge_consecutive", "orb_bridge_read",
    "orb_adjust_consecutive", "orb_adjust_read",
    "orb_place_frames", "orb_place_read", "orb_place_signature",
    "orb_match_pairs", "orb_match_pairs_read", "orb_verify_pairs", "orb_verify_pairs_read",
    "orb_loop_pairs", "orb_loop_pairs_read", "orb_debug_loop_buffer",
    "orb_graph_pairs", "orb_graph_read", "orb_graph_edges",
    "orb_join_pairs", "orb_join_read", "orb_join_segments", "orb_join_links", "orb_debug_loop_mask_buffer",
    "orb_remap_frames", "orb_remap_read", "orb_remap_landmarks",
    "orb_keyframes_reserve", "orb_keyframes_insert", "orb_keyframes_read", "orb_keyframes_load", "orb_keyframes_remove",
    "orb_match_keyframes", "orb_match_keyframes_read", "orb_localize_keyframes", "orb_localize_keyframes_read",
    "orb_anchor_frames", "orb_anchor_read", "orb_anchor_segments", "orb_anchor_links", "orb_anchor_landmarks", "orb_debug_keyframe_buffers",
]


def level0_xy(corners):
    """Centres of the keypoints' pixels in level-0 pixel units (orb_corner_level0_xy of include/tinyorb.h)."""
    s = np.left_shift(1, corners["octave"].astype(np.int64)).astype(np.float32)
    return ((corners["x"].astype(np.float32) + np.float32(0.5)) * s - np.float32(0.5),
            (corners["y"].astype(np.float32) + np.float32(0.5)) * s - np.float32(0.5))


class OrbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("tinyorb error %d: %s" % (code, msg))
        self.code = code


class _Extent3d(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("depth_or_array_layers", ctypes.c_uint32)]


class _Config(ctypes.Structure):
    _fields_ = [("image_size", _Extent3d), ("max_features", ctypes.c_uint32), ("hierarchy_depth", ctypes.c_uint32),
                ("initial_threshold", ctypes.c_float)]


class _VerifyParams(ctypes.Structure):
    """OrbVerifyParams (32 bytes; zero fields = the defaults)"""
    _fields_ = [("hypotheses", ctypes.c_uint32), ("max_distance", ctypes.c_uint32), ("ratio", ctypes.c_float),
                ("inlier_px", ctypes.c_float), ("seed", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class _GuideParams(ctypes.Structure):
    """OrbGuideParams (32 bytes; zero fields = the defaults)"""
    _fields_ = [("source", ctypes.c_uint32), ("radius_px", ctypes.c_float), ("octave_window", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]


class _BandParams(ctypes.Structure):
    """OrbBandParams (32 bytes; zero fields = the defaults)"""
    _fields_ = [("source", ctypes.c_uint32), ("band_px", ctypes.c_float), ("radius_px", ctypes.c_float),
                ("octave_window", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class _PoseParams(ctypes.Structure):
    """OrbPoseParams (32 bytes; fx and fy must be > 0, the other zero fields = the defaults)"""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("max_reproj_px", ctypes.c_float), ("max_cos_parallax", ctypes.c_float), ("min_good", ctypes.c_uint32),
                ("ambiguity_permille", ctypes.c_uint32)]


class _TrajectoryParams(ctypes.Structure):
    """OrbTrajectoryParams (32 bytes; zero fields = the defaults)"""
    _fields_ = [("min_shared", ctypes.c_uint32), ("scale_tolerance", ctypes.c_float), ("consistent_permille", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]


OrbTrajectoryParams = _TrajectoryParams


class _LocalizeParams(ctypes.Structure):
    """OrbLocalizeParams (64 bytes; fx and fy must be > 0, the other zero fields = the defaults)"""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("max_reproj_px", ctypes.c_float), ("hypotheses", ctypes.c_uint32), ("max_distance", ctypes.c_uint32),
                ("ratio", ctypes.c_float), ("seed", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 7)]


OrbLocalizeParams = _LocalizeParams


class _LandmarkParams(ctypes.Structure):
    """OrbLandmarkParams (32 bytes; fx and fy must be > 0, the other zero fields = the defaults)"""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("max_reproj_px", ctypes.c_float), ("min_views", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


OrbLandmarkParams = _LandmarkParams


class _BridgeParams(ctypes.Structure):
    """OrbBridgeParams (64 bytes; fx and fy must be > 0, the other zero fields = the defaults)"""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("max_reproj_px", ctypes.c_float), ("hypotheses", ctypes.c_uint32), ("max_distance", ctypes.c_uint32),
                ("ratio", ctypes.c_float), ("seed", ctypes.c_uint32), ("max_hops", ctypes.c_uint32), ("window", ctypes.c_uint32),
                ("min_shared", ctypes.c_uint32), ("scale_tolerance", ctypes.c_float), ("consistent_permille", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 2)]


OrbBridgeParams = _BridgeParams


class _AdjustParams(ctypes.Structure):
    """OrbAdjustParams (32 bytes; fx and fy must be > 0, the other zero fields = the defaults)"""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("max_reproj_px", ctypes.c_float), ("rounds", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


OrbAdjustParams = _AdjustParams


class _LoopParams(ctypes.Structure):
    """OrbLoopParams (64 bytes; fx and fy must be > 0, the other zero fields = the defaults)"""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("max_reproj_px", ctypes.c_float), ("hypotheses", ctypes.c_uint32), ("max_distance", ctypes.c_uint32),
                ("ratio", ctypes.c_float), ("seed", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 7)]


OrbLoopParams = _LoopParams


class _GraphParams(ctypes.Structure):
    """OrbGraphParams (32 bytes; zero fields = the defaults)"""
    _fields_ = [("rounds", ctypes.c_uint32), ("cg_iterations", ctypes.c_uint32), ("min_inliers", ctypes.c_uint32),
                ("loop_weight", ctypes.c_float), ("rotation_weight", ctypes.c_float), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 2)]


OrbGraphParams = _GraphParams


class _JoinParams(ctypes.Structure):
    """OrbJoinParams (32 bytes; zero fields = the defaults)"""
    _fields_ = [("min_inliers", ctypes.c_uint32), ("min_shared", ctypes.c_uint32), ("scale_tolerance", ctypes.c_float),
                ("consistent_permille", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


OrbJoinParams = _JoinParams


class _AnchorParams(ctypes.Structure):
    """OrbAnchorParams (32 bytes; zero fields = the defaults)"""
    _fields_ = [("min_inliers", ctypes.c_uint32), ("min_shared", ctypes.c_uint32), ("scale_tolerance", ctypes.c_float),
                ("consistent_permille", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


OrbAnchorParams = _AnchorParams


class _RemapParams(ctypes.Structure):
    """OrbRemapParams (32 bytes; zero fields = the defaults)"""
    _fields_ = [("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 7)]


OrbRemapParams = _RemapParams


class _PlaceParams(ctypes.Structure):
    """OrbPlaceParams (32 bytes; zero fields = the defaults)"""
    _fields_ = [("bits", ctypes.c_uint32), ("tables", ctypes.c_uint32), ("min_gap", ctypes.c_uint32), ("top", ctypes.c_uint32),
                ("min_score", ctypes.c_uint32), ("min_permille", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


OrbPlaceParams = _PlaceParams


class _TrackParams(ctypes.Structure):
    """OrbTrackParams (32 bytes; zero fields = the defaults)"""
    _fields_ = [("source", ctypes.c_uint32), ("max_distance", ctypes.c_uint32), ("ratio", ctypes.c_float), ("min_gap", ctypes.c_uint32),
                ("max_gap", ctypes.c_uint32), ("keep_permille", ctypes.c_uint32), ("min_shared", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class _Options(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("max_batch", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("fast_arc", ctypes.c_uint32), ("oob_policy", ctypes.c_uint32), ("sampler_weight_bits", ctypes.c_uint32),
                ("fp_contract", ctypes.c_uint32), ("angle_bins", ctypes.c_uint32)]


_lib = None


def _preload_hip_runtime():
    """If PyTorch is installed, bind to ITS bundled libamdhip64 so that a later `import torch`
    (bench.py, torch.distributed) shares one HIP runtime with libtinyorb instead of loading a
    second copy next to the system one."""
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load_library(path=None):
    """Loads libtinyorb.so.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise OrbError(ORB_EHIP, "%s not found: run `python -m tinyslam_amd.build` (hipcc, gfx950)" % path)
    _preload_hip_runtime()
    L = ctypes.CDLL(path)
    vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    L.orb_abi_version.restype = u32
    L.orb_last_error.restype = ctypes.c_char_p
    L.orb_last_error.argtypes = [vp]
    L.orb_kernel_name.restype = ctypes.c_char_p
    L.orb_pipeline.restype = ctypes.c_char_p
    L.orb_pipeline.argtypes = [vp]
    L.orb_pipeline_note.restype = ctypes.c_char_p
    L.orb_pipeline_note.argtypes = [vp]
    L.orb_kernel_name.argtypes = [ctypes.c_int]
    L.orb_program_create.argtypes = [ctypes.POINTER(_Config), ctypes.POINTER(_Options), ctypes.POINTER(vp)]
    L.orb_program_destroy.argtypes = [vp]
    L.orb_program_destroy.restype = None
    L.orb_write_input_image.argtypes = [vp, vp, sz]
    L.orb_write_input_image_pinned.argtypes = [vp, vp, sz]
    L.orb_set_threshold.argtypes = [vp, ctypes.c_float]
    L.orb_extract_corners.argtypes = [vp, ctypes.POINTER(u32)]
    L.orb_read_corners.argtypes = [vp, vp, sz]
    L.orb_read_descriptors.argtypes = [vp, vp, sz]
    L.orb_extract_batch_device.argtypes = [vp, vp, u32, vp]
    L.orb_extract_batch_host.argtypes = [vp, vp, u32]
    L.orb_batch_sync.argtypes = [vp]
    L.orb_batch_counts.argtypes = [vp, vp, u32]
    L.orb_batch_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_batch_select_output.argtypes = [vp, u32]
    L.orb_batch_device_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.orb_level_size.argtypes = [vp, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.orb_debug_pose_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.orb_debug_frame_buffer.argtypes = [vp, ctypes.POINTER(vp)]
    L.orb_debug_read_plane.argtypes = [vp, u32, ctypes.c_int, u32, vp, sz]
    L.orb_debug_f32_to_f16.argtypes = [vp, vp, vp, sz]
    L.orb_debug_angle_code.argtypes = [vp, vp, vp, vp, sz]
    L.orb_debug_rot_table.argtypes = [vp, vp, sz, vp, vp]
    L.orb_debug_blur_col_table.argtypes = [vp, u32, vp, sz, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.orb_match_consecutive.argtypes = [vp, u32, vp]
    L.orb_match_read.argtypes = [vp, u32, vp, ctypes.c_size_t]
    L.orb_verify_consecutive.argtypes = [vp, u32, ctypes.POINTER(_VerifyParams), vp]
    L.orb_verify_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_verify_epipolar.argtypes = [vp, u32, ctypes.POINTER(_VerifyParams), vp]
    L.orb_verify_epipolar_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_match_guided.argtypes = [vp, u32, ctypes.POINTER(_GuideParams), vp, vp]
    L.orb_match_guided_read.argtypes = [vp, u32, vp, sz]
    L.orb_match_epipolar.argtypes = [vp, u32, ctypes.POINTER(_BandParams), vp, vp]
    L.orb_match_epipolar_read.argtypes = [vp, u32, vp, sz]
    L.orb_pose_consecutive.argtypes = [vp, u32, ctypes.POINTER(_PoseParams), vp]
    L.orb_pose_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_trajectory_consecutive.argtypes = [vp, u32, ctypes.POINTER(_TrajectoryParams), vp]
    L.orb_trajectory_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_localize_consecutive.argtypes = [vp, u32, ctypes.POINTER(_LocalizeParams), vp]
    L.orb_localize_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_landmarks_consecutive.argtypes = [vp, u32, ctypes.POINTER(_LandmarkParams), vp]
    L.orb_landmarks_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_bridge_consecutive.argtypes = [vp, u32, ctypes.POINTER(_BridgeParams), vp]
    L.orb_bridge_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_adjust_consecutive.argtypes = [vp, u32, ctypes.POINTER(_AdjustParams), vp]
    L.orb_adjust_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_place_frames.argtypes = [vp, u32, ctypes.POINTER(_PlaceParams), vp, u32, vp]
    L.orb_place_read.argtypes = [vp, u32, vp, sz]
    L.orb_place_signature.argtypes = [vp, u32, vp, sz]
    L.orb_match_pairs.argtypes = [vp, vp, u32, vp]
    L.orb_match_pairs_read.argtypes = [vp, u32, vp, sz]
    L.orb_verify_pairs.argtypes = [vp, u32, u32, ctypes.POINTER(_VerifyParams), vp]
    L.orb_verify_pairs_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_loop_pairs.argtypes = [vp, u32, ctypes.POINTER(_LoopParams), vp]
    L.orb_loop_pairs_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_debug_loop_buffer.argtypes = [vp, ctypes.POINTER(vp)]
    L.orb_graph_pairs.argtypes = [vp, u32, ctypes.POINTER(_GraphParams), vp]
    L.orb_graph_read.argtypes = [vp, u32, vp]
    L.orb_graph_edges.argtypes = [vp, vp, sz]
    L.orb_join_pairs.argtypes = [vp, u32, ctypes.POINTER(_JoinParams), vp]
    L.orb_join_read.argtypes = [vp, u32, vp]
    L.orb_join_segments.argtypes = [vp, vp, sz]
    L.orb_join_links.argtypes = [vp, vp, sz]
    L.orb_debug_loop_mask_buffer.argtypes = [vp, ctypes.POINTER(vp)]
    L.orb_remap_frames.argtypes = [vp, ctypes.POINTER(_RemapParams), vp]
    L.orb_remap_read.argtypes = [vp, u32, vp]
    L.orb_remap_landmarks.argtypes = [vp, u32, vp, vp, sz]
    L.orb_keyframes_reserve.argtypes = [vp, u32]
    L.orb_keyframes_insert.argtypes = [vp, vp, u32, vp]
    L.orb_keyframes_read.argtypes = [vp, u32, vp, vp, vp, vp, sz]
    L.orb_keyframes_load.argtypes = [vp, u32, vp, vp, vp, vp, sz]
    L.orb_keyframes_remove.argtypes = [vp, u32]
    L.orb_match_keyframes.argtypes = [vp, vp, u32, vp]
    L.orb_match_keyframes_read.argtypes = [vp, u32, vp, sz]
    L.orb_localize_keyframes.argtypes = [vp, u32, ctypes.POINTER(_LoopParams), vp]
    L.orb_localize_keyframes_read.argtypes = [vp, u32, vp, vp, sz]
    L.orb_anchor_frames.argtypes = [vp, u32, ctypes.POINTER(_AnchorParams), vp]
    L.orb_anchor_read.argtypes = [vp, u32, vp]
    L.orb_anchor_segments.argtypes = [vp, vp, sz]
    L.orb_anchor_links.argtypes = [vp, vp, sz]
    L.orb_anchor_landmarks.argtypes = [vp, u32, vp, vp, sz]
    L.orb_debug_keyframe_buffers.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.orb_track_consecutive.argtypes = [vp, u32, ctypes.POINTER(_TrackParams), vp]
    L.orb_track_read.argtypes = [vp, u32, vp, sz]
    L.orb_track_frames.argtypes = [vp, vp, sz]
    L.orb_profile_enable.argtypes = [vp, ctypes.c_int]
    L.orb_profile_reset.argtypes = [vp]
    L.orb_profile_get.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
    L.orb_synth_frames_device.argtypes = [vp, vp, u32, u32, u32, ctypes.POINTER(vp)]
    L.orb_copy_to_host.argtypes = [vp, vp, vp, sz]
    L.orb_debug_stamps.argtypes = [vp, vp, sz]
    L.orb_corner_level0_xy.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.orb_corner_level0_xy.restype = None
    L.orb_batch_read_all.argtypes = [vp, u32, vp, vp, vp, vp, sz, vp]
    L.orb_batch_compact_device.argtypes = [vp, u32, vp, vp, vp, vp, sz, vp]
    L.orb_batch_pack.argtypes = [vp, u32, vp]
    L.orb_batch_fetch.argtypes = [vp, u32, vp, vp, vp, vp, sz, vp]
    L.orb_batch_pack_transport.argtypes = [vp, u32, u32, vp, sz, vp, vp]
    L.orb_unpack_transport.argtypes = [vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.orb_host_alloc.argtypes = [sz, ctypes.POINTER(vp)]
    L.orb_host_free.argtypes = [vp]
    L.orb_host_free.restype = None
    L.orb_stream_sync.argtypes = [vp, vp]
    L.orb_program_stream.argtypes = [vp]
    L.orb_program_stream.restype = vp
    L.orb_node_create.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(_Config), ctypes.POINTER(_Options),
                                  ctypes.POINTER(vp)]
    L.orb_node_destroy.argtypes = [vp]
    L.orb_node_destroy.restype = None
    L.orb_node_last_error.argtypes = [vp]
    L.orb_node_last_error.restype = ctypes.c_char_p
    L.orb_node_device_count.argtypes = [vp]
    L.orb_node_program.argtypes = [vp, ctypes.c_int]
    L.orb_node_program.restype = vp
    L.orb_node_shard.argtypes = [vp, u32, ctypes.c_int, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.orb_node_extract_batch.argtypes = [vp, ctypes.POINTER(vp), u32]
    L.orb_node_extract_batch_host.argtypes = [vp, vp, u32]
    L.orb_node_collate.argtypes = [vp, vp, vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.orb_node_read_collated.argtypes = [vp, vp, vp, sz]
    L.orb_node_collate_begin.argtypes = [vp]
    L.orb_node_collate_end.argtypes = [vp, vp, vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.orb_node_pending.argtypes = [vp]
    L.orb_node_set_results.argtypes = [vp, ctypes.c_int]
    L.orb_node_shard_result.argtypes = [vp, ctypes.c_int, ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.orb_node_exchange_backend.argtypes = [vp]
    L.orb_node_exchange_backend.restype = ctypes.c_char_p
    L.orb_node_rccl_pairs.argtypes = [vp]
    L.orb_node_rccl_pairs.restype = ctypes.c_uint64
    L.orb_extract_batch_pinned.argtypes = [vp, vp, u32]
    L.orb_upload_sync.argtypes = [vp]
    if L.orb_abi_version() != 5 and not os.environ.get("TINYORB_ALLOW_ABI"):  # (tools/ab_old_new.sh alternates libraries of other commits)
        raise OrbError(ORB_EINVAL, "libtinyorb ABI version mismatch")
    if path == LIB_PATH:
        _lib = L
    return L


class PinnedArray:
    """A numpy array over pinned, device-visible host memory from orb_host_alloc (freed with the object)."""

    def __init__(self, shape, dtype):
        L = load_library()
        self._lib = L
        dtype = np.dtype(dtype)
        n = int(np.prod(shape))
        self.nbytes = max(n * dtype.itemsize, 1)
        ptr = ctypes.c_void_p()
        rc = L.orb_host_alloc(self.nbytes, ctypes.byref(ptr))
        if rc != ORB_OK:
            raise OrbError(rc, (L.orb_last_error(None) or b"").decode())
        self.ptr = ptr
        buf = (ctypes.c_uint8 * self.nbytes).from_address(ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)

    def close(self):
        if self.ptr is not None:
            self.array = None
            self._lib.orb_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBatch:
    """Pinned host destination of orb_batch_read_all: counts[n], offsets[n+1], corners[capacity], descriptors[capacity]."""

    def __init__(self, n_frames, capacity):
        self.n_frames, self.capacity = n_frames, capacity
        self._c = PinnedArray((n_frames,), np.uint32)
        self._o = PinnedArray((n_frames + 1,), np.uint64)
        self._k = PinnedArray((capacity,), CORNER_DTYPE)
        self._d = PinnedArray((capacity, 8), np.uint32)
        self.counts, self.offsets, self.corners, self.descriptors = self._c.array, self._o.array, self._k.array, self._d.array

    def frame(self, f):
        lo, hi = int(self.offsets[f]), int(self.offsets[f + 1])
        return self.corners[lo:hi], self.descriptors[lo:hi]

    def close(self):
        self.counts = self.offsets = self.corners = self.descriptors = None
        for a in (self._c, self._o, self._k, self._d):
            a.close()


@dataclass
class Extent3d:
    """wgpu::Extent3d as used by OrbConfig.image_size."""
    width: int
    height: int
    depth_or_array_layers: int = 1


@dataclass
class OrbConfig:
    """orb.rs:40-45."""
    image_size: Extent3d
    max_features: int = 8192
    hierarchy_depth: int = 2
    initial_threshold: float = 20.0 / 255.0
    # build-side options (no counterpart in the reference)
    device: int = 0
    max_batch: int = 1
    flags: int = 0
    fast_arc: int = 0  # 0 -> 12 (reference; 9 with ORB_FLAG_INTENDED); 9..16 opt-in
    # the two implementation-defined points of the reference's WGSL as switches (include/tinyorb.h, OrbOptions)
    oob_policy: int = 0           # ORB_OOB_ZERO / ORB_OOB_CLAMP / ORB_OOB_UMIN: textureLoad outside the level
    sampler_weight_bits: int = 0  # 0: exact bilinear weights; n: weights held in n fractional bits
    angle_bins: int = 0   # ORB_FLAG_INTENDED, IM-6b: 0 = rotate by the milliradian code; 8..6284 = by the centre of the angle bin
    fp_contract: int = 0  # CRD-13: mask of ORB_FP_CONTRACT_LUMINANCE / _BLUR / _ROTATION (that stage's products and sums as fmas) and ORB_FP_LAST_TERM_FIRST


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class OrbProgram:
    """orb.rs:47-51 + impl 106-590.  Construct, then `init()` (the reference builds the struct
    by literal and calls `init`, orb.rs:107)."""

    def __init__(self, config: OrbConfig):
        self.config = config
        self._h = None
        self._lib_obj = None

    @property
    def _lib(self):
        if self._lib_obj is None:
            raise OrbError(ORB_ESTATE, "OrbProgram.init() has not been called")
        return self._lib_obj

    # ---- lifetime -------------------------------------------------------------------------
    def init(self):
        L = load_library()
        c = self.config
        cfg = _Config(_Extent3d(c.image_size.width, c.image_size.height, c.image_size.depth_or_array_layers),
                      c.max_features, c.hierarchy_depth, float(np.float32(c.initial_threshold)))
        opt = _Options(c.device, c.max_batch, c.flags, c.fast_arc, c.oob_policy, c.sampler_weight_bits, c.fp_contract, c.angle_bins)
        h = ctypes.c_void_p()
        rc = L.orb_program_create(ctypes.byref(cfg), ctypes.byref(opt), ctypes.byref(h))
        if rc != ORB_OK:
            raise OrbError(rc, (L.orb_last_error(None) or b"").decode())
        self._h, self._lib_obj = h, L
        return self

    def close(self):
        if self._h is not None:
            if not getattr(self, "_borrowed", False):  # programs of an OrbNode belong to the node
                self._lib.orb_program_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self if self._h is not None else self.init()

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, allow=()):
        if rc != ORB_OK and rc not in allow:
            raise OrbError(rc, (self._lib.orb_last_error(self._h) or b"").decode())
        return rc

    def _handle(self):
        if self._h is None:
            raise OrbError(ORB_ESTATE, "OrbProgram.init() has not been called")
        return self._h

    # ---- the reference's six methods --------------------------------------------------------
    def write_input_image(self, data):
        """orb.rs:567: tightly packed RGBA8 bytes (any buffer / uint8 array of 4*W*H bytes)."""
        a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview))
                                 else np.asarray(data, dtype=np.uint8))
        self._check(self._lib.orb_write_input_image(self._handle(), _ptr(a), a.size))

    def write_input_image_pinned(self, frame):
        """orb_write_input_image_pinned: `frame` is a numpy view of PINNED memory (PinnedArray.array); asynchronous, one image
        may be written ahead of extract_corners (upload_sync() waits until the array may be reused)."""
        a = np.asarray(frame)
        assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
        self._check(self._lib.orb_write_input_image_pinned(self._handle(), ctypes.c_void_p(a.ctypes.data), a.size))

    def set_threshold(self, threshold):
        """orb.rs:585"""
        self._check(self._lib.orb_set_threshold(self._handle(), float(np.float32(threshold))))

    def extract_corners(self):
        """orb.rs:469: returns the RAW counter (may exceed max_features, like the reference)."""
        n = ctypes.c_uint32(0)
        self._check(self._lib.orb_extract_corners(self._handle(), ctypes.byref(n)), allow=(ORB_ECAPACITY,))
        return n.value

    def read_corners(self, dst):
        """orb.rs:559: fills a CORNER_DTYPE array (the reference's &mut [CornerData])."""
        assert dst.dtype == CORNER_DTYPE and dst.flags.c_contiguous
        self._check(self._lib.orb_read_corners(self._handle(), _ptr(dst), dst.size))
        return dst

    def read_descriptors(self, dst):
        """orb.rs:563: fills a DESCRIPTOR_DTYPE (or uint8 (n,32) / uint32 (n,8)) array."""
        assert dst.flags.c_contiguous and dst.nbytes % 32 == 0
        self._check(self._lib.orb_read_descriptors(self._handle(), _ptr(dst), dst.nbytes // 32))
        return dst

    # ---- conveniences over the six methods -------------------------------------------------
    def extract(self, rgba):
        """One frame in -> (total, corners[stored], descriptors u32 (stored, 8))."""
        self.write_input_image(rgba)
        total = self.extract_corners()
        n = min(total, self.config.max_features)
        corners = self.read_corners(np.zeros(n, dtype=CORNER_DTYPE))
        desc = self.read_descriptors(np.zeros((n, 8), dtype=np.uint32))
        return total, corners, desc

    # ---- batched mode -----------------------------------------------------------------------
    def extract_batch_device(self, frames_dev_ptr, n_frames, stream=None):
        self._check(self._lib.orb_extract_batch_device(self._handle(), ctypes.c_void_p(frames_dev_ptr), n_frames,
                                                       ctypes.c_void_p(stream) if stream else None))

    def extract_batch_host(self, frames):
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        self._check(self._lib.orb_extract_batch_host(self._handle(), _ptr(a), a.shape[0]))

    def extract_batch_pinned(self, frames, n_frames=None):
        """orb_extract_batch_pinned: `frames` is a numpy view of PINNED memory (PinnedArray.array); asynchronous."""
        a = np.asarray(frames)
        assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
        self._check(self._lib.orb_extract_batch_pinned(self._handle(), ctypes.c_void_p(a.ctypes.data),
                                                       a.shape[0] if n_frames is None else n_frames))

    def upload_sync(self):
        self._check(self._lib.orb_upload_sync(self._handle()))

    def batch_sync(self):
        self._check(self._lib.orb_batch_sync(self._handle()))

    def batch_counts(self, n_frames):
        out = np.zeros(n_frames, dtype=np.uint32)
        self._check(self._lib.orb_batch_counts(self._handle(), _ptr(out), n_frames))
        return out

    def batch_read(self, frame, n):
        corners = np.zeros(n, dtype=CORNER_DTYPE)
        desc = np.zeros((n, 8), dtype=np.uint32)
        self._check(self._lib.orb_batch_read(self._handle(), frame, _ptr(corners), _ptr(desc), n))
        return corners, desc

    def batch_read_all(self, n_frames, out=None, stream=None, sync=True):
        """Bulk read-back of the last batch (orb_batch_read_all): returns a `HostBatch` whose arrays live in pinned host
        memory (reused when `out` is passed).  The stored records of all frames are packed back to back in frame
        order; frame f owns records [offsets[f], offsets[f+1])."""
        cap = self.config.max_features
        hb = out if out is not None else HostBatch(n_frames, n_frames * cap)
        assert hb.n_frames >= n_frames
        self._check(self._lib.orb_batch_read_all(self._handle(), n_frames, hb.counts.ctypes.data, hb.offsets.ctypes.data,
                                                 hb.corners.ctypes.data, hb.descriptors.ctypes.data, hb.capacity,
                                                 ctypes.c_void_p(stream) if stream else None))
        if sync:
            if stream:
                self.stream_sync(stream)
            else:
                self.batch_sync()
        return hb

    def batch_pack(self, n_frames, stream=None):
        """Step 1 of the streaming read-back (orb_batch_pack): pack the last batch of the selected output set on the device."""
        self._check(self._lib.orb_batch_pack(self._handle(), n_frames, ctypes.c_void_p(stream) if stream else None))

    def batch_fetch(self, out_set, out, stream=None):
        """Step 2 (orb_batch_fetch): waits for that set's pack, fills out.counts / out.offsets and enqueues the exact-size
        copies of the records into the pinned HostBatch `out` on `stream`; returns the total record count."""
        self._check(self._lib.orb_batch_fetch(self._handle(), out_set, out.counts.ctypes.data, out.offsets.ctypes.data,
                                              out.corners.ctypes.data, out.descriptors.ctypes.data, out.capacity,
                                              ctypes.c_void_p(stream) if stream else None))

    def batch_pack_transport(self, out_set, n_frames, dst_dev_ptr, capacity_records, offsets_dev_ptr=None, stream=None):
        """orb_batch_pack_transport: the stored records of output set `out_set` as 40-byte transport records in device
        memory, enqueued on `stream` (the caller orders it behind the batch)."""
        self._check(self._lib.orb_batch_pack_transport(self._handle(), out_set, n_frames, ctypes.c_void_p(dst_dev_ptr),
                                                       capacity_records, ctypes.c_void_p(offsets_dev_ptr) if offsets_dev_ptr else None,
                                                       ctypes.c_void_p(stream) if stream else None))

    def unpack_transport(self, src_dev_ptr, src_first, count, dst_first, corners_dev_ptr, desc_dev_ptr, stream=None):
        """orb_unpack_transport: runs of transport records -> CornerData / CornerDescriptor arrays on this device."""
        a = [np.ascontiguousarray(v, dtype=np.uint64) for v in (src_first, count, dst_first)]
        assert a[0].shape == a[1].shape == a[2].shape and a[0].ndim == 1
        self._check(self._lib.orb_unpack_transport(self._handle(), ctypes.c_void_p(src_dev_ptr), a[0].shape[0], _ptr(a[0]), _ptr(a[1]),
                                                   _ptr(a[2]), ctypes.c_void_p(corners_dev_ptr), ctypes.c_void_p(desc_dev_ptr),
                                                   ctypes.c_void_p(stream) if stream else None))

    def stream_sync(self, stream=None):
        self._check(self._lib.orb_stream_sync(self._handle(), ctypes.c_void_p(stream) if stream else None))

    def match_consecutive(self, n_frames, stream=None):
        """Hamming-match frame f against f+1 for the first n_frames of the last batch (not in the reference)."""
        self._check(self._lib.orb_match_consecutive(self._handle(), n_frames, ctypes.c_void_p(stream) if stream else None))

    def match_read(self, frame, n):
        out = np.zeros(n, dtype=MATCH_DTYPE)
        self._check(self._lib.orb_match_read(self._handle(), frame, _ptr(out), n))
        return out

    def verify_consecutive(self, n_frames, hypotheses=0, max_distance=0, ratio=0.0, inlier_px=0.0, seed=0, stream=None, reserved=(0, 0, 0)):
        """Geometric verification of the last match_consecutive (not in the reference): per pair
        (f, f+1), f < n_frames - 1, a RANSAC fit of a homography over `hypotheses` minimal samples (0: 512) of the candidates --
        matches with distance <= max_distance (0: 64) and distance < ratio * second (0: 0.8) -- a least-squares refit over the
        winner's inliers (transfer error below inlier_px level-0 pixels, 0: 3.0) and an inlier byte per query.  Asynchronous on
        `stream` (None: the stream of the program's last batched call, match or verification, as the matcher chooses); raises OrbError(ORB_ESTATE) without a match of the current batch and output set."""
        prm = _VerifyParams(hypotheses, max_distance, float(np.float32(ratio)), float(np.float32(inlier_px)), seed & 0xFFFFFFFF,
                            (ctypes.c_uint32 * 3)(*reserved))
        self._check(self._lib.orb_verify_consecutive(self._handle(), n_frames, ctypes.byref(prm),
                                                     ctypes.c_void_p(stream) if stream else None))

    def verify_read(self, pair, n):
        """(record of VERIFY_MODEL_DTYPE, uint8[min(n, max_features)] inlier bytes of pair's queries) -- synchronises.  The record's
        h maps level-0 keypoint coordinates of frame `pair` to frame `pair` + 1 (row-major; literal mode: the mirrored y of the
        keypoints)."""
        rec = np.zeros((), dtype=VERIFY_MODEL_DTYPE)
        mask = np.zeros(min(n, self.config.max_features), dtype=np.uint8)
        self._check(self._lib.orb_verify_read(self._handle(), pair, _ptr(rec), _ptr(mask) if len(mask) else None, len(mask)))
        return rec, mask

    def verify_epipolar(self, n_frames, hypotheses=0, max_distance=0, ratio=0.0, inlier_px=0.0, seed=0, stream=None, reserved=(0, 0, 0)):
        """Epipolar verification of the last match_consecutive (not in the reference): the
        candidates of verify_consecutive, a RANSAC fit of a fundamental matrix over `hypotheses` minimal eight-point samples (0: 512),
        a least-squares refit over the winner's inliers (Sampson distance below inlier_px level-0 pixels, 0: 3.0) and an inlier byte
        per query.  Results of its own: verify_consecutive's stay as they are.  Asynchronous on `stream` as verify_consecutive."""
        prm = _VerifyParams(hypotheses, max_distance, float(np.float32(ratio)), float(np.float32(inlier_px)), seed & 0xFFFFFFFF,
                            (ctypes.c_uint32 * 3)(*reserved))
        self._check(self._lib.orb_verify_epipolar(self._handle(), n_frames, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def verify_epipolar_read(self, pair, n):
        """(record of VERIFY_MODEL_DTYPE, uint8[min(n, max_features)] inlier bytes of pair's queries) of the last verify_epipolar --
        synchronises.  The record's h is F (row-major, x2^T F x1 = 0 for level-0 keypoint coordinates x1 of frame `pair` and x2 of
        frame `pair` + 1), divided by its first entry of largest magnitude."""
        rec = np.zeros((), dtype=VERIFY_MODEL_DTYPE)
        mask = np.zeros(min(n, self.config.max_features), dtype=np.uint8)
        self._check(self._lib.orb_verify_epipolar_read(self._handle(), pair, _ptr(rec), _ptr(mask) if len(mask) else None, len(mask)))
        return rec, mask

    def match_guided(self, n_frames, source=ORB_GUIDE_VERIFIED, radius_px=0.0, octave_window=0, scale_radius=False, models=None,
                     stream=None, flags=0, reserved=(0, 0, 0, 0)):
        """Guided matching of the last batch (not in the reference): per pair (f, f+1),
        f < n_frames - 1, every keypoint of f is sent through the pair's 3 x 3 model -- the last verify_consecutive's h
        (ORB_GUIDE_VERIFIED, pairs with status OK / MINIMAL only), the unit matrix (ORB_GUIDE_IDENTITY) or models[f]
        (ORB_GUIDE_HOST: (n_frames - 1) x 9 or x 3 x 3 float32, read during the call) -- and matched against the keypoints of f+1
        within radius_px level-0 pixels of the prediction (0: 16; times 2^octave with scale_radius) and, with octave_window n > 0,
        |octave difference| < n.  Asynchronous on `stream` (None: the stream of the program's last batched call, match or
        verification, as the matcher chooses).  `flags` and `reserved` are OR'ed / passed into OrbGuideParams as they are."""
        prm = _GuideParams(source, float(np.float32(radius_px)), octave_window, (ORB_GUIDE_SCALE_RADIUS if scale_radius else 0) | flags,
                           (ctypes.c_uint32 * 4)(*reserved))
        m = None
        if models is not None:
            m = np.ascontiguousarray(models, dtype=np.float32)
            if source == ORB_GUIDE_HOST and m.size < (n_frames - 1) * 9:
                raise ValueError("models: need (n_frames - 1) x 9 floats, got %d" % m.size)
        self._check(self._lib.orb_match_guided(self._handle(), n_frames, ctypes.byref(prm), _ptr(m) if m is not None else None,
                                               ctypes.c_void_p(stream) if stream else None))

    def match_guided_read(self, frame, n):
        """MATCH_DTYPE records of the queries of `frame` (the first min(n, max_features)) of the last match_guided -- synchronises."""
        out = np.zeros(min(n, self.config.max_features), dtype=MATCH_DTYPE)
        self._check(self._lib.orb_match_guided_read(self._handle(), frame, _ptr(out) if len(out) else None, len(out)))
        return out

    def match_epipolar(self, n_frames, source=ORB_BAND_VERIFIED, models=None, band_px=0.0, radius_px=0.0, octave_window=0, scale=False,
                       stream=None, flags=0, reserved=(0, 0, 0)):
        """Epipolar-band guided matching of the last batch (not in the reference): per pair
        (f, f+1), f < n_frames - 1, every keypoint of f is sent to its epipolar line in f+1 by the pair's fundamental matrix -- the
        last verify_epipolar's h (ORB_BAND_VERIFIED, pairs with status OK / MINIMAL only) or models[f] (ORB_BAND_HOST:
        (n_frames - 1) x 9 or x 3 x 3 float32, x2^T F x1 = 0, read during the call) -- and matched against the keypoints of f+1
        within band_px level-0 pixels of that line (0: 2.0), inside a window of radius_px around the keypoint's own position
        (0: none) and, with octave_window n > 0, |octave difference| < n; `scale` multiplies band_px and radius_px by 2^octave of
        the query.  Asynchronous on `stream` (None: as match_guided chooses).  `flags` and `reserved` are OR'ed / passed into
        OrbBandParams as they are."""
        prm = _BandParams(source, float(np.float32(band_px)), float(np.float32(radius_px)), octave_window,
                          (ORB_BAND_SCALE if scale else 0) | flags, (ctypes.c_uint32 * 3)(*reserved))
        m = None
        if models is not None:
            m = np.ascontiguousarray(models, dtype=np.float32)
            if source == ORB_BAND_HOST and m.size < (n_frames - 1) * 9:
                raise ValueError("models: need (n_frames - 1) x 9 floats, got %d" % m.size)
        self._check(self._lib.orb_match_epipolar(self._handle(), n_frames, ctypes.byref(prm), _ptr(m) if m is not None else None,
                                                 ctypes.c_void_p(stream) if stream else None))

    def match_epipolar_read(self, frame, n):
        """MATCH_DTYPE records of the queries of `frame` (the first min(n, max_features)) of the last match_epipolar -- synchronises."""
        out = np.zeros(min(n, self.config.max_features), dtype=MATCH_DTYPE)
        self._check(self._lib.orb_match_epipolar_read(self._handle(), frame, _ptr(out) if len(out) else None, len(out)))
        return out

    def pose_consecutive(self, n_frames, fx, fy, cx, cy, max_reproj_px=0.0, max_cos_parallax=0.0, min_good=0, ambiguity_permille=0,
                         stream=None):
        """Relative pose and triangulation of the last batch (not in the reference): per pair
        (f, f+1), f < n_frames - 1, the last verify_epipolar's F and the pinhole intrinsics (fx, fy, cx, cy, in level0_xy
        coordinates) give the essential matrix, its four (R, t) candidates in closed form, and the one under which the most epipolar
        inliers triangulate in front of both cameras within max_reproj_px (0: 2.0) of their frame f+1 keypoint.  max_cos_parallax
        (0: 0.99998), min_good (0: 8) and ambiguity_permille (0: 700) decide the status only.  Asynchronous on `stream` (None: as
        match_guided chooses)."""
        prm = _PoseParams(float(np.float32(fx)), float(np.float32(fy)), float(np.float32(cx)), float(np.float32(cy)),
                          float(np.float32(max_reproj_px)), float(np.float32(max_cos_parallax)), min_good, ambiguity_permille)
        self._check(self._lib.orb_pose_consecutive(self._handle(), n_frames, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def pose_read(self, pair, n=None):
        """(record of POSE_DTYPE, POINT_DTYPE[min(n, max_features)] of pair's queries, in camera f's frame; n None: max_features) of
        the last pose_consecutive -- synchronises.  Queries that are not good points hold zeros."""
        rec = np.zeros((), dtype=POSE_DTYPE)
        pts = np.zeros(self.config.max_features if n is None else min(n, self.config.max_features), dtype=POINT_DTYPE)
        self._check(self._lib.orb_pose_read(self._handle(), pair, _ptr(rec), _ptr(pts) if len(pts) else None, len(pts)))
        return rec, pts

    def trajectory_consecutive(self, n_frames, min_shared=0, scale_tolerance=0.0, consistent_permille=0, flags=0, stream=None,
                               reserved=(0, 0, 0, 0)):
        """Camera path and point map of the last batch in one frame and one unit (not in the reference; DESIGN.md section 20,
        TJ-1..TJ-7): the landmarks that two consecutive pairs of the last pose_consecutive both triangulated give the ratio of the
        pairs' baselines (the lower median of the depth ratios), and the pair poses are chained with it.  A joint holds when it has
        min_shared ratios (0: 8) of which consistent_permille (0: 500) per thousand lie within scale_tolerance (0: 0.1) of the
        median; otherwise a new segment starts.  flags: ORB_TRAJ_NEED_PARALLAX.  Asynchronous on `stream` (None: as match_guided
        chooses)."""
        prm = _TrajectoryParams(min_shared, float(np.float32(scale_tolerance)), consistent_permille, flags, (ctypes.c_uint32 * 4)(*reserved))
        self._check(self._lib.orb_trajectory_consecutive(self._handle(), n_frames, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def trajectory_read(self, frame, n=None):
        """(record of FRAME_POSE_DTYPE, POINT_DTYPE[min(n, max_features)]; n None: max_features) of the last trajectory_consecutive
        -- synchronises.  The record takes the frame of `origin` to camera `frame`'s; the points are those of the pair
        (frame, frame + 1), indexed as pose_read's, in the frame and unit of the origin of frame + 1."""
        rec = np.zeros((), dtype=FRAME_POSE_DTYPE)
        pts = np.zeros(self.config.max_features if n is None else min(n, self.config.max_features), dtype=POINT_DTYPE)
        self._check(self._lib.orb_trajectory_read(self._handle(), frame, _ptr(rec), _ptr(pts) if len(pts) else None, len(pts)))
        return rec, pts

    def localize_consecutive(self, n_frames, fx, fy, cx, cy, max_reproj_px=0.0, hypotheses=0, max_distance=0, ratio=0.0, seed=0,
                             stream=None, reserved=(0, 0, 0, 0, 0, 0, 0)):
        """Absolute pose of camera f + 1 relative to camera f from the map points of the pair before (not in the reference; DESIGN.md
        section 21, LO-1..LO-7): per pair (f, f+1), 1 <= f < n_frames - 1, the GOOD points of pair f - 1 in the last pose_consecutive,
        carried by the matcher's records to a keypoint of frame f + 1 (the second hop filtered by max_distance (0: 64) and ratio
        (0: 0.8)), give 3D-2D correspondences; a RANSAC over `hypotheses` (0: 512) six-point DLT samples within max_reproj_px
        (0: 2.0) and four Gauss-Newton steps on the winner's inliers give R and a metric t in units of pair f - 1's baseline.  The
        intrinsics are those given to pose_consecutive.  Asynchronous on `stream` (None: as match_guided chooses)."""
        prm = _LocalizeParams(float(np.float32(fx)), float(np.float32(fy)), float(np.float32(cx)), float(np.float32(cy)),
                              float(np.float32(max_reproj_px)), hypotheses, max_distance, float(np.float32(ratio)), seed & 0xFFFFFFFF,
                              (ctypes.c_uint32 * 7)(*reserved))
        self._check(self._lib.orb_localize_consecutive(self._handle(), n_frames, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def localize_read(self, pair, n=None):
        """(record of FIX_DTYPE, uint8[min(n, max_features)]: the inlier bytes of frame pair - 1's slots; n None: max_features) of the
        last localize_consecutive -- synchronises."""
        rec = np.zeros((), dtype=FIX_DTYPE)
        mask = np.zeros(self.config.max_features if n is None else min(n, self.config.max_features), dtype=np.uint8)
        self._check(self._lib.orb_localize_read(self._handle(), pair, _ptr(rec), _ptr(mask) if len(mask) else None, len(mask)))
        return rec, mask

    def landmarks_consecutive(self, n_frames, fx, fy, cx, cy, max_reproj_px=0.0, min_views=0, stream=None, reserved=(0, 0)):
        """One multi-view map point per landmark (not in the reference): the GOOD points of the last
        pose_consecutive chained by the matcher's records across the consecutive pairs of one segment of the last
        trajectory_consecutive; every chain's start is a landmark, the point nearest to the rays of all its views under the frame
        poses, GOOD when it has min_views (0: 2) views and all reproject within max_reproj_px (0: 2.0).  The intrinsics are those
        given to pose_consecutive.  Asynchronous on `stream` (None: as match_guided chooses)."""
        prm = _LandmarkParams(float(np.float32(fx)), float(np.float32(fy)), float(np.float32(cx)), float(np.float32(cy)),
                              float(np.float32(max_reproj_px)), min_views, (ctypes.c_uint32 * 2)(*reserved))
        self._check(self._lib.orb_landmarks_consecutive(self._handle(), n_frames, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def landmarks_read(self, pair, n=None):
        """(row of LANDMARK_ROW_DTYPE, LANDMARK_DTYPE[min(n, max_features)]: the records at pair `pair`'s slots; n None: max_features)
        of the last landmarks_consecutive -- synchronises."""
        row = np.zeros((), dtype=LANDMARK_ROW_DTYPE)
        lm = np.zeros(self.config.max_features if n is None else min(n, self.config.max_features), dtype=LANDMARK_DTYPE)
        self._check(self._lib.orb_landmarks_read(self._handle(), pair, _ptr(row), _ptr(lm) if len(lm) else None, len(lm)))
        return row, lm

    def bridge_consecutive(self, n_frames, fx, fy, cx, cy, max_reproj_px=0.0, hypotheses=0, max_distance=0, ratio=0.0, seed=0, max_hops=0,
                           window=0, min_shared=0, scale_tolerance=0.0, consistent_permille=0, stream=None, reserved=(0, 0)):
        """A trajectory carried across LOST frames (not in the reference): for every LOST frame of
        the last trajectory_consecutive, the GOOD landmarks of the last landmarks_consecutive that end in the frame before the gap
        are followed through the matcher's records into it and give its pose by localize_consecutive's RANSAC; a segment that
        starts behind it is measured against the old one by the lower median of depth ratios.  Every frame gets a pose in the
        frame and unit of its root.  Zero parameters are the defaults; asynchronous on `stream`."""
        prm = _BridgeParams(float(np.float32(fx)), float(np.float32(fy)), float(np.float32(cx)), float(np.float32(cy)),
                            float(np.float32(max_reproj_px)), hypotheses, max_distance, float(np.float32(ratio)), seed & 0xFFFFFFFF, max_hops,
                            window, min_shared, float(np.float32(scale_tolerance)), consistent_permille, (ctypes.c_uint32 * 2)(*reserved))
        self._check(self._lib.orb_bridge_consecutive(self._handle(), n_frames, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def bridge_read(self, frame, n=None):
        """(record of BRIDGE_POSE_DTYPE, uint8[min(n, max_features)]: the inlier bytes of frame `frame`'s keypoint slots; n None:
        max_features) of the last bridge_consecutive -- synchronises."""
        rec = np.zeros((), dtype=BRIDGE_POSE_DTYPE)
        mask = np.zeros(self.config.max_features if n is None else min(n, self.config.max_features), dtype=np.uint8)
        self._check(self._lib.orb_bridge_read(self._handle(), frame, _ptr(rec), _ptr(mask) if len(mask) else None, len(mask)))
        return rec, mask

    def adjust_consecutive(self, n_frames, fx, fy, cx, cy, max_reproj_px=0.0, rounds=0, stream=None, reserved=(0, 0)):
        """Poses and landmarks refined by reprojection (not in the reference): `rounds` (0: 4;
        1..16) alternations of a Gauss-Newton step on every CHAINED frame of the last trajectory_consecutive over the keypoints
        that GOOD landmarks of the last landmarks_consecutive own, and the point nearest to all rays for every such landmark
        under the new poses; every other frame is held.  A closing pass checks every landmark's views within max_reproj_px
        (0: 2.0).  The intrinsics are those given to pose_consecutive.  Asynchronous on `stream` (None: as match_guided chooses)."""
        prm = _AdjustParams(float(np.float32(fx)), float(np.float32(fy)), float(np.float32(cx)), float(np.float32(cy)),
                            float(np.float32(max_reproj_px)), rounds, (ctypes.c_uint32 * 2)(*reserved))
        self._check(self._lib.orb_adjust_consecutive(self._handle(), n_frames, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def adjust_read(self, frame, n=None):
        """(record of ADJUSTED_POSE_DTYPE, LANDMARK_DTYPE[min(n, max_features)]: the refined records at pair `frame`'s slots, zeros
        for the last frame; n None: max_features) of the last adjust_consecutive -- synchronises."""
        rec = np.zeros((), dtype=ADJUSTED_POSE_DTYPE)
        lm = np.zeros(self.config.max_features if n is None else min(n, self.config.max_features), dtype=LANDMARK_DTYPE)
        self._check(self._lib.orb_adjust_read(self._handle(), frame, _ptr(rec), _ptr(lm) if len(lm) else None, len(lm)))
        return rec, lm

    def place_frames(self, n_frames, db=None, stream=None, bits=0, tables=0, min_gap=0, top=0, min_score=0, min_permille=0, flags=0,
                     reserved=0):
        """Loop candidates of frames 0 .. n_frames - 1 of the last batch (not in the reference):
        a frame's signature is `tables` (0: 8) bitmaps of 2^bits (0: 16) bits over the low bits of its descriptors' 16-bit
        halves, a score the bits two signatures share, and frame f's candidates the entries of `db` (uint8 (n_db, sig_bytes):
        signatures kept from earlier calls with the same bits and tables; None: no database) and the frames g <= f - min_gap
        (0: 32) -- keyframes of the last track_consecutive only with ORB_PLACE_KEYFRAMES -- with score >= min_score (0: 1) and
        1000 score >= min_permille bits_set; the best `top` (0: 4; at most 8) are kept.  Meant for ORB_FLAG_INTENDED programs.
        Asynchronous on `stream` (None: as match_guided chooses); `db` may be reused as soon as the call returns."""
        prm = _PlaceParams(bits, tables, min_gap, top, min_score, min_permille, flags, reserved)
        n_db = 0
        if db is not None:
            db = np.ascontiguousarray(db, dtype=np.uint8)
            if db.ndim != 2:
                raise OrbError(ORB_EINVAL, "place_frames: db must be a (n_db, sig_bytes) array")
            n_db = db.shape[0]
        self._check(self._lib.orb_place_frames(self._handle(), n_frames, ctypes.byref(prm), _ptr(db) if n_db else None, n_db,
                                               ctypes.c_void_p(stream) if stream else None))
        self._place = (n_frames, ((tables or 8) << (bits or 16)) // 8)

    def place_read(self, first, n):
        """PLACE_ROW_DTYPE records of frames first .. first + n - 1 of the last place_frames (clipped to its frames) --
        synchronises."""
        out = np.zeros(max(min(n, getattr(self, "_place", (first + n, 0))[0] - first), 0), dtype=PLACE_ROW_DTYPE)
        self._check(self._lib.orb_place_read(self._handle(), first, _ptr(out) if len(out) else None, len(out)))
        return out

    def place_signature(self, frame):
        """The signature of `frame` as the last place_frames built it, uint8 (sig_bytes,): what a caller keeps and hands back
        as a row of `db` in a later batch -- synchronises."""
        out = np.zeros(getattr(self, "_place", (0, ORB_PLACE_SIG_BYTES_MAX))[1], dtype=np.uint8)
        self._check(self._lib.orb_place_signature(self._handle(), frame, _ptr(out), len(out)))
        return out

    def match_pairs(self, pairs, stream=None):
        """Hamming-match caller-listed frame pairs of the last batch (not in the reference):
        `pairs` is an (n, 2) integer array, a list of (query, target) tuples or a FRAME_PAIR_DTYPE array; row i of the result
        holds match_consecutive's record for every stored keypoint of frame query_i against those of frame target_i.  At most
        ORB_PAIRS_PER_FRAME * max_batch pairs, frames of the last batch, query != target; duplicates, backward and consecutive
        pairs are allowed.  Asynchronous on `stream` (None: as match_guided chooses); `pairs` may be reused as soon as the call
        returns."""
        a = np.asarray(pairs)
        if a.dtype != FRAME_PAIR_DTYPE:
            a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            if len(a) and (a.min() < 0 or a.max() > 0xFFFFFFFF):
                raise OrbError(ORB_EINVAL, "match_pairs: frame indices must be 0 .. 2^32 - 1")
            a = np.ascontiguousarray(a.astype(np.uint32)).view(FRAME_PAIR_DTYPE).reshape(-1)
        a = np.ascontiguousarray(a.reshape(-1))
        self._check(self._lib.orb_match_pairs(self._handle(), _ptr(a) if len(a) else None, len(a), ctypes.c_void_p(stream) if stream else None))

    def match_pairs_read(self, pair, n):
        """MATCH_DTYPE records of the first n queries of pair `pair` of the last match_pairs (its query frame's) -- synchronises."""
        out = np.zeros(min(n, self.config.max_features), dtype=MATCH_DTYPE)
        self._check(self._lib.orb_match_pairs_read(self._handle(), pair, _ptr(out) if len(out) else None, len(out)))
        return out

    def verify_pairs(self, n_pairs, model=ORB_PAIRS_HOMOGRAPHY, hypotheses=0, max_distance=0, ratio=0.0, inlier_px=0.0, seed=0, stream=None,
                     reserved=(0, 0, 0)):
        """Geometric verification of pairs 0 .. n_pairs - 1 of the last match_pairs: model
        ORB_PAIRS_HOMOGRAPHY gives pair i what verify_consecutive gives a consecutive pair (GV-1..GV-7), ORB_PAIRS_EPIPOLAR what
        verify_epipolar gives (EP-1..EP-6), with the list index i as the pair of the draw stream's seed.  Parameters and defaults
        as verify_consecutive.  Asynchronous on `stream` (None: as match_guided chooses); raises OrbError(ORB_ESTATE) without a
        match_pairs of the current batch and output set."""
        prm = _VerifyParams(hypotheses, max_distance, float(np.float32(ratio)), float(np.float32(inlier_px)), seed & 0xFFFFFFFF,
                            (ctypes.c_uint32 * 3)(*reserved))
        self._check(self._lib.orb_verify_pairs(self._handle(), n_pairs, model, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def verify_pairs_read(self, pair, n):
        """(record of VERIFY_MODEL_DTYPE, uint8[min(n, max_features)] inlier bytes of the queries of pair's query frame) of the last
        verify_pairs -- synchronises.  The record's h maps (homography) or relates (F: x2^T F x1 = 0) level-0 keypoint coordinates
        of the pair's query frame to its target frame."""
        rec = np.zeros((), dtype=VERIFY_MODEL_DTYPE)
        mask = np.zeros(min(n, self.config.max_features), dtype=np.uint8)
        self._check(self._lib.orb_verify_pairs_read(self._handle(), pair, _ptr(rec), _ptr(mask) if len(mask) else None, len(mask)))
        return rec, mask

    def loop_pairs(self, n_pairs, fx, fy, cx, cy, max_reproj_px=0.0, hypotheses=0, max_distance=0, ratio=0.0, seed=0, stream=None,
                   reserved=(0,) * 7):
        """The pose of each listed query frame from its target's landmarks (not in the reference; DESIGN.md section 28,
        LC-1..LC-7): row i of the last match_pairs sends the keypoints of entry i's query frame to keypoints of its target frame,
        those are views of GOOD landmarks of the last landmarks_consecutive, and localize_consecutive's RANSAC on the 3D-2D
        correspondences gives the query camera relative to the target camera in the unit of the target's segment, and, composed
        with the target's pose of the last trajectory_consecutive, in that segment's frame.  Zero parameters are the defaults; the
        intrinsics are those given to pose_consecutive.  Asynchronous on `stream` (None: as match_guided chooses)."""
        prm = _LoopParams(float(np.float32(fx)), float(np.float32(fy)), float(np.float32(cx)), float(np.float32(cy)),
                          float(np.float32(max_reproj_px)), hypotheses, max_distance, float(np.float32(ratio)), seed & 0xFFFFFFFF,
                          (ctypes.c_uint32 * 7)(*reserved))
        self._check(self._lib.orb_loop_pairs(self._handle(), n_pairs, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def loop_pairs_read(self, pair, n=None):
        """(record of LOOP_FIX_DTYPE, uint8[min(n, max_features)]: the inlier bytes of the keypoint slots of entry `pair`'s query
        frame; n None: max_features) of the last loop_pairs -- synchronises."""
        rec = np.zeros((), dtype=LOOP_FIX_DTYPE)
        mask = np.zeros(self.config.max_features if n is None else min(n, self.config.max_features), dtype=np.uint8)
        self._check(self._lib.orb_loop_pairs_read(self._handle(), pair, _ptr(rec), _ptr(mask) if len(mask) else None, len(mask)))
        return rec, mask

    def debug_loop_buffer(self):
        """For tests: the device address of the fix records [ORB_PAIRS_PER_FRAME * max_batch] LOOP_FIX_DTYPE that loop_pairs writes
        and loop_pairs_read and graph_pairs read.  The caller orders its own writes."""
        a = ctypes.c_void_p()
        self._check(self._lib.orb_debug_loop_buffer(self._handle(), ctypes.byref(a)))
        return a.value

    def graph_pairs(self, n_pairs, rounds=0, cg_iterations=0, min_inliers=0, loop_weight=0.0, rotation_weight=0.0, flags=0, stream=None,
                    reserved=(0, 0)):
        """Pose-graph correction of every segment of the last trajectory_consecutive from entries 0 .. n_pairs - 1 of the last
        loop_pairs (not in the reference): the segment's cameras are the nodes, the relative
        poses of consecutive cameras the chain edges, the qualifying fixes the loop edges; `rounds` Gauss-Newton rounds, each
        solved by `cg_iterations` preconditioned conjugate-gradient iterations, move every camera but the segment's origin.  Zero
        parameters are the defaults.  Asynchronous on `stream` (None: as match_guided chooses)."""
        prm = _GraphParams(rounds, cg_iterations, min_inliers, float(np.float32(loop_weight)), float(np.float32(rotation_weight)), flags,
                           (ctypes.c_uint32 * 2)(*reserved))
        self._check(self._lib.orb_graph_pairs(self._handle(), n_pairs, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def graph_read(self, frame):
        """The record of GRAPH_POSE_DTYPE of frame `frame` of the last graph_pairs -- synchronises."""
        rec = np.zeros((), dtype=GRAPH_POSE_DTYPE)
        self._check(self._lib.orb_graph_read(self._handle(), frame, _ptr(rec)))
        return rec

    def graph_edges(self, n):
        """GRAPH_EDGE_DTYPE verdicts of entries 0 .. n - 1 of the last graph_pairs -- synchronises."""
        out = np.zeros(n, dtype=GRAPH_EDGE_DTYPE)
        self._check(self._lib.orb_graph_edges(self._handle(), _ptr(out) if n else None, n))
        return out

    def debug_loop_mask_buffer(self):
        """For tests: the device address of the inlier bytes [ORB_PAIRS_PER_FRAME * max_batch][max_features] that loop_pairs writes
        and loop_pairs_read and join_pairs read.  The caller orders its own writes."""
        a = ctypes.c_void_p()
        self._check(self._lib.orb_debug_loop_mask_buffer(self._handle(), ctypes.byref(a)))
        return a.value

    def join_pairs(self, n_pairs, min_inliers=0, min_shared=0, scale_tolerance=0.0, consistent_permille=0, flags=0, stream=None,
                   reserved=(0, 0, 0)):
        """Joins the segments of the last trajectory_consecutive through entries 0 .. n_pairs - 1 of the last loop_pairs (not in the
        reference): an entry whose query and target lie in different segments gives the
        similarity between them, its scale the lower median of the depth ratios of the inlier keypoints that a landmark of each
        segment owns; every segment takes its most consistent entry as its link to an earlier origin, the links are chained and
        every frame is written in its root's frame and unit.  Zero parameters are the defaults.  Asynchronous on `stream` (None:
        as match_guided chooses)."""
        prm = _JoinParams(min_inliers, min_shared, float(np.float32(scale_tolerance)), consistent_permille, flags,
                          (ctypes.c_uint32 * 3)(*reserved))
        self._check(self._lib.orb_join_pairs(self._handle(), n_pairs, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def join_read(self, frame):
        """The record of JOIN_POSE_DTYPE of frame `frame` of the last join_pairs -- synchronises."""
        rec = np.zeros((), dtype=JOIN_POSE_DTYPE)
        self._check(self._lib.orb_join_read(self._handle(), frame, _ptr(rec)))
        return rec

    def join_segments(self, n):
        """JOIN_SEGMENT_DTYPE records of frame slots 0 .. n - 1 of the last join_pairs -- synchronises."""
        out = np.zeros(n, dtype=JOIN_SEGMENT_DTYPE)
        self._check(self._lib.orb_join_segments(self._handle(), _ptr(out) if n else None, n))
        return out

    def join_links(self, n):
        """JOIN_LINK_DTYPE records of entries 0 .. n - 1 of the last join_pairs -- synchronises."""
        out = np.zeros(n, dtype=JOIN_LINK_DTYPE)
        self._check(self._lib.orb_join_links(self._handle(), _ptr(out) if n else None, n))
        return out

    def remap_frames(self, flags=0, stream=None, reserved=(0, 0, 0, 0, 0, 0, 0)):
        """The corrected map in one root frame (not in the reference): every frame's camera, the last
        graph_pairs' where it moved it (ORB_REMAP_GRAPH), composed with its segment's similarity of the last join_pairs
        (ORB_REMAP_JOIN), and every GOOD landmark of the last landmarks_consecutive carried along with the camera of its first view
        and through the similarity.  flags 0: both sources.  Asynchronous on `stream` (None: as match_guided chooses)."""
        prm = _RemapParams(flags, (ctypes.c_uint32 * 7)(*reserved))
        self._check(self._lib.orb_remap_frames(self._handle(), ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def remap_read(self, frame):
        """The record of REMAP_POSE_DTYPE of frame `frame` of the last remap_frames -- synchronises."""
        rec = np.zeros((), dtype=REMAP_POSE_DTYPE)
        self._check(self._lib.orb_remap_read(self._handle(), frame, _ptr(rec)))
        return rec

    def remap_landmarks(self, pair, n=None):
        """(row of REMAP_ROW_DTYPE, LANDMARK_DTYPE[min(n, max_features)]; n None: max_features) of pair `pair` of the last
        remap_frames, indexed as landmarks_read -- synchronises."""
        row = np.zeros((), dtype=REMAP_ROW_DTYPE)
        out = np.zeros(self.config.max_features if n is None else min(n, self.config.max_features), dtype=LANDMARK_DTYPE)
        self._check(self._lib.orb_remap_landmarks(self._handle(), pair, _ptr(row), _ptr(out) if len(out) else None, len(out)))
        return row, out

    def keyframes_reserve(self, slots):
        """Allocates the program's keyframe store of `slots` slots (1 .. ORB_KEYFRAME_SLOTS_MAX; not in the reference; DESIGN.md
        section 32, KF-1): it survives every later batch and stage call.  The same number again does nothing; another raises
        OrbError(ORB_ESTATE)."""
        self._check(self._lib.orb_keyframes_reserve(self._handle(), slots))

    def keyframes_insert(self, entries, stream=None):
        """Fills slots from frames of the last batch (KF-2): `entries` is a list of (frame, slot) or (frame, slot, user0, user1)
        tuples or a KEYFRAME_ENTRY_DTYPE array.  Needs match_consecutive, trajectory_consecutive and landmarks_consecutive of
        the current batch.  Asynchronous on `stream` (None: as match_guided chooses)."""
        a = np.asarray(entries)
        if a.dtype != KEYFRAME_ENTRY_DTYPE:
            rows = [tuple(int(v) for v in e) for e in entries]
            a = np.zeros(len(rows), dtype=KEYFRAME_ENTRY_DTYPE)
            for i, e in enumerate(rows):
                a[i] = (e[0], e[1], tuple(e[2:4]) if len(e) > 2 else (0, 0))
        a = np.ascontiguousarray(a.reshape(-1))
        self._check(self._lib.orb_keyframes_insert(self._handle(), _ptr(a) if len(a) else None, len(a), ctypes.c_void_p(stream) if stream else None))

    def keyframes_read(self, slot, n=None):
        """(header of KEYFRAME_DTYPE, CORNER_DTYPE[n], DESCRIPTOR_DTYPE[n], MAP_POINT_DTYPE[n]) of `slot`; n None: the header's
        keypoints, else min(n, max_features) -- synchronises.  An EMPTY slot reads as zeros."""
        head = np.zeros((), dtype=KEYFRAME_DTYPE)
        self._check(self._lib.orb_keyframes_read(self._handle(), slot, _ptr(head), None, None, None, 0))
        n = int(head["keypoints"]) if n is None else min(n, self.config.max_features)
        corners, desc, points = np.zeros(n, dtype=CORNER_DTYPE), np.zeros(n, dtype=DESCRIPTOR_DTYPE), np.zeros(n, dtype=MAP_POINT_DTYPE)
        if n:
            self._check(self._lib.orb_keyframes_read(self._handle(), slot, None, _ptr(corners), _ptr(desc), _ptr(points), n))
        return head, corners, desc, points

    def keyframes_load(self, slot, header, corners, descriptors, points):
        """Writes `slot` from the host, as keyframes_read gave it in this program or another of the same configuration (KF-5);
        len(corners) == len(descriptors) == len(points) == header["keypoints"]."""
        head = np.ascontiguousarray(np.asarray(header, dtype=KEYFRAME_DTYPE).reshape(()))
        c = np.ascontiguousarray(corners, dtype=CORNER_DTYPE)
        d = np.ascontiguousarray(descriptors, dtype=DESCRIPTOR_DTYPE)
        x = np.ascontiguousarray(points, dtype=MAP_POINT_DTYPE)
        if not len(c) == len(d) == len(x):
            raise OrbError(ORB_EINVAL, "keyframes_load: the three arrays must have one length")
        n = len(c)
        self._check(self._lib.orb_keyframes_load(self._handle(), slot, _ptr(head), _ptr(c) if n else None, _ptr(d) if n else None,
                                                 _ptr(x) if n else None, n))

    def keyframes_remove(self, slot):
        """Empties `slot`."""
        self._check(self._lib.orb_keyframes_remove(self._handle(), slot))

    def match_keyframes(self, pairs, stream=None):
        """Hamming-match frames of the last batch against slots of the store (KF-3): `pairs` is an (n, 2) integer array, a list
        of (query, slot) tuples or a KEYFRAME_PAIR_DTYPE array; row i holds match_pairs' record for every stored keypoint of
        frame query_i against the keypoints of slot_i.  Asynchronous on `stream` (None: as match_guided chooses)."""
        a = np.asarray(pairs)
        if a.dtype != KEYFRAME_PAIR_DTYPE:
            a = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            if len(a) and (a.min() < 0 or a.max() > 0xFFFFFFFF):
                raise OrbError(ORB_EINVAL, "match_keyframes: indices must be 0 .. 2^32 - 1")
            a = np.ascontiguousarray(a.astype(np.uint32)).view(KEYFRAME_PAIR_DTYPE).reshape(-1)
        a = np.ascontiguousarray(a.reshape(-1))
        self._check(self._lib.orb_match_keyframes(self._handle(), _ptr(a) if len(a) else None, len(a), ctypes.c_void_p(stream) if stream else None))

    def match_keyframes_read(self, entry, n):
        """MATCH_DTYPE records of the first n queries of entry `entry` of the last match_keyframes -- synchronises."""
        out = np.zeros(min(n, self.config.max_features), dtype=MATCH_DTYPE)
        self._check(self._lib.orb_match_keyframes_read(self._handle(), entry, _ptr(out) if len(out) else None, len(out)))
        return out

    def localize_keyframes(self, n, fx, fy, cx, cy, max_reproj_px=0.0, hypotheses=0, max_distance=0, ratio=0.0, seed=0, stream=None,
                           reserved=(0,) * 7):
        """The pose of each listed query frame from its slot's points (KF-4): loop_pairs' RANSAC, refit and compose on entries
        0 .. n - 1 of the last match_keyframes, with the same parameters and draw stream.  Raises OrbError(ORB_ESTATE) when the
        store has changed since that call.  Asynchronous on `stream` (None: as match_guided chooses)."""
        prm = _LoopParams(float(np.float32(fx)), float(np.float32(fy)), float(np.float32(cx)), float(np.float32(cy)),
                          float(np.float32(max_reproj_px)), hypotheses, max_distance, float(np.float32(ratio)), seed & 0xFFFFFFFF,
                          (ctypes.c_uint32 * 7)(*reserved))
        self._check(self._lib.orb_localize_keyframes(self._handle(), n, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def localize_keyframes_read(self, entry, n=None):
        """(record of KEYFRAME_FIX_DTYPE, uint8[min(n, max_features)]: the inlier bytes of the keypoint slots of entry `entry`'s
        query frame; n None: max_features) of the last localize_keyframes -- synchronises."""
        rec = np.zeros((), dtype=KEYFRAME_FIX_DTYPE)
        mask = np.zeros(self.config.max_features if n is None else min(n, self.config.max_features), dtype=np.uint8)
        self._check(self._lib.orb_localize_keyframes_read(self._handle(), entry, _ptr(rec), _ptr(mask) if len(mask) else None, len(mask)))
        return rec, mask

    def anchor_frames(self, n, min_inliers=0, min_shared=0, scale_tolerance=0.0, consistent_permille=0, flags=0, stream=None,
                      reserved=(0, 0, 0)):
        """The last batch's trajectory and landmarks in the stored map (not in the reference):
        entries 0 .. n - 1 of the last localize_keyframes give the similarity between the query's segment and the keyframe's, its
        scale the lower median of the depth ratios of the inlier keypoints that a stored point and a landmark of the batch both
        own; every segment takes its most consistent entry and hangs directly under that keyframe's segment, and its frames and
        GOOD landmarks are written in the map's frame and unit.  Zero parameters are the defaults.  Raises OrbError(ORB_ESTATE)
        when the store has changed since the last match_keyframes.  Asynchronous on `stream` (None: as match_guided chooses)."""
        prm = _AnchorParams(min_inliers, min_shared, float(np.float32(scale_tolerance)), consistent_permille, flags,
                            (ctypes.c_uint32 * 3)(*reserved))
        self._check(self._lib.orb_anchor_frames(self._handle(), n, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))

    def anchor_read(self, frame):
        """The record of ANCHOR_POSE_DTYPE of frame `frame` of the last anchor_frames -- synchronises."""
        rec = np.zeros((), dtype=ANCHOR_POSE_DTYPE)
        self._check(self._lib.orb_anchor_read(self._handle(), frame, _ptr(rec)))
        return rec

    def anchor_segments(self, n):
        """ANCHOR_SEGMENT_DTYPE records of frame slots 0 .. n - 1 of the last anchor_frames -- synchronises."""
        out = np.zeros(n, dtype=ANCHOR_SEGMENT_DTYPE)
        self._check(self._lib.orb_anchor_segments(self._handle(), _ptr(out) if n else None, n))
        return out

    def anchor_links(self, n):
        """ANCHOR_LINK_DTYPE records of entries 0 .. n - 1 of the last anchor_frames -- synchronises."""
        out = np.zeros(n, dtype=ANCHOR_LINK_DTYPE)
        self._check(self._lib.orb_anchor_links(self._handle(), _ptr(out) if n else None, n))
        return out

    def anchor_landmarks(self, pair, n=None):
        """(row of ANCHOR_ROW_DTYPE, LANDMARK_DTYPE[min(n, max_features)]; n None: max_features) of pair `pair` of the last
        anchor_frames, indexed as landmarks_read -- synchronises."""
        row = np.zeros((), dtype=ANCHOR_ROW_DTYPE)
        out = np.zeros(self.config.max_features if n is None else min(n, self.config.max_features), dtype=LANDMARK_DTYPE)
        self._check(self._lib.orb_anchor_landmarks(self._handle(), pair, _ptr(row), _ptr(out) if len(out) else None, len(out)))
        return row, out

    def debug_keyframe_buffers(self):
        """For tests: the device addresses (rows, fixes, inlier bytes) of what match_keyframes and localize_keyframes write --
        [ORB_PAIRS_PER_FRAME * max_batch][max_features] MATCH_DTYPE, [ORB_PAIRS_PER_FRAME * max_batch] KEYFRAME_FIX_DTYPE and
        [ORB_PAIRS_PER_FRAME * max_batch][max_features] bytes -- and anchor_frames reads.  The caller orders its own writes."""
        r, f, m = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.orb_debug_keyframe_buffers(self._handle(), ctypes.byref(r), ctypes.byref(f), ctypes.byref(m)))
        return r.value, f.value, m.value

    def track_consecutive(self, n_frames, source=ORB_TRACK_VERIFIED, max_distance=0, ratio=0.0, min_gap=0, max_gap=0, keep_permille=0,
                          min_shared=0, stream=None, reserved=0):
        """Feature tracks and keyframes of the last batch (not in the reference): the pairs
        (f, f + 1), f < n_frames - 1, are linked by the last verify_consecutive's inliers (ORB_TRACK_VERIFIED), the last
        match_guided's records (ORB_TRACK_GUIDED) or the last match_consecutive's (ORB_TRACK_MATCHED) -- the latter two through
        the verifier's candidate test with max_distance (0: 64) and ratio (0: 0.8) --, made one-to-one, chained into tracks, and
        keyframes picked with min_gap (0: 1), max_gap (0: none), keep_permille (0: 900) and min_shared.  Asynchronous on `stream`
        (None: the stream of the program's last batched call)."""
        prm = _TrackParams(source, max_distance, float(np.float32(ratio)), min_gap, max_gap, keep_permille, min_shared, reserved)
        self._check(self._lib.orb_track_consecutive(self._handle(), n_frames, ctypes.byref(prm), ctypes.c_void_p(stream) if stream else None))
        self._track_n = n_frames

    def track_read(self, frame, n):
        """TRACK_DTYPE entries of the keypoints of `frame` (the first min(n, max_features)) of the last track_consecutive --
        synchronises."""
        out = np.zeros(min(n, self.config.max_features), dtype=TRACK_DTYPE)
        self._check(self._lib.orb_track_read(self._handle(), frame, _ptr(out) if len(out) else None, len(out)))
        return out

    def track_frames(self, n):
        """TRACK_FRAME_DTYPE records of the first n frames of the last track_consecutive (at most its n_frames) -- synchronises."""
        out = np.zeros(min(n, getattr(self, "_track_n", n)), dtype=TRACK_FRAME_DTYPE)
        self._check(self._lib.orb_track_frames(self._handle(), _ptr(out) if len(out) else None, len(out)))
        return out

    def batch_select_output(self, slot):
        self._check(self._lib.orb_batch_select_output(self._handle(), slot))

    def batch_device_buffers(self):
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.orb_batch_device_buffers(self._handle(), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def debug_pose_buffers(self):
        """For tests: device addresses of (matches [max_batch][max_features] MATCH_DTYPE, poses [max_batch] POSE_DTYPE, points
        [max_batch][max_features] POINT_DTYPE), what trajectory_consecutive reads.  The caller orders its own writes."""
        a, b, c = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.orb_debug_pose_buffers(self._handle(), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def debug_frame_buffer(self):
        """For tests: the device address of the frame records [max_batch] FRAME_POSE_DTYPE that trajectory_consecutive writes and
        trajectory_read, landmarks_consecutive and bridge_consecutive read.  The caller orders its own writes."""
        a = ctypes.c_void_p()
        self._check(self._lib.orb_debug_frame_buffer(self._handle(), ctypes.byref(a)))
        return a.value

    # ---- inspection / measurement -------------------------------------------------------------
    def pipeline(self):
        return self._lib.orb_pipeline(self._handle()).decode()

    def pipeline_note(self):
        """Why the staged kernels were chosen although nobody asked for them ('' otherwise)."""
        return self._lib.orb_pipeline_note(self._handle()).decode()

    def level_size(self, level):
        w, h = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.orb_level_size(self._handle(), level, ctypes.byref(w), ctypes.byref(h)))
        return w.value, h.value

    def read_plane(self, kind, level, frame=0):
        w, h = self.level_size(level)
        out = np.zeros((h, w), dtype=np.uint16)
        self._check(self._lib.orb_debug_read_plane(self._handle(), frame, kind, level, _ptr(out), out.size))
        return out

    def device_f32_to_f16(self, src):
        src = np.ascontiguousarray(src, dtype=np.float32)
        out = np.zeros(src.shape, dtype=np.uint16)
        self._check(self._lib.orb_debug_f32_to_f16(self._handle(), _ptr(src), _ptr(out), src.size))
        return out

    def device_angle_code(self, cy, cx):
        cy = np.ascontiguousarray(cy, dtype=np.float32)
        cx = np.ascontiguousarray(cx, dtype=np.float32)
        out = np.zeros(cy.shape, dtype=np.uint32)
        self._check(self._lib.orb_debug_angle_code(self._handle(), _ptr(cy), _ptr(cx), _ptr(out), cy.size))
        return out

    def rot_table(self):
        """The rotated-pattern table as (int16 array [codes, 64, 4, 2] of byte offsets, pitch)."""
        codes, pitch = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(self._lib.orb_debug_rot_table(self._handle(), None, 0, ctypes.byref(codes), ctypes.byref(pitch)))
        out = np.zeros((codes.value, 64, 4, 2), dtype=np.int16)
        self._check(self._lib.orb_debug_rot_table(self._handle(), _ptr(out), out.size, None, None))
        return out, pitch.value

    def blur_col_table(self, level):
        """k_front's ready-made blur column table of one level, as the device built it -> (entries (BLUR_COL_DTYPE; empty: the level's
        bands build their own), blur_p, blur_q)."""
        fn = self._lib.orb_debug_blur_col_table
        n, p, q = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(fn(self._handle(), level, None, 0, ctypes.byref(n), ctypes.byref(p), ctypes.byref(q)))
        out = np.zeros(n.value, dtype=BLUR_COL_DTYPE)
        if n.value:
            self._check(fn(self._handle(), level, _ptr(out), out.size, None, None, None))
        return out, p.value, q.value

    def profile_enable(self, on=True):
        self._check(self._lib.orb_profile_enable(self._handle(), 1 if on else 0))

    def profile_reset(self):
        self._check(self._lib.orb_profile_reset(self._handle()))

    def profile(self):
        """{kernel name: (total_ms, launches)} for kernels launched since the last reset."""
        out = {}
        for i in range(ORB_KERNEL_COUNT):
            ms, n = ctypes.c_double(), ctypes.c_uint64()
            self._check(self._lib.orb_profile_get(self._handle(), i, ctypes.byref(ms), ctypes.byref(n)))
            if n.value:
                out[self._lib.orb_kernel_name(i).decode()] = (ms.value, n.value)
        return out

    def synth_frames_device(self, n_frames, seed0, flags=SYN_ALL, frames_dev_ptr=None):
        """Generates synthetic frames on the device; returns the device address."""
        out = ctypes.c_void_p()
        self._check(self._lib.orb_synth_frames_device(self._handle(), ctypes.c_void_p(frames_dev_ptr) if frames_dev_ptr else None,
                                                      n_frames, seed0 & 0xFFFFFFFF, flags, ctypes.byref(out)))
        return out.value

    def debug_stamps(self, n_workgroups):
        out = np.zeros((n_workgroups, 6), dtype=np.uint64)
        self._check(self._lib.orb_debug_stamps(self._handle(), _ptr(out), out.size))
        return out

    def copy_to_host(self, dev_ptr, nbytes):
        out = np.zeros(nbytes, dtype=np.uint8)
        self._check(self._lib.orb_copy_to_host(self._handle(), _ptr(out), ctypes.c_void_p(dev_ptr), nbytes))
        return out


class OrbNode:
    """One process, several GPUs of one node (include/tinyorb.h, orb_node_*): one OrbProgram per device, contiguous
    frame shards, collate on the first device over RCCL.  Not in the reference (single wgpu device, orb.rs:47-51)."""

    def __init__(self, config: OrbConfig, devices):
        self.config = config
        self.devices = list(devices)
        self._h = None
        self._lib = None

    def init(self):
        L = load_library()
        c = self.config
        cfg = _Config(_Extent3d(c.image_size.width, c.image_size.height, c.image_size.depth_or_array_layers),
                      c.max_features, c.hierarchy_depth, float(np.float32(c.initial_threshold)))
        opt = _Options(0, c.max_batch, c.flags, c.fast_arc, c.oob_policy, c.sampler_weight_bits, c.fp_contract, c.angle_bins)
        devs = (ctypes.c_int * len(self.devices))(*self.devices)
        h = ctypes.c_void_p()
        rc = L.orb_node_create(devs, len(self.devices), ctypes.byref(cfg), ctypes.byref(opt), ctypes.byref(h))
        if rc != ORB_OK:
            raise OrbError(rc, (L.orb_node_last_error(None) or b"").decode())
        self._h, self._lib = h, L
        return self

    def close(self):
        if self._h is not None:
            self._lib.orb_node_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self if self._h is not None else self.init()

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != ORB_OK:
            raise OrbError(rc, (self._lib.orb_node_last_error(self._h) or b"").decode())

    def device_count(self):
        return self._lib.orb_node_device_count(self._h)

    def program(self, rank):
        """Borrowed OrbProgram of one rank (do not close it)."""
        h = self._lib.orb_node_program(self._h, rank)
        if not h:
            raise OrbError(ORB_EINVAL, "no such rank")
        p = OrbProgram(self.config)
        p._h, p._lib_obj, p._borrowed = ctypes.c_void_p(h), self._lib, True
        return p

    def shard(self, n_frames, rank):
        lo, hi = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.orb_node_shard(self._h, n_frames, rank, ctypes.byref(lo), ctypes.byref(hi)))
        return lo.value, hi.value

    def extract_batch(self, frames_dev_ptrs, n_frames):
        arr = (ctypes.c_void_p * len(frames_dev_ptrs))(*[ctypes.c_void_p(x) for x in frames_dev_ptrs])
        self._check(self._lib.orb_node_extract_batch(self._h, arr, n_frames))

    def extract_batch_host(self, frames):
        a = np.ascontiguousarray(frames, dtype=np.uint8)
        self._check(self._lib.orb_node_extract_batch_host(self._h, _ptr(a), a.shape[0]))

    def collate(self, n_frames):
        """-> counts (n,), offsets (n+1,), device addresses of the packed corners / descriptors on the first device."""
        counts = np.zeros(n_frames, dtype=np.uint32)
        offsets = np.zeros(n_frames + 1, dtype=np.uint64)
        c, d = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.orb_node_collate(self._h, _ptr(counts), _ptr(offsets), ctypes.byref(c), ctypes.byref(d)))
        return counts, offsets, c.value, d.value

    def collate_begin(self):
        """Stage 2 of the oldest job that has not begun it: enqueue its exchange (waits only for its counters)."""
        self._check(self._lib.orb_node_collate_begin(self._h))

    def collate_end(self, n_frames):
        """Stage 3 of the oldest job: blocks until its collated result is on the first device; returns like collate()."""
        counts = np.zeros(n_frames, dtype=np.uint32)
        offsets = np.zeros(n_frames + 1, dtype=np.uint64)
        c, d = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.orb_node_collate_end(self._h, _ptr(counts), _ptr(offsets), ctypes.byref(c), ctypes.byref(d)))
        return counts, offsets, c.value, d.value

    def pending(self):
        return self._lib.orb_node_pending(self._h)

    def set_results(self, sharded):
        """Results collated on the first device (False, the default) or left packed on the device that computed them (True)."""
        self._check(self._lib.orb_node_set_results(self._h, 1 if sharded else 0))

    def shard_result(self, rank):
        """Sharded results: (frames, records, device addresses of rank's packed corners / descriptors) of the job ended last."""
        nf, nr, c, d = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.orb_node_shard_result(self._h, rank, ctypes.byref(nf), ctypes.byref(nr), ctypes.byref(c), ctypes.byref(d)))
        return nf.value, nr.value, c.value, d.value

    def exchange_backend(self):
        """'rccl', 'rccl-self' (TINYORB_NODE_LOOPBACK=2), 'copies' (TINYORB_NODE_LOOPBACK=1) or 'none' (one device)."""
        return self._lib.orb_node_exchange_backend(self._h).decode()

    def rccl_pairs(self):
        """ncclSend + ncclRecv pairs this node has enqueued so far."""
        return int(self._lib.orb_node_rccl_pairs(self._h))

    def read_collated(self, total):
        corners = np.zeros(total, dtype=CORNER_DTYPE)
        desc = np.zeros((total, 8), dtype=np.uint32)
        self._check(self._lib.orb_node_read_collated(self._h, _ptr(corners), _ptr(desc), total))
        return corners, desc
