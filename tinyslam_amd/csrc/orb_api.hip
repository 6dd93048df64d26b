// orb_api.hip -- libtinyorb: the C ABI of include/tinyorb.h over the HIP kernels.
//
// Host-side counterpart of src/orb.rs in the reference: OrbProgram::init (orb.rs:107-219) becomes
// orb_program_create (device allocations instead of wgpu textures/buffers/pipelines), and
// extract_corners (orb.rs:469-557) becomes a short sequence of kernel launches on one HIP stream
// instead of 3*D render passes + D+1 compute dispatches + 3 staging copies.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cmath>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <optional>
#include <string>
#include <algorithm>
#include <vector>

#include "../../include/tinyorb.h"
#include "orb_plan.h"
#include "orb_kernels_fused.h"
#include "orb_kernels_brief.h"
#include "orb_kernels_intended.h"
#include "orb_kernels_staged.h"
#include "orb_kernels_collate.h"
#include "orb_kernels_match.h"
#include "orb_kernels_verify.h"
#include "orb_kernels_epipolar.h"
#include "orb_kernels_guide.h"
#include "orb_kernels_band.h"
#include "orb_kernels_pose.h"
#include "orb_kernels_traj.h"
#include "orb_kernels_localize.h"
#include "orb_kernels_landmark.h"
#include "orb_kernels_bridge.h"
#include "orb_kernels_adjust.h"
#include "orb_kernels_place.h"
#include "orb_kernels_pairs.h"
#include "orb_kernels_loop.h"
#include "orb_kernels_graph.h"
#include "orb_kernels_join.h"
#include "orb_kernels_remap.h"
#include "orb_kernels_keyframes.h"
#include "orb_kernels_anchor.h"
#include "orb_kernels_track.h"

using namespace orb;

namespace {

enum KernelId { KID_GRAY = 0, KID_MIP, KID_BLUR, KID_FAST, KID_BRIEF, KID_FUSED_L0, KID_FUSED_LN, KID_SYNTH, KID_BRIEF_ROWS, KID_PREFIX, KID_FRONT_I, KID_SELECT_I, KID_BRIEF_I, KID_MATCH, KID_COMPACT, KID_BRIEF_T, KID_BRIEF_NF, KID_PACK_T, KID_UNPACK_T, KID_BRIEF_ONE, KID_FRONT_I_LN, KID_DESC_EXPAND, KID_VERIFY_GATHER, KID_VERIFY_SCORE, KID_VERIFY_REFINE };
const char* const kKernelNames[ORB_KERNEL_COUNT] = {"k_grayscale", "k_mip",      "k_blur_rows", "k_fast",       "k_brief",
                                                    "k_front_l0",  "k_front_ln", "k_synth",     "k_brief_rows", "k_slot_prefix",
                                                    "k_front_i_l0", "k_select_i", "k_brief_i",   "k_match",      "k_compact",
                                                    "k_brief_t",   "k_brief_nf",  "k_compact_transport", "k_unpack_transport",
                                                    "k_brief_one", "k_front_i_ln", "k_desc_expand", "k_verify_gather",
                                                    "k_verify_score", "k_verify_refine"};

thread_local std::string g_create_error;

// k_front's instances by arithmetic form (orb_front_launch.h: front_form())
hipError_t (*const kFrontLaunch[8])(const FrontLaunch&) = {front_launch_fp0, front_launch_fp1, front_launch_fp2, front_launch_fp3,
                                                           front_launch_fp4, front_launch_fp5, front_launch_fp6, front_launch_fp7};
hipError_t (*const kFrontPairLaunch[8])(const FrontPairLaunch&) = {front_pair_launch_fp0, front_pair_launch_fp1, front_pair_launch_fp2, front_pair_launch_fp3,
                                                                   front_pair_launch_fp4, front_pair_launch_fp5, front_pair_launch_fp6, front_pair_launch_fp7};
hipError_t (*const kFrontSetMaxLds[8])(int) = {front_set_max_lds_fp0, front_set_max_lds_fp1, front_set_max_lds_fp2, front_set_max_lds_fp3,
                                               front_set_max_lds_fp4, front_set_max_lds_fp5, front_set_max_lds_fp6, front_set_max_lds_fp7};

struct ProfSpan {
    int kid;
    hipEvent_t start, stop;
};

}  // namespace

// The stages that run after extraction.  Each owns ONE set of buffers per program, shared by both output sets and by whatever stream
// the caller passes, so a call is ordered (stage_begin) behind the last call of: the stage itself, whose buffers it overwrites; the
// stages whose results it reads, a subset of its row of kStages; and the stages that read what it overwrites, kReaders.of[stage],
// which is that table transposed.
enum StageId { ST_MATCH = 0, ST_VERIFY, ST_EPI, ST_GUIDE, ST_TRACK, ST_BAND, ST_POSE, ST_TRAJ, ST_LOCALIZE, ST_LANDMARK, ST_BRIDGE, ST_ADJUST, ST_GRAPH, ST_JOIN, ST_REMAP, ST_ANCHOR, ST_PLACE, ST_PAIRS, ST_KEYFRAMES, ST_KF_MATCH, ST_KF_LOC, ST_PAIRS_VERIFY, ST_LOOP, ST_COUNT };

// A stage, said once: what messages call it and its read call, and every stage whose results a call of it may read (bits 1 << StageId)
struct StageInfo {
    const char* name;
    const char* read_name;
    uint32_t reads;
};
constexpr StageInfo kStages[ST_COUNT] = {
    {"match_consecutive", "match_read", 0u},
    {"verify_consecutive", "verify_read",
     1u << ST_MATCH},     // d_matches: the gather's candidates
    {"verify_epipolar", "verify_epipolar_read",
     1u << ST_MATCH},     // d_matches: the same gather
    {"match_guided", "match_guided_read",
     1u << ST_VERIFY},    // verify.model (ORB_GUIDE_VERIFIED; waited for whatever the source)
    {"track_consecutive", "track_read",
     1u << ST_MATCH |     // d_matches: the links of MATCHED and VERIFIED
     1u << ST_VERIFY |    // verify.mask (ORB_TRACK_VERIFIED)
     1u << ST_GUIDE},     // guide.match (ORB_TRACK_GUIDED)
    {"match_epipolar", "match_epipolar_read",
     1u << ST_EPI},       // epi.model (ORB_BAND_VERIFIED; waited for whatever the source)
    {"pose_consecutive", "pose_read",
     1u << ST_MATCH |     // d_matches: pairs the inliers
     1u << ST_EPI},       // epi.model, epi.mask
    {"trajectory_consecutive", "trajectory_read",
     1u << ST_MATCH |     // d_matches: pairs the points of two pairs
     1u << ST_POSE},      // d_pose, d_ppoints
    {"localize_consecutive", "localize_read",
     1u << ST_MATCH |     // d_matches: carries a point over two pairs
     1u << ST_POSE},      // d_pose, d_ppoints
    {"landmarks_consecutive", "landmarks_read",
     1u << ST_MATCH |     // d_matches: chains the pairs' points
     1u << ST_POSE |      // d_ppoints
     1u << ST_TRAJ},      // d_jframe
    {"bridge_consecutive", "bridge_read",
     1u << ST_MATCH |     // d_matches: carries a landmark into a LOST frame
     1u << ST_POSE |      // d_ppoints
     1u << ST_TRAJ |      // d_jframe
     1u << ST_LANDMARK},  // d_mland
    {"adjust_consecutive", "adjust_read",
     1u << ST_MATCH |     // d_matches: the views of a landmark
     1u << ST_TRAJ |      // d_jframe
     1u << ST_LANDMARK},  // d_mland
    {"graph_pairs", "graph_read",  // the two refinements side by side: an id carries no order
     1u << ST_TRAJ |      // d_jframe: the nodes and the chain edges
     1u << ST_PAIRS |     // d_plist: q and T of an entry
     1u << ST_LOOP},      // loop.fix: the loop edges
    {"join_pairs", "join_read",
     1u << ST_MATCH |     // d_matches: the owners' walk
     1u << ST_TRAJ |      // d_jframe: the segments and camera q in its own
     1u << ST_LANDMARK |  // d_mland: the two landmarks of a ratio
     1u << ST_PAIRS |     // d_plist, d_prows: q, T and the matched keypoint
     1u << ST_LOOP},      // loop.fix, loop.mask: camera q in the target's segment, the inliers
    {"remap_frames", "remap_read",  // a call waits for the sources its flags name
     1u << ST_TRAJ |      // d_jframe: the cameras and their segments
     1u << ST_LANDMARK |  // d_mland, d_mrow: the records it moves
     1u << ST_GRAPH |     // d_gpose (ORB_REMAP_GRAPH)
     1u << ST_JOIN},      // d_sseg (ORB_REMAP_JOIN)
    {"anchor_frames", "anchor_read",
     1u << ST_MATCH |     // d_matches: the owners' walk
     1u << ST_TRAJ |      // d_jframe: the segments and camera q in its own
     1u << ST_LANDMARK |  // d_mland, d_mrow: the landmark of a ratio, the records it moves
     1u << ST_KF_MATCH |  // d_kmlist, d_kmrows: q, the slot and the matched keypoint
     1u << ST_KF_LOC |    // kfloc.fix, kfloc.mask: camera q in the keyframe's segment, the inliers
     1u << ST_KEYFRAMES}, // d_khead, d_kpoints: the stored points and where the slot came from
    {"place_frames", "place_read",
     1u << ST_TRACK},     // d_tframe: the keyframe column (ORB_PLACE_KEYFRAMES)
    {"match_pairs", "match_pairs_read", 0u},
    {"keyframes_insert", "keyframes_read",  // the store: it outlives the batch (kOutlivesBatch)
     1u << ST_MATCH |     // d_matches: the views of a landmark
     1u << ST_TRAJ |      // d_jframe
     1u << ST_LANDMARK},  // d_mland
    {"match_keyframes", "match_keyframes_read",
     1u << ST_KEYFRAMES}, // d_kcounts, d_kdesc: the slots' rows
    {"localize_keyframes", "localize_keyframes_read",
     1u << ST_KF_MATCH |  // d_kmlist, d_kmrows: the list and its rows
     1u << ST_KEYFRAMES}, // d_khead, d_kpoints
    {"verify_pairs", "verify_pairs_read",
     1u << ST_PAIRS},     // d_plist, d_prows: the list and its rows
    {"loop_pairs", "loop_pairs_read",
     1u << ST_PAIRS |     // d_plist, d_prows: the list and its rows
     1u << ST_MATCH |     // d_matches: the views of a landmark
     1u << ST_TRAJ |      // d_jframe
     1u << ST_LANDMARK},  // d_mland
};
static_assert(kStages[ST_COUNT - 1].name != nullptr, "a row of kStages for every StageId");

// kReaders.of[s]: the stages that read what stage s writes (0: its results are read back by the host only)
struct ReadersOf {
    uint32_t of[ST_COUNT];
};
constexpr ReadersOf readers_of() {
    ReadersOf r{};
    for (int reader = 0; reader < ST_COUNT; reader++)
        for (int s = 0; s < ST_COUNT; s++)
            if (kStages[reader].reads >> s & 1u) r.of[s] |= 1u << reader;
    return r;
}
constexpr ReadersOf kReaders = readers_of();
// The stages whose results do not go stale with the batch: a reader is ordered behind them like behind any other, but asks for the
// store generation it matched against (OrbProgram::kf_gen) where stages_fresh asks for the current batch and output set.
constexpr uint32_t kOutlivesBatch = 1u << ST_KEYFRAMES;

// What the stages' kernels write as words and the reads hand out as structs of tinyorb.h; the parameter blocks
static_assert(sizeof(OrbMatch) == sizeof(MatchRecord), "OrbMatch layout");
static_assert(sizeof(OrbPairModel) == kVerifyModelWords * sizeof(uint32_t) && sizeof(OrbVerifyParams) == 32, "verify layouts");
static_assert(sizeof(OrbGuideParams) == 32 && sizeof(OrbBandParams) == 32, "guided and band layouts");
static_assert(sizeof(OrbTrack) == 16 && sizeof(OrbTrackFrame) == 32 && sizeof(OrbTrackParams) == 32, "track layouts");
static_assert(sizeof(OrbPairPose) == kPoseWords * sizeof(uint32_t) && sizeof(OrbPoint) == sizeof(float4) && sizeof(OrbPoseParams) == 32, "pose layouts");
static_assert(sizeof(OrbFramePose) == kTrajFrameWords * sizeof(uint32_t) && sizeof(OrbTrajectoryParams) == 32, "trajectory layouts");
static_assert(sizeof(OrbFrameFix) == kLocFixWords * sizeof(uint32_t) && sizeof(OrbLocalizeParams) == 64, "localize layouts");
static_assert(sizeof(OrbLandmark) == 32 && sizeof(OrbLandmarkRow) == kLmRowWords * sizeof(uint32_t) && sizeof(OrbLandmarkParams) == 32, "landmark layouts");
static_assert(sizeof(OrbBridgePose) == kBrOutWords * sizeof(uint32_t) && sizeof(OrbBridgeParams) == 64 && kBrFrameWords * sizeof(uint32_t) == sizeof(OrbFramePose),
              "bridge layouts");
static_assert(sizeof(OrbAdjustedPose) == kBaPoseWords * sizeof(uint32_t) && sizeof(OrbAdjustParams) == 32 && kBaFrameWords * sizeof(uint32_t) == sizeof(OrbFramePose),
              "adjust layouts");
static_assert(sizeof(OrbPlaceRow) == kPlaceRowWords * sizeof(uint32_t) && sizeof(OrbPlaceParams) == 32 && sizeof(OrbPlaceCandidate) == 8 &&
                  sizeof(OrbTrackFrame) == kPlaceFrameWords * sizeof(uint32_t) && offsetof(OrbTrackFrame, keyframe) == kPlaceKeyframeWord * sizeof(uint32_t),
              "place layouts");
static_assert(sizeof(OrbFramePair) == 8 && offsetof(OrbFramePair, target) == 4, "pairs layouts");
static_assert(sizeof(OrbLoopFix) == kLcFixWords * sizeof(uint32_t) && sizeof(OrbLoopParams) == 64 && offsetof(OrbLoopFix, pose_r) == 13 * sizeof(uint32_t) &&
                  offsetof(OrbLoopFix, origin) == 25 * sizeof(uint32_t) && kLcFrameWords * sizeof(uint32_t) == sizeof(OrbFramePose) && sizeof(OrbFramePair) == sizeof(uint2),
              "loop layouts");
static_assert(sizeof(OrbKeyframe) == kKfHeadWords * sizeof(uint32_t) && offsetof(OrbKeyframe, keypoints) == 13 * sizeof(uint32_t) &&
                  offsetof(OrbKeyframe, status) == 19 * sizeof(uint32_t) && sizeof(OrbMapPoint) == sizeof(float4) && sizeof(OrbKeyframeEntry) == sizeof(uint4) &&
                  sizeof(OrbKeyframePair) == sizeof(uint2) && sizeof(OrbKeyframeFix) == sizeof(OrbLoopFix) &&
                  offsetof(OrbKeyframeFix, slot) == offsetof(OrbLoopFix, query_origin) && ORB_KEYFRAME_STORED == kKfStored && ORB_KEYFRAME_NOMAP == kKfNomap &&
                  ORB_KEYFRAME_NONE == kLcNone && ORB_KEYFRAME_SLOTS_MAX == ORB_PLACE_DB_MAX,
              "keyframe layouts");
static_assert(sizeof(OrbGraphPose) == kPgPoseWords * sizeof(uint32_t) && sizeof(OrbGraphEdge) == kPgEdgeWords * sizeof(uint32_t) && sizeof(OrbGraphParams) == 32 &&
                  offsetof(OrbGraphPose, status) == 15 * sizeof(uint32_t) && kPgFrameWords * sizeof(uint32_t) == sizeof(OrbFramePose) &&
                  kPgFixWords * sizeof(uint32_t) == sizeof(OrbLoopFix) && offsetof(OrbLoopFix, status) == 30 * sizeof(uint32_t),
              "graph layouts");
static_assert(sizeof(OrbJoinPose) == kSjPoseWords * sizeof(uint32_t) && sizeof(OrbJoinSegment) == kSjSegWords * sizeof(uint32_t) &&
                  sizeof(OrbJoinLink) == kSjLinkWords * sizeof(uint32_t) && sizeof(OrbJoinParams) == 32 && offsetof(OrbJoinPose, root) == 14 * sizeof(uint32_t) &&
                  offsetof(OrbJoinSegment, sigma) == 12 * sizeof(uint32_t) && offsetof(OrbJoinLink, gamma) == 5 * sizeof(uint32_t) &&
                  kSjFrameWords * sizeof(uint32_t) == sizeof(OrbFramePose) && kSjFixWords * sizeof(uint32_t) == sizeof(OrbLoopFix) &&
                  offsetof(OrbLoopFix, inliers) == 28 * sizeof(uint32_t) && offsetof(OrbLoopFix, pose_t) == 22 * sizeof(uint32_t),
              "join layouts");
static_assert(sizeof(OrbRemapPose) == kRmPoseWords * sizeof(uint32_t) && sizeof(OrbRemapRow) == kRmRowWords * sizeof(uint32_t) && sizeof(OrbRemapParams) == 32 &&
                  sizeof(OrbLandmarkRow) == kRmRowWords * sizeof(uint32_t) && offsetof(OrbLandmarkRow, origin) == 3 * sizeof(uint32_t) &&
                  offsetof(OrbLandmark, origin) == 5 * sizeof(uint32_t) && offsetof(OrbLandmark, views) == 4 * sizeof(uint32_t) &&
                  kRmFrameWords * sizeof(uint32_t) == sizeof(OrbFramePose) && kRmGraphWords * sizeof(uint32_t) == sizeof(OrbGraphPose) &&
                  kRmSegWords * sizeof(uint32_t) == sizeof(OrbJoinSegment) && offsetof(OrbJoinSegment, root) == 13 * sizeof(uint32_t) &&
                  kRmFromGraph == ORB_REMAP_FROM_GRAPH && kRmMoved == ORB_REMAP_MOVED && kRmSegLinked == ORB_JOIN_SEGMENT_LINKED &&
                  kRmGraphRefined == ORB_GRAPH_REFINED && kRmGraphFailed == ORB_GRAPH_FAILED && ORB_GRAPH_STALLED == 3u,
              "remap layouts");
static_assert(sizeof(OrbAnchorPose) == kAnPoseWords * sizeof(uint32_t) && sizeof(OrbAnchorSegment) == kAnSegWords * sizeof(uint32_t) &&
                  sizeof(OrbAnchorLink) == kAnLinkWords * sizeof(uint32_t) && sizeof(OrbAnchorRow) == kAnRowWords * sizeof(uint32_t) && sizeof(OrbAnchorParams) == 32 &&
                  offsetof(OrbAnchorPose, slot) == 14 * sizeof(uint32_t) && offsetof(OrbAnchorSegment, gamma) == 12 * sizeof(uint32_t) &&
                  offsetof(OrbAnchorSegment, map_origin) == 15 * sizeof(uint32_t) && offsetof(OrbAnchorSegment, status) == 19 * sizeof(uint32_t) &&
                  offsetof(OrbAnchorLink, gamma) == 5 * sizeof(uint32_t) && offsetof(OrbAnchorRow, origin) == 3 * sizeof(uint32_t) &&
                  kAnFrameWords * sizeof(uint32_t) == sizeof(OrbFramePose) && kAnFixWords * sizeof(uint32_t) == sizeof(OrbKeyframeFix) &&
                  kAnLmRowWords * sizeof(uint32_t) == sizeof(OrbLandmarkRow) && offsetof(OrbKeyframeFix, inliers) == 28 * sizeof(uint32_t) &&
                  offsetof(OrbKeyframeFix, pose_r) == 13 * sizeof(uint32_t) && offsetof(OrbKeyframeFix, status) == 30 * sizeof(uint32_t) &&
                  offsetof(OrbKeyframe, frame) == 15 * sizeof(uint32_t) && offsetof(OrbKeyframe, user) == 17 * sizeof(uint32_t) &&
                  kAnSegAnchored == ORB_ANCHOR_SEGMENT_ANCHORED && kAnSegFree == ORB_ANCHOR_SEGMENT_FREE && kAnAnchored == ORB_ANCHOR_ANCHORED &&
                  kAnRatioSpread == ORB_ANCHOR_LINK_RATIO_SPREAD && kAnNonfinite == ORB_ANCHOR_LINK_NONFINITE && kAnNone == ORB_ANCHOR_NONE,
              "anchor layouts");

// The last call of a stage
struct Stage {
    hipEvent_t done = nullptr;     // behind it (created by the stage's first call)
    hipStream_t stream = nullptr;  // the stream it ran on
    uint64_t seq = 0;              // batch_seq of the batch it read
    uint32_t set = 0;              // output set it read
    uint32_t extent = 0;           // pairs (verify, epi, guide) or frames (match, track) it covered; 0: the stage has never run
};

// The buffers of VerifyArgs, one set per verifier
struct VerifierState {
    float4* rec = nullptr;              // [max_batch][max_features] candidates (u, v, u2, v2)
    uint32_t* cand = nullptr;           // [max_batch][max_features] candidate of each query
    uint32_t* n = nullptr;              // [max_batch] candidates per pair
    unsigned long long* keys = nullptr; // [max_batch][kVerifyMaxHyp]
    uint32_t* model = nullptr;          // [max_batch] OrbPairModel
    uint8_t* mask = nullptr;            // [max_batch][max_features] inlier bytes
    uint32_t* qcount = nullptr;         // orb_verify_pairs only: [pairs] the raw counter of each pair's query frame (k_verify_gather_pairs)
};

// The buffers of a grid search (k_guide_bin and a search kernel), one set for the guided and one for the band call
struct GridSearchState {
    uint4* srec = nullptr;              // [max_batch][max_features] records in cell order (x0, y0, index, octave)
    uint4* sdesc = nullptr;             // [max_batch][max_features][2] descriptors in cell order
    uint32_t* cell = nullptr;           // [max_batch][kGuideMaxCells + 1] cell starts
    MatchRecord* match = nullptr;       // [max_batch][max_features] results
    float* d_model = nullptr;           // [max_batch][9] the caller's models (ORB_GUIDE_HOST, ORB_BAND_HOST)
    float* h_model = nullptr;           // pinned staging of the same
};

// The buffers of LocArgs, one set for the localize and one for the bridge call
struct PnpState {
    uint32_t* fix = nullptr;            // [max_batch][words] the fix of every row
    float4* reca = nullptr;             // [max_batch][max_features] candidates: the landmark in the earlier camera's frame
    float4* recb = nullptr;             // [max_batch][max_features] candidates: the keypoint of the later frame and its ray
    uint32_t* cand = nullptr;           // [max_batch][max_features] candidate of each slot of frame f - 1 (localize only)
    uint32_t* n = nullptr;              // [max_batch] candidates per row
    unsigned long long* keys = nullptr; // [max_batch][kVerifyMaxHyp]
    uint8_t* mask = nullptr;            // [max_batch][max_features] inlier bytes
};

struct OrbProgram {
    OrbConfig cfg{};
    OrbOptions opt{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;  // chunked uploads of orb_extract_batch_host
    hipEvent_t order_event = nullptr;   // orders work on a caller's stream behind the last batch
    std::vector<hipEvent_t> upload_events;  // one per chunk of a chunked upload (reused)
    hipEvent_t upload_done = nullptr;       // behind the last host-to-device copy of the last host batch
    // orb_batch_pack / orb_batch_fetch: packed records of an output set on the device, its counters and offsets in pinned
    // host memory (written by the packing kernel), and the event that says the pack is done
    CornerData* d_pack_c[2] = {nullptr, nullptr};
    CornerDescriptor* d_pack_d[2] = {nullptr, nullptr};
    uint32_t* h_pack_counts[2] = {nullptr, nullptr};
    uint64_t* h_pack_offsets[2] = {nullptr, nullptr};
    hipEvent_t pack_event[2] = {nullptr, nullptr};
    uint32_t pack_n[2] = {0u, 0u};
    uint32_t cur_set = 0;
    ProgramPlan plan;  // which pipeline and its geometry (orb_plan.h): written once by orb_program_create, only read afterwards
    PlanEnv env;       // the create-time environment switches, read once (read_plan_env)
    float threshold = 0.f;
    // opt-in NMS (staged pipeline): provisional detections + score planes
    uint32_t* d_prov_counts = nullptr;
    CornerData* d_prov = nullptr;
    float* d_prov_scores = nullptr;
    float* d_score_planes = nullptr;
    // fused "intended" and arc / NMS pipelines: the tile slots' segments (record + score), the cut
    uint32_t* d_xband_counts = nullptr;  // band-slot counters written by the blur-only k_front launches (unused)
    CornerData* d_iseg = nullptr;
    float* d_iseg_scores = nullptr;
    uint32_t* d_iseg_counts = nullptr;
    uint32_t* d_iseg_before = nullptr;
    unsigned long long* d_thr_key = nullptr;
    uint64_t batch_seq = 0;    // batched calls so far (every call that sets last_batch); a stage records which one it read
    Stage stage[ST_COUNT];     // the last call of each stage after extraction
    // orb_match_consecutive (orb_kernels_match.h)
    MatchRecord* d_matches = nullptr;  // [max_batch][max_features]
    uint8_t* d_desc8 = nullptr;        // [max_batch][max_features][128 or 256]: the descriptors as +-1 in fp4 (k_match_fp4) or +-127 in int8 (k_match_mfma)
    int match_valu = -1;               // which matcher (0 fp4, 1 vector unit: TINYORB_MATCH_VALU=1, 2 int8: TINYORB_MATCH_I8=1); read once
    // orb_verify_consecutive (orb_kernels_verify.h) and orb_verify_epipolar (orb_kernels_epipolar.h): a set of buffers each
    VerifierState verify, epi;
    // orb_match_guided (orb_kernels_guide.h) and orb_match_epipolar (orb_kernels_band.h): a set of buffers each, on the same grid
    GridSearchState guide, band;
    int guide_cell = -1;                  // log2 of the grid's cell size (TINYORB_GUIDE_CELL); -1 until the first call
    // orb_pose_consecutive (orb_kernels_pose.h)
    uint32_t* d_pose = nullptr;           // [max_batch][16] OrbPairPose
    float4* d_ppoints = nullptr;          // [max_batch][max_features] OrbPoint
    uint32_t* d_pcount = nullptr;         // [max_batch][kPoseCounters]
    // orb_trajectory_consecutive (orb_kernels_traj.h)
    uint32_t* d_jframe = nullptr;         // [max_batch][20] OrbFramePose
    float4* d_jmap = nullptr;             // [max_batch][max_features] OrbPoint in the origin's frame and unit
    uint32_t* d_jratio = nullptr;         // [max_batch][max_features] the bits of a joint's ratios
    uint32_t* d_jjoint = nullptr;         // [max_batch][kTrajJointWords]
    // orb_localize_consecutive (orb_kernels_localize.h): fix is [max_batch][20] OrbFrameFix, a row is a pair
    PnpState loc;
    // orb_landmarks_consecutive (orb_kernels_landmark.h)
    float4* d_mland = nullptr;            // [max_batch][max_features][2] OrbLandmark
    uint32_t* d_mrow = nullptr;           // [max_batch][4] OrbLandmarkRow
    uint8_t* d_mpred = nullptr;           // [max_batch][max_features] a live slot of the pair before continues into this slot
    // orb_bridge_consecutive (orb_kernels_bridge.h): fix is [max_batch][kBrFixWords], the fix and join of every frame; a row is a
    // LOST frame, a landmark in its anchor's frame with the keypoint slot; no cand
    PnpState bridge;
    uint32_t* d_bout = nullptr;           // [max_batch][24] OrbBridgePose
    uint32_t* d_bratio = nullptr;         // [max_batch][max_features] the bits of a join's ratios
    // orb_adjust_consecutive (orb_kernels_adjust.h)
    uint32_t* d_apose = nullptr;          // [max_batch][16] OrbAdjustedPose: the current poses during a call
    float4* d_ax = nullptr;               // [max_batch][max_features] the current point of every landmark slot
    uint32_t* d_aowner = nullptr;         // [max_batch][max_features] the owner of every keypoint slot
    float4* d_aland = nullptr;            // [max_batch][max_features][2] OrbLandmark
    // orb_place_frames (orb_kernels_place.h)
    uint32_t* d_psig = nullptr;           // [max_batch][sig_bytes of the last call / 4] signatures (room for ORB_PLACE_SIG_BYTES_MAX each)
    uint32_t* d_pdb = nullptr;            // [n_db][the same] the caller's database (room for ORB_PLACE_DB_MAX of ORB_PLACE_SIG_BYTES_MAX)
    uint32_t* d_ptbits = nullptr;         // [max_batch][16] set bits per table
    uint32_t* d_pscore = nullptr;         // [slices][n_frames][n_db + n_frames] partial scores (room for max_batch x (ORB_PLACE_DB_MAX + max_batch))
    uint32_t* d_prow = nullptr;           // [max_batch] OrbPlaceRow
    hipEvent_t place_copied = nullptr;    // behind the database's copy of the last call
    uint32_t place_sig_bytes = 0;         // of the last call
    // orb_match_pairs and orb_verify_pairs (orb_kernels_pairs.h); P = ORB_PAIRS_PER_FRAME * max_batch
    OrbFramePair* d_plist = nullptr;      // [P] the list of the last orb_match_pairs call
    OrbFramePair* h_plist = nullptr;      // pinned staging of the same
    MatchRecord* d_prows = nullptr;       // [P][max_features] row i: the queries of pair i's query frame
    uint8_t* d_pdesc4 = nullptr;          // [max_batch][max_features][128] the descriptors as +-1 in fp4: the stage's own, apart from d_desc8
    VerifierState pverify;                // orb_verify_pairs: every per-pair dimension is P
    // orb_loop_pairs (orb_kernels_loop.h): fix is [P][32] OrbLoopFix, a row is a list entry, cand the candidate of each slot of its query frame
    PnpState loop;
    uint32_t* d_lowner = nullptr;         // [max_batch][max_features] the owner of every keypoint slot
    // the keyframe store (orb_kernels_keyframes.h); S = kf_slots, the matchers' rows are the batch's max_batch followed by the S slots'
    uint32_t kf_slots = 0;                // of orb_keyframes_reserve (0: none)
    uint64_t kf_gen = 0;                  // store generation: bumped by reserve, insert, load and remove
    uint64_t kf_match_gen = 0;            // the generation the last orb_match_keyframes read
    uint64_t kf_desc4_gen = 0;            // the generation the slots' rows of d_kdesc4 were expanded at (0: never)
    uint64_t kf_match_call = 0;           // orb_match_keyframes calls so far
    uint64_t kf_loc_call = 0;             // kf_match_call of the rows the last orb_localize_keyframes read
    std::vector<uint8_t> kf_filled;       // [S] host mirror: the slot is not EMPTY
    uint32_t* d_khead = nullptr;          // [S] OrbKeyframe
    CornerData* d_kcorners = nullptr;     // [S][max_features]
    CornerDescriptor* d_kdesc = nullptr;  // [max_batch + S][max_features]: rows below max_batch are orb_match_keyframes' copy of the batch's
    uint32_t* d_kcounts = nullptr;        // [max_batch + S] the matchers' counters of those rows
    float4* d_kpoints = nullptr;          // [S][max_features] OrbMapPoint
    uint8_t* d_kdesc4 = nullptr;          // [max_batch + S][max_features][128] the same rows as +-1 in fp4 (orb_match_keyframes, softly)
    uint32_t* d_kowner = nullptr;         // [max_batch][max_features] orb_keyframes_insert's owners (LC-2)
    OrbKeyframeEntry* d_klist = nullptr;  // [max_batch] the list of the last insert
    OrbKeyframeEntry* h_klist = nullptr;  // pinned staging of the same
    // orb_match_keyframes
    OrbKeyframePair* d_kmlist = nullptr;  // [P] the list of the last call
    OrbKeyframePair* h_kmlist = nullptr;  // pinned staging of the same
    MatchRecord* d_kmrows = nullptr;      // [P][max_features] row i: the queries of entry i's query frame
    // orb_localize_keyframes: fix is [P][32] OrbKeyframeFix, as `loop`
    PnpState kfloc;
    // orb_graph_pairs (orb_kernels_graph.h)
    uint32_t* d_gpose = nullptr;          // [max_batch][16] OrbGraphPose; the poses of before a round during a call
    uint32_t* d_gedge = nullptr;          // [P][4] OrbGraphEdge
    uint32_t* d_grow = nullptr;           // [max_batch + 1] CSR row starts: the USED entries at every frame
    uint32_t* d_gcol = nullptr;           // [2 P] their list indices, ascending within a row
    float* d_gwork = nullptr;             // [max_batch][kPgNodeWords] the node words of a segment above kPgLdsNodes free nodes
    uint32_t graph_pairs = 0;             // n_pairs of the last call (its Stage's extent is the frames)
    // orb_join_pairs (orb_kernels_join.h)
    uint32_t* d_sowner = nullptr;         // [max_batch][max_features] the owner of every keypoint slot, of this call's landmarks
    uint32_t* d_sratio = nullptr;         // [P][max_features] the bits of an entry's ratios
    uint32_t* d_slink = nullptr;          // [P][8] OrbJoinLink
    unsigned long long* d_skey = nullptr; // [max_batch] the best entry of every segment
    uint32_t* d_sseg = nullptr;           // [max_batch][16] OrbJoinSegment
    uint32_t* d_spose = nullptr;          // [max_batch][16] OrbJoinPose
    uint32_t join_pairs = 0;              // n_pairs of the last call (its Stage's extent is the frames)
    // orb_remap_frames (orb_kernels_remap.h)
    uint32_t* d_rpose = nullptr;          // [max_batch][16] OrbRemapPose
    uint32_t* d_rrow = nullptr;           // [max_batch][4] OrbRemapRow
    float4* d_rland = nullptr;            // [max_batch][max_features][2] OrbLandmark
    uint32_t remap_pairs = 0;             // the pairs of the last call (its Stage's extent is the frames)
    int remap_slots = 0;                  // slots per thread of k_rm_land: two (TINYORB_REMAP_SLOTS=1: one); 0 until the first call
    // orb_anchor_frames (orb_kernels_anchor.h)
    uint32_t* d_nowner = nullptr;         // [max_batch][max_features] the owner of every keypoint slot, of this call's landmarks
    uint32_t* d_nratio = nullptr;         // [P][max_features] the bits of an entry's ratios
    uint32_t* d_nlink = nullptr;          // [P][8] OrbAnchorLink
    unsigned long long* d_nkey = nullptr; // [max_batch] the best entry of every segment
    uint32_t* d_nseg = nullptr;           // [max_batch][24] OrbAnchorSegment
    uint32_t* d_npose = nullptr;          // [max_batch][16] OrbAnchorPose
    uint32_t* d_nrow = nullptr;           // [max_batch][8] OrbAnchorRow
    float4* d_nland = nullptr;            // [max_batch][max_features][2] OrbLandmark
    uint32_t anchor_entries = 0;          // n of the last call (its Stage's extent is the frames)
    uint32_t anchor_pairs = 0;            // the pairs of the last call
    // orb_track_consecutive (orb_kernels_track.h)
    uint32_t* d_tkeys = nullptr;          // [max_batch][max_features] link keys (global form of k_track_link)
    uint32_t* d_tprev = nullptr;          // [max_batch][max_features]
    uint32_t* d_tnext = nullptr;          // [max_batch][max_features]
    uint4* d_tptr = nullptr;              // [2][max_batch][max_features] pointer-doubling ping-pong
    uint4* d_track = nullptr;             // [max_batch][max_features] OrbTrack
    uint32_t* d_tlinks = nullptr;         // [max_batch] links per pair
    uint32_t* d_tshared = nullptr;        // [max_batch][max_batch] shared(k, f) at [f][k]
    uint32_t* d_tframe = nullptr;         // [max_batch] OrbTrackFrame
    int track_global_keys = -1;           // TINYORB_TRACK_GLOBAL_KEYS; -1 until the first call
    uint32_t* d_prov2_counts = nullptr;
    CornerData* d_prov2 = nullptr;
    float* d_prov2_scores = nullptr;

    uint8_t* d_input = nullptr;  // max_batch frames (single-frame API, host batches, synth)
    // single-frame API: up to two images may be written ahead of extract_corners (orb_write_input_image_pinned uploads frame
    // k + 1 on the copy stream while frame k is extracted); slab 0 is d_input's first frame, slab 1 d_input_alt
    uint8_t* d_input_alt = nullptr;
    uint32_t in_last = 0;                 // slab of the image the last extract_corners worked on (and the next one will, if nothing is pending)
    uint32_t in_pending = 0;              // images written and not yet extracted (0..2)
    uint32_t in_queue[2] = {0u, 0u};      // their slabs, oldest first
    hipEvent_t in_uploaded[2] = {nullptr, nullptr};  // behind the asynchronous upload into the slab
    bool in_async[2] = {false, false};    // the slab's image came through the copy stream: extract_corners orders its kernels behind in_uploaded
    // device-visible addresses of the pinned single-frame staging arrays (resolved once)
    uint32_t* dv_count = nullptr;
    CornerData* dv_corners = nullptr;
    CornerDescriptor* dv_desc = nullptr;
    uint16_t* d_gray = nullptr;  // max_batch x pyr.stride
    uint16_t* d_blur = nullptr;
    uint16_t* d_blur_rowc = nullptr;  // fused path: [max_batch][row_stride] blur row constants (columns < plan.blur_qa)
    uint32_t* d_counts = nullptr;  // currently selected output set (orb_batch_select_output)
    CornerData* d_corners = nullptr;
    CornerDescriptor* d_desc = nullptr;
    uint32_t* out_counts[2] = {nullptr, nullptr};
    CornerData* out_corners[2] = {nullptr, nullptr};
    CornerDescriptor* out_desc[2] = {nullptr, nullptr};
    CornerData* d_seg = nullptr;     // fused path: [max_batch][n_slots][seg_classes][seg_cap] band segments
    uint32_t* d_seg_counts = nullptr;  // [max_batch][n_slots][seg_classes]
    uint32_t* d_seg_before = nullptr;  // [max_batch][seg_classes][n_slots] exclusive prefix of the stored counts
    // [max_batch][brief_mask_words(max_features)] per output set, like the final lists it describes: bit i of word c of a frame = keypoint
    // 64 c + i of the final list is not flat.  k_brief_t writes every word of the frames it runs on, k_brief_nf starts from them.
    uint64_t* d_nf_mask[2] = {nullptr, nullptr};
    uint32_t* d_pattern = nullptr;
    float* d_cos = nullptr;
    float* d_sin = nullptr;
    uint4* d_rot = nullptr;  // the pattern rotated by every angle code (k_rot_table), for k_brief_nf or k_brief_i
    uint4* d_blur_tab = nullptr;  // the plain fused path: k_front's BlurCol table of level 0 (k_blur_col_table), in 16-byte pieces; null when level 0 runs on column tiles
    unsigned long long* d_stamps = nullptr;  // TINYORB_STAMPS=1: phase cycle sums of k_front (2 x 16 slots)

    // host staging of the single-frame API (orb.rs:216-218 staging buffers)
    uint32_t* h_count = nullptr;      // pinned: [0] the raw counter of the last single-frame extract, [kSingleDoneWord] its completion sequence number (own cache line)
    uint32_t* d_single_done = nullptr;  // workgroups of k_brief_one that have finished (the last one publishes the sequence number and clears it)
    hipEvent_t single_done_ev = nullptr;  // blocking-sync event behind k_brief_one (TINYORB_SINGLE_WAIT=block / ORB_FLAG_SINGLE_BLOCKING_WAIT)
    uint32_t single_seq = 0;
    CornerData* h_corners = nullptr;
    CornerDescriptor* h_desc = nullptr;
    bool single_valid = false;

    uint32_t last_batch = 0;  // frames of the last batched call
    hipStream_t last_stream = nullptr;
    bool planes_valid = false;
    uint32_t max_lds = 0;
    uint32_t n_cus = 256;

    bool profiling = false;
    std::vector<ProfSpan> pending;
    std::vector<hipEvent_t> event_pool;
    double prof_ms[ORB_KERNEL_COUNT] = {0};
    uint64_t prof_n[ORB_KERNEL_COUNT] = {0};

    std::string err;
};

namespace {

int fail(OrbProgram* p, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (p)
        p->err = buf;
    else
        g_create_error = buf;
    return code;
}

#define HIP_TRY(p, expr)                                                                                  \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail((p), ORB_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// The stream of a call that takes one: the caller's, else the last batch's, else the program's own.
hipStream_t call_stream(const OrbProgram* p, void* stream) {
    return stream ? (hipStream_t)stream : (p->last_stream ? p->last_stream : p->stream);
}

struct Buf {
    void** slot;   // where the program keeps the buffer's address
    size_t bytes;
    bool pinned;   // host memory (hipHostMalloc); else device memory
    bool cleared = false;        // a create-time buffer that is zeroed before any launch
    const char* name = nullptr;  // a create-time buffer's, for the message of a failed allocation
    bool soft = false;           // a stage's buffer that its call allocates itself and can do without: listed to be freed
};
// A list of buffers of fixed capacity on the caller's stack, which says so when more are named than it holds
template <int N>
struct BufList {
    static constexpr int kMax = N;
    Buf b[N];
    int n = 0;
    bool overflow = false;
    void add(const Buf& x) {
        if (n < N)
            b[n++] = x;
        else
            overflow = true;
    }
};
using StageBufs = BufList<10>;    // a stage's (stage_buffers)
using ProgramBufs = BufList<48>;  // orb_program_create's (program_buffers)

template <int N>
void free_bufs(const BufList<N>& l) {
    for (int i = 0; i < l.n; i++) {
        if (*l.b[i].slot) (void)(l.b[i].pinned ? hipHostFree(*l.b[i].slot) : hipFree(*l.b[i].slot));
        *l.b[i].slot = nullptr;
    }
}

// The buffers of stage `which`, named here and nowhere else: its first call fills the slots, orb_program_destroy frees them.
StageBufs stage_buffers(OrbProgram* p, int which) {
    const size_t cap = p->cfg.max_features, B = p->plan.max_batch;
    StageBufs l;
    const auto add = [&](auto** slot, size_t bytes, bool pinned = false) { l.add(Buf{(void**)slot, bytes, pinned}); };
    switch (which) {
    case ST_MATCH:  // allocated by orb_match_consecutive itself (d_desc8 only for a matrix-core matcher, and softly); listed to be freed
        add(&p->d_matches, 0);
        add(&p->d_desc8, 0);
        break;
    case ST_VERIFY:
    case ST_EPI: {
        VerifierState& v = which == ST_VERIFY ? p->verify : p->epi;
        add(&v.rec, B * cap * sizeof(float4));
        add(&v.cand, B * cap * sizeof(uint32_t));
        add(&v.n, B * sizeof(uint32_t));
        add(&v.keys, B * kVerifyMaxHyp * sizeof(unsigned long long));
        add(&v.model, B * sizeof(OrbPairModel));
        add(&v.mask, B * cap);
        break;
    }
    case ST_GUIDE:
    case ST_BAND: {
        GridSearchState& g = which == ST_GUIDE ? p->guide : p->band;
        add(&g.srec, B * cap * sizeof(uint4));
        add(&g.sdesc, B * cap * 2u * sizeof(uint4));
        add(&g.cell, B * (kGuideMaxCells + 1u) * sizeof(uint32_t));
        add(&g.match, B * cap * sizeof(MatchRecord));
        add(&g.d_model, B * 9u * sizeof(float));
        add(&g.h_model, B * 9u * sizeof(float), true);
        break;
    }
    case ST_TRACK:
        add(&p->d_tkeys, B * cap * sizeof(uint32_t));
        add(&p->d_tprev, B * cap * sizeof(uint32_t));
        add(&p->d_tnext, B * cap * sizeof(uint32_t));
        add(&p->d_tptr, 2u * B * cap * sizeof(uint4));
        add(&p->d_tlinks, B * sizeof(uint32_t));
        add(&p->d_tshared, B * B * sizeof(uint32_t));
        add(&p->d_tframe, B * sizeof(OrbTrackFrame));
        add(&p->d_track, B * cap * sizeof(OrbTrack));
        break;
    case ST_POSE:
        add(&p->d_pose, B * sizeof(OrbPairPose));
        add(&p->d_ppoints, B * cap * sizeof(OrbPoint));
        add(&p->d_pcount, B * kPoseCounters * sizeof(uint32_t));
        break;
    case ST_TRAJ:
        add(&p->d_jframe, B * sizeof(OrbFramePose));
        add(&p->d_jmap, B * cap * sizeof(OrbPoint));
        add(&p->d_jratio, B * cap * sizeof(uint32_t));
        add(&p->d_jjoint, B * kTrajJointWords * sizeof(uint32_t));
        break;
    case ST_LOCALIZE:
    case ST_BRIDGE: {
        const bool br = which == ST_BRIDGE;
        PnpState& l = br ? p->bridge : p->loc;
        if (br) add(&p->d_bout, B * sizeof(OrbBridgePose));
        add(&l.fix, B * (br ? kBrFixWords : kLocFixWords) * sizeof(uint32_t));
        add(&l.reca, B * cap * sizeof(float4));
        add(&l.recb, B * cap * sizeof(float4));
        if (!br) add(&l.cand, B * cap * sizeof(uint32_t));  // k_br_gather keeps none, and k_loc_score reads none
        add(&l.n, B * sizeof(uint32_t));
        add(&l.keys, B * kVerifyMaxHyp * sizeof(unsigned long long));
        add(&l.mask, B * cap);
        if (br) add(&p->d_bratio, B * cap * sizeof(uint32_t));
        break;
    }
    case ST_LANDMARK:
        add(&p->d_mland, B * cap * sizeof(OrbLandmark));
        add(&p->d_mrow, B * sizeof(OrbLandmarkRow));
        add(&p->d_mpred, B * cap);
        break;
    case ST_ADJUST:
        add(&p->d_apose, B * sizeof(OrbAdjustedPose));
        add(&p->d_ax, B * cap * sizeof(float4));
        add(&p->d_aowner, B * cap * sizeof(uint32_t));
        add(&p->d_aland, B * cap * sizeof(OrbLandmark));
        break;
    case ST_PLACE:
        add(&p->d_psig, B * (size_t)ORB_PLACE_SIG_BYTES_MAX);
        add(&p->d_pdb, (size_t)ORB_PLACE_DB_MAX * ORB_PLACE_SIG_BYTES_MAX);
        add(&p->d_ptbits, B * kPlaceMaxTables * sizeof(uint32_t));
        add(&p->d_pscore, B * (ORB_PLACE_DB_MAX + B) * sizeof(uint32_t));
        add(&p->d_prow, B * sizeof(OrbPlaceRow));
        break;
    case ST_PAIRS: {
        const size_t P = (size_t)ORB_PAIRS_PER_FRAME * B;
        add(&p->d_plist, P * sizeof(OrbFramePair));
        add(&p->h_plist, P * sizeof(OrbFramePair), true);
        add(&p->d_prows, P * cap * sizeof(MatchRecord));
        add(&p->d_pdesc4, B * cap * 128u);  // allocated by orb_match_pairs itself, for the fp4 matcher only, and softly
        l.b[l.n - 1].soft = true;
        break;
    }
    case ST_PAIRS_VERIFY: {
        const size_t P = (size_t)ORB_PAIRS_PER_FRAME * B;
        VerifierState& v = p->pverify;
        add(&v.rec, P * cap * sizeof(float4));
        add(&v.cand, P * cap * sizeof(uint32_t));
        add(&v.n, P * sizeof(uint32_t));
        add(&v.keys, P * kVerifyMaxHyp * sizeof(unsigned long long));
        add(&v.model, P * sizeof(OrbPairModel));
        add(&v.mask, P * cap);
        add(&v.qcount, P * sizeof(uint32_t));
        break;
    }
    case ST_LOOP: {
        const size_t P = (size_t)ORB_PAIRS_PER_FRAME * B;
        PnpState& l = p->loop;
        add(&l.fix, P * sizeof(OrbLoopFix));
        add(&l.reca, P * cap * sizeof(float4));
        add(&l.recb, P * cap * sizeof(float4));
        add(&l.cand, P * cap * sizeof(uint32_t));
        add(&l.n, P * sizeof(uint32_t));
        add(&l.keys, P * kVerifyMaxHyp * sizeof(unsigned long long));
        add(&l.mask, P * cap);
        add(&p->d_lowner, B * cap * sizeof(uint32_t));
        break;
    }
    case ST_KEYFRAMES: {  // allocated by orb_keyframes_reserve (d_kdesc4 by orb_match_keyframes, for the fp4 matcher only, and softly)
        const size_t S = p->kf_slots;
        add(&p->d_khead, S * sizeof(OrbKeyframe));
        add(&p->d_kcorners, S * cap * sizeof(CornerData));
        add(&p->d_kdesc, (B + S) * cap * sizeof(CornerDescriptor));
        add(&p->d_kcounts, (B + S) * sizeof(uint32_t));
        add(&p->d_kpoints, S * cap * sizeof(OrbMapPoint));
        add(&p->d_kowner, B * cap * sizeof(uint32_t));
        add(&p->d_klist, B * sizeof(OrbKeyframeEntry));
        add(&p->h_klist, B * sizeof(OrbKeyframeEntry), true);
        add(&p->d_kdesc4, (B + S) * cap * 128u);
        l.b[l.n - 1].soft = true;
        break;
    }
    case ST_KF_MATCH: {
        const size_t P = (size_t)ORB_PAIRS_PER_FRAME * B;
        add(&p->d_kmlist, P * sizeof(OrbKeyframePair));
        add(&p->h_kmlist, P * sizeof(OrbKeyframePair), true);
        add(&p->d_kmrows, P * cap * sizeof(MatchRecord));
        break;
    }
    case ST_KF_LOC: {
        const size_t P = (size_t)ORB_PAIRS_PER_FRAME * B;
        PnpState& l = p->kfloc;
        add(&l.fix, P * sizeof(OrbKeyframeFix));
        add(&l.reca, P * cap * sizeof(float4));
        add(&l.recb, P * cap * sizeof(float4));
        add(&l.cand, P * cap * sizeof(uint32_t));
        add(&l.n, P * sizeof(uint32_t));
        add(&l.keys, P * kVerifyMaxHyp * sizeof(unsigned long long));
        add(&l.mask, P * cap);
        break;
    }
    case ST_GRAPH: {
        const size_t P = (size_t)ORB_PAIRS_PER_FRAME * B;
        add(&p->d_gpose, B * sizeof(OrbGraphPose));
        add(&p->d_gedge, P * sizeof(OrbGraphEdge));
        add(&p->d_grow, (B + 1u) * sizeof(uint32_t));
        add(&p->d_gcol, 2u * P * sizeof(uint32_t));
        add(&p->d_gwork, B * kPgNodeWords * sizeof(float));
        break;
    }
    case ST_JOIN: {
        const size_t P = (size_t)ORB_PAIRS_PER_FRAME * B;
        add(&p->d_sowner, B * cap * sizeof(uint32_t));
        add(&p->d_sratio, P * cap * sizeof(uint32_t));
        add(&p->d_slink, P * sizeof(OrbJoinLink));
        add(&p->d_skey, B * sizeof(unsigned long long));
        add(&p->d_sseg, B * sizeof(OrbJoinSegment));
        add(&p->d_spose, B * sizeof(OrbJoinPose));
        break;
    }
    case ST_REMAP:
        add(&p->d_rpose, B * sizeof(OrbRemapPose));
        add(&p->d_rrow, B * sizeof(OrbRemapRow));
        add(&p->d_rland, B * cap * sizeof(OrbLandmark));
        break;
    case ST_ANCHOR: {
        const size_t P = (size_t)ORB_PAIRS_PER_FRAME * B;
        add(&p->d_nowner, B * cap * sizeof(uint32_t));
        add(&p->d_nratio, P * cap * sizeof(uint32_t));
        add(&p->d_nlink, P * sizeof(OrbAnchorLink));
        add(&p->d_nkey, B * sizeof(unsigned long long));
        add(&p->d_nseg, B * sizeof(OrbAnchorSegment));
        add(&p->d_npose, B * sizeof(OrbAnchorPose));
        add(&p->d_nrow, B * sizeof(OrbAnchorRow));
        add(&p->d_nland, B * cap * sizeof(OrbLandmark));
        break;
    }
    }
    return l;
}

void free_stage_buffers(OrbProgram* p, int which) { free_bufs(stage_buffers(p, which)); }

// A stage's buffers on its first call, all or none: a failure frees the earlier ones and leaves every slot null, so the next call
// allocates again.
int alloc_all_or_none(OrbProgram* p, int which, const char* who) {
    const StageBufs l = stage_buffers(p, which);
    if (l.overflow) return fail(p, ORB_ESTATE, "%s: internal: the stage names more than %d buffers", who, StageBufs::kMax);
    if (*l.b[0].slot) return ORB_OK;
    for (int i = 0; i < l.n; i++) {
        const Buf& b = l.b[i];
        if (b.soft) continue;
        const hipError_t e = b.pinned ? hipHostMalloc(b.slot, b.bytes, hipHostMallocDefault) : hipMalloc(b.slot, b.bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *b.slot = nullptr;
            free_stage_buffers(p, which);
            if (b.pinned) return fail(p, ORB_EHIP, "%s: hipHostMalloc failed: %s", who, hipGetErrorString(e));
            return fail(p, ORB_EHIP, "%s: hipMalloc of %zu bytes failed: %s", who, b.bytes, hipGetErrorString(e));
        }
    }
    return ORB_OK;
}

// "The last call of this stage is of the current batch and output set": what a later stage asks before it reads the stage's results.
bool stage_fresh(const OrbProgram* p, const Stage& st) { return st.extent && st.seq == p->batch_seq && st.set == p->cur_set; }

// The same of every stage in `need` (bits 1 << StageId), for a call of stage `which`: ORB_OK, or ORB_ESTATE with their names
int stages_fresh(OrbProgram* p, int which, uint32_t need) {
    need &= ~kOutlivesBatch;  // the store is never "of the current batch": its reader checks the generation instead
    uint32_t stale = 0;
    for (int i = 0; i < ST_COUNT; i++)
        if ((need >> i & 1u) && !stage_fresh(p, p->stage[i])) stale |= 1u << i;
    if (!stale) return ORB_OK;
    std::string names;
    for (int i = 0; i < ST_COUNT; i++)
        if (need >> i & 1u) names += std::string(names.empty() ? "orb_" : ", orb_") + kStages[i].name;
    return fail(p, ORB_ESTATE, "%s: needs %s of the current batch and output set", kStages[which].name, names.c_str());
}

// Opens a call of stage `which`: its stream, its event on first use, and the waits behind the stage itself, the stages in `reads` (bits
// 1 << StageId, of the stage's row of kStages) and the readers of what it overwrites -- those that have run, and on another stream.
int stage_begin(OrbProgram* p, int which, void* stream, uint32_t reads, hipStream_t* s_out) {
    if (reads & ~kStages[which].reads)
        return fail(p, ORB_ESTATE, "%s: internal: reads stages 0x%x, kStages says 0x%x", kStages[which].name, reads, kStages[which].reads);
    const hipStream_t s = call_stream(p, stream);
    Stage& self = p->stage[which];
    if (!self.done) HIP_TRY(p, hipEventCreateWithFlags(&self.done, hipEventDisableTiming));
    const uint32_t behind = 1u << which | reads | kReaders.of[which];
    for (int i = 0; i < ST_COUNT; i++) {
        const Stage& o = p->stage[i];
        if ((behind >> i & 1u) && o.stream && o.stream != s) HIP_TRY(p, hipStreamWaitEvent(s, o.done, 0));
    }
    *s_out = s;
    return ORB_OK;
}

// The same with what comes before it in every stage but the matcher: the device, and the stage's buffers on its first call
int stage_open(OrbProgram* p, int which, void* stream, uint32_t reads, hipStream_t* s_out) {
    HIP_TRY(p, hipSetDevice(p->device));
    if (int rc = alloc_all_or_none(p, which, kStages[which].name)) return rc;
    return stage_begin(p, which, stream, reads, s_out);
}

// Closes it after the launches.  p->last_stream is the entry point's business: only the matcher and the verifiers move it.
int stage_end(OrbProgram* p, int which, hipStream_t s, uint32_t extent) {
    HIP_TRY(p, hipGetLastError());
    Stage& self = p->stage[which];
    HIP_TRY(p, hipEventRecord(self.done, s));
    self = {self.done, s, p->batch_seq, p->cur_set, extent};
    return ORB_OK;
}

// Bracket one kernel launch with events when profiling is on.
struct LaunchScope {
    OrbProgram* p;
    hipStream_t s;
    int kid;
    hipEvent_t start = nullptr, stop = nullptr;
    LaunchScope(OrbProgram* p_, hipStream_t s_, int kid_) : p(p_), s(s_), kid(kid_) {
        if (!p->profiling) return;
        auto get = [&]() -> hipEvent_t {
            if (!p->event_pool.empty()) {
                hipEvent_t e = p->event_pool.back();
                p->event_pool.pop_back();
                return e;
            }
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            return e;
        };
        start = get();
        stop = get();
        if (start && stop) (void)hipEventRecord(start, s);
    }
    ~LaunchScope() {
        if (start && stop) {
            (void)hipEventRecord(stop, s);
            p->pending.push_back({kid, start, stop});
        }
    }
};

int drain_profile(OrbProgram* p) {
    for (auto& sp : p->pending) {
        HIP_TRY(p, hipEventSynchronize(sp.stop));
        float ms = 0.f;
        HIP_TRY(p, hipEventElapsedTime(&ms, sp.start, sp.stop));
        p->prof_ms[sp.kid] += ms;
        p->prof_n[sp.kid] += 1;
        p->event_pool.push_back(sp.start);
        p->event_pool.push_back(sp.stop);
    }
    p->pending.clear();
    return ORB_OK;
}

// The staged pipeline for `n` frames starting at device pointer `frames` (orb.rs:469-534).
int run_staged(OrbProgram* p, const uint8_t* frames, uint32_t n, hipStream_t s) {
    const Pyramid& pyr = p->plan.pyr;
    const uint32_t W = pyr.w[0], H = pyr.h[0], D = pyr.depth, cap = p->cfg.max_features;
    HIP_TRY(p, hipMemsetAsync(p->d_counts, 0, sizeof(uint32_t) * n, s));  // orb.rs:475 clear_buffer(counter)
    {
        LaunchScope ls(p, s, KID_GRAY);
        dim3 grid((W + 1023u) / 1024u, H, n);
        if (p->plan.input_y8)
            hipLaunchKernelGGL(k_grayscale_y8, grid, dim3(256), 0, s, frames, p->plan.frame_bytes, p->d_gray, pyr);
        else if (p->plan.intended)
            hipLaunchKernelGGL(k_grayscale<true>, grid, dim3(256), 0, s, frames, p->plan.frame_bytes, p->d_gray, pyr);
        else
            hipLaunchKernelGGL(k_grayscale<false>, grid, dim3(256), 0, s, frames, p->plan.frame_bytes, p->d_gray, pyr, p->opt.fp_contract);
    }
    for (uint32_t m = 1; m < D; m++) {  // orb.rs:413-429
        LaunchScope ls(p, s, KID_MIP);
        dim3 grid((pyr.w[m] + 63u) / 64u, (pyr.h[m] + 4u * kMipRows - 1u) / (4u * kMipRows), n);
        hipLaunchKernelGGL(k_mip, grid, dim3(64, 4), 0, s, p->d_gray, pyr, m, (float)pyr.w[m - 1] / (float)pyr.w[m], (float)pyr.h[m - 1] / (float)pyr.h[m], p->plan.wq);
    }
    for (uint32_t m = 0; m < D; m++) {  // orb.rs:432-466 (both passes)
        LaunchScope ls(p, s, KID_BLUR);
        if (p->plan.intended) {
            hipLaunchKernelGGL(k_gauss, dim3((pyr.w[m] + kGaussTW - 1u) / kGaussTW, (pyr.h[m] + kGaussTH - 1u) / kGaussTH, n), dim3(256), 0, s,
                               p->d_gray, p->d_blur, pyr, m);
            continue;
        }
        dim3 grid(pyr.h[m], 1, n);
        size_t lds = (size_t)pyr.w[m] * 2u * sizeof(uint16_t);
        hipLaunchKernelGGL(k_blur_rows, grid, dim3(256), lds, s, p->d_gray, p->d_blur, pyr, m, p->plan.wq, p->opt.fp_contract);
    }
    const bool nms = (p->opt.flags & ORB_FLAG_NMS) != 0u;
    const uint32_t im = p->plan.intended ? 1u : 0u;
    const bool prov = nms || p->plan.intended;  // the detector writes the provisional list
    if (prov) HIP_TRY(p, hipMemsetAsync(p->d_prov_counts, 0, sizeof(uint32_t) * n, s));
    if (nms && p->plan.intended) HIP_TRY(p, hipMemsetAsync(p->d_prov2_counts, 0, sizeof(uint32_t) * n, s));
    if (nms) {
        HIP_TRY(p, hipMemsetAsync(p->d_score_planes, 0, sizeof(float) * (size_t)p->plan.score_layout.stride * n, s));
    }
    uint32_t width = W, height = H;  // orb.rs:501-519
    for (uint32_t oct = 0; oct < D; oct++) {
        const uint32_t gw = ((width + 7u) / 8u) * 8u, gh = ((height + 7u) / 8u) * 8u;
        if (gw && gh) {
            LaunchScope ls(p, s, KID_FAST);
            dim3 grid((gw + 15u) / 16u, (gh + 15u) / 16u, n);
            if (prov)
                hipLaunchKernelGGL(k_fast, grid, dim3(16, 16), 0, s, p->d_gray, pyr, oct, gw, gh, p->threshold, p->plan.arc, im,
                                   p->d_prov_counts, p->d_prov, p->plan.cap_prov, p->d_prov_scores,
                                   nms ? p->d_score_planes : (float*)nullptr, p->plan.score_layout);
            else
                hipLaunchKernelGGL(k_fast, grid, dim3(16, 16), 0, s, p->d_gray, pyr, oct, gw, gh, p->threshold, p->plan.arc, im,
                                   p->d_counts, p->d_corners, cap, (float*)nullptr, (float*)nullptr, p->plan.score_layout, p->plan.oob);
        }
        width /= 2u;
        height /= 2u;
    }
    const uint32_t nms_blocks = std::min<uint32_t>((p->plan.cap_prov + 255u) / 256u, 64u);
    if (nms && !p->plan.intended) {
        LaunchScope ls(p, s, KID_FAST);
        hipLaunchKernelGGL(k_nms, dim3(nms_blocks, 1, n), dim3(256), 0, s, p->d_prov_counts, p->d_prov,
                           p->d_prov_scores, p->plan.cap_prov, p->d_score_planes, p->plan.score_layout, p->d_counts, p->d_corners,
                           cap, (float*)nullptr);
    }
    if (p->plan.intended) {  // [NMS ->] top-K cut -> final list (IM-7, IM-8)
        LaunchScope ls(p, s, KID_FAST);
        if (nms)
            hipLaunchKernelGGL(k_nms, dim3(nms_blocks, 1, n), dim3(256), 0, s, p->d_prov_counts,
                               p->d_prov, p->d_prov_scores, p->plan.cap_prov, p->d_score_planes, p->plan.score_layout,
                               p->d_prov2_counts, p->d_prov2, p->plan.cap_prov, p->d_prov2_scores);
        hipLaunchKernelGGL(k_topk, dim3(n), dim3(1024), 0, s, nms ? p->d_prov2_counts : p->d_prov_counts,
                           nms ? p->d_prov2 : p->d_prov, nms ? p->d_prov2_scores : p->d_prov_scores, p->plan.cap_prov,
                           p->d_counts, p->d_corners, cap);
    }
    {  // orb.rs:523-534
        LaunchScope ls(p, s, KID_BRIEF);
        BriefTables tab{p->d_pattern, p->d_cos, p->d_sin, p->d_rot};
        uint32_t bx = (cap + 127u) / 128u;  // ~32 keypoints per wave at a full frame
        if (bx > 64u) bx = 64u;
        if (bx < 1u) bx = 1u;
        hipLaunchKernelGGL(k_brief, dim3(bx, 1, n), dim3(256), 0, s, p->d_blur, pyr, p->d_counts, p->d_corners, cap,
                           p->d_desc, tab, im, p->plan.oob, p->opt.fp_contract, p->opt.angle_bins);
    }
    HIP_TRY(p, hipGetLastError());
    p->planes_valid = true;
    return ORB_OK;
}

// k_slot_prefix + BRIEF over the band (or tile) slots `rows_geom` of frames [f0, f0 + n).
int launch_brief(OrbProgram* p, hipStream_t s, uint32_t n, const RowsGeom& rows_geom, const uint16_t* d_blur,
                 const uint16_t* d_blur_rowc, const uint32_t* seg_counts, uint32_t* seg_before, const CornerData* seg,
                 uint32_t* d_counts, CornerData* d_corners, CornerDescriptor* d_desc, uint32_t f0 = 0) {
    const uint32_t cap = p->cfg.max_features;
    const BriefTables tab{p->d_pattern, p->d_cos, p->d_sin, p->d_rot};
    const bool use_t = p->plan.use_brief_t;
    {
        LaunchScope ls(p, s, KID_PREFIX);
        hipLaunchKernelGGL(k_slot_prefix, dim3(n), dim3(64), 0, s, seg_counts, seg_before, d_counts, rows_geom.n_slots,
                           rows_geom.seg_cap, use_t ? p->plan.brieft.n_classes : 1u);
    }
    if (use_t) {
        const BriefTGeom& tg = p->plan.brieft;
        const dim3 grid(n, (cap + (uint32_t)kBriefNfChunk - 1u) / (uint32_t)kBriefNfChunk);  // k_brief_nf's
        // the not-flat mask of these frames in the current output set: written by k_brief_t, read by k_brief_nf behind it on the stream
        const uint32_t mask_words = brief_mask_words(cap);
        uint64_t* const nf_mask = p->d_nf_mask[p->cur_set] + (size_t)f0 * mask_words;
        {
            LaunchScope ls(p, s, KID_BRIEF_T);
#define BRIEF_T_LAUNCH(ROT_)                                                                                                         \
    hipLaunchKernelGGL((k_brief_t<kBriefTWaves, ROT_>), dim3(n, (cap + kBriefTThreads - 1u) / kBriefTThreads), dim3(kBriefTThreads), \
                       brieft_lds_bytes(tg), s, d_blur_rowc, p->plan.pyr, tg, seg_counts, seg_before, seg, d_corners, cap, d_desc, tab, nf_mask, mask_words)
            switch (rot_form(p->opt.fp_contract)) {  // the rotation's form (OrbOptions::fp_contract): a template parameter of the straight-line tests
                case 1: BRIEF_T_LAUNCH(1); break;
                case 2: BRIEF_T_LAUNCH(2); break;
                default: BRIEF_T_LAUNCH(0); break;
            }
#undef BRIEF_T_LAUNCH
        }
        LaunchScope ls(p, s, KID_BRIEF_NF);
        // the level constants: a scalar select between two levels' kernel arguments, or the LDS table for deeper pyramids
#define BRIEF_NF_LAUNCH(OOB_, TABLE_)                                                                                                  \
    hipLaunchKernelGGL((k_brief_nf<OOB_, TABLE_>), grid, dim3(256), 0, s, d_blur, d_blur_rowc, p->plan.pyr, tg, d_corners, cap, d_desc, tab, \
                       nf_mask, mask_words)
        const bool table = p->plan.pyr.depth > 2u;
        if (p->plan.oob != kOobZero) {
            if (table) BRIEF_NF_LAUNCH(true, true); else BRIEF_NF_LAUNCH(true, false);
        } else {
            if (table) BRIEF_NF_LAUNCH(false, true); else BRIEF_NF_LAUNCH(false, false);
        }
#undef BRIEF_NF_LAUNCH
    } else {
        LaunchScope ls(p, s, KID_BRIEF_ROWS);
        RowsGeom rg = rows_geom;
        rg.oob = p->plan.oob;
        rg.fp = p->opt.fp_contract;
        rg.split = 1u;  // small batches: several workgroups per band slot so that the chip still sees ~2000 of them
        while (rg.split < 16u && rg.n_slots * n * rg.split < 2048u) rg.split *= 2u;
        hipLaunchKernelGGL(k_brief_rows, dim3(rg.n_slots * rg.split, n), dim3(256), 0, s, d_blur, d_blur_rowc, p->plan.pyr, rg,
                           seg_counts, seg_before, seg, d_corners, cap, d_desc, tab);
    }
    return ORB_OK;
}

// The program's ready-made blur column table for a launch of geometry g (FrontGeom::blur_tab): level 0 on full-width bands has one.
const BlurCol* front_blur_tab(const OrbProgram* p, const FrontGeom& g) {
    return (g.lvl == 0u && !g.tiled) ? reinterpret_cast<const BlurCol*>(p->d_blur_tab) : nullptr;
}

// The geometry of level `lvl` of the plain fused pipeline for a batch of n frames: the plan's, with the program's device pointers.
FrontGeom fused_level_geometry(const OrbProgram* p, uint32_t lvl, uint32_t gw, uint32_t gh, uint32_t n) {
    FrontGeom g = plan_level_geometry(p->plan, p->opt, p->env, lvl, gw, gh, n);
    g.stamps = p->d_stamps;
    g.blur_tab = front_blur_tab(p, g);
    return g;
}

// The fused pipeline for frames [f0, f0 + n) of the batch on stream s: one k_front launch per level + BRIEF
// (with_brief = false: the caller launches its own BRIEF kernel -- the single-frame path's k_brief_one).
// first_level > 0 (single-frame call): the levels below it have been launched already (k_front_pair).
int run_fused_range(OrbProgram* p, const uint8_t* frames_all, uint32_t f0, uint32_t n, hipStream_t s, bool with_brief = true,
                    uint32_t first_level = 0) {
    const Pyramid& pyr = p->plan.pyr;
    const uint32_t D = pyr.depth, cap = p->cfg.max_features;
    const uint8_t* frames = frames_all + (size_t)f0 * p->plan.frame_bytes;
    uint16_t* const d_gray = p->d_gray + (size_t)f0 * pyr.stride;
    uint16_t* const d_blur = p->d_blur + (size_t)f0 * pyr.stride;
    uint16_t* const d_blur_rowc = p->d_blur_rowc + (size_t)f0 * pyr.row_stride;
    const size_t lists = (size_t)p->plan.bands.n_slots * p->plan.seg_classes;  // lists per frame
    uint32_t* const d_seg_counts = p->d_seg_counts + (size_t)f0 * lists;
    uint32_t* const d_seg_before = p->d_seg_before + (size_t)f0 * lists;
    CornerData* const d_seg = p->d_seg + (size_t)f0 * lists * p->plan.bands.seg_cap;
    uint32_t* const d_counts = p->d_counts + f0;
    CornerData* const d_corners = p->d_corners + (size_t)f0 * cap;
    CornerDescriptor* const d_desc = p->d_desc + (size_t)f0 * cap;
    // orb.rs:475 clear_buffer(counter): every band slot's count is rewritten by its k_front block and
    // counts[] by k_slot_prefix, so nothing needs clearing here.
    uint32_t width = pyr.w[0], height = pyr.h[0];  // orb.rs:501-519
    for (uint32_t lvl = 0; lvl < D; lvl++) {
        const uint32_t gw = ((width + 7u) / 8u) * 8u, gh = ((height + 7u) / 8u) * 8u;
        width /= 2u;
        height /= 2u;
        if (lvl < first_level) continue;  // launched by the caller
        if (lvl > 0 && !(pyr.w[lvl - 1] == 2u * pyr.w[lvl] && pyr.h[lvl - 1] == 2u * pyr.h[lvl])) {
            hipStream_t sm = s;
            LaunchScope ls(p, sm, KID_MIP);  // inexact reduction (odd source size): generic bilinear blit
            dim3 grid((pyr.w[lvl] + 63u) / 64u, (pyr.h[lvl] + 4u * kMipRows - 1u) / (4u * kMipRows), n);
            hipLaunchKernelGGL(k_mip, grid, dim3(64, 4), 0, sm, d_gray, pyr, lvl, (float)pyr.w[lvl - 1] / (float)pyr.w[lvl], (float)pyr.h[lvl - 1] / (float)pyr.h[lvl], p->plan.wq);
        }
        const FrontGeom g = fused_level_geometry(p, lvl, gw, gh, n);
        hipStream_t s_lvl = s;
        if (g.n_bands * (g.tiled ? g.n_ct : 1u) != p->plan.bands.slot_base[lvl + 1] - p->plan.bands.slot_base[lvl])
            return fail(p, ORB_EINVAL, "internal: band count mismatch at level %u", lvl);
        if (!g.tiled && sizeof(BlurCol) * (size_t)g.n_var > 8u * (size_t)g.ts)  // the column table borrows the queues' storage
            return fail(p, ORB_EINVAL, "internal: blur column table of level %u does not fit", lvl);
        uint32_t lds = front_lds_bytes(g);
        lds += (uint32_t)p->env.lds_pad;  // TINYORB_LDS_PAD: occupancy experiments only
        if (lds > p->max_lds) return fail(p, ORB_EINVAL, "level %u needs %u bytes of LDS", lvl, lds);
        const dim3 grid(g.n_bands * (g.tiled ? g.n_ct : 1u) * n);
        // The kernel instances live in orb_front_inst.hip, one translation unit per arithmetic form (orb_front_launch.h); the form a
        // launch takes carries the luminance bits only where a luminance is computed (level 0 from RGBA).
        FrontLaunch L{frames, p->plan.frame_bytes, d_gray, d_blur, d_blur_rowc, pyr, g, p->threshold, d_seg_counts, d_seg, s_lvl, grid.x, lds,
                      p->plan.band_rows_lvl[lvl], p->plan.ln_threads[lvl], p->plan.input_y8,
                      // rows not aligned to a quad, or the level-0 plane is needed (level 1 not an exact half): the general variant
                      lvl == 0 && ((pyr.w[0] & 3u) || g.store_grey), p->plan.oob != kOobZero, false};
        L.geo = front_pick_geo(p->env, p->opt.fp_contract, L);
        {
            LaunchScope ls(p, s_lvl, lvl == 0 ? KID_FUSED_L0 : KID_FUSED_LN);
            const hipError_t e = kFrontLaunch[front_form(p->opt.fp_contract, lvl == 0 && !p->plan.input_y8)](L);
            if (e != hipSuccess) return fail(p, ORB_EHIP, "k_front (level %u) failed to launch: %s", lvl, hipGetErrorString(e));
        }
    }
    // orb.rs:523-534, plus the compaction of the band segments into the final lists
    if (with_brief) launch_brief(p, s, n, p->plan.rows, d_blur, d_blur_rowc, d_seg_counts, d_seg_before, d_seg, d_counts, d_corners, d_desc, f0);
    HIP_TRY(p, hipGetLastError());
    return ORB_OK;
}

int run_fused(OrbProgram* p, const uint8_t* frames, uint32_t n, hipStream_t s) {
    // One launch per kernel for the whole batch.  Cutting the batch was measured twice and lost both times (NOTEBOOK.md): round 1, whole
    // pipelines of 2 / 4 / 8 chunks on two streams: + 5 %, + 4 %, + 6 % time; round 4 (TINYORB_BATCH_SPLIT, profiles/r04_split_ab.txt), the
    // BRIEF kernels of sub-range i on a side stream under the front kernels of sub-range i + 1: 45 us MORE per cut -- k_front's two
    // workgroups per CU hold all of the CU's LDS and wave slots, k_brief_t is as bound by the vector units as k_front is, and every
    // cross-queue dependency costs a signal round trip.  The experiment's code left the tree in round 5.
    if (int rc = run_fused_range(p, frames, 0, n, s)) return rc;
    p->planes_valid = true;  // except the level-0 grey plane, which the fused path keeps in LDS only
    return ORB_OK;
}

// The fused "intended" pipeline: k_front_i per level (+ k_mip where a level is not an exact half), k_gauss per
// level, k_select_i, k_brief_i.
int run_fused_i(OrbProgram* p, const uint8_t* frames, uint32_t n, hipStream_t s) {
    const Pyramid& pyr = p->plan.pyr;
    const uint32_t D = pyr.depth, cap = p->cfg.max_features;
    const IBriefGeom& bg = p->plan.itiles;
    for (uint32_t lvl = 0; lvl < D; lvl++) {
        if (lvl > 0 && !(pyr.w[lvl - 1] == 2u * pyr.w[lvl] && pyr.h[lvl - 1] == 2u * pyr.h[lvl])) {
            LaunchScope ls(p, s, KID_MIP);
            dim3 grid((pyr.w[lvl] + 63u) / 64u, (pyr.h[lvl] + 4u * kMipRows - 1u) / (4u * kMipRows), n);
            hipLaunchKernelGGL(k_mip, grid, dim3(64, 4), 0, s, p->d_gray, pyr, lvl, (float)pyr.w[lvl - 1] / (float)pyr.w[lvl], (float)pyr.h[lvl - 1] / (float)pyr.h[lvl]);
        }
        IGeom g{};
        g.lvl = lvl;
        g.tw = bg.tw[lvl];
        g.n_ct = bg.n_ct[lvl];
        g.n_bands = (pyr.h[lvl] + kFrontRows - 1) / kFrontRows;
        g.ls = kIPad + g.tw + 16u;
        g.write_mip = (lvl + 1 < D && pyr.w[lvl] == 2u * pyr.w[lvl + 1] && pyr.h[lvl] == 2u * pyr.h[lvl + 1]) ? 1u : 0u;
        g.xcd_swizzle = (n % 8u == 0u) ? 1u : 0u;
        g.slot_base = bg.slot_base[lvl];
        g.n_slots = bg.n_slots;
        g.seg_cap = bg.seg_cap;
        g.arc = p->plan.arc;
        g.nms = (p->opt.flags & ORB_FLAG_NMS) ? 1u : 0u;
        g.phase_mask = p->env.phase_mask >= 0 ? (uint32_t)p->env.phase_mask : 63u;
        g.literal = 0u;
        g.dw = pyr.w[lvl];
        g.dh = pyr.h[lvl];
        g.gx1 = (uint32_t)((int)pyr.w[lvl] - 16);
        g.gy1 = (uint32_t)((int)pyr.h[lvl] - 16);
        g.blur = p->plan.igauss_fused ? 1u : 0u;
        g.store_grey = p->plan.igrey_stored ? 1u : 0u;
        if (g.n_bands * g.n_ct != bg.slot_base[lvl + 1] - bg.slot_base[lvl])
            return fail(p, ORB_EINVAL, "internal: tile count mismatch at level %u", lvl);
        if (g.blur && !ifront_gauss_fits(g.tw)) return fail(p, ORB_EINVAL, "internal: tile width %u too wide for the fused Gaussian", g.tw);
        const dim3 grid(g.n_bands * g.n_ct * n);
        LaunchScope ls(p, s, lvl == 0 ? KID_FRONT_I : KID_FRONT_I_LN);  // level 0 (RGBA in) and the levels above are different launches: one id each
        if (lvl == 0)
            hipLaunchKernelGGL(k_front_i<true>, grid, dim3(kIThreads), ifront_lds_bytes(g), s, frames, p->plan.frame_bytes,
                               p->d_gray, p->d_blur, pyr, g, p->threshold, p->d_iseg_counts, p->d_iseg, p->d_iseg_scores);
        else
            hipLaunchKernelGGL(k_front_i<false>, grid, dim3(kIThreads), ifront_lds_bytes(g), s, frames, p->plan.frame_bytes,
                               p->d_gray, p->d_blur, pyr, g, p->threshold, p->d_iseg_counts, p->d_iseg, p->d_iseg_scores);
    }
    for (uint32_t m = 0; m < D && !p->plan.igauss_fused; m++) {
        LaunchScope ls(p, s, KID_BLUR);
        hipLaunchKernelGGL(k_gauss, dim3((pyr.w[m] + kGaussTW - 1u) / kGaussTW, (pyr.h[m] + kGaussTH - 1u) / kGaussTH, n), dim3(256), 0, s, p->d_gray,
                           p->d_blur, pyr, m);
    }
    {
        LaunchScope ls(p, s, KID_SELECT_I);
        hipLaunchKernelGGL(k_select_i, dim3(n), dim3(1024), 0, s, p->d_iseg_counts, p->d_iseg, p->d_iseg_scores, bg.n_slots,
                           bg.seg_cap, cap, p->d_counts, p->d_thr_key, p->d_iseg_before);
    }
    {
        LaunchScope ls(p, s, KID_BRIEF_I);
        IBriefGeom bgl = bg;
        bgl.xcd_swizzle = (n % 8u == 0u) ? 1u : 0u;
        bgl.phase_mask = p->env.brief_i_mask >= 0 ? (uint32_t)p->env.brief_i_mask : 3u;
        bgl.angle_bins = p->opt.angle_bins;
        hipLaunchKernelGGL(k_brief_i, dim3(bg.group_base[D] * n), dim3(kIBriefThreads), p->plan.ibrief_lds, s, p->d_blur, pyr, bgl,
                           p->d_iseg_counts, p->d_iseg_before, p->d_thr_key, p->d_iseg, p->d_iseg_scores, p->d_corners, cap,
                           p->d_desc, BriefTables{p->d_pattern, p->d_cos, p->d_sin, p->d_rot});
    }
    HIP_TRY(p, hipGetLastError());
    p->planes_valid = true;
    return ORB_OK;
}

// The reference's algorithm with the opt-in arc length / NMS, fused: k_front_i per level
// in its literal setting (grey plane, detector, NMS, mip), k_front<false> per level with only its blur phase (row
// constants + stored tail from the grey plane), k_slot_prefix, k_brief_rows over the tile slots.
int run_fused_x(OrbProgram* p, const uint8_t* frames, uint32_t n, hipStream_t s) {
    const Pyramid& pyr = p->plan.pyr;
    const uint32_t D = pyr.depth;
    const IBriefGeom& bg = p->plan.itiles;
    uint32_t band_base = 0;
    for (uint32_t lvl = 0; lvl < D; lvl++) {
        if (lvl > 0 && !(pyr.w[lvl - 1] == 2u * pyr.w[lvl] && pyr.h[lvl - 1] == 2u * pyr.h[lvl])) {
            LaunchScope ls(p, s, KID_MIP);
            dim3 grid((pyr.w[lvl] + 63u) / 64u, (pyr.h[lvl] + 4u * kMipRows - 1u) / (4u * kMipRows), n);
            hipLaunchKernelGGL(k_mip, grid, dim3(64, 4), 0, s, p->d_gray, pyr, lvl, (float)pyr.w[lvl - 1] / (float)pyr.w[lvl], (float)pyr.h[lvl - 1] / (float)pyr.h[lvl]);
        }
        uint32_t gw, gh;
        reference_grid(pyr, lvl, &gw, &gh);
        IGeom g{};
        g.lvl = lvl;
        g.tw = bg.tw[lvl];
        g.n_ct = bg.n_ct[lvl];
        g.n_bands = bg.n_bands[lvl];
        g.ls = kIPad + g.tw + 16u;
        g.write_mip = (lvl + 1 < D && pyr.w[lvl] == 2u * pyr.w[lvl + 1] && pyr.h[lvl] == 2u * pyr.h[lvl + 1]) ? 1u : 0u;
        g.xcd_swizzle = (n % 8u == 0u) ? 1u : 0u;
        g.slot_base = bg.slot_base[lvl];
        g.n_slots = bg.n_slots;
        g.seg_cap = bg.seg_cap;
        g.arc = p->plan.arc;
        g.nms = (p->opt.flags & ORB_FLAG_NMS) ? 1u : 0u;
        g.phase_mask = 63u;
        g.literal = 1u;
        g.store_grey = 1u;  // the literal blur below reads the grey plane
        g.blur = 0u;
        g.dw = std::max(pyr.w[lvl], gw);
        g.dh = std::max(pyr.h[lvl], gh);
        g.gx1 = std::min<uint32_t>(gw, pyr.w[0] > 16u ? pyr.w[0] - 16u : 0u);  // fast.wgsl:77 with level-0 dimensions (Q8)
        g.gy1 = std::min<uint32_t>(gh, pyr.h[0] > 16u ? pyr.h[0] - 16u : 0u);
        if (g.n_bands * g.n_ct != bg.slot_base[lvl + 1] - bg.slot_base[lvl])
            return fail(p, ORB_EINVAL, "internal: tile count mismatch at level %u", lvl);
        if (gw && gh) {
            LaunchScope ls(p, s, lvl == 0 ? KID_FRONT_I : KID_FRONT_I_LN);  // level 0 (RGBA in) and the levels above are different launches: one id each
            const dim3 grid(g.n_bands * g.n_ct * n);
            if (lvl == 0)
                hipLaunchKernelGGL(k_front_i<true>, grid, dim3(kIThreads), ifront_lds_bytes(g), s, frames, p->plan.frame_bytes,
                                   p->d_gray, p->d_blur, pyr, g, p->threshold, p->d_iseg_counts, p->d_iseg, p->d_iseg_scores);
            else
                hipLaunchKernelGGL(k_front_i<false>, grid, dim3(kIThreads), ifront_lds_bytes(g), s, frames, p->plan.frame_bytes,
                                   p->d_gray, p->d_blur, pyr, g, p->threshold, p->d_iseg_counts, p->d_iseg, p->d_iseg_scores);
        }
        // else: no FAST dispatch at this octave (orb.rs:511-515 with width 0).  Its tile slots were zeroed at create and
        // no kernel of this program ever writes them, so there is nothing to clear (clearing the whole counter array
        // here would erase the counts the earlier levels have just produced).
        {   // literal blur of this level from its grey plane: k_front's staging + phase C, nothing else
            FrontGeom fg = front_geometry(pyr, lvl, gw ? gw : 8u, gh, n);
            fg.phase_mask = 8u;
            fg.write_mip = 0u;
            fg.slot_base = band_base;
            fg.n_slots = p->plan.xband_slots;
            fg.seg_cap = 1u;
            fg.n_classes = 1u;
            fg.stamps = nullptr;
            band_base += fg.n_bands;
            const uint32_t lds = front_lds_bytes(fg);
            if (lds > p->max_lds) return fail(p, ORB_EINVAL, "level %u needs %u bytes of LDS", lvl, lds);
            LaunchScope ls(p, s, KID_FUSED_LN);
            const FrontLaunch L{frames, p->plan.frame_bytes, p->d_gray, p->d_blur, p->d_blur_rowc, pyr, fg, p->threshold, p->d_xband_counts, p->d_iseg, s,
                                fg.n_bands * n, lds, (uint32_t)kFrontRows, (uint32_t)kFrontThreadsLN, false, false, false, true};
            const hipError_t e = kFrontLaunch[0](L);  // k_front<false> (16 rows, 512 threads), from the unit that instantiates it
            if (e != hipSuccess) return fail(p, ORB_EHIP, "k_front (blur of level %u) failed to launch: %s", lvl, hipGetErrorString(e));
        }
    }
    launch_brief(p, s, n, p->plan.xrows, p->d_blur, p->d_blur_rowc, p->d_iseg_counts, p->d_iseg_before, p->d_iseg, p->d_counts,
                 p->d_corners, p->d_desc);
    HIP_TRY(p, hipGetLastError());
    p->planes_valid = true;
    return ORB_OK;
}

int launch_compact(OrbProgram* p, uint32_t n, uint32_t* counts, uint64_t* offsets, CornerData* corners, CornerDescriptor* desc,
                   size_t capacity, void* stream, hipStream_t* used);  // below, with the bulk read-back

int run_pipeline(OrbProgram* p, const uint8_t* frames, uint32_t n, hipStream_t s) {
    if (p->plan.fused_i) return run_fused_i(p, frames, n, s);
    if (p->plan.fused_x) return run_fused_x(p, frames, n, s);
    return p->plan.fused ? run_fused(p, frames, n, s) : run_staged(p, frames, n, s);
}

int ensure_input(OrbProgram* p) {
    if (!p->d_input) HIP_TRY(p, hipMalloc(&p->d_input, p->plan.frame_bytes * p->plan.max_batch));
    return ORB_OK;
}

// Entries of the rotated-pattern table, for the consumer this program has: k_brief_i's window (intended, full circle; IM-6b,
// OrbOptions::angle_bins: one entry per angle bin instead of one per milliradian code) or k_brief_nf's patch (the reference's codes 0..3141)
uint32_t rot_codes(const OrbProgram* p) {
    return p->plan.fused_i ? (p->opt.angle_bins ? p->opt.angle_bins : (uint32_t)ORB_ANGLE_STEPS_FULL) : (uint32_t)ORB_ANGLE_STEPS;
}

// k_front's blur column table of level 0: a function of the level's width (and the sampler's weight bits) alone, so built at create
// once, with the band's own arithmetic (blur_col_entry), instead of by every band of every frame.  A level 0 on column tiles
// and the levels above keep building theirs in the band (orb_front_body.inc): n_var = 0, no table.
FrontGeom blur_tab_geometry(const OrbProgram* p) {
    if (!p->plan.fused || p->plan.tile_w_lvl[0]) return FrontGeom{};
    return front_geometry(p->plan.pyr, 0, 8u, 8u, 1, p->plan.band_rows_lvl[0]);  // blur_p, blur_q, n_var: of the width alone
}

// The buffers orb_program_create allocates, named here and nowhere else: create fills the slots (and zeroes the cleared ones, a blocking
// hipMemset before any launch), orb_program_destroy frees them.  A function of the plan, the options and the switches, which do not change.
// Not here: what is allocated on first use (d_input, d_input_alt, the pack buffers, the stages' buffers).
ProgramBufs program_buffers(OrbProgram* p) {
    const ProgramPlan& pl = p->plan;
    const size_t B = pl.max_batch, cap = p->cfg.max_features;
    const int sets = (p->opt.flags & ORB_FLAG_DOUBLE_OUTPUT) ? 2 : 1;
    ProgramBufs l;
    enum { kDevice = 0, kPinned = 1, kCleared = 2 };
#define PBUF(slot, bytes, kind) l.add(Buf{(void**)&p->slot, (bytes), ((kind) & kPinned) != 0, ((kind) & kCleared) != 0, #slot})
    PBUF(d_gray, B * pl.pyr.stride * sizeof(uint16_t), kDevice);
    PBUF(d_blur, B * pl.pyr.stride * sizeof(uint16_t), kDevice);
    for (int set = 0; set < sets; set++) {
        PBUF(out_counts[set], B * sizeof(uint32_t), kDevice | kCleared);
        PBUF(out_corners[set], B * cap * sizeof(CornerData), kDevice | kCleared);
        PBUF(out_desc[set], B * cap * sizeof(CornerDescriptor), kDevice | kCleared);
    }
    if (pl.fused || pl.fused_x) PBUF(d_blur_rowc, B * pl.pyr.row_stride * sizeof(uint16_t), kDevice | kCleared);
    if (pl.fused) {
        const size_t lists = (size_t)pl.bands.n_slots * pl.seg_classes;
        PBUF(d_seg, B * lists * (size_t)pl.bands.seg_cap * sizeof(CornerData), kDevice);
        PBUF(d_seg_counts, B * lists * sizeof(uint32_t), kDevice | kCleared);
        PBUF(d_seg_before, B * lists * sizeof(uint32_t), kDevice);
    }
    if (pl.use_brief_t)  // (the band pipeline or the tile pipeline: whichever launch_brief serves)
        for (int set = 0; set < sets; set++)  // (not cleared: k_brief_t writes every word of the frames of a batch before k_brief_nf reads them)
            PBUF(d_nf_mask[set], B * brief_mask_words((uint32_t)cap) * sizeof(uint64_t), kDevice);
    if (pl.fused_x) PBUF(d_xband_counts, B * (size_t)pl.xband_slots * sizeof(uint32_t), kDevice);
    if (pl.fused_i || pl.fused_x) {
        const size_t n_seg = B * (size_t)pl.itiles.n_slots;
        PBUF(d_iseg, n_seg * pl.itiles.seg_cap * sizeof(CornerData), kDevice);
        PBUF(d_iseg_scores, n_seg * pl.itiles.seg_cap * sizeof(float), kDevice);
        PBUF(d_iseg_counts, n_seg * sizeof(uint32_t), kDevice | kCleared);
        PBUF(d_iseg_before, n_seg * sizeof(uint32_t), kDevice);
        PBUF(d_thr_key, B * sizeof(unsigned long long), kDevice);
    } else if (p->opt.flags & (ORB_FLAG_NMS | ORB_FLAG_INTENDED)) {  // the staged kernels' score planes and provisional lists
        if (p->opt.flags & ORB_FLAG_NMS) PBUF(d_score_planes, B * (size_t)pl.score_layout.stride * sizeof(float), kDevice);
        PBUF(d_prov_counts, B * sizeof(uint32_t), kDevice);
        PBUF(d_prov, B * (size_t)pl.cap_prov * sizeof(CornerData), kDevice);
        PBUF(d_prov_scores, B * (size_t)pl.cap_prov * sizeof(float), kDevice);
        if (pl.intended && (p->opt.flags & ORB_FLAG_NMS)) {
            PBUF(d_prov2_counts, B * sizeof(uint32_t), kDevice);
            PBUF(d_prov2, B * (size_t)pl.cap_prov * sizeof(CornerData), kDevice);
            PBUF(d_prov2_scores, B * (size_t)pl.cap_prov * sizeof(float), kDevice);
        }
    }
    PBUF(d_pattern, 256 * sizeof(uint32_t), kDevice);
    PBUF(d_cos, ORB_ANGLE_STEPS_FULL * sizeof(float), kDevice);
    PBUF(d_sin, ORB_ANGLE_STEPS_FULL * sizeof(float), kDevice);
    PBUF(d_rot, (size_t)rot_codes(p) * 64u * sizeof(uint4), kDevice);
    // (cleared on the program's stream in front of its kernel, create_tables: an odd n_var ends in the middle of a piece)
    if (const uint32_t pieces = blur_col_pieces(blur_tab_geometry(p).n_var)) PBUF(d_blur_tab, (size_t)pieces * sizeof(uint4), kDevice);
    if (pl.fused && p->env.stamps) PBUF(d_stamps, 32 * sizeof(unsigned long long), kDevice | kCleared);  // diagnostic builds only (tools/stamps.py)
    PBUF(h_count, kSingleCountWords * sizeof(uint32_t), kPinned);  // (cleared by the host, create_buffers)
    PBUF(d_single_done, sizeof(uint32_t), kDevice | kCleared);
    PBUF(h_corners, cap * sizeof(CornerData), kPinned);
    PBUF(h_desc, cap * sizeof(CornerDescriptor), kPinned);
#undef PBUF
    return l;
}

// orb_program_create, step by step.  Each returns ORB_OK or the code of fail(p, ...); create then destroys the program.

int create_device(OrbProgram* p) {
    int n_dev = 0;
    const hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0) return fail(p, ORB_EHIP, "no HIP device available (%s)", e == hipSuccess ? "count is 0" : hipGetErrorString(e));
    if (p->device < 0 || p->device >= n_dev) return fail(p, ORB_EINVAL, "device %d out of range (0..%d)", p->device, n_dev - 1);
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    int lds_max = 0, cus = 0;
    HIP_TRY(p, hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, p->device));
    HIP_TRY(p, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->device));
    p->max_lds = (uint32_t)lds_max;
    p->n_cus = cus > 0 ? (uint32_t)cus : 256u;
    return ORB_OK;
}

// The dynamic-LDS attribute belongs to the function on this device, not to the program: always raise it to the device's limit (less
// the kernel's static LDS), never to this program's own need, so that a later, smaller program never lowers it under a live, larger one.
int create_attributes(OrbProgram* p) {
    if (p->plan.fused)
        for (auto set_max_lds : kFrontSetMaxLds) HIP_TRY(p, set_max_lds((int)p->max_lds));  // every instance of k_front / k_front_pair
    if (p->plan.fused_i) {
        hipFuncAttributes fa{};
        hipError_t ea = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&k_brief_i));
        if (ea == hipSuccess && p->plan.ibrief_lds + (uint32_t)fa.sharedSizeBytes > p->max_lds)
            return fail(p, ORB_EINVAL, "k_brief_i needs %u bytes of LDS", p->plan.ibrief_lds + (uint32_t)fa.sharedSizeBytes);
        if (ea == hipSuccess)
            ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_brief_i), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(p->max_lds - (uint32_t)fa.sharedSizeBytes));
        if (ea != hipSuccess) return fail(p, ORB_EHIP, "hipFuncSetAttribute(k_brief_i): %s", hipGetErrorString(ea));
    }
    if (p->plan.fused_x) {
        const hipError_t ea = kFrontSetMaxLds[0]((int)p->max_lds);  // (the unit that holds k_front<false>)
        if (ea != hipSuccess) return fail(p, ORB_EHIP, "hipFuncSetAttribute(k_front): %s", hipGetErrorString(ea));
    }
    return ORB_OK;
}

// TINYORB_FRONT_TRACE=1: which instance of k_front a full batch takes at each level; and the staged pipeline's note, once per process
void create_say(const OrbProgram* p) {
    if (p->plan.fused && p->env.front_trace) fputs(front_trace_text(p->plan, p->opt, p->env).c_str(), stderr);
    static bool warned = false;
    if (!p->plan.pipeline_note.empty() && !warned && !p->env.quiet) {
        warned = true;
        fprintf(stderr, "libtinyorb: %s\n", p->plan.pipeline_note.c_str());
    }
}

int create_buffers(OrbProgram* p) {
    const ProgramBufs l = program_buffers(p);
    if (l.overflow) return fail(p, ORB_ESTATE, "internal: the program names more than %d buffers", ProgramBufs::kMax);
    for (int i = 0; i < l.n; i++) {
        const Buf& b = l.b[i];
        const hipError_t e = b.pinned ? hipHostMalloc(b.slot, b.bytes, hipHostMallocDefault) : hipMalloc(b.slot, b.bytes);
        if (e != hipSuccess) {
            *b.slot = nullptr;
            return fail(p, ORB_EHIP, "%s of %s (%zu bytes) failed: %s", b.pinned ? "hipHostMalloc" : "hipMalloc", b.name, b.bytes, hipGetErrorString(e));
        }
        if (b.cleared) HIP_TRY(p, hipMemset(*b.slot, 0, b.bytes));
    }
    memset(p->h_count, 0, kSingleCountWords * sizeof(uint32_t));
    p->d_counts = p->out_counts[0];
    p->d_corners = p->out_corners[0];
    p->d_desc = p->out_desc[0];
    return ORB_OK;
}

// The constant tables and the two kernels that derive a table from them, on the program's stream
int create_tables(OrbProgram* p) {
    HIP_TRY(p, hipMemcpy(p->d_pattern, ORB_BRIEF_PATTERN, 1024, hipMemcpyHostToDevice));
    HIP_TRY(p, hipMemcpy(p->d_cos, ORB_COS_BITS, ORB_ANGLE_STEPS_FULL * 4, hipMemcpyHostToDevice));
    HIP_TRY(p, hipMemcpy(p->d_sin, ORB_SIN_BITS, ORB_ANGLE_STEPS_FULL * 4, hipMemcpyHostToDevice));
    const bool fi = p->plan.fused_i;  // the pattern rotated by every angle code, for k_brief_i's window or k_brief_nf's patch (rot_codes)
    hipLaunchKernelGGL(k_rot_table, dim3(rot_codes(p)), dim3(64), 0, p->stream, p->d_pattern, p->d_cos, p->d_sin, fi ? (int)p->plan.itiles.pitch : kNfPatchCols,
                       fi ? 1 : 0, p->d_rot, p->opt.fp_contract, fi ? p->opt.angle_bins : 0u);
    HIP_TRY(p, hipGetLastError());
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    if (p->d_blur_tab) {
        const FrontGeom g = blur_tab_geometry(p);
        HIP_TRY(p, hipMemsetAsync(p->d_blur_tab, 0, (size_t)blur_col_pieces(g.n_var) * sizeof(uint4), p->stream));  // an odd n_var ends in the middle of a piece
        hipLaunchKernelGGL(k_blur_col_table<>, dim3((g.n_var + 63u) / 64u), dim3(64), 0, p->stream, p->plan.pyr.w[0], g.blur_p, g.blur_q, g.n_var, p->plan.wq,
                           reinterpret_cast<BlurCol*>(p->d_blur_tab));
        HIP_TRY(p, hipGetLastError());
        HIP_TRY(p, hipStreamSynchronize(p->stream));
    }
    return ORB_OK;
}

// Device-visible addresses of the staging arrays, once (null: the runtime cannot map them -> the three copies of orb.rs:537-547)
void create_staging_pointers(OrbProgram* p) {
    void *dc = nullptr, *dk = nullptr, *dd = nullptr;
    if (hipHostGetDevicePointer(&dc, p->h_count, 0) == hipSuccess && hipHostGetDevicePointer(&dk, p->h_corners, 0) == hipSuccess &&
        hipHostGetDevicePointer(&dd, p->h_desc, 0) == hipSuccess) {
        p->dv_count = static_cast<uint32_t*>(dc);
        p->dv_corners = static_cast<CornerData*>(dk);
        p->dv_desc = static_cast<CornerDescriptor*>(dd);
    } else {
        (void)hipGetLastError();
    }
}

}  // namespace

extern "C" {

uint32_t orb_abi_version(void) { return TINYORB_ABI_VERSION; }

const char* orb_last_error(const OrbProgram* p) { return p ? p->err.c_str() : g_create_error.c_str(); }

const char* orb_pipeline(const OrbProgram* p) { return p ? ((p->plan.fused || p->plan.fused_i || p->plan.fused_x) ? "fused" : "staged") : ""; }

const char* orb_pipeline_note(const OrbProgram* p) { return p ? p->plan.pipeline_note.c_str() : ""; }

const char* orb_kernel_name(int id) { return (id >= 0 && id < ORB_KERNEL_COUNT) ? kKernelNames[id] : ""; }

int orb_program_create(const OrbConfig* config, const OrbOptions* options, OrbProgram** out) {
    if (!out) return fail(nullptr, ORB_EINVAL, "out is NULL");
    *out = nullptr;
    if (const char* msg = check_config(config, options)) return fail(nullptr, ORB_EINVAL, "%s", msg);
    OrbProgram* p = new (std::nothrow) OrbProgram();
    if (!p) return fail(nullptr, ORB_EINVAL, "out of host memory");
    p->cfg = *config;
    if (options) p->opt = *options;
    p->device = p->opt.device;
    p->threshold = config->initial_threshold;  // orb.rs:178
    p->env = read_plan_env(p->opt.flags);
    int rc = create_device(p);
    if (!rc) {
        p->plan = plan_program(p->cfg, p->opt, p->max_lds, p->env);
        rc = create_attributes(p);
    }
    if (!rc) {
        create_say(p);
        rc = create_buffers(p);
    }
    if (!rc) rc = create_tables(p);
    if (rc) {
        g_create_error = p->err;
        orb_program_destroy(p);
        return rc;
    }
    create_staging_pointers(p);
    *out = p;
    return ORB_OK;
}

void orb_program_destroy(OrbProgram* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    const auto drop = [](hipEvent_t ev) {
        if (ev) (void)hipEventDestroy(ev);
    };
    for (auto& sp : p->pending) drop(sp.start), drop(sp.stop);
    for (hipEvent_t ev : p->event_pool) drop(ev);
    (void)hipFree(p->d_input);  // these two and the pack buffers: allocated on first use
    (void)hipFree(p->d_input_alt);
    for (hipEvent_t ev : p->in_uploaded) drop(ev);
    free_bufs(program_buffers(p));
    for (int st = 0; st < ST_COUNT; st++) {
        free_stage_buffers(p, st);
        drop(p->stage[st].done);
    }
    drop(p->single_done_ev);
    drop(p->place_copied);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
    drop(p->order_event);
    for (hipEvent_t ev : p->upload_events) drop(ev);
    drop(p->upload_done);
    for (int set = 0; set < 2; set++) {
        (void)hipFree(p->d_pack_c[set]);
        (void)hipFree(p->d_pack_d[set]);
        if (p->h_pack_counts[set]) (void)hipHostFree(p->h_pack_counts[set]);
        if (p->h_pack_offsets[set]) (void)hipHostFree(p->h_pack_offsets[set]);
        drop(p->pack_event[set]);
    }
    delete p;
}

// Slab an image written now goes to, and its place in the queue of images waiting for extract_corners (at most two: the
// one being extracted next and the one uploaded under it).  With nothing pending the slab of the last extract is reused.
// ahead = false (the blocking write, the reference's): the last write wins -- an image that is still waiting is overwritten,
// the queue never grows past one.  ahead = true (orb_write_input_image_pinned): the image is queued behind a waiting one.
// Nothing is published here: the queue, the pending count and the slab's "came through the copy stream" mark change only once the image
// is really on its way (publish_input_slab), so that a failed allocation, event creation or copy leaves the program as it was.
static int pick_input_slab(OrbProgram* p, bool ahead, uint32_t* slab_out, uint8_t** dst, bool* appended) {
    if (ahead && p->in_pending >= 2u)
        return fail(p, ORB_ESTATE, "two images are already waiting for extract_corners");
    if (int rc = ensure_input(p)) return rc;
    uint32_t slab;
    if (p->in_pending == 0u || ahead) {
        slab = p->in_pending == 0u ? p->in_last : (p->in_queue[0] ^ 1u);
        *appended = true;
    } else {
        slab = p->in_queue[p->in_pending - 1u];  // overwrite the newest waiting image
        if (p->in_async[slab]) HIP_TRY(p, hipEventSynchronize(p->in_uploaded[slab]));  // its upload must not land on top of this one
        *appended = false;
    }
    if (slab == 1u && !p->d_input_alt) HIP_TRY(p, hipMalloc(&p->d_input_alt, p->plan.frame_bytes));
    *slab_out = slab;
    *dst = slab ? p->d_input_alt : p->d_input;
    return ORB_OK;
}
static void publish_input_slab(OrbProgram* p, uint32_t slab, bool appended, bool async) {
    if (appended) p->in_queue[p->in_pending++] = slab;
    p->in_async[slab] = async;
}
// A copy into a slab that was already queued (the blocking write overwrites the newest waiting image) failed half-way: that image
// is gone, the queue must not name it any more.
static void drop_newest_input(OrbProgram* p, bool appended) {
    if (!appended && p->in_pending) p->in_pending--;
}

int orb_write_input_image(OrbProgram* p, const uint8_t* bytes, size_t len) {
    if (!p) return ORB_EINVAL;
    if (!bytes || len != p->plan.frame_bytes)
        return fail(p, ORB_EINVAL, "write_input_image: expected %zu bytes (4*W*H), got %zu", p->plan.frame_bytes, len);
    HIP_TRY(p, hipSetDevice(p->device));
    uint32_t slab = 0;
    uint8_t* dst = nullptr;
    bool appended = false;
    if (int rc = pick_input_slab(p, false, &slab, &dst, &appended)) return rc;
    hipError_t e = hipMemcpyAsync(dst, bytes, len, hipMemcpyHostToDevice, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);  // the caller's slice may be reused right away
    if (e != hipSuccess) {
        drop_newest_input(p, appended);
        return fail(p, ORB_EHIP, "write_input_image: the upload failed: %s", hipGetErrorString(e));
    }
    publish_input_slab(p, slab, appended, false);
    return ORB_OK;
}

int orb_write_input_image_pinned(OrbProgram* p, const uint8_t* bytes_pinned, size_t len) {
    if (!p) return ORB_EINVAL;
    if (!bytes_pinned || len != p->plan.frame_bytes)
        return fail(p, ORB_EINVAL, "write_input_image_pinned: expected %zu bytes, got %zu", p->plan.frame_bytes, len);
    HIP_TRY(p, hipSetDevice(p->device));
    uint32_t slab = 0;
    uint8_t* dst = nullptr;
    bool appended = false;
    if (int rc = pick_input_slab(p, true, &slab, &dst, &appended)) return rc;
    if (!p->copy_stream) HIP_TRY(p, hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking));
    if (!p->in_uploaded[slab]) HIP_TRY(p, hipEventCreateWithFlags(&p->in_uploaded[slab], hipEventDisableTiming));
    if (!p->upload_done) HIP_TRY(p, hipEventCreateWithFlags(&p->upload_done, hipEventDisableTiming));
    // The slab is free: the extract that last read it has returned (extract_corners blocks).  The copy runs on the copy
    // stream, beside the kernels of the image extracted meanwhile; extract_corners orders its kernels behind it.
    HIP_TRY(p, hipMemcpyAsync(dst, bytes_pinned, len, hipMemcpyHostToDevice, p->copy_stream));
    HIP_TRY(p, hipEventRecord(p->in_uploaded[slab], p->copy_stream));
    HIP_TRY(p, hipEventRecord(p->upload_done, p->copy_stream));  // orb_upload_sync(): the host array may be reused
    publish_input_slab(p, slab, appended, true);  // only now: every call above succeeded, the image is on its way
    return ORB_OK;
}

int orb_set_threshold(OrbProgram* p, float threshold) {
    if (!p) return ORB_EINVAL;
    if (!(threshold >= 0.f)) return fail(p, ORB_EINVAL, "threshold must be >= 0");
    p->threshold = threshold;
    return ORB_OK;
}

int orb_extract_corners(OrbProgram* p, uint32_t* corner_count) {
    if (!p) return ORB_EINVAL;
    if (!corner_count) return fail(p, ORB_EINVAL, "corner_count is NULL");
    HIP_TRY(p, hipSetDevice(p->device));
    if (int rc = ensure_input(p)) return rc;
    hipStream_t s = p->stream;
    const size_t cap = p->cfg.max_features;
    // the oldest image written and not yet extracted; with none pending, the last one again (as the reference would)
    uint32_t slab = p->in_last;
    if (p->in_pending) {
        slab = p->in_queue[0];
        p->in_queue[0] = p->in_queue[1];
        p->in_pending--;
        p->in_last = slab;
    }
    const uint8_t* const d_in = slab ? p->d_input_alt : p->d_input;
    if (p->in_async[slab]) {  // uploaded on the copy stream (orb_write_input_image_pinned)
        HIP_TRY(p, hipStreamWaitEvent(s, p->in_uploaded[slab], 0));
        p->in_async[slab] = false;
    }
    // orb.rs:537-547: counter, corners and descriptors go to host staging, then block.  The reference copies the three
    // whole buffers; here a kernel writes the counter and the STORED records into the (pinned, device-visible) staging
    // memory: no size has to reach the host first, and 48 bytes per keypoint cross PCIe instead of 48 * max_features.
    // What lies behind the stored records in the staging arrays is stale, as it is in the reference's buffers.
    void *dc = p->dv_count, *dk = p->dv_corners, *dd = p->dv_desc;
    const bool direct = !p->env.single_memcpy && dc != nullptr;
    if (direct && p->plan.fused && p->plan.use_brief_t && p->plan.oob == kOobZero && !p->env.single_split) {  // k_brief_one is built for the default policy
        // Three launches per frame: one k_front per level, then k_brief_one -- slot prefix, both BRIEF kernels and the
        // write to host staging in one (a dependent launch costs 6-10 us whatever it does, and this call is the
        // reference's only shape).
        // Levels 0 and 1 in ONE launch when level 1 can build its rows from the frame (k_front_pair): RGBA or Y8 input, level 1 an
        // exact half of a level 0 whose width is a multiple of 8, both on full-width bands of 8 rows (the latency shape).
        const Pyramid& py = p->plan.pyr;
        const bool pair_ok = py.depth >= 2u && py.w[0] == 2u * py.w[1] && py.h[0] == 2u * py.h[1] && (py.w[0] & 7u) == 0u &&
                             p->plan.tile_w_lvl[0] == 0u && p->plan.tile_w_lvl[1] == 0u && p->plan.band_rows_lvl[0] == 8u && p->plan.band_rows_lvl[1] == 8u &&
                             !p->d_stamps && !p->env.single_serial &&
                             // a band stages a row with one thread per four texels (level 1 from the frame: per four of ITS texels):
                             // both rows must fit the 1024 threads, else no thread would stage anything (orb_front_body.inc)
                             (py.w[0] >> 2) <= (uint32_t)kFrontThreadsL0 &&
                             ((((std::max(py.w[1], ((py.w[0] / 2u + 7u) / 8u) * 8u) + 4u + 7u) & ~7u)) >> 2) <= (uint32_t)kFrontThreadsL0;
        if (pair_ok) {
            FrontGeom g[2];
            uint32_t width = py.w[0], height = py.h[0], lds = 0;
            for (uint32_t lvl = 0; lvl < 2u; lvl++) {
                const uint32_t gw = ((width + 7u) / 8u) * 8u, gh = ((height + 7u) / 8u) * 8u;
                width /= 2u;
                height /= 2u;
                g[lvl] = front_geometry(py, lvl, gw ? gw : 8u, gh, 1, 8u, 0u);
                if (gw == 0) g[lvl].gh = 0;
                g[lvl].slot_base = p->plan.bands.slot_base[lvl];
                g[lvl].n_slots = p->plan.bands.n_slots;
                g[lvl].seg_cap = p->plan.bands.seg_cap;
                g[lvl].n_classes = p->plan.seg_classes;
                g[lvl].xcd_swizzle = 0u;
                g[lvl].wq = p->plan.wq;
                g[lvl].fp = p->opt.fp_contract;
                g[lvl].blur_tab = front_blur_tab(p, g[lvl]);
                if (p->env.phase_mask >= 0) g[lvl].phase_mask = (uint32_t)p->env.phase_mask;
                lds = std::max(lds, front_lds_bytes(g[lvl]));
            }
            // a level-1 band stages a row with one thread per four texels, a level-0 band with one per quad (orb_front_body.inc)
            if (lds > p->max_lds || ((g[1].ls - (uint32_t)kLdsPad) >> 2) > (uint32_t)kFrontThreadsL0 || (py.w[0] >> 2) > (uint32_t)kFrontThreadsL0)
                return fail(p, ORB_EINVAL, "internal: k_front_pair does not fit this frame (%u bytes of LDS, %u columns)", lds, py.w[0]);
            {
                LaunchScope ls(p, s, KID_FUSED_L0);
                const FrontPairLaunch PL{d_in, p->plan.frame_bytes, p->d_gray, p->d_blur, p->d_blur_rowc, py, g[0], g[1], p->threshold, p->d_seg_counts, p->d_seg, s, lds,
                                         p->plan.input_y8};
                const hipError_t e = kFrontPairLaunch[front_form(p->opt.fp_contract, !p->plan.input_y8)](PL);
                if (e != hipSuccess) return fail(p, ORB_EHIP, "k_front_pair failed to launch: %s", hipGetErrorString(e));
            }
            if (py.depth > 2u)
                if (int rc = run_fused_range(p, d_in, 0, 1, s, false, 2u)) return rc;
        } else if (int rc = run_fused_range(p, d_in, 0, 1, s, false)) {
            return rc;
        }
        const uint32_t seq = ++p->single_seq ? p->single_seq : ++p->single_seq;  // never 0
        {
            LaunchScope ls(p, s, KID_BRIEF_ONE);
#define BRIEF_ONE_LAUNCH(ROT_)                                                                                                                                  \
    hipLaunchKernelGGL(k_brief_one<ROT_>, dim3((unsigned)((cap + kBriefOneChunk - 1u) / kBriefOneChunk)), dim3(kBriefOneThreads), brieft_lds_bytes(p->plan.brieft), s, \
                       p->d_blur, p->d_blur_rowc, p->plan.pyr, p->plan.brieft, p->d_seg_counts, p->d_seg_before, p->d_seg, p->d_counts, p->d_corners, (uint32_t)cap,      \
                       p->d_desc, BriefTables{p->d_pattern, p->d_cos, p->d_sin, p->d_rot}, static_cast<uint32_t*>(dc), static_cast<CornerData*>(dk),            \
                       static_cast<CornerDescriptor*>(dd), p->d_single_done, seq)
            switch (rot_form(p->opt.fp_contract)) {  // the rotation's form (OrbOptions::fp_contract)
                case 1: BRIEF_ONE_LAUNCH(1); break;
                case 2: BRIEF_ONE_LAUNCH(2); break;
                default: BRIEF_ONE_LAUNCH(0); break;
            }
#undef BRIEF_ONE_LAUNCH
        }
        HIP_TRY(p, hipGetLastError());
        if (p->env.single_block) {
            if (!p->single_done_ev) HIP_TRY(p, hipEventCreateWithFlags(&p->single_done_ev, hipEventBlockingSync | hipEventDisableTiming));
            HIP_TRY(p, hipEventRecord(p->single_done_ev, s));
        }
        p->planes_valid = true;
        // Block (orb.rs:549): the last workgroup of k_brief_one to finish publishes the call's sequence number in pinned memory
        // behind everything the launch wrote there, and the host polls that word -- hipStreamSynchronize costs 5 us more
        // than the poll (tools/ubench/launch_floor.hip: 11.6 against 6.5 us for an empty launch).  The poll gives up after
        // 20 ms (a faulted kernel never publishes) and a stream synchronisation reports what happened.
        // A host thread that spins on a shared box now and then loses its CPU for a scheduler slice (two to four iterations of 200
        // take 20 ms, NOTEBOOK.md): with TINYORB_SINGLE_WAIT=block / ORB_FLAG_SINGLE_BLOCKING_WAIT the spin is bounded (kSingleSpinUs: the call
        // normally completes inside it) and the thread then SLEEPS in hipEventSynchronize on a blocking-sync event recorded behind the launch
        // -- woken by the completion interrupt, as the reference's device.poll(Wait) is (orb.rs:547).
        bool seen = false;
        constexpr int kSingleSpinUs = 50;
        if (!p->profiling && !p->env.single_sync) {
            const volatile uint32_t* const done = p->h_count + kSingleDoneWord;
            const auto t0 = std::chrono::steady_clock::now();
            const auto limit = p->env.single_block ? std::chrono::microseconds(kSingleSpinUs) : std::chrono::microseconds(20000);
            const uint32_t check = p->env.single_block ? 63u : 1023u;
            for (uint32_t spins = 0; !(seen = __atomic_load_n(done, __ATOMIC_ACQUIRE) == seq); spins++)
                if ((spins & check) == check && std::chrono::steady_clock::now() - t0 > limit) break;
            if (!seen && p->env.single_block) {
                HIP_TRY(p, hipEventSynchronize(p->single_done_ev));  // sleeps; the kernel is over when it returns, its stores are in host memory
                seen = __atomic_load_n(done, __ATOMIC_ACQUIRE) == seq;
            }
        }
        if (!seen) {
            HIP_TRY(p, hipStreamSynchronize(s));
            // not published within 20 ms (or polling is off): whatever happened, the launch is over now -- a launch that
            // was cut short must not leave its workgroup count behind for the next call to add to
            if (!p->profiling && !p->env.single_sync) HIP_TRY(p, hipMemsetAsync(p->d_single_done, 0, sizeof(uint32_t), s));
        }
#ifdef TINYORB_STAMPS
        if (getenv("TINYORB_PRINT_STAMPS")) {  // k_brief_one's joints, workgroups 0 and 24, in units of 10 ns
            fprintf(stderr, "k_brief_one stamps (load+stage, scan, flat body, other body, fence) x 10 ns:");
            for (int i = 1; i <= 10; i++) fprintf(stderr, " %u%s", p->h_count[i], i == 5 ? " |" : "");
            fprintf(stderr, "\n");
        }
#endif
        p->single_valid = true;
        p->last_batch = 1;
        p->batch_seq++;
        p->last_stream = s;
        *corner_count = *p->h_count;  // raw counter, orb.rs:550-556
        if (*corner_count > cap) return fail(p, ORB_ECAPACITY, "%u corners detected, max_features is %zu", *corner_count, cap);
        return ORB_OK;
    }
    if (int rc = run_pipeline(p, d_in, 1, s)) return rc;
    if (direct) {
        p->last_batch = 1;
        p->batch_seq++;
        p->last_stream = s;
        if (int rc = launch_compact(p, 1, static_cast<uint32_t*>(dc), nullptr, static_cast<CornerData*>(dk),
                                    static_cast<CornerDescriptor*>(dd), cap, s, nullptr))
            return rc;
    } else {
        (void)hipGetLastError();
        HIP_TRY(p, hipMemcpyAsync(p->h_count, p->d_counts, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(p, hipMemcpyAsync(p->h_corners, p->d_corners, cap * sizeof(CornerData), hipMemcpyDeviceToHost, s));
        HIP_TRY(p, hipMemcpyAsync(p->h_desc, p->d_desc, cap * sizeof(CornerDescriptor), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(p, hipStreamSynchronize(s));
    p->single_valid = true;
    p->last_batch = 1;
    p->batch_seq++;
    p->last_stream = s;
    *corner_count = *p->h_count;  // raw counter, orb.rs:550-556
    if (*corner_count > cap) return fail(p, ORB_ECAPACITY, "%u corners detected, max_features is %zu", *corner_count, cap);
    return ORB_OK;
}

int orb_read_corners(OrbProgram* p, CornerData* dst, size_t n) {
    if (!p) return ORB_EINVAL;
    if (!dst && n) return fail(p, ORB_EINVAL, "dst is NULL");
    if (!p->single_valid) return fail(p, ORB_ESTATE, "read_corners before extract_corners");
    const size_t cap = p->cfg.max_features;
    memcpy(dst, p->h_corners, (n < cap ? n : cap) * sizeof(CornerData));
    return ORB_OK;
}

int orb_read_descriptors(OrbProgram* p, CornerDescriptor* dst, size_t n) {
    if (!p) return ORB_EINVAL;
    if (!dst && n) return fail(p, ORB_EINVAL, "dst is NULL");
    if (!p->single_valid) return fail(p, ORB_ESTATE, "read_descriptors before extract_corners");
    const size_t cap = p->cfg.max_features;
    memcpy(dst, p->h_desc, (n < cap ? n : cap) * sizeof(CornerDescriptor));
    return ORB_OK;
}

int orb_extract_batch_device(OrbProgram* p, const uint8_t* frames_dev, uint32_t n_frames, void* stream) {
    if (!p) return ORB_EINVAL;
    if (!frames_dev) return fail(p, ORB_EINVAL, "frames_dev is NULL");
    if (n_frames == 0 || n_frames > p->plan.max_batch)
        return fail(p, ORB_EINVAL, "n_frames %u outside 1..=max_batch (%u)", n_frames, p->plan.max_batch);
    HIP_TRY(p, hipSetDevice(p->device));
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    if (int rc = run_pipeline(p, frames_dev, n_frames, s)) return rc;
    p->last_batch = n_frames;
    p->batch_seq++;
    p->last_stream = s;
    p->single_valid = false;
    return ORB_OK;
}

// Chunked upload of pinned host frames on the copy stream, the kernels of chunk c running while chunk c+1 is still
// crossing PCIe (only the fused path can work on a sub-range of the batch).  Asynchronous.
static int upload_chunked_and_run(OrbProgram* p, const uint8_t* frames_pinned, uint32_t n_frames, hipStream_t s) {
    const uint32_t chunk = 16;
    const size_t total = p->plan.frame_bytes * n_frames;
    if (!p->upload_done) HIP_TRY(p, hipEventCreateWithFlags(&p->upload_done, hipEventDisableTiming));
    if (!p->plan.fused || n_frames <= chunk) {
        HIP_TRY(p, hipMemcpyAsync(p->d_input, frames_pinned, total, hipMemcpyHostToDevice, s));
        HIP_TRY(p, hipEventRecord(p->upload_done, s));
        return run_pipeline(p, p->d_input, n_frames, s);
    }
    if (!p->copy_stream) HIP_TRY(p, hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking));
    const size_t n_chunks = (n_frames + chunk - 1) / chunk;
    while (p->upload_events.size() < n_chunks) {
        hipEvent_t ev = nullptr;
        HIP_TRY(p, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        p->upload_events.push_back(ev);
    }
    // the input slab is reused: the first upload must not overtake the kernels of the previous batch that still read it
    if (!p->order_event) HIP_TRY(p, hipEventCreateWithFlags(&p->order_event, hipEventDisableTiming));
    HIP_TRY(p, hipEventRecord(p->order_event, s));
    HIP_TRY(p, hipStreamWaitEvent(p->copy_stream, p->order_event, 0));
    for (uint32_t c = 0, f0 = 0; f0 < n_frames; c++, f0 += chunk) {
        const uint32_t m = n_frames - f0 < chunk ? n_frames - f0 : chunk;
        HIP_TRY(p, hipMemcpyAsync(p->d_input + (size_t)f0 * p->plan.frame_bytes, frames_pinned + (size_t)f0 * p->plan.frame_bytes,
                                  (size_t)m * p->plan.frame_bytes, hipMemcpyHostToDevice, p->copy_stream));
        HIP_TRY(p, hipEventRecord(p->upload_events[c], p->copy_stream));
        HIP_TRY(p, hipStreamWaitEvent(s, p->upload_events[c], 0));
        if (int rc = run_fused_range(p, p->d_input, f0, m, s)) return rc;
    }
    HIP_TRY(p, hipEventRecord(p->upload_done, p->copy_stream));
    p->planes_valid = true;
    return ORB_OK;
}

int orb_extract_batch_pinned(OrbProgram* p, const uint8_t* frames_pinned, uint32_t n_frames) {
    if (!p) return ORB_EINVAL;
    if (!frames_pinned) return fail(p, ORB_EINVAL, "frames_pinned is NULL");
    if (n_frames == 0 || n_frames > p->plan.max_batch)
        return fail(p, ORB_EINVAL, "n_frames %u outside 1..=max_batch (%u)", n_frames, p->plan.max_batch);
    HIP_TRY(p, hipSetDevice(p->device));
    if (int rc = ensure_input(p)) return rc;
    if (int rc = upload_chunked_and_run(p, frames_pinned, n_frames, p->stream)) return rc;
    p->last_batch = n_frames;
    p->batch_seq++;
    p->last_stream = p->stream;
    p->single_valid = false;
    return ORB_OK;
}

int orb_upload_sync(OrbProgram* p) {
    if (!p) return ORB_EINVAL;
    HIP_TRY(p, hipSetDevice(p->device));
    if (p->upload_done) HIP_TRY(p, hipEventSynchronize(p->upload_done));  // recorded behind the last upload
    return ORB_OK;
}

int orb_extract_batch_host(OrbProgram* p, const uint8_t* frames_host, uint32_t n_frames) {
    if (!p) return ORB_EINVAL;
    if (!frames_host) return fail(p, ORB_EINVAL, "frames_host is NULL");
    if (n_frames == 0 || n_frames > p->plan.max_batch)
        return fail(p, ORB_EINVAL, "n_frames %u outside 1..=max_batch (%u)", n_frames, p->plan.max_batch);
    HIP_TRY(p, hipSetDevice(p->device));
    if (int rc = ensure_input(p)) return rc;
    hipStream_t s = p->stream;
    // Ingest (README.md:42 of the reference): the caller's frames are pinned in place for the
    // duration of the call and uploaded in chunks on a copy stream; the kernels of chunk c run while chunk c+1 is
    // still crossing PCIe.
    const size_t total = p->plan.frame_bytes * n_frames;
    const bool pinned = hipHostRegister(const_cast<uint8_t*>(frames_host), total, hipHostRegisterDefault) == hipSuccess;
    if (!pinned) (void)hipGetLastError();
    int rc = ORB_OK;
    if (!pinned) {  // pageable source: the copy is staged by the runtime
        hipError_t e = hipMemcpyAsync(p->d_input, frames_host, total, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) rc = fail(p, ORB_EHIP, "upload failed: %s", hipGetErrorString(e));
        if (!rc) rc = run_pipeline(p, p->d_input, n_frames, s);
    } else {
        rc = upload_chunked_and_run(p, frames_host, n_frames, s);
        // the host pages must stay pinned until the last upload has finished
        if (p->upload_done && hipEventSynchronize(p->upload_done) != hipSuccess && !rc) rc = fail(p, ORB_EHIP, "upload sync failed");
        if (rc) (void)hipStreamSynchronize(s), (void)(p->copy_stream && hipStreamSynchronize(p->copy_stream));
        (void)hipHostUnregister(const_cast<uint8_t*>(frames_host));
    }
    if (rc) return rc;
    p->last_batch = n_frames;
    p->batch_seq++;
    p->last_stream = s;
    p->single_valid = false;
    return ORB_OK;
}

int orb_batch_sync(OrbProgram* p) {
    if (!p) return ORB_EINVAL;
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipStreamSynchronize(call_stream(p, nullptr)));
    return ORB_OK;
}

int orb_batch_counts(OrbProgram* p, uint32_t* totals, uint32_t n_frames) {
    if (!p) return ORB_EINVAL;
    if (!totals || n_frames > p->last_batch) return fail(p, ORB_EINVAL, "batch_counts: bad arguments");
    if (int rc = orb_batch_sync(p)) return rc;
    HIP_TRY(p, hipMemcpy(totals, p->d_counts, sizeof(uint32_t) * n_frames, hipMemcpyDeviceToHost));
    return ORB_OK;
}

int orb_batch_read(OrbProgram* p, uint32_t frame, CornerData* corners, CornerDescriptor* descriptors, size_t n) {
    if (!p) return ORB_EINVAL;
    if (frame >= p->last_batch) return fail(p, ORB_EINVAL, "batch_read: frame %u not in the last batch", frame);
    if (int rc = orb_batch_sync(p)) return rc;
    const size_t cap = p->cfg.max_features;
    if (n > cap) n = cap;
    if (corners)
        HIP_TRY(p, hipMemcpy(corners, p->d_corners + (size_t)frame * cap, n * sizeof(CornerData), hipMemcpyDeviceToHost));
    if (descriptors)
        HIP_TRY(p, hipMemcpy(descriptors, p->d_desc + (size_t)frame * cap, n * sizeof(CornerDescriptor),
                             hipMemcpyDeviceToHost));
    return ORB_OK;
}

}  // extern "C"

namespace {

// Launches k_compact for the first n frames of the last batch on `stream` (NULL: the batch's own stream); a foreign
// stream is first ordered behind the batch with an event.
int launch_compact(OrbProgram* p, uint32_t n, uint32_t* counts, uint64_t* offsets, CornerData* corners,
                   CornerDescriptor* desc, size_t capacity, void* stream, hipStream_t* used) {
    hipStream_t batch = call_stream(p, nullptr), s = call_stream(p, stream);
    if (s != batch) {
        if (!p->order_event) HIP_TRY(p, hipEventCreateWithFlags(&p->order_event, hipEventDisableTiming));
        HIP_TRY(p, hipEventRecord(p->order_event, batch));
        HIP_TRY(p, hipStreamWaitEvent(s, p->order_event, 0));
    }
    const uint32_t cap = p->cfg.max_features;
    {
        LaunchScope ls(p, s, KID_COMPACT);
        hipLaunchKernelGGL(k_compact, dim3(n, (cap + kCompactChunk - 1u) / kCompactChunk), dim3(256), 0, s, p->d_counts,
                           p->d_corners, p->d_desc, cap, n, counts, reinterpret_cast<unsigned long long*>(offsets), corners, desc,
                           (unsigned long long)capacity);
    }
    HIP_TRY(p, hipGetLastError());
    if (used) *used = s;
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_batch_compact_device(OrbProgram* p, uint32_t n_frames, uint32_t* counts_dev, uint64_t* offsets_dev,
                             CornerData* corners_dev, CornerDescriptor* descriptors_dev, size_t capacity, void* stream) {
    if (!p) return ORB_EINVAL;
    if (n_frames == 0 || n_frames > p->last_batch) return fail(p, ORB_EINVAL, "compact: n_frames %u not in the last batch (%u)", n_frames, p->last_batch);
    if (!corners_dev || !descriptors_dev) return fail(p, ORB_EINVAL, "compact: destination is NULL");
    HIP_TRY(p, hipSetDevice(p->device));
    return launch_compact(p, n_frames, counts_dev, offsets_dev, corners_dev, descriptors_dev, capacity, stream, nullptr);
}

int orb_batch_read_all(OrbProgram* p, uint32_t n_frames, uint32_t* counts, uint64_t* offsets, CornerData* corners,
                       CornerDescriptor* descriptors, size_t capacity, void* stream) {
    if (!p) return ORB_EINVAL;
    if (n_frames == 0 || n_frames > p->last_batch) return fail(p, ORB_EINVAL, "read_all: n_frames %u not in the last batch (%u)", n_frames, p->last_batch);
    if (!corners || !descriptors) return fail(p, ORB_EINVAL, "read_all: destination is NULL");
    HIP_TRY(p, hipSetDevice(p->device));
    // Device-visible addresses of the host buffers.  Pinned memory (orb_host_alloc / hipHostRegister by the caller)
    // resolves directly; anything else is registered for the duration of the call, which then has to block.
    struct Buf { void* host; size_t bytes; void* dev; bool registered; };
    Buf bufs[4] = {{counts, sizeof(uint32_t) * n_frames, nullptr, false},
                   {offsets, sizeof(uint64_t) * ((size_t)n_frames + 1u), nullptr, false},
                   {corners, sizeof(CornerData) * capacity, nullptr, false},
                   {descriptors, sizeof(CornerDescriptor) * capacity, nullptr, false}};
    bool blocking = false;
    int rc = ORB_OK;
    for (Buf& b : bufs) {
        if (!b.host || b.bytes == 0) continue;
        if (hipHostGetDevicePointer(&b.dev, b.host, 0) == hipSuccess && b.dev) continue;
        (void)hipGetLastError();
        hipError_t e = hipHostRegister(b.host, b.bytes, hipHostRegisterMapped);
        if (e == hipSuccess) {
            b.registered = true;
            e = hipHostGetDevicePointer(&b.dev, b.host, 0);
        }
        if (e != hipSuccess) {
            rc = fail(p, ORB_EHIP, "read_all: host buffer cannot be made device-visible: %s", hipGetErrorString(e));
            break;
        }
        blocking = true;
    }
    hipStream_t used = nullptr;
    if (!rc)
        rc = launch_compact(p, n_frames, (uint32_t*)bufs[0].dev, (uint64_t*)bufs[1].dev, (CornerData*)bufs[2].dev,
                            (CornerDescriptor*)bufs[3].dev, capacity, stream, &used);
    if (blocking || rc) {
        if (used && hipStreamSynchronize(used) != hipSuccess && !rc) rc = fail(p, ORB_EHIP, "read_all: stream sync failed");
        for (Buf& b : bufs)
            if (b.registered) (void)hipHostUnregister(b.host);
    }
    return rc;
}

int orb_batch_pack(OrbProgram* p, uint32_t n_frames, void* stream) {
    if (!p) return ORB_EINVAL;
    if (n_frames == 0 || n_frames > p->last_batch) return fail(p, ORB_EINVAL, "pack: n_frames %u not in the last batch (%u)", n_frames, p->last_batch);
    HIP_TRY(p, hipSetDevice(p->device));
    const uint32_t set = p->cur_set;
    const size_t B = p->plan.max_batch, cap = p->cfg.max_features;
    if (!p->d_pack_c[set]) {
        HIP_TRY(p, hipMalloc(&p->d_pack_c[set], B * cap * sizeof(CornerData)));
        HIP_TRY(p, hipMalloc(&p->d_pack_d[set], B * cap * sizeof(CornerDescriptor)));
        HIP_TRY(p, hipHostMalloc(&p->h_pack_counts[set], B * sizeof(uint32_t), hipHostMallocMapped));
        HIP_TRY(p, hipHostMalloc(&p->h_pack_offsets[set], (B + 1u) * sizeof(uint64_t), hipHostMallocMapped));
        HIP_TRY(p, hipEventCreateWithFlags(&p->pack_event[set], hipEventDisableTiming));
    }
    void *dc = nullptr, *dof = nullptr;
    HIP_TRY(p, hipHostGetDevicePointer(&dc, p->h_pack_counts[set], 0));
    HIP_TRY(p, hipHostGetDevicePointer(&dof, p->h_pack_offsets[set], 0));
    hipStream_t used = nullptr;
    if (int rc = launch_compact(p, n_frames, (uint32_t*)dc, (uint64_t*)dof, p->d_pack_c[set], p->d_pack_d[set], B * cap, stream, &used))
        return rc;
    HIP_TRY(p, hipEventRecord(p->pack_event[set], used));
    p->pack_n[set] = n_frames;
    return ORB_OK;
}

int orb_batch_fetch(OrbProgram* p, uint32_t set, uint32_t* counts, uint64_t* offsets, CornerData* corners,
                    CornerDescriptor* descriptors, size_t capacity, void* stream) {
    if (!p) return ORB_EINVAL;
    if (set > 1u || !p->pack_event[set] || p->pack_n[set] == 0u) return fail(p, ORB_ESTATE, "fetch: output set %u has not been packed", set);
    if (!corners || !descriptors) return fail(p, ORB_EINVAL, "fetch: destination is NULL");
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipEventSynchronize(p->pack_event[set]));  // the sizes are on the host now
    const uint32_t n = p->pack_n[set];
    if (counts) memcpy(counts, p->h_pack_counts[set], n * sizeof(uint32_t));
    if (offsets) memcpy(offsets, p->h_pack_offsets[set], ((size_t)n + 1u) * sizeof(uint64_t));
    const uint64_t total = p->h_pack_offsets[set][n];
    const size_t m = total < capacity ? (size_t)total : capacity;
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    if (m) {
        HIP_TRY(p, hipMemcpyAsync(corners, p->d_pack_c[set], m * sizeof(CornerData), hipMemcpyDeviceToHost, s));
        HIP_TRY(p, hipMemcpyAsync(descriptors, p->d_pack_d[set], m * sizeof(CornerDescriptor), hipMemcpyDeviceToHost, s));
    }
    return ORB_OK;
}

int orb_batch_pack_transport(OrbProgram* p, uint32_t set, uint32_t n_frames, void* dst_dev, size_t capacity_records,
                             uint64_t* offsets_dev, void* stream) {
    if (!p) return ORB_EINVAL;
    if (set > 1u || !p->out_counts[set]) return fail(p, ORB_EINVAL, "pack_transport: output set %u does not exist", set);
    if (n_frames == 0 || n_frames > p->plan.max_batch) return fail(p, ORB_EINVAL, "pack_transport: n_frames %u outside 1..=max_batch (%u)", n_frames, p->plan.max_batch);
    if (!dst_dev) return fail(p, ORB_EINVAL, "pack_transport: destination is NULL");
    if (p->plan.pyr.w[0] >= 65536u || p->plan.pyr.h[0] >= 65536u) return fail(p, ORB_EINVAL, "pack_transport: coordinates do not fit 16 bits");
    HIP_TRY(p, hipSetDevice(p->device));
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    const uint32_t cap = p->cfg.max_features;
    {
        LaunchScope ls(p, s, KID_PACK_T);
        hipLaunchKernelGGL(k_compact_transport, dim3(n_frames, (cap + kCompactChunk - 1u) / kCompactChunk), dim3(256), 0, s,
                           p->out_counts[set], p->out_corners[set], p->out_desc[set], cap, n_frames,
                           reinterpret_cast<unsigned long long*>(offsets_dev), static_cast<TransportRecord*>(dst_dev),
                           (unsigned long long)capacity_records);
    }
    HIP_TRY(p, hipGetLastError());
    return ORB_OK;
}

int orb_unpack_transport(OrbProgram* p, const void* src_dev, uint32_t n_segments, const uint64_t* src_first, const uint64_t* count,
                         const uint64_t* dst_first, CornerData* corners_dev, CornerDescriptor* descriptors_dev, void* stream) {
    if (!p) return ORB_EINVAL;
    if (!src_dev || !corners_dev || !descriptors_dev || (n_segments && (!src_first || !count || !dst_first)))
        return fail(p, ORB_EINVAL, "unpack_transport: NULL argument");
    HIP_TRY(p, hipSetDevice(p->device));
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    for (uint32_t s0 = 0; s0 < n_segments; s0 += (uint32_t)kUnpackSegments) {
        const uint32_t m = std::min<uint32_t>(n_segments - s0, (uint32_t)kUnpackSegments);
        UnpackGeom g{};
        unsigned long long most = 0;
        for (uint32_t i = 0; i < m; i++) {
            g.src_first[i] = src_first[s0 + i], g.count[i] = count[s0 + i], g.dst_first[i] = dst_first[s0 + i];
            most = std::max<unsigned long long>(most, g.count[i]);
        }
        if (most == 0) continue;
        const unsigned long long chunks = std::min<unsigned long long>((most + 255u) / 256u, 4096u);
        LaunchScope ls(p, s, KID_UNPACK_T);
        hipLaunchKernelGGL(k_unpack_transport, dim3((uint32_t)chunks, m), dim3(256), 0, s,
                           static_cast<const TransportRecord*>(src_dev), g, corners_dev, descriptors_dev);
    }
    HIP_TRY(p, hipGetLastError());
    return ORB_OK;
}

int orb_host_alloc(size_t nbytes, void** out) {
    if (!out || nbytes == 0) return ORB_EINVAL;
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, nbytes, hipHostMallocMapped | hipHostMallocPortable);
    if (e != hipSuccess) return fail(nullptr, ORB_EHIP, "hipHostMalloc(%zu) failed: %s", nbytes, hipGetErrorString(e));
    return ORB_OK;
}

void orb_host_free(void* ptr) {
    if (ptr) (void)hipHostFree(ptr);
}

int orb_stream_sync(OrbProgram* p, void* stream) {
    if (!p) return ORB_EINVAL;
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipStreamSynchronize(stream ? (hipStream_t)stream : p->stream));
    return ORB_OK;
}

void* orb_program_stream(OrbProgram* p) { return p ? (void*)p->stream : nullptr; }

}  // extern "C"

extern "C" {

void orb_corner_level0_xy(const CornerData* c, float* x0, float* y0) {
    if (!c || !x0 || !y0) return;
    const float s = (float)(1u << (c->octave & 31u));
    *x0 = ((float)c->x + 0.5f) * s - 0.5f;
    *y0 = ((float)c->y + 0.5f) * s - 0.5f;
}

}  // extern "C"

namespace {

// Which matcher, read once per program: 0 the block-scaled fp4 form on the matrix cores (default), 1 the vector unit
// (TINYORB_MATCH_VALU=1), 2 the int8 form (TINYORB_MATCH_I8=1; orb_match_pairs has none and takes fp4)
int match_form(OrbProgram* p) {
    if (p->match_valu < 0) {
        const char* e = getenv("TINYORB_MATCH_VALU");
        const char* e8 = getenv("TINYORB_MATCH_I8");
        p->match_valu = (e && atoi(e) != 0) ? 1 : ((e8 && atoi(e8) != 0) ? 2 : 0);
    }
    return p->match_valu;
}

}  // namespace

extern "C" {

int orb_match_consecutive(OrbProgram* p, uint32_t n_frames, void* stream) {
    if (!p) return ORB_EINVAL;
    if (n_frames < 2u || n_frames > p->last_batch)
        return fail(p, ORB_EINVAL, "match_consecutive: need 2..%u frames of the last batch", p->last_batch);
    if (p->cfg.max_features > (1u << 23)) return fail(p, ORB_EINVAL, "match_consecutive: max_features must be <= 2^23");
    HIP_TRY(p, hipSetDevice(p->device));
    const size_t cap = p->cfg.max_features;
    if (!p->d_matches) HIP_TRY(p, hipMalloc(&p->d_matches, (size_t)p->plan.max_batch * cap * sizeof(MatchRecord)));
    match_form(p);
    // The matrix-core matchers (orb_kernels_match.h) need the descriptors as signed elements: 128 (fp4) or 256 (int8) bytes per
    // record of the batch.  A capacity beyond their key's index range, or no memory for the bytes, leaves the vector-unit kernel.
    const bool i8 = p->match_valu == 2;
    bool mfma = p->match_valu != 1 && cap <= (size_t)(i8 ? kMatchMaxCap : kMatch4MaxCap);
    if (mfma && !p->d_desc8 && hipMalloc(&p->d_desc8, (size_t)p->plan.max_batch * cap * (i8 ? 256u : 128u)) != hipSuccess) {
        (void)hipGetLastError();
        p->d_desc8 = nullptr;
        mfma = false;
    }
    const dim3 grid_e((unsigned)((cap + 31u) / 32u), n_frames), grid_m(n_frames - 1u, (unsigned)((cap + kMatchQueriesPerWg - 1u) / kMatchQueriesPerWg));
    hipStream_t s;
    if (int rc = stage_begin(p, ST_MATCH, stream, 0u, &s)) return rc;  // reads no other stage's results
    if (mfma && !i8) {
        {
            LaunchScope ls(p, s, KID_DESC_EXPAND);
            hipLaunchKernelGGL(k_desc_expand4, grid_e, dim3(256), 0, s, p->d_counts, p->d_desc, (uint32_t)cap, p->d_desc8);
        }
        LaunchScope ls(p, s, KID_MATCH);
        hipLaunchKernelGGL(k_match_fp4, grid_m, dim3(64 * kMatchWaves), 0, s, p->d_counts, p->d_desc8, (uint32_t)cap, p->d_matches);
    } else if (mfma) {
        {
            LaunchScope ls(p, s, KID_DESC_EXPAND);
            hipLaunchKernelGGL(k_desc_expand, grid_e, dim3(256), 0, s, p->d_counts, p->d_desc, (uint32_t)cap, p->d_desc8);
        }
        LaunchScope ls(p, s, KID_MATCH);
        hipLaunchKernelGGL(k_match_mfma, grid_m, dim3(64 * kMatchWaves), 0, s, p->d_counts, p->d_desc8, (uint32_t)cap, p->d_matches);
    } else {
        LaunchScope ls(p, s, KID_MATCH);
        hipLaunchKernelGGL(k_match, dim3(n_frames - 1u, (unsigned)((cap + 64u * kMatchQ - 1u) / (64u * kMatchQ))), dim3(64), 0, s, p->d_counts,
                           p->d_desc, (uint32_t)cap, p->d_matches);
    }
    if (int rc = stage_end(p, ST_MATCH, s, n_frames)) return rc;
    p->last_stream = s;  // the matcher and the verifiers move the batch's stream (orb_batch_sync, orb_match_read); guided and track calls do not
    return ORB_OK;
}

int orb_match_read(OrbProgram* p, uint32_t frame, OrbMatch* dst, size_t n) {
    if (!p || !dst) return ORB_EINVAL;
    if (!p->d_matches || frame + 1u >= p->last_batch) return fail(p, ORB_EINVAL, "match_read: no matches for frame %u", frame);
    if (int rc = orb_batch_sync(p)) return rc;  // the batch's stream (the matcher moved it to its own), not the matcher's event
    const size_t cap = p->cfg.max_features;
    if (n > cap) n = cap;
    HIP_TRY(p, hipMemcpy(dst, p->d_matches + (size_t)frame * cap, n * sizeof(OrbMatch), hipMemcpyDeviceToHost));
    return ORB_OK;
}

}  // extern "C"

namespace {

// What orb_verify_consecutive and orb_verify_epipolar differ in
struct VerifierKind {
    uint32_t seed_salt;           // the draw stream's seed is lowbias32(seed ^ seed_salt)
    void (*score)(VerifyArgs);
    void (*refine)(VerifyArgs);
    StageId stage;
    bool profiled;                // launches under LaunchScope (KID_VERIFY_*)
};
const VerifierKind kHomography = {0u, k_verify_score, k_verify_refine, ST_VERIFY, true};
const VerifierKind kEpipolar = {kEpiSeedSalt, k_epi_score, k_epi_refine, ST_EPI, false};

// A RANSAC call's hypotheses, max_distance and ratio (the verifiers, localize, bridge): ORB_EINVAL out of range, else 0 becomes the default
int ransac_params(OrbProgram* p, int which, uint32_t* hypotheses, uint32_t* max_distance, float* ratio) {
    if (*hypotheses > kVerifyMaxHyp || *max_distance > 256u || !(std::isfinite(*ratio) && *ratio >= 0.0f))
        return fail(p, ORB_EINVAL, "%s: hypotheses must be 0..%u, max_distance 0..256, ratio finite and >= 0", kStages[which].name, kVerifyMaxHyp);
    if (!*hypotheses) *hypotheses = 512u;
    if (!*max_distance) *max_distance = 64u;
    if (*ratio == 0.0f) *ratio = 0.8f;
    return ORB_OK;
}

// The intrinsics of a pose, localize, landmarks or bridge call
int check_intrinsics(OrbProgram* p, int which, float fx, float fy, float cx, float cy) {
    if (!(std::isfinite(fx) && fx > 0.0f) || !(std::isfinite(fy) && fy > 0.0f) || !std::isfinite(cx) || !std::isfinite(cy))
        return fail(p, ORB_EINVAL, "%s: fx and fy must be finite and > 0, cx and cy finite", kStages[which].name);
    return ORB_OK;
}

// A read call of stage `which`: the head record of row `index` (head NULL: not asked for) and the first n elements of that row of
// max_features.  Waits for the stage's event on the host.
int read_stage(OrbProgram* p, int which, uint32_t index, void* head, const void* d_head, size_t head_bytes, void* rows, const void* d_rows,
               size_t elem_bytes, size_t n) {
    const Stage& last = p->stage[which];
    const StageInfo& k = kStages[which];
    if (!last.extent) return fail(p, ORB_ESTATE, "%s before %s", k.read_name, k.name);
    if (index >= last.extent || (!rows && n))
        return fail(p, ORB_EINVAL, "%s: index %u of %u, or the destination of %zu elements is NULL", k.read_name, index, last.extent, n);
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipEventSynchronize(last.done));
    const size_t cap = p->cfg.max_features;
    if (n > cap) n = cap;
    if (head) HIP_TRY(p, hipMemcpy(head, (const char*)d_head + (size_t)index * head_bytes, head_bytes, hipMemcpyDeviceToHost));
    if (n) HIP_TRY(p, hipMemcpy(rows, (const char*)d_rows + (size_t)index * cap * elem_bytes, n * elem_bytes, hipMemcpyDeviceToHost));
    return ORB_OK;
}

// What the consecutive verifiers and orb_verify_pairs share: the parameter block, the VerifyArgs and the three launches.  They differ
// in the gather kernel, the state, the stage, the freshness test and the extent, which stay with the two callers below.

// OrbVerifyParams checked, zero fields replaced by the defaults (params NULL: all defaults); `which` names the call in messages
int verifier_params(OrbProgram* p, int which, const OrbVerifyParams* params, OrbVerifyParams* out) {
    const char* const name = kStages[which].name;
    OrbVerifyParams v{};
    if (params) v = *params;
    if (v.reserved[0] || v.reserved[1] || v.reserved[2]) return fail(p, ORB_EINVAL, "%s: reserved words must be 0", name);
    if (int rc = ransac_params(p, which, &v.hypotheses, &v.max_distance, &v.ratio)) return rc;
    if (!(std::isfinite(v.inlier_px) && v.inlier_px >= 0.0f)) return fail(p, ORB_EINVAL, "%s: inlier_px must be finite and >= 0", name);
    if (v.inlier_px == 0.0f) v.inlier_px = 3.0f;
    *out = v;
    return ORB_OK;
}

// VerifyArgs over a set of buffers and the match rows the gather reads
VerifyArgs verifier_args(const OrbProgram* p, const VerifierKind& kind, const VerifierState& st, const OrbVerifyParams& v, const MatchRecord* matches) {
    // GV-2: coordinates centred on the level-0 image and scaled by 2 / max(W, H)
    const uint32_t W = p->plan.pyr.w[0], H = p->plan.pyr.h[0];
    VerifyArgs a{};
    a.counts = p->d_counts;
    a.corners = p->d_corners;
    a.matches = matches;
    a.cap = p->cfg.max_features;
    a.hyps = v.hypotheses;
    a.max_distance = v.max_distance;
    a.ratio = v.ratio;
    a.cx = 0.5f * (float)(W - 1u);
    a.cy = 0.5f * (float)(H - 1u);
    a.k = 2.0f / (float)(W > H ? W : H);
    const float t = v.inlier_px * a.k;
    a.t2 = t * t;
    a.seed_mix = lowbias32(v.seed ^ kind.seed_salt);
    a.rec = st.rec;
    a.cand_of = st.cand;
    a.n_cand = st.n;
    a.keys = st.keys;
    a.model = st.model;
    a.mask = st.mask;
    return a;
}

// The three launches over `pairs` rows: `gather` launches the caller's gather kernel (EP-1: GV-1 and GV-2 serve both verifiers), then
// the kind's score and refine kernels on `tail` -- the gather's arguments, or those with the counters the rows are indexed by
template <class Gather>
void verifier_launches(OrbProgram* p, hipStream_t s, const VerifierKind& kind, bool profiled, const VerifyArgs& tail, uint32_t pairs, Gather gather) {
    const auto scoped = [&](int kid, auto&& launch) {
        std::optional<LaunchScope> ls;
        if (profiled) ls.emplace(p, s, kid);
        launch();
    };
    scoped(KID_VERIFY_GATHER, gather);
    scoped(KID_VERIFY_SCORE, [&] {
        hipLaunchKernelGGL(kind.score, dim3(pairs, (tail.hyps + kVerifyHypPerWg - 1u) / kVerifyHypPerWg), dim3(256), 0, s, tail);
    });
    scoped(KID_VERIFY_REFINE, [&] { hipLaunchKernelGGL(kind.refine, dim3(pairs), dim3(256), 0, s, tail); });
}

int run_verifier(OrbProgram* p, const VerifierKind& kind, VerifierState& st, uint32_t n_frames, const OrbVerifyParams* params, void* stream) {
    const char* const name = kStages[kind.stage].name;
    OrbVerifyParams v;
    if (int rc = verifier_params(p, kind.stage, params, &v)) return rc;
    if (int rc = stages_fresh(p, kind.stage, kStages[kind.stage].reads)) return rc;
    const Stage& m = p->stage[ST_MATCH];
    if (n_frames < 2u || n_frames > m.extent) return fail(p, ORB_EINVAL, "%s: need 2..%u frames (the matched ones)", name, m.extent);
    hipStream_t s;
    if (int rc = stage_open(p, kind.stage, stream, kStages[kind.stage].reads, &s)) return rc;  // the matches come from the matcher's stream
    const VerifyArgs a = verifier_args(p, kind, st, v, p->d_matches);
    const uint32_t pairs = n_frames - 1u;
    verifier_launches(p, s, kind, kind.profiled, a, pairs, [&] { hipLaunchKernelGGL(k_verify_gather, dim3(pairs), dim3(256), 0, s, a); });
    // The batch and output set stage_end records are the matcher's, which this call read: stage_fresh(p, m) above says they are the
    // same.  Guided and track calls check them before they read the homography verifier's models and inlier bytes, the band
    // call before it reads the epipolar verifier's models.
    if (int rc = stage_end(p, kind.stage, s, pairs)) return rc;
    p->last_stream = s;  // as the matcher does
    return ORB_OK;
}

// orb_verify_pairs: the same on the list and rows of the last orb_match_pairs, into the pairs stage's own state
int run_pairs_verifier(OrbProgram* p, const VerifierKind& kind, uint32_t n_pairs, const OrbVerifyParams* params, void* stream) {
    OrbVerifyParams v;
    if (int rc = verifier_params(p, ST_PAIRS_VERIFY, params, &v)) return rc;
    if (int rc = stages_fresh(p, ST_PAIRS_VERIFY, kStages[ST_PAIRS_VERIFY].reads)) return rc;
    const Stage& m = p->stage[ST_PAIRS];
    if (n_pairs < 1u || n_pairs > m.extent) return fail(p, ORB_EINVAL, "verify_pairs: need 1..%u pairs (the matched ones)", m.extent);
    hipStream_t s;
    if (int rc = stage_open(p, ST_PAIRS_VERIFY, stream, kStages[ST_PAIRS_VERIFY].reads, &s)) return rc;
    const VerifierState& st = p->pverify;
    const VerifyArgs a = verifier_args(p, kind, st, v, p->d_prows);
    VerifyArgs tail = a;
    tail.counts = st.qcount;  // row i's queries are frame list[i].query's: the gather leaves that frame's counter at i
    verifier_launches(p, s, kind, false, tail, n_pairs,
                      [&] { hipLaunchKernelGGL(k_verify_gather_pairs, dim3(n_pairs), dim3(256), 0, s, a, (const OrbFramePair*)p->d_plist, st.qcount); });
    return stage_end(p, ST_PAIRS_VERIFY, s, n_pairs);  // p->last_stream stays, as after a guided call
}

// k_guide_bin's part of GuideArgs, for the guided and the band call: the frame's records into the cells of the program's grid
GuideArgs guide_bin_args(const OrbProgram* p, const GridSearchState& g) {
    const uint32_t W = p->plan.pyr.w[0], H = p->plan.pyr.h[0];
    GuideArgs a{};
    a.counts = p->d_counts;
    a.corners = p->d_corners;
    a.desc = p->d_desc;
    a.cap = p->cfg.max_features;
    a.shift = (uint32_t)p->guide_cell;
    a.gw = (W + (1u << a.shift) - 1u) >> a.shift;
    a.gh = (H + (1u << a.shift) - 1u) >> a.shift;
    a.srec = g.srec;
    a.sdesc = g.sdesc;
    a.cell_start = g.cell;
    return a;
}

// The caller's models, 9 floats a pair, through the stage's pinned staging buffer, once the previous call's copy out of it is done
int stage_host_models(OrbProgram* p, int which, const GridSearchState& g, const float* models_host, uint32_t pairs, hipStream_t s) {
    if (p->stage[which].stream) HIP_TRY(p, hipEventSynchronize(p->stage[which].done));
    memcpy(g.h_model, models_host, (size_t)pairs * 9u * sizeof(float));
    HIP_TRY(p, hipMemcpyAsync(g.d_model, g.h_model, (size_t)pairs * 9u * sizeof(float), hipMemcpyHostToDevice, s));
    return ORB_OK;
}

// LocArgs on a set of buffers, from the fields OrbLocalizeParams and OrbBridgeParams share (defaults applied)
template <class Params>
LocArgs loc_args(const OrbProgram* p, const PnpState& l, const Params& g, uint32_t seed_salt) {
    LocArgs a{};
    a.counts = p->d_counts;
    a.corners = p->d_corners;
    a.matches = p->d_matches;
    a.cap = p->cfg.max_features;
    a.poses = p->d_pose;
    a.points = p->d_ppoints;
    a.hyps = g.hypotheses;
    a.max_distance = g.max_distance;
    a.ratio = g.ratio;
    a.fx = g.fx;
    a.fy = g.fy;
    a.cx = g.cx;
    a.cy = g.cy;
    a.r2 = g.max_reproj_px * g.max_reproj_px;
    a.seed_mix = lowbias32(g.seed ^ seed_salt);
    a.reca = l.reca;
    a.recb = l.recb;
    a.cand_of = l.cand;  // bridge: NULL, k_loc_score reads none
    a.n_cand = l.n;
    a.keys = l.keys;
    a.fix = l.fix;
    a.mask = l.mask;
    return a;
}

// The grid of the guided and the band search, fixed by the program's first such call: the smallest cell (8, or TINYORB_GUIDE_CELL: a
// power of two 1..256) that keeps the frame within kGuideMaxCells
void guide_grid(OrbProgram* p) {
    if (p->guide_cell >= 0) return;
    const uint32_t W = p->plan.pyr.w[0], H = p->plan.pyr.h[0];
    int sh = 3;
    if (const char* e = getenv("TINYORB_GUIDE_CELL")) {
        const int c = atoi(e);
        if (c >= 1 && c <= 256 && (c & (c - 1)) == 0) sh = __builtin_ctz((unsigned)c);
    }
    while ((size_t)((W + (1u << sh) - 1u) >> sh) * ((H + (1u << sh) - 1u) >> sh) > kGuideMaxCells) sh++;
    p->guide_cell = sh;
}

}  // namespace

extern "C" {

int orb_verify_consecutive(OrbProgram* p, uint32_t n_frames, const OrbVerifyParams* params, void* stream) {
    return p ? run_verifier(p, kHomography, p->verify, n_frames, params, stream) : ORB_EINVAL;
}

int orb_verify_read(OrbProgram* p, uint32_t pair, OrbPairModel* model, uint8_t* inlier, size_t n) {
    return p ? read_stage(p, ST_VERIFY, pair, model, p->verify.model, sizeof(OrbPairModel), inlier, p->verify.mask, 1, n) : ORB_EINVAL;
}

int orb_verify_epipolar(OrbProgram* p, uint32_t n_frames, const OrbVerifyParams* params, void* stream) {
    return p ? run_verifier(p, kEpipolar, p->epi, n_frames, params, stream) : ORB_EINVAL;
}

int orb_verify_epipolar_read(OrbProgram* p, uint32_t pair, OrbPairModel* model, uint8_t* inlier, size_t n) {
    return p ? read_stage(p, ST_EPI, pair, model, p->epi.model, sizeof(OrbPairModel), inlier, p->epi.mask, 1, n) : ORB_EINVAL;
}

int orb_match_pairs(OrbProgram* p, const OrbFramePair* pairs_host, uint32_t n_pairs, void* stream) {
    if (!p) return ORB_EINVAL;
    if (!p->last_batch) return fail(p, ORB_ESTATE, "match_pairs before a batch");
    const size_t cap = p->cfg.max_features, P = (size_t)ORB_PAIRS_PER_FRAME * p->plan.max_batch;
    if (!pairs_host || n_pairs < 1u || n_pairs > P) return fail(p, ORB_EINVAL, "match_pairs: need a list of 1..%zu pairs", P);
    if (cap > (1u << 23)) return fail(p, ORB_EINVAL, "match_pairs: max_features must be <= 2^23");
    uint32_t last = 0;  // MP-1: the largest listed frame
    for (uint32_t i = 0; i < n_pairs; i++) {
        const OrbFramePair e = pairs_host[i];
        if (e.query >= p->last_batch || e.target >= p->last_batch || e.query == e.target)
            return fail(p, ORB_EINVAL, "match_pairs: entry %u is (%u, %u): two different frames below %u are needed", i, e.query, e.target, p->last_batch);
        last = std::max(last, std::max(e.query, e.target));
    }
    hipStream_t s;
    if (int rc = stage_open(p, ST_PAIRS, stream, 0u, &s)) return rc;  // reads no other stage's results
    // The matrix-core matcher needs the descriptors as fp4, 128 bytes per record of the batch, in a buffer of the stage's own.  A
    // capacity beyond its key's index range, TINYORB_MATCH_VALU=1 or no memory for the bytes leaves the vector-unit kernel.
    bool mfma = match_form(p) != 1 && cap <= (size_t)kMatch4MaxCap;
    if (mfma && !p->d_pdesc4 && hipMalloc(&p->d_pdesc4, (size_t)p->plan.max_batch * cap * 128u) != hipSuccess) {
        (void)hipGetLastError();
        p->d_pdesc4 = nullptr;
        mfma = false;
    }
    // MP-5: the list through the stage's pinned buffer, once the previous call's copy out of it is done
    if (p->stage[ST_PAIRS].stream) HIP_TRY(p, hipEventSynchronize(p->stage[ST_PAIRS].done));
    memcpy(p->h_plist, pairs_host, (size_t)n_pairs * sizeof(OrbFramePair));
    HIP_TRY(p, hipMemcpyAsync(p->d_plist, p->h_plist, (size_t)n_pairs * sizeof(OrbFramePair), hipMemcpyHostToDevice, s));
    if (mfma) {
        hipLaunchKernelGGL(k_desc_expand4, dim3((unsigned)((cap + 31u) / 32u), last + 1u), dim3(256), 0, s, p->d_counts, p->d_desc, (uint32_t)cap, p->d_pdesc4);
        hipLaunchKernelGGL(k_match_pairs_fp4, dim3(n_pairs, (unsigned)((cap + kMatchQueriesPerWg - 1u) / kMatchQueriesPerWg)), dim3(64 * kMatchWaves), 0, s,
                           (const OrbFramePair*)p->d_plist, p->d_counts, p->d_pdesc4, (uint32_t)cap, p->d_prows);
    } else {
        hipLaunchKernelGGL(k_match_pairs, dim3(n_pairs, (unsigned)((cap + 64u * kMatchQ - 1u) / (64u * kMatchQ))), dim3(64), 0, s,
                           (const OrbFramePair*)p->d_plist, p->d_counts, p->d_desc, (uint32_t)cap, p->d_prows);
    }
    return stage_end(p, ST_PAIRS, s, n_pairs);  // p->last_stream stays, as after a guided call
}

int orb_match_pairs_read(OrbProgram* p, uint32_t pair, OrbMatch* dst, size_t n) {
    return p ? read_stage(p, ST_PAIRS, pair, nullptr, nullptr, 0, dst, p->d_prows, sizeof(OrbMatch), n) : ORB_EINVAL;
}

int orb_verify_pairs(OrbProgram* p, uint32_t n_pairs, uint32_t model, const OrbVerifyParams* params, void* stream) {
    if (!p) return ORB_EINVAL;
    if (model > ORB_PAIRS_EPIPOLAR) return fail(p, ORB_EINVAL, "verify_pairs: unknown model %u", model);
    return run_pairs_verifier(p, model == ORB_PAIRS_EPIPOLAR ? kEpipolar : kHomography, n_pairs, params, stream);
}

int orb_verify_pairs_read(OrbProgram* p, uint32_t pair, OrbPairModel* model, uint8_t* inlier, size_t n) {
    return p ? read_stage(p, ST_PAIRS_VERIFY, pair, model, p->pverify.model, sizeof(OrbPairModel), inlier, p->pverify.mask, 1, n) : ORB_EINVAL;
}

int orb_loop_pairs(OrbProgram* p, uint32_t n_pairs, const OrbLoopParams* params, void* stream) {
    if (!p || !params) return p ? fail(p, ORB_EINVAL, "loop_pairs: params is NULL") : ORB_EINVAL;
    OrbLoopParams g = *params;
    for (uint32_t w : g.reserved)
        if (w) return fail(p, ORB_EINVAL, "loop_pairs: reserved words must be 0");
    if (int rc = check_intrinsics(p, ST_LOOP, g.fx, g.fy, g.cx, g.cy)) return rc;
    if (!(std::isfinite(g.max_reproj_px) && g.max_reproj_px >= 0.0f)) return fail(p, ORB_EINVAL, "loop_pairs: max_reproj_px must be finite and >= 0");
    if (int rc = ransac_params(p, ST_LOOP, &g.hypotheses, &g.max_distance, &g.ratio)) return rc;
    if (int rc = stages_fresh(p, ST_LOOP, kStages[ST_LOOP].reads)) return rc;
    const Stage* const st = p->stage;
    if (n_pairs < 1u || n_pairs > st[ST_PAIRS].extent) return fail(p, ORB_EINVAL, "loop_pairs: need 1..%u pairs (the matched ones)", st[ST_PAIRS].extent);
    // LC-1: L, the frames of the last landmarks call (a later matcher or trajectory call of fewer frames lowers it)
    const uint32_t n_frames = std::min(st[ST_LANDMARK].extent + 1u, std::min(st[ST_MATCH].extent, st[ST_TRAJ].extent));
    const size_t cap = p->cfg.max_features;
    if ((unsigned long long)n_frames * cap >= 0xffffffffull)  // LC-2: a key p * cap + i below the "no owner" word
        return fail(p, ORB_EINVAL, "loop_pairs: the landmarks call's frames * max_features must be below 2^32 - 1");
    if (g.max_reproj_px == 0.0f) g.max_reproj_px = 2.0f;
    hipStream_t s;
    if (int rc = stage_open(p, ST_LOOP, stream, kStages[ST_LOOP].reads, &s)) return rc;
    LcArgs a{};
    a.loc = loc_args(p, p->loop, g, kLcSeedSalt);
    a.list = (const uint2*)p->d_plist;
    a.rows = p->d_prows;
    a.frames = p->d_jframe;
    a.lms = p->d_mland;
    a.n_frames = n_frames;
    a.traj_frames = st[ST_TRAJ].extent;
    a.owner = p->d_lowner;
    HIP_TRY(p, hipMemsetAsync(p->d_lowner, 0xff, (size_t)n_frames * cap * sizeof(uint32_t), s));
    if (n_frames > 1u)
        hipLaunchKernelGGL(k_lc_index, dim3(n_frames - 1u, (unsigned)((cap + kLcThreads - 1u) / kLcThreads)), dim3(kLcThreads), 0, s, a);
    hipLaunchKernelGGL(k_lc_gather, dim3(n_pairs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_loc_score, dim3(n_pairs, (g.hypotheses + kVerifyHypPerWg - 1u) / kVerifyHypPerWg), dim3(256), 0, s, a.loc);
    hipLaunchKernelGGL(k_lc_refine, dim3(n_pairs), dim3(256), 0, s, a);
    return stage_end(p, ST_LOOP, s, n_pairs);  // p->last_stream stays, as after a guided call
}

int orb_loop_pairs_read(OrbProgram* p, uint32_t pair, OrbLoopFix* fix, uint8_t* inliers, size_t n) {
    return p ? read_stage(p, ST_LOOP, pair, fix, p->loop.fix, sizeof(OrbLoopFix), inliers, p->loop.mask, 1, n) : ORB_EINVAL;
}

// ---- the keyframe store ----

// A host-side access to the store (read, load, remove): the device, the store itself, the slot, and every keyframe call in flight done
static int keyframes_host_access(OrbProgram* p, const char* who, uint32_t slot) {
    if (!p->kf_slots) return fail(p, ORB_ESTATE, "%s before orb_keyframes_reserve", who);
    if (slot >= p->kf_slots) return fail(p, ORB_EINVAL, "%s: slot %u of %u", who, slot, p->kf_slots);
    HIP_TRY(p, hipSetDevice(p->device));
    for (int st : {ST_KEYFRAMES, ST_KF_MATCH, ST_KF_LOC, ST_ANCHOR})
        if (p->stage[st].stream) HIP_TRY(p, hipEventSynchronize(p->stage[st].done));
    return ORB_OK;
}

// Every byte of `slot` to 0 on the program's stream (the caller synchronises it)
static int keyframes_clear_slot(OrbProgram* p, uint32_t slot) {
    const size_t cap = p->cfg.max_features, B = p->plan.max_batch;
    HIP_TRY(p, hipMemsetAsync(p->d_khead + (size_t)slot * kKfHeadWords, 0, sizeof(OrbKeyframe), p->stream));
    HIP_TRY(p, hipMemsetAsync(p->d_kcorners + (size_t)slot * cap, 0, cap * sizeof(CornerData), p->stream));
    HIP_TRY(p, hipMemsetAsync(p->d_kdesc + (B + slot) * cap, 0, cap * sizeof(CornerDescriptor), p->stream));
    HIP_TRY(p, hipMemsetAsync(p->d_kpoints + (size_t)slot * cap, 0, cap * sizeof(OrbMapPoint), p->stream));
    HIP_TRY(p, hipMemsetAsync(p->d_kcounts + B + slot, 0, sizeof(uint32_t), p->stream));
    return ORB_OK;
}

int orb_keyframes_reserve(OrbProgram* p, uint32_t slots) {
    if (!p) return ORB_EINVAL;
    if (slots < 1u || slots > ORB_KEYFRAME_SLOTS_MAX) return fail(p, ORB_EINVAL, "keyframes_reserve: need 1..%u slots", ORB_KEYFRAME_SLOTS_MAX);
    if (p->kf_slots) return p->kf_slots == slots ? ORB_OK : fail(p, ORB_ESTATE, "keyframes_reserve: the store has %u slots", p->kf_slots);
    HIP_TRY(p, hipSetDevice(p->device));
    p->kf_slots = slots;
    if (int rc = alloc_all_or_none(p, ST_KEYFRAMES, "keyframes_reserve")) {
        p->kf_slots = 0;
        return rc;
    }
    // Every slot EMPTY.  A failure here leaves no store behind: the buffers are freed and the next call reserves again.
    const StageBufs l = stage_buffers(p, ST_KEYFRAMES);
    hipError_t e = hipSuccess;
    for (int i = 0; i < l.n && e == hipSuccess; i++)
        if (!l.b[i].pinned && !l.b[i].soft) e = hipMemsetAsync(*l.b[i].slot, 0, l.b[i].bytes, p->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess) {
        free_stage_buffers(p, ST_KEYFRAMES);
        p->kf_slots = 0;
        return fail(p, ORB_EHIP, "keyframes_reserve: clearing the store failed: %s", hipGetErrorString(e));
    }
    p->kf_filled.assign(slots, 0);
    p->kf_gen++;
    return ORB_OK;
}

int orb_keyframes_insert(OrbProgram* p, const OrbKeyframeEntry* list, uint32_t n, void* stream) {
    if (!p) return ORB_EINVAL;
    if (!p->kf_slots) return fail(p, ORB_ESTATE, "keyframes_insert before orb_keyframes_reserve");
    if (!p->last_batch) return fail(p, ORB_ESTATE, "keyframes_insert before a batch");
    if (!list || n < 1u || n > p->plan.max_batch) return fail(p, ORB_EINVAL, "keyframes_insert: need a list of 1..%u entries", p->plan.max_batch);
    std::vector<uint8_t> named(p->kf_slots, 0);
    for (uint32_t i = 0; i < n; i++) {
        const OrbKeyframeEntry e = list[i];
        if (e.frame >= p->last_batch || e.slot >= p->kf_slots || named[e.slot])
            return fail(p, ORB_EINVAL, "keyframes_insert: entry %u is (frame %u, slot %u): a frame below %u and a slot below %u that no earlier entry names are needed", i,
                        e.frame, e.slot, p->last_batch, p->kf_slots);
        named[e.slot] = 1;
    }
    if (int rc = stages_fresh(p, ST_KEYFRAMES, kStages[ST_KEYFRAMES].reads)) return rc;
    const Stage* const st = p->stage;
    // LC-1: L, the frames of the last landmarks call (a later matcher or trajectory call of fewer frames lowers it)
    const uint32_t n_frames = std::min(st[ST_LANDMARK].extent + 1u, std::min(st[ST_MATCH].extent, st[ST_TRAJ].extent));
    const size_t cap = p->cfg.max_features, B = p->plan.max_batch;
    if ((unsigned long long)n_frames * cap >= 0xffffffffull)  // LC-2: a key p * cap + i below the "no owner" word
        return fail(p, ORB_EINVAL, "keyframes_insert: the landmarks call's frames * max_features must be below 2^32 - 1");
    hipStream_t s;
    if (int rc = stage_open(p, ST_KEYFRAMES, stream, kStages[ST_KEYFRAMES].reads, &s)) return rc;
    // the list through the stage's pinned buffer, once the previous call's copy out of it is done
    if (p->stage[ST_KEYFRAMES].stream) HIP_TRY(p, hipEventSynchronize(p->stage[ST_KEYFRAMES].done));
    memcpy(p->h_klist, list, (size_t)n * sizeof(OrbKeyframeEntry));
    HIP_TRY(p, hipMemcpyAsync(p->d_klist, p->h_klist, (size_t)n * sizeof(OrbKeyframeEntry), hipMemcpyHostToDevice, s));
    KfInsertArgs a{};
    a.lc.loc.counts = p->d_counts;
    a.lc.loc.matches = p->d_matches;
    a.lc.loc.cap = (uint32_t)cap;
    a.lc.frames = p->d_jframe;
    a.lc.lms = p->d_mland;
    a.lc.n_frames = n_frames;
    a.lc.traj_frames = st[ST_TRAJ].extent;
    a.lc.owner = p->d_kowner;
    a.list = (const uint4*)p->d_klist;
    a.corners = (const uint4*)p->d_corners;
    a.desc = (const uint4*)p->d_desc;
    a.n_entries = n;
    a.heads = p->d_khead;
    a.slot_counts = p->d_kcounts + B;
    a.kcorners = (uint4*)p->d_kcorners;
    a.kdesc = (uint4*)(p->d_kdesc + B * cap);
    a.kpoints = p->d_kpoints;
    HIP_TRY(p, hipMemsetAsync(p->d_kowner, 0xff, (size_t)n_frames * cap * sizeof(uint32_t), s));
    if (n_frames > 1u)
        hipLaunchKernelGGL(k_lc_index, dim3(n_frames - 1u, (unsigned)((cap + kLcThreads - 1u) / kLcThreads)), dim3(kLcThreads), 0, s, a.lc);
    hipLaunchKernelGGL(k_kf_head, dim3((n + kKfThreads - 1u) / kKfThreads), dim3(kKfThreads), 0, s, a);
    hipLaunchKernelGGL(k_kf_insert, dim3((unsigned)((cap + kKfThreads - 1u) / kKfThreads), n), dim3(kKfThreads), 0, s, a);
    for (uint32_t i = 0; i < n; i++) p->kf_filled[list[i].slot] = 1;
    p->kf_gen++;
    return stage_end(p, ST_KEYFRAMES, s, n);  // p->last_stream stays, as after a guided call
}

int orb_keyframes_read(OrbProgram* p, uint32_t slot, OrbKeyframe* header, CornerData* corners, CornerDescriptor* descriptors, OrbMapPoint* points,
                       size_t n) {
    if (!p) return ORB_EINVAL;
    if (int rc = keyframes_host_access(p, "keyframes_read", slot)) return rc;
    const size_t cap = p->cfg.max_features, B = p->plan.max_batch;
    if (n > cap) n = cap;
    if (header) HIP_TRY(p, hipMemcpy(header, p->d_khead + (size_t)slot * kKfHeadWords, sizeof(OrbKeyframe), hipMemcpyDeviceToHost));
    if (corners && n) HIP_TRY(p, hipMemcpy(corners, p->d_kcorners + (size_t)slot * cap, n * sizeof(CornerData), hipMemcpyDeviceToHost));
    if (descriptors && n) HIP_TRY(p, hipMemcpy(descriptors, p->d_kdesc + (B + slot) * cap, n * sizeof(CornerDescriptor), hipMemcpyDeviceToHost));
    if (points && n) HIP_TRY(p, hipMemcpy(points, p->d_kpoints + (size_t)slot * cap, n * sizeof(OrbMapPoint), hipMemcpyDeviceToHost));
    return ORB_OK;
}

int orb_keyframes_load(OrbProgram* p, uint32_t slot, const OrbKeyframe* header, const CornerData* corners, const CornerDescriptor* descriptors,
                       const OrbMapPoint* points, size_t n) {
    if (!p) return ORB_EINVAL;
    if (int rc = keyframes_host_access(p, "keyframes_load", slot)) return rc;
    const size_t cap = p->cfg.max_features, B = p->plan.max_batch;
    if (!header || n != header->keypoints || n > cap || (n && (!corners || !descriptors || !points)))
        return fail(p, ORB_EINVAL, "keyframes_load: need a header, n == header->keypoints <= %zu and the three arrays", cap);
    if (header->status != ORB_KEYFRAME_STORED && header->status != ORB_KEYFRAME_NOMAP)
        return fail(p, ORB_EINVAL, "keyframes_load: status %u is neither STORED nor NOMAP", header->status);
    for (uint32_t w : header->reserved)
        if (w) return fail(p, ORB_EINVAL, "keyframes_load: reserved words must be 0");
    uint32_t keys = 0;
    for (size_t i = 0; i < n; i++) keys += points[i].key != ORB_KEYFRAME_NONE;
    if (keys != header->points) return fail(p, ORB_EINVAL, "keyframes_load: header->points is %u, %u of the points have a key", header->points, keys);
    if (int rc = keyframes_clear_slot(p, slot)) return rc;
    const uint32_t count = (uint32_t)n;
    HIP_TRY(p, hipMemcpyAsync(p->d_khead + (size_t)slot * kKfHeadWords, header, sizeof(OrbKeyframe), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(p, hipMemcpyAsync(p->d_kcounts + B + slot, &count, sizeof(uint32_t), hipMemcpyHostToDevice, p->stream));
    if (n) {
        HIP_TRY(p, hipMemcpyAsync(p->d_kcorners + (size_t)slot * cap, corners, n * sizeof(CornerData), hipMemcpyHostToDevice, p->stream));
        HIP_TRY(p, hipMemcpyAsync(p->d_kdesc + (B + slot) * cap, descriptors, n * sizeof(CornerDescriptor), hipMemcpyHostToDevice, p->stream));
        HIP_TRY(p, hipMemcpyAsync(p->d_kpoints + (size_t)slot * cap, points, n * sizeof(OrbMapPoint), hipMemcpyHostToDevice, p->stream));
    }
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    p->kf_filled[slot] = 1;
    p->kf_gen++;
    return ORB_OK;
}

int orb_keyframes_remove(OrbProgram* p, uint32_t slot) {
    if (!p) return ORB_EINVAL;
    if (int rc = keyframes_host_access(p, "keyframes_remove", slot)) return rc;
    if (int rc = keyframes_clear_slot(p, slot)) return rc;
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    p->kf_filled[slot] = 0;
    p->kf_gen++;
    return ORB_OK;
}

int orb_match_keyframes(OrbProgram* p, const OrbKeyframePair* list, uint32_t n, void* stream) {
    if (!p) return ORB_EINVAL;
    if (!p->kf_slots) return fail(p, ORB_ESTATE, "match_keyframes before orb_keyframes_reserve");
    if (!p->last_batch) return fail(p, ORB_ESTATE, "match_keyframes before a batch");
    const size_t cap = p->cfg.max_features, B = p->plan.max_batch, P = (size_t)ORB_PAIRS_PER_FRAME * B;
    if (!list || n < 1u || n > P) return fail(p, ORB_EINVAL, "match_keyframes: need a list of 1..%zu entries", P);
    if (cap > (1u << 23)) return fail(p, ORB_EINVAL, "match_keyframes: max_features must be <= 2^23");
    uint32_t last = 0;  // the largest listed query
    for (uint32_t i = 0; i < n; i++) {
        const OrbKeyframePair e = list[i];
        if (e.query >= p->last_batch || e.slot >= p->kf_slots)
            return fail(p, ORB_EINVAL, "match_keyframes: entry %u is (%u, %u): a frame below %u and a slot below %u are needed", i, e.query, e.slot, p->last_batch,
                        p->kf_slots);
        if (!p->kf_filled[e.slot]) return fail(p, ORB_EINVAL, "match_keyframes: entry %u names slot %u, which is empty", i, e.slot);
        last = std::max(last, e.query);
    }
    hipStream_t s;
    if (int rc = stage_open(p, ST_KF_MATCH, stream, kStages[ST_KF_MATCH].reads, &s)) return rc;
    // The matrix-core matcher as orb_match_pairs chooses it: the rows as fp4, 128 bytes per record, in a buffer of the store's
    bool mfma = match_form(p) != 1 && cap <= (size_t)kMatch4MaxCap;
    if (mfma && !p->d_kdesc4 && hipMalloc(&p->d_kdesc4, (B + p->kf_slots) * cap * 128u) != hipSuccess) {
        (void)hipGetLastError();
        p->d_kdesc4 = nullptr;
        mfma = false;
    }
    if (p->stage[ST_KF_MATCH].stream) HIP_TRY(p, hipEventSynchronize(p->stage[ST_KF_MATCH].done));
    memcpy(p->h_kmlist, list, (size_t)n * sizeof(OrbKeyframePair));
    HIP_TRY(p, hipMemcpyAsync(p->d_kmlist, p->h_kmlist, (size_t)n * sizeof(OrbKeyframePair), hipMemcpyHostToDevice, s));
    // KF-3: the batch's rows in front of the slots'
    HIP_TRY(p, hipMemcpyAsync(p->d_kcounts, p->d_counts, (size_t)(last + 1u) * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    const unsigned gx = (unsigned)((cap + 31u) / 32u);
    if (mfma) {
        hipLaunchKernelGGL(k_desc_expand4, dim3(gx, last + 1u), dim3(256), 0, s, p->d_counts, p->d_desc, (uint32_t)cap, p->d_kdesc4);
        if (p->kf_desc4_gen != p->kf_gen) {  // the slots' rows, once per state of the store
            hipLaunchKernelGGL(k_desc_expand4, dim3(gx, p->kf_slots), dim3(256), 0, s, p->d_kcounts + B, p->d_kdesc + B * cap, (uint32_t)cap,
                               p->d_kdesc4 + B * cap * 128u);
            p->kf_desc4_gen = p->kf_gen;
        }
        hipLaunchKernelGGL(k_match_kf_fp4, dim3(n, (unsigned)((cap + kMatchQueriesPerWg - 1u) / kMatchQueriesPerWg)), dim3(64 * kMatchWaves), 0, s,
                           (const uint2*)p->d_kmlist, (uint32_t)B, p->d_kcounts, p->d_kdesc4, (uint32_t)cap, p->d_kmrows);
    } else {
        HIP_TRY(p, hipMemcpyAsync(p->d_kdesc, p->d_desc, (size_t)(last + 1u) * cap * sizeof(CornerDescriptor), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_match_kf, dim3(n, (unsigned)((cap + 64u * kMatchQ - 1u) / (64u * kMatchQ))), dim3(64), 0, s, (const uint2*)p->d_kmlist,
                           (uint32_t)B, p->d_kcounts, p->d_kdesc, (uint32_t)cap, p->d_kmrows);
    }
    p->kf_match_gen = p->kf_gen;
    p->kf_match_call++;
    return stage_end(p, ST_KF_MATCH, s, n);  // p->last_stream stays, as after a guided call
}

int orb_match_keyframes_read(OrbProgram* p, uint32_t entry, OrbMatch* dst, size_t n) {
    return p ? read_stage(p, ST_KF_MATCH, entry, nullptr, nullptr, 0, dst, p->d_kmrows, sizeof(OrbMatch), n) : ORB_EINVAL;
}

int orb_localize_keyframes(OrbProgram* p, uint32_t n, const OrbLoopParams* params, void* stream) {
    if (!p || !params) return p ? fail(p, ORB_EINVAL, "localize_keyframes: params is NULL") : ORB_EINVAL;
    OrbLoopParams g = *params;
    for (uint32_t w : g.reserved)  // orb_loop_pairs' checks, through the same two checkers
        if (w) return fail(p, ORB_EINVAL, "localize_keyframes: reserved words must be 0");
    if (int rc = check_intrinsics(p, ST_KF_LOC, g.fx, g.fy, g.cx, g.cy)) return rc;
    if (!(std::isfinite(g.max_reproj_px) && g.max_reproj_px >= 0.0f)) return fail(p, ORB_EINVAL, "localize_keyframes: max_reproj_px must be finite and >= 0");
    if (int rc = ransac_params(p, ST_KF_LOC, &g.hypotheses, &g.max_distance, &g.ratio)) return rc;
    if (int rc = stages_fresh(p, ST_KF_LOC, kStages[ST_KF_LOC].reads)) return rc;
    if (p->kf_match_gen != p->kf_gen) return fail(p, ORB_ESTATE, "localize_keyframes: the store has changed since the last orb_match_keyframes");
    const Stage* const st = p->stage;
    if (n < 1u || n > st[ST_KF_MATCH].extent) return fail(p, ORB_EINVAL, "localize_keyframes: need 1..%u entries (the matched ones)", st[ST_KF_MATCH].extent);
    if (g.max_reproj_px == 0.0f) g.max_reproj_px = 2.0f;
    hipStream_t s;
    if (int rc = stage_open(p, ST_KF_LOC, stream, kStages[ST_KF_LOC].reads, &s)) return rc;
    KfArgs a{};
    a.loc = loc_args(p, p->kfloc, g, kLcSeedSalt);
    a.list = (const uint2*)p->d_kmlist;
    a.rows = p->d_kmrows;
    a.heads = p->d_khead;
    a.kpoints = p->d_kpoints;
    hipLaunchKernelGGL(k_kf_gather, dim3(n), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_loc_score, dim3(n, (g.hypotheses + kVerifyHypPerWg - 1u) / kVerifyHypPerWg), dim3(256), 0, s, a.loc);
    hipLaunchKernelGGL(k_kf_refine, dim3(n), dim3(256), 0, s, a);
    p->kf_loc_call = p->kf_match_call;
    return stage_end(p, ST_KF_LOC, s, n);  // p->last_stream stays, as after a guided call
}

int orb_localize_keyframes_read(OrbProgram* p, uint32_t entry, OrbKeyframeFix* fix, uint8_t* inliers, size_t n) {
    return p ? read_stage(p, ST_KF_LOC, entry, fix, p->kfloc.fix, sizeof(OrbKeyframeFix), inliers, p->kfloc.mask, 1, n) : ORB_EINVAL;
}

int orb_debug_loop_buffer(OrbProgram* p, void** fixes) {
    if (!p) return ORB_EINVAL;
    if (!p->stage[ST_LOOP].extent) return fail(p, ORB_ESTATE, "debug_loop_buffer before orb_loop_pairs");
    if (fixes) *fixes = p->loop.fix;
    return ORB_OK;
}

int orb_graph_pairs(OrbProgram* p, uint32_t n_pairs, const OrbGraphParams* params, void* stream) {
    if (!p) return ORB_EINVAL;
    OrbGraphParams g{};
    if (params) g = *params;
    if (g.reserved[0] | g.reserved[1]) return fail(p, ORB_EINVAL, "graph_pairs: reserved words must be 0");
    if (g.rounds > 16u || g.cg_iterations > kPgMaxCg || (g.flags & ~ORB_GRAPH_USE_MINIMAL))
        return fail(p, ORB_EINVAL, "graph_pairs: rounds 0..16, cg_iterations 0..%u, flags ORB_GRAPH_USE_MINIMAL or 0", kPgMaxCg);
    if (!(std::isfinite(g.loop_weight) && g.loop_weight >= 0.0f) || !(std::isfinite(g.rotation_weight) && g.rotation_weight >= 0.0f))
        return fail(p, ORB_EINVAL, "graph_pairs: loop_weight and rotation_weight must be finite and >= 0");
    if (int rc = stages_fresh(p, ST_GRAPH, kStages[ST_GRAPH].reads)) return rc;
    const Stage* const st = p->stage;
    if (n_pairs < 1u || n_pairs > st[ST_LOOP].extent) return fail(p, ORB_EINVAL, "graph_pairs: need 1..%u pairs (the last orb_loop_pairs' entries)", st[ST_LOOP].extent);
    const bool first = !p->d_gpose;
    hipStream_t s;
    if (int rc = stage_open(p, ST_GRAPH, stream, kStages[ST_GRAPH].reads, &s)) return rc;
    if (first)  // k_pg_solve keeps a segment in all of a CU's LDS but the reductions' partials
        HIP_TRY(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_pg_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPgLdsBytes));
    PgArgs a{};
    a.frames = p->d_jframe;
    a.list = (const uint2*)p->d_plist;
    a.fixes = p->loop.fix;
    a.n_frames = st[ST_TRAJ].extent;  // PG-1: F
    a.n_pairs = n_pairs;
    a.min_inliers = g.min_inliers ? g.min_inliers : 12u;
    a.use_minimal = g.flags & ORB_GRAPH_USE_MINIMAL;
    a.rounds = g.rounds ? g.rounds : 4u;
    a.cg_iterations = g.cg_iterations;
    a.loop_weight = g.loop_weight == 0.0f ? 1.0f : g.loop_weight;
    a.rotation_weight = g.rotation_weight == 0.0f ? 1.0f : g.rotation_weight;
    a.edges = p->d_gedge;
    a.row = p->d_grow;
    a.col = p->d_gcol;
    a.out = p->d_gpose;
    a.work = p->d_gwork;
    const uint32_t F = a.n_frames;
    hipLaunchKernelGGL(k_pg_edges, dim3((n_pairs + kPgThreads - 1u) / kPgThreads), dim3(kPgThreads), 0, s, a);
    hipLaunchKernelGGL(k_pg_index, dim3(1), dim3(kPgThreads), 0, s, a);
    hipLaunchKernelGGL(k_pg_write, dim3((F + kPgThreads - 1u) / kPgThreads), dim3(kPgThreads), 0, s, a);
    hipLaunchKernelGGL(k_pg_solve, dim3(F), dim3(kPgThreads), kPgLdsBytes, s, a);
    if (int rc = stage_end(p, ST_GRAPH, s, F)) return rc;  // p->last_stream stays, as after a guided call
    p->graph_pairs = n_pairs;
    return ORB_OK;
}

int orb_graph_read(OrbProgram* p, uint32_t frame, OrbGraphPose* pose) {
    if (!p) return ORB_EINVAL;
    if (p->stage[ST_GRAPH].extent && !pose) return fail(p, ORB_EINVAL, "graph_read: pose is NULL");
    return read_stage(p, ST_GRAPH, frame, pose, p->d_gpose, sizeof(OrbGraphPose), nullptr, nullptr, 0, 0);
}

int orb_graph_edges(OrbProgram* p, OrbGraphEdge* dst, size_t n) {
    if (!p) return ORB_EINVAL;
    const Stage& last = p->stage[ST_GRAPH];
    if (!last.extent) return fail(p, ORB_ESTATE, "graph_edges before graph_pairs");
    if (n > p->graph_pairs || (!dst && n)) return fail(p, ORB_EINVAL, "graph_edges: %zu entries of %u, or the destination is NULL", n, p->graph_pairs);
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipEventSynchronize(last.done));
    if (n) HIP_TRY(p, hipMemcpy(dst, p->d_gedge, n * sizeof(OrbGraphEdge), hipMemcpyDeviceToHost));
    return ORB_OK;
}

int orb_debug_loop_mask_buffer(OrbProgram* p, void** mask) {
    if (!p) return ORB_EINVAL;
    if (!p->stage[ST_LOOP].extent) return fail(p, ORB_ESTATE, "debug_loop_mask_buffer before orb_loop_pairs");
    if (mask) *mask = p->loop.mask;
    return ORB_OK;
}

int orb_join_pairs(OrbProgram* p, uint32_t n_pairs, const OrbJoinParams* params, void* stream) {
    if (!p) return ORB_EINVAL;
    OrbJoinParams g{};
    if (params) g = *params;
    if (g.reserved[0] | g.reserved[1] | g.reserved[2]) return fail(p, ORB_EINVAL, "join_pairs: reserved words must be 0");
    if (g.consistent_permille > 1000u || (g.flags & ~ORB_JOIN_USE_MINIMAL))
        return fail(p, ORB_EINVAL, "join_pairs: consistent_permille 0..1000, flags ORB_JOIN_USE_MINIMAL or 0");
    if (!(std::isfinite(g.scale_tolerance) && g.scale_tolerance >= 0.0f)) return fail(p, ORB_EINVAL, "join_pairs: scale_tolerance must be finite and >= 0");
    if (int rc = stages_fresh(p, ST_JOIN, kStages[ST_JOIN].reads)) return rc;
    const Stage* const st = p->stage;
    if (n_pairs < 1u || n_pairs > st[ST_LOOP].extent) return fail(p, ORB_EINVAL, "join_pairs: need 1..%u pairs (the last orb_loop_pairs' entries)", st[ST_LOOP].extent);
    // SJ-1: L is LC-1's, the frames of the last landmarks call (a later matcher or trajectory call of fewer frames lowers it)
    const uint32_t F = st[ST_TRAJ].extent;
    const uint32_t L = std::min(st[ST_LANDMARK].extent + 1u, std::min(st[ST_MATCH].extent, F));
    const size_t cap = p->cfg.max_features;
    if ((unsigned long long)L * cap >= 0xffffffffull)  // LC-2: a key p * cap + i below the "no owner" word
        return fail(p, ORB_EINVAL, "join_pairs: the landmarks call's frames * max_features must be below 2^32 - 1");
    hipStream_t s;
    if (int rc = stage_open(p, ST_JOIN, stream, kStages[ST_JOIN].reads, &s)) return rc;
    LcArgs o{};  // SJ-2: k_lc_index reads the capacity, the counters, the consecutive records, the frames, the landmarks, L and the owners
    o.loc.cap = (uint32_t)cap;
    o.loc.counts = p->d_counts;
    o.loc.matches = p->d_matches;
    o.frames = p->d_jframe;
    o.lms = p->d_mland;
    o.n_frames = L;
    o.traj_frames = F;
    o.owner = p->d_sowner;
    SjArgs a{};
    a.counts = p->d_counts;
    a.cap = (uint32_t)cap;
    a.list = (const uint2*)p->d_plist;
    a.rows = p->d_prows;
    a.frames = p->d_jframe;
    a.lms = p->d_mland;
    a.fixes = p->loop.fix;
    a.mask = p->loop.mask;
    a.owner = p->d_sowner;
    a.n_frames = F;
    a.map_frames = L;
    a.n_pairs = n_pairs;
    a.min_inliers = g.min_inliers ? g.min_inliers : 12u;
    a.use_minimal = g.flags & ORB_JOIN_USE_MINIMAL;
    a.min_shared = g.min_shared ? g.min_shared : 8u;
    a.tol = g.scale_tolerance == 0.0f ? 0.1f : g.scale_tolerance;
    a.permille = g.consistent_permille ? g.consistent_permille : 500u;
    a.ratios = p->d_sratio;
    a.links = p->d_slink;
    a.keys = p->d_skey;
    a.segs = p->d_sseg;
    a.out = p->d_spose;
    // the owners of all F frames: rows L .. F - 1 have none
    HIP_TRY(p, hipMemsetAsync(p->d_sowner, 0xff, (size_t)F * cap * sizeof(uint32_t), s));
    HIP_TRY(p, hipMemsetAsync(p->d_skey, 0, (size_t)F * sizeof(unsigned long long), s));
    HIP_TRY(p, hipMemsetAsync(p->d_sseg, 0, (size_t)F * sizeof(OrbJoinSegment), s));
    if (L > 1u) hipLaunchKernelGGL(k_lc_index, dim3(L - 1u, (unsigned)((cap + kLcThreads - 1u) / kLcThreads)), dim3(kLcThreads), 0, s, o);
    hipLaunchKernelGGL(k_sj_ratio, dim3(n_pairs), dim3(kSjThreads), 0, s, a);
    hipLaunchKernelGGL(k_sj_chain, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_sj_write, dim3((F + kSjThreads - 1u) / kSjThreads), dim3(kSjThreads), 0, s, a);
    if (int rc = stage_end(p, ST_JOIN, s, F)) return rc;  // p->last_stream stays, as after a guided call
    p->join_pairs = n_pairs;
    return ORB_OK;
}

int orb_join_read(OrbProgram* p, uint32_t frame, OrbJoinPose* pose) {
    if (!p) return ORB_EINVAL;
    if (p->stage[ST_JOIN].extent && !pose) return fail(p, ORB_EINVAL, "join_read: pose is NULL");
    return read_stage(p, ST_JOIN, frame, pose, p->d_spose, sizeof(OrbJoinPose), nullptr, nullptr, 0, 0);
}

// The first n records of one of stage `which`'s tables, behind its last call (the join's and the anchor's segments and links)
static int table_copy(OrbProgram* p, int which, const char* who, void* dst, const void* src, size_t n, size_t have, size_t bytes) {
    if (!p) return ORB_EINVAL;
    const Stage& last = p->stage[which];
    if (!last.extent) return fail(p, ORB_ESTATE, "%s before %s", who, kStages[which].name);
    if (n > have || (!dst && n)) return fail(p, ORB_EINVAL, "%s: %zu records of %zu, or the destination is NULL", who, n, have);
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipEventSynchronize(last.done));
    if (n) HIP_TRY(p, hipMemcpy(dst, src, n * bytes, hipMemcpyDeviceToHost));
    return ORB_OK;
}

int orb_join_segments(OrbProgram* p, OrbJoinSegment* dst, size_t n) {
    return p ? table_copy(p, ST_JOIN, "join_segments", dst, p->d_sseg, n, p->stage[ST_JOIN].extent, sizeof(OrbJoinSegment)) : ORB_EINVAL;
}

int orb_join_links(OrbProgram* p, OrbJoinLink* dst, size_t n) {
    return p ? table_copy(p, ST_JOIN, "join_links", dst, p->d_slink, n, p->join_pairs, sizeof(OrbJoinLink)) : ORB_EINVAL;
}

int orb_remap_frames(OrbProgram* p, const OrbRemapParams* params, void* stream) {
    if (!p) return ORB_EINVAL;
    OrbRemapParams g{};
    if (params) g = *params;
    for (uint32_t w : g.reserved)
        if (w) return fail(p, ORB_EINVAL, "remap_frames: reserved words must be 0");
    if (g.flags & ~(ORB_REMAP_GRAPH | ORB_REMAP_JOIN)) return fail(p, ORB_EINVAL, "remap_frames: flags ORB_REMAP_GRAPH, ORB_REMAP_JOIN or 0");
    const uint32_t sources = g.flags ? g.flags : (ORB_REMAP_GRAPH | ORB_REMAP_JOIN);
    const bool graph = sources & ORB_REMAP_GRAPH, join = sources & ORB_REMAP_JOIN;
    // RM-1: the part of the stage's row that the flags name
    const uint32_t reads = 1u << ST_TRAJ | 1u << ST_LANDMARK | (graph ? 1u << ST_GRAPH : 0u) | (join ? 1u << ST_JOIN : 0u);
    if (int rc = stages_fresh(p, ST_REMAP, reads)) return rc;
    const Stage* const st = p->stage;
    const uint32_t F = st[ST_TRAJ].extent;
    if ((graph && st[ST_GRAPH].extent != F) || (join && st[ST_JOIN].extent != F))
        return fail(p, ORB_ESTATE, "remap_frames: a source covered another number of frames than the last trajectory call's %u", F);
    const uint32_t pairs = std::min(st[ST_LANDMARK].extent, F - 1u);  // P_l
    const size_t cap = p->cfg.max_features;
    hipStream_t s;
    if (int rc = stage_open(p, ST_REMAP, stream, reads, &s)) return rc;
    if (!p->remap_slots) {
        const char* const e = getenv("TINYORB_REMAP_SLOTS");
        p->remap_slots = e && atoi(e) == 1 ? 1 : 2;  // two measured faster
    }
    RmArgs a{};
    a.frames = p->d_jframe;
    a.gposes = graph ? p->d_gpose : nullptr;
    a.segs = join ? p->d_sseg : nullptr;
    a.lms = p->d_mland;
    a.lrows = p->d_mrow;
    a.cap = (uint32_t)cap;
    a.n_frames = F;
    a.n_pairs = pairs;
    a.poses = p->d_rpose;
    a.rows = p->d_rrow;
    a.out = p->d_rland;
    const uint32_t per_wg = kRmThreads * (uint32_t)p->remap_slots;
    const dim3 grid((unsigned)((cap + per_wg - 1u) / per_wg), pairs);
    hipLaunchKernelGGL(k_rm_pose, dim3((F + kRmThreads - 1u) / kRmThreads), dim3(kRmThreads), 0, s, a);
    if (pairs) {
        if (p->remap_slots == 2)
            hipLaunchKernelGGL(k_rm_land<2u>, grid, dim3(kRmThreads), 0, s, a);
        else
            hipLaunchKernelGGL(k_rm_land<1u>, grid, dim3(kRmThreads), 0, s, a);
    }
    if (int rc = stage_end(p, ST_REMAP, s, F)) return rc;  // p->last_stream stays, as after a guided call
    p->remap_pairs = pairs;
    return ORB_OK;
}

int orb_remap_read(OrbProgram* p, uint32_t frame, OrbRemapPose* pose) {
    if (!p) return ORB_EINVAL;
    if (p->stage[ST_REMAP].extent && !pose) return fail(p, ORB_EINVAL, "remap_read: pose is NULL");
    return read_stage(p, ST_REMAP, frame, pose, p->d_rpose, sizeof(OrbRemapPose), nullptr, nullptr, 0, 0);
}

int orb_remap_landmarks(OrbProgram* p, uint32_t pair, OrbRemapRow* row, OrbLandmark* landmarks, size_t n) {
    if (!p) return ORB_EINVAL;
    // the stage's extent is the frames; the pairs it covered are kept beside it
    if (p->stage[ST_REMAP].extent && pair >= p->remap_pairs) return fail(p, ORB_EINVAL, "remap_landmarks: pair %u of %u", pair, p->remap_pairs);
    return read_stage(p, ST_REMAP, pair, row, p->d_rrow, sizeof(OrbRemapRow), landmarks, p->d_rland, sizeof(OrbLandmark), n);
}

// ---- the batch in the stored map ----

int orb_anchor_frames(OrbProgram* p, uint32_t n, const OrbAnchorParams* params, void* stream) {
    if (!p) return ORB_EINVAL;
    OrbAnchorParams g{};
    if (params) g = *params;
    if (g.reserved[0] | g.reserved[1] | g.reserved[2]) return fail(p, ORB_EINVAL, "anchor_frames: reserved words must be 0");
    if (g.consistent_permille > 1000u || (g.flags & ~ORB_ANCHOR_USE_MINIMAL))
        return fail(p, ORB_EINVAL, "anchor_frames: consistent_permille 0..1000, flags ORB_ANCHOR_USE_MINIMAL or 0");
    if (!(std::isfinite(g.scale_tolerance) && g.scale_tolerance >= 0.0f)) return fail(p, ORB_EINVAL, "anchor_frames: scale_tolerance must be finite and >= 0");
    if (int rc = stages_fresh(p, ST_ANCHOR, kStages[ST_ANCHOR].reads)) return rc;
    if (p->kf_match_gen != p->kf_gen) return fail(p, ORB_ESTATE, "anchor_frames: the store has changed since the last orb_match_keyframes");
    if (p->kf_loc_call != p->kf_match_call) return fail(p, ORB_ESTATE, "anchor_frames: the last orb_localize_keyframes read the rows of an earlier orb_match_keyframes");
    const Stage* const st = p->stage;
    if (n < 1u || n > st[ST_KF_LOC].extent) return fail(p, ORB_EINVAL, "anchor_frames: need 1..%u entries (the last orb_localize_keyframes')", st[ST_KF_LOC].extent);
    // AN-1: L is LC-1's, the frames of the last landmarks call (a later matcher or trajectory call of fewer frames lowers it)
    const uint32_t F = st[ST_TRAJ].extent;
    const uint32_t L = std::min(st[ST_LANDMARK].extent + 1u, std::min(st[ST_MATCH].extent, F));
    const size_t cap = p->cfg.max_features;
    if ((unsigned long long)L * cap >= 0xffffffffull)  // LC-2: a key p * cap + i below the "no owner" word
        return fail(p, ORB_EINVAL, "anchor_frames: the landmarks call's frames * max_features must be below 2^32 - 1");
    hipStream_t s;
    if (int rc = stage_open(p, ST_ANCHOR, stream, kStages[ST_ANCHOR].reads, &s)) return rc;
    LcArgs o{};  // AN-2: k_lc_index reads the capacity, the counters, the consecutive records, the frames, the landmarks, L and the owners
    o.loc.cap = (uint32_t)cap;
    o.loc.counts = p->d_counts;
    o.loc.matches = p->d_matches;
    o.frames = p->d_jframe;
    o.lms = p->d_mland;
    o.n_frames = L;
    o.traj_frames = F;
    o.owner = p->d_nowner;
    const uint32_t pairs = L - 1u;  // L >= 1: the stages are fresh
    AnArgs a{};
    a.counts = p->d_counts;
    a.cap = (uint32_t)cap;
    a.list = (const uint2*)p->d_kmlist;
    a.rows = p->d_kmrows;
    a.frames = p->d_jframe;
    a.lms = p->d_mland;
    a.lrows = p->d_mrow;
    a.fixes = p->kfloc.fix;
    a.mask = p->kfloc.mask;
    a.heads = p->d_khead;
    a.kpoints = p->d_kpoints;
    a.owner = p->d_nowner;
    a.n_frames = F;
    a.map_frames = L;
    a.n_pairs = pairs;
    a.n_entries = n;
    a.min_inliers = g.min_inliers ? g.min_inliers : 12u;
    a.use_minimal = g.flags & ORB_ANCHOR_USE_MINIMAL;
    a.min_shared = g.min_shared ? g.min_shared : 8u;
    a.tol = g.scale_tolerance == 0.0f ? 0.1f : g.scale_tolerance;
    a.permille = g.consistent_permille ? g.consistent_permille : 500u;
    a.ratios = p->d_nratio;
    a.links = p->d_nlink;
    a.keys = p->d_nkey;
    a.segs = p->d_nseg;
    a.poses = p->d_npose;
    a.out_rows = p->d_nrow;
    a.out = p->d_nland;
    // the owners of all F frames: rows L .. F - 1 have none
    HIP_TRY(p, hipMemsetAsync(p->d_nowner, 0xff, (size_t)F * cap * sizeof(uint32_t), s));
    HIP_TRY(p, hipMemsetAsync(p->d_nkey, 0, (size_t)F * sizeof(unsigned long long), s));
    HIP_TRY(p, hipMemsetAsync(p->d_nseg, 0, (size_t)F * sizeof(OrbAnchorSegment), s));
    const unsigned fblocks = (F + kAnThreads - 1u) / kAnThreads;
    if (L > 1u) hipLaunchKernelGGL(k_lc_index, dim3(L - 1u, (unsigned)((cap + kLcThreads - 1u) / kLcThreads)), dim3(kLcThreads), 0, s, o);
    hipLaunchKernelGGL(k_an_ratio, dim3(n), dim3(kAnThreads), 0, s, a);
    hipLaunchKernelGGL(k_an_segment, dim3(fblocks), dim3(kAnThreads), 0, s, a);
    hipLaunchKernelGGL(k_an_write, dim3(fblocks), dim3(kAnThreads), 0, s, a);
    if (pairs) {
        const uint32_t per_wg = kAnThreads * kAnLandSlots;
        hipLaunchKernelGGL(k_an_land<kAnLandSlots>, dim3((unsigned)((cap + per_wg - 1u) / per_wg), pairs), dim3(kAnThreads), 0, s, a);
    }
    if (int rc = stage_end(p, ST_ANCHOR, s, F)) return rc;  // p->last_stream stays, as after a guided call
    p->anchor_entries = n;
    p->anchor_pairs = pairs;
    return ORB_OK;
}

int orb_anchor_read(OrbProgram* p, uint32_t frame, OrbAnchorPose* pose) {
    if (!p) return ORB_EINVAL;
    if (p->stage[ST_ANCHOR].extent && !pose) return fail(p, ORB_EINVAL, "anchor_read: pose is NULL");
    return read_stage(p, ST_ANCHOR, frame, pose, p->d_npose, sizeof(OrbAnchorPose), nullptr, nullptr, 0, 0);
}

int orb_anchor_segments(OrbProgram* p, OrbAnchorSegment* dst, size_t n) {
    return p ? table_copy(p, ST_ANCHOR, "anchor_segments", dst, p->d_nseg, n, p->stage[ST_ANCHOR].extent, sizeof(OrbAnchorSegment)) : ORB_EINVAL;
}

int orb_anchor_links(OrbProgram* p, OrbAnchorLink* dst, size_t n) {
    return p ? table_copy(p, ST_ANCHOR, "anchor_links", dst, p->d_nlink, n, p->anchor_entries, sizeof(OrbAnchorLink)) : ORB_EINVAL;
}

int orb_anchor_landmarks(OrbProgram* p, uint32_t pair, OrbAnchorRow* row, OrbLandmark* landmarks, size_t n) {
    if (!p) return ORB_EINVAL;
    // the stage's extent is the frames; the pairs it covered are kept beside it
    if (p->stage[ST_ANCHOR].extent && pair >= p->anchor_pairs) return fail(p, ORB_EINVAL, "anchor_landmarks: pair %u of %u", pair, p->anchor_pairs);
    return read_stage(p, ST_ANCHOR, pair, row, p->d_nrow, sizeof(OrbAnchorRow), landmarks, p->d_nland, sizeof(OrbLandmark), n);
}

int orb_debug_keyframe_buffers(OrbProgram* p, void** rows, void** fixes, void** mask) {
    if (!p) return ORB_EINVAL;
    if (!p->stage[ST_KF_LOC].extent) return fail(p, ORB_ESTATE, "debug_keyframe_buffers before orb_localize_keyframes");
    if (rows) *rows = p->d_kmrows;
    if (fixes) *fixes = p->kfloc.fix;
    if (mask) *mask = p->kfloc.mask;
    return ORB_OK;
}

int orb_match_guided(OrbProgram* p, uint32_t n_frames, const OrbGuideParams* params, const float* models_host, void* stream) {
    if (!p) return ORB_EINVAL;
    OrbGuideParams g{};
    if (params) g = *params;
    if (g.reserved[0] || g.reserved[1] || g.reserved[2] || g.reserved[3]) return fail(p, ORB_EINVAL, "match_guided: reserved words must be 0");
    if (g.source > ORB_GUIDE_HOST || (g.flags & ~ORB_GUIDE_SCALE_RADIUS))
        return fail(p, ORB_EINVAL, "match_guided: unknown source %u or flags 0x%x", g.source, g.flags);
    if (!(std::isfinite(g.radius_px) && g.radius_px >= 0.0f)) return fail(p, ORB_EINVAL, "match_guided: radius_px must be finite and >= 0");
    if (n_frames < 2u || n_frames > p->last_batch)
        return fail(p, ORB_EINVAL, "match_guided: need 2..%u frames of the last batch", p->last_batch);
    if (p->cfg.max_features > (1u << 23)) return fail(p, ORB_EINVAL, "match_guided: max_features must be <= 2^23");
    if ((g.source == ORB_GUIDE_HOST) != (models_host != nullptr))
        return fail(p, ORB_EINVAL, "match_guided: models_host is required with ORB_GUIDE_HOST and only then");
    if (g.source == ORB_GUIDE_VERIFIED) {
        if (int rc = stages_fresh(p, ST_GUIDE, kStages[ST_GUIDE].reads)) return rc;
        const uint32_t verified = p->stage[ST_VERIFY].extent;
        if (n_frames - 1u > verified) return fail(p, ORB_EINVAL, "match_guided: %u pairs, the last verification has %u", n_frames - 1u, verified);
    }
    if (g.radius_px == 0.0f) g.radius_px = 16.0f;
    const size_t cap = p->cfg.max_features;
    guide_grid(p);
    hipStream_t s;
    // the models come from the last verification (waited for whatever the source is)
    if (int rc = stage_open(p, ST_GUIDE, stream, kStages[ST_GUIDE].reads, &s)) return rc;
    const uint32_t pairs = n_frames - 1u;
    if (g.source == ORB_GUIDE_HOST)
        if (int rc = stage_host_models(p, ST_GUIDE, p->guide, models_host, pairs, s)) return rc;
    GuideArgs a = guide_bin_args(p, p->guide);
    a.pairs = pairs;
    a.source = g.source;
    a.vmodel = p->verify.model;
    a.hmodel = p->guide.d_model;
    a.radius = g.radius_px;
    a.octave_window = g.octave_window;
    a.scale_radius = (g.flags & ORB_GUIDE_SCALE_RADIUS) ? 1u : 0u;
    a.out = p->guide.match;
    hipLaunchKernelGGL(k_guide_bin, dim3(n_frames), dim3(kGuideBinThreads), 0, s, a);
    hipLaunchKernelGGL(k_guide_search, dim3(pairs * (unsigned)((cap + kGuideSearchThreads - 1u) / kGuideSearchThreads)),
                       dim3(kGuideSearchThreads), 0, s, a);
    return stage_end(p, ST_GUIDE, s, pairs);  // p->last_stream stays: guided results are read through the stage's event
}

int orb_match_guided_read(OrbProgram* p, uint32_t frame, OrbMatch* dst, size_t n) {
    return p ? read_stage(p, ST_GUIDE, frame, nullptr, nullptr, 0, dst, p->guide.match, sizeof(OrbMatch), n) : ORB_EINVAL;
}

int orb_match_epipolar(OrbProgram* p, uint32_t n_frames, const OrbBandParams* params, const float* models_host, void* stream) {
    if (!p) return ORB_EINVAL;
    OrbBandParams g{};
    if (params) g = *params;
    if (g.reserved[0] || g.reserved[1] || g.reserved[2]) return fail(p, ORB_EINVAL, "match_epipolar: reserved words must be 0");
    if (g.source > ORB_BAND_HOST || (g.flags & ~ORB_BAND_SCALE))
        return fail(p, ORB_EINVAL, "match_epipolar: unknown source %u or flags 0x%x", g.source, g.flags);
    if (!(std::isfinite(g.band_px) && g.band_px >= 0.0f) || !(std::isfinite(g.radius_px) && g.radius_px >= 0.0f))
        return fail(p, ORB_EINVAL, "match_epipolar: band_px and radius_px must be finite and >= 0");
    if (n_frames < 2u || n_frames > p->last_batch)
        return fail(p, ORB_EINVAL, "match_epipolar: need 2..%u frames of the last batch", p->last_batch);
    if (p->cfg.max_features > (1u << 23)) return fail(p, ORB_EINVAL, "match_epipolar: max_features must be <= 2^23");
    if ((g.source == ORB_BAND_HOST) != (models_host != nullptr))
        return fail(p, ORB_EINVAL, "match_epipolar: models_host is required with ORB_BAND_HOST and only then");
    if (g.source == ORB_BAND_VERIFIED) {
        if (int rc = stages_fresh(p, ST_BAND, kStages[ST_BAND].reads)) return rc;
        const uint32_t verified = p->stage[ST_EPI].extent;
        if (n_frames - 1u > verified)
            return fail(p, ORB_EINVAL, "match_epipolar: %u pairs, the last epipolar verification has %u", n_frames - 1u, verified);
    }
    if (g.band_px == 0.0f) g.band_px = 2.0f;
    const size_t cap = p->cfg.max_features;
    guide_grid(p);
    hipStream_t s;
    // the models come from the last epipolar verification (waited for whatever the source is, as the guided call does)
    if (int rc = stage_open(p, ST_BAND, stream, kStages[ST_BAND].reads, &s)) return rc;
    const uint32_t pairs = n_frames - 1u;
    if (g.source == ORB_BAND_HOST)
        if (int rc = stage_host_models(p, ST_BAND, p->band, models_host, pairs, s)) return rc;
    const GuideArgs bin = guide_bin_args(p, p->band);  // k_guide_bin as it is, on this stage's buffers
    BandArgs a{};
    a.counts = bin.counts;
    a.cap = bin.cap;
    a.gw = bin.gw;
    a.gh = bin.gh;
    a.shift = bin.shift;
    a.fw = (float)p->plan.pyr.w[0];
    a.fh = (float)p->plan.pyr.h[0];
    a.srec = bin.srec;
    a.sdesc = bin.sdesc;
    a.cell_start = bin.cell_start;
    a.pairs = pairs;
    a.source = g.source;
    a.vmodel = p->epi.model;
    a.hmodel = p->band.d_model;
    a.band = g.band_px;
    a.radius = g.radius_px;
    a.octave_window = g.octave_window;
    a.scale = (g.flags & ORB_BAND_SCALE) ? 1u : 0u;
    a.out = p->band.match;
    hipLaunchKernelGGL(k_guide_bin, dim3(n_frames), dim3(kGuideBinThreads), 0, s, bin);
    hipLaunchKernelGGL(k_band_search, dim3(pairs * (unsigned)((cap + kGuideSearchThreads - 1u) / kGuideSearchThreads)),
                       dim3(kGuideSearchThreads), 0, s, a);
    return stage_end(p, ST_BAND, s, pairs);  // p->last_stream stays, as after a guided call
}

int orb_match_epipolar_read(OrbProgram* p, uint32_t frame, OrbMatch* dst, size_t n) {
    return p ? read_stage(p, ST_BAND, frame, nullptr, nullptr, 0, dst, p->band.match, sizeof(OrbMatch), n) : ORB_EINVAL;
}

int orb_pose_consecutive(OrbProgram* p, uint32_t n_frames, const OrbPoseParams* params, void* stream) {
    if (!p || !params) return p ? fail(p, ORB_EINVAL, "pose_consecutive: params is NULL") : ORB_EINVAL;
    OrbPoseParams g = *params;
    if (int rc = check_intrinsics(p, ST_POSE, g.fx, g.fy, g.cx, g.cy)) return rc;
    if (!(std::isfinite(g.max_reproj_px) && g.max_reproj_px >= 0.0f) || !(g.max_cos_parallax >= 0.0f && g.max_cos_parallax <= 1.0f) ||
        g.ambiguity_permille > 1000u)
        return fail(p, ORB_EINVAL, "pose_consecutive: max_reproj_px must be finite and >= 0, max_cos_parallax in (0, 1] (0: the default), ambiguity_permille 0..1000");
    if (int rc = stages_fresh(p, ST_POSE, kStages[ST_POSE].reads)) return rc;
    const uint32_t verified = p->stage[ST_EPI].extent;
    if (n_frames < 2u || n_frames - 1u > verified)
        return fail(p, ORB_EINVAL, "pose_consecutive: need 2..%u frames (the last epipolar verification's pairs + 1)", verified + 1u);
    if (g.max_reproj_px == 0.0f) g.max_reproj_px = 2.0f;
    if (g.max_cos_parallax == 0.0f) g.max_cos_parallax = 0.99998f;
    if (!g.min_good) g.min_good = 8u;
    if (!g.ambiguity_permille) g.ambiguity_permille = 700u;
    const size_t cap = p->cfg.max_features;
    hipStream_t s;
    if (int rc = stage_open(p, ST_POSE, stream, kStages[ST_POSE].reads, &s)) return rc;
    const uint32_t pairs = n_frames - 1u;
    PoseArgs a{};
    a.counts = p->d_counts;
    a.corners = p->d_corners;
    a.matches = p->d_matches;
    a.cap = (uint32_t)cap;
    a.vmodel = p->epi.model;
    a.vmask = p->epi.mask;
    a.fx = g.fx;
    a.fy = g.fy;
    a.cx = g.cx;
    a.cy = g.cy;
    a.r2 = g.max_reproj_px * g.max_reproj_px;
    a.c2 = g.max_cos_parallax * g.max_cos_parallax;
    a.min_good = g.min_good;
    a.permille = g.ambiguity_permille;
    a.counters = p->d_pcount;
    a.poses = p->d_pose;
    a.points = p->d_ppoints;
    const dim3 grid(pairs, (unsigned)((cap + kPoseThreads - 1u) / kPoseThreads));
    HIP_TRY(p, hipMemsetAsync(p->d_pcount, 0, (size_t)pairs * kPoseCounters * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_pose_count, grid, dim3(kPoseThreads), 0, s, a);
    hipLaunchKernelGGL(k_pose_points, grid, dim3(kPoseThreads), 0, s, a);
    return stage_end(p, ST_POSE, s, pairs);  // p->last_stream stays, as after a guided call
}

int orb_pose_read(OrbProgram* p, uint32_t pair, OrbPairPose* pose, OrbPoint* points, size_t n) {
    return p ? read_stage(p, ST_POSE, pair, pose, p->d_pose, sizeof(OrbPairPose), points, p->d_ppoints, sizeof(OrbPoint), n) : ORB_EINVAL;
}

int orb_trajectory_consecutive(OrbProgram* p, uint32_t n_frames, const OrbTrajectoryParams* params, void* stream) {
    if (!p) return ORB_EINVAL;
    OrbTrajectoryParams g{};
    if (params) g = *params;
    if (g.reserved[0] | g.reserved[1] | g.reserved[2] | g.reserved[3]) return fail(p, ORB_EINVAL, "trajectory_consecutive: reserved words must be 0");
    if (g.flags & ~ORB_TRAJ_NEED_PARALLAX) return fail(p, ORB_EINVAL, "trajectory_consecutive: unknown flags 0x%x", g.flags);
    if (!(std::isfinite(g.scale_tolerance) && g.scale_tolerance >= 0.0f) || g.consistent_permille > 1000u)
        return fail(p, ORB_EINVAL, "trajectory_consecutive: scale_tolerance must be finite and >= 0, consistent_permille 0..1000");
    const size_t cap = p->cfg.max_features;
    if (cap > (1u << 23)) return fail(p, ORB_EINVAL, "trajectory_consecutive: max_features above 2^23");
    if (int rc = stages_fresh(p, ST_TRAJ, kStages[ST_TRAJ].reads)) return rc;
    const uint32_t most = std::min(4096u, p->stage[ST_POSE].extent + 1u);
    if (n_frames < 2u || n_frames > most) return fail(p, ORB_EINVAL, "trajectory_consecutive: need 2..%u frames (the last pose call's pairs + 1, at most 4096)", most);
    if (!g.min_shared) g.min_shared = 8u;
    if (g.scale_tolerance == 0.0f) g.scale_tolerance = 0.1f;
    if (!g.consistent_permille) g.consistent_permille = 500u;
    hipStream_t s;
    if (int rc = stage_open(p, ST_TRAJ, stream, kStages[ST_TRAJ].reads, &s)) return rc;
    TrajArgs a{};
    a.counts = p->d_counts;
    a.matches = p->d_matches;
    a.cap = (uint32_t)cap;
    a.n_frames = n_frames;
    a.poses = p->d_pose;
    a.points = p->d_ppoints;
    a.min_shared = g.min_shared;
    a.tol = g.scale_tolerance;
    a.permille = g.consistent_permille;
    a.need_parallax = g.flags & ORB_TRAJ_NEED_PARALLAX;
    a.ratios = p->d_jratio;
    a.joints = p->d_jjoint;
    a.frames = p->d_jframe;
    a.map = p->d_jmap;
    if (n_frames > 2u) hipLaunchKernelGGL(k_traj_joint, dim3(n_frames - 2u), dim3(kTrajThreads), 0, s, a);
    hipLaunchKernelGGL(k_traj_chain, dim3(1), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_traj_map, dim3(n_frames - 1u, (unsigned)((cap + kTrajThreads - 1u) / kTrajThreads)), dim3(kTrajThreads), 0, s, a);
    HIP_TRY(p, hipMemsetAsync(p->d_jmap + (size_t)(n_frames - 1u) * cap, 0, cap * sizeof(OrbPoint), s));  // TJ-6: the last frame's row
    return stage_end(p, ST_TRAJ, s, n_frames);  // p->last_stream stays, as after a guided call
}

int orb_trajectory_read(OrbProgram* p, uint32_t frame, OrbFramePose* pose, OrbPoint* points, size_t n) {
    return p ? read_stage(p, ST_TRAJ, frame, pose, p->d_jframe, sizeof(OrbFramePose), points, p->d_jmap, sizeof(OrbPoint), n) : ORB_EINVAL;
}

int orb_localize_consecutive(OrbProgram* p, uint32_t n_frames, const OrbLocalizeParams* params, void* stream) {
    if (!p || !params) return p ? fail(p, ORB_EINVAL, "localize_consecutive: params is NULL") : ORB_EINVAL;
    OrbLocalizeParams g = *params;
    for (uint32_t w : g.reserved)
        if (w) return fail(p, ORB_EINVAL, "localize_consecutive: reserved words must be 0");
    if (int rc = check_intrinsics(p, ST_LOCALIZE, g.fx, g.fy, g.cx, g.cy)) return rc;
    if (!(std::isfinite(g.max_reproj_px) && g.max_reproj_px >= 0.0f)) return fail(p, ORB_EINVAL, "localize_consecutive: max_reproj_px must be finite and >= 0");
    if (int rc = ransac_params(p, ST_LOCALIZE, &g.hypotheses, &g.max_distance, &g.ratio)) return rc;
    if (int rc = stages_fresh(p, ST_LOCALIZE, kStages[ST_LOCALIZE].reads)) return rc;
    // pair f reads the matches of frame f and the pose of pair f - 1
    const uint32_t most = std::min(p->stage[ST_MATCH].extent, p->stage[ST_POSE].extent + 1u);
    if (n_frames < 3u || n_frames > most)
        return fail(p, ORB_EINVAL, "localize_consecutive: need 3..%u frames (the last pose call's pairs + 1)", most);
    if (g.max_reproj_px == 0.0f) g.max_reproj_px = 2.0f;
    hipStream_t s;
    if (int rc = stage_open(p, ST_LOCALIZE, stream, kStages[ST_LOCALIZE].reads, &s)) return rc;
    const uint32_t pairs = n_frames - 1u;
    const LocArgs a = loc_args(p, p->loc, g, kLocSeedSalt);
    hipLaunchKernelGGL(k_loc_gather, dim3(pairs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_loc_score, dim3(pairs, (g.hypotheses + kVerifyHypPerWg - 1u) / kVerifyHypPerWg), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_loc_refine, dim3(pairs), dim3(256), 0, s, a);
    return stage_end(p, ST_LOCALIZE, s, pairs);  // p->last_stream stays, as after a guided call
}

int orb_localize_read(OrbProgram* p, uint32_t pair, OrbFrameFix* fix, uint8_t* inliers, size_t n) {
    return p ? read_stage(p, ST_LOCALIZE, pair, fix, p->loc.fix, sizeof(OrbFrameFix), inliers, p->loc.mask, 1, n) : ORB_EINVAL;
}

int orb_landmarks_consecutive(OrbProgram* p, uint32_t n_frames, const OrbLandmarkParams* params, void* stream) {
    if (!p || !params) return p ? fail(p, ORB_EINVAL, "landmarks_consecutive: params is NULL") : ORB_EINVAL;
    OrbLandmarkParams g = *params;
    if (g.reserved[0] | g.reserved[1]) return fail(p, ORB_EINVAL, "landmarks_consecutive: reserved words must be 0");
    if (int rc = check_intrinsics(p, ST_LANDMARK, g.fx, g.fy, g.cx, g.cy)) return rc;
    if (!(std::isfinite(g.max_reproj_px) && g.max_reproj_px >= 0.0f)) return fail(p, ORB_EINVAL, "landmarks_consecutive: max_reproj_px must be finite and >= 0");
    if (int rc = stages_fresh(p, ST_LANDMARK, kStages[ST_LANDMARK].reads)) return rc;
    // pair p reads the matches of frame p, the points of pair p, the records of frames p and p + 1
    const uint32_t most = std::min(std::min(p->stage[ST_MATCH].extent, p->stage[ST_POSE].extent + 1u), p->stage[ST_TRAJ].extent);
    if (n_frames < 2u || n_frames > most) return fail(p, ORB_EINVAL, "landmarks_consecutive: need 2..%u frames (the last trajectory call's frames)", most);
    if (g.max_reproj_px == 0.0f) g.max_reproj_px = 2.0f;
    if (!g.min_views) g.min_views = 2u;
    const size_t cap = p->cfg.max_features;
    hipStream_t s;
    if (int rc = stage_open(p, ST_LANDMARK, stream, kStages[ST_LANDMARK].reads, &s)) return rc;
    const uint32_t pairs = n_frames - 1u;
    LmArgs a{};
    a.counts = p->d_counts;
    a.corners = p->d_corners;
    a.matches = p->d_matches;
    a.cap = (uint32_t)cap;
    a.n_frames = n_frames;
    a.points = p->d_ppoints;
    a.frames = p->d_jframe;
    a.fx = g.fx;
    a.fy = g.fy;
    a.cx = g.cx;
    a.cy = g.cy;
    a.r2 = g.max_reproj_px * g.max_reproj_px;
    a.min_views = g.min_views;
    a.pred = p->d_mpred;
    a.rows = p->d_mrow;
    a.out = p->d_mland;
    const dim3 grid(pairs, (unsigned)((cap + kLmThreads - 1u) / kLmThreads));
    HIP_TRY(p, hipMemsetAsync(p->d_mpred, 0, (size_t)pairs * cap, s));
    hipLaunchKernelGGL(k_lm_mark, grid, dim3(kLmThreads), 0, s, a);
    hipLaunchKernelGGL(k_lm_fuse, grid, dim3(kLmThreads), 0, s, a);
    return stage_end(p, ST_LANDMARK, s, pairs);  // p->last_stream stays, as after a guided call
}

int orb_landmarks_read(OrbProgram* p, uint32_t pair, OrbLandmarkRow* row, OrbLandmark* landmarks, size_t n) {
    // an OrbLandmark is two float4 of d_mland
    return p ? read_stage(p, ST_LANDMARK, pair, row, p->d_mrow, sizeof(OrbLandmarkRow), landmarks, p->d_mland, sizeof(OrbLandmark), n) : ORB_EINVAL;
}

int orb_bridge_consecutive(OrbProgram* p, uint32_t n_frames, const OrbBridgeParams* params, void* stream) {
    if (!p || !params) return p ? fail(p, ORB_EINVAL, "bridge_consecutive: params is NULL") : ORB_EINVAL;
    OrbBridgeParams g = *params;
    if (g.reserved[0] | g.reserved[1]) return fail(p, ORB_EINVAL, "bridge_consecutive: reserved words must be 0");
    if (int rc = check_intrinsics(p, ST_BRIDGE, g.fx, g.fy, g.cx, g.cy)) return rc;
    if (!(std::isfinite(g.max_reproj_px) && g.max_reproj_px >= 0.0f) || !(std::isfinite(g.scale_tolerance) && g.scale_tolerance >= 0.0f))
        return fail(p, ORB_EINVAL, "bridge_consecutive: max_reproj_px and scale_tolerance must be finite and >= 0");
    if (int rc = ransac_params(p, ST_BRIDGE, &g.hypotheses, &g.max_distance, &g.ratio)) return rc;
    if (g.max_hops > kBrMaxHops || g.window > 4095u || g.consistent_permille > 1000u)
        return fail(p, ORB_EINVAL, "bridge_consecutive: max_hops must be 0..%u, window 0..4095, consistent_permille 0..1000", kBrMaxHops);
    if (int rc = stages_fresh(p, ST_BRIDGE, kStages[ST_BRIDGE].reads)) return rc;
    const Stage* const st = p->stage;
    const uint32_t most = std::min(std::min(st[ST_MATCH].extent, st[ST_POSE].extent + 1u), std::min(st[ST_TRAJ].extent, st[ST_LANDMARK].extent + 1u));
    if (n_frames < 2u || n_frames > most) return fail(p, ORB_EINVAL, "bridge_consecutive: need 2..%u frames (the last landmarks call's frames)", most);
    if (g.max_reproj_px == 0.0f) g.max_reproj_px = 2.0f;
    if (!g.max_hops) g.max_hops = 4u;
    if (!g.window) g.window = 32u;
    if (!g.min_shared) g.min_shared = 8u;
    if (g.scale_tolerance == 0.0f) g.scale_tolerance = 0.1f;
    if (!g.consistent_permille) g.consistent_permille = 500u;
    const size_t cap = p->cfg.max_features;
    hipStream_t s;
    if (int rc = stage_open(p, ST_BRIDGE, stream, kStages[ST_BRIDGE].reads, &s)) return rc;
    BrArgs a{};
    a.loc = loc_args(p, p->bridge, g, kBrSeedSalt);
    a.frames = p->d_jframe;
    a.lms = p->d_mland;
    a.n_frames = n_frames;
    a.max_hops = g.max_hops;
    a.window = g.window;
    a.min_shared = g.min_shared;
    a.tol = g.scale_tolerance;
    a.permille = g.consistent_permille;
    a.ratios = p->d_bratio;
    a.out = p->d_bout;
    HIP_TRY(p, hipMemsetAsync(p->bridge.mask, 0, (size_t)n_frames * cap, s));
    hipLaunchKernelGGL(k_br_gather, dim3(n_frames), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_loc_score, dim3(n_frames, (g.hypotheses + kVerifyHypPerWg - 1u) / kVerifyHypPerWg), dim3(256), 0, s, a.loc);
    hipLaunchKernelGGL(k_br_refine, dim3(n_frames), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_br_chain, dim3(1), dim3(64), 0, s, a);
    return stage_end(p, ST_BRIDGE, s, n_frames);  // p->last_stream stays, as after a guided call
}

int orb_bridge_read(OrbProgram* p, uint32_t frame, OrbBridgePose* pose, uint8_t* inliers, size_t n) {
    return p ? read_stage(p, ST_BRIDGE, frame, pose, p->d_bout, sizeof(OrbBridgePose), inliers, p->bridge.mask, 1, n) : ORB_EINVAL;
}

int orb_adjust_consecutive(OrbProgram* p, uint32_t n_frames, const OrbAdjustParams* params, void* stream) {
    if (!p || !params) return p ? fail(p, ORB_EINVAL, "adjust_consecutive: params is NULL") : ORB_EINVAL;
    OrbAdjustParams g = *params;
    if (g.reserved[0] | g.reserved[1]) return fail(p, ORB_EINVAL, "adjust_consecutive: reserved words must be 0");
    if (int rc = check_intrinsics(p, ST_ADJUST, g.fx, g.fy, g.cx, g.cy)) return rc;
    if (!(std::isfinite(g.max_reproj_px) && g.max_reproj_px >= 0.0f) || g.rounds > 16u)
        return fail(p, ORB_EINVAL, "adjust_consecutive: max_reproj_px must be finite and >= 0, rounds 0..16");
    if (int rc = stages_fresh(p, ST_ADJUST, kStages[ST_ADJUST].reads)) return rc;
    // frame g reads the matches, the frame record and the landmarks of index g (the last frame only its frame record)
    const Stage* const st = p->stage;
    const uint32_t most = std::min(st[ST_MATCH].extent, std::min(st[ST_TRAJ].extent, st[ST_LANDMARK].extent + 1u));
    if (n_frames < 2u || n_frames > most) return fail(p, ORB_EINVAL, "adjust_consecutive: need 2..%u frames (the last landmarks call's frames)", most);
    const size_t cap = p->cfg.max_features;
    if ((unsigned long long)n_frames * cap >= 0xffffffffull)  // BA-3: a key p * cap + i below the "no owner" word
        return fail(p, ORB_EINVAL, "adjust_consecutive: n_frames * max_features must be below 2^32 - 1");
    if (g.max_reproj_px == 0.0f) g.max_reproj_px = 2.0f;
    if (!g.rounds) g.rounds = 4u;
    hipStream_t s;
    if (int rc = stage_open(p, ST_ADJUST, stream, kStages[ST_ADJUST].reads, &s)) return rc;
    BaArgs a{};
    a.counts = p->d_counts;
    a.corners = p->d_corners;
    a.matches = p->d_matches;
    a.cap = (uint32_t)cap;
    a.n_frames = n_frames;
    a.frames = p->d_jframe;
    a.lms = p->d_mland;
    a.fx = g.fx;
    a.fy = g.fy;
    a.cx = g.cx;
    a.cy = g.cy;
    a.r2 = g.max_reproj_px * g.max_reproj_px;
    a.owner = p->d_aowner;
    a.X = p->d_ax;
    a.pose = p->d_apose;
    a.out = p->d_aland;
    const unsigned blocks = (unsigned)((cap + kBaThreads - 1u) / kBaThreads);
    const dim3 by_frame(n_frames, blocks), by_pair(n_frames - 1u, blocks);
    HIP_TRY(p, hipMemsetAsync(p->d_aowner, 0xff, (size_t)n_frames * cap * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_ba_index, by_frame, dim3(kBaThreads), 0, s, a);
    for (uint32_t r = 0; r < g.rounds; r++) {  // BA-6
        hipLaunchKernelGGL(k_ba_motion, dim3(n_frames), dim3(kBaThreads), 0, s, a, r ? kBaStep : kBaFirst);
        hipLaunchKernelGGL(k_ba_structure, by_pair, dim3(kBaThreads), 0, s, a);
    }
    hipLaunchKernelGGL(k_ba_motion, dim3(n_frames), dim3(kBaThreads), 0, s, a, kBaClose);
    hipLaunchKernelGGL(k_ba_check, by_frame, dim3(kBaThreads), 0, s, a);
    return stage_end(p, ST_ADJUST, s, n_frames);  // p->last_stream stays, as after a guided call
}

int orb_adjust_read(OrbProgram* p, uint32_t frame, OrbAdjustedPose* pose, OrbLandmark* landmarks, size_t n) {
    return p ? read_stage(p, ST_ADJUST, frame, pose, p->d_apose, sizeof(OrbAdjustedPose), landmarks, p->d_aland, sizeof(OrbLandmark), n) : ORB_EINVAL;
}

int orb_place_frames(OrbProgram* p, uint32_t n_frames, const OrbPlaceParams* params, const uint8_t* db_host, uint32_t n_db, void* stream) {
    if (!p) return ORB_EINVAL;
    OrbPlaceParams g{};
    if (params) g = *params;
    if (g.reserved || (g.flags & ~ORB_PLACE_KEYFRAMES)) return fail(p, ORB_EINVAL, "place_frames: reserved word must be 0, flags ORB_PLACE_KEYFRAMES or 0");
    if (!g.bits) g.bits = 16u;
    if (!g.tables) g.tables = 8u;
    if (!g.min_gap) g.min_gap = 32u;
    if (!g.top) g.top = 4u;
    if (!g.min_score) g.min_score = 1u;
    if (g.bits < 8u || g.bits > 16u || g.tables > 16u || g.top > 8u || g.min_permille > 1000u)
        return fail(p, ORB_EINVAL, "place_frames: bits must be 8..16, tables 1..16, top 1..8, min_permille 0..1000");
    if (((size_t)g.tables << g.bits) > 8u * (size_t)ORB_PLACE_SIG_BYTES_MAX)
        return fail(p, ORB_EINVAL, "place_frames: tables << bits must not exceed %u bits", 8u * ORB_PLACE_SIG_BYTES_MAX);
    if (n_db > ORB_PLACE_DB_MAX || (db_host != nullptr) != (n_db != 0u))
        return fail(p, ORB_EINVAL, "place_frames: n_db must be 0..%u, and db_host NULL exactly when it is 0", ORB_PLACE_DB_MAX);
    if (!p->last_batch) return fail(p, ORB_ESTATE, "place_frames before a batch");
    if (n_frames < 1u || n_frames > p->last_batch) return fail(p, ORB_EINVAL, "place_frames: need 1..%u frames of the last batch", p->last_batch);
    const bool keyed = (g.flags & ORB_PLACE_KEYFRAMES) != 0u;
    const uint32_t reads = keyed ? 1u << ST_TRACK : 0u;  // the track stage is waited for only when its keyframes are read
    if (keyed) {
        if (int rc = stages_fresh(p, ST_PLACE, reads)) return rc;
        if (p->stage[ST_TRACK].extent < n_frames)
            return fail(p, ORB_ESTATE, "place_frames: %u frames, the last orb_track_consecutive tracked %u", n_frames, p->stage[ST_TRACK].extent);
    }
    const size_t sig_bytes = ((size_t)g.tables << g.bits) / 8u;
    hipStream_t s;
    if (int rc = stage_open(p, ST_PLACE, stream, reads, &s)) return rc;
    if (n_db) {  // the caller's rows are the caller's again when this returns: the copy alone is waited for
        if (!p->place_copied) HIP_TRY(p, hipEventCreateWithFlags(&p->place_copied, hipEventDisableTiming));
        HIP_TRY(p, hipMemcpyAsync(p->d_pdb, db_host, (size_t)n_db * sig_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(p, hipEventRecord(p->place_copied, s));
    }
    PlaceArgs a{};
    a.counts = p->d_counts;
    a.desc = p->d_desc;
    a.cap = p->cfg.max_features;
    a.n_frames = n_frames;
    a.bits = g.bits;
    a.tables = g.tables;
    a.words = (uint32_t)(sig_bytes / 4u);
    a.n_db = n_db;
    a.min_gap = g.min_gap;
    a.top = g.top;
    a.min_score = g.min_score;
    a.min_permille = g.min_permille;
    a.keyframe = keyed ? p->d_tframe : nullptr;
    a.sig = p->d_psig;
    a.db = p->d_pdb;
    a.tbits = p->d_ptbits;
    a.score = p->d_pscore;
    a.rows = p->d_prow;
    const uint32_t n_ids = n_db + n_frames;
    // slices of a signature's words (orb_kernels_place.h): whole chunks, as many as the score buffer has room for beside each other
    const dim3 tiles((n_ids + kPlaceTile - 1u) / kPlaceTile, (n_frames + kPlaceTile - 1u) / kPlaceTile);
    const size_t room = (size_t)p->plan.max_batch * (ORB_PLACE_DB_MAX + p->plan.max_batch) / ((size_t)n_frames * n_ids);
    const uint32_t chunks = (a.words + kPlaceChunk - 1u) / kPlaceChunk;
    const uint32_t wanted = std::max(1u, kPlaceWantedGroups / (tiles.x * tiles.y));
    const uint32_t most = (uint32_t)std::min<size_t>(std::min<size_t>(kPlaceMaxSlices, room), std::min(chunks, wanted));
    const uint32_t per = (chunks + most - 1u) / most;
    a.slice_words = per * kPlaceChunk;
    a.slices = (chunks + per - 1u) / per;
    hipLaunchKernelGGL(k_place_sign, dim3(g.tables, n_frames), dim3(kPlaceSignThreads), 0, s, a);
    hipLaunchKernelGGL(k_place_score, dim3(tiles.x, tiles.y, a.slices), dim3(kPlaceScoreThreads), 0, s, a);
    hipLaunchKernelGGL(k_place_select, dim3(n_frames), dim3(kPlaceSelectThreads), 0, s, a);
    if (int rc = stage_end(p, ST_PLACE, s, n_frames)) return rc;  // p->last_stream stays, as after a guided call
    p->place_sig_bytes = (uint32_t)sig_bytes;
    if (n_db) HIP_TRY(p, hipEventSynchronize(p->place_copied));
    return ORB_OK;
}

}  // extern "C"

namespace {

// What orb_place_read and orb_place_signature share: the state and argument rules, and the wait for the stage's event
int place_read_open(OrbProgram* p, const char* who, uint32_t frame, const void* dst, size_t n) {
    const Stage& last = p->stage[ST_PLACE];
    if (!last.extent) return fail(p, ORB_ESTATE, "%s before place_frames", who);
    if (frame >= last.extent || (!dst && n)) return fail(p, ORB_EINVAL, "%s: frame %u of %u, or the destination of %zu elements is NULL", who, frame, last.extent, n);
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipEventSynchronize(last.done));
    return ORB_OK;
}

}  // namespace

extern "C" {

int orb_place_read(OrbProgram* p, uint32_t frame, OrbPlaceRow* rows, size_t n) {
    if (!p) return ORB_EINVAL;
    if (int rc = place_read_open(p, "place_read", frame, rows, n)) return rc;
    n = std::min<size_t>(n, p->stage[ST_PLACE].extent - frame);
    if (n) HIP_TRY(p, hipMemcpy(rows, p->d_prow + (size_t)frame * kPlaceRowWords, n * sizeof(OrbPlaceRow), hipMemcpyDeviceToHost));
    return ORB_OK;
}

int orb_place_signature(OrbProgram* p, uint32_t frame, uint8_t* dst, size_t n_bytes) {
    if (!p) return ORB_EINVAL;
    if (int rc = place_read_open(p, "place_signature", frame, dst, n_bytes)) return rc;
    n_bytes = std::min<size_t>(n_bytes, p->place_sig_bytes);
    if (n_bytes) HIP_TRY(p, hipMemcpy(dst, (const uint8_t*)p->d_psig + (size_t)frame * p->place_sig_bytes, n_bytes, hipMemcpyDeviceToHost));
    return ORB_OK;
}

int orb_track_consecutive(OrbProgram* p, uint32_t n_frames, const OrbTrackParams* params, void* stream) {
    if (!p) return ORB_EINVAL;
    OrbTrackParams t{};
    if (params) t = *params;
    if (t.reserved) return fail(p, ORB_EINVAL, "track_consecutive: reserved word must be 0");
    if (t.source > ORB_TRACK_MATCHED) return fail(p, ORB_EINVAL, "track_consecutive: unknown source %u", t.source);
    if (t.source == ORB_TRACK_VERIFIED ? (t.max_distance != 0u || t.ratio != 0.0f)
                                       : (t.max_distance > 256u || !(std::isfinite(t.ratio) && t.ratio >= 0.0f)))
        return fail(p, ORB_EINVAL, "track_consecutive: max_distance must be 0..256 and ratio finite and >= 0 (both 0 with ORB_TRACK_VERIFIED)");
    if (!t.min_gap) t.min_gap = 1u;
    if (!t.keep_permille) t.keep_permille = 900u;
    if (t.keep_permille > 1000u || (t.max_gap != 0u && t.max_gap < t.min_gap))
        return fail(p, ORB_EINVAL, "track_consecutive: keep_permille must be 1..1000 and max_gap 0 or >= min_gap");
    if (n_frames < 2u || n_frames > p->last_batch || n_frames > kTrackMaxFrames)
        return fail(p, ORB_EINVAL, "track_consecutive: need 2..%u frames of the last batch", std::min(p->last_batch, kTrackMaxFrames));
    if (p->cfg.max_features > (1u << 23)) return fail(p, ORB_EINVAL, "track_consecutive: max_features must be <= 2^23");
    const Stage &m = p->stage[ST_MATCH], &v = p->stage[ST_VERIFY], &gd = p->stage[ST_GUIDE];
    uint32_t pairs_avail = 0, reads = 0;  // reads: the stages whose results the links come from
    if (t.source == ORB_TRACK_VERIFIED) {  // the inlier bytes and the matches they mark, which must be the ones the verification read
        if (int rc = stages_fresh(p, ST_TRACK, 1u << ST_VERIFY)) return rc;
        if (m.seq != v.seq || m.set != v.set) return fail(p, ORB_ESTATE, "track_consecutive: orb_match_consecutive ran again since orb_verify_consecutive");
        pairs_avail = v.extent;
        reads = 1u << ST_MATCH | 1u << ST_VERIFY;
    } else if (t.source == ORB_TRACK_GUIDED) {
        if (int rc = stages_fresh(p, ST_TRACK, 1u << ST_GUIDE)) return rc;
        pairs_avail = gd.extent;
        reads = 1u << ST_GUIDE;
    } else {
        if (int rc = stages_fresh(p, ST_TRACK, 1u << ST_MATCH)) return rc;
        pairs_avail = m.extent - 1u;
        reads = 1u << ST_MATCH;
    }
    if (n_frames - 1u > pairs_avail)
        return fail(p, ORB_EINVAL, "track_consecutive: %u pairs, the source has %u", n_frames - 1u, pairs_avail);
    if (t.source != ORB_TRACK_VERIFIED) {
        if (!t.max_distance) t.max_distance = 64u;
        if (t.ratio == 0.0f) t.ratio = 0.8f;
    }
    const size_t cap = p->cfg.max_features, B = p->plan.max_batch;
    if (p->track_global_keys < 0) {
        const char* e = getenv("TINYORB_TRACK_GLOBAL_KEYS");
        p->track_global_keys = (e && atoi(e) != 0) ? 1 : 0;
    }
    hipStream_t s;
    if (int rc = stage_open(p, ST_TRACK, stream, reads, &s)) return rc;
    TrackArgs a{};
    a.counts = p->d_counts;
    a.cap = (uint32_t)cap;
    a.frames = n_frames;
    a.stride = (uint32_t)B;
    a.source = t.source;
    a.rec = t.source == ORB_TRACK_GUIDED ? p->guide.match : p->d_matches;
    a.mask = p->verify.mask;
    a.max_distance = t.max_distance;
    a.ratio = t.ratio;
    a.gkeys = p->d_tkeys;
    a.prev = p->d_tprev;
    a.next = p->d_tnext;
    a.links = p->d_tlinks;
    a.ptr[0] = p->d_tptr;
    a.ptr[1] = p->d_tptr + B * cap;
    a.out = p->d_track;
    a.shared = p->d_tshared;
    a.min_gap = t.min_gap;
    a.max_gap = t.max_gap;
    a.keep_permille = t.keep_permille;
    a.min_shared = t.min_shared;
    a.frame_out = p->d_tframe;
    const uint32_t pairs = n_frames - 1u;
    if (!p->track_global_keys && cap <= kTrackLdsKeys)
        hipLaunchKernelGGL(k_track_link<true>, dim3(pairs), dim3(kTrackLinkThreads), cap * sizeof(uint32_t), s, a);
    else
        hipLaunchKernelGGL(k_track_link<false>, dim3(pairs), dim3(kTrackLinkThreads), 0, s, a);
    // pointer doubling: the first round covers chains of 2 links, every further one doubles that; ceil(log2(n_frames - 1)) rounds,
    // at least one, the last of them inside k_track_hist
    uint32_t rounds = 1u;
    while ((1u << rounds) < pairs) rounds++;
    a.first = 1u;
    a.src = 1u;  // the first round writes ptr[0]
    for (uint32_t r = 0; r + 1u < rounds; r++) {
        hipLaunchKernelGGL(k_track_jump, dim3((unsigned)((cap + kTrackJumpThreads - 1u) / kTrackJumpThreads), n_frames),
                           dim3(kTrackJumpThreads), 0, s, a);
        a.first = 0u;
        a.src ^= 1u;
    }
    hipLaunchKernelGGL(k_track_hist, dim3(n_frames), dim3(kTrackHistThreads), 0, s, a);
    hipLaunchKernelGGL(k_track_key, dim3(1), dim3(kTrackKeyThreads), 0, s, a);
    return stage_end(p, ST_TRACK, s, n_frames);  // p->last_stream stays, as after a guided call
}

int orb_track_read(OrbProgram* p, uint32_t frame, OrbTrack* dst, size_t n) {
    return p ? read_stage(p, ST_TRACK, frame, nullptr, nullptr, 0, dst, p->d_track, sizeof(OrbTrack), n) : ORB_EINVAL;
}

int orb_track_frames(OrbProgram* p, OrbTrackFrame* dst, size_t n) {
    if (!p) return ORB_EINVAL;
    const Stage& last = p->stage[ST_TRACK];
    if (!last.extent) return fail(p, ORB_ESTATE, "track_frames before track_consecutive");
    if (!dst && n) return fail(p, ORB_EINVAL, "track_frames: dst is NULL");
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipEventSynchronize(last.done));
    if (n > last.extent) n = last.extent;
    if (n) HIP_TRY(p, hipMemcpy(dst, p->d_tframe, n * sizeof(OrbTrackFrame), hipMemcpyDeviceToHost));
    return ORB_OK;
}

int orb_batch_select_output(OrbProgram* p, uint32_t set) {
    if (!p) return ORB_EINVAL;
    if (set > 1u || !p->out_counts[set])
        return fail(p, ORB_EINVAL, "output set %u does not exist (create with ORB_FLAG_DOUBLE_OUTPUT)", set);
    p->d_counts = p->out_counts[set];
    p->d_corners = p->out_corners[set];
    p->d_desc = p->out_desc[set];
    p->cur_set = set;
    return ORB_OK;
}

int orb_batch_device_buffers(OrbProgram* p, void** counts, void** corners, void** descriptors) {
    if (!p) return ORB_EINVAL;
    if (counts) *counts = p->d_counts;
    if (corners) *corners = p->d_corners;
    if (descriptors) *descriptors = p->d_desc;
    return ORB_OK;
}

int orb_debug_pose_buffers(OrbProgram* p, void** matches, void** poses, void** points) {
    if (!p) return ORB_EINVAL;
    if (!p->d_matches || !p->d_pose || !p->d_ppoints)
        return fail(p, ORB_ESTATE, "debug_pose_buffers before orb_match_consecutive and orb_pose_consecutive");
    if (matches) *matches = p->d_matches;
    if (poses) *poses = p->d_pose;
    if (points) *points = p->d_ppoints;
    return ORB_OK;
}

int orb_debug_frame_buffer(OrbProgram* p, void** frames) {
    if (!p) return ORB_EINVAL;
    if (!p->d_jframe) return fail(p, ORB_ESTATE, "debug_frame_buffer before orb_trajectory_consecutive");
    if (frames) *frames = p->d_jframe;
    return ORB_OK;
}

int orb_level_size(const OrbProgram* p, uint32_t level, uint32_t* width, uint32_t* height) {
    if (!p || level >= p->plan.pyr.depth) return ORB_EINVAL;
    if (width) *width = p->plan.pyr.w[level];
    if (height) *height = p->plan.pyr.h[level];
    return ORB_OK;
}

int orb_debug_read_plane(OrbProgram* p, uint32_t frame, int kind, uint32_t level, uint16_t* dst, size_t n_texels) {
    if (!p) return ORB_EINVAL;
    if (!dst || level >= p->plan.pyr.depth || frame >= p->last_batch || (kind != ORB_PLANE_GRAY && kind != ORB_PLANE_BLUR))
        return fail(p, ORB_EINVAL, "debug_read_plane: bad arguments");
    if (!p->planes_valid || ((p->plan.fused || (p->plan.fused_i && !p->plan.igrey_stored)) && kind == ORB_PLANE_GRAY && level == 0))
        return fail(p, ORB_ESTATE, "plane not materialised by the last call");
    const size_t texels = (size_t)p->plan.pyr.w[level] * p->plan.pyr.h[level];
    if (n_texels != texels) return fail(p, ORB_EINVAL, "debug_read_plane: expected %zu texels", texels);
    if (int rc = orb_batch_sync(p)) return rc;
    const uint16_t* base = (kind == ORB_PLANE_GRAY ? p->d_gray : p->d_blur) + (size_t)frame * p->plan.pyr.stride + p->plan.pyr.off[level];
    HIP_TRY(p, hipMemcpy(dst, base, texels * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if ((p->plan.fused || p->plan.fused_x) && kind == ORB_PLANE_BLUR && p->plan.blur_qa[level] > 0) {
        // the fused path keeps columns [0, qa) of a blur level as one constant per row (k_front, phase C)
        const uint32_t w = p->plan.pyr.w[level], h = p->plan.pyr.h[level], qa = p->plan.blur_qa[level];
        std::vector<uint16_t> rowc(h);
        HIP_TRY(p, hipMemcpy(rowc.data(), p->d_blur_rowc + (size_t)frame * p->plan.pyr.row_stride + p->plan.pyr.row_off[level],
                             h * sizeof(uint16_t), hipMemcpyDeviceToHost));
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < qa && x < w; x++) dst[(size_t)y * w + x] = rowc[y];
    }
    return ORB_OK;
}

int orb_debug_f32_to_f16(OrbProgram* p, const float* src, uint16_t* dst, size_t n) {
    if (!p || !src || !dst) return ORB_EINVAL;
    if (n == 0) return ORB_OK;
    HIP_TRY(p, hipSetDevice(p->device));
    float* d_src = nullptr;
    uint16_t* d_dst = nullptr;
    HIP_TRY(p, hipMalloc(&d_src, n * sizeof(float)));
    hipError_t e = hipMalloc(&d_dst, n * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMemcpy(d_src, src, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_f16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, p->stream, d_src, d_dst, n);
        e = hipStreamSynchronize(p->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(dst, d_dst, n * sizeof(uint16_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_src);
    (void)hipFree(d_dst);
    if (e != hipSuccess) return fail(p, ORB_EHIP, "debug_f32_to_f16: %s", hipGetErrorString(e));
    return ORB_OK;
}

int orb_debug_angle_code(OrbProgram* p, const float* cy, const float* cx, uint32_t* dst, size_t n) {
    if (!p || !cy || !cx || !dst) return ORB_EINVAL;
    if (n == 0) return ORB_OK;
    HIP_TRY(p, hipSetDevice(p->device));
    float *d_cy = nullptr, *d_cx = nullptr;
    uint32_t* d_dst = nullptr;
    HIP_TRY(p, hipMalloc(&d_cy, n * sizeof(float)));
    hipError_t e = hipMalloc(&d_cx, n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&d_dst, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d_cy, cy, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_cx, cx, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_angle, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, p->stream, d_cy, d_cx, d_dst, n);
        e = hipStreamSynchronize(p->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(dst, d_dst, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_cy);
    (void)hipFree(d_cx);
    (void)hipFree(d_dst);
    if (e != hipSuccess) return fail(p, ORB_EHIP, "debug_angle_code: %s", hipGetErrorString(e));
    return ORB_OK;
}

int orb_debug_rot_table(OrbProgram* p, int16_t* dst, size_t n_entries, uint32_t* codes, uint32_t* pitch) {
    if (!p) return ORB_EINVAL;
    if (!p->d_rot) return fail(p, ORB_ESTATE, "this program has no rotated-pattern table");
    const uint32_t n_codes = p->plan.fused_i ? (p->opt.angle_bins ? p->opt.angle_bins : (uint32_t)ORB_ANGLE_STEPS_FULL) : (uint32_t)ORB_ANGLE_STEPS;
    if (codes) *codes = n_codes;
    if (pitch) *pitch = p->plan.fused_i ? p->plan.itiles.pitch : (uint32_t)kNfPatchCols;
    const size_t n = std::min(n_entries, (size_t)n_codes * 512u);
    if (n && !dst) return fail(p, ORB_EINVAL, "dst is NULL");
    HIP_TRY(p, hipSetDevice(p->device));
    if (n) HIP_TRY(p, hipMemcpy(dst, p->d_rot, n * sizeof(int16_t), hipMemcpyDeviceToHost));
    return ORB_OK;
}

// The program's ready-made BlurCol table of one level, as k_blur_col_table wrote it (tinyorb.h).
int orb_debug_blur_col_table(OrbProgram* p, uint32_t level, void* dst, size_t n_entries, uint32_t* n_var, uint32_t* blur_p, uint32_t* blur_q) {
    if (!p) return ORB_EINVAL;
    if (level >= p->plan.pyr.depth) return fail(p, ORB_EINVAL, "level %u of %u", level, p->plan.pyr.depth);
    FrontGeom g = front_geometry(p->plan.pyr, level, 8u, 8u, 1, p->plan.band_rows_lvl[level] ? p->plan.band_rows_lvl[level] : (uint32_t)kFrontRows, p->plan.tile_w_lvl[level]);
    const BlurCol* tab = front_blur_tab(p, g);
    if (n_var) *n_var = tab ? g.n_var : 0u;
    if (blur_p) *blur_p = g.blur_p;
    if (blur_q) *blur_q = g.blur_q;
    const size_t n = tab ? std::min<size_t>(n_entries, g.n_var) : 0;
    if (n && !dst) return fail(p, ORB_EINVAL, "dst is NULL");
    HIP_TRY(p, hipSetDevice(p->device));
    if (n) HIP_TRY(p, hipMemcpy(dst, tab, n * sizeof(BlurCol), hipMemcpyDeviceToHost));
    return ORB_OK;
}

int orb_profile_enable(OrbProgram* p, int enable) {
    if (!p) return ORB_EINVAL;
    p->profiling = enable != 0;
    return ORB_OK;
}

int orb_profile_reset(OrbProgram* p) {
    if (!p) return ORB_EINVAL;
    HIP_TRY(p, hipSetDevice(p->device));
    if (int rc = drain_profile(p)) return rc;
    for (int i = 0; i < ORB_KERNEL_COUNT; i++) {
        p->prof_ms[i] = 0;
        p->prof_n[i] = 0;
    }
    return ORB_OK;
}

int orb_profile_get(OrbProgram* p, int id, double* total_ms, uint64_t* launches) {
    if (!p || id < 0 || id >= ORB_KERNEL_COUNT) return ORB_EINVAL;
    HIP_TRY(p, hipSetDevice(p->device));
    if (int rc = drain_profile(p)) return rc;
    if (total_ms) *total_ms = p->prof_ms[id];
    if (launches) *launches = p->prof_n[id];
    return ORB_OK;
}

int orb_synth_frames_device(OrbProgram* p, uint8_t* frames_dev, uint32_t n_frames, uint32_t seed0, uint32_t flags,
                            uint8_t** out_dev) {
    if (!p) return ORB_EINVAL;
    if (n_frames == 0) return fail(p, ORB_EINVAL, "n_frames is 0");
    HIP_TRY(p, hipSetDevice(p->device));
    if (!frames_dev) {
        if (n_frames > p->plan.max_batch) return fail(p, ORB_EINVAL, "n_frames %u > max_batch %u", n_frames, p->plan.max_batch);
        if (int rc = ensure_input(p)) return rc;
        frames_dev = p->d_input;
        // the program's own slab is what extract_corners works on next: an upload still in flight on the copy stream
        // (orb_write_input_image_pinned) must not land on top of the synthesised frames -- wait for every slab's before the state is reset
        for (uint32_t sl = 0; sl < 2u; sl++)
            if (p->in_async[sl] && p->in_uploaded[sl]) HIP_TRY(p, hipEventSynchronize(p->in_uploaded[sl]));
        p->in_pending = 0u, p->in_last = 0u, p->in_async[0] = p->in_async[1] = false;
    }
    const uint32_t W = p->plan.pyr.w[0], H = p->plan.pyr.h[0];
    if (p->plan.input_y8) flags |= ORB_SYN_Y8;  // a Y8 program's frames are one byte per pixel
    if ((flags & ORB_SYN_Y8) && !p->plan.input_y8) return fail(p, ORB_EINVAL, "ORB_SYN_Y8 needs a program created with ORB_FLAG_INPUT_Y8");
    {
        LaunchScope ls(p, p->stream, KID_SYNTH);
        hipLaunchKernelGGL(k_synth, dim3((W + 255u) / 256u, H, n_frames), dim3(256), 0, p->stream, frames_dev,
                           p->plan.frame_bytes, W, H, seed0, flags);
    }
    HIP_TRY(p, hipGetLastError());
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    if (out_dev) *out_dev = frames_dev;
    return ORB_OK;
}

int orb_debug_stamps(OrbProgram* p, unsigned long long* dst, size_t n) {
    if (!p || !dst) return ORB_EINVAL;
    if (!p->d_stamps) return fail(p, ORB_ESTATE, "stamps are collected only with TINYORB_STAMPS=1");
    if (n > 32) n = 32;
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipDeviceSynchronize());
    HIP_TRY(p, hipMemcpy(dst, p->d_stamps, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return ORB_OK;
}

int orb_copy_to_host(OrbProgram* p, void* dst_host, const void* src_dev, size_t nbytes) {
    if (!p || !dst_host || !src_dev) return ORB_EINVAL;
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipMemcpy(dst_host, src_dev, nbytes, hipMemcpyDeviceToHost));
    return ORB_OK;
}

}  // extern "C"
