/*
 * tinyorb.h -- C ABI of the MI355X-native ORB feature-extraction front-end.
 *
 * This is the drop-in boundary for the `tinyslam::orb` module of ccaven/tinyslam
 * (src/lib.rs:1, src/orb.rs).  Each entry point names the reference item it replaces;
 * INTEGRATION.md shows the Rust `extern "C"` shim a maintainer would add on the reference
 * side.  Plain pointers and sizes only: no C++, HIP or torch types cross this boundary.
 *
 * Semantics follow the reference's literal behaviour:
 * keypoints are FAST-12 corners on an R16Float luminance pyramid (vertically flipped frame),
 * orientation is the 16-pixel ring centroid in milliradians (negative angles stored as 0),
 * descriptors are 256-bit rotated BRIEF on the reference's (x-only, UV-offset) blur.
 *
 * Threading: calls on one OrbProgram must be serialised by the caller; distinct programs are
 * independent (one program = one device + its streams), like one wgpu Device/Queue per
 * OrbProgram in the reference (orb.rs:47-51), and may be created, used and destroyed from
 * different host threads at the same time (tests/test_gpu_round4.py::test_programs_on_different_threads).
 */
#ifndef TINYORB_H
#define TINYORB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TINYORB_ABI_VERSION 5

/* status codes (the reference panics instead: orb.rs:553 unwrap, label look-ups) */
#define ORB_OK 0
#define ORB_EINVAL 1    /* bad argument / configuration (reference: wgpu validation panic) */
#define ORB_EHIP 2      /* HIP runtime failure; text in orb_last_error() */
#define ORB_ECAPACITY 3 /* more corners detected than max_features; first max_features kept */
#define ORB_ESTATE 4    /* call out of order (e.g. read before extract) */

#define ORB_MAX_HIERARCHY_DEPTH 10 /* orb.rs:67 MAX_HIERARCHY_DEPTH */

/* wgpu::Extent3d as used by OrbConfig.image_size (orb.rs:41, 120, 227) */
typedef struct OrbExtent3d {
    uint32_t width;
    uint32_t height;
    uint32_t depth_or_array_layers; /* must be 1 */
} OrbExtent3d;

/* orb.rs:40-45 `pub struct OrbConfig` -- same field order */
typedef struct OrbConfig {
    OrbExtent3d image_size;
    uint32_t max_features;
    uint32_t hierarchy_depth; /* 1..=10; the reference needs >= 2 */
    float initial_threshold;  /* intensity units, [0,1] */
} OrbConfig;

/* orb.rs:10-17 `#[repr(C)] CornerData` == WGSL `Feature` (fast.wgsl:1-6); 16 bytes.
 * x,y are in the octave's own pixel grid of the vertically flipped image (Q2);
 * angle is milliradians 0..3141 (Q7). */
typedef struct CornerData {
    uint32_t x;
    uint32_t y;
    uint32_t angle;
    uint32_t octave;
} CornerData;

/* orb.rs:19-23 `#[repr(C)] CornerDescriptor`; 32 bytes = 8 little-endian u32 words
 * (brief.wgsl:15); bit i of word k is BRIEF test 32k+i (brief.wgsl:47,63). */
typedef struct CornerDescriptor {
    uint8_t bits[32];
} CornerDescriptor;

/* Build-side options with no counterpart in the reference. Zero-initialise for defaults. */
typedef struct OrbOptions {
    int32_t device;       /* HIP device ordinal */
    uint32_t max_batch;   /* frames per batched call; 0 -> 1 */
    uint32_t flags;       /* ORB_FLAG_* */
    uint32_t fast_arc;    /* 0 -> 12 (the reference's FAST-12, fast.wgsl:56-60; 9 with ORB_FLAG_INTENDED);
                           * 9..16: corner = run of >= fast_arc */
    /* Two things the reference's WGSL leaves to the adapter it runs on, as switches (the defaults, 0 and 0, are the
     * canonical decisions CRD-6 / CRD-5 of SURVEY.md 8a; until a dump from the reference itself pins them --
     * rust/dump_config0, tools/pin_oracle.py -- a caller who knows the adapter can follow it).  For the reference's
     * detector only (RGBA or Y8 input): refused together with ORB_FLAG_INTENDED, ORB_FLAG_NMS or a fast_arc other
     * than 12, which have no reference behaviour to follow. */
    uint32_t oob_policy;          /* ORB_OOB_*: what a textureLoad OUTSIDE the addressed level returns (fast.wgsl:78,86,103
                                   * at octaves >= 1, whose guard uses the level-0 size; brief.wgsl:59-60) */
    uint32_t sampler_weight_bits; /* 0: bilinear weights are the exact binary32 fractions; n = 1..23: a sampler that holds
                                   * them in n fractional bits, rounded to nearest, halves up (8 is common): the blur's
                                   * lerps (gaussian_blur_x.wgsl:53-58) and the blit of an odd-sized level (blit.wgsl:35) */
    uint32_t fp_contract;         /* CRD-13: the arithmetic WGSL leaves to the adapter's shader compiler, a mask of
                                   * ORB_FP_*.  0 = every binary32 product and sum of the shaders rounded on its own, dot() reduced from its
                                   * first component (the default).  ORB_FP_CONTRACT_LUMINANCE / _BLUR / _ROTATION: that stage's
                                   * product-and-sum pairs as fused multiply-adds -- dot() (grayscale.wgsl:36), `result += sample *
                                   * weight` (gaussian_blur_x.wgsl:58), matrix * vector (brief.wgsl:53-54).  ORB_FP_LAST_TERM_FIRST: dot()
                                   * and matrix * vector reduced from the last component / column down (Mesa's lowering) instead of the
                                   * first up.  Carried by the fused AND the per-stage kernels at full speed (the luminance and rotation
                                   * forms are template instances, the blur's is a set of scalar constants).  RGBA input, the reference's
                                   * detector.  ABI 4 knew the values 0 and 1 (= every stage contracted, per-stage kernels only). */
    uint32_t angle_bins;          /* ORB_FLAG_INTENDED only (IM-6b): 0 = a descriptor is rotated by its keypoint's milliradian
                                   * code (6284 rotated patterns: a 6.4 MB table that misses the 4 MB L2 of an XCD); N = 8..6284 = by the
                                   * centre of its angle bin, bin = code * N / 6284, centre code = (bin * 6284 + 3142) / N -- 1024 bins are a
                                   * 1 MB table (OpenCV's ORB uses 30).  The keypoint's reported angle stays the milliradian code.
                                   * (Took the last reserved word.) */
} OrbOptions;

#define ORB_OOB_ZERO 0u  /* 0.0 -- Vulkan robust image access; naga: image_load = Unchecked on such devices */
#define ORB_OOB_CLAMP 1u /* every coordinate clamped into [0, size - 1] */
#define ORB_OOB_UMIN 2u  /* naga's `Restrict` policy as its SPIR-V writer emits it: min(coordinate AS UNSIGNED, size - 1) --
                          * a negative coordinate lands on the LAST column / row of the level */

#define ORB_FP_CONTRACT_LUMINANCE 1u
#define ORB_FP_CONTRACT_BLUR 2u
#define ORB_FP_CONTRACT_ROTATION 4u
#define ORB_FP_CONTRACT_ALL 7u
#define ORB_FP_LAST_TERM_FIRST 8u

#define ORB_FLAG_STAGED 1u        /* force the one-kernel-per-stage pipeline (cross-check of the fused path) */
#define ORB_FLAG_DOUBLE_OUTPUT 2u /* two sets of output slabs: batch k+1 computes while batch k is collated */
#define ORB_FLAG_NMS 4u           /* opt-in, NOT in the reference: 3x3 non-maximum suppression per
                                   * octave on the arc score sum(|v - c| - threshold); the counter is then the number
                                   * of survivors. */
#define ORB_FLAG_INTENDED 8u      /* opt-in, NOT in the reference: the algorithm the reference's
                                   * README describes, with the shaders' accidents repaired -- BT.601 luminance (0.299),
                                   * no vertical mirror, a true separable 7-tap Gaussian (X then Y), the octave's own
                                   * border guard, angle codes over the full circle (0..6283 mrad), BRIEF rotated by
                                   * +theta, fast_arc 0 -> 9, optional ORB_FLAG_NMS, and when more than max_features
                                   * keypoints remain the max_features best by score are kept (ties: smaller octave, y,
                                   * x).  Definitions IM-1..IM-8 in DESIGN.md section 8; has its own fused kernels (widths that are a
                                   * multiple of 4), ORB_FLAG_STAGED selects the per-stage cross-check. */

#define ORB_FLAG_INPUT_Y8 16u     /* opt-in, NOT in the reference's code (its roadmap: README.md:42 "Use Y channel of YUV
                                   * stream directly"): frames are ONE byte per pixel (W*H bytes,
                                   * tightly packed) and the grey image is that sample, gray(x,y) = f16(Y(x, H-1-y)/255)
                                   * -- the vertical mirror of the reference's full-screen pass is kept, everything
                                   * downstream is the literal path, unchanged.  Not combined with ORB_FLAG_INTENDED, ORB_FLAG_NMS
                                   * or a fast_arc other than 12 (those have no Y8 definition to check against). */

#define ORB_FLAG_SINGLE_BLOCKING_WAIT 32u /* how orb_extract_corners waits for the device.  Default: the host thread polls a completion word
                                   * in pinned memory (the shortest latency; a spinning thread on a shared box now and then loses its CPU
                                   * for a scheduler slice).  With this flag (or TINYORB_SINGLE_WAIT=block in the environment) the spin is
                                   * bounded to 50 us, after which the thread sleeps until the completion interrupt -- what the reference's
                                   * device.poll(Wait) does (orb.rs:547). */

typedef struct OrbProgram OrbProgram; /* opaque; replaces orb.rs:47-51 `OrbProgram` */

/* ---- lifetime: replaces the struct literal + OrbProgram::init (orb.rs:107-219) ---- */
int orb_program_create(const OrbConfig *config, const OrbOptions *options, OrbProgram **out);
void orb_program_destroy(OrbProgram *p);
/* last error text of this program (or of the failed create when p == NULL) */
const char *orb_last_error(const OrbProgram *p);
uint32_t orb_abi_version(void);
/* "fused" (one kernel per pyramid level + BRIEF) or "staged" (one kernel per reference stage;
 * taken with ORB_FLAG_STAGED or for shapes the fused kernels do not cover: more than 2^26 pixels; the reference's
 * algorithm (RGBA or Y8 input): width > 4096 only -- any other width and any halving run fused; the arc/NMS extensions
 * and the intended mode also need a width that is a multiple of 4, arc/NMS a level 0 that halves exactly.  The band
 * height of the fused kernels is chosen per level from 64 / 32 / 16 / 8 rows). */
const char *orb_pipeline(const OrbProgram *p);
/* Empty unless the program runs on the staged kernels WITHOUT having asked for them: then the reason, e.g.
 * "staged pipeline (...): width 5120 exceeds 4096 (...)".  The same line goes to stderr once per process (silence it
 * with TINYORB_QUIET=1): the staged kernels run at about 1/7 of the fused rate and nobody should find that out late. */
const char *orb_pipeline_note(const OrbProgram *p);

/* ---- single-frame API, one call per reference method ---- */
/* orb.rs:567-583 write_input_image: tightly packed RGBA8, rows of 4*width bytes (ORB_FLAG_INPUT_Y8: rows of width bytes). */
int orb_write_input_image(OrbProgram *p, const uint8_t *bytes, size_t len);
/* The same upload without the wait (orb.rs:567-583 returns after queue.write_texture, before the copy has happened): `bytes`
 * lies in PINNED host memory (orb_host_alloc, or registered with the HIP runtime by the caller) and goes up on the program's
 * copy stream; the call returns at once, orb_upload_sync() waits until the array may be reused.  Images are extracted in the
 * order they were written, and ONE may be written ahead: a camera loop uploads frame k + 1 under the kernels of frame k --
 *     write_pinned(f0);  loop { write_pinned(f[k+1]); extract_corners(&n) [frame k]; read_corners; read_descriptors; }
 * A third write while two images wait returns ORB_ESTATE.  With nothing written since, extract_corners works on the last
 * image again. */
int orb_write_input_image_pinned(OrbProgram *p, const uint8_t *bytes_pinned, size_t len);
/* orb.rs:585-589 set_threshold */
int orb_set_threshold(OrbProgram *p, float threshold);
/* orb.rs:469-557 extract_corners: runs the whole pipeline, blocks until the results are in
 * host staging, returns the RAW detection counter (may exceed max_features, Q9/Q19; then the
 * status is ORB_ECAPACITY and the first max_features records are valid). */
int orb_extract_corners(OrbProgram *p, uint32_t *corner_count);
/* orb.rs:559-561 read_corners: copies min(n, max_features) records from staging. */
int orb_read_corners(OrbProgram *p, CornerData *dst, size_t n);
/* orb.rs:563-565 read_descriptors */
int orb_read_descriptors(OrbProgram *p, CornerDescriptor *dst, size_t n);

/* ---- batched mode (BASELINE.json configs[3], [4]): independent frames, one call ---- */
/* frames_dev: n_frames contiguous RGBA8 frames in DEVICE memory.  stream: a hipStream_t (or
 * NULL for the program's own stream).  Asynchronous: results stay device-resident in the
 * program's output slabs until the next batched call. */
int orb_extract_batch_device(OrbProgram *p, const uint8_t *frames_dev, uint32_t n_frames, void *stream);
/* Same with host frames: they are pinned in place for the call and uploaded in chunks on a copy stream while the
 * kernels of the chunks already on the device run.  Blocks until the uploads are done; results as above. */
int orb_extract_batch_host(OrbProgram *p, const uint8_t *frames_host, uint32_t n_frames);
/* The same for frames that already lie in PINNED host memory (orb_host_alloc, or registered with the HIP runtime by the
 * caller), without pinning and without blocking: returns once the chunked uploads and the kernels are enqueued.
 * orb_upload_sync() waits until the last upload has left the host array (which may then be reused); the kernels may
 * still be running (orb_batch_sync). */
int orb_extract_batch_pinned(OrbProgram *p, const uint8_t *frames_pinned, uint32_t n_frames);
int orb_upload_sync(OrbProgram *p);
/* Wait for the last batched call to finish. */
int orb_batch_sync(OrbProgram *p);
/* Raw per-frame counters of the last batch (synchronises). */
int orb_batch_counts(OrbProgram *p, uint32_t *totals, uint32_t n_frames);
/* Copy up to n records of one frame of the last batch to the host (synchronises). */
int orb_batch_read(OrbProgram *p, uint32_t frame, CornerData *corners, CornerDescriptor *descriptors, size_t n);
/* Selects which output set (0 or 1; 1 needs ORB_FLAG_DOUBLE_OUTPUT) the next batched call writes and the
 * batch read/buffer calls refer to. */
int orb_batch_select_output(OrbProgram *p, uint32_t set);
/* Device pointers of the output slabs, for a device-side collate (RCCL gather):
 * counts[max_batch] u32, corners[max_batch][max_features], descriptors[max_batch][max_features]. */
int orb_batch_device_buffers(OrbProgram *p, void **counts, void **corners, void **descriptors);

/* ---- bulk read-back (orb.rs:537-565: the reference copies counter + corners + descriptors to host staging after
 * every frame; the batched mode returns a whole batch in one go) ----
 * Packs the STORED records (min(counter, max_features) per frame) of the first n_frames frames of the last batch
 * back to back, in frame order, into caller-allocated buffers:
 *   counts[n_frames]       raw per-frame counters (may be NULL)
 *   offsets[n_frames + 1]  exclusive prefix of the stored counts; offsets[n_frames] = total records (may be NULL)
 *   corners / descriptors  [capacity] records; records past `capacity` are dropped (compare offsets[n_frames]).
 * orb_batch_read_all: HOST buffers.  With pinned memory (orb_host_alloc, or registered with the HIP runtime by the
 * caller) the device writes them directly over PCIe, asynchronously on `stream` (NULL: the stream of the batch; then
 * orb_batch_sync() waits for it; another stream is ordered behind the batch and waited for with orb_stream_sync()).
 * Pageable buffers are pinned for the duration of the call, which then blocks.
 * orb_batch_compact_device: the same into DEVICE buffers (payload of a device-side collate). */
int orb_batch_read_all(OrbProgram *p, uint32_t n_frames, uint32_t *counts, uint64_t *offsets, CornerData *corners,
                       CornerDescriptor *descriptors, size_t capacity, void *stream);
int orb_batch_compact_device(OrbProgram *p, uint32_t n_frames, uint32_t *counts_dev, uint64_t *offsets_dev,
                             CornerData *corners_dev, CornerDescriptor *descriptors_dev, size_t capacity, void *stream);
/* The same read-back in two steps, for a host that streams batches: the packed records go to program-owned device
 * memory first and cross PCIe as two exact-size DMA copies (about 56 GB/s on an MI355X box; the device writing pinned
 * host memory itself, as orb_batch_read_all does, reaches about 31 GB/s).
 * orb_batch_pack:  enqueues the packing of the first n_frames frames of the last batch (of the selected output set, see
 *                  orb_batch_select_output) behind that batch; asynchronous.
 * orb_batch_fetch: waits ON THE HOST until the pack of output set `set` (0 or 1) is done, fills counts / offsets (either
 *                  may be NULL) and enqueues the copies of min(total, capacity) records on `stream` (NULL: the program's
 *                  stream); with pinned destinations it returns while they are in flight (orb_stream_sync waits).
 * With ORB_FLAG_DOUBLE_OUTPUT: pack batch k (set k % 2), then fetch batch k - 1 on another stream -- its copies overlap
 * batch k's kernels.  A set may be packed again once its fetch has completed. */
int orb_batch_pack(OrbProgram *p, uint32_t n_frames, void *stream);
int orb_batch_fetch(OrbProgram *p, uint32_t set, uint32_t *counts, uint64_t *offsets, CornerData *corners,
                    CornerDescriptor *descriptors, size_t capacity, void *stream);
/* ---- transport records (multi-GPU collate; not in the reference, which has one device).  On the wire between GPUs a
 * keypoint is ORB_TRANSPORT_RECORD_BYTES = 40 bytes instead of 16 + 32: ten u32 words {x | y << 16, angle | octave << 16,
 * descriptor[8]} (angle code < 6284, octave < 8; frames of 65536 or more texels in either direction are refused with
 * ORB_EINVAL), records of a batch back to back in frame order.  Lossless.
 * orb_batch_pack_transport:  packs the stored records of the first n_frames frames of the batch in output set `set` into
 *     dst_dev[capacity_records] and writes offsets_dev[n_frames + 1] (exclusive prefix of min(counter, max_features);
 *     device memory, may be NULL).  Enqueued on `stream` (NULL: the program's stream) WITHOUT implicit ordering: the caller
 *     orders `stream` behind the batch's kernels (an event, or the same stream).
 * orb_unpack_transport:      n_segments runs of records in src_dev (run i: count[i] records from record src_first[i]) are
 *     expanded into corners_dev / descriptors_dev from record dst_first[i] on; the three arrays are HOST memory, read
 *     during the call.  Enqueued on `stream` (NULL: the program's stream), no implicit ordering. */
#define ORB_TRANSPORT_RECORD_BYTES 40
int orb_batch_pack_transport(OrbProgram *p, uint32_t set, uint32_t n_frames, void *dst_dev, size_t capacity_records,
                             uint64_t *offsets_dev, void *stream);
int orb_unpack_transport(OrbProgram *p, const void *src_dev, uint32_t n_segments, const uint64_t *src_first,
                         const uint64_t *count, const uint64_t *dst_first, CornerData *corners_dev,
                         CornerDescriptor *descriptors_dev, void *stream);
/* Pinned, device-visible host memory for callers without a HIP binding of their own. */
int orb_host_alloc(size_t nbytes, void **out);
void orb_host_free(void *ptr);
/* Waits for `stream` (a hipStream_t; NULL: the program's own stream) on the program's device. */
int orb_stream_sync(OrbProgram *p, void *stream);
/* The program's own stream (a hipStream_t), for callers that order their own work behind it. */
void *orb_program_stream(OrbProgram *p);

/* ---- one node, several GPUs (BASELINE.json configs[4]).  NOT in the reference, which drives one wgpu
 * device (orb.rs:47-51): an OrbNode owns one OrbProgram per listed device of this process and shards a batch of
 * independent frames over them in contiguous ranges (rank r gets frames [F*r/n, F*(r+1)/n) -- no data-path
 * collective).  The only exchange is the collate to the first device: every other device sends its packed records by
 * grouped ncclSend/ncclRecv of their EXACT sizes (RCCL over xGMI, one link per peer; librccl is loaded on first use, a
 * single-GPU program never needs it); the per-frame counters reach the host through pinned memory, no all-gather.
 *
 * A job runs through three stages -- extract, collate_begin, collate_end -- and up to two jobs may be outstanding, so
 * that a host which streams batches overlaps the collate of batch k with the kernels of batch k+1:
 *     orb_node_extract_batch(k);  orb_node_collate_begin() [job k-1];  orb_node_collate_end() [job k-1];  ...
 * One blocking call per job stays available: orb_node_extract_batch + orb_node_collate (the reference's call shape,
 * orb.rs:469-557, is one blocking call per frame). ---- */
typedef struct OrbNode OrbNode;
/* options->device is ignored (devices[] decides); options->max_batch is the largest shard of one device;
 * ORB_FLAG_DOUBLE_OUTPUT is implied.  ORB_FLAG_INPUT_Y8 nodes take one byte per pixel, as their programs do.
 * TINYORB_NODE_LOOPBACK in the environment (tests): 1 = devices may repeat and the exchange uses device copies, not RCCL;
 * 2 = every rank on ONE device and the exchange through RCCL all the same: a one-rank communicator over that device, each
 * rank's records sent to the communicator's own rank (ncclSend + ncclRecv in one group; with n_devices == 1 rank 0's own
 * records take that way too) -- how a one-GPU box executes the RCCL code. */
int orb_node_create(const int *devices, int n_devices, const OrbConfig *config, const OrbOptions *options, OrbNode **out);
void orb_node_destroy(OrbNode *node);
const char *orb_node_last_error(const OrbNode *node);
int orb_node_device_count(const OrbNode *node);
/* The program of rank `rank` (borrowed; e.g. for orb_synth_frames_device or orb_set_threshold on every rank). */
OrbProgram *orb_node_program(OrbNode *node, int rank);
/* Frame range [*lo, *hi) of rank `rank` for a job of n_frames frames. */
int orb_node_shard(const OrbNode *node, uint32_t n_frames, int rank, uint32_t *lo, uint32_t *hi);
/* Stage 1.  frames_dev[r]: rank r's shard, resident on ITS device (frames lo_r.. of the job, contiguous).  Asynchronous:
 * every device runs its shard on its own stream and packs the results behind it on a second one.  ORB_ESTATE when two
 * jobs are already outstanding. */
int orb_node_extract_batch(OrbNode *node, const uint8_t *const *frames_dev, uint32_t n_frames);
/* The same from one host array of n_frames frames: every shard is uploaded in chunks while its first chunks already
 * compute (orb_extract_batch_pinned; the array is pinned in place for the call).  Returns when the uploads are done. */
int orb_node_extract_batch_host(OrbNode *node, const uint8_t *frames_host, uint32_t n_frames);
/* Stage 2, for the oldest job that has not begun it: waits on the host for that job's per-frame counters (its kernels
 * and pack; later jobs keep the devices busy meanwhile) and enqueues the exchange -- exact-size transport records to
 * the first device, expanded there behind its own records.  Does not wait for the exchange. */
int orb_node_collate_begin(OrbNode *node);
/* Stage 3, for the oldest job (begins its exchange if nobody has): blocks until the collated result is on the first
 * device.  counts[n_frames] and offsets[n_frames + 1] are HOST arrays (as in orb_batch_read_all; either may be NULL);
 * *corners_dev / *descriptors_dev receive the addresses of the packed records (frame order), which stay valid while
 * the next TWO jobs are extracted (three result buffers). */
int orb_node_collate_end(OrbNode *node, uint32_t *counts, uint64_t *offsets, void **corners_dev, void **descriptors_dev);
/* orb_node_collate_begin + orb_node_collate_end for the oldest job: the blocking form. */
int orb_node_collate(OrbNode *node, uint32_t *counts, uint64_t *offsets, void **corners_dev, void **descriptors_dev);
/* Jobs extracted and not yet ended (0..2). */
int orb_node_pending(const OrbNode *node);
/* How the records of ranks >= 1 reach the first device: "rccl" (ncclSend/ncclRecv between devices), "rccl-self"
 * (TINYORB_NODE_LOOPBACK=2), "copies" (TINYORB_NODE_LOOPBACK=1) or "none" (one device, nothing to exchange); and the
 * number of ncclSend + ncclRecv pairs enqueued so far.  A failure in the middle of an enqueue sequence (HIP or RCCL) takes
 * the node out of service: every later extract / collate returns ORB_ESTATE -- destroy it and create a new one. */
const char *orb_node_exchange_backend(const OrbNode *node);
uint64_t orb_node_rccl_pairs(const OrbNode *node);
/* Where a job's results end up.  ORB_NODE_RESULTS_ROOT (default): collated on the first device, as described above.
 * ORB_NODE_RESULTS_SHARDED: nothing is exchanged -- every rank packs the stored records of its shard back to back, in frame
 * order, into buffers on ITS OWN device (for a consumer that runs where the frames were extracted, e.g. a matcher per GPU:
 * with eight GPUs the collate into one device runs at the rate of its links, the kernels do not).  The three stages and their
 * overlap stay; orb_node_collate_end fills counts[] and offsets[] as before (offsets[] keep counting across ranks: rank r's
 * records are offsets[first frame of r] .. and lie at the start of its own buffer) and returns NULL record pointers;
 * orb_node_shard_result hands out rank r's buffers of the job ended last (valid while the next two jobs are extracted).
 * May only be changed while no job is outstanding. */
#define ORB_NODE_RESULTS_ROOT 0
#define ORB_NODE_RESULTS_SHARDED 1
int orb_node_set_results(OrbNode *node, int where);
int orb_node_shard_result(OrbNode *node, int rank, uint32_t *n_frames, uint64_t *n_records, void **corners_dev,
                          void **descriptors_dev);
/* Copies the records of the job ended last to the host (sharded results: rank by rank, i.e. still in frame order); capacity in
 * records. */
int orb_node_read_collated(OrbNode *node, CornerData *corners, CornerDescriptor *descriptors, size_t capacity);

/* ---- descriptor matching (the SLAM stage that consumes this path's output; NOT in the
 * reference, definition is the build's own) ----
 * Brute-force Hamming matching between consecutive frames of the last batch: for every stored keypoint i of frame
 * f (query) the stored keypoint j of frame f+1 with the smallest popcount(desc_f[i] ^ desc_f+1[j]); ties go to the
 * smallest j.  `second` is the smallest distance over all other j (for a ratio test).  Without candidates:
 * index = ORB_MATCH_NONE, distance = second = 0xffff; with one candidate second = 0xffff.
 * Runs on the matrix cores (descriptors as +-1 in fp4, block-scaled MFMA: csrc/orb_kernels_match.h; the first call
 * allocates 128 bytes per record of a batch for them) when max_features <= 16383, else on the vector unit. */
typedef struct {
    uint32_t index;
    uint16_t distance;
    uint16_t second;
} OrbMatch;
#define ORB_MATCH_NONE 0xffffffffu
/* Matches frame f against f+1 for f in [0, n_frames - 1) of the last batch, asynchronously on `stream` (NULL: the
 * program's stream; it is ordered after the batch that produced the descriptors when that ran on the same stream).  A program has ONE
 * result buffer (and one buffer of expanded descriptors), whichever output set the batch went to: a call overwrites the matches of the
 * call before -- read them first -- and a call on another stream than the last one is ordered behind it. */
int orb_match_consecutive(OrbProgram *p, uint32_t n_frames, void *stream);
/* Copy up to n matches of the queries of `frame` to the host (synchronises). */
int orb_match_read(OrbProgram *p, uint32_t frame, OrbMatch *dst, size_t n);

/* ---- geometric verification of the matches (NOT in the reference; definition GV-1..GV-7 in DESIGN.md section 13) ----
 * For every consecutive pair (f, f+1) of the last orb_match_consecutive call: the matches that pass a distance and ratio
 * filter are the candidates; a RANSAC over minimal 4-point homographies picks the model with the most inliers (one-way
 * transfer error below inlier_px), a least-squares refit over its inliers replaces it unless it loses 1/16 of them or more,
 * and every candidate gets an inlier byte.  Coordinates are the level-0 pixel centres of orb_corner_level0_xy: in the
 * default (literal) mode y is therefore in the reference's vertically mirrored frame (row 0 = the image's bottom row);
 * with ORB_FLAG_INTENDED there is no mirror.  Integer and binary32 arithmetic only (+ - * /, no sqrt), in a fixed order:
 * a CPU restatement gives the same bits. */
typedef struct {           /* zero-initialised = the defaults */
    uint32_t hypotheses;   /* minimal samples per pair, 1..4096 (0: 512) */
    uint32_t max_distance; /* Hamming distance a candidate may have, 0..256 (0: 64) */
    float ratio;           /* candidate iff distance < ratio * second, in binary32 (0: 0.8); finite, >= 0 */
    float inlier_px;       /* one-way transfer error threshold in level-0 pixels (0: 3.0); finite, >= 0 */
    uint32_t seed;         /* of the sample draws */
    uint32_t reserved[3];  /* must be 0 (ORB_EINVAL otherwise) */
} OrbVerifyParams;         /* 32 bytes */

typedef struct {
    float h[9];            /* row-major, level-0 keypoint coordinates of frame f -> frame f+1, divided by its [2][2] entry:
                            * h[8] == 1 when status is OK / MINIMAL (unless that entry of the kept model is 0 -- a model that
                            * sends the pixel (0, 0) to infinity -- and then every h is inf / NaN; the inliers and the bytes
                            * stay valid); all 0 for FEW / DEGENERATE */
    uint32_t candidates;   /* matches that passed the filters */
    uint32_t inliers;      /* candidates that are inliers of the model in h */
    uint32_t hypothesis;   /* index of the winning minimal sample, ORB_MATCH_NONE if none was valid */
    uint32_t status;       /* ORB_VERIFY_* */
    uint32_t reserved[3];  /* 0 */
} OrbPairModel;            /* 64 bytes */

#define ORB_VERIFY_OK 0u         /* the least-squares refit over the winner's inliers */
#define ORB_VERIFY_FEW 1u        /* fewer than 4 candidates: no model */
#define ORB_VERIFY_DEGENERATE 2u /* no hypothesis drew a valid (non-degenerate) sample: no model */
#define ORB_VERIFY_MINIMAL 3u    /* the refit failed or kept fewer than 15/16 of the inliers: the winning minimal model */

/* Verifies the pairs (f, f+1), f in [0, n_frames - 1), of the last orb_match_consecutive call (params NULL: the defaults).
 * ORB_ESTATE when there was no such call, when a batch was extracted after it or when orb_batch_select_output changed the
 * output set since; ORB_EINVAL when n_frames exceeds the matched frame count (or is < 2) or a parameter is out of range.
 * Asynchronous on `stream` -- NULL: the stream of the program's last batched call, match or verification (its own stream
 * before any), as the matcher chooses -- and ordered behind the matcher's last call and the last verification when they ran
 * on another stream.  ONE result buffer per program (allocated by the first call): a call overwrites the results of the
 * call before. */
int orb_verify_consecutive(OrbProgram *p, uint32_t n_frames, const OrbVerifyParams *params, void *stream);
/* Synchronises, copies the record of `pair` and min(n, max_features) inlier bytes (may be NULL when n == 0), indexed like
 * orb_match_read's output (query i of frame `pair`): 1 for a candidate that is an inlier of the model in the record, 0
 * for every other query. */
int orb_verify_read(OrbProgram *p, uint32_t pair, OrbPairModel *model, uint8_t *inlier, size_t n);

/* ---- epipolar verification of the matches (NOT in the reference; definition EP-1..EP-6 in DESIGN.md section 16) ----
 * The homography above is the right model for a planar scene or a camera that only rotates; a camera that translates through
 * a scene with depth needs the epipolar constraint x2^T F x1 = 0.  Same candidates (GV-1) and coordinates (GV-2) as
 * orb_verify_consecutive; a RANSAC over minimal 8-point fundamental matrices (null vector by elimination with complete
 * pivoting) picks the model with the most inliers (Sampson distance below inlier_px, tested without a division or a square
 * root), a least-squares refit over its inliers replaces it unless it loses 1/16 of them or more, and every candidate gets an
 * inlier byte.  OrbVerifyParams and its defaults as above; the record is an OrbPairModel whose h holds F (row-major, level-0
 * keypoint coordinates, x2^T F x1 = 0 for x1 of frame f and x2 of frame f+1), divided by its first entry of largest magnitude
 * (that entry is 1; all 0 for FEW / DEGENERATE).  F is NOT projected to rank 2 (that needs an SVD).  The status codes keep
 * their meaning, except that ORB_VERIFY_FEW means fewer than 8 candidates.  Integer and binary32 arithmetic only, in a fixed
 * order: a CPU restatement gives the same bits.
 *
 * State, arguments and streams as orb_verify_consecutive: ORB_ESTATE without an orb_match_consecutive of the current batch and
 * output set; ORB_EINVAL for n_frames or a parameter out of range; asynchronous on `stream` (NULL: as orb_verify_consecutive),
 * ordered behind the matcher's last call and the last epipolar call on another stream; orb_match_consecutive waits for an
 * epipolar call on another stream.  Result buffers of its own (allocated by the first call): it never writes
 * orb_verify_consecutive's results, and orb_match_guided and orb_track_consecutive keep reading those. */
int orb_verify_epipolar(OrbProgram *p, uint32_t n_frames, const OrbVerifyParams *params, void *stream);
/* As orb_verify_read, for the last orb_verify_epipolar call (ORB_ESTATE before the first). */
int orb_verify_epipolar_read(OrbProgram *p, uint32_t pair, OrbPairModel *model, uint8_t *inlier, size_t n);

/* ---- guided matching, "search by projection" (NOT in the reference; definition GM-1..GM-6 in DESIGN.md section 14) ----
 * For every consecutive pair (f, f+1) of the last batch: each stored keypoint i of frame f is sent through a row-major 3 x 3
 * model M (level-0 coordinates of orb_corner_level0_xy, binary32, no fused operations, in the order
 * w = (m6 x + m7 y) + m8, px = ((m0 x + m1 y) + m2) / w, py = ((m3 x + m4 y) + m5) / w) and matched against the stored
 * keypoints j of frame f+1 with fabsf(x_j - px) <= r and fabsf(y_j - py) <= r (and, with octave_window n > 0,
 * |octave_j - octave_i| < n) only.  The record is orb_match_consecutive's restricted to that window: the smallest
 * popcount(desc_f[i] ^ desc_f+1[j]), ties to the smallest j, `second` the smallest distance over the window's other j;
 * ORB_MATCH_NONE / 0xffff / 0xffff without a target or without a prediction (w not > 0, px or py not finite, no model).
 * Queries past a frame's stored keypoints get ORB_MATCH_NONE records.  With ORB_GUIDE_IDENTITY, octave_window 0 and a radius
 * that covers the frame every record equals orb_match_consecutive's. */
typedef struct {              /* zero-initialised = the defaults */
    uint32_t source;          /* ORB_GUIDE_VERIFIED (0), ORB_GUIDE_IDENTITY (1), ORB_GUIDE_HOST (2) */
    float radius_px;          /* window half-size r in level-0 pixels, finite, >= 0 (0: 16) */
    uint32_t octave_window;   /* 0: any octave; n: |octave_j - octave_i| < n */
    uint32_t flags;           /* ORB_GUIDE_SCALE_RADIUS */
    uint32_t reserved[4];     /* must be 0 (ORB_EINVAL otherwise) */
} OrbGuideParams;             /* 32 bytes */

#define ORB_GUIDE_VERIFIED 0u     /* the h of the pair's record from the last orb_verify_consecutive, if its status is OK or MINIMAL */
#define ORB_GUIDE_IDENTITY 1u     /* the unit matrix: a window around the keypoint's own position */
#define ORB_GUIDE_HOST 2u         /* models_host: (n_frames - 1) x 9 floats, read during the call */
#define ORB_GUIDE_SCALE_RADIUS 1u /* r = radius_px * 2^octave_i */

/* Matches the pairs (f, f+1), f in [0, n_frames - 1), of the last batch (params NULL: the defaults).  ORB_EINVAL when n_frames is
 * not 2..frames of the last batch, max_features > 2^23, models_host is NULL with ORB_GUIDE_HOST or not NULL with another source,
 * or a parameter is out of range; with ORB_GUIDE_VERIFIED, ORB_ESTATE when the last orb_verify_consecutive was not of the
 * current batch and output set, ORB_EINVAL when n_frames - 1 exceeds its pairs.  Asynchronous on `stream` (NULL: the stream of
 * the program's last batched call, match or verification, as the matcher chooses; the guided call does not change it), ordered
 * behind the last verification and the last guided call when they ran on another stream.  ONE result buffer per program
 * (allocated by the first call), apart from orb_match_consecutive's: a call overwrites the results of the call before and
 * leaves the matcher's and the verifier's untouched.  Environment: TINYORB_GUIDE_CELL (read once per program) sets the
 * cell size of the acceleration grid, which changes no record. */
int orb_match_guided(OrbProgram *p, uint32_t n_frames, const OrbGuideParams *params, const float *models_host, void *stream);
/* Copy up to n records of the queries of frame `frame` of the last orb_match_guided call to the host (synchronises);
 * ORB_ESTATE before any call, ORB_EINVAL for a frame outside its pairs. */
int orb_match_guided_read(OrbProgram *p, uint32_t frame, OrbMatch *dst, size_t n);

/* ---- epipolar-band guided matching, "search for triangulation" (NOT in the reference; definition EB-1..EB-6 in DESIGN.md
 * section 18) ----
 * For every consecutive pair (f, f+1) of the last batch: each stored keypoint i of frame f is sent to its epipolar line in
 * frame f+1 by the pair's row-major fundamental matrix F (x2^T F x1 = 0, level-0 coordinates of orb_corner_level0_xy, binary32,
 * no fused operations, in the order a0 = (f0 x + f1 y) + f2, a1 = (f3 x + f4 y) + f5, a2 = (f6 x + f7 y) + f8,
 * n2 = a0 a0 + a1 a1, t = (d d) n2) and matched against the stored keypoints j of frame f+1 with r = (a0 x_j + a1 y_j) + a2,
 * r r <= t -- within d pixels of the line, tested without a division or a square root -- and, with radius_px R > 0,
 * fabsf(x_j - x) <= R and fabsf(y_j - y) <= R around the query's OWN position (and, with octave_window n > 0,
 * |octave_j - octave_i| < n) only.  The record is orb_match_consecutive's restricted to that set, as orb_match_guided's is to
 * its window; ORB_MATCH_NONE / 0xffff / 0xffff without a target or without a line (no model, a0, a1, a2 or t not finite, or
 * n2 < 2^-64: the query is at the epipole, or F is zero).  Queries past a frame's stored keypoints get ORB_MATCH_NONE records.
 * With ORB_BAND_HOST, a band that covers the frame (e.g. 1e6) and radius_px 0, every query that has a line gets
 * orb_match_consecutive's record. */
typedef struct {              /* zero-initialised = the defaults */
    uint32_t source;          /* ORB_BAND_VERIFIED (0), ORB_BAND_HOST (1) */
    float band_px;            /* half-width d of the band around the line, level-0 pixels, finite, >= 0 (0: 2.0) */
    float radius_px;          /* window half-size R around the query's OWN position, finite, >= 0 (0: no window, the whole line) */
    uint32_t octave_window;   /* as OrbGuideParams */
    uint32_t flags;           /* ORB_BAND_SCALE */
    uint32_t reserved[3];     /* must be 0 (ORB_EINVAL otherwise) */
} OrbBandParams;              /* 32 bytes */

#define ORB_BAND_VERIFIED 0u  /* h (= F) of the pair's record of the last orb_verify_epipolar, status OK or MINIMAL */
#define ORB_BAND_HOST 1u      /* models_host: (n_frames - 1) x 9 floats, row-major F, read during the call */
#define ORB_BAND_SCALE 1u     /* d and R multiplied by 2^octave_i (exact) */

/* Matches the pairs (f, f+1), f in [0, n_frames - 1), of the last batch (params NULL: the defaults).  ORB_EINVAL when n_frames is
 * not 2..frames of the last batch, max_features > 2^23, models_host is NULL with ORB_BAND_HOST or not NULL with
 * ORB_BAND_VERIFIED, or a parameter is out of range; with ORB_BAND_VERIFIED, ORB_ESTATE when the last orb_verify_epipolar was
 * not of the current batch and output set, ORB_EINVAL when n_frames - 1 exceeds its pairs.  Asynchronous on `stream` (NULL: as
 * orb_match_guided chooses; the call does not change it), ordered behind the last epipolar verification and the last call of
 * its own when they ran on another stream; orb_verify_epipolar waits for such a call on another stream before it overwrites
 * the models.  ONE result buffer per program (allocated by the first call), of its own: the matcher's, the verifiers', the
 * guided call's and the track call's results are never written.  TINYORB_GUIDE_CELL sets the cell size of this call's grid
 * too, and changes no record. */
int orb_match_epipolar(OrbProgram *p, uint32_t n_frames, const OrbBandParams *params, const float *models_host, void *stream);
/* Copy up to n records of the queries of frame `frame` of the last orb_match_epipolar call to the host (synchronises);
 * ORB_ESTATE before any call, ORB_EINVAL for a frame outside its pairs. */
int orb_match_epipolar_read(OrbProgram *p, uint32_t frame, OrbMatch *dst, size_t n);

/* ---- relative pose and triangulation of the epipolar inliers (NOT in the reference; definition RP-1..RP-7 in DESIGN.md
 * section 19) ----
 * For every consecutive pair (f, f+1) of the last batch: the F of the last orb_verify_epipolar (status OK or MINIMAL) and the
 * caller's pinhole intrinsics give the essential matrix E = K^T F K, scaled to sum(E^2) = 2; the baseline direction t is the row
 * of I - E E^T with the largest diagonal entry, divided by that entry's square root; the two rotations are Cof(E) - [t]x E and
 * Cof(E) + [t]x E (Horn's closed form), each taken to the nearest rotation by three steps R <- (R + Cof(R) / det R) / 2.  No SVD
 * and no iteration whose length depends on the data.  Every query i whose epipolar inlier byte is 1, with its partner
 * j = the matcher's index, is triangulated under the four candidates (Ra, t), (Ra, -t), (Rb, t), (Rb, -t): rays
 * d = ((u - cx) / fx, (v - cy) / fy, 1), depths z1, z2 from the 2 x 2 normal equations of z1 R d1 - z2 d2 = -t, X = z1 d1.  A
 * point is GOOD when both depths are finite and > 0 and X reprojects within max_reproj_px of the keypoint in frame f+1; it has
 * PARALLAX when the cosine of the angle between its rays is below max_cos_parallax.  The candidate with the most good points
 * wins (the first of equals).  Binary32 arithmetic in a fixed order, no fused operations: a CPU restatement gives the same bits.
 * X2 = R X1 + t takes camera f's frame to camera f+1's; the scale of t is unobservable, so |t| = 1 and the points share it. */
typedef struct {            /* zero-initialised is NOT valid: fx, fy must be > 0 */
    float fx, fy, cx, cy;   /* pinhole intrinsics in orb_corner_level0_xy coordinates (literal mode: the mirrored frame) */
    float max_reproj_px;    /* frame f+1 reprojection error a good point may have (0: 2.0); finite, >= 0 */
    float max_cos_parallax; /* a point has parallax iff cos(angle between its rays) < this (0: 0.99998); in (0, 1] */
    uint32_t min_good;      /* good points the winner needs (0: 8) */
    uint32_t ambiguity_permille; /* AMBIGUOUS iff 1000*second >= this*best (0: 700); 1..1000 */
} OrbPoseParams;            /* 32 bytes */

#define ORB_POSE_OK 0u           /* R, t and the points can be used */
#define ORB_POSE_NOMODEL 1u      /* no F (the epipolar status is FEW or DEGENERATE), or E, t or both rotations degenerate: all 0 */
#define ORB_POSE_FEW 2u          /* fewer than 8 epipolar inliers (all 0), or the winner has fewer than min_good good points */
#define ORB_POSE_AMBIGUOUS 3u    /* the runner-up explains nearly as many points */
#define ORB_POSE_LOW_PARALLAX 4u /* fewer than half of the winner's good points have parallax: R holds, t and the depths do not */

typedef struct {
    float r[9];             /* row-major R, X2 = R X1 + t */
    float t[3];             /* unit length (scale is unobservable) */
    uint32_t inliers;       /* epipolar inliers considered */
    uint32_t good;          /* of them: in front of both cameras and within max_reproj_px, under the winner */
    uint32_t second;        /* the runner-up candidate's good count */
    uint32_t status;        /* ORB_POSE_* */
} OrbPairPose;              /* 64 bytes */

#define ORB_POINT_GOOD 1u
#define ORB_POINT_PARALLAX 2u
typedef struct { float x, y, z; uint32_t flags; } OrbPoint;  /* 16 bytes; camera-f frame; flags: ORB_POINT_GOOD, ORB_POINT_PARALLAX */

/* Poses of the pairs (f, f+1), f in [0, n_frames - 1), of the last batch.  ORB_EINVAL for a NULL program or params, fx or fy not
 * finite or not > 0, cx or cy not finite, another parameter out of range, or n_frames not in 2 .. the last
 * orb_verify_epipolar's pairs + 1; ORB_ESTATE unless the last orb_match_consecutive and the last orb_verify_epipolar are both of
 * the current batch and output set.  Asynchronous on `stream` (NULL: as orb_match_guided chooses; the call does not change it),
 * ordered behind the matcher's and the epipolar verifier's last calls and the last call of its own when they ran on another
 * stream; orb_match_consecutive and orb_verify_epipolar wait for such a call on another stream before they overwrite what it
 * reads.  Result buffers of its own (allocated by the first call): no other stage's results are ever written.  R, t and the
 * counts are written for every status except NOMODEL and the FEW of fewer than 8 inliers (all 0 then), and so are the points:
 * the status says what to trust. */
int orb_pose_consecutive(OrbProgram *p, uint32_t n_frames, const OrbPoseParams *params, void *stream);
/* Copy the record of pair `pair` of the last orb_pose_consecutive call (pose may be NULL) and up to n points of the queries of
 * frame `pair` (indexed as orb_match_read; 0, 0, 0, flags 0 for every query that is not a good point) to the host
 * (synchronises); ORB_ESTATE before any call, ORB_EINVAL for a pair outside its pairs or points NULL with n > 0. */
int orb_pose_read(OrbProgram *p, uint32_t pair, OrbPairPose *pose, OrbPoint *points, size_t n);

/* ---- trajectory: the pair poses chained into one camera path and one point map with a common scale (NOT in the reference;
 * definition TJ-1..TJ-7 in DESIGN.md section 20) ----
 * Every pair of orb_pose_consecutive stands alone: |t| = 1 and the points are in the pair's own camera frame and unit.  Frame f is
 * the joint of the pairs (f-1, f) and (f, f+1): pair f-1 triangulated point i from camera f-1, the matcher's index j says which
 * keypoint of frame f it is, and pair f triangulated j again from camera f.  When both poses are OK and both points GOOD, the
 * depth of R X + t (pair f-1's pose and point) over the depth of pair f's point is the ratio of the two baselines.  The joint's
 * step g is the lower median of its ratios; the joint holds when there are at least min_shared ratios of which at least
 * consistent_permille per thousand lie within scale_tolerance * g of g.  Frame poses follow in sequence: a pose that is not OK
 * loses the frame (LOST: a new origin), an OK pose after one that is not starts a segment (START: the pair's own pose, scale 1),
 * a joint that does not hold restarts one (RESTART_FEW, RESTART_SPREAD), and one that holds chains: scale = scale * g,
 * R = P.r R', t = P.r t' + scale P.t, with R taken one polar step towards a rotation.  The points of pair f are mapped into the
 * frame and unit of frame f+1's origin.  Binary32 arithmetic in a fixed order, no fused operations: a CPU restatement gives the
 * same bits. */
typedef struct {                  /* zero-initialised = the defaults */
    uint32_t min_shared;          /* ratios a joint needs (0: 8) */
    float scale_tolerance;        /* a ratio is consistent within this share of the median (0: 0.1); finite, >= 0 */
    uint32_t consistent_permille; /* consistent ratios a joint needs, per thousand (0: 500); 0..1000 */
    uint32_t flags;               /* ORB_TRAJ_NEED_PARALLAX */
    uint32_t reserved[4];         /* must be 0 */
} OrbTrajectoryParams;            /* 32 bytes */

#define ORB_TRAJ_NEED_PARALLAX 1u /* only points with ORB_POINT_PARALLAX in both pairs give a ratio */

#define ORB_TRAJ_CHAINED 0u        /* the joint before the frame holds: the pose continues its segment */
#define ORB_TRAJ_START 1u          /* the pair before the frame is OK, the one before that is not (or there is none) */
#define ORB_TRAJ_RESTART_FEW 2u    /* both pairs are OK, the joint has fewer than min_shared ratios */
#define ORB_TRAJ_RESTART_SPREAD 3u /* both pairs are OK, too few of the joint's ratios agree with their median */
#define ORB_TRAJ_LOST 4u           /* the pair before the frame is not OK: identity, the frame is its own origin */
#define ORB_TRAJ_ORIGIN 5u         /* frame 0 */

typedef struct {
    float r[9];             /* row-major R, X_f = R X_origin + t */
    float t[3];             /* in units of the baseline of the pair (origin, origin + 1) */
    float scale;            /* the baseline of the pair (f-1, f) in that unit (START, RESTART_*: 1; LOST, ORIGIN: 0) */
    float step;             /* g of the joint before the frame (CHAINED, RESTART_SPREAD), else 0 */
    uint32_t origin;        /* the frame whose camera frame this pose starts from */
    uint32_t shared;        /* ratios of the joint before the frame (0 where none was evaluated) */
    uint32_t consistent;    /* of them: within scale_tolerance of the median */
    uint32_t status;        /* ORB_TRAJ_* */
    uint32_t reserved[2];   /* 0 */
} OrbFramePose;             /* 80 bytes */

/* Poses of the frames 0 .. n_frames - 1 of the last batch and the map points of its pairs.  params NULL: the defaults.
 * ORB_EINVAL for a NULL program, n_frames not in 2 .. min(4096, the last orb_pose_consecutive's pairs + 1), scale_tolerance not
 * finite or < 0, consistent_permille > 1000, an unknown flag, a reserved word that is not 0, or a program with max_features above
 * 2^23; ORB_ESTATE unless the last orb_match_consecutive and the last orb_pose_consecutive are both of the current batch and
 * output set.  Asynchronous on `stream` (NULL: as orb_match_guided chooses; the call does not change it), ordered behind the
 * matcher's and the pose stage's last calls and the last call of its own when they ran on another stream;
 * orb_match_consecutive and orb_pose_consecutive wait for such a call on another stream before they overwrite what it reads.
 * Result buffers of its own (allocated by the first call): no other stage's results are ever written. */
int orb_trajectory_consecutive(OrbProgram *p, uint32_t n_frames, const OrbTrajectoryParams *params, void *stream);
/* Copy the record of frame `frame` of the last orb_trajectory_consecutive call (pose may be NULL) and up to n map points of the
 * pair (frame, frame + 1) -- indexed as orb_pose_read's, in the frame and unit of the origin of frame + 1; zeros for every slot
 * that is not a good point, for a pair whose next frame is LOST and for the last frame -- to the host (synchronises); ORB_ESTATE
 * before any call, ORB_EINVAL for a frame outside the call's frames or points NULL with n > 0. */
int orb_trajectory_read(OrbProgram *p, uint32_t frame, OrbFramePose *pose, OrbPoint *points, size_t n);

/* ---- absolute pose from the previous pair's map points: PnP RANSAC (NOT in the reference; definition LO-1..LO-7 in DESIGN.md
 * section 21) ----
 * Pair f - 1 of the last orb_pose_consecutive triangulated landmarks from cameras f - 1 and f.  The matcher's records carry each
 * of them on: slot i of frame f - 1 matched keypoint j of frame f, and j matched keypoint k of frame f + 1 (that second hop under
 * max_distance and ratio).  A GOOD point X of pair f - 1, moved into camera f's frame by that pair's pose (Y = R X + t), and the
 * level-0 position of k are a 3D-2D correspondence.  They give the pose of camera f + 1 relative to camera f with a metric
 * translation, in units of pair f - 1's baseline, without pair f's fundamental matrix: a RANSAC over six-point DLT samples (the
 * first 11 of the 12 equations, solved by complete pivoting; sign from det, scale from the Frobenius norm, three polar steps),
 * scored by the reprojection error in frame f + 1, then four Gauss-Newton steps on the winner's inliers, kept when they hold at
 * least 15/16 of the winner's count.  So a pair with little or no translation, whose two-view pose is LOW_PARALLAX or AMBIGUOUS,
 * still gets a pose while the map of the pair before is in view.  Binary32 arithmetic in a fixed order, no fused operations: a
 * CPU restatement gives the same bits.  Nothing is fed back into orb_trajectory_consecutive; orb_bridge_consecutive below runs the
 * same RANSAC on the landmarks of orb_landmarks_consecutive to carry the trajectory across LOST frames. */
typedef struct {            /* zero-initialised is NOT valid: fx, fy must be > 0 */
    float fx, fy, cx, cy;   /* the intrinsics given to orb_pose_consecutive */
    float max_reproj_px;    /* frame f+1 reprojection error an inlier may have (0: 2.0); finite, >= 0 */
    uint32_t hypotheses;    /* minimal samples per pair, 1..4096 (0: 512) */
    uint32_t max_distance;  /* second hop: a match is a candidate iff distance <= this (0: 64); 0..256 */
    float ratio;            /* ... and distance < ratio * second (0: 0.8); finite, >= 0 */
    uint32_t seed;          /* of the sampling; the same seed gives the same result */
    uint32_t reserved[7];   /* must be 0 (ORB_EINVAL otherwise) */
} OrbLocalizeParams;        /* 64 bytes */

#define ORB_LOCALIZE_OK 0u         /* the refit was kept */
#define ORB_LOCALIZE_NOMAP 1u      /* pair 0, or the pose of pair f - 1 is not ORB_POSE_OK: all 0 */
#define ORB_LOCALIZE_FEW 2u        /* fewer than 6 correspondences: all 0 */
#define ORB_LOCALIZE_DEGENERATE 3u /* no valid hypothesis (coplanar, collinear or repeated points): all 0 */
#define ORB_LOCALIZE_MINIMAL 4u    /* the refit failed or lost more than 1/16 of the inliers: the winning six-point model */

typedef struct {
    float r[9];             /* row-major R, X(f+1) = R X(f) + t */
    float t[3];             /* in units of the baseline of pair f - 1 */
    float step;             /* |t|: the baseline of pair f over that of pair f - 1 (compare OrbFramePose.step) */
    uint32_t candidates;    /* 3D-2D correspondences */
    uint32_t inliers;       /* of them: within max_reproj_px under the model written */
    uint32_t hypothesis;    /* the winning sample */
    uint32_t status;        /* ORB_LOCALIZE_* */
    uint32_t reserved[3];   /* 0 */
} OrbFrameFix;              /* 80 bytes */

/* Fixes of the pairs (f, f+1), f in [0, n_frames - 1), of the last batch (pair 0 is NOMAP).  ORB_EINVAL for a NULL program or
 * params, fx or fy not finite or not > 0, cx or cy not finite, another parameter out of range, a reserved word that is not 0, or
 * n_frames not in 3 .. the last orb_pose_consecutive's pairs + 1; ORB_ESTATE unless the last orb_match_consecutive and the last
 * orb_pose_consecutive are both of the current batch and output set.  Asynchronous on `stream` (NULL: as orb_match_guided
 * chooses; the call does not change it), ordered behind the matcher's and the pose stage's last calls and the last call of its
 * own when they ran on another stream; orb_match_consecutive and orb_pose_consecutive wait for such a call on another stream
 * before they overwrite what it reads.  Result buffers of its own (allocated by the first call): no other stage's results are
 * ever written. */
int orb_localize_consecutive(OrbProgram *p, uint32_t n_frames, const OrbLocalizeParams *params, void *stream);
/* Copy the record of pair `pair` of the last orb_localize_consecutive call (fix may be NULL) and up to n inlier bytes -- byte i is
 * 1 iff slot i of frame pair - 1 (indexed as orb_match_read) gave a correspondence that is an inlier of the model written -- to the
 * host (synchronises); ORB_ESTATE before any call, ORB_EINVAL for a pair outside its pairs or inliers NULL with n > 0. */
int orb_localize_read(OrbProgram *p, uint32_t pair, OrbFrameFix *fix, uint8_t *inliers, size_t n);

/* ---- one multi-view map point per landmark (NOT in the reference; definition LM-1..LM-6 in DESIGN.md section 22) ----
 * The map of orb_trajectory_consecutive holds a landmark once per pair that triangulated it, each copy with the error of one short
 * baseline.  Here the matcher's records chain the GOOD points of consecutive pairs of one segment: slot i of pair p continues into
 * slot j = matches[p][i].index of pair p + 1 when that point is GOOD too and frame p + 2 is CHAINED.  A GOOD slot that no GOOD slot
 * of the pair before continues into is a start, and each start is one landmark: the point nearest to the rays of all its views
 * (midpoint method) under the frame poses of the last orb_trajectory_consecutive, in the frame and unit of its segment's origin,
 * then checked by reprojection into every view.  Binary32 arithmetic in a fixed order, no fused operations, no square root: a CPU
 * restatement gives the same bits.  Nothing is fed back into another stage; orb_bridge_consecutive below reads the landmarks. */
typedef struct {            /* zero-initialised is NOT valid: fx, fy must be > 0 */
    float fx, fy, cx, cy;   /* the intrinsics given to orb_pose_consecutive */
    float max_reproj_px;    /* reprojection error a view may have (0: 2.0); finite, >= 0 */
    uint32_t min_views;     /* views a GOOD landmark needs (0: 2) */
    uint32_t reserved[2];   /* must be 0 (ORB_EINVAL otherwise) */
} OrbLandmarkParams;        /* 32 bytes */

typedef struct {
    float x, y, z;          /* in the frame and unit of frame `origin`; 0 when the solve failed */
    uint32_t flags;         /* ORB_POINT_GOOD: solved, views >= min_views and every view an inlier; ORB_POINT_PARALLAX: GOOD and a point of the chain has it */
    uint16_t views;         /* 0: this slot starts no landmark (then the whole record is 0) */
    uint16_t inliers;       /* views within max_reproj_px of the point's reprojection */
    uint32_t origin;        /* the segment's origin frame (OrbFramePose.origin) */
    uint32_t tail_index;    /* keypoint slot of the last view, in frame pair + views - 1 */
    uint32_t reserved[1];   /* 0 */
} OrbLandmark;              /* 32 bytes */

typedef struct {
    uint32_t landmarks;     /* starts of this pair */
    uint32_t good;          /* of them GOOD */
    uint32_t longest;       /* the largest `views` */
    uint32_t origin;        /* the pair's segment, 0xffffffff when frame pair + 1 is LOST (no landmarks) */
} OrbLandmarkRow;           /* 16 bytes */

/* Landmarks of the pairs (f, f+1), f in [0, n_frames - 1), of the last batch: the record of a landmark is at the pair and slot of its
 * first view.  ORB_EINVAL for a NULL program or params, fx or fy not finite or not > 0, cx or cy not finite, max_reproj_px not
 * finite or < 0, a reserved word that is not 0, or n_frames not in 2 .. the last orb_trajectory_consecutive's frames; ORB_ESTATE
 * unless the last orb_match_consecutive, orb_pose_consecutive and orb_trajectory_consecutive are all of the current batch and
 * output set.  Asynchronous on `stream` (NULL: as orb_match_guided chooses; the call does not change it), ordered behind those
 * three stages' last calls and the last call of its own when they ran on another stream; the three wait for such a call on another
 * stream before they overwrite what it reads.  Result buffers of its own (allocated by the first call): no other stage's results
 * are ever written. */
int orb_landmarks_consecutive(OrbProgram *p, uint32_t n_frames, const OrbLandmarkParams *params, void *stream);
/* Copy the row of pair `pair` of the last orb_landmarks_consecutive call (row may be NULL) and its first n landmark records (indexed
 * as orb_match_read) to the host (synchronises); ORB_ESTATE before any call, ORB_EINVAL for a pair outside its pairs or landmarks
 * NULL with n > 0. */
int orb_landmarks_read(OrbProgram *p, uint32_t pair, OrbLandmarkRow *row, OrbLandmark *landmarks, size_t n);

/* ---- a trajectory carried across LOST frames (NOT in the reference; definition BR-1..BR-7 in DESIGN.md section 23) ----
 * One pair with little translation ends a segment of orb_trajectory_consecutive: its frame is LOST and the frames behind it start
 * a new segment with a new origin and a new unit, although the landmarks built just before are still in view.  For every LOST
 * frame g, with T the last frame before it that is not LOST (its anchor), the GOOD landmarks of the last
 * orb_landmarks_consecutive whose last view is in frame T are followed through the matcher's records from their tail_index hop
 * by hop into frame g (every hop under max_distance and ratio).  Each, moved into camera T's frame, and the level-0 position of
 * its keypoint in frame g are a 3D-2D correspondence; orb_localize_consecutive's RANSAC and refit give camera g relative to
 * camera T in the unit of T's segment.  When frame g + 1 starts a segment, the new segment's points at those keypoints give the
 * ratio of the two units (lower median of depth ratios, accepted as a joint of the trajectory is).  The call writes, for every
 * frame of the batch, a pose in the frame and unit of the earliest origin the frame can be traced back to (its root).  A batch
 * without a LOST frame gives the trajectory's poses bit for bit.  Binary32 arithmetic in a fixed order, no fused operations: a
 * CPU restatement gives the same bits.  RESTART_FEW and RESTART_SPREAD frames are not joined. */
typedef struct {                  /* zero-initialised is NOT valid: fx, fy must be > 0 */
    float fx, fy, cx, cy;         /* the intrinsics given to orb_pose_consecutive */
    float max_reproj_px;          /* frame g reprojection error an inlier may have (0: 2.0); finite, >= 0 */
    uint32_t hypotheses;          /* minimal samples per LOST frame, 1..4096 (0: 512) */
    uint32_t max_distance;        /* a hop is followed iff distance <= this (0: 64); 0..256 */
    float ratio;                  /* ... and distance < ratio * second (0: 0.8); finite, >= 0 */
    uint32_t seed;                /* of the sampling; the same seed gives the same result */
    uint32_t max_hops;            /* a LOST frame further than this behind its anchor is not fixed (0: 4); 0..16 */
    uint32_t window;              /* landmark rows T - window .. T - 1 are searched (0: 32); 0..4095 */
    uint32_t min_shared;          /* depth ratios a join needs (0: 8) */
    float scale_tolerance;        /* a ratio is consistent within this, relative to the median (0: 0.1); finite, >= 0 */
    uint32_t consistent_permille; /* share of the ratios that must be consistent (0: 500); 0..1000 */
    uint32_t reserved[2];         /* must be 0 (ORB_EINVAL otherwise) */
} OrbBridgeParams;                /* 64 bytes */

#define ORB_BRIDGE_COPIED 0u  /* not LOST, in a segment whose origin is its own root: the trajectory's pose and scale, gain 1 */
#define ORB_BRIDGE_MOVED 1u   /* not LOST, in a segment joined to an earlier one: the trajectory's pose moved into the root's frame and unit */
#define ORB_BRIDGE_FIXED 2u   /* LOST, fixed against its anchor; the frames behind it are a map of their own (gain 0) */
#define ORB_BRIDGE_JOINED 3u  /* LOST, fixed, and the segment that starts behind it measured against the old one */
#define ORB_BRIDGE_UNFIXED 4u /* LOST and not fixed: the trajectory's record (identity), root = the frame itself, gain 0 */

typedef struct {
    float r[9];             /* row-major R, X_f = R X_root + t */
    float t[3];             /* in units of the root segment */
    float scale;            /* COPIED, MOVED: the trajectory's scale in root units; FIXED, JOINED: |t| of the fix in root units; UNFIXED: 0 */
    float gain;             /* root units per unit of the segment this frame belongs to (COPIED: 1) or starts (JOINED); else 0 */
    uint32_t root;          /* the origin frame the pose refers to */
    uint32_t anchor;        /* LOST frames: the last frame before that is not LOST; else 0 */
    uint32_t candidates;    /* LOST frames: 3D-2D correspondences (at most the capacity) */
    uint32_t inliers;       /* of them: within max_reproj_px under the fix */
    uint32_t hypothesis;    /* the winning sample */
    uint32_t shared;        /* depth ratios of the join, when one was evaluated */
    uint32_t consistent;    /* of them within scale_tolerance of their median */
    uint32_t fix;           /* ORB_LOCALIZE_*; ORB_LOCALIZE_NOMAP for frames that are not LOST */
    uint32_t status;        /* ORB_BRIDGE_* */
    uint32_t reserved[1];   /* 0 */
} OrbBridgePose;            /* 96 bytes */

/* Bridged poses of frames 0 .. n_frames - 1 of the last batch.  ORB_EINVAL for a NULL program or params, fx or fy not finite or
 * not > 0, cx or cy not finite, another parameter out of range, a reserved word that is not 0, or n_frames not in 2 .. the last
 * orb_landmarks_consecutive's frames; ORB_ESTATE unless the last orb_match_consecutive, orb_pose_consecutive,
 * orb_trajectory_consecutive and orb_landmarks_consecutive are all of the current batch and output set.  Asynchronous on `stream`
 * (NULL: as orb_match_guided chooses; the call does not change it), ordered behind those four stages' last calls and the last
 * call of its own when they ran on another stream; the four wait for such a call on another stream before they overwrite what
 * it reads.  Result buffers of its own (allocated by the first call): no other stage's results are ever written. */
int orb_bridge_consecutive(OrbProgram *p, uint32_t n_frames, const OrbBridgeParams *params, void *stream);
/* Copy the record of frame `frame` of the last orb_bridge_consecutive call (pose may be NULL) and up to n inlier bytes -- byte k is
 * 1 iff keypoint k of a LOST frame (indexed as orb_match_read) ends a correspondence that is an inlier of the fix written; all 0
 * for every other frame -- to the host (synchronises); ORB_ESTATE before any call, ORB_EINVAL for a frame outside its frames or
 * inliers NULL with n > 0. */
int orb_bridge_read(OrbProgram *p, uint32_t frame, OrbBridgePose *pose, uint8_t *inliers, size_t n);

/* ---- poses and landmarks refined by reprojection (NOT in the reference; definition BA-1..BA-7 in DESIGN.md section 24) ----
 * Every OrbFramePose is a product of two-view poses, and orb_landmarks_consecutive places its points under those poses without
 * moving one.  Here the two are alternated (resection-intersection: bundle adjustment by block coordinate descent).  A frame is
 * free iff its trajectory status is CHAINED; every other frame is held, so the first two cameras of a segment never move and
 * the result stays in the trajectory's frame and unit.  The GOOD landmarks whose views all lie inside the call's frames take
 * part; keypoint k of a free frame g belongs to the landmark of g's segment with the smallest pair * capacity + slot among
 * those that see it.  A round is one Gauss-Newton step of orb_localize_consecutive's refit on every free frame over the
 * keypoints that have an owner (all from the points of the round before), then orb_landmarks_consecutive's point nearest to all
 * rays for every landmark under the new poses; an unsolved landmark keeps its point.  No step is damped or rejected: the
 * record reports the cost (the sum of squared pixel residuals over the frame's owned keypoints) before the first step and
 * after the last.  Binary32 arithmetic in a fixed order, no fused operations: a CPU restatement gives the same bits.  Nothing
 * is fed back into another stage. */
typedef struct {            /* zero-initialised is NOT valid: fx, fy must be > 0 */
    float fx, fy, cx, cy;   /* the intrinsics given to orb_pose_consecutive */
    float max_reproj_px;    /* closing check: reprojection error a view may have (0: 2.0); finite, >= 0 */
    uint32_t rounds;        /* alternations, 1..16 (0: 4) */
    uint32_t reserved[2];   /* must be 0 (ORB_EINVAL otherwise) */
} OrbAdjustParams;          /* 32 bytes */

#define ORB_ADJUST_HELD 0u    /* not CHAINED: r and t are the trajectory's bits, the other words 0 */
#define ORB_ADJUST_REFINED 1u /* every round's step was taken */
#define ORB_ADJUST_FEW 2u     /* fewer than 6 owned keypoints: the trajectory's pose, observations, costs 0 */
#define ORB_ADJUST_FAILED 3u  /* a step failed: the last pose kept and both costs; or the trajectory's record is not finite: all 0 but observations */

typedef struct {
    float r[9];             /* row-major R, X_f = R X_origin + t, as OrbFramePose */
    float t[3];
    float cost_before;      /* sum of squared pixel residuals over the owned keypoints, under the trajectory's pose and the landmark stage's points */
    float cost_after;       /* the same under the poses and points written (a cost that is not finite reads FLT_MAX) */
    uint32_t observations;  /* keypoints of this frame that have an owner */
    uint32_t status;        /* ORB_ADJUST_* */
} OrbAdjustedPose;          /* 64 bytes */

/* Refined poses of frames 0 .. n_frames - 1 of the last batch and refined landmarks of its pairs.  ORB_EINVAL for a NULL program
 * or params, fx or fy not finite or not > 0, cx or cy not finite, max_reproj_px not finite or < 0, rounds above 16, a reserved
 * word that is not 0, n_frames not in 2 .. the last orb_landmarks_consecutive's frames, or n_frames * max_features >= 2^32 - 1;
 * ORB_ESTATE unless the last orb_match_consecutive, orb_trajectory_consecutive and orb_landmarks_consecutive are all of the
 * current batch and output set.  Asynchronous on `stream` (NULL: as orb_match_guided chooses; the call does not change it),
 * ordered behind those three stages' last calls and the last call of its own when they ran on another stream; the three wait for
 * such a call on another stream before they overwrite what it reads.  Result buffers of its own (allocated by the first call):
 * no other stage's results are ever written. */
int orb_adjust_consecutive(OrbProgram *p, uint32_t n_frames, const OrbAdjustParams *params, void *stream);
/* Copy the record of frame `frame` of the last orb_adjust_consecutive call (pose may be NULL) and the first n landmark records of
 * the pair (frame, frame + 1) -- indexed and laid out as orb_landmarks_read's: a landmark that took part with its refined point,
 * inliers recounted and GOOD iff every view is one, every other record as the landmark stage wrote it; zeros for the last
 * frame -- to the host (synchronises); ORB_ESTATE before any call, ORB_EINVAL for a frame outside its frames or landmarks NULL
 * with n > 0. */
int orb_adjust_read(OrbProgram *p, uint32_t frame, OrbAdjustedPose *pose, OrbLandmark *landmarks, size_t n);

/* ---- feature tracks and keyframes (NOT in the reference; definition TK-1..TK-5 in DESIGN.md section 15) ----
 * Over the pairs (f, f+1), f in [0, n_frames - 1), of the last batch: query i of frame f links to target j of frame f+1 by the
 * source's record (VERIFIED: the matcher's record where the last verification's inlier byte is 1; GUIDED / MATCHED: the last
 * orb_match_guided's / orb_match_consecutive's record when it passes the verifier's candidate test with max_distance and ratio).
 * Of the links to one target only the one with the smallest key (distance << 23) | i survives, giving prev / next; head_* and
 * tail_frame follow them to the ends of the chain.  Keyframes: frame 0, then every frame f at least min_gap after the current
 * keyframe k with max_gap reached (max_gap != 0), no track left from k to f, 1000 shared < keep_permille links_out(k), or
 * shared < min_shared, where shared = the tracks that run from k to f. */
typedef struct {              /* zero-initialised = the defaults */
    uint32_t source;          /* ORB_TRACK_VERIFIED (0), ORB_TRACK_GUIDED (1), ORB_TRACK_MATCHED (2) */
    uint32_t max_distance;    /* GUIDED / MATCHED: 0..256 (0: 64); must be 0 with VERIFIED */
    float ratio;              /* GUIDED / MATCHED: finite, >= 0 (0: 0.8); must be 0 with VERIFIED */
    uint32_t min_gap;         /* frames between keyframes, at least (0: 1) */
    uint32_t max_gap;         /* 0: no bound; else >= min_gap */
    uint32_t keep_permille;   /* 1..1000 (0: 900) */
    uint32_t min_shared;      /* 0: no absolute floor */
    uint32_t reserved;        /* must be 0 (ORB_EINVAL otherwise) */
} OrbTrackParams;             /* 32 bytes */

#define ORB_TRACK_VERIFIED 0u     /* the last orb_verify_consecutive's inliers (and the matcher's records it verified) */
#define ORB_TRACK_GUIDED 1u       /* the last orb_match_guided's records */
#define ORB_TRACK_MATCHED 2u      /* the last orb_match_consecutive's records */

typedef struct {
    uint32_t prev;            /* the keypoint of frame f-1 linked to this one, ORB_MATCH_NONE if none */
    uint32_t next;            /* the keypoint of frame f+1 this one links to, ORB_MATCH_NONE if none */
    uint32_t head_index;      /* first keypoint of the chain (this one if prev is NONE) */
    uint16_t head_frame;      /* its frame */
    uint16_t tail_frame;      /* the frame of the chain's last keypoint */
} OrbTrack;                   /* 16 bytes; entries past a frame's stored keypoints: NONE, NONE, NONE, 0xffff, 0xffff */

typedef struct {
    uint32_t keypoints;       /* min(count, max_features) */
    uint32_t links_in;        /* keypoints with prev != NONE */
    uint32_t links_out;       /* keypoints with next != NONE */
    uint32_t keyframe;        /* 1 for a keyframe */
    uint32_t ref_keyframe;    /* the keyframe the frame was tested against (0 for frame 0) */
    uint32_t shared;          /* tracks running from ref_keyframe to this frame */
    uint32_t reserved[2];     /* 0 */
} OrbTrackFrame;              /* 32 bytes */

/* Chains the pairs of the last batch into tracks and picks keyframes (params NULL: the defaults).  ORB_EINVAL when n_frames is not
 * 2..min(4096, frames of the last batch) or exceeds the source's pairs + 1, max_features > 2^23, or a parameter is out of range;
 * ORB_ESTATE when the source's last call was not of the current batch and output set (VERIFIED: also when the matcher ran on
 * another batch or output set than the verification).  Asynchronous on `stream` (NULL: the stream of the program's last batched
 * call; the track call does not change it), ordered behind the source's last call and the last track call when they ran on another
 * stream; orb_match_consecutive, orb_verify_consecutive and orb_match_guided wait for a track call on another stream.  Result
 * buffers of its own (allocated by the first call): the matcher's, the verifier's and the guided call's are never written.
 * Environment: TINYORB_TRACK_GLOBAL_KEYS=1 (read once per program) keeps the link keys in global memory, which changes no
 * result. */
int orb_track_consecutive(OrbProgram *p, uint32_t n_frames, const OrbTrackParams *params, void *stream);
/* Copy up to n OrbTrack entries of frame `frame` of the last orb_track_consecutive call to the host (synchronises); ORB_ESTATE
 * before any call, ORB_EINVAL for a frame outside its frames. */
int orb_track_read(OrbProgram *p, uint32_t frame, OrbTrack *dst, size_t n);
/* Copy the first min(n, n_frames) OrbTrackFrame records of the last orb_track_consecutive call (synchronises); ORB_ESTATE before
 * any call. */
int orb_track_frames(OrbProgram *p, OrbTrackFrame *dst, size_t n);

/* ---- loop candidates by descriptor-signature overlap (NOT in the reference; definition PL-1..PL-6 in DESIGN.md section 25) ----
 * Place recognition: which earlier frames, of this batch or of a database kept from earlier batches, show what frame f shows.
 * A descriptor is 16 little-endian 16-bit halves; table t < tables gives a record the key (half t) & (2^bits - 1).  A frame's
 * signature is `tables` bitmaps of 2^bits bits -- bit `key` of bitmap t (bit key & 7 of byte t * 2^bits / 8 + (key >> 3)) is set
 * iff one of the frame's stored records, the first min(count, max_features), has that key in table t --, sig_bytes =
 * tables * 2^bits / 8 bytes in all, and score(a, b) the number of bits two signatures share.  Ids: database entry e is e, batch
 * frame g is n_db + g.  For query f every database entry is eligible, and batch frame g iff g + min_gap <= f (with
 * ORB_PLACE_KEYFRAMES: and g is a keyframe of the last orb_track_consecutive).  An eligible id is a candidate iff score >=
 * max(min_score, 1) and 1000 score >= min_permille bits_set(f); the row lists the min(candidates, top) candidates with the
 * greatest (score << 32) | (0xffffffff - id), greatest first, so equal scores go to the smaller id.  Integer arithmetic only: a
 * CPU restatement gives the same bytes.  The descriptors of the literal mode change under translation (README, the verifier's
 * paragraph) and recognise nothing here: like the verifier, the stage is meant for ORB_FLAG_INTENDED programs.  Nothing is fed
 * back into another stage. */
typedef struct {            /* zero-initialised = the defaults */
    uint32_t bits;          /* key width, 8..16 (0: 16) */
    uint32_t tables;        /* 1..16 (0: 8); tables << bits must not exceed 8 * ORB_PLACE_SIG_BYTES_MAX */
    uint32_t min_gap;       /* >= 1 (0: 32) */
    uint32_t top;           /* 1..8 (0: 4) */
    uint32_t min_score;     /* 0: 1 */
    uint32_t min_permille;  /* 0..1000 */
    uint32_t flags;         /* ORB_PLACE_KEYFRAMES (1) or 0 */
    uint32_t reserved;      /* must be 0 */
} OrbPlaceParams;           /* 32 bytes */

#define ORB_PLACE_KEYFRAMES 1u           /* only keyframes of the last orb_track_consecutive are eligible batch frames */
#define ORB_PLACE_DB 0x80000000u         /* OrbPlaceCandidate::frame of database entry e is ORB_PLACE_DB | e */
#define ORB_PLACE_SIG_BYTES_MAX 65536u
#define ORB_PLACE_DB_MAX 1024u

typedef struct { uint32_t frame; uint32_t score; } OrbPlaceCandidate;   /* 8 bytes */

typedef struct {
    uint32_t keypoints;     /* min(count, max_features) */
    uint32_t bits_set;      /* set bits of the frame's signature */
    uint32_t eligible;      /* eligible ids, database entries included */
    uint32_t candidates;    /* of them candidates */
    uint32_t n;             /* min(candidates, top) */
    uint32_t reserved[3];   /* 0 */
    OrbPlaceCandidate best[8];  /* the first n: a batch frame g as g, a database entry e as ORB_PLACE_DB | e; the rest ORB_MATCH_NONE, score 0 */
} OrbPlaceRow;              /* 96 bytes */

/* Signatures and candidate rows of frames 0 .. n_frames - 1 of the last batch and the current output set (params NULL: the
 * defaults).  db_host: n_db signatures of sig_bytes each, row after row, made by earlier calls with the same bits and tables
 * (orb_place_signature); NULL with n_db 0.  ORB_EINVAL for a NULL program, a parameter out of range, a reserved word that is
 * not 0, unknown flags, n_db above ORB_PLACE_DB_MAX, exactly one of db_host and n_db zero, or n_frames not in 1 .. the frames of
 * the last batch; ORB_ESTATE when the program holds no batch, and with ORB_PLACE_KEYFRAMES unless the last
 * orb_track_consecutive is of the current batch and output set and tracked at least n_frames frames.  Asynchronous on `stream`
 * (NULL: as orb_match_guided chooses; the call does not change it), ordered behind the last call of its own and, with
 * ORB_PLACE_KEYFRAMES, the last orb_track_consecutive when they ran on another stream; orb_track_consecutive waits for a place
 * call on another stream before it overwrites its frame records.  The database is copied to the device on the call's stream
 * and the call waits on the host for that copy alone: db_host may be freed or overwritten as soon as it returns.  Result
 * buffers of its own (allocated by the first call: max_batch + ORB_PLACE_DB_MAX signatures of ORB_PLACE_SIG_BYTES_MAX and a
 * score matrix): no other stage's results are ever written. */
int orb_place_frames(OrbProgram *p, uint32_t n_frames, const OrbPlaceParams *params, const uint8_t *db_host, uint32_t n_db, void *stream);
/* Copy up to n OrbPlaceRow records, frames `frame`, frame + 1, ... of the last orb_place_frames call clipped to its frames, to
 * the host (synchronises); ORB_ESTATE before any call, ORB_EINVAL for a frame outside its frames or rows NULL with n > 0. */
int orb_place_read(OrbProgram *p, uint32_t frame, OrbPlaceRow *rows, size_t n);
/* Copy the first min(n_bytes, sig_bytes) bytes of the signature of frame `frame` as the last orb_place_frames call built it
 * (synchronises): what a caller keeps, for a keyframe say, and hands back as a row of db_host in a later batch.  ORB_ESTATE
 * before any call, ORB_EINVAL for a frame outside its frames or dst NULL with n_bytes > 0. */
int orb_place_signature(OrbProgram *p, uint32_t frame, uint8_t *dst, size_t n_bytes);

/* ---- matching and verification of caller-listed frame pairs (NOT in the reference; definition MP-1..MP-5 in DESIGN.md section 27) ----
 * orb_match_consecutive and the two verifiers work on the pairs (f, f + 1).  A loop candidate of orb_place_frames is a pair of
 * frames far apart: these two calls match and verify any pairs of frames of the last batch that the caller lists.  Entry i of
 * the list is pair i: frame `query` gives the queries, frame `target` the candidates.  Duplicates, backward pairs
 * (query > target) and consecutive pairs are allowed; 1 <= n_pairs <= ORB_PAIRS_PER_FRAME * max_batch, query and target below
 * the last batch's frame count, query != target.  Nothing is fed back into another stage, and no other stage's results are
 * written. */
typedef struct { uint32_t query, target; } OrbFramePair;            /* 8 bytes */
#define ORB_PAIRS_PER_FRAME 4u           /* a call takes at most this many pairs per frame of max_batch (orb_place_frames' default `top`) */
#define ORB_PAIRS_HOMOGRAPHY 0u          /* orb_verify_pairs: GV-1..GV-7, as orb_verify_consecutive */
#define ORB_PAIRS_EPIPOLAR 1u            /* orb_verify_pairs: EP-1..EP-6, as orb_verify_epipolar */
/* Row i of the result holds orb_match_consecutive's record for every stored keypoint of frame pairs_host[i].query against the
 * stored keypoints of frame pairs_host[i].target (best index with ties to the smallest, distance, runner-up distance;
 * ORB_MATCH_NONE / 0xffff without candidates): for a listed pair (f, f + 1) the row equals orb_match_read(f) byte for byte.
 * ORB_EINVAL for a NULL program or list, n_pairs outside 1 .. ORB_PAIRS_PER_FRAME * max_batch, or an entry that breaks the rules
 * above (the message names the first one); ORB_ESTATE when the program holds no batch.  Asynchronous on `stream` (NULL: as
 * orb_match_guided chooses; the call does not change it), ordered behind its own last call and a running orb_verify_pairs on
 * another stream.  The list is copied through a pinned buffer of the stage: pairs_host is the caller's again when the call
 * returns.  Buffers of its own, allocated by the first call: the list, ORB_PAIRS_PER_FRAME * max_batch rows of max_features
 * records, and -- on the matrix cores: max_features <= 16383, TINYORB_MATCH_VALU unset, memory at hand -- 128 bytes per record
 * of a batch for the descriptors as fp4, apart from orb_match_consecutive's (TINYORB_MATCH_I8 has no form here and selects
 * fp4). */
int orb_match_pairs(OrbProgram *p, const OrbFramePair *pairs_host, uint32_t n_pairs, void *stream);
/* Copy up to n records of row `pair` of the last orb_match_pairs call, the queries of that entry's `query` frame (synchronises);
 * ORB_ESTATE before any call, ORB_EINVAL for a pair at or past its n_pairs or dst NULL with n > 0; n is clipped to
 * max_features. */
int orb_match_pairs_read(OrbProgram *p, uint32_t pair, OrbMatch *dst, size_t n);
/* Verifies pairs 0 .. n_pairs - 1 of the last orb_match_pairs call on its rows and the two frames' keypoints: `model`
 * ORB_PAIRS_HOMOGRAPHY gives pair i exactly what orb_verify_consecutive gives a consecutive pair, ORB_PAIRS_EPIPOLAR what
 * orb_verify_epipolar gives, with the list index i wherever those definitions say "pair" (the draw stream's seed, the record's
 * place) -- never a frame.  params NULL: the defaults.  The record's h maps (relates) frame `query` to frame `target`; one
 * inlier byte per query of frame `query`.  ORB_ESTATE unless the last orb_match_pairs is of the current batch and output set;
 * ORB_EINVAL for n_pairs outside 1 .. the pairs it matched, an unknown model or a parameter out of OrbVerifyParams' ranges.
 * Asynchronous on `stream` (NULL: as orb_match_guided chooses; the call does not change it), ordered behind the last
 * orb_match_pairs and its own last call on another stream; an orb_match_pairs on another stream waits for it.  Result buffers
 * of its own (allocated by the first call), shared by the two models: a call overwrites the results of the call before. */
int orb_verify_pairs(OrbProgram *p, uint32_t n_pairs, uint32_t model, const OrbVerifyParams *params, void *stream);
/* As orb_verify_read, for pair `pair` of the last orb_verify_pairs call (ORB_ESTATE before the first). */
int orb_verify_pairs_read(OrbProgram *p, uint32_t pair, OrbPairModel *model, uint8_t *inlier, size_t n);

/* ---- a listed query's pose from its target's landmarks (NOT in the reference; definition LC-1..LC-7 in DESIGN.md section 28) ----
 * A pair confirmed by orb_verify_pairs says that two frames show the same place, not where the query camera is in the map.  Here
 * row i of the last orb_match_pairs sends every keypoint of entry i's `query` frame q to a keypoint of its `target` frame T; that
 * keypoint is a view of a GOOD landmark of the last orb_landmarks_consecutive (when several see it, the one of T's segment with
 * the smallest pair * capacity + slot), and the landmark is a 3D point in the frame and unit of T's segment.  Each such landmark,
 * moved into camera T's frame, and the level-0 position of the query keypoint are a 3D-2D correspondence;
 * orb_localize_consecutive's RANSAC and refit (with the list index in the draw stream's seed) give camera q relative to camera T
 * in the unit of T's segment -- X_q = r X_T + t -- and, composed with T's pose, camera q in that segment's frame (pose_r,
 * pose_t).  T must lie inside the landmarks call's frames; q may be any frame of the batch.  orb_verify_pairs is not read: the
 * RANSAC is the outlier filter.  Binary32 arithmetic in a fixed order, no fused operations: a CPU restatement gives the same
 * bits.  Nothing is fed back into another stage. */
typedef struct {            /* zero-initialised is NOT valid: fx, fy must be > 0 */
    float fx, fy, cx, cy;   /* the intrinsics given to orb_pose_consecutive */
    float max_reproj_px;    /* frame q reprojection error an inlier may have (0: 2.0); finite, >= 0 */
    uint32_t hypotheses;    /* minimal samples per list entry, 1..4096 (0: 512) */
    uint32_t max_distance;  /* a record of the row is followed iff distance <= this (0: 64); 0..256 */
    float ratio;            /* ... and distance < ratio * second (0: 0.8); finite, >= 0 */
    uint32_t seed;          /* of the sampling; the same seed gives the same result */
    uint32_t reserved[7];   /* must be 0 (ORB_EINVAL otherwise) */
} OrbLoopParams;            /* 64 bytes */

typedef struct {
    float r[9];             /* row-major R, X_q = R X_T + t */
    float t[3];             /* in units of the segment of frame T */
    float step;             /* |t| */
    float pose_r[9];        /* row-major R, X_q = R X_origin + t: camera q in the frame of `origin`; 0 when an entry is not finite */
    float pose_t[3];        /* in units of that segment */
    uint32_t origin;        /* the origin of frame T in the last orb_trajectory_consecutive */
    uint32_t query_origin;  /* the origin of frame q there, 0xffffffff for a q above that call's frames: pose_* compares with q's own
                             * OrbFramePose exactly when the two origins are equal */
    uint32_t candidates;    /* 3D-2D correspondences */
    uint32_t inliers;       /* of them: within max_reproj_px under the model written */
    uint32_t hypothesis;    /* the winning sample */
    uint32_t status;        /* ORB_LOCALIZE_*; NOMAP: T outside the landmarks call's frames, or its pose there not finite.  NOMAP, FEW
                             * and DEGENERATE: every other word 0 */
    uint32_t reserved[1];   /* 0 */
} OrbLoopFix;               /* 128 bytes */

/* Fixes of entries 0 .. n_pairs - 1 of the last orb_match_pairs call.  ORB_EINVAL for a NULL program or params, fx or fy not
 * finite or not > 0, cx or cy not finite, another parameter out of range or a reserved word that is not 0; then ORB_ESTATE unless
 * the last orb_match_pairs, orb_match_consecutive, orb_trajectory_consecutive and orb_landmarks_consecutive are all of the current
 * batch and output set; then ORB_EINVAL for n_pairs outside 1 .. the pairs the last orb_match_pairs matched, or when the landmarks
 * call's frames * max_features reach 2^32 - 1.  Asynchronous on `stream` (NULL: as orb_match_guided chooses; the call does not
 * change it), ordered behind those four stages' last calls and the last call of its own when they ran on another stream; the four
 * wait for such a call on another stream before they overwrite what it reads.  Result buffers of its own (allocated by the first
 * call: about 40 bytes per keypoint slot of ORB_PAIRS_PER_FRAME * max_batch rows and 32 KiB of keys per row): no other stage's
 * results are ever written. */
int orb_loop_pairs(OrbProgram *p, uint32_t n_pairs, const OrbLoopParams *params, void *stream);
/* Copy the record of entry `pair` of the last orb_loop_pairs call (fix may be NULL) and up to n inlier bytes -- byte a is 1 iff
 * keypoint a of the entry's query frame (indexed as orb_match_pairs_read) gave a correspondence that is an inlier of the model
 * written -- to the host (synchronises); ORB_ESTATE before any call, ORB_EINVAL for a pair outside its pairs or inliers NULL with
 * n > 0. */
int orb_loop_pairs_read(OrbProgram *p, uint32_t pair, OrbLoopFix *fix, uint8_t *inliers, size_t n);
/* For tests: the device address of the OrbLoopFix records [ORB_PAIRS_PER_FRAME * max_batch] that orb_loop_pairs writes and
 * orb_loop_pairs_read and orb_graph_pairs read.  The caller orders its own writes.  ORB_ESTATE until a loop call has run. */
int orb_debug_loop_buffer(OrbProgram *p, void **fixes);

/* ---- pose-graph correction from the loop fixes (NOT in the reference; definition PG-1..PG-8 in DESIGN.md section 29) ----
 * The trajectory chains pair poses, so its error grows along a segment (a run of frames with one origin); an OrbLoopFix measures
 * camera q relative to camera T without passing through that chain.  orb_graph_pairs takes every segment of the last
 * orb_trajectory_consecutive as a graph of its own: the nodes are the segment's cameras, the chain edges the relative poses of
 * consecutive cameras as the trajectory holds them (weight 1), the loop edges the entries 0 .. n_pairs - 1 of the last
 * orb_loop_pairs that qualify (weight loop_weight, measurement r, t of the fix).  The cost of an edge (a -> b, R_z, t_z, w) is
 * w (rotation_weight |e_R|^2 + |e_t|^2) with e_R the vector part of the skew part of R_b R_a^T R_z^T and e_t = t_b - R_b R_a^T t_a -
 * t_z; `rounds` Gauss-Newton rounds, each solved by `cg_iterations` conjugate-gradient iterations preconditioned by the 6 x 6
 * diagonal blocks, move every camera of the segment but its origin; a round that does not lower the cost is undone and ends the
 * segment.  SE(3) only: the unit of a segment is carried by the edges' translations and is not corrected.  Binary32 arithmetic in
 * a fixed order, no fused operations: a CPU restatement gives the same bits.  Nothing is fed back into another stage, and no
 * other stage's results are written. */
#define ORB_GRAPH_USE_MINIMAL 1u        /* flags: a fix of status ORB_LOCALIZE_MINIMAL qualifies too */
#define ORB_GRAPH_HELD 0u               /* an origin, a LOST or ORIGIN frame, a frame outside every segment: the trajectory's r, t; other words 0 */
#define ORB_GRAPH_UNCHANGED 1u          /* the segment has no USED edge: the poses copied bit for bit */
#define ORB_GRAPH_REFINED 2u            /* every round lowered the segment's cost */
#define ORB_GRAPH_STALLED 3u            /* a round did not lower the cost: the poses of before that round */
#define ORB_GRAPH_FAILED 4u             /* a diagonal block could not be inverted: the poses of before that round */
#define ORB_GRAPH_INVALID 5u            /* a pose entry of a free camera of the segment is not finite: the poses copied bit for bit */
#define ORB_GRAPH_EDGE_USED 0u          /* the entry is a loop edge of segment `origin` */
#define ORB_GRAPH_EDGE_STATUS 1u        /* the fix is not OK (nor MINIMAL under ORB_GRAPH_USE_MINIMAL) */
#define ORB_GRAPH_EDGE_FEW 2u           /* inliers < min_inliers */
#define ORB_GRAPH_EDGE_RANGE 3u         /* q or T at or above the trajectory call's frames */
#define ORB_GRAPH_EDGE_SEGMENT 4u       /* q and T are not cameras of one segment */
#define ORB_GRAPH_EDGE_NONFINITE 5u     /* an entry of the fix's r, t is not finite */
#define ORB_GRAPH_EDGE_SEGMENT_INVALID 6u /* the segment is ORB_GRAPH_INVALID */
typedef struct {            /* zero-initialised = the defaults */
    uint32_t rounds;        /* Gauss-Newton rounds, 1..16 (0: 4) */
    uint32_t cg_iterations; /* conjugate-gradient iterations of a round, 1..512 (0: the segment's free cameras, at most 512) */
    uint32_t min_inliers;   /* a fix qualifies with at least this many inliers (0: 12) */
    float loop_weight;      /* weight of a loop edge against a chain edge's 1 (0: 1.0); finite, >= 0 */
    float rotation_weight;  /* weight of |e_R|^2 against |e_t|^2 (0: 1.0); finite, >= 0 */
    uint32_t flags;         /* ORB_GRAPH_USE_MINIMAL or 0 */
    uint32_t reserved[2];   /* must be 0 (ORB_EINVAL otherwise) */
} OrbGraphParams;           /* 32 bytes */

typedef struct {
    float r[9];             /* row-major R, X_g = R X_origin + t: the camera in its segment's frame, as OrbFramePose */
    float t[3];
    float cost_before;      /* the segment's cost under the trajectory's poses; the same in each of its frames */
    float cost_after;       /* ... under the poses written */
    uint32_t loops;         /* the segment's USED edges */
    uint32_t status;        /* ORB_GRAPH_HELD .. ORB_GRAPH_INVALID */
} OrbGraphPose;             /* 64 bytes */

typedef struct {
    uint32_t verdict;       /* ORB_GRAPH_EDGE_*: the first of PG-4 that applies */
    float cost_before;      /* the edge's own cost under the trajectory's poses and under the poses written; 0 unless USED */
    float cost_after;
    uint32_t origin;        /* the fix's `origin`, as read */
} OrbGraphEdge;             /* 16 bytes */

/* ORB_EINVAL for a NULL program, rounds > 16, cg_iterations > 512, a weight that is not finite or negative, an unknown flag or a
 * reserved word that is not 0 (params NULL: the defaults); then ORB_ESTATE unless the last orb_trajectory_consecutive,
 * orb_match_pairs and orb_loop_pairs are all of the current batch and output set; then ORB_EINVAL for n_pairs outside 1 .. the
 * entries of the last orb_loop_pairs.  Asynchronous on `stream` (NULL: as orb_match_guided chooses; the call does not change it),
 * ordered behind those three stages' last calls and the last call of its own when they ran on another stream; the three wait for
 * such a call on another stream before they overwrite what it reads.  Result buffers of its own (allocated by the first call:
 * about 400 bytes per frame of max_batch). */
int orb_graph_pairs(OrbProgram *p, uint32_t n_pairs, const OrbGraphParams *params, void *stream);
/* Copy the record of frame `frame` of the last orb_graph_pairs call to the host (synchronises); ORB_ESTATE before any call,
 * ORB_EINVAL for a frame outside the frames of the trajectory call it read or pose NULL. */
int orb_graph_read(OrbProgram *p, uint32_t frame, OrbGraphPose *pose);
/* Copy the verdicts of entries 0 .. n - 1 of the last orb_graph_pairs call (synchronises); ORB_ESTATE before any call, ORB_EINVAL
 * for n above its n_pairs or dst NULL with n > 0. */
int orb_graph_edges(OrbProgram *p, OrbGraphEdge *dst, size_t n);

/* ---- trajectory segments joined through loop fixes (NOT in the reference; definition SJ-1..SJ-7 in DESIGN.md section 30) ----
 * A LOST frame or a RESTART starts a new segment of the trajectory with its own frame and unit, and orb_graph_pairs refuses a fix
 * whose query and target lie in different segments.  Such a fix gives the whole similarity between the two: camera q in segment
 * `origin`'s frame and unit (pose_r, pose_t) and, from the trajectory, in segment `query_origin`'s; an inlier keypoint of q that a
 * landmark of each segment owns has a depth in each unit, and the lower median of the ratios is the scale (TJ-3, TJ-4 on this
 * call's parameters).  Every segment takes, among its entries that hold, the one with the most consistent ratios (then the lowest
 * index) as its link to an EARLIER origin; the links form a forest and are chained, and every frame is written in the frame and
 * unit of its segment's root.  Binary32 arithmetic in a fixed order, no fused operations: a CPU restatement gives the same bits.
 * Nothing is fed back into another stage, and no other stage's results are written. */
#define ORB_JOIN_USE_MINIMAL 1u         /* flags: a fix of status ORB_LOCALIZE_MINIMAL qualifies too */
#define ORB_JOIN_COPIED 0u              /* the frame's segment is a root: r, t, scale of the trajectory bit for bit, gain 1 */
#define ORB_JOIN_MOVED 1u               /* the frame in its root's frame and unit */
#define ORB_JOIN_SEGMENT_NONE 0u        /* the frame is no segment's origin */
#define ORB_JOIN_SEGMENT_ROOT 1u        /* an origin without a chosen link */
#define ORB_JOIN_SEGMENT_LINKED 2u      /* an origin joined to an earlier one */
#define ORB_JOIN_LINK_HOLDS 0u          /* the entry gives a similarity between its two segments */
#define ORB_JOIN_LINK_STATUS 1u         /* the fix is not OK (nor MINIMAL under ORB_JOIN_USE_MINIMAL) */
#define ORB_JOIN_LINK_FEW 2u            /* inliers < min_inliers */
#define ORB_JOIN_LINK_RANGE 3u          /* q or T outside the trajectory's frames, q outside the landmarks', or q without an origin */
#define ORB_JOIN_LINK_SAME 4u           /* q and T lie in one segment: orb_graph_pairs' business */
#define ORB_JOIN_LINK_FORWARD 5u        /* origin > query_origin: a link hangs the later origin under the earlier one */
#define ORB_JOIN_LINK_NONFINITE 6u      /* an entry of pose_r, pose_t, of camera q's record or of the similarity is not finite */
#define ORB_JOIN_LINK_RATIO_FEW 7u      /* fewer than min_shared ratios */
#define ORB_JOIN_LINK_RATIO_SPREAD 8u   /* fewer than consistent_permille of them within scale_tolerance of their median */
typedef struct {            /* zero-initialised = the defaults */
    uint32_t min_inliers;   /* a fix qualifies with at least this many inliers (0: 12) */
    uint32_t min_shared;    /* ratios an entry needs (0: 8) */
    float scale_tolerance;  /* a ratio is consistent within this share of the median (0: 0.1); finite, >= 0 */
    uint32_t consistent_permille; /* consistent ratios an entry needs, per thousand (0: 500; <= 1000) */
    uint32_t flags;         /* ORB_JOIN_USE_MINIMAL or 0 */
    uint32_t reserved[3];   /* must be 0 (ORB_EINVAL otherwise) */
} OrbJoinParams;            /* 32 bytes */

typedef struct {
    float r[9];             /* row-major R, X_f = R X_root + t: the camera in its root's frame and unit */
    float t[3];
    float scale;            /* gain * the trajectory's scale */
    float gain;             /* units of the root per unit of the frame's segment; 1 when COPIED */
    uint32_t root;          /* the origin whose frame this is */
    uint32_t status;        /* ORB_JOIN_COPIED, ORB_JOIN_MOVED */
} OrbJoinPose;              /* 64 bytes */

typedef struct {
    float r[9];             /* sigma X_b = R X_root + t: the root's coordinates in this origin's frame (the identity for a root) */
    float t[3];
    float sigma;            /* units of the root per unit of this segment */
    uint32_t root;
    uint32_t link;          /* the list index of the chosen entry, 0xffffffff: none */
    uint32_t status;        /* ORB_JOIN_SEGMENT_* */
} OrbJoinSegment;           /* 64 bytes */

typedef struct {
    uint32_t verdict;       /* ORB_JOIN_LINK_*: the first of SJ-3 that applies */
    uint32_t origin;        /* the fix's words, as read */
    uint32_t query_origin;
    uint32_t shared;        /* the entry's ratios; 0 unless HOLDS, RATIO_FEW or RATIO_SPREAD */
    uint32_t consistent;    /* ... those within scale_tolerance of gamma */
    float gamma;            /* their lower median: units of `origin` per unit of `query_origin` */
    uint32_t chosen;        /* 1: this entry is its segment's link */
    uint32_t reserved;
} OrbJoinLink;              /* 32 bytes */

/* ORB_EINVAL for a NULL program, a scale_tolerance that is not finite or negative, consistent_permille > 1000, an unknown flag or
 * a reserved word that is not 0 (params NULL: the defaults); then ORB_ESTATE unless the last orb_match_consecutive,
 * orb_trajectory_consecutive, orb_landmarks_consecutive, orb_match_pairs and orb_loop_pairs are all of the current batch and output
 * set; then ORB_EINVAL for n_pairs outside 1 .. the entries of the last orb_loop_pairs, or when the landmarks call's frames *
 * max_features reaches 2^32 - 1.  Asynchronous on `stream` (NULL: as orb_match_guided chooses; the call does not change it),
 * ordered behind those five stages' last calls and the last call of its own when they ran on another stream; the five wait for
 * such a call on another stream before they overwrite what it reads.  Result buffers of its own (allocated by the first call:
 * about 4 + 4 ORB_PAIRS_PER_FRAME bytes per keypoint slot of max_batch). */
int orb_join_pairs(OrbProgram *p, uint32_t n_pairs, const OrbJoinParams *params, void *stream);
/* Copy the record of frame `frame` of the last orb_join_pairs call to the host (synchronises); ORB_ESTATE before any call,
 * ORB_EINVAL for a frame outside the frames of the trajectory call it read or pose NULL. */
int orb_join_read(OrbProgram *p, uint32_t frame, OrbJoinPose *pose);
/* Copy the segment records of frame slots 0 .. n - 1 of the last orb_join_pairs call (synchronises); ORB_ESTATE before any call,
 * ORB_EINVAL for n above its frames or dst NULL with n > 0. */
int orb_join_segments(OrbProgram *p, OrbJoinSegment *dst, size_t n);
/* Copy the link records of entries 0 .. n - 1 of the last orb_join_pairs call (synchronises); ORB_ESTATE before any call, ORB_EINVAL
 * for n above its n_pairs or dst NULL with n > 0. */
int orb_join_links(OrbProgram *p, OrbJoinLink *dst, size_t n);
/* For tests: the device address of the inlier bytes [ORB_PAIRS_PER_FRAME * max_batch][max_features] that orb_loop_pairs writes and
 * orb_loop_pairs_read and orb_join_pairs read.  The caller orders its own writes.  ORB_ESTATE until a loop call has run. */
int orb_debug_loop_mask_buffer(OrbProgram *p, void **mask);

/* ---- corrected poses and landmarks in one root frame (NOT in the reference; definition RM-1..RM-6 in DESIGN.md section 31) ----
 * orb_graph_pairs leaves corrected cameras per segment and orb_join_pairs every segment's similarity to its root; neither moves a
 * landmark.  This stage hands out one corrected map: every frame's camera -- the graph's where the graph moved it, else the
 * trajectory's -- composed with its segment's similarity, and every GOOD landmark of orb_landmarks_consecutive carried along: with
 * the camera of its first view from where the trajectory had it to where the graph put it, then through the similarity into the
 * root's frame and unit.  Nothing is triangulated again.  Binary32 arithmetic in a fixed order, no fused operations: a CPU
 * restatement gives the same bits.  Nothing is fed back into another stage, and no other stage's results are written. */
#define ORB_REMAP_GRAPH 1u              /* flags: the last orb_graph_pairs is a source */
#define ORB_REMAP_JOIN 2u               /* flags: the last orb_join_pairs is a source; flags 0: both */
#define ORB_REMAP_FROM_GRAPH 1u         /* status bit: r, t start from the graph's record (REFINED, STALLED or FAILED) */
#define ORB_REMAP_MOVED 2u              /* status bit: the frame's segment is LINKED: the frame in its root's frame and unit */
typedef struct {            /* zero-initialised = the defaults */
    uint32_t flags;         /* ORB_REMAP_GRAPH | ORB_REMAP_JOIN; 0: both */
    uint32_t reserved[7];   /* must be 0 (ORB_EINVAL otherwise) */
} OrbRemapParams;           /* 32 bytes */

typedef struct {
    float r[9];             /* row-major R, X_f = R X_root + t */
    float t[3];
    float scale;            /* gain * the trajectory's scale */
    float gain;             /* units of the root per unit of the frame's segment; 1 unless MOVED */
    uint32_t root;          /* the origin whose frame this is */
    uint32_t status;        /* ORB_REMAP_FROM_GRAPH | ORB_REMAP_MOVED */
} OrbRemapPose;             /* 64 bytes */

typedef struct {
    uint32_t good;          /* records with ORB_POINT_GOOD among the pair's max_features slots */
    uint32_t moved;         /* of them, those written through at least one step with finite coordinates */
    uint32_t dropped;       /* of them, those a step left with a coordinate that is not finite: written with x, y, z, flags 0 */
    uint32_t root;          /* the root of the pair's segment; the landmark row's origin when it has none (0xffffffff as it is) */
} OrbRemapRow;              /* 16 bytes */

/* ORB_EINVAL for a NULL program, an unknown flag or a reserved word that is not 0 (params NULL: the defaults); then ORB_ESTATE
 * unless the last orb_trajectory_consecutive, orb_landmarks_consecutive and every named source are all of the current batch and
 * output set; then ORB_ESTATE when a named source covered another number of frames than the last trajectory call (it was computed
 * from an earlier one).  Asynchronous on `stream` (NULL: as orb_match_guided chooses; the call does not change it), ordered behind
 * those stages' last calls and the last call of its own when they ran on another stream; they wait for such a call on another
 * stream before they overwrite what it reads.  Result buffers of its own (allocated by the first call: 32 bytes per keypoint slot
 * of max_batch). */
int orb_remap_frames(OrbProgram *p, const OrbRemapParams *params, void *stream);
/* Copy the record of frame `frame` of the last orb_remap_frames call to the host (synchronises); ORB_ESTATE before any call,
 * ORB_EINVAL for a frame outside the frames of the trajectory call it read or pose NULL. */
int orb_remap_read(OrbProgram *p, uint32_t frame, OrbRemapPose *pose);
/* Copy the row of pair `pair` of the last orb_remap_frames call (row may be NULL) and its first n landmark records (indexed as
 * orb_landmarks_read) to the host (synchronises); ORB_ESTATE before any call, ORB_EINVAL for a pair outside the pairs it covered
 * (the landmarks call's, at most the trajectory call's frames - 1) or landmarks NULL with n > 0. */
int orb_remap_landmarks(OrbProgram *p, uint32_t pair, OrbRemapRow *row, OrbLandmark *landmarks, size_t n);

/* ---- a keyframe store that outlives a batch (NOT in the reference; definition KF-1..KF-5 in DESIGN.md section 32) ----
 * Every stage above works on the last batch, and a database hit of orb_place_frames (ORB_PLACE_DB | e) names a frame whose
 * keypoints, descriptors and landmarks left the device with its batch.  A program may keep `slots` keyframes on the device: a
 * slot is a header, max_features CornerData, max_features CornerDescriptor and max_features OrbMapPoint.  orb_keyframes_insert
 * fills slots from frames of the last batch, orb_match_keyframes matches frames of the last batch against slots and
 * orb_localize_keyframes gives the query camera from the slot's points, as orb_match_pairs and orb_loop_pairs do inside one
 * batch: for a frame T inserted into slot s, an entry (q, s) gives the bytes the entry (q, T) gives there.  The store survives
 * orb_extract_batch_*, orb_batch_select_output and every stage call; only the calls of this section write it, and they write no
 * other stage's buffer.  Binary32 arithmetic in a fixed order, no fused operations: a CPU restatement gives the same bits. */
#define ORB_KEYFRAME_SLOTS_MAX 1024u     /* = ORB_PLACE_DB_MAX: database row e of orb_place_frames can be slot e */
#define ORB_KEYFRAME_NONE 0xffffffffu    /* OrbMapPoint::key of a keypoint without a landmark; OrbKeyframe::origin of a NOMAP keyframe */
#define ORB_KEYFRAME_EMPTY 0u            /* OrbKeyframe::status: the slot holds nothing (every byte of it is 0) */
#define ORB_KEYFRAME_STORED 1u           /* a camera and points in its frame */
#define ORB_KEYFRAME_NOMAP 2u            /* keypoints and descriptors only: the frame lay outside the map, or its pose was not finite */
typedef struct {
    float x, y, z;          /* the landmark in the keyframe camera's frame, in the unit of its segment (0 without one) */
    uint32_t key;           /* pair * max_features + slot of the landmark in the landmarks call it came from (LC-2's owner key);
                             * ORB_KEYFRAME_NONE: the keypoint views no landmark */
} OrbMapPoint;              /* 16 bytes */
typedef struct {
    float r[9];             /* row-major R, X_kf = R X_origin + t: the keyframe camera in its segment's frame (the identity when the
                             * frame is its own origin), as OrbFramePose */
    float t[3];             /* in units of that segment */
    float scale;            /* OrbFramePose::scale of the source frame */
    uint32_t keypoints;     /* records of the slot: min(the frame's counter, max_features) */
    uint32_t points;        /* of them: with a key that is not ORB_KEYFRAME_NONE */
    uint32_t frame;         /* the source frame in its batch */
    uint32_t origin;        /* OrbFramePose::origin of the source frame; ORB_KEYFRAME_NONE for NOMAP */
    uint32_t user[2];       /* the caller's, carried and never read */
    uint32_t status;        /* ORB_KEYFRAME_*; NOMAP: r, t, scale 0 and every point (0, 0, 0, NONE) */
    uint32_t reserved[4];   /* 0 */
} OrbKeyframe;              /* 96 bytes */
typedef struct { uint32_t frame, slot, user[2]; } OrbKeyframeEntry; /* 16 bytes */
typedef struct { uint32_t query, slot; } OrbKeyframePair;           /* 8 bytes */
typedef struct {            /* OrbLoopFix word for word, with the slot where the query's origin is there */
    float r[9];             /* row-major R, X_q = R X_kf + t */
    float t[3];             /* in units of the keyframe's segment */
    float step;             /* |t| */
    float pose_r[9];        /* row-major R, X_q = R X_origin + t: camera q in the frame of `origin`; 0 when an entry is not finite */
    float pose_t[3];        /* in units of that segment */
    uint32_t origin;        /* OrbKeyframe::origin of the slot */
    uint32_t slot;          /* the entry's slot */
    uint32_t candidates;    /* 3D-2D correspondences */
    uint32_t inliers;       /* of them: within max_reproj_px under the model written */
    uint32_t hypothesis;    /* the winning sample */
    uint32_t status;        /* ORB_LOCALIZE_*; NOMAP: a NOMAP keyframe.  NOMAP, FEW and DEGENERATE: every other word 0 */
    uint32_t reserved[1];   /* 0 */
} OrbKeyframeFix;           /* 128 bytes */

/* Allocates the store, all or none: slots x (96 + 64 max_features) bytes, and (max_batch + slots) x 32 max_features bytes for the
 * descriptors of a batch in front of the slots' (the matchers address both through one base).  ORB_EINVAL for a NULL program or
 * slots outside 1 .. ORB_KEYFRAME_SLOTS_MAX; a repeat with the same number does nothing, with another number it is ORB_ESTATE.
 * Every slot starts EMPTY.  Synchronises. */
int orb_keyframes_reserve(OrbProgram *p, uint32_t slots);
/* Fills slot list[i].slot from frame list[i].frame of the last batch, a filled slot included: the first min(counter,
 * max_features) corners and descriptors byte for byte, the camera of the frame in its segment as orb_loop_pairs takes a target's
 * (LC-3), and for every keypoint the landmark that owns it (LC-2, on the last orb_landmarks_consecutive) under that camera --
 * exactly the point orb_loop_pairs would localise against.  A frame outside the landmarks call's frames, or with a pose that is
 * not finite, is stored NOMAP.  The rest of the slot is 0.  ORB_EINVAL for a NULL program; ORB_ESTATE before
 * orb_keyframes_reserve or a batch; ORB_EINVAL for a NULL list, n outside 1 .. max_batch, a frame at or above the last batch's
 * frames, a slot at or above the store's, or two entries naming one slot (the message names the first); then ORB_ESTATE unless
 * the last orb_match_consecutive, orb_trajectory_consecutive and orb_landmarks_consecutive are all of the current batch and
 * output set; then ORB_EINVAL when the landmarks call's frames * max_features reach 2^32 - 1.  Asynchronous on `stream` (NULL:
 * as orb_match_guided chooses; the call does not change it), ordered behind those three stages, its own last call and the
 * keyframe calls that read the store when they ran on another stream.  The list is copied through a pinned buffer: it is the
 * caller's again when the call returns. */
int orb_keyframes_insert(OrbProgram *p, const OrbKeyframeEntry *list, uint32_t n, void *stream);
/* Copy the header of `slot` (may be NULL) and the first n records of each array that is not NULL to the host (synchronises; n
 * is clipped to max_features).  An EMPTY slot reads as zeros.  ORB_EINVAL for a NULL program, ORB_ESTATE before
 * orb_keyframes_reserve, ORB_EINVAL for a slot at or above the store's. */
int orb_keyframes_read(OrbProgram *p, uint32_t slot, OrbKeyframe *header, CornerData *corners, CornerDescriptor *descriptors,
                       OrbMapPoint *points, size_t n);
/* Writes `slot` from the host: what orb_keyframes_read gave, in this program or another of the same configuration, behaves the
 * same byte for byte.  The records past n become 0.  ORB_EINVAL for a NULL program, ORB_ESTATE before orb_keyframes_reserve;
 * ORB_EINVAL for a slot at or above the store's, a NULL header, n != header->keypoints or above max_features, a NULL array with
 * n > 0, a status that is neither STORED nor NOMAP, a reserved word that is not 0, or header->points other than the keys among
 * the n points that are not ORB_KEYFRAME_NONE.  Synchronises (it waits for the keyframe calls in flight). */
int orb_keyframes_load(OrbProgram *p, uint32_t slot, const OrbKeyframe *header, const CornerData *corners,
                       const CornerDescriptor *descriptors, const OrbMapPoint *points, size_t n);
/* Empties `slot` (every byte 0).  Errors as orb_keyframes_read; synchronises as orb_keyframes_load. */
int orb_keyframes_remove(OrbProgram *p, uint32_t slot);
/* Row i of the result holds orb_match_pairs' record (MP-2) for every stored keypoint of frame list[i].query of the last batch
 * against the `keypoints` records of slot list[i].slot.  Duplicates are allowed.  The call needs a batch and a store, no stage.
 * ORB_EINVAL for a NULL program; ORB_ESTATE before orb_keyframes_reserve or a batch; ORB_EINVAL for a NULL list, n outside
 * 1 .. ORB_PAIRS_PER_FRAME * max_batch, a query at or above the last batch's frames, a slot at or above the store's or an EMPTY
 * slot (the message names the first entry).  The matcher is chosen as orb_match_pairs chooses it; on the matrix cores the store
 * keeps 128 bytes per record for the descriptors as fp4 (allocated by the first call, refreshed when the store has changed).
 * Asynchronous on `stream` as orb_match_pairs, ordered behind the store's last insert and its own last call on another stream. */
int orb_match_keyframes(OrbProgram *p, const OrbKeyframePair *list, uint32_t n, void *stream);
/* As orb_match_pairs_read, for row `entry` of the last orb_match_keyframes call. */
int orb_match_keyframes_read(OrbProgram *p, uint32_t entry, OrbMatch *dst, size_t n);
/* Fixes of entries 0 .. n - 1 of the last orb_match_keyframes call: orb_loop_pairs' candidates, RANSAC, refit and compose (the
 * same draw stream, the list index as the pair) with the slot's `keypoints`, keys and points where that call takes the target
 * frame's counter, owners and landmarks under camera T.  params as orb_loop_pairs checks them, with the same errors; then
 * ORB_ESTATE unless the last orb_match_keyframes is of the current batch and output set and no orb_keyframes_reserve, _insert,
 * _load or _remove came after it; then ORB_EINVAL for n outside 1 .. the entries it matched.  Asynchronous on `stream` as
 * orb_loop_pairs.  Result buffers of its own (allocated by the first call, the size of orb_loop_pairs').  (Declared `extern`, as
 * its read call: the two are no part of the orb_localize_consecutive family, which is listed by its prefix.) */
extern int orb_localize_keyframes(OrbProgram *p, uint32_t n, const OrbLoopParams *params, void *stream);
/* As orb_loop_pairs_read, for entry `entry` of the last orb_localize_keyframes call. */
extern int orb_localize_keyframes_read(OrbProgram *p, uint32_t entry, OrbKeyframeFix *fix, uint8_t *inliers, size_t n);

/* ---- a batch's path and landmarks in the stored map (NOT in the reference; definition AN-1..AN-7 in DESIGN.md section 33) ----
 * An OrbKeyframeFix is one camera of the batch in the frame and unit of one keyframe's segment; the batch's trajectory and
 * landmarks stay in the batch's own frames and units.  This stage is orb_join_pairs with a keyframe on the far side: entry
 * (q, s) of the last orb_localize_keyframes gives camera q in the keyframe's segment (pose_r, pose_t) and, from the trajectory,
 * in its own segment b = the origin of frame q's record; an inlier keypoint of q whose matched keypoint of the slot carries a
 * stored point and which a landmark of b owns has a depth in each unit, and the lower median of the ratios is the scale (TJ-3,
 * TJ-4 on this call's parameters).  Every segment of the batch takes, among its entries that hold, the one with the most
 * consistent ratios (then the lowest index) and hangs directly under that keyframe's segment -- there is no chain.  Every frame
 * of an anchored segment is written in the map's frame and unit, and every GOOD landmark of such a segment carried along.
 * Binary32 arithmetic in a fixed order, no fused operations: a CPU restatement gives the same bits.  Nothing is fed back into
 * another stage, and neither another stage's results nor the store are written. */
#define ORB_ANCHOR_USE_MINIMAL 1u       /* flags: a fix of status ORB_LOCALIZE_MINIMAL qualifies too */
#define ORB_ANCHOR_FREE 0u              /* OrbAnchorPose::status: r, t, scale of the trajectory bit for bit, gain 1, slot 0xffffffff */
#define ORB_ANCHOR_ANCHORED 1u          /* the frame in the frame and unit of the segment of keyframe `slot` */
#define ORB_ANCHOR_SEGMENT_NONE 0u      /* the frame slot is no segment's origin */
#define ORB_ANCHOR_SEGMENT_FREE 1u      /* an origin without a chosen entry */
#define ORB_ANCHOR_SEGMENT_ANCHORED 2u  /* an origin hung under a keyframe's segment */
#define ORB_ANCHOR_LINK_HOLDS 0u        /* the entry gives a similarity between its segment and the keyframe's */
#define ORB_ANCHOR_LINK_STATUS 1u       /* the fix is not OK (nor MINIMAL under ORB_ANCHOR_USE_MINIMAL); a NOMAP keyframe */
#define ORB_ANCHOR_LINK_FEW 2u          /* inliers < min_inliers */
#define ORB_ANCHOR_LINK_RANGE 3u        /* q outside the trajectory's or the landmarks' frames, or q without an origin */
#define ORB_ANCHOR_LINK_NONFINITE 4u    /* an entry of r, t, pose_r, pose_t, of camera q's record or of the similarity is not finite */
#define ORB_ANCHOR_LINK_RATIO_FEW 5u    /* fewer than min_shared ratios */
#define ORB_ANCHOR_LINK_RATIO_SPREAD 6u /* fewer than consistent_permille of them within scale_tolerance of their median */
#define ORB_ANCHOR_NONE 0xffffffffu     /* no slot, no entry, no origin */
typedef struct {            /* zero-initialised = the defaults; OrbJoinParams' fields */
    uint32_t min_inliers;   /* a fix qualifies with at least this many inliers (0: 12) */
    uint32_t min_shared;    /* ratios an entry needs (0: 8) */
    float scale_tolerance;  /* a ratio is consistent within this share of the median (0: 0.1); finite, >= 0 */
    uint32_t consistent_permille; /* consistent ratios an entry needs, per thousand (0: 500; <= 1000) */
    uint32_t flags;         /* ORB_ANCHOR_USE_MINIMAL or 0 */
    uint32_t reserved[3];   /* must be 0 (ORB_EINVAL otherwise) */
} OrbAnchorParams;          /* 32 bytes */

typedef struct {
    float r[9];             /* row-major R, X_f = R X_map + t: the camera in the frame of the keyframe's segment (FREE: of its own) */
    float t[3];             /* in units of that segment */
    float scale;            /* gain * the trajectory's scale */
    float gain;             /* units of the map per unit of the frame's segment; 1 when FREE */
    uint32_t slot;          /* the keyframe the frame's segment hangs under; ORB_ANCHOR_NONE when FREE */
    uint32_t status;        /* ORB_ANCHOR_FREE, ORB_ANCHOR_ANCHORED */
} OrbAnchorPose;            /* 64 bytes */

typedef struct {
    float r[9];             /* gamma X_b = R X_map + t: the map's coordinates in this origin's frame (the identity unless ANCHORED) */
    float t[3];
    float gamma;            /* units of the map per unit of this segment (1 unless ANCHORED) */
    uint32_t slot;          /* the chosen entry's slot; ORB_ANCHOR_NONE unless ANCHORED, as link, map_origin and map_frame */
    uint32_t link;          /* the list index of the chosen entry */
    uint32_t map_origin;    /* OrbKeyframe::origin, frame and user of that slot: which stored map the segment landed in */
    uint32_t map_frame;
    uint32_t user[2];       /* 0 unless ANCHORED */
    uint32_t status;        /* ORB_ANCHOR_SEGMENT_* */
    uint32_t reserved[4];   /* 0 */
} OrbAnchorSegment;         /* 96 bytes */

typedef struct {
    uint32_t verdict;       /* ORB_ANCHOR_LINK_*: the first of AN-3 that applies */
    uint32_t query_origin;  /* the origin word of frame q's record, as read; 0 when q lies outside the trajectory's frames */
    uint32_t slot;          /* the entry's slot */
    uint32_t shared;        /* the entry's ratios; 0 unless HOLDS, RATIO_FEW or RATIO_SPREAD */
    uint32_t consistent;    /* ... those within scale_tolerance of gamma */
    float gamma;            /* their lower median: units of the keyframe's segment per unit of `query_origin` */
    uint32_t chosen;        /* 1: this entry anchors its segment */
    uint32_t reserved;
} OrbAnchorLink;            /* 32 bytes */

typedef struct {
    uint32_t good;          /* records with ORB_POINT_GOOD among the pair's max_features slots */
    uint32_t moved;         /* of them, those written in the map's frame with finite coordinates */
    uint32_t dropped;       /* of them, those the step left with a coordinate that is not finite: written with x, y, z, flags 0 */
    uint32_t origin;        /* the landmark row's origin, as it is */
    uint32_t slot;          /* the keyframe that origin hangs under, ORB_ANCHOR_NONE when it is not ANCHORED */
    uint32_t map_origin;    /* OrbKeyframe::origin of that slot, ORB_ANCHOR_NONE likewise */
    uint32_t reserved[2];   /* 0 */
} OrbAnchorRow;             /* 32 bytes */

/* Entries 0 .. n - 1 of the last orb_localize_keyframes.  ORB_EINVAL for a NULL program, a scale_tolerance that is not finite
 * or negative, consistent_permille > 1000, an unknown flag or a reserved word that is not 0 (params NULL: the defaults); then
 * ORB_ESTATE unless the last orb_match_consecutive, orb_trajectory_consecutive, orb_landmarks_consecutive, orb_match_keyframes
 * and orb_localize_keyframes are all of the current batch and output set and no orb_keyframes_reserve, _insert, _load or _remove
 * came after that orb_match_keyframes; then ORB_EINVAL for n outside 1 .. the entries of the last orb_localize_keyframes, or
 * when the landmarks call's frames * max_features reaches 2^32 - 1.  Asynchronous on `stream` (NULL: as orb_match_guided
 * chooses; the call does not change it), ordered behind those five stages' last calls, the store's last insert and the last call
 * of its own when they ran on another stream; they wait for such a call on another stream before they overwrite what it reads,
 * and orb_keyframes_load and _remove wait for it on the host.  Result buffers of its own (allocated by the first call: about
 * 36 + 4 ORB_PAIRS_PER_FRAME bytes per keypoint slot of max_batch).  A landmark record keeps its origin word: the row says where
 * the pair's segment went. */
int orb_anchor_frames(OrbProgram *p, uint32_t n, const OrbAnchorParams *params, void *stream);
/* Copy the record of frame `frame` of the last orb_anchor_frames call to the host (synchronises); ORB_ESTATE before any call,
 * ORB_EINVAL for a frame outside the frames of the trajectory call it read or pose NULL. */
int orb_anchor_read(OrbProgram *p, uint32_t frame, OrbAnchorPose *pose);
/* Copy the segment records of frame slots 0 .. n - 1 of the last orb_anchor_frames call (synchronises); ORB_ESTATE before any
 * call, ORB_EINVAL for n above its frames or dst NULL with n > 0. */
int orb_anchor_segments(OrbProgram *p, OrbAnchorSegment *dst, size_t n);
/* Copy the link records of entries 0 .. n - 1 of the last orb_anchor_frames call (synchronises); ORB_ESTATE before any call,
 * ORB_EINVAL for n above its entries or dst NULL with n > 0. */
int orb_anchor_links(OrbProgram *p, OrbAnchorLink *dst, size_t n);
/* Copy the row of pair `pair` of the last orb_anchor_frames call (row may be NULL) and its first n landmark records (indexed as
 * orb_landmarks_read) to the host (synchronises); ORB_ESTATE before any call, ORB_EINVAL for a pair outside the pairs it covered
 * (LC-1's frames - 1) or landmarks NULL with n > 0. */
int orb_anchor_landmarks(OrbProgram *p, uint32_t pair, OrbAnchorRow *row, OrbLandmark *landmarks, size_t n);
/* For tests: the device addresses of the rows [ORB_PAIRS_PER_FRAME * max_batch][max_features] OrbMatch that orb_match_keyframes
 * writes, and of the records [ORB_PAIRS_PER_FRAME * max_batch] OrbKeyframeFix and the inlier bytes [ORB_PAIRS_PER_FRAME *
 * max_batch][max_features] that orb_localize_keyframes writes; orb_anchor_frames reads all three.  Each pointer may be NULL.  The
 * caller orders its own writes.  ORB_ESTATE until a localize_keyframes call has run. */
int orb_debug_keyframe_buffers(OrbProgram *p, void **rows, void **fixes, void **mask);

/* Keypoint coordinates are in the octave's own pixel grid (fast.wgsl:143-150).  Centre of that pixel in level-0
 * pixel units, for consumers that work across octaves: a level-m texel covers 2^m level-0
 * pixels (exact halving; for odd sizes the blit's own mapping, blit.wgsl:17-36, differs by less than a pixel). */
void orb_corner_level0_xy(const CornerData *c, float *x0, float *y0);

/* ---- inspection (parity tests) ---- */
#define ORB_PLANE_GRAY 0
#define ORB_PLANE_BLUR 1
/* Copies one pyramid level (binary16 bit patterns, row-major) of a frame of the last call.
 * The fused pipeline does not materialise every plane; it returns ORB_ESTATE for those. */
int orb_debug_read_plane(OrbProgram *p, uint32_t frame, int kind, uint32_t level, uint16_t *dst, size_t n_texels);
/* Level geometry: width/height of mip `level` (max(1, W>>level), wgpu mip chain orb.rs:224-233). */
int orb_level_size(const OrbProgram *p, uint32_t level, uint32_t *width, uint32_t *height);
/* Device scalar helpers, so the tests can pin CRD-3 / CRD-9 on the GPU itself (host arrays). */
int orb_debug_f32_to_f16(OrbProgram *p, const float *src, uint16_t *dst, size_t n);
int orb_debug_angle_code(OrbProgram *p, const float *cy, const float *cx, uint32_t *dst, size_t n);
/* The program's table of the BRIEF pattern rotated by every angle code (brief.wgsl:50-57 evaluated once per code instead
 * of once per keypoint): codes x 256 tests x {a, b} int16 BYTE offsets 2 * (ry * pitch + rx) into a window of binary16 texels,
 * stored [code][lane 0..63][test lane + 64 e, e = 0..3][a, b].  Writes min(n_entries, codes * 512) values; *codes and *pitch
 * (either may be NULL) say what the table was built for. */
int orb_debug_rot_table(OrbProgram *p, int16_t *dst, size_t n_entries, uint32_t *codes, uint32_t *pitch);
/* For tests: the blur column table that the program built at creation for the bands of `level` (the fused pipeline's level 0 on
 * full-width bands), one 24-byte entry per column blur_q .. width - 1: uint16 a0, a1, b0, b1, float fa, fb, f2, uint32 0 -- pass 2
 * at the column lerps pass 1 at two columns with fraction f2; pass 1 at the first (second) of them lerps the grey texels a0, a1
 * (b0, b1) with fraction fa (fb), and a0 (b0) == 0xffff says that pass-1 column lies where pass 1 is one value per row.  Writes
 * min(n_entries, *n_var) entries; *n_var is 0 for a level whose bands build the table themselves; *blur_p and *blur_q are the
 * level's constant stretches of pass 1 and of the final blur.  dst may be NULL with n_entries 0, and so may each of the three. */
int orb_debug_blur_col_table(OrbProgram *p, uint32_t level, void *dst, size_t n_entries, uint32_t *n_var, uint32_t *blur_p,
                             uint32_t *blur_q);
/* For tests: device pointers of what orb_trajectory_consecutive reads besides the raw counters (any of the three may be NULL):
 * matches[max_batch][max_features] OrbMatch (row f: the queries of frame f), poses[max_batch] OrbPairPose and
 * points[max_batch][max_features] OrbPoint (row f: pair (f, f + 1)).  ORB_ESTATE until an orb_match_consecutive and an
 * orb_pose_consecutive call have allocated them.  A test that writes them orders its own writes: orb_batch_sync / orb_stream_sync
 * on every stream a stage ran on before writing, a device synchronise after writing and before the next call.  No stage's
 * freshness state is touched: the library goes on treating the buffers as the results of its last match and pose calls. */
int orb_debug_pose_buffers(OrbProgram *p, void **matches, void **poses, void **points);
/* For tests: the device pointer of the frame records that orb_trajectory_consecutive writes and that orb_trajectory_read,
 * orb_landmarks_consecutive and orb_bridge_consecutive read (frames may be NULL): frames[max_batch] OrbFramePose, 20 words each.
 * ORB_ESTATE until an orb_trajectory_consecutive call has allocated it.  The ordering of a test's own writes is the caller's, as
 * for orb_debug_pose_buffers, and no stage's freshness state is touched: the library goes on treating the buffer as the result
 * of its last trajectory call. */
int orb_debug_frame_buffer(OrbProgram *p, void **frames);

/* ---- measurement ---- */
#define ORB_KERNEL_COUNT 25
/* When enabled every kernel launch is bracketed by hipEvents on its stream. */
int orb_profile_enable(OrbProgram *p, int enable);
int orb_profile_reset(OrbProgram *p);
/* Accumulated device time and number of launches of kernel `id` (synchronises). */
int orb_profile_get(OrbProgram *p, int id, double *total_ms, uint64_t *launches);
const char *orb_kernel_name(int id);

/* ---- synthetic frames, generated on the device ---- */
#define ORB_SYN_GRADIENT 1u
#define ORB_SYN_BLOBS 2u
#define ORB_SYN_WEDGES 4u
#define ORB_SYN_NOISE 8u
#define ORB_SYN_Y8 16u /* one byte per pixel: (77 R + 150 G + 29 B + 128) >> 8 of the recipe (ORB_FLAG_INPUT_Y8 programs) */
/* Frame i gets seed seed0+i.  frames_dev == NULL allocates/uses the program's own input slab
 * (max_batch frames) and returns its address in *out_dev. */
int orb_synth_frames_device(OrbProgram *p, uint8_t *frames_dev, uint32_t n_frames, uint32_t seed0, uint32_t flags,
                            uint8_t **out_dev);
/* Diagnostic: cycle sums of the phases of k_front (2 x 16 values: level 0, levels >= 1); filled only by a
 * diagnostic build (TINYORB_BUILD_STAMPS=1) when the program was created with TINYORB_STAMPS=1. */
int orb_debug_stamps(OrbProgram *p, unsigned long long *dst, size_t n);
/* Device-to-host copy helper for tests that have no other HIP binding. */
int orb_copy_to_host(OrbProgram *p, void *dst_host, const void *src_dev, size_t nbytes);

#ifdef __cplusplus
}
#endif
#endif /* TINYORB_H */
