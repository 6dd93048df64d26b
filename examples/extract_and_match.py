#!/usr/bin/env python3
"""Minimal tour of the Python mirror of `tinyslam::orb` (needs an MI355X; build first: python -m tinyslam_amd.build).

    python examples/extract_and_match.py            # the reference's algorithm (default)
    python examples/extract_and_match.py intended   # the opt-in repaired algorithm, FAST-9 + NMS
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tinyslam_amd import orb

W, H = 640, 480
intended = len(sys.argv) > 1 and sys.argv[1] == "intended"
cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=4096, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=2,
                    flags=(orb.ORB_FLAG_INTENDED | orb.ORB_FLAG_NMS) if intended else 0, fast_arc=9 if intended else 0)

with orb.OrbProgram(cfg) as prog:  # == OrbProgram { config, .. }.init() in the reference (orb.rs:107)
    # --- the reference's six calls, one frame at a time -------------------------------------------------------
    dev = prog.synth_frames_device(2, seed0=7)                      # two synthetic RGBA frames on the device
    frames = prog.copy_to_host(dev, 2 * W * H * 4).reshape(2, H, W, 4)
    prog.write_input_image(frames[0])                               # orb.rs:567
    prog.set_threshold(20.0 / 255.0)                                # orb.rs:585
    total = prog.extract_corners()                                  # orb.rs:469 (raw counter)
    n = min(total, cfg.max_features)
    corners = prog.read_corners(np.zeros(n, dtype=orb.CORNER_DTYPE))       # orb.rs:559
    descriptors = prog.read_descriptors(np.zeros((n, 8), dtype=np.uint32))  # orb.rs:563
    print("%s pipeline, frame 0: %d keypoints, first: %s" % (prog.pipeline(), total, corners[0]))
    x0, y0 = orb.level0_xy(corners)
    print("octave-1 keypoints in level-0 pixels:", np.stack([x0, y0], 1)[corners["octave"] == 1][:3])

    # --- batched mode + matching between consecutive frames ---------------------------------------------------
    prog.extract_batch_host(frames)
    counts = np.minimum(prog.batch_counts(2), cfg.max_features)
    prog.match_consecutive(2)
    m = prog.match_read(0, int(counts[0]))
    good = m["distance"] < 0.8 * m["second"]                        # ratio test on the two best Hamming distances
    print("frame 0 -> 1: %d of %d keypoints pass the ratio test (the two synthetic frames are unrelated scenes)"
          % (int(good.sum()), int(counts[0])))

    # --- geometric verification: a RANSAC homography per pair, refit over its inliers -----------
    prog.verify_consecutive(2)
    model, inlier = prog.verify_read(0, int(counts[0]))
    status = {orb.ORB_VERIFY_OK: "ok", orb.ORB_VERIFY_FEW: "fewer than 4 candidates", orb.ORB_VERIFY_DEGENERATE: "degenerate",
              orb.ORB_VERIFY_MINIMAL: "minimal model"}[int(model["status"])]
    print("frame 0 -> 1 verified: %d candidates, %d inliers (%s), H =\n%s"
          % (int(model["candidates"]), int(model["inliers"]), status, model["h"].reshape(3, 3)))

    # --- epipolar verification and the band search along its lines (DESIGN.md sections 16 and 18) --------------------------
    prog.verify_epipolar(2)
    fmodel, _ = prog.verify_epipolar_read(0, 0)
    if int(fmodel["status"]) in (orb.ORB_VERIFY_OK, orb.ORB_VERIFY_MINIMAL):
        prog.match_epipolar(2, band_px=2.0, radius_px=32.0)  # within 2 px of the epipolar line, 32 px around the keypoint itself
        band = prog.match_epipolar_read(0, int(counts[0]))
        print("frame 0 -> 1 along the epipolar lines: %d keypoints have a candidate" % int((band["index"] != orb.ORB_MATCH_NONE).sum()))
        # --- how the camera moved and where the points are; the intrinsics are the caller's ------------
        prog.pose_consecutive(2, fx=500.0, fy=500.0, cx=(W - 1) / 2, cy=(H - 1) / 2)
        pose, points = prog.pose_read(0, int(counts[0]))
        good = (points["flags"] & orb.ORB_POINT_GOOD) != 0
        print("frame 0 -> 1 pose: status %d, %d of %d inliers triangulated, R =\n%s\nt = %s"
              % (int(pose["status"]), int(good.sum()), int(pose["inliers"]), pose["r"].reshape(3, 3), pose["t"]))
        # --- the pair poses chained into one path and one map; two frames: the origin and one START --------
        prog.trajectory_consecutive(2)
        frame1, world = prog.trajectory_read(1, 0)[0], prog.trajectory_read(0, int(counts[0]))[1]
        print("frame 1 in frame %d's coordinates: status %d, scale %.3f, %d map points"
              % (int(frame1["origin"]), int(frame1["status"]), float(frame1["scale"]), int(((world["flags"] & orb.ORB_POINT_GOOD) != 0).sum())))
    else:
        print("frame 0 -> 1: no fundamental matrix (status %d), no band search and no pose" % int(fmodel["status"]))

    # --- place recognition across batches (meant for the intended mode) -----------------------------------
    # batch A: keep the signatures of the frames worth remembering (here both; a SLAM front-end keeps its keyframes') ...
    prog.place_frames(2, min_gap=1)
    kept = np.stack([prog.place_signature(f) for f in range(2)])        # uint8 (2, 65536) at the default 16 bits x 8 tables
    # ... batch B, later: the same two scenes in the other order, with the kept signatures as the database
    prog.extract_batch_host(frames[::-1].copy())
    prog.place_frames(2, db=kept, min_gap=1)
    for f, row in enumerate(prog.place_read(0, 2)):
        best, who = row["best"][0], int(row["best"][0]["frame"])
        where = ("entry %d of the database" % (who & 0x7FFFFFFF) if who & orb.ORB_PLACE_DB
                 else "frame %d of this batch" % who) if row["n"] else "nothing"
        print("batch B frame %d: %d of its %d signature bits are shared with %s" % (f, int(best["score"]), int(row["bits_set"]), where))

    # --- closing a proposed loop: the place stage proposes frames of this batch, match_pairs and verify_pairs
    # confirm them.  The caller reads the rows and decides which pairs to list; any pairs of the batch's frames may be listed.
    prog.place_frames(2, min_gap=1)
    rows = prog.place_read(0, 2)
    proposed = [(f, int(c["frame"])) for f in range(2) for c in rows[f]["best"][:int(rows[f]["n"])] if c["frame"] < orb.ORB_PLACE_DB]
    pairs = proposed or [(1, 0)]  # (query frame, target frame); backward, distant, consecutive and repeated pairs are all allowed
    prog.match_pairs(pairs)
    prog.verify_pairs(len(pairs), model=orb.ORB_PAIRS_HOMOGRAPHY)
    for i, (q, t) in enumerate(pairs):
        model, inlier = prog.verify_pairs_read(i, int(prog.batch_counts(2)[q]))
        print("loop candidate %d -> %d: status %d, %d candidates, %d inliers" % (q, t, int(model["status"]), int(model["candidates"]), int(inlier.sum())))
