#!/usr/bin/env python3
"""Relocalising a batch against keyframes of an earlier one (needs an MI355X; build first: python -m tinyslam_amd.build).

    python examples/relocalize.py

Two batches of eight views of one synthetic scene.  The first is run through the map chain (match, epipolar verification, pose,
trajectory, landmarks); four of its frames become keyframes: each one's place signature is kept as row e of a database and the
frame itself goes into slot e of the program's keyframe store.  The second batch is extracted over the
first -- the first batch's keypoints, descriptors and landmarks are gone from the device, the store is not --, orb_place_frames
proposes database rows for its frames (ORB_PLACE_DB | e), and those hits are the list of orb_match_keyframes and
orb_localize_keyframes: the pose of each new frame relative to the keyframe and in the keyframe's segment.

The views are near-planar warps of one image, not a camera's motion, so the chain runs with the permissive parameters of
tools/loop_rate.py; the statuses say how the stage judges such views, the calls are what is shown.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from tinyslam_amd import orb
from verify_rate import synth_views

W, H, B, CAP, FOCAL = 640, 480, 8, 4096, 500.0
KEYFRAMES = (0, 2, 4, 6)  # frames of the first batch; frame KEYFRAMES[e] is database row e and slot e
intr = dict(fx=FOCAL, fy=FOCAL, cx=(W - 1) / 2, cy=(H - 1) / 2)
views = synth_views(2 * B, W, H, seed=3)  # sixteen views of one scene
cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=CAP, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B,
                    flags=orb.ORB_FLAG_INTENDED, fast_arc=9)

with orb.OrbProgram(cfg) as prog:
    # --- the first batch: a map, signatures, keyframes ---------------------------------------------------------
    prog.extract_batch_host(views[:B])
    prog.match_consecutive(B)
    prog.verify_epipolar(B)
    prog.pose_consecutive(B, max_reproj_px=1e6, min_good=1, ambiguity_permille=1000, **intr)
    prog.trajectory_consecutive(B, min_shared=1, scale_tolerance=1e6, consistent_permille=1)
    prog.landmarks_consecutive(B, max_reproj_px=1e6, **intr)
    prog.place_frames(B)                                            # builds every frame's signature
    db = np.stack([prog.place_signature(f) for f in KEYFRAMES])     # row e: the signature of keyframe e
    prog.keyframes_reserve(len(KEYFRAMES))
    prog.keyframes_insert([(f, e, f, 0) for e, f in enumerate(KEYFRAMES)])  # user[0]: the source frame, carried along
    for e in range(len(KEYFRAMES)):
        head = prog.keyframes_read(e, 0)[0]
        print("slot %d: frame %d, %d keypoints, %d with a landmark, status %d" % (e, head["frame"], head["keypoints"], head["points"], head["status"]))

    # --- the second batch: database hits, matched and localised against the store ------------------------------
    prog.extract_batch_host(views[B:])
    prog.place_frames(B, db=db, min_gap=B)                          # min_gap = B: no candidates inside the batch, the database only
    rows = prog.place_read(0, B)
    hits = [(q, int(g) & ~orb.ORB_PLACE_DB) for q in range(B) for g in rows[q]["best"]["frame"][:int(rows[q]["n"])] if int(g) & orb.ORB_PLACE_DB]
    print("%d database hits for %d frames" % (len(hits), B))
    if not hits:
        sys.exit(0)
    prog.match_keyframes(hits)                                      # needs the batch and the store, no stage
    prog.localize_keyframes(len(hits), max_reproj_px=1e6, **intr)
    names = {orb.ORB_LOCALIZE_OK: "OK", orb.ORB_LOCALIZE_NOMAP: "NOMAP", orb.ORB_LOCALIZE_FEW: "FEW", orb.ORB_LOCALIZE_DEGENERATE: "DEGENERATE",
             orb.ORB_LOCALIZE_MINIMAL: "MINIMAL"}
    for i, (q, e) in enumerate(hits):
        fix, inliers = prog.localize_keyframes_read(i)
        print("frame %d against slot %d (frame %d of the first batch): %s, %d candidates, %d inliers, t = %s in units of segment %d" %
              (q, e, KEYFRAMES[e], names[int(fix["status"])], fix["candidates"], fix["inliers"], np.round(fix["t"], 3), fix["origin"]))
