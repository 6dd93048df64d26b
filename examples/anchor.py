#!/usr/bin/env python3
"""A second batch's path in the map of the first (needs an MI355X; build first: python -m tinyslam_amd.build).

    python examples/anchor.py

The two batches of examples/relocalize.py: the first is run through the map chain and four of its frames become keyframes of the
program's store; the second is extracted over it, run through the same chain -- its trajectory and landmarks are in a frame and a
unit of its own --, and its database hits are matched and localised against the store.  orb_anchor_frames
then takes, for every segment of the second batch, the entry whose depth ratios agree best, and writes the segment's frames and
landmarks in the frame and unit of that keyframe's segment: the second batch's path in the first map.

The views are near-planar warps of one image, not a camera's motion, so the chain runs with the permissive parameters of
tools/loop_rate.py; the verdicts say how the stage judges such views, the calls are what is shown.
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


def chain(prog):
    """Match, epipolar verification, pose, trajectory, landmarks of the batch the program holds."""
    prog.match_consecutive(B)
    prog.verify_epipolar(B)
    prog.pose_consecutive(B, max_reproj_px=1e6, min_good=1, ambiguity_permille=1000, **intr)
    prog.trajectory_consecutive(B, min_shared=1, scale_tolerance=1e6, consistent_permille=1)
    prog.landmarks_consecutive(B, max_reproj_px=1e6, **intr)


with orb.OrbProgram(cfg) as prog:
    # --- the first batch: a map, signatures, keyframes ---------------------------------------------------------
    prog.extract_batch_host(views[:B])
    chain(prog)
    prog.place_frames(B)
    db = np.stack([prog.place_signature(f) for f in KEYFRAMES])
    prog.keyframes_reserve(len(KEYFRAMES))
    prog.keyframes_insert([(f, e, f, 0) for e, f in enumerate(KEYFRAMES)])

    # --- the second batch: its own map, then the database hits against the store -------------------------------
    prog.extract_batch_host(views[B:])
    chain(prog)                                                     # orb_anchor_frames needs the batch's own trajectory and landmarks
    prog.place_frames(B, db=db, min_gap=B)
    rows = prog.place_read(0, B)
    hits = [(q, int(g) & ~orb.ORB_PLACE_DB) for q in range(B) for g in rows[q]["best"]["frame"][:int(rows[q]["n"])] if int(g) & orb.ORB_PLACE_DB]
    print("%d database hits for %d frames" % (len(hits), B))
    if not hits:
        sys.exit(0)
    prog.match_keyframes(hits)
    prog.localize_keyframes(len(hits), max_reproj_px=1e6, **intr)

    # --- the anchor: every segment of the second batch under one keyframe's segment ----------------------------
    prog.anchor_frames(len(hits), min_shared=1, scale_tolerance=1e6, consistent_permille=1, flags=orb.ORB_ANCHOR_USE_MINIMAL)
    verdicts = ("HOLDS", "STATUS", "FEW", "RANGE", "NONFINITE", "RATIO_FEW", "RATIO_SPREAD")
    for i, link in enumerate(prog.anchor_links(len(hits))):
        print("entry %d, frame %d against slot %d: %s, %d ratios, %d consistent, gamma %.4f%s" %
              (i, hits[i][0], link["slot"], verdicts[int(link["verdict"])], link["shared"], link["consistent"], link["gamma"], " (chosen)" if link["chosen"] else ""))
    for b, seg in enumerate(prog.anchor_segments(B)):
        if seg["status"] == orb.ORB_ANCHOR_SEGMENT_ANCHORED:
            print("segment %d hangs under slot %d (frame %d of the first batch, segment %d there): one unit is %.4f of the map's" %
                  (b, seg["slot"], seg["user"][0], seg["map_origin"], seg["gamma"]))
    for f in range(B):
        pose = prog.anchor_read(f)
        R, t = pose["r"].reshape(3, 3).astype(np.float64), pose["t"].astype(np.float64)
        where = "in the first map" if pose["status"] == orb.ORB_ANCHOR_ANCHORED else "in its own segment (no entry held)"
        print("frame %d: camera centre %s %s" % (f, np.round(-R.T @ t, 3), where))
    moved = sum(int(prog.anchor_landmarks(p, 0)[0]["moved"]) for p in range(B - 1))
    print("%d landmarks of the second batch written in the first map's frame" % moved)
