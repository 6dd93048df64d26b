"""Hand-built inputs of the remap stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_remap_frames reads the trajectory's frame records, the landmark records and rows, the graph stage's
poses and the join stage's segment records, so a case is a join_cases / graph_cases case carried through those two stages.
`anchored` is the rail camera under a plan whose second segment the graph refines and the join links, with landmarks that begin at
the root's origin, at a HELD frame and at a moved frame.  `sources`, `check` and `program` drive a device program; `reference`
carries a case through the restatements.
"""
import numpy as np

import graph_cases as G
import graph_ref as gr
import join_cases as J
import landmark_cases as L
import remap_ref as rr
from tinyslam_amd import orb

NONE = 0xFFFFFFFF
GRAPH, JOIN = orb.ORB_REMAP_GRAPH, orb.ORB_REMAP_JOIN
FROM_GRAPH, MOVED = orb.ORB_REMAP_FROM_GRAPH, orb.ORB_REMAP_MOVED
FLAGS = (0, GRAPH, JOIN, GRAPH | JOIN)
program = J.program
load, load_rail = J.load, J.load_rail

# segment 0: frames 0, 1; frame 2 is LOST (HELD by the graph) and the origin of frames 3 .. 5, which the graph moves
ANCHOR_PLAN = [L.ORIGIN, L.START, L.LOST, L.START, L.CHAINED, L.CHAINED]
ANCHOR_GRAPH_PAIRS = [(5, 2), (4, 2)]
ANCHOR_JOIN_PAIRS = [(4, 1), (5, 0)]
ANCHOR_PAIRS = ANCHOR_GRAPH_PAIRS + ANCHOR_JOIN_PAIRS
ANCHOR_LATE = (0, 1, 2)   # these landmarks of segment 2 begin at frame 3
ANCHOR_LM = dict(max_reproj_px=1000.0)  # the cameras have drifted: every chain is GOOD all the same


def anchored(cap=16, K_=12):
    """(batch, list, fixes, masks): the rail camera under ANCHOR_PLAN.  Segment 2's frame records are graph_cases.drifted ones of the
    rail's true cameras; entries 0, 1 are its true loop fixes, entries 2, 3 the true fixes that link it to segment 0.  The landmarks
    ANCHOR_LATE have no match and no point in pair 2, so their chain in segment 2 begins in pair 3, at a frame the graph moves."""
    b = L.rail(6, K_, cap=cap, plan=ANCHOR_PLAN, v_hi=L.V_HI)
    s = b["slots"][2][list(ANCHOR_LATE)]
    b["matches"]["index"][2, s] = L.NONE
    b["points"][2, s] = 0
    step = (-L.RAIL_BASE, 0.0, 0.0)
    true = G.line(4, step=step, turn=0.0)
    b["frames"] = np.concatenate([G.frames_of(G.line(2, step=step, turn=0.0)), G.frames_of(G.drifted(true), origin=2, first=2)])
    b["scales"] = {}
    assert b["frames"]["origin"].tolist() == [0, 0, 2, 2, 2, 2] and b["frames"]["status"].tolist() == ANCHOR_PLAN
    fixes = np.concatenate([G.fixes_of(true, ANCHOR_GRAPH_PAIRS, origin=2, first=2), J.fixes(b, ANCHOR_JOIN_PAIRS)])
    masks = np.array([J.mask(b, q) for q, _ in ANCHOR_PAIRS])
    return b, list(ANCHOR_PAIRS), fixes, masks


def reference(b, lms, pairs, fixes=None, masks=None, frames=None, flags=0, graph=None, join=None):
    """A rail batch and its landmark records through graph_ref, join_ref and remap_ref.  Returns (graph poses, segments, links,
    (remap poses, rows, landmarks))."""
    fr = b["frames"] if frames is None else frames
    fx = J.fixes(b, pairs, frames=fr) if fixes is None else fixes
    gp, _ = gr.graph_pairs(fr, pairs, fx, **(graph or {}))
    _, segs, links = J.run(b, lms, pairs, fx=fx, masks=masks, frames=fr, **(join or {}))
    lrows = L.rows_from(np.array(lms), [origin_of_pair(fr, p) for p in range(len(lms))])
    return gp, segs, links, rr.remap_frames(fr, lrows, lms, gp, segs, flags=flags)


def origin_of_pair(frames, p):
    """LM-6: the row's origin, 0xffffffff when frame p + 1 is LOST."""
    return NONE if int(frames["status"][p + 1]) == L.LOST else int(frames["origin"][p + 1])


def sources(prog, inp, flags=0):
    """What a remap call reads, as the device holds it now: (frames, landmark rows, landmarks, graph poses, segments); a source that
    `flags` does not name is None."""
    nF = len(inp.frames)
    g, j = rr.sources(flags)
    frames = np.array([prog.trajectory_read(f, 0)[0] for f in range(nF)])
    pairs = min(inp.L - 1, nF - 1)
    lm = [prog.landmarks_read(p, inp.cap) for p in range(pairs)]
    gp = np.array([prog.graph_read(f) for f in range(nF)]) if g else None
    sg = prog.join_segments(nF) if j else None
    return frames, np.array([r for r, _ in lm]), [l for _, l in lm], gp, sg


def check(prog, inp, flags=0, stream=None, call=True, held=None):
    """remap_frames (call=False: the last one's results), then all three outputs against the restatement fed with what the device
    holds (`held`: what it held when the call was made), byte for byte.  Returns (poses, rows, landmarks, the bytes of all three)."""
    src = sources(prog, inp, flags) if held is None else held
    if call:
        prog.remap_frames(flags, stream=stream)
    want = rr.remap_frames(*src, flags=flags)
    nF, pairs = len(src[0]), len(want[1])
    poses = np.array([prog.remap_read(f) for f in range(nF)])
    got = [prog.remap_landmarks(p, inp.cap) for p in range(pairs)]
    rows, lms = np.array([r for r, _ in got]), [l for _, l in got]
    for f in range(nF):
        assert poses[f].tobytes() == want[0][f].tobytes(), ("pose", f, flags, poses[f], want[0][f])
    for p in range(pairs):
        assert rows[p].tobytes() == want[1][p].tobytes(), ("row", p, flags, rows[p], want[1][p])
        bad = np.nonzero(lms[p] != want[2][p])[0] if lms[p].tobytes() != want[2][p].tobytes() else []
        assert lms[p].tobytes() == want[2][p].tobytes(), ("landmarks", p, flags, bad[:4], lms[p][bad[:4]], want[2][p][bad[:4]])
    assert pairs == 0 or prog.remap_landmarks(pairs - 1, 0)[0].tobytes() == rows[-1].tobytes()  # the row alone
    return poses, rows, lms, poses.tobytes() + rows.tobytes() + b"".join(l.tobytes() for l in lms)
