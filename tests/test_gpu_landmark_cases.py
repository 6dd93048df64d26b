"""The hand-built cases of tests/landmark_cases.py (`cases`) on the GPU: orb_landmarks_consecutive fed through the debug accessors --
counters and keypoint records (orb_batch_device_buffers), match records and points (orb_debug_pose_buffers), frame records
(orb_debug_frame_buffer) -- every OrbLandmarkRow and every one of the capacity's OrbLandmark records of every pair against the CPU
restatement (tests/landmark_ref.py) fed with what the device holds, byte for byte, and then the outcome each construction implies on
the device's own records.  No tolerance anywhere.

The images are zeros at 64 x 48 with two levels: the match, epipolar and pose stages run once on empty frames and the trajectory
stage once on what they left, only to be fresh; what the landmarks call reads is then written over their buffers.  The stage reads
no image, and the rail's keypoints stay inside such a frame (landmark_cases.V_HI).  One program per capacity, every case of that
capacity on it in turn, so the stage's own buffers -- the predecessor bytes, the rows, the records -- carry from case to case."""
import time

import numpy as np
import pytest

import constructed as C
import landmark_cases as L
import landmark_ref as lmr
import trajectory_cases as tc

pytestmark = pytest.mark.gpu

W0, H0 = 64, 48
MAX_BATCH = 6
CASES = L.cases()
CAPS = sorted({c["cap"] for c in CASES})  # every case has one of them, so the capacities' counts add up to len(CASES)
assert CAPS == [L.SMALL, 64, 256, 257, 1100] and len(CASES) == 30


def _program(tinyorb, cap):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=MAX_BATCH)
    return tinyorb.OrbProgram(cfg).init()


def _load(prog, b):
    """The batch over the program's buffers, with every stage the landmarks call needs fresh."""
    n = b["n"]
    tc.prepare(prog, n, W0, H0)
    C.inject(prog, b["counts"], b["corners"])
    tc.inject_pose(prog, matches=b["matches"], points_=b["points"])  # the rail has no pose records and the stage reads none
    prog.trajectory_consecutive(n)  # fresh; its records are overwritten before every call


def _inputs(prog, n_frames, cap):
    """What the call reads, as the device holds it."""
    counts = np.minimum(prog.batch_counts(n_frames), cap).astype(np.int64)
    corners = [prog.batch_read(f, int(counts[f]))[0] for f in range(n_frames)]
    matches = [prog.match_read(f, int(counts[f])) for f in range(n_frames - 1)]
    points = [prog.pose_read(f, cap)[1] for f in range(n_frames - 1)]
    frames = np.array([prog.trajectory_read(f, 0)[0] for f in range(n_frames)])
    return counts, corners, matches, points, frames


def _call(prog, k, cap):
    """One call of a case: the frame records in, the call, every byte against the restatement of the device's inputs.  Returns the
    device's (records (n_frames - 1, cap), rows (n_frames - 1,))."""
    b, n = k["batch"], k["n_frames"]
    L.inject_frames(prog, k["frames"])
    counts, corners, matches, points, frames = _inputs(prog, b["n"], cap)
    assert frames.tobytes() == np.ascontiguousarray(k["frames"]).tobytes()  # orb_trajectory_read returns what was injected
    assert counts.tolist() == np.minimum(b["counts"], cap).tolist() and np.stack(points).tobytes() == b["points"].tobytes()
    prog.landmarks_consecutive(n, **k["intr"], **k["params"])
    want, wrows = lmr.landmarks(counts[:n], corners[:n], matches[:n - 1], points[:n - 1], frames[:n], cap, n_frames=n, **k["intr"], **k["params"])
    got = [prog.landmarks_read(p, cap) for p in range(n - 1)]
    rows, recs = np.array([g[0] for g in got]), np.stack([g[1] for g in got])
    for p in range(n - 1):
        assert rows[p].tobytes() == wrows[p].tobytes(), (p, k["params"], rows[p], wrows[p])
        if recs[p].tobytes() != want[p].tobytes():
            bad = np.nonzero((recs[p].view(np.uint32).reshape(cap, 8) != want[p].view(np.uint32).reshape(cap, 8)).any(1))[0]
            raise AssertionError((p, k["params"], bad[:8], recs[p][bad[:8]], want[p][bad[:8]]))
    return recs, rows


@pytest.mark.parametrize("cap", CAPS)
def test_cases(tinyorb, cap):
    """Capacity 8: the cases of LM-2..LM-6.  64, 256, 257, 1100: every slot a start, in one block of k_lm_fuse's 256 threads a
    quarter full, one exactly full, a second block of one thread, and five blocks of which the last has 76."""
    t0 = time.perf_counter()
    cases = [c for c in CASES if c["cap"] == cap]
    checked = calls = 0
    with _program(tinyorb, cap) as prog:
        held = None
        for c in cases:
            res = []
            for k in c["calls"]:
                if k["batch"] is not held:
                    held = k["batch"]
                    _load(prog, held)
                res.append(_call(prog, k, cap))
                calls += 1
            try:
                c["expect"](res)
            except AssertionError as e:
                raise AssertionError("case %r: %s" % (c["name"], e)) from e
            checked += 1
    assert checked == len(cases) and checked > 0
    print("capacity %d: %d cases, %d calls, %.2f s" % (cap, checked, calls, time.perf_counter() - t0))


def test_the_frame_buffer(tinyorb):
    """orb_debug_frame_buffer: ORB_ESTATE until a trajectory call has allocated the records, a NULL out-pointer allowed, the address
    that of the records orb_trajectory_read copies, and no stage's freshness moved by asking or by writing."""
    t0 = time.perf_counter()
    T = tinyorb
    b = L.rail(4, 6, cap=L.SMALL, v_hi=L.V_HI)
    lib = T.load_library()
    with _program(T, L.SMALL) as prog:
        with pytest.raises(T.OrbError) as e:
            prog.debug_frame_buffer()
        assert e.value.code == T.ORB_ESTATE
        tc.prepare(prog, b["n"], W0, H0)
        with pytest.raises(T.OrbError) as e:
            prog.debug_frame_buffer()  # match and pose have run, the trajectory stage has not
        assert e.value.code == T.ORB_ESTATE
        _load(prog, b)
        assert prog.debug_frame_buffer() and lib.orb_debug_frame_buffer(prog._handle(), None) == T.ORB_OK
        before = np.array([prog.trajectory_read(f, 0)[0] for f in range(b["n"])])
        assert (before["status"][1:] == L.LOST).all()  # the empty frames' pairs are not OK
        L.inject_frames(prog, b["frames"][2:], first=2)
        after = np.array([prog.trajectory_read(f, 0)[0] for f in range(b["n"])])
        assert after[:2].tobytes() == before[:2].tobytes() and after[2:].tobytes() == b["frames"][2:].tobytes()
        prog.landmarks_consecutive(b["n"], **L.RAIL)  # still fresh
        assert prog.landmarks_read(0, 0)[0].tolist() == (0, 0, 0, T.ORB_LANDMARK_NO_ORIGIN)  # frame 1 is still LOST
    print("frame buffer: %.2f s" % (time.perf_counter() - t0))
