"""The stages behind extraction on extracted views, on the GPU: pixels -> extraction -> match -> verify_epipolar -> pose -> trajectory
-> localize -> landmarks -> bridge -> adjust on tests/layered_views.py's scenes (two textured planes, a camera moving sideways), every
stage's read-back against the chained CPU restatements fed with the device's own counters, records and descriptors in the device's
own order, byte for byte.  No stage's inputs are written by the test: descriptors that went through the matcher, counts of 504 to
616 that differ from frame to frame, the matcher's many-to-one records, the pose stage's own GOOD flags.

Every test: (1) extraction equals the oracle's as a sorted set; (2) every stage equals the chain of restatements; (3) the device's
records show the stages at work (the conditions tests/test_layered_chain_ref.py holds under 17 orders of the records); (4) the calls
from match_consecutive on, made again on the same batch, leave the same bytes.  Intended mode with the oracle's settings (arc 9,
non-maximum suppression, depth 2, threshold 20/255)."""
import time

import numpy as np
import pytest

import landmark_cases as L
import layered_views as lv
import trajectory_cases as tc

pytestmark = pytest.mark.gpu

POISON = 0xA5


def _program(tinyorb, cap, max_batch):
    T = tinyorb
    cfg = T.OrbConfig(T.Extent3d(lv.W0, lv.H0), max_features=cap, hierarchy_depth=2, initial_threshold=lv.THR, max_batch=max_batch,
                      flags=T.ORB_FLAG_INTENDED | T.ORB_FLAG_NMS, fast_arc=9)
    return T.OrbProgram(cfg).init()


def _extract(prog, oracle, name):
    """Step 1: the scene's frames through extract_batch_host; the raw counters are the oracle's and the stored records, as a sorted
    set, are the oracle's (below the capacity) or a subset of them with equal descriptors (above it: IM-8's cut).  Returns (scene,
    n, the device's (counters, records, descriptors))."""
    s = lv.scene(oracle, name)
    n, cap = len(s["frames"]), s["cap"]
    prog.extract_batch_host(s["frames"])
    counts, corners, desc = lv.device_records(prog, n, cap)
    wcounts, wcor, wdesc = s["whole"]
    assert counts.tolist() == wcounts.tolist(), (counts, wcounts)
    for f in range(n):
        assert len(corners[f]) == min(int(counts[f]), cap)
        c, d = oracle.sort_keypoints(corners[f], desc[f])
        if counts[f] <= cap:
            assert np.array_equal(c, wcor[f]), "records of frame %d" % f
            assert np.array_equal(d, wdesc[f]), "descriptors of frame %d" % f
        else:
            have = {a.tobytes(): b.tobytes() for a, b in zip(wcor[f], wdesc[f])}
            assert len({a.tobytes() for a in c}) == cap, "frame %d stores a record twice" % f
            for a, b in zip(c, d):
                assert have.get(a.tobytes()) == b.tobytes(), "frame %d: record %s" % (f, a)
    return s, n, (counts, corners, desc)


def _parity(prog, n, batch, cap, intr=lv.INTR, first="match", prior=None, **stage):
    """Step 2: the calls from `first` on, every read-back against the restatements chained on the device's records."""
    got = lv.device_chain(prog, n, intr, first=first, **stage)
    want = lv.chain(*batch, lv.W0, lv.H0, cap, intr, n_frames=n, first=first, prior=prior, **stage)
    d = lv.differences(got, want)
    assert d is None, d
    return got, want


def _repeat(prog, n, got):
    """Step 4."""
    again = lv.device_chain(prog, n, lv.INTR)
    d = lv.differences(again, got)
    assert d is None, "second run against the first: " + d
    assert lv.blob(again) == lv.blob(got)


def _show(name, res, t0):
    for k, v in lv.summary(res).items():
        print("  %s %s: %s" % (name, k, v))
    print("%s: %.2f s" % (name, time.perf_counter() - t0))


def _poison_behind(prog, n):
    """Bytes of 0xA5 over the rows of frames n .. max_batch - 1 in the buffers a test can reach (match records, pose records,
    points, frame records): no call on n frames reads or writes them."""
    from tinyslam_amd import orb
    cfg = prog.config
    k, cap = cfg.max_batch - n, cfg.max_features

    def fill(shape, dtype):
        return np.full(int(np.prod(shape)) * dtype.itemsize, POISON, np.uint8).view(dtype).reshape(shape)

    tc.inject_pose(prog, fill((k, cap), orb.MATCH_DTYPE), fill((k,), orb.POSE_DTYPE), fill((k, cap), orb.POINT_DTYPE), first=n)
    L.inject_frames(prog, fill((k,), orb.FRAME_POSE_DTYPE), first=n)


def _behind(prog, n):
    """The bytes of rows n .. max_batch - 1 of the seven buffers a test can reach: the extraction's counters, records and
    descriptors, the match records, pose records, points and frame records."""
    import torch
    from tinyslam_amd import node
    cfg = prog.config
    B, cap = cfg.max_batch, cfg.max_features
    dev = torch.device("cuda", cfg.device)
    prog.batch_sync()
    torch.cuda.synchronize(dev)
    d_counts, d_corners, d_desc = prog.batch_device_buffers()
    d_m, d_p, d_x = prog.debug_pose_buffers()
    out = []
    for addr, words in ((d_counts, 1), (d_corners, cap * 4), (d_desc, cap * 8), (d_m, cap * 2), (d_p, 16), (d_x, cap * 4),
                        (prog.debug_frame_buffer(), 20)):
        out.append(node.as_tensor(addr, (B, words), "<i4", dev)[n:].cpu().numpy().tobytes())
    return out


def test_roomy(tinyorb, oracle):
    """Variant a: nine frames at capacity 1500 in a program of twelve, so rows behind the batch exist: they are marked between the
    two runs of the chain and found unchanged after the second."""
    T = tinyorb
    t0 = time.perf_counter()
    with _program(T, lv.ROOMY, 12) as prog:
        s, n, batch = _extract(prog, oracle, "roomy")
        assert n == 9 and (batch[0] < lv.ROOMY).all() and all(c % 64 for c in batch[0])
        got, _ = _parity(prog, n, batch, lv.ROOMY)
        _show("roomy", got, t0)
        lv.check_roomy(got)
        dev = lv.step_deviations(got, s["truth"])
        print("roomy: step deviations of the OK fixes", dev)
        # the stages' buffers exist from their first call on: the rows behind the batch are marked between the two runs
        _poison_behind(prog, n)
        behind = _behind(prog, n)
        assert behind[3] == bytes([POISON]) * len(behind[3]) and behind[6] == bytes([POISON]) * len(behind[6])
        _repeat(prog, n, got)
        names = ("counters", "records", "descriptors", "match records", "pose records", "points", "frame records")
        for name, a, b in zip(names, behind, _behind(prog, n)):
            assert a == b, "rows behind the batch: " + name
    print("roomy: %.2f s" % (time.perf_counter() - t0))


def test_every_frame_over_capacity(tinyorb, oracle):
    """Variant b: the same views at capacity 512, below every frame's raw counter (527 to 616)."""
    T = tinyorb
    t0 = time.perf_counter()
    with _program(T, lv.FULL, 9) as prog:
        s, n, batch = _extract(prog, oracle, "full")
        assert (batch[0] > lv.FULL).all() and all(len(c) == lv.FULL for c in batch[1]), batch[0]
        got, _ = _parity(prog, n, batch, lv.FULL)
        _show("full", got, t0)
        assert (got["nq"] == lv.FULL).all()
        lv.check_full(got)
        _repeat(prog, n, got)
    print("full: %.2f s" % (time.perf_counter() - t0))


def test_empty_frame_inside(tinyorb, oracle):
    """Variant c: frame 4 of nine is a constant grey: a raw counter of 0 out of extraction, in the middle of the batch."""
    T = tinyorb
    t0 = time.perf_counter()
    e = lv.EMPTY
    with _program(T, lv.ROOMY, 9) as prog:
        s, n, batch = _extract(prog, oracle, "empty")
        assert batch[0][e] == 0 and (np.delete(batch[0], e) > 400).all(), batch[0]
        got, _ = _parity(prog, n, batch, lv.ROOMY)
        _show("empty", got, t0)
        lv.check_empty(got, e)
        assert got["bridge"]["status"][e] == T.ORB_BRIDGE_UNFIXED and got["adjusted"]["status"][e] == T.ORB_ADJUST_HELD
        _repeat(prog, n, got)
    print("empty: %.2f s" % (time.perf_counter() - t0))


# variant d: (what, intrinsics, first stage called again, n_frames (None: the batch), per-stage parameters)
def _late(reproj, hyps, rounds):
    return dict(localize=dict(max_reproj_px=reproj, hypotheses=hyps), landmarks=dict(max_reproj_px=reproj),
                bridge=dict(max_reproj_px=reproj, hypotheses=hyps), adjust=dict(max_reproj_px=reproj, rounds=rounds))


# in this order: a localize call needs the trajectory of the whole batch, and every stage reads the pose stage's intrinsics
PARAMETERS = [("0.5 px, one hypothesis, one round", lv.INTR, "localize", None, _late(0.5, 1, 1)),
              ("1000 px, 65 hypotheses, 16 rounds", lv.INTR, "localize", None, _late(1000.0, 65, 16)),
              ("three frames", lv.INTR, "trajectory", 3, {}),
              ("intrinsics off the centre, fx != fy", lv.INTR_OFF, "pose", None, {})]


def test_other_parameters_on_the_roomy_batch(tinyorb, oracle):
    """Variant d: one extraction, then the later stages under other intrinsics, thresholds, hypothesis counts, rounds and extents,
    each against the restatements; the defaults on the whole batch again give the first run's bytes."""
    T = tinyorb
    t0 = time.perf_counter()
    with _program(T, lv.ROOMY, 9) as prog:
        s, n, batch = _extract(prog, oracle, "roomy")
        base, want = _parity(prog, n, batch, lv.ROOMY)
        for what, intr, first, frames, stage in PARAMETERS:
            t1 = time.perf_counter()
            k = frames or n
            # the stages before `first` are not called again: the restatements take the first run's for them
            got, _ = _parity(prog, k, batch, lv.ROOMY, intr=intr, first=first, prior=want, **stage)
            assert frames or lv.differences(got, base) is not None, what  # the parameters moved something
            print("%s: fixes %s, landmarks GOOD %s, bridge %s, adjusted %s, %.2f s" % (
                what, got["fix"]["status"].tolist(), lv.summary(got)["landmarks_good"], got["bridge"]["status"].tolist(),
                got["adjusted"]["status"].tolist(), time.perf_counter() - t1))
            if frames:
                with pytest.raises(T.OrbError) as err:
                    prog.adjust_read(frames, lv.ROOMY)
                assert err.value.code == T.ORB_EINVAL
        again = lv.device_chain(prog, n, lv.INTR, first="pose")
        d = lv.differences(again, base)
        assert d is None, "the defaults again: " + d
    print("parameters: %.2f s" % (time.perf_counter() - t0))
