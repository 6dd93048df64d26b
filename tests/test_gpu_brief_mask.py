"""GPU parity of the hand-off between the two BRIEF kernels of a batch: k_brief_t leaves one 64-bit word per 64 keypoints of a
frame's final list (bit i: keypoint 64 c + i is NOT flat -- within 18 px of the left border or in the stored tail of the blur
plane), k_brief_nf starts from that word.  The program has no entry that reads the words back, so every case checks them through
what they decide: a keypoint whose bit is wrongly clear keeps the descriptor the buffer held before (zeros, or another batch's) --
records and descriptors against the CPU restatement and against the per-stage pipeline, integers and bit patterns only.  What
this cannot see: a bit wrongly set for a flat keypoint (k_brief_nf then stores the same descriptor again) and a bit set for a slot
at or past the frame's count (a store beyond what a read-back returns); the kernel's predicate (`live && !flat`, zeros from the
workgroups past the count) is what rules those out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
OOB = {"zero": 0, "clamp": 1, "umin": 2}


def _sorted(corners, desc):
    order = np.lexsort((corners["x"], corners["y"], corners["octave"]))
    return corners[order], desc[order]


def _noise(W, H, seed, x0=0, x1=None, density=0.08):
    """White salt on black in columns [x0, x1), black elsewhere: hundreds of FAST corners where the salt is, none elsewhere."""
    rng = np.random.default_rng(seed)
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    x1 = W if x1 is None else x1
    rgba[:, x0:x1, :3] = (rng.random((H, x1 - x0, 1)) < density) * 255
    rgba[..., 3] = 255
    return rgba


def _flat(W, H):
    rgba = np.full((H, W, 4), 128, dtype=np.uint8)
    rgba[..., 3] = 255
    return rgba


def _check(ref, cap, total, corners, desc):
    """One frame against the restatement run WITHOUT a cap.  Up to the cap: the same records and descriptors.  Cut at the cap (the
    device keeps cap records of its own list order): every kept record is one of the restatement's, once, with its descriptor."""
    assert total == ref["total"]
    n = min(total, cap)
    assert len(corners) == n and len(desc) == n
    if total <= cap:
        c, d = _sorted(corners, desc)
        order = np.lexsort((ref["corners"]["x"], ref["corners"]["y"], ref["corners"]["octave"]))
        for k in ("octave", "y", "x", "angle"):
            assert np.array_equal(c[k], ref["corners"][k][order]), k
        assert np.array_equal(d, ref["descriptors"][order]), "descriptors differ"
        return
    full = {(int(c["octave"]), int(c["y"]), int(c["x"])): (int(c["angle"]), d.tobytes()) for c, d in zip(ref["corners"], ref["descriptors"])}
    seen = set()
    for c, d in zip(corners, desc):
        key = (int(c["octave"]), int(c["y"]), int(c["x"]))
        assert key not in seen and full[key] == (int(c["angle"]), d.tobytes()), key
        seen.add(key)


def _ref(oracle, frame, depth, oob="zero"):
    return oracle.extract(frame, depth=depth, threshold=THR, max_features=1 << 16, oob=oob)


def _program(tinyorb, W, H, depth, **kw):
    return tinyorb.OrbProgram(tinyorb.OrbConfig(tinyorb.Extent3d(W, H), hierarchy_depth=depth, initial_threshold=THR, **kw)).init()


def _run_batch(prog, frames, refs, cap, staged=False):
    """One batch against the restatement.  A fused program must have taken the path under test: both BRIEF kernels of the batch
    launched, the wave-per-keypoint fallback (k_brief_rows, for frames too large for k_brief_t's staging) not."""
    assert prog.pipeline() == ("staged" if staged else "fused") and prog.pipeline_note() == ""
    prog.profile_enable()
    prog.profile_reset()
    prog.extract_batch_host(np.stack(frames))
    counts = prog.batch_counts(len(frames))
    launched = prog.profile()
    prog.profile_enable(False)
    if not staged:
        assert "k_brief_t" in launched and "k_brief_nf" in launched and "k_brief_rows" not in launched, sorted(launched)
    for i, r in enumerate(refs):
        c, d = prog.batch_read(i, min(int(counts[i]), cap))
        _check(r, cap, int(counts[i]), c, d)
    return counts


@pytest.mark.parametrize("flags_double", [False, True])
def test_no_stale_bits_between_batches(tinyorb, oracle, flags_double):
    """Many keypoints, then few, then a frame with none among others, on one program and output set: every word is rewritten by
    every batch, so a chunk that held not-flat keypoints in the batch before and holds none (or nothing) now reads zero.  With two
    output sets the batches alternate between them."""
    W, H, depth, cap = 160, 120, 2, 2048
    many = [_noise(W, H, 1), _noise(W, H, 2), _noise(W, H, 3)]
    few = [oracle.synth_frame(W, H, 5), _noise(W, H, 6, 60, 90, 0.02), oracle.synth_frame(W, H, 7)]
    holed = [_noise(W, H, 8), _flat(W, H), _noise(W, H, 9, 16, 18, 0.3)]
    batches = [many, few, holed, many, holed]
    refs = {id(b): [_ref(oracle, f, depth) for f in b] for b in batches}
    assert min(r["total"] for r in refs[id(many)]) > 4 * max(r["total"] for r in refs[id(few)]) > 0
    assert refs[id(holed)][1]["total"] == 0 < refs[id(holed)][2]["total"]
    flags = tinyorb.ORB_FLAG_DOUBLE_OUTPUT if flags_double else 0
    with _program(tinyorb, W, H, depth, max_batch=3, max_features=cap, flags=flags) as prog:
        for i, b in enumerate(batches):
            if flags_double:
                prog.batch_select_output(i & 1)
            _run_batch(prog, b, refs[id(b)], cap)
        if flags_double:  # set 0 still holds its last batch (`holed`, i = 4) after set 1 was written in between
            prog.batch_select_output(1)
            _run_batch(prog, few, refs[id(few)], cap)
            prog.batch_select_output(0)
            counts = prog.batch_counts(3)
            for i, r in enumerate(refs[id(holed)]):
                c, d = prog.batch_read(i, min(int(counts[i]), cap))
                _check(r, cap, int(counts[i]), c, d)


@pytest.mark.parametrize("cap", [100, 128, 130, 256, 300])
def test_counts_that_straddle_the_cap_and_the_chunk(tinyorb, oracle, cap):
    """Caps that are no multiple of 64 (100, 130, 300), of 256 (128), and exactly one workgroup of k_brief_t (256), on frames with
    more keypoints than the cap (cut inside a chunk: the lanes past the count leave zero bits) and with fewer (the last wave of the
    last workgroup is part empty; the chunks behind it are zero words)."""
    W, H, depth = 160, 120, 2
    frames = [_noise(W, H, 11), oracle.synth_frame(W, H, 12), _noise(W, H, 13, 0, 40, 0.03)]
    refs = [_ref(oracle, f, depth) for f in frames]
    assert refs[0]["total"] > 300 and 0 < min(r["total"] for r in refs[1:])
    with _program(tinyorb, W, H, depth, max_batch=3, max_features=cap) as prog:
        _run_batch(prog, frames, refs, cap)
        _run_batch(prog, frames[::-1], refs[::-1], cap)


def test_population_extremes(tinyorb, oracle):
    """Frames whose keypoints are ALL within 18 px of the left border (FAST starts at column 17: one column of them, more than
    four to a chunk, so a wave takes several turns), all in the stored tail on the right, all one or the other (every bit of every
    word set: whole chunks of 64 not-flat keypoints, a wave takes sixteen turns), and none of either (every word zero)."""
    W, H, depth, cap = 160, 120, 2, 2048
    left, right, mid = _noise(W, H, 21, 16, 18, 0.3), _noise(W, H, 22, 132, W, 0.2), _noise(W, H, 23, 46, 92, 0.1)
    both = np.maximum(left, right)
    frames = [left, right, both, mid]
    refs = [_ref(oracle, f, depth) for f in frames]
    lw = [W >> o for o in range(depth)]
    is_left = lambda c: c["x"] < 18
    is_tail = lambda c: c["x"] >= (8 * lw[c["octave"]]) // 10  # the plane's constant part ends at 88 % of a row, flat at 18 less
    assert refs[0]["total"] >= 16 and all(is_left(c) for c in refs[0]["corners"])
    assert refs[1]["total"] >= 100 and all(is_tail(c) for c in refs[1]["corners"])
    assert refs[2]["total"] >= 130 and all(is_left(c) or is_tail(c) for c in refs[2]["corners"])
    # between the left margin and 60 % of the level's width: flat
    assert refs[3]["total"] >= 130 and all(18 <= c["x"] < (6 * lw[c["octave"]]) // 10 for c in refs[3]["corners"])
    with _program(tinyorb, W, H, depth, max_batch=4, max_features=cap) as prog:
        _run_batch(prog, frames, refs, cap)
        _run_batch(prog, frames[::-1], refs[::-1], cap)
    with _program(tinyorb, W, H, depth, max_batch=4, max_features=cap, flags=tinyorb.ORB_FLAG_STAGED) as staged:
        _run_batch(staged, frames, refs, cap, staged=True)


@pytest.mark.parametrize("W,H,depth", [(160, 120, 1), (160, 120, 2), (160, 120, 3), (200, 97, 3), (202, 98, 2), (320, 240, 4)])
@pytest.mark.parametrize("oob", ["zero", "clamp", "umin"])
def test_widths_depths_and_policies(tinyorb, oracle, W, H, depth, oob):
    """Depth 1 and 2 (the level's constants by a scalar select between kernel arguments) and 3, 4 (the LDS table), even widths, odd
    ones (200x97 depth 3: levels of 100 and 50 and an odd row count; 202: level 1 is 101 wide, the gather path) and every
    out-of-level policy; B = 3 with differing counts, B = 1, the six-call single-frame path on the same frames, and the per-stage
    pipeline."""
    frames = [oracle.synth_frame(W, H, 31), _noise(W, H, 32), _noise(W, H, 33, 0, 30, 0.05)]
    refs = [_ref(oracle, f, depth, oob) for f in frames]
    assert len({r["total"] for r in refs}) == 3 and min(r["total"] for r in refs) > 0
    cap = 8192
    outs = []
    with _program(tinyorb, W, H, depth, max_batch=3, oob_policy=OOB[oob]) as prog:
        _run_batch(prog, frames, refs, cap)
        for i in range(3):
            outs.append(_sorted(*prog.batch_read(i, refs[i]["total"])))
        _run_batch(prog, frames[1:2], refs[1:2], cap)  # B = 1 on the same program
    with _program(tinyorb, W, H, depth, oob_policy=OOB[oob]) as one:  # the single-frame call: untouched by the mask
        assert one.pipeline() == "fused" and one.pipeline_note() == ""
        for f, r, (c0, d0) in zip(frames, refs, outs):
            total, corners, desc = one.extract(f)
            _check(r, cap, total, corners, desc)
            c, d = _sorted(corners, desc)
            assert np.array_equal(c, c0) and np.array_equal(d, d0)
    if oob == "zero":
        with _program(tinyorb, W, H, depth, max_batch=3, flags=tinyorb.ORB_FLAG_STAGED) as staged:
            assert staged.pipeline() == "staged"
            staged.extract_batch_host(np.stack(frames))
            for i in range(3):
                c, d = _sorted(*staged.batch_read(i, refs[i]["total"]))
                assert np.array_equal(c, outs[i][0]) and np.array_equal(d, outs[i][1])
