"""k_front's instances with a compile-time geometry (csrc/orb_kernels_front.h, FrontGeo720pL0 / FrontGeo720pL1) against the generic
instances and the oracle.  The 1280x720, depth-2, literal, RGBA batch program takes the specialised instances at both levels; with
TINYORB_FRONT_GENERIC=1 it takes the generic ones, and the two agree bit for bit; every near miss -- another width or height, another
depth, another band height, Y8 input, a program of one frame -- takes the generic instances and equals the oracle.  Each case runs in a
fresh child process (the environment is read when a program is created; a child's stderr carries its TINYORB_FRONT_TRACE lines)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 21  # above the pixels of both levels: no frame, not even noise, loses a record to the capacity
SEED0 = 1000   # bench.py's
# bench.py's --content: (synthetic-frame flags, FAST threshold in 1/255)
CONTENT = {"flat": (1, 20), "default": (15, 20), "dense": (15, 16), "overflow": (15, 8)}
BATCH = 8      # a multiple of 8, as the headline's 256: the workgroups of a frame stay on one XCD (FrontGeom::xcd_swizzle)


def make_frames(oracle, W, H, content, n, y8=False):
    """n - 1 synthetic frames of the bench's content and one frame of bytes from a seeded generator."""
    flags, _ = CONTENT[content]
    synth = oracle.synth_frame_y8 if y8 else oracle.synth_frame
    frames = [synth(W, H, SEED0 + i, flags) for i in range(max(n - 1, 1))]
    if n > 1:
        rng = np.random.default_rng(W * 10007 + H)
        frames.append(rng.integers(0, 256, size=frames[0].shape, dtype=np.uint8))
    return np.stack(frames[:n])


def _child(spec_json, out_path):
    """Runs one case and stores what the frames gave: counters, the planes, records and descriptors in (octave, y, x) order."""
    sys.path.insert(0, ROOT)
    from oracle import orb_oracle as oracle
    from tinyslam_amd import orb
    oracle.build()
    c = json.loads(spec_json)
    W, H, depth, n, y8 = c["W"], c["H"], c["depth"], c["n"], c["y8"]
    frames = make_frames(oracle, W, H, c["content"], n, y8)
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=CAP, hierarchy_depth=depth, initial_threshold=CONTENT[c["content"]][1] / 255.0,
                        max_batch=c["max_batch"], flags=orb.ORB_FLAG_INPUT_Y8 if y8 else 0)
    out = {}
    with orb.OrbProgram(cfg).init() as prog:
        assert prog.pipeline() == "fused", prog.pipeline()
        for i in range(n):
            if c["max_batch"] == 1:  # a program of one frame: frame by frame
                prog.extract_batch_host(frames[i:i + 1])
                f = 0
            elif i == 0:
                prog.extract_batch_host(frames)
                f = 0
            else:
                f = i
            count = int(prog.batch_counts(f + 1)[f])
            assert count <= CAP
            corners, desc = prog.batch_read(f, count)
            order = np.lexsort((corners["x"], corners["y"], corners["octave"]))
            out["count%d" % i] = np.uint32(count)
            out["corners%d" % i] = corners[order]
            out["desc%d" % i] = desc[order]
            for m in range(depth):
                if m > 0:  # the fused path keeps level 0's grey in LDS
                    out["gray%d_%d" % (i, m)] = prog.read_plane(orb.ORB_PLANE_GRAY, m, frame=f)
                out["blur%d_%d" % (i, m)] = prog.read_plane(orb.ORB_PLANE_BLUR, m, frame=f)  # row constants and the stored tail
    np.savez(out_path, **out)


def run_case(tmp_path, name, W=1280, H=720, depth=2, content="default", n=BATCH, max_batch=BATCH, y8=False, env=None):
    """-> (what each level's trace line says it took, the child's results)"""
    out_path = str(tmp_path / (name + ".npz"))
    spec = dict(W=W, H=H, depth=depth, content=content, n=n, max_batch=max_batch, y8=y8)
    e = dict(os.environ)
    e.pop("TINYORB_FRONT_GENERIC", None)
    e.pop("TINYORB_BAND_ROWS", None)
    e["TINYORB_FRONT_TRACE"] = "1"
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(spec), out_path], env=e, cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, "child %s failed (%d):\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    took = {}
    for m in re.finditer(r"tinyorb: k_front level (\d+) .* takes the (\S+)(?: \S+)? instance", r.stderr):
        took[int(m.group(1))] = m.group(2)
    assert sorted(took) == list(range(depth)), "no trace line for every level:\n" + r.stderr[-2000:]
    return took, dict(np.load(out_path))


def assert_same(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k]), k


def assert_equals_oracle(oracle, got, W, H, depth, content, n, y8=False):
    frames = make_frames(oracle, W, H, content, n, y8)
    thr = CONTENT[content][1] / 255.0
    dims, _ = oracle.level_dims(W, H, depth)
    for i in range(n):
        if y8:
            ref = oracle.extract_y8(frames[i], depth=depth, threshold=thr, max_features=CAP, planes=True)
        else:
            ref = oracle.extract(frames[i], depth=depth, threshold=thr, max_features=CAP, planes=True)
        assert int(got["count%d" % i]) == ref["total"], "count of frame %d" % i
        rc, rd = oracle.sort_keypoints(ref["corners"], ref["descriptors"])
        c = got["corners%d" % i]
        assert len(c) == len(rc)
        for k in ("octave", "y", "x", "angle"):
            assert np.array_equal(c[k], rc[k]), "%s of frame %d" % (k, i)
        assert np.array_equal(got["desc%d" % i], rd), "descriptors of frame %d" % i
        for m, (w, h, off) in enumerate(dims):
            if m > 0:
                assert np.array_equal(got["gray%d_%d" % (i, m)].ravel(), ref["gray"][off:off + w * h]), "gray level %d of frame %d" % (m, i)
            assert np.array_equal(got["blur%d_%d" % (i, m)].ravel(), ref["blur"][off:off + w * h]), "blur level %d of frame %d" % (m, i)


@pytest.mark.parametrize("content", ["default", "dense", "overflow", "flat"])
def test_specialised_equals_generic(tmp_path, content):
    """The headline's program -- 1280x720, depth 2, literal, RGBA, a batch -- takes the specialised instance at both levels, the generic
    ones under TINYORB_FRONT_GENERIC=1, and both give the same bits: counters, level 1's grey plane, the blur planes (row constants and
    tail), records and descriptors.  Seven frames of the bench's content and one of seeded noise."""
    took_s, spec = run_case(tmp_path, "spec", content=content)
    assert took_s == {0: "specialised", 1: "specialised"}, took_s
    took_g, gen = run_case(tmp_path, "gen", content=content, env={"TINYORB_FRONT_GENERIC": "1"})
    assert took_g == {0: "generic", 1: "generic"}, took_g
    assert int(spec["count0"]) > 0 or content == "flat"
    assert_same(spec, gen)


def test_specialised_equals_oracle(tmp_path, oracle):
    """... and the specialised instances equal the oracle on those frames (content `default`)."""
    took, got = run_case(tmp_path, "spec_oracle", content="default")
    assert took == {0: "specialised", 1: "specialised"}, took
    assert_equals_oracle(oracle, got, 1280, 720, 2, "default", BATCH)


NEAR_MISSES = {
    "w1272": dict(W=1272),
    "w1288": dict(W=1288),
    "h712": dict(H=712),
    "depth3": dict(depth=3),
    "band_rows8": dict(env={"TINYORB_BAND_ROWS": "8"}),
    "y8": dict(y8=True),
    "max_batch1": dict(max_batch=1, n=2),
}


@pytest.mark.parametrize("case", sorted(NEAR_MISSES))
def test_near_miss_takes_generic_and_equals_oracle(tmp_path, oracle, case):
    """One step away from the headline's program: the host compares every field the geometry replaces, finds one that differs at either
    level (another depth leaves both levels' shapes alone and still changes the band slots per frame and the pyramid's strides), takes
    the generic instances, and the result is the oracle's."""
    kw = dict(NEAR_MISSES[case])
    took, got = run_case(tmp_path, case, **kw)
    assert set(took.values()) == {"generic"}, took
    assert_equals_oracle(oracle, got, kw.get("W", 1280), kw.get("H", 720), kw.get("depth", 2), "default", kw.get("n", BATCH), kw.get("y8", False))


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child(sys.argv[2], sys.argv[3])
