"""CPU checks of the track stage's C ABI (orb_track_consecutive): the OrbTrackParams, OrbTrack and
OrbTrackFrame layouts against include/tinyorb.h and the Python mirror, the source constants, the documented defaults against the
restatement's, the exports, and ORB_EINVAL without a program.  Parameter ranges on a live program: tests/test_gpu_track.py."""
import ctypes
import os
import re

import numpy as np

import track_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")


def _struct_fields(name):
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text, re.S).group(1)
    return re.findall(r"^\s*(?:u?int(?:16|32)_t|float)\s+([\w, ]+?)(?:\[\d+\])?;", body, re.M), body


def test_track_params_layout(tinyorb):
    names = ["source", "max_distance", "ratio", "min_gap", "max_gap", "keep_permille", "min_shared", "reserved"]
    assert ctypes.sizeof(tinyorb._TrackParams) == 32
    assert [getattr(tinyorb._TrackParams, k).offset for k in names] == list(range(0, 32, 4))
    fields, _ = _struct_fields("OrbTrackParams")
    assert fields == names


def test_track_record_layouts(tinyorb):
    t = tinyorb.TRACK_DTYPE
    assert t.itemsize == 16
    assert [t.fields[k][1] for k in ("prev", "next", "head_index", "head_frame", "tail_frame")] == [0, 4, 8, 12, 14]
    fields, _ = _struct_fields("OrbTrack")
    assert [n.strip() for f in fields for n in f.split(",")] == ["prev", "next", "head_index", "head_frame", "tail_frame"]
    fr = tinyorb.TRACK_FRAME_DTYPE
    assert fr.itemsize == 32
    names = ["keypoints", "links_in", "links_out", "keyframe", "ref_keyframe", "shared", "reserved"]
    assert [fr.fields[k][1] for k in names] == [0, 4, 8, 12, 16, 20, 24]
    fields, _ = _struct_fields("OrbTrackFrame")
    assert [n.strip() for f in fields for n in f.split(",")] == names


def test_track_constants(tinyorb):
    consts = dict(re.findall(r"#define\s+(ORB_TRACK_[A-Z_]+)\s+(\d+)u?\b", open(HEADER).read()))
    assert {k: int(v) for k, v in consts.items()} == {"ORB_TRACK_VERIFIED": 0, "ORB_TRACK_GUIDED": 1, "ORB_TRACK_MATCHED": 2}
    for k, v in consts.items():
        assert getattr(tinyorb, k) == int(v), k


def test_track_defaults_match_header():
    """Every '(0: N)' of OrbTrackParams' comments is the restatement's default."""
    _, body = _struct_fields("OrbTrackParams")
    documented = {name: float(v) for name, v in re.findall(r"^\s*(?:uint32_t|float)\s+(\w+);.*\(0: ([\d.]+)\)", body, re.M)}
    assert documented == {"max_distance": 64.0, "ratio": 0.8, "min_gap": 1.0, "keep_permille": 900.0}
    d = tr.defaults()
    for k, v in documented.items():
        assert np.float32(d[k]) == np.float32(v), k
    assert d["max_gap"] == 0 and d["min_shared"] == 0


def test_track_exports(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_track_consecutive", "orb_track_read", "orb_track_frames"):
        assert n in tinyorb.EXPORTS
        assert hasattr(L, n)


def test_track_abi_without_program(tinyorb):
    L = tinyorb.load_library()
    prm = tinyorb._TrackParams()
    assert L.orb_track_consecutive(None, 2, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_track_consecutive(None, 2, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_track_read(None, 0, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_track_frames(None, None, 0) == tinyorb.ORB_EINVAL
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("track" in n for n in names)
