"""The C ABI of the trajectory stage (orb_trajectory_consecutive) as far as it can be checked without a device:
the header's declarations, structs and constants against the Python mirror and the library's exports."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")


def _struct_fields(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)


def test_structs_and_constants(tinyorb):
    text = open(HEADER).read()
    assert ctypes.sizeof(tinyorb._TrajectoryParams) == 32 and tinyorb.OrbTrajectoryParams is tinyorb._TrajectoryParams
    assert tinyorb.FRAME_POSE_DTYPE.itemsize == 80
    names = ("r", "t", "scale", "step", "origin", "shared", "consistent", "status", "reserved")
    assert [tinyorb.FRAME_POSE_DTYPE.fields[k][1] for k in names] == [0, 36, 48, 52, 56, 60, 64, 68, 72]
    assert _struct_fields(text, "OrbTrajectoryParams") == [f[0] for f in tinyorb._TrajectoryParams._fields_]
    assert _struct_fields(text, "OrbFramePose") == list(names)
    consts = dict(re.findall(r"#define\s+(ORB_TRAJ_[A-Z_]+)\s+(\d+)u\b", text))
    assert sorted(consts) == ["ORB_TRAJ_CHAINED", "ORB_TRAJ_LOST", "ORB_TRAJ_NEED_PARALLAX", "ORB_TRAJ_ORIGIN", "ORB_TRAJ_RESTART_FEW",
                              "ORB_TRAJ_RESTART_SPREAD", "ORB_TRAJ_START"]
    for name, value in consts.items():
        assert int(value) == getattr(tinyorb, name), name
    assert [tinyorb.ORB_TRAJ_CHAINED, tinyorb.ORB_TRAJ_START, tinyorb.ORB_TRAJ_RESTART_FEW, tinyorb.ORB_TRAJ_RESTART_SPREAD,
            tinyorb.ORB_TRAJ_LOST, tinyorb.ORB_TRAJ_ORIGIN] == [0, 1, 2, 3, 4, 5]
    sigs = dict(re.findall(r"^int (orb_trajectory_\w+)\(([^)]*)\);", text, re.M))
    assert sigs == {"orb_trajectory_consecutive": "OrbProgram *p, uint32_t n_frames, const OrbTrajectoryParams *params, void *stream",
                    "orb_trajectory_read": "OrbProgram *p, uint32_t frame, OrbFramePose *pose, OrbPoint *points, size_t n"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_program(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_trajectory_consecutive", "orb_trajectory_read", "orb_debug_pose_buffers"):
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    out = ctypes.c_void_p()
    assert L.orb_debug_pose_buffers(None, ctypes.byref(out), None, None) == tinyorb.ORB_EINVAL and not out.value
    prm = tinyorb.OrbTrajectoryParams()
    assert L.orb_trajectory_consecutive(None, 2, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_trajectory_consecutive(None, 2, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_trajectory_read(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("traj" in n for n in names)
