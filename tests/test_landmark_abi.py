"""The C ABI of the landmark stage (orb_landmarks_consecutive) as far as it can be checked without a device: the
header's declarations and structs against the Python mirror and the library's exports."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")


def _struct_fields(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)


def test_structs(tinyorb):
    text = open(HEADER).read()
    P = tinyorb._LandmarkParams
    assert ctypes.sizeof(P) == 32 and tinyorb.OrbLandmarkParams is P
    fields = ("fx", "fy", "cx", "cy", "max_reproj_px", "min_views", "reserved")
    assert [f[0] for f in P._fields_] == list(fields) and [getattr(P, k).offset for k in fields] == [0, 4, 8, 12, 16, 20, 24]
    assert _struct_fields(text, "OrbLandmarkParams") == list(fields)
    D = tinyorb.LANDMARK_DTYPE
    names = ("x", "y", "z", "flags", "views", "inliers", "origin", "tail_index", "reserved")
    assert D.itemsize == 32 and [D.fields[k][1] for k in names] == [0, 4, 8, 12, 16, 18, 20, 24, 28]
    assert D.fields["views"][0].itemsize == 2 and D.fields["inliers"][0].itemsize == 2
    assert _struct_fields(text, "OrbLandmark") == list(names)
    R = tinyorb.LANDMARK_ROW_DTYPE
    names = ("landmarks", "good", "longest", "origin")
    assert R.itemsize == 16 and [R.fields[k][1] for k in names] == [0, 4, 8, 12]
    assert _struct_fields(text, "OrbLandmarkRow") == list(names)
    assert tinyorb.ORB_LANDMARK_NO_ORIGIN == 0xFFFFFFFF
    sigs = dict(re.findall(r"^int (orb_landmarks_\w+)\(([^)]*)\);", text, re.M))
    assert sigs == {"orb_landmarks_consecutive": "OrbProgram *p, uint32_t n_frames, const OrbLandmarkParams *params, void *stream",
                    "orb_landmarks_read": "OrbProgram *p, uint32_t pair, OrbLandmarkRow *row, OrbLandmark *landmarks, size_t n"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_landmarks_consecutive", "orb_landmarks_read"):
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    prm = tinyorb.OrbLandmarkParams(fx=100.0, fy=100.0)
    assert L.orb_landmarks_consecutive(None, 3, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_landmarks_consecutive(None, 3, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_landmarks_read(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("k_lm" in n for n in names)


def test_the_frame_buffer_accessor(tinyorb):
    """orb_debug_frame_buffer, the tests' way to the frame records the stage reads: declared, exported, mirrored, and ORB_EINVAL for a
    NULL program without touching the out-pointer."""
    text = open(HEADER).read()
    sigs = dict(re.findall(r"^int (orb_debug_(?:frame|pose)_buffers?)\(([^)]*)\);", text, re.M))
    assert sigs == {"orb_debug_pose_buffers": "OrbProgram *p, void **matches, void **poses, void **points",
                    "orb_debug_frame_buffer": "OrbProgram *p, void **frames"}
    L = tinyorb.load_library()
    assert "orb_debug_frame_buffer" in tinyorb.EXPORTS and hasattr(L, "orb_debug_frame_buffer")
    vp = ctypes.c_void_p
    assert L.orb_debug_frame_buffer.argtypes == [vp, ctypes.POINTER(vp)] and hasattr(tinyorb.OrbProgram, "debug_frame_buffer")
    out = vp()
    assert L.orb_debug_frame_buffer(None, ctypes.byref(out)) == tinyorb.ORB_EINVAL and not out.value
    assert L.orb_debug_frame_buffer(None, None) == tinyorb.ORB_EINVAL
    assert tinyorb.FRAME_POSE_DTYPE.itemsize == 80  # the 20 words a row of the buffer has


def test_the_restatement_reads_the_mirror_and_the_kernels_the_same_layout():
    """The record's words as the kernel header stores them: two 16-byte halves, views in the low half of the fifth word."""
    import landmark_ref as lmr
    from tinyslam_amd import orb
    text = open(os.path.join(ROOT, "tinyslam_amd", "csrc", "orb_kernels_landmark.h")).read()

    def const(name):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % name, text).group(1)

    assert int(const("kLmFrameWords").rstrip("u")) * 4 == orb.FRAME_POSE_DTYPE.itemsize
    assert int(const("kLmRowWords").rstrip("u")) * 4 == orb.LANDMARK_ROW_DTYPE.itemsize
    assert int(const("kLmNoOrigin").rstrip("u"), 16) == orb.ORB_LANDMARK_NO_ORIGIN
    assert "hi0 = views | inliers << 16" in text
    assert [orb.FRAME_POSE_DTYPE.fields[k][1] // 4 for k in ("t", "origin", "status")] == [9, 14, 17]  # the words lm_view, lm_origin, lm_mapped read
    assert lmr.defaults(1, 1, 0, 0) == dict(fx=1, fy=1, cx=0, cy=0, max_reproj_px=2.0, min_views=2)
