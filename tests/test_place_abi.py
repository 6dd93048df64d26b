"""The C ABI of the place stage (orb_place_frames) as far as it can be checked without a device: the header's
declarations and structs against the Python mirror and the library's exports, and the defaults and ranges the call applies
against the restatement's."""
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
    P = tinyorb._PlaceParams
    assert ctypes.sizeof(P) == 32 and tinyorb.OrbPlaceParams is P
    fields = ("bits", "tables", "min_gap", "top", "min_score", "min_permille", "flags", "reserved")
    assert [f[0] for f in P._fields_] == list(fields) and [getattr(P, k).offset for k in fields] == [4 * i for i in range(8)]
    assert _struct_fields(text, "OrbPlaceParams") == list(fields)
    C = tinyorb.PLACE_CANDIDATE_DTYPE
    assert C.itemsize == 8 and C.names == ("frame", "score") and [C.fields[k][1] for k in C.names] == [0, 4]
    assert _struct_fields(text, "OrbPlaceCandidate") == ["frame", "score"]
    D = tinyorb.PLACE_ROW_DTYPE
    names = ("keypoints", "bits_set", "eligible", "candidates", "n", "reserved", "best")
    assert D.itemsize == 96 and D.names == names and [D.fields[k][1] for k in names] == [0, 4, 8, 12, 16, 20, 32]
    assert D.fields["best"][0].shape == (8,) and D.fields["best"][0].base == C
    assert _struct_fields(text, "OrbPlaceRow") == list(names)
    for name, value in (("ORB_PLACE_KEYFRAMES", "1u"), ("ORB_PLACE_DB", "0x80000000u"), ("ORB_PLACE_SIG_BYTES_MAX", "65536u"),
                        ("ORB_PLACE_DB_MAX", "1024u")):
        assert re.search(r"#define %s %s\b" % (name, value), text), name
        assert getattr(tinyorb, name) == int(value.rstrip("u"), 0)
    sigs = dict(re.findall(r"^int (orb_place_\w+)\(([^)]*)\);", text, re.M))
    assert sigs == {
        "orb_place_frames": "OrbProgram *p, uint32_t n_frames, const OrbPlaceParams *params, const uint8_t *db_host, uint32_t n_db, void *stream",
        "orb_place_read": "OrbProgram *p, uint32_t frame, OrbPlaceRow *rows, size_t n",
        "orb_place_signature": "OrbProgram *p, uint32_t frame, uint8_t *dst, size_t n_bytes"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_place_frames", "orb_place_read", "orb_place_signature"):
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    prm = tinyorb.OrbPlaceParams()
    assert L.orb_place_frames(None, 3, ctypes.byref(prm), None, 0, None) == tinyorb.ORB_EINVAL
    assert L.orb_place_frames(None, 3, None, None, 0, None) == tinyorb.ORB_EINVAL
    assert L.orb_place_read(None, 0, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_place_signature(None, 0, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any(n.startswith("k_place_") for n in names)


def test_defaults_and_ranges_are_the_restatements():
    """What orb_place_frames applies and checks before it touches the device, read from its source, against tests/place_ref.py."""
    import place_ref as pr
    text = open(os.path.join(ROOT, "tinyslam_amd", "csrc", "orb_api.hip")).read()
    body = text[text.index("int orb_place_frames("):text.index("int orb_place_read(")]
    for field, value in (("bits", pr.BITS_DEFAULT), ("tables", pr.TABLES_DEFAULT), ("min_gap", pr.MIN_GAP_DEFAULT),
                         ("top", pr.TOP_DEFAULT), ("min_score", pr.MIN_SCORE_DEFAULT)):
        assert "if (!g.%s) g.%s = %du;" % (field, field, value) in body, field
    assert pr.defaults() == dict(bits=16, tables=8, min_gap=32, top=4, min_score=1, min_permille=0, flags=0)
    assert ("g.bits < %du || g.bits > %du || g.tables > %du || g.top > %du || g.min_permille > %du"
            % (pr.BITS_MIN, pr.BITS_MAX, pr.TABLES_MAX, pr.TOP_MAX, pr.PERMILLE_MAX)) in body
    assert "((size_t)g.tables << g.bits) > 8u * (size_t)ORB_PLACE_SIG_BYTES_MAX" in body
    assert "g.reserved || (g.flags & ~ORB_PLACE_KEYFRAMES)" in body
    assert "n_db > ORB_PLACE_DB_MAX || (db_host != nullptr) != (n_db != 0u)" in body
    from tinyslam_amd import orb
    assert (pr.SIG_BYTES_MAX, pr.DB_MAX, pr.KEYFRAMES) == (orb.ORB_PLACE_SIG_BYTES_MAX, orb.ORB_PLACE_DB_MAX, orb.ORB_PLACE_KEYFRAMES)
    # the same ranges in the restatement
    assert pr.valid() and pr.valid(bits=8, tables=16, top=8, min_permille=1000, flags=1) and pr.valid(bits=16, tables=8)
    assert pr.valid(bits=15, tables=16) and not pr.valid(bits=16, tables=16) and not pr.valid(bits=16, tables=9)
    for bad in (dict(bits=7), dict(bits=17), dict(tables=17), dict(top=9), dict(min_permille=1001), dict(flags=2), dict(reserved=1)):
        assert not pr.valid(**bad), bad
    assert pr.sig_bytes() == 65536 and pr.sig_bytes(8, 1) == 32


def test_the_kernels_read_the_mirrors_layouts():
    from tinyslam_amd import orb
    text = open(os.path.join(ROOT, "tinyslam_amd", "csrc", "orb_kernels_place.h")).read()

    def const(name):
        return int(re.search(r"constexpr uint32_t %s = (\d+)u;" % name, text).group(1))

    assert const("kPlaceRowWords") * 4 == orb.PLACE_ROW_DTYPE.itemsize
    assert const("kPlaceTop") == orb.PLACE_ROW_DTYPE.fields["best"][0].shape[0]
    assert const("kPlaceFrameWords") * 4 == orb.TRACK_FRAME_DTYPE.itemsize
    assert const("kPlaceKeyframeWord") * 4 == orb.TRACK_FRAME_DTYPE.fields["keyframe"][1]
    import place_ref as pr
    assert const("kPlaceMaxTableWords") * 32 == 1 << pr.BITS_MAX and const("kPlaceMaxTables") == pr.TABLES_MAX
    assert const("kPlaceTile") == 32  # tests/test_gpu_place.py puts frame and id counts below, at and above it
