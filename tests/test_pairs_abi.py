"""The C ABI of orb_match_pairs and orb_verify_pairs as far as it can be checked without a device: the header's
declarations and struct against the Python mirror and the library's exports, and the capacity, the models and the defaults the
calls apply against the restatement's (tests/pairs_ref.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
NAMES = ("orb_match_pairs", "orb_match_pairs_read", "orb_verify_pairs", "orb_verify_pairs_read")


def test_struct_constants_and_signatures(tinyorb):
    text = open(HEADER).read()
    D = tinyorb.FRAME_PAIR_DTYPE
    assert D.itemsize == 8 and D.names == ("query", "target") and [D.fields[k][1] for k in D.names] == [0, 4]
    body = re.search(r"typedef struct \{([^}]*)\} OrbFramePair;", text).group(1)
    assert re.findall(r"(\w+)\s*[,;]", body) == ["query", "target"] and body.split()[0] == "uint32_t"
    for name, value in (("ORB_PAIRS_PER_FRAME", 4), ("ORB_PAIRS_HOMOGRAPHY", 0), ("ORB_PAIRS_EPIPOLAR", 1)):
        assert re.search(r"#define %s %du\b" % (name, value), text), name
        assert getattr(tinyorb, name) == value
    sigs = dict(re.findall(r"^int (orb_(?:match|verify)_pairs\w*)\(([^)]*)\);", text, re.M))
    assert sigs == {
        "orb_match_pairs": "OrbProgram *p, const OrbFramePair *pairs_host, uint32_t n_pairs, void *stream",
        "orb_match_pairs_read": "OrbProgram *p, uint32_t pair, OrbMatch *dst, size_t n",
        "orb_verify_pairs": "OrbProgram *p, uint32_t n_pairs, uint32_t model, const OrbVerifyParams *params, void *stream",
        "orb_verify_pairs_read": "OrbProgram *p, uint32_t pair, OrbPairModel *model, uint8_t *inlier, size_t n"}
    # the records are the consecutive stages' own
    assert tinyorb.MATCH_DTYPE.itemsize == 8 and tinyorb.VERIFY_MODEL_DTYPE.itemsize == 64 and ctypes.sizeof(tinyorb._VerifyParams) == 32
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    L = tinyorb.load_library()
    for n in NAMES:
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    one = (ctypes.c_uint32 * 2)(0, 1)
    prm = tinyorb._VerifyParams()
    assert L.orb_match_pairs(None, one, 1, None) == tinyorb.ORB_EINVAL
    assert L.orb_match_pairs(None, None, 0, None) == tinyorb.ORB_EINVAL
    assert L.orb_match_pairs_read(None, 0, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_verify_pairs(None, 1, 0, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_verify_pairs(None, 1, 1, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_verify_pairs_read(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("pairs" in n for n in names)  # no profile ids for the new kernels


def test_capacity_models_and_defaults_are_the_restatements():
    """What the two calls apply and check before they touch the device, read from their source, against tests/pairs_ref.py."""
    import pairs_ref as pf
    import place_ref as pr
    import verify_ref as vr
    from tinyslam_amd import orb
    text = open(os.path.join(ROOT, "tinyslam_amd", "csrc", "orb_api.hip")).read()
    match = text[text.index("int orb_match_pairs("):text.index("int orb_match_pairs_read(")]
    assert "P = (size_t)ORB_PAIRS_PER_FRAME * p->plan.max_batch" in match
    assert "!pairs_host || n_pairs < 1u || n_pairs > P" in match
    assert "e.query >= p->last_batch || e.target >= p->last_batch || e.query == e.target" in match
    assert 'if (!p->last_batch) return fail(p, ORB_ESTATE' in match
    assert (pf.PAIRS_PER_FRAME, pf.HOMOGRAPHY, pf.EPIPOLAR) == (orb.ORB_PAIRS_PER_FRAME, orb.ORB_PAIRS_HOMOGRAPHY, orb.ORB_PAIRS_EPIPOLAR)
    assert pf.PAIRS_PER_FRAME == pr.TOP_DEFAULT and pf.capacity(7) == 28 and pf.FRAME_PAIR_DTYPE == orb.FRAME_PAIR_DTYPE
    verify = text[text.index("int orb_verify_pairs("):text.index("int orb_verify_pairs_read(")]
    assert "model > ORB_PAIRS_EPIPOLAR" in verify and "model == ORB_PAIRS_EPIPOLAR ? kEpipolar : kHomography" in verify
    # the parameter block is the consecutive verifiers': one function checks it and applies the defaults for all three calls
    shared = text[text.index("int verifier_params("):text.index("VerifyArgs verifier_args(")]
    assert "if (v.inlier_px == 0.0f) v.inlier_px = 3.0f;" in shared and "ransac_params(p, which, &v.hypotheses, &v.max_distance, &v.ratio)" in shared
    ransac = text[text.index("int ransac_params("):text.index("int check_intrinsics(")]
    assert "if (!*hypotheses) *hypotheses = 512u;" in ransac and "if (!*max_distance) *max_distance = 64u;" in ransac and "*ratio = 0.8f;" in ransac
    d = pf.defaults()
    assert (d["hypotheses"], d["max_distance"], float(d["ratio"]), float(d["inlier_px"]), d["seed"]) == (512, 64, float(vr.F(0.8)), 3.0, 0)
    assert text.count("verifier_params(p, ") == 2  # run_verifier and run_pairs_verifier
    # the two stages' rows of the stage table: the pairs verifier reads the pairs matcher alone
    assert '{"match_pairs", "match_pairs_read", 0u}' in text
    assert re.search(r'\{"verify_pairs", "verify_pairs_read",\s*1u << ST_PAIRS\}', text)


def test_the_kernels_share_their_bodies_with_the_consecutive_ones():
    """One source per body: the consecutive kernel and its pairs form include the same text."""
    csrc = os.path.join(ROOT, "tinyslam_amd", "csrc")
    pairs = open(os.path.join(csrc, "orb_kernels_pairs.h")).read()
    for inc, home in (("orb_match_fp4_body.inc", "orb_kernels_match.h"), ("orb_match_valu_body.inc", "orb_kernels_staged.h"),
                      ("orb_verify_gather_body.inc", "orb_kernels_verify.h")):
        line = '#include "%s"' % inc
        assert pairs.count(line) == 1 and open(os.path.join(csrc, home)).read().count(line) == 1, inc
