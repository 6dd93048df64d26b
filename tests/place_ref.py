"""CPU restatement of the place stage, PL-1..PL-6 of DESIGN.md section 25, in NumPy (test infrastructure, not a test file).

Integer arithmetic only: the signatures and the OrbPlaceRow bytes of orb_place_frames must equal what this module returns, bit
for bit.  Written from the definition, not from the kernels: a signature is the OR of one bit per stored record and table, a score
a byte-wise population count of the AND, and a row a sort of all candidates by PL-6's key.
"""
import numpy as np

from tinyslam_amd.orb import ORB_MATCH_NONE as NONE, ORB_PLACE_DB, PLACE_ROW_DTYPE

BITS_MIN, BITS_MAX, BITS_DEFAULT = 8, 16, 16
TABLES_MAX, TABLES_DEFAULT = 16, 8
TOP_MAX, TOP_DEFAULT = 8, 4
MIN_GAP_DEFAULT = 32
MIN_SCORE_DEFAULT = 1
PERMILLE_MAX = 1000
SIG_BYTES_MAX = 65536
DB_MAX = 1024
KEYFRAMES = 1              # ORB_PLACE_KEYFRAMES

_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def defaults(bits=0, tables=0, min_gap=0, top=0, min_score=0, min_permille=0, flags=0):
    """OrbPlaceParams with its zero fields replaced by the defaults."""
    return dict(bits=bits or BITS_DEFAULT, tables=tables or TABLES_DEFAULT, min_gap=min_gap or MIN_GAP_DEFAULT, top=top or TOP_DEFAULT,
                min_score=min_score or MIN_SCORE_DEFAULT, min_permille=min_permille, flags=flags)


def valid(bits=0, tables=0, min_gap=0, top=0, min_score=0, min_permille=0, flags=0, reserved=0):
    """The ranges orb_place_frames accepts (ORB_EINVAL otherwise)."""
    p = defaults(bits, tables, min_gap, top, min_score, min_permille, flags)
    return (BITS_MIN <= p["bits"] <= BITS_MAX and 1 <= p["tables"] <= TABLES_MAX and (p["tables"] << p["bits"]) <= 8 * SIG_BYTES_MAX
            and 1 <= p["top"] <= TOP_MAX and 0 <= min_permille <= PERMILLE_MAX and not (flags & ~KEYFRAMES) and reserved == 0)


def sig_bytes(bits=0, tables=0):
    p = defaults(bits, tables)
    return (p["tables"] << p["bits"]) // 8


def keys(desc, t, bits):
    """PL-1: the key of every record ((n, 8) uint32 descriptors) in table t."""
    d = np.asarray(desc, dtype=np.uint32).reshape(-1, 8)
    half = (d[:, t >> 1] >> np.uint32(16 * (t & 1))) & np.uint32(0xFFFF)
    return (half & np.uint32((1 << bits) - 1)).astype(np.int64)


def signature(desc, stored, bits=0, tables=0):
    """PL-2: the signature (uint8 (sig_bytes,)) of a frame from its first `stored` records."""
    p = defaults(bits, tables)
    bits, tables = p["bits"], p["tables"]
    per = (1 << bits) // 8
    sig = np.zeros(tables * per, np.uint8)
    d = np.asarray(desc, dtype=np.uint32).reshape(-1, 8)[:stored]
    for t in range(tables):
        k = keys(d, t, bits)
        np.bitwise_or.at(sig, t * per + (k >> 3), np.left_shift(1, k & 7).astype(np.uint8))
    return sig


def popcount(a):
    """Set bits of every row of a uint8 array."""
    return _POP8[a].sum(-1, dtype=np.int64)


def score(a, b):
    """PL-3."""
    return int(popcount(np.bitwise_and(a, b)))


def place(counts, desc, cap, n_frames=None, db=None, keyframes=None, **params):
    """orb_place_frames over frames [0, n_frames) (None: len(counts)).  counts: the raw counters; desc[f]: uint32 (m_f, 8) with
    m_f >= min(counts[f], cap) -- rows past the stored count are stale data and never read; db: uint8 (n_db, sig_bytes) or None;
    keyframes: a flag per frame, required iff flags has KEYFRAMES.  Returns (signatures uint8 (n_frames, sig_bytes),
    PLACE_ROW_DTYPE (n_frames,))."""
    p = defaults(**params)
    assert valid(**params), params
    n = len(counts) if n_frames is None else n_frames
    nb = sig_bytes(p["bits"], p["tables"])
    stored = [min(int(counts[f]), cap) for f in range(n)]
    sigs = np.stack([signature(desc[f], stored[f], p["bits"], p["tables"]) for f in range(n)])
    db = np.zeros((0, nb), np.uint8) if db is None else np.asarray(db, np.uint8).reshape(-1, nb)
    n_db = len(db)
    assert n_db <= DB_MAX
    use_key = bool(p["flags"] & KEYFRAMES)
    assert use_key == (keyframes is not None)
    rows = np.zeros(n, PLACE_ROW_DTYPE)
    rows["best"]["frame"] = NONE
    every = np.concatenate([db, sigs])       # by id (PL-4)
    for f in range(n):
        bits_f = int(popcount(sigs[f]))
        ids = list(range(n_db)) + [n_db + g for g in range(n)
                                   if g + p["min_gap"] <= f and (not use_key or int(keyframes[g]) != 0)]
        sc = popcount(np.bitwise_and(every[ids], sigs[f])) if ids else np.zeros(0, np.int64)
        cand = [(int(s), i) for s, i in zip(sc, ids)
                if s >= max(p["min_score"], 1) and 1000 * int(s) >= p["min_permille"] * bits_f]      # PL-5
        cand.sort(key=lambda c: (c[0] << 32) | (0xFFFFFFFF - c[1]), reverse=True)                     # PL-6
        r = rows[f]
        r["keypoints"], r["bits_set"], r["eligible"], r["candidates"] = stored[f], bits_f, len(ids), len(cand)
        r["n"] = min(len(cand), p["top"])
        for j, (s, i) in enumerate(cand[:p["top"]]):
            r["best"][j] = ((ORB_PLACE_DB | i) if i < n_db else i - n_db, s)
    return sigs, rows
