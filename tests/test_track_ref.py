"""CPU checks of the track restatement (tests/track_ref.py, TK-1..TK-5 of DESIGN.md section 15) on hand-built link tables: the
one-to-one rule and its ties, chains that break and restart, blank frames, capacity cuts, each keyframe clause on its own and the
permille boundary."""
import numpy as np

import track_ref as tr
from tinyslam_amd.orb import MATCH_DTYPE, ORB_MATCH_NONE as NONE, ORB_TRACK_GUIDED, ORB_TRACK_MATCHED, ORB_TRACK_VERIFIED


def _links(pairs):
    """pairs[f]: {query: (target, distance)} -> the (target, distance) arrays track() takes, sized by the largest query + 1."""
    out = []
    for m in pairs:
        n = max(m) + 1 if m else 0
        j, d = np.full(n, -1, np.int64), np.zeros(n, np.int64)
        for i, (t, dist) in m.items():
            j[i], d[i] = t, dist
        out.append((j, d))
    return out


def _pad(links, counts):
    """Extend every pair's arrays to counts[f] queries (no link)."""
    out = []
    for f, (j, d) in enumerate(links):
        n = counts[f]
        jj, dd = np.full(n, -1, np.int64), np.zeros(n, np.int64)
        jj[:min(n, len(j))], dd[:min(n, len(d))] = j[:n], d[:n]
        out.append((jj, dd))
    return out


def test_many_to_one_keeps_smallest_key_and_ties_go_to_smallest_i():
    # queries 0, 1, 2 of frame 0 all link to target 1 of frame 1; 1 and 2 at distance 5, 0 at 7 -> query 1 wins (tie broken by i)
    counts = [4, 3]
    links = _pad(_links([{0: (1, 7), 1: (1, 5), 2: (1, 5), 3: (2, 9)}]), counts)
    t, fr = tr.track(counts, 8, links)
    assert list(t[0]["next"][:4]) == [NONE, 1, NONE, 2]
    assert list(t[1]["prev"][:3]) == [NONE, 1, 3]
    assert list(fr["links_out"]) == [2, 0] and list(fr["links_in"]) == [0, 2]
    # the order of the links does not matter: the same table with the queries permuted gives the permuted winners
    links = _pad(_links([{0: (1, 5), 1: (1, 5), 2: (1, 7), 3: (2, 9)}]), counts)
    t, _ = tr.track(counts, 8, links)
    assert list(t[0]["next"][:4]) == [1, NONE, NONE, 2]


def test_chains_break_and_restart():
    # keypoint chains: (0,0)->(1,1)->(2,0)->(3,2); (1,0) starts a new chain ->(2,1); (3,0) is alone; (0,1)->(1,2) then breaks
    counts = [2, 3, 2, 3]
    links = _pad(_links([{0: (1, 3), 1: (2, 4)}, {1: (0, 2), 0: (1, 6)}, {0: (2, 1)}]), counts)
    t, fr = tr.track(counts, 4, links)
    assert (t[3]["head_frame"][2], t[3]["head_index"][2]) == (0, 0)
    assert (t[2]["head_frame"][1], t[2]["head_index"][1]) == (1, 0)
    assert t[1]["tail_frame"][0] == 2 and t[1]["tail_frame"][1] == 3 and t[1]["tail_frame"][2] == 1
    assert (t[3]["head_frame"][0], t[3]["head_index"][0], t[3]["tail_frame"][0]) == (3, 0, 3)  # a track of length 1
    assert t[0]["tail_frame"][0] == 3 and t[0]["tail_frame"][1] == 1
    # entries past n_f
    assert t[0]["prev"][2] == NONE and t[0]["head_frame"][3] == 0xFFFF and t[0]["tail_frame"][2] == 0xFFFF
    assert list(fr["links_out"]) == [2, 2, 1, 0] and list(fr["links_in"]) == [0, 2, 2, 1]
    # TK-4: frame 2 keeps 1 of frame 0's 2 links (a keyframe at the default 900 permille); frame 3 shares 1 track with it
    assert list(fr["shared"]) == [2, 2, 1, 1]


def test_blank_frames_cut_every_track():
    counts = [3, 0, 3]
    links = _pad(_links([{}, {}]), counts)
    t, fr = tr.track(counts, 4, links)
    assert list(fr["keypoints"]) == [3, 0, 3]
    assert np.all(t[1]["prev"] == NONE) and np.all(t[1]["head_frame"] == 0xFFFF)
    assert list(t[2]["head_frame"][:3]) == [2, 2, 2]
    # frame 1: nothing is shared with frame 0 -> s == 0 -> keyframe; frame 2 against 1: s = 0 again
    assert list(fr["keyframe"]) == [1, 1, 1] and list(fr["shared"]) == [3, 0, 0] and list(fr["ref_keyframe"]) == [0, 0, 1]


def test_capacity_cut():
    # counts above cap: only the first cap queries and targets take part; links to targets >= n_t are dropped by pair_links
    rec = np.zeros(6, MATCH_DTYPE)
    rec["index"] = [0, 5, 2, 1, 3, 0]
    rec["distance"] = [1, 1, 1, 1, 1, 1]
    rec["second"] = [50, 50, 50, 50, 50, 50]
    j, d = tr.pair_links(ORB_TRACK_MATCHED, rec, 4, 4)
    assert list(j) == [0, -1, 2, 1]
    t, fr = tr.track([9, 7], 4, [(j, d)])
    assert len(t[0]) == 4 and list(t[0]["next"]) == [0, NONE, 2, 1] and list(fr["keypoints"]) == [4, 4]


def test_sources_and_candidate_test():
    rec = np.zeros(5, MATCH_DTYPE)
    rec["index"] = [0, 1, NONE, 3, 2]
    rec["distance"] = [10, 70, 10, 20, 40]
    rec["second"] = [20, 0xFFFF, 30, 25, 50]
    inl = np.array([1, 0, 0, 1, 1], np.uint8)
    j, _ = tr.pair_links(ORB_TRACK_VERIFIED, rec, 5, 4, inlier=inl)
    assert list(j) == [0, -1, -1, 3, 2]
    # 10 < 0.8 * 20; 70 > 64; NONE; 20 == 0.8 * 25 fails; 40 == 0.8 * 50 fails
    j, _ = tr.pair_links(ORB_TRACK_GUIDED, rec, 5, 4)
    assert list(j) == [0, -1, -1, -1, -1]
    j, _ = tr.pair_links(ORB_TRACK_MATCHED, rec, 5, 4, max_distance=80, ratio=0.9)
    assert list(j) == [0, 1, -1, 3, 2]
    j, _ = tr.pair_links(ORB_TRACK_MATCHED, rec, 5, 3, max_distance=80, ratio=0.9)  # target 3 is past n_t
    assert list(j) == [0, 1, -1, -1, 2]


def _straight(F, n, cut=None):
    """F frames of n keypoints, keypoint i linked to i in the next frame; cut[f] = the number of links kept out of frame f."""
    links = []
    for f in range(F - 1):
        m = n if cut is None else cut.get(f, n)
        j = np.full(n, -1, np.int64)
        j[:m] = np.arange(m)
        links.append((j, np.zeros(n, np.int64)))
    return [n] * F, links


def test_keyframe_min_gap_and_max_gap():
    counts, links = _straight(10, 5)
    _, fr = tr.track(counts, 8, links)
    assert list(fr["keyframe"]) == [1] + [0] * 9 and list(fr["shared"]) == [5] * 10  # everything tracked: no keyframe
    _, fr = tr.track(counts, 8, links, max_gap=3)
    assert list(np.nonzero(fr["keyframe"])[0]) == [0, 3, 6, 9]
    assert list(fr["ref_keyframe"]) == [0, 0, 0, 0, 3, 3, 3, 6, 6, 6]
    # min_gap holds back every other clause: with nothing shared (no links) every frame would be a keyframe
    counts, links = _straight(8, 5, cut={f: 0 for f in range(7)})
    _, fr = tr.track(counts, 8, links)
    assert list(fr["keyframe"]) == [1] * 8
    _, fr = tr.track(counts, 8, links, min_gap=3)
    assert list(np.nonzero(fr["keyframe"])[0]) == [0, 3, 6]
    _, fr = tr.track(counts, 8, links, min_gap=3, max_gap=3)
    assert list(np.nonzero(fr["keyframe"])[0]) == [0, 3, 6]


def test_keyframe_no_shared_tracks():
    counts, links = _straight(5, 4, cut={2: 0})  # every track ends at frame 2
    _, fr = tr.track(counts, 8, links, keep_permille=1)
    assert list(fr["keyframe"]) == [1, 0, 0, 1, 0] and list(fr["shared"]) == [4, 4, 4, 0, 4]


def test_keyframe_ratio_and_permille_boundary():
    # 10 keypoints; out of frame 0 all 10 link; 8 of the tracks reach frame 3, 5 reach frame 5
    counts, links = _straight(6, 10, cut={2: 8, 4: 5})
    _, fr = tr.track(counts, 16, links, keep_permille=800)
    # frame 3: 1000 * 8 == 800 * 10 -> not below -> no keyframe; frame 5: 5000 < 8000 -> keyframe
    assert list(fr["shared"][1:]) == [10, 10, 8, 8, 5]
    assert list(fr["keyframe"]) == [1, 0, 0, 0, 0, 1]
    _, fr = tr.track(counts, 16, links, keep_permille=801)
    # 8000 < 8010; then against frame 3 (10 links out): frame 4 shares all 10 (two tracks start at 3), frame 5 keeps 5 -> keyframe
    assert list(fr["keyframe"]) == [1, 0, 0, 1, 0, 1]
    assert list(fr["ref_keyframe"]) == [0, 0, 0, 0, 3, 3] and list(fr["shared"]) == [10, 10, 10, 8, 10, 5]


def test_keyframe_min_shared():
    counts, links = _straight(6, 10, cut={2: 8, 4: 5})
    _, fr = tr.track(counts, 16, links, keep_permille=1, min_shared=8)
    assert list(fr["keyframe"]) == [1, 0, 0, 0, 0, 1]  # 8 is not below 8, 5 is
    _, fr = tr.track(counts, 16, links, keep_permille=1, min_shared=9)
    assert list(fr["keyframe"]) == [1, 0, 0, 1, 0, 1]
