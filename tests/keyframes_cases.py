"""Inputs of the keyframe tests, for the CPU restatement and for the device (test infrastructure, not a test file).

The first batch is loop_cases.out_and_back; `second_batch` is five views of the same cloud on a path of its own -- the generator
draws the cloud first, so the same seed gives the same landmarks -- and `plant_pair` gives both batches descriptors from the same
per-landmark draws, so that a frame of the second batch matches a keyframe of the first as two frames of one batch match.
`reference` runs the first batch through the trajectory and landmark restatements and inserts frames into a store.
"""
import numpy as np

import constructed as C
import keyframes_ref as kfr
import landmark_cases as L
import localize_cases as lc
import loop_cases as K
import trajectory_ref as tr

SECOND_FRAMES = 5
# (query of the second batch, slot = frame of the first): near and far keyframes, a duplicate slot, both ends of the path
SECOND_PAIRS = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (4, 0), (0, 4), (2, 10), (3, 7), (1, 9)]


def second_steps():
    """Four camera steps from the first batch's frame 0: more pitch than the first path's, sideways and a little back."""
    lengths = [0.35, 0.3, 0.45, 0.25]
    return [(tr.rot("y", 0.5) @ tr.rot("x", -0.4), np.array([-l, -0.15 * l, -0.1 * l])) for l in lengths]


def second_batch(seed, n_land=200, cap=128, wrong=0.05, noise=0.001):
    """Five views of out_and_back(seed)'s cloud on second_steps()."""
    return lc.views(np.random.default_rng(seed), SECOND_FRAMES, n_land, cap, steps=second_steps(), wrong=wrong, noise=noise)


def plant_pair(b1, b2, seed, max_flips=8):
    """loop_cases.plant on both batches from generators of one seed: its first draw is the per-landmark descriptors."""
    return K.plant(b1, np.random.default_rng(seed), max_flips), K.plant(b2, np.random.default_rng(seed), max_flips)


def true_relative(b1, b2, q, T, o):
    """loop_cases.true_relative for camera q of the second batch and camera T of the first, in the unit of the first batch's
    segment of origin o: ((R, t) of q relative to T, (R, t) of q relative to o)."""
    c1, c2 = K.cameras(b1), K.cameras(b2)
    unit = np.linalg.norm(b1["steps"][o][1])

    def rel(a, c):
        (Ra, ta), (Rc, tc_) = a, c
        R = Ra @ Rc.T
        return R, (ta - R @ tc_) / unit

    return rel(c2[q], c1[T]), rel(c2[q], c1[o])


def batch_inputs(b, desc, n=None):
    """(stored counts, corners, descriptors, matches) of a views batch as the restatements take them."""
    n = b["n"] if n is None else n
    nq = lc.stored(b)
    return nq, [c[:nq[f]] for f, c in enumerate(b["corners"])], [np.asarray(d, np.uint32).reshape(-1, 8)[:nq[f]] for f, d in enumerate(desc)], \
        [b["matches"][f][:nq[f]] for f in range(n - 1)]


def reference(b, desc, entries, traj=None, L_frames=None, store=None):
    """A views batch through the trajectory and landmark restatements, then KF-2 of `entries`.  Returns (frame records, landmark
    records, store)."""
    n = b["n"] if L_frames is None else L_frames
    fr, lms, _ = L.reference(b, n, traj=traj)
    if n < b["n"]:
        fr = L.tc.reference(b, b["n"], **(traj or {}))[0]
    nq, corners, descs, matches = batch_inputs(b, desc, n)
    store = {} if store is None else store
    kfr.insert(store, entries, nq, corners, descs, matches, fr, list(lms), b["cap"], L=n)
    return fr, lms, store
