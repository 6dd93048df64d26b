"""CPU restatement of the graph stage, PG-1..PG-8 of DESIGN.md section 29, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_graph.h
perform, in the same order: the OrbGraphPose and OrbGraphEdge bytes of orb_graph_pairs must equal what this module returns, bit
for bit.  The chain edges of a segment are vectorised over its nodes (entry k of an array belongs to the edge into node k); the
loop edges are taken one by one in ascending list index, which is the order of every node's CSR row; the 6 x 6 blocks of all nodes
are inverted together, the six unit vectors as six right sides of one elimination (the matrix part of verify_solve_n's
elimination does not depend on the right side).
"""
import numpy as np

from tinyslam_amd.orb import (GRAPH_EDGE_DTYPE, GRAPH_POSE_DTYPE, ORB_GRAPH_EDGE_FEW, ORB_GRAPH_EDGE_NONFINITE, ORB_GRAPH_EDGE_RANGE,
                              ORB_GRAPH_EDGE_SEGMENT, ORB_GRAPH_EDGE_SEGMENT_INVALID, ORB_GRAPH_EDGE_STATUS, ORB_GRAPH_EDGE_USED,
                              ORB_GRAPH_FAILED, ORB_GRAPH_HELD, ORB_GRAPH_INVALID, ORB_GRAPH_REFINED, ORB_GRAPH_STALLED,
                              ORB_GRAPH_UNCHANGED, ORB_GRAPH_USE_MINIMAL, ORB_LOCALIZE_MINIMAL, ORB_LOCALIZE_OK, ORB_TRAJ_LOST,
                              ORB_TRAJ_ORIGIN)

F = np.float32
NONE = 0xFFFFFFFF
MAX_ROUNDS, MAX_CG, LDS_NODES = 16, 512, 512


def defaults(rounds=0, cg_iterations=0, min_inliers=0, loop_weight=0.0, rotation_weight=0.0, flags=0):
    """OrbGraphParams with its zero fields replaced by the defaults (cg_iterations 0 stays: it is the segment's free nodes)."""
    return dict(rounds=rounds or 4, cg_iterations=cg_iterations, min_inliers=min_inliers or 12,
                loop_weight=F(loop_weight) if loop_weight else F(1), rotation_weight=F(rotation_weight) if rotation_weight else F(1), flags=flags)


# ---- PG-2 --------------------------------------------------------------------------------------------------------------------
def _member(frames, h, o):
    return int(frames["origin"][h]) == o and int(frames["status"][h]) not in (ORB_TRAJ_LOST, ORB_TRAJ_ORIGIN)


def free_origin(frames, g):
    """The origin of the segment in which frame g is a free node, NONE when it is free in none: its record names an origin o < g
    and every frame o + 1 .. g names the same one with a status other than LOST / ORIGIN."""
    if g >= len(frames):
        return NONE
    o = int(frames["origin"][g])
    if o >= g or not all(_member(frames, h, o) for h in range(o + 1, g + 1)):
        return NONE
    return o


def segment_nodes(frames, o):
    """n: the free nodes of segment o are frames o + 1 .. o + n."""
    n = 0
    while o + 1 + n < len(frames) and _member(frames, o + 1 + n, o):
        n += 1
    return n


def segment_invalid(frames, o, n):
    sel = frames[o + 1:o + 1 + n]
    return not (np.isfinite(sel["r"]).all() and np.isfinite(sel["t"]).all())


def is_node(frames, g, o):
    return g == o or free_origin(frames, g) == o


# ---- PG-4 --------------------------------------------------------------------------------------------------------------------
def verdict(frames, q, T, fix, p):
    st = int(fix["status"])
    o, qo, nF = int(fix["origin"]), int(fix["query_origin"]), len(frames)
    if not (st == ORB_LOCALIZE_OK or (st == ORB_LOCALIZE_MINIMAL and p["flags"] & ORB_GRAPH_USE_MINIMAL)):
        return ORB_GRAPH_EDGE_STATUS
    if int(fix["inliers"]) < p["min_inliers"]:
        return ORB_GRAPH_EDGE_FEW
    if q >= nF or T >= nF or qo == NONE:
        return ORB_GRAPH_EDGE_RANGE
    if o != qo or not is_node(frames, q, o) or not is_node(frames, T, o):
        return ORB_GRAPH_EDGE_SEGMENT
    if not (np.isfinite(fix["r"]).all() and np.isfinite(fix["t"]).all()):
        return ORB_GRAPH_EDGE_NONFINITE
    if segment_invalid(frames, o, segment_nodes(frames, o)):
        return ORB_GRAPH_EDGE_SEGMENT_INVALID
    return ORB_GRAPH_EDGE_USED


# ---- PG-5 on lists of arrays: an entry per edge -------------------------------------------------------------------------------
def _matvec(M, v):
    return [(M[3 * r] * v[0] + M[3 * r + 1] * v[1]) + M[3 * r + 2] * v[2] for r in range(3)]


def _matvec_t(M, v):
    return [(M[r] * v[0] + M[3 + r] * v[1]) + M[6 + r] * v[2] for r in range(3)]


def _cross(x, y):
    return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]


def geom(Ra, ta, Rb, tb, a_held):
    """(R^, s = R^ t_a, t^, t_a) of the edges a -> b; where a_held, camera a is the origin: R^ = R_b and t^ = t_b exactly."""
    Rh = [(Rb[3 * r] * Ra[3 * c] + Rb[3 * r + 1] * Ra[3 * c + 1]) + Rb[3 * r + 2] * Ra[3 * c + 2] for r in range(3) for c in range(3)]
    Rh = [np.where(a_held, Rb[k], Rh[k]) for k in range(9)]
    s = _matvec(Rh, ta)
    s = [np.where(a_held, F(0), s[r]) for r in range(3)]
    tav = [np.where(a_held, F(0), ta[r]) for r in range(3)]
    th = [tb[r] - s[r] for r in range(3)]
    return Rh, s, th, tav


def residual(G, Rz, tz):
    Rh, s, th, ta = G
    E = [(Rh[3 * r] * Rz[3 * c] + Rh[3 * r + 1] * Rz[3 * c + 1]) + Rh[3 * r + 2] * Rz[3 * c + 2] for r in range(3) for c in range(3)]
    return [F(0.5) * (E[7] - E[5]), F(0.5) * (E[2] - E[6]), F(0.5) * (E[3] - E[1])] + [th[r] - tz[r] for r in range(3)]


def edge_cost(e, w, rho):
    return w * (rho * ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + ((e[3] * e[3] + e[4] * e[4]) + e[5] * e[5]))


def forward(G, pa, pb):
    """u = v_b - v_a; a None end is held."""
    Rh, s, th, ta = G
    zero = np.zeros_like(Rh[0])
    vb, va = [zero] * 6, [zero] * 6
    if pb is not None:
        c = _cross(s, pb)
        vb = [pb[r] for r in range(3)] + [c[r] + pb[3 + r] for r in range(3)]
    if pa is not None:
        c = _cross(ta, pa)
        d = [c[r] + pa[3 + r] for r in range(3)]
        va = _matvec(Rh, pa) + _matvec(Rh, d)
    return [vb[k] - va[k] for k in range(6)]


def back(G, head, w, rho, u):
    Rh, s, th, ta = G
    qR = [w * (rho * u[r]) for r in range(3)]
    qt = [w * u[3 + r] for r in range(3)]
    if head:
        x = _cross(qt, s)
        return [qR[r] + x[r] for r in range(3)] + qt
    x, y = _matvec_t(Rh, qR), _matvec_t(Rh, qt)
    z = _cross(ta, y)
    return [z[r] - x[r] for r in range(3)] + [-y[r] for r in range(3)]


def _units(n):
    return [[np.full(n, 1 if k == c else 0, F) for k in range(6)] for c in range(6)]


# ---- PG-6 --------------------------------------------------------------------------------------------------------------------
def invert_blocks(D):
    """D[r][c]: arrays (n,).  Section 21's solver (localize_ref.solve at n = 6: the upper triangle mirrored, partial pivoting with
    the first maximal pivot) on the six unit vectors: (Dinv (n, 6, 6), ok (n,))."""
    n = len(D[0][0])
    A = np.zeros((n, 6, 12), F)
    for r in range(6):
        for c in range(r, 6):
            A[:, r, c] = A[:, c, r] = D[r][c]
        A[:, r, 6 + r] = 1
    with np.errstate(all="ignore"):
        ok = np.ones(n, bool)
        idx = np.arange(n)
        for c in range(6):
            piv, pmax = np.full(n, c), np.abs(A[:, c, c])
            for r in range(c + 1, 6):
                v = np.abs(A[:, r, c])
                gt = v > pmax
                pmax, piv = np.where(gt, v, pmax), np.where(gt, r, piv)
            ok &= pmax != 0
            rows = A[idx, piv].copy()
            A[idx, piv] = A[:, c]
            A[:, c] = rows
            for r in range(c + 1, 6):
                f = A[:, r, c] / A[:, c, c]
                A[:, r, c + 1:] = A[:, r, c + 1:] - f[:, None] * A[:, c, c + 1:]
        X = np.zeros((n, 6, 6), F)
        for k in range(6):
            for r in range(5, -1, -1):
                s = A[:, r, 6 + k]
                for q in range(r + 1, 6):
                    s = s - A[:, r, q] * X[:, q, k]
                X[:, r, k] = s / A[:, r, r]
                ok &= np.isfinite(X[:, r, k])
    return X, ok


def total(d):
    """The sum of one value per node: node j into partial j mod 256 in ascending j, then GV-6's tree s = 128 .. 1."""
    part = np.zeros(256, F)
    for c0 in range(0, len(d), 256):
        seg = d[c0:c0 + 256]
        part[:len(seg)] = part[:len(seg)] + seg
    s = 128
    while s >= 1:
        part[:s] = part[:s] + part[s:2 * s]
        s >>= 1
    return part[0]


def dot6(x, y):
    return ((((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]) + x[3] * y[3]) + x[4] * y[4]) + x[5] * y[5]


def precondition(Dinv, r):
    return [dot6([Dinv[:, i, k] for k in range(6)], r) for i in range(6)]


# ---- a segment ---------------------------------------------------------------------------------------------------------------
class Segment:
    """Segment o with n free nodes: R (9, n), t (3, n) current poses; loops: (i, q, T, Rz, tz) of its USED entries, ascending."""

    def __init__(self, frames, o, n, loops, p):
        self.o, self.n, self.p = o, n, p
        sel = frames[o + 1:o + 1 + n]
        self.R = np.ascontiguousarray(sel["r"].T.astype(F))
        self.t = np.ascontiguousarray(sel["t"].T.astype(F))
        self.loops = loops
        held0 = np.arange(n) == 0
        self.held0 = held0
        G = self.chain_geom()
        self.Rz, self.tz = G[0], G[2]  # PG-3: from the records as read

    def pose(self, f):
        """Lists of (1,) arrays: node f - o - 1, or the identity for the origin."""
        if f == self.o:
            return [np.full(1, 1 if k % 4 == 0 else 0, F) for k in range(9)], [np.zeros(1, F)] * 3
        j = f - self.o - 1
        return [self.R[k, j:j + 1] for k in range(9)], [self.t[k, j:j + 1] for k in range(3)]

    def chain_geom(self):
        R, t, n = self.R, self.t, self.n
        ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F)
        Ra = [np.concatenate([ident[k:k + 1], R[k, :n - 1]]) for k in range(9)]
        ta = [np.concatenate([np.zeros(1, F), t[k, :n - 1]]) for k in range(3)]
        return geom(Ra, ta, list(R), list(t), self.held0)

    def loop_geom(self, q, T):
        Ra, ta = self.pose(T)
        Rb, tb = self.pose(q)
        return geom(Ra, ta, Rb, tb, np.full(1, T == self.o))

    def node(self, f):
        return None if f == self.o else f - self.o - 1

    def scatter(self, vec):
        """(6, n) p -> the function f -> list of (1,) arrays or None for the origin."""
        def get(f):
            j = self.node(f)
            return None if j is None else [vec[k, j:j + 1] for k in range(6)]
        return get

    def cost(self):
        """(the segment's cost, {i: the cost of loop edge i}): an edge is indexed by its head, a loop edge onto the origin by its
        tail."""
        p = self.p
        c = edge_cost(residual(self.chain_geom(), self.Rz, self.tz), F(1), p["rotation_weight"]).astype(F)
        own = {}
        for i, q, T, Rz, tz in self.loops:
            ec = edge_cost(residual(self.loop_geom(q, T), Rz, tz), p["loop_weight"], p["rotation_weight"])[0]
            own[i] = ec
            j = self.node(q) if q != self.o else self.node(T)
            c[j] = c[j] + ec
        return total(c), own

    def accumulate(self, contrib_chain, contrib_loop):
        """PG-5's order at every node: the chain edge into it, the chain edge out of it, its loop edges in ascending list index.
        contrib_chain(G, head) -> list of (n,) arrays; contrib_loop(G, head, q, T) -> list of (1,) arrays."""
        n = self.n
        G = self.chain_geom()
        acc = np.stack(contrib_chain(G, True)).astype(F)
        if n > 1:
            out = np.stack(contrib_chain(G, False)).astype(F)
            acc[:, :n - 1] = acc[:, :n - 1] + out[:, 1:]
        for i, q, T, Rz, tz in self.loops:
            G = self.loop_geom(q, T)
            for head, f in ((True, q), (False, T)):
                j = self.node(f)
                if j is not None:
                    acc[:, j] = acc[:, j] + np.stack(contrib_loop(G, head, i, q, T))[:, 0]
        return acc

    def gradient_and_blocks(self):
        p = self.p
        rho, lw = p["rotation_weight"], p["loop_weight"]
        meas = {i: (Rz, tz) for i, q, T, Rz, tz in self.loops}
        g = self.accumulate(lambda G, head: back(G, head, F(1), rho, residual(G, self.Rz, self.tz)),
                            lambda G, head, i, q, T: back(G, head, lw, rho, residual(G, *meas[i])))
        D = [[None] * 6 for _ in range(6)]
        for col in range(6):
            def chain(G, head, col=col):
                unit = _units(len(G[0][0]))[col]
                return back(G, head, F(1), rho, forward(G, None if head else unit, unit if head else None))

            def loop(G, head, i, q, T, col=col):
                unit = _units(1)[col]
                return back(G, head, lw, rho, forward(G, None if head else unit, unit if head else None))
            c = self.accumulate(chain, loop)
            for k in range(6):
                D[k][col] = c[k]
        return g, D

    def apply(self, vec):
        """H vec, edge by edge."""
        p = self.p
        rho, lw, n = p["rotation_weight"], p["loop_weight"], self.n
        pb = list(vec)
        pa = [np.concatenate([np.zeros(1, F), vec[k, :n - 1]]) for k in range(6)]
        get = self.scatter(vec)

        def chain(G, head):
            # the edge into node 0 has a held tail: v_a = 0 there, and 0 is what a None end subtracts
            u = forward(G, pa, pb)
            u0 = forward(G, None, pb)
            u = [np.where(self.held0, u0[k], u[k]) for k in range(6)]
            return back(G, head, F(1), rho, u)
        return self.accumulate(chain, lambda G, head, i, q, T: back(G, head, lw, rho, forward(G, get(T), get(q))))

    def solve_round(self):
        """PG-6: x of one round, or None when a block cannot be inverted."""
        g, D = self.gradient_and_blocks()
        Dinv, ok = invert_blocks(D)
        if not ok.all():
            return None
        n = self.n
        x = np.zeros((6, n), F)
        r = (-g).astype(F)
        z = np.stack(precondition(Dinv, list(r)))
        pv = z.copy()
        rz = total(dot6(list(r), list(z)))
        K = self.p["cg_iterations"] or min(n, MAX_CG)
        for _ in range(K):
            hp = self.apply(pv)
            php = total(dot6(list(pv), list(hp)))
            if not (np.isfinite(php) and php > 0):
                break
            alpha = rz / php
            x = x + alpha * pv
            r = r - alpha * hp
            z = np.stack(precondition(Dinv, list(r)))
            rz_new = total(dot6(list(r), list(z)))
            beta = rz_new / rz
            rz = rz_new
            pv = z + beta * pv
        return x

    def update(self, x):
        """PG-5: R <- one polar step of (I + [w]x) R, t <- t + v."""
        R, t = self.R, self.t
        M = [None] * 9
        for c in range(3):
            M[c] = R[c] + (x[1] * R[6 + c] - x[2] * R[3 + c])
            M[3 + c] = R[3 + c] + (x[2] * R[c] - x[0] * R[6 + c])
            M[6 + c] = R[6 + c] + (x[0] * R[3 + c] - x[1] * R[c])
        cof = _cof(M)
        det = (M[0] * cof[0] + M[1] * cof[1]) + M[2] * cof[2]
        ok = np.isfinite(det) & (det > 0)
        self.R = np.stack([np.where(ok, F(0.5) * (M[k] + cof[k] / det), M[k]) for k in range(9)]).astype(F)
        self.t = np.stack([t[k] + x[3 + k] for k in range(3)]).astype(F)

    def run(self):
        """PG-7: (status, cost_before, cost_after, the loop edges' own costs before, after)."""
        cost_before, own_before = self.cost()
        cost, status = cost_before, ORB_GRAPH_REFINED
        for _ in range(self.p["rounds"]):
            x = self.solve_round()
            if x is None:
                status = ORB_GRAPH_FAILED
                break
            keep = self.R, self.t
            self.update(x)
            after, _ = self.cost()
            if not (np.isfinite(after) and after < cost):
                self.R, self.t = keep
                status = ORB_GRAPH_STALLED
                break
            cost = after
        cost_after, own_after = self.cost()
        return status, cost_before, cost_after, own_before, own_after


def _cof(m):
    """pose_cof of orb_kernels_pose.h on a list of nine arrays."""
    return [m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6],
            m[7] * m[2] - m[8] * m[1], m[8] * m[0] - m[6] * m[2], m[6] * m[1] - m[7] * m[0],
            m[1] * m[5] - m[2] * m[4], m[2] * m[3] - m[0] * m[5], m[0] * m[4] - m[1] * m[3]]


# ---- PG-1 .. PG-8 ------------------------------------------------------------------------------------------------------------
def graph_pairs(frames, pairs, fixes, n_pairs=None, trace=None, **params):
    """frames: FRAME_POSE_DTYPE of the last trajectory call, all its frames; pairs: the list of the last match_pairs, (query,
    target) per entry; fixes: LOOP_FIX_DTYPE of the last loop_pairs.  `trace`: a dict that receives the Segment of every solved
    origin.  Returns (GRAPH_POSE_DTYPE (F,), GRAPH_EDGE_DTYPE (n_pairs,))."""
    p = defaults(**params)
    nF = len(frames)
    pairs = [(int(q), int(T)) for q, T in np.asarray(pairs).reshape(-1, 2)] if not isinstance(pairs, np.ndarray) or pairs.dtype.names is None \
        else [(int(e["query"]), int(e["target"])) for e in pairs]
    n = len(pairs) if n_pairs is None else n_pairs
    edges = np.zeros(n, GRAPH_EDGE_DTYPE)
    out = np.zeros(nF, GRAPH_POSE_DTYPE)
    by_origin = {}
    for i in range(n):
        q, T = pairs[i]
        edges[i]["verdict"] = v = verdict(frames, q, T, fixes[i], p)
        edges[i]["origin"] = fixes[i]["origin"]
        if v == ORB_GRAPH_EDGE_USED:
            Rz = [np.full(1, x, F) for x in fixes[i]["r"]]
            tz = [np.full(1, x, F) for x in fixes[i]["t"]]
            by_origin.setdefault(int(fixes[i]["origin"]), []).append((i, q, T, Rz, tz))
    with np.errstate(all="ignore"):
        for g in range(nF):
            out[g]["r"], out[g]["t"] = frames[g]["r"], frames[g]["t"]
            o = free_origin(frames, g)
            out[g]["status"] = ORB_GRAPH_HELD if o == NONE else \
                (ORB_GRAPH_INVALID if segment_invalid(frames, o, segment_nodes(frames, o)) else ORB_GRAPH_UNCHANGED)
        for o, loops in sorted(by_origin.items()):
            seg = Segment(frames, o, segment_nodes(frames, o), loops, p)
            status, cb, ca, own_b, own_a = seg.run()
            if trace is not None:
                trace[o] = seg
            for j in range(seg.n):
                rec = out[o + 1 + j]
                rec["r"], rec["t"] = seg.R[:, j], seg.t[:, j]
                rec["cost_before"], rec["cost_after"], rec["loops"], rec["status"] = cb, ca, len(loops), status
            for i in own_b:
                edges[i]["cost_before"], edges[i]["cost_after"] = own_b[i], own_a[i]
    return out, edges
