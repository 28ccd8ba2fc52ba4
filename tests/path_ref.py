"""Ground truth of mlm_query_paths (include/mlmap_hip.h) in plain Python integers, kept apart from the code under test: the trace
along the parent codes, vis with its tie subsets, the shortening, the table words and the length with math.sqrt and left-to-right
float adds.  Fields come from tests/route_ref.py and tests/reach_ref.py (genuine ones) or are written by hand.

A field is a uint8 array [z][y][x]; voxels are (x, y, z) tuples relative to the box unless said otherwise."""
import itertools
import math

import numpy as np

from tests import reach_ref, route_ref

REACH, ROUTE, ROW = 0, 1, 8
OFFSETS = route_ref.OFFSETS  # (dx, dy, dz) of the codes 0..25; the first six are reach_ref.CODES
assert [(dx, dy, dz) for dz, dy, dx in reach_ref.CODES] == OFFSETS[:6]


def seed_code(kind):
    return {REACH: reach_ref.SEED, ROUTE: route_ref.SEED}[kind]


class Field:
    """the bytes of a box as nested lists, with the contract's open()"""

    def __init__(self, parent, kind):
        p = np.asarray(parent, dtype=np.uint8)
        self.dz, self.dy, self.dx = p.shape
        self.M = seed_code(kind)
        self.code = p.tolist()

    def inside(self, v):
        return 0 <= v[0] < self.dx and 0 <= v[1] < self.dy and 0 <= v[2] < self.dz

    def open(self, v):
        return self.inside(v) and self.code[v[2]][v[1]][v[0]] <= self.M


def trace(F, goal, max_moves):
    """(status, [u_0 .. u_K]) of an open goal"""
    path = [tuple(goal)]
    while True:
        u = path[-1]
        c = F.code[u[2]][u[1]][u[0]]
        if c == F.M:
            return 1, path
        if len(path) - 1 == max_moves:
            return -1, path
        o = OFFSETS[c]
        v = (u[0] + o[0], u[1] + o[1], u[2] + o[2])
        if not F.open(v):
            return -2, path
        path.append(v)


def walk_sets(a, b):
    """the voxel sets vis(a, b) tests, one list per step of the walk: [(T, [voxels])]; T the tuple of axes that tie"""
    a, b = [int(v) for v in a], [int(v) for v in b]
    n = [abs(b[x] - a[x]) for x in range(3)]
    s = [(b[x] > a[x]) - (b[x] < a[x]) for x in range(3)]
    k = [0, 0, 0]
    c = list(a)
    out = []
    while tuple(c) != tuple(b):
        act = [x for x in range(3) if k[x] < n[x]]
        # the smallest (2 k_x + 1) / (2 n_x), by cross-multiplication
        best = act[0]
        for x in act[1:]:
            if (2 * k[x] + 1) * n[best] < (2 * k[best] + 1) * n[x]:
                best = x
        T = tuple(x for x in act if (2 * k[x] + 1) * n[best] == (2 * k[best] + 1) * n[x])
        vox = []
        for r in range(1, len(T) + 1):
            for S in itertools.combinations(T, r):
                vox.append(tuple(c[x] + (s[x] if x in S else 0) for x in range(3)))
        out.append((T, vox))
        for x in T:
            c[x] += s[x]
            k[x] += 1
    return out


def vis(F, a, b, seen_ties=None):
    """the contract's vis; seen_ties (a set) collects the sizes of the tie groups met before the answer was known"""
    for T, vox in walk_sets(a, b):
        if seen_ties is not None and len(T) > 1:
            seen_ties.add(len(T))
        if not all(F.open(v) for v in vox):
            return False
    return True


def shorten(F, path, L, seen_ties=None, counts=None):
    """the indices i_0 .. i_{W-1}; counts (a list of two) accumulates [candidates tested, candidates refused]"""
    K = len(path) - 1
    idx = [0]
    while idx[-1] < K:
        i = idx[-1]
        hi = min(K, i + L)
        best = i + 1
        for j in range(hi, i + 1, -1):
            ok = vis(F, path[i], path[j], seen_ties)
            if counts is not None:
                counts[0] += 1
                counts[1] += not ok
            if ok:
                best = j
                break
        idx.append(best)
    return idx


def kinds_of(path):
    """face, edge and corner moves"""
    n = [0, 0, 0]
    for p, q in zip(path[:-1], path[1:]):
        n[sum(1 for x in range(3) if p[x] != q[x]) - 1] += 1
    return n


def query(parent, kind, lo, goals, lookahead, max_moves, cap, d_sub, way=None, seen_ties=None, counts=None, detail=None):
    """the four outputs of the call: goals absolute (x, y, z); way: the initial content of the way3 buffer (n, cap, 3), zeros if None;
    detail (a list) receives per goal (path, idx) or None"""
    F = Field(parent, kind)
    g = np.asarray(goals, dtype=np.int64).reshape(-1, 3)
    n = len(g)
    out = {"status": np.zeros(n, dtype=np.int8), "way": np.zeros((n, cap, 3), dtype=np.int32) if way is None else np.array(way, dtype=np.int32),
           "length": np.full(n, -1.0, dtype=np.float64), "table": np.zeros((n, ROW), dtype=np.int64)}
    d = float(np.float32(d_sub))
    for i in range(n):
        v = tuple(int(g[i, x]) - int(lo[x]) for x in range(3))
        if not F.open(v):
            if detail is not None:
                detail.append(None)
            continue
        st, path = trace(F, v, max_moves)
        out["status"][i] = st
        out["table"][i, 0] = len(path) - 1
        if st != 1:
            if detail is not None:
                detail.append(None)
            continue
        idx = shorten(F, path, lookahead, seen_ties, counts)
        if detail is not None:
            detail.append((path, idx))
        K, W = len(path) - 1, len(idx)
        acc = 0.0
        for t in range(W - 1):
            p, q = path[idx[t]], path[idx[t + 1]]
            sq = sum((q[x] - p[x]) ** 2 for x in range(3))
            acc = acc + (d * math.sqrt(float(sq)))
        out["length"][i] = acc
        for t in range(min(W, cap)):
            out["way"][i, t] = [path[idx[t]][x] + int(lo[x]) for x in range(3)]
        legs = [idx[t + 1] - idx[t] for t in range(W - 1)]
        out["table"][i, 1:7] = [W, *kinds_of(path), max(legs, default=0), sum(min(K, idx[t] + lookahead) - idx[t + 1] for t in range(W - 1))]
    return out
