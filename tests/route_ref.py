"""Ground truth of mlm_export_route (include/mlmap_hip.h) in plain numpy, kept apart from the code under test.

classes(obstacles_grown, r, n_penalty): the class byte of every voxel of the box (255 blocked, else its ring min(k, n_penalty)) from
the obstacle mask of the box grown by r + n_penalty + 1 per side, by the exact truncated squared-distance transform of
tests/reach_ref.py (edt_separable).
route(cls, seeds, ...): `cost` by a vectorised label-correcting relaxation over shifted arrays, iterated until nothing changes
(exact in integers; the permitted-move masks are built from the definition), `parent` by the header's rule applied literally to
that field, and the summary counters.  dijkstra(cls, seeds, ...): the cost alone by a plain heapq Dijkstra that tests every move
against the definition voxel by voxel — a second, independent form.  walk(parent, v): the path `parent` describes."""
import heapq
import itertools

import numpy as np

from tests.reach_ref import edt_separable

NONE, SEED, BLOCKED = -1, 26, 255


def _offsets():
    """(dx, dy, dz) of the codes 0..25: the faces -x, +x, -y, +y, -z, +z, then the offsets with two and with three non-zero entries,
    each group in ascending lexicographic order of (dz, dy, dx)"""
    faces = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    rest = [(dx, dy, dz) for dz, dy, dx in itertools.product((-1, 0, 1), repeat=3)]  # (product varies the last entry fastest)
    return faces + [o for o in rest if np.count_nonzero(o) == 2] + [o for o in rest if np.count_nonzero(o) == 3]


OFFSETS = _offsets()


def intermediates(o):
    """the offsets obtained from o by zeroing a non-empty proper subset of its non-zero entries"""
    nz = [a for a in range(3) if o[a]]
    out = []
    for k in range(1, len(nz)):
        for zero in itertools.combinations(nz, k):
            out.append(tuple(0 if a in zero else o[a] for a in range(3)))
    return out


def classes(obstacles_grown, r, n_penalty):
    """class byte [z][y][x] of the box from the obstacle mask of the box grown by g = r + n_penalty + 1 voxels per side"""
    g = r + n_penalty + 1
    d = edt_separable(obstacles_grown, g)[g:-g, g:-g, g:-g]
    cls = np.full(d.shape, n_penalty, dtype=np.uint8)
    for k in range(n_penalty - 1, -1, -1):
        cls[d <= (r + 1 + k) ** 2] = k
    cls[d <= r * r] = BLOCKED
    return cls


def pen_of(cls, penalty):
    """entry penalty per voxel (0 beyond the rings and where blocked)"""
    tab = np.zeros(256, dtype=np.int64)
    tab[:len(penalty)] = penalty
    tab[BLOCKED] = 0
    return tab[cls]


def _shift(a, o, fill):
    """b[v] = a[v + o] ([z][y][x] arrays, o = (dx, dy, dz)), `fill` where v + o leaves the array"""
    b = np.full(a.shape, fill, dtype=a.dtype)
    src, dst = [], []
    for n, d in zip(a.shape, (o[2], o[1], o[0])):
        src.append(slice(max(d, 0), n + min(d, 0)))
        dst.append(slice(max(-d, 0), n + min(-d, 0)))
    b[tuple(dst)] = a[tuple(src)]
    return b


def permitted(T, o):
    """mask of the voxels v for which the move between v and v + o is permitted (T: traversable, False outside the box)"""
    m = T & _shift(T, o, False)
    for q in intermediates(o):
        m &= _shift(T, q, False)
    return m


def effective_seeds(T, seeds):
    dz, dy, dx = T.shape
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 3)
    s = s[((s >= 0) & (s < np.array([dx, dy, dz]))).all(1)]
    return np.unique(s[T[s[:, 2], s[:, 1], s[:, 0]]], axis=0)


def route(cls, seeds, connectivity=26, move_cost=(10, 14, 17), penalty=(), max_cost=None):
    """{"cost", "parent", "summary" [traversable, reached, largest cost]} of the box with class bytes cls; seeds (x, y, z) relative to the box"""
    cls = np.asarray(cls, dtype=np.uint8)
    T = cls != BLOCKED
    pen = pen_of(cls, penalty)
    INF = np.int64(1) << 60
    cost = np.full(T.shape, INF, dtype=np.int64)
    s = effective_seeds(T, seeds)
    cost[s[:, 2], s[:, 1], s[:, 0]] = 0
    moves = [(c, o, permitted(T, o), move_cost[np.count_nonzero(o) - 1]) for c, o in enumerate(OFFSETS[:connectivity])]
    changed = len(s) > 0
    while changed:
        changed = False
        for _, o, ok, w in moves:
            cand = _shift(cost, o, INF) + w + pen
            better = ok & (cand < cost)
            if better.any():
                cost[better] = cand[better]
                changed = True
    reached = cost < INF
    # parent: the lowest code whose move is permitted and whose voxel explains the cost; 26 at seeds; 255 where not reached
    parent = np.full(T.shape, 255, dtype=np.uint8)
    for c, o, ok, w in reversed(moves):
        parent[reached & ok & (_shift(cost, o, INF) + w + pen == cost)] = c
    parent[s[:, 2], s[:, 1], s[:, 0]] = SEED
    full = {"cost": np.where(reached, cost, NONE), "parent": parent, "summary": np.array([T.sum(), 0, 0], dtype=np.int64)}
    return truncate(full, 2 ** 31 - 1 if max_cost is None else int(max_cost))


def truncate(full, max_cost):
    """the result at max_cost from a result at a larger one: every value above max_cost cut away (all weights are positive, so
    every voxel before a kept one on its path is kept too)"""
    keep = (full["cost"] >= 0) & (full["cost"] <= max_cost)
    cost = np.where(keep, full["cost"], NONE).astype(np.int32)
    summary = np.array([full["summary"][0], keep.sum(), cost.max() if keep.any() else -1], dtype=np.int64)
    return {"cost": np.ascontiguousarray(cost), "parent": np.where(keep, full["parent"], 255).astype(np.uint8), "summary": summary}


def dijkstra(cls, seeds, connectivity=26, move_cost=(10, 14, 17), penalty=(), max_cost=None):
    """the cost field alone, voxel by voxel: a binary heap, every move tested against the definition"""
    cls = np.asarray(cls, dtype=np.uint8)
    dz, dy, dx = cls.shape

    def trav(x, y, z):
        return 0 <= x < dx and 0 <= y < dy and 0 <= z < dz and cls[z, y, x] != BLOCKED

    pen = [int(p) for p in penalty]
    best = {}
    heap = []
    for x, y, z in np.asarray(seeds, dtype=np.int64).reshape(-1, 3).tolist():
        if trav(x, y, z) and (x, y, z) not in best:
            best[(x, y, z)] = 0
            heap.append((0, x, y, z))
    heapq.heapify(heap)
    inter = [intermediates(o) for o in OFFSETS]
    while heap:
        c, x, y, z = heapq.heappop(heap)
        if c > best[(x, y, z)]:
            continue
        for k, o in enumerate(OFFSETS[:connectivity]):
            v = (x + o[0], y + o[1], z + o[2])
            if not trav(*v) or not all(trav(x + q[0], y + q[1], z + q[2]) for q in inter[k]):
                continue
            ring = int(cls[v[2], v[1], v[0]])
            n = c + move_cost[np.count_nonzero(o) - 1] + (pen[ring] if ring < len(pen) else 0)
            if n < best.get(v, 1 << 60):
                best[v] = n
                heapq.heappush(heap, (n, *v))
    out = np.full(cls.shape, NONE, dtype=np.int32)
    limit = 2 ** 31 - 1 if max_cost is None else int(max_cost)
    for (x, y, z), c in best.items():
        if c <= limit:
            out[z, y, x] = c
    return out


def walk(parent, v):
    """the path that `parent` describes from voxel v = (x, y, z) to a seed"""
    path = [tuple(int(a) for a in v)]
    while parent[path[-1][2], path[-1][1], path[-1][0]] != SEED:
        x, y, z = path[-1]
        c = parent[z, y, x]
        assert c < 26
        o = OFFSETS[c]
        path.append((x + o[0], y + o[1], z + o[2]))
    return path
