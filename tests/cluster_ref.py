"""Ground truth of mlm_export_clusters (include/mlmap_hip.h) in plain numpy, kept apart from the code under test.

frontier_set(occ_grown): the frontier set of a box from the occ classes (-1 UNKNOWN, 0 OCCUPIED, 1 FREE) of the box grown by one
voxel per side.  class_set(occ, infl, ...): the class sets (mlm_export_esdf's predicate).  clusters(S, ...): components by a
breadth-first search over index arrays from the smallest voxel not yet visited (so components come out in root order), then
numbering, labels, table and summary by the header's rules applied literally.  Mask builders for the crafted cases."""
import numpy as np

from tests.reach_ref import serpentine_3d, serpentine_slab  # noqa: F401  (mask builders shared with the reach tests)

NONE, SMALL, ROW = -1, -2, 16
FRONTIER = 16


def offsets(connectivity):
    """the moves (dz, dy, dx) of a connectivity: 1, at most 2, at most 3 non-zero entries"""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 1 <= (dz != 0) + (dy != 0) + (dx != 0) <= most]


def frontier_set(occ_grown):
    """S of the box [1:-1]^3: FREE and at least one of the six face neighbours UNKNOWN"""
    o = np.asarray(occ_grown)
    c = o[1:-1, 1:-1, 1:-1]
    unk = o == -1
    nb = (unk[1:-1, 1:-1, :-2] | unk[1:-1, 1:-1, 2:] | unk[1:-1, :-2, 1:-1] | unk[1:-1, 2:, 1:-1] | unk[:-2, 1:-1, 1:-1] |
          unk[2:, 1:-1, 1:-1])
    return (c == 1) & nb


def class_set(occ, infl, use_occ=False, use_infl=False, use_unknown=False):
    s = np.zeros(np.shape(occ), dtype=bool)
    if use_occ:
        s |= np.asarray(occ) == 0
    if use_infl:
        s |= np.asarray(infl) == 0
    if use_unknown:
        s |= np.asarray(occ) == -1
    return s


def components(S, connectivity):
    """(comp, n): comp int64 [z][y][x], the component's index in root order (-1 off S); n components"""
    S = np.asarray(S, dtype=bool)
    dz, dy, dx = S.shape
    pad = np.zeros((dz + 2, dy + 2, dx + 2), dtype=bool)  # a rim off S: no bounds checks, and a chain never leaves the box
    pad[1:-1, 1:-1, 1:-1] = S
    sy, sz = dx + 2, (dx + 2) * (dy + 2)
    flat = pad.ravel()
    comp = np.full(flat.size, -1, dtype=np.int64)
    offs = np.array([oz * sz + oy * sy + ox for oz, oy, ox in offsets(connectivity)], dtype=np.int64)
    cand = np.flatnonzero(flat)  # ascending padded index = ascending box index
    n, ptr = 0, 0
    while ptr < len(cand):
        blk = cand[ptr:ptr + 4096]
        free = np.flatnonzero(comp[blk] < 0)
        if len(free) == 0:
            ptr += len(blk)
            continue
        ptr += int(free[0])
        front = cand[ptr:ptr + 1]
        comp[front] = n
        while len(front):
            nb = (front[:, None] + offs[None, :]).ravel()
            nb = nb[flat[nb] & (comp[nb] < 0)]
            front = np.unique(nb)
            comp[front] = n
        n += 1
        ptr += 1
    return comp.reshape(pad.shape)[1:-1, 1:-1, 1:-1].copy(), n


def clusters(S, connectivity=26, min_size=1, cap=None, lo=(0, 0, 0)):
    """{"labels" int32 [z][y][x], "table" int64 (min(K, cap), 16), "summary" int64 [voxels of S, components, K, voxels in kept
    components, largest component]}; cap None: every row"""
    S = np.asarray(S, dtype=bool)
    dz, dy, dx = S.shape
    comp, n = components(S, connectivity)
    inS = comp >= 0
    ids = comp[inS]
    size = np.bincount(ids, minlength=n).astype(np.int64)
    kept = size >= min_size
    number = np.where(kept, np.cumsum(kept) - 1, SMALL)
    K = int(kept.sum())
    labels = np.full(S.shape, NONE, dtype=np.int32)
    labels[inS] = number[ids]
    rows = K if cap is None else min(K, cap)
    table = np.zeros((rows, ROW), dtype=np.int64)
    z, y, x = np.nonzero(labels >= 0)
    k = labels[z, y, x].astype(np.int64)
    sel = k < rows
    z, y, x, k = z[sel].astype(np.int64), y[sel].astype(np.int64), x[sel].astype(np.int64), k[sel]
    if rows:
        lin = (z * dy + y) * dx + x
        root = np.full(rows, np.iinfo(np.int64).max)
        np.minimum.at(root, k, lin)
        table[:, 0] = size[kept][:rows]
        table[:, 1:4] = np.stack([root % dx, (root // dx) % dy, root // (dx * dy)], 1) + np.asarray(lo, dtype=np.int64)
        for a, v in enumerate((x, y, z)):
            mn = np.full(rows, np.iinfo(np.int64).max)
            mx = np.full(rows, np.iinfo(np.int64).min)
            sm = np.zeros(rows, dtype=np.int64)
            np.minimum.at(mn, k, v)
            np.maximum.at(mx, k, v)
            np.add.at(sm, k, v)
            table[:, 4 + a] = mn + lo[a]
            table[:, 7 + a] = mx + lo[a]
            table[:, 10 + a] = sm
        faces = ((x == 0) * 1 | (x == dx - 1) * 2 | (y == 0) * 4 | (y == dy - 1) * 8 | (z == 0) * 16 | (z == dz - 1) * 32).astype(np.int64)
        fb = np.zeros(rows, dtype=np.int64)
        np.bitwise_or.at(fb, k, faces)
        table[:, 13] = fb
    summary = np.array([inS.sum(), n, K, size[kept].sum(), size.max() if n else 0], dtype=np.int64)
    return {"labels": labels, "table": table, "summary": summary}


def checkerboard(shape):
    """voxels with even x + y + z: no two share a face"""
    z, y, x = np.indices(shape)
    return (x + y + z) % 2 == 0
