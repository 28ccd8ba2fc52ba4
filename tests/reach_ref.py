"""Ground truth of mlm_export_reach (include/mlmap_hip.h) in plain numpy, kept apart from the code under test.

reach(T, seeds, max_steps): `steps` by a wavefront breadth-first search over index arrays of the traversable mask T ([z][y][x],
seeds as (x, y, z) relative to the box), `parent` by the header's rule applied literally to that field, and the summary counters.
blocked(obstacles_grown, r): the blocked mask of clearance r from the obstacle mask of the box grown by r + 1 per side, by the
separable truncated transform (edt_separable, the form of tests/esdf_ref.py that tests/test_gpu_esdf.py checks against the definition).
Mask builders for the crafted cases: serpentine slabs and the layered 3-D maze."""
import numpy as np

NONE, SEED = -1, 6
# neighbour codes 0: -x, 1: +x, 2: -y, 3: +y, 4: -z, 5: +z as (dz, dy, dx)
CODES = [(0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)]


def edt_separable(mask, C):
    """min(C^2, squared distance to the nearest True of mask) per voxel, by three 1-D truncated passes; exact wherever every
    voxel within C - 1 on each axis is inside the array"""
    C2 = C * C
    f = np.where(mask, 0, C2).astype(np.uint16)
    for axis in (2, 1, 0):
        g = f.copy()
        for k in range(1, C):
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[axis], b[axis] = slice(0, -k), slice(k, None)
            a, b = tuple(a), tuple(b)
            np.minimum(g[a], f[b] + np.uint16(k * k), out=g[a])
            np.minimum(g[b], f[a] + np.uint16(k * k), out=g[b])
        f = g
    return f.astype(np.int32)


def blocked(obstacles_grown, r):
    """blocked mask of the box from the obstacle mask of the box grown by r + 1 voxels per side: some obstacle within r^2"""
    if r == 0:
        return obstacles_grown[1:-1, 1:-1, 1:-1].copy()
    g = r + 1
    return (edt_separable(obstacles_grown, r + 1) <= r * r)[g:-g, g:-g, g:-g]


def reach(T, seeds, max_steps=None):
    """{"steps", "parent", "summary" [traversable, reached, largest steps]} of the box whose traversable mask is T"""
    T = np.asarray(T, dtype=bool)
    dz, dy, dx = T.shape
    pad = np.zeros((dz + 2, dy + 2, dx + 2), dtype=bool)  # a blocked rim: no bounds checks, and a path never leaves the box
    pad[1:-1, 1:-1, 1:-1] = T
    sy, sz = dx + 2, (dx + 2) * (dy + 2)
    flat_T = pad.ravel()
    st = np.full(flat_T.size, NONE, dtype=np.int64)
    s = np.asarray(seeds, dtype=np.int64).reshape(-1, 3)
    inside = ((s >= 0) & (s < np.array([dx, dy, dz]))).all(1)
    s = s[inside]
    front = np.unique((s[:, 2] + 1) * sz + (s[:, 1] + 1) * sy + s[:, 0] + 1)
    front = front[flat_T[front]]
    st[front] = 0
    offs = np.array([-1, 1, -sy, sy, -sz, sz], dtype=np.int64)
    k = 0
    limit = np.iinfo(np.int64).max if max_steps is None else int(max_steps)
    while len(front) and k < limit:
        k += 1
        nb = (front[:, None] + offs[None, :]).ravel()
        nb = nb[flat_T[nb] & (st[nb] == NONE)]
        front = np.unique(nb)
        st[front] = k
    steps = st.reshape(pad.shape)
    # parent: the lowest code whose neighbour (in the box) has steps - 1; 6 at seeds; 255 where not reached
    parent = np.full(pad.shape, 255, dtype=np.uint8)
    core = (slice(1, -1),) * 3
    p, sc = parent[core], steps[core]
    p[sc == 0] = SEED
    for c, (oz, oy, ox) in enumerate(CODES):
        nbv = steps[1 + oz:dz + 1 + oz, 1 + oy:dy + 1 + oy, 1 + ox:dx + 1 + ox]
        p[(sc > 0) & (p == 255) & (nbv == sc - 1)] = c
    sc = sc.astype(np.int32)
    reached = sc >= 0
    summary = np.array([T.sum(), reached.sum(), sc.max() if reached.any() else -1], dtype=np.int64)
    return {"steps": np.ascontiguousarray(sc), "parent": np.ascontiguousarray(p), "summary": summary}


def walk(parent, v):
    """the path that `parent` describes from voxel v = (x, y, z) to a seed (the client's ten-line loop)"""
    path = [tuple(v)]
    while parent[path[-1][2], path[-1][1], path[-1][0]] != SEED:
        x, y, z = path[-1]
        c = parent[z, y, x]
        assert c < 6
        oz, oy, ox = CODES[c]
        path.append((x + ox, y + oy, z + oz))
    return path


def serpentine_slab(nx, ny, nz=1):
    """blocked mask [nz][ny][nx]: a wall in every odd row y with a one-voxel gap at alternating ends, the same in every layer"""
    b = np.zeros((nz, ny, nx), dtype=bool)
    for y in range(1, ny, 2):
        b[:, y, :] = True
        b[:, y, nx - 1 if (y // 2) % 2 == 0 else 0] = False
    return b


def serpentine_3d(n):
    """blocked mask [n][n][n]: even z layers are serpentine slabs, odd layers solid except one hole, placed alternately over the
    end and over the start of the layer below, so that the only path runs every layer end to end"""
    b = np.zeros((n, n, n), dtype=bool)
    b[0::2] = serpentine_slab(n, n)[0]
    # end of a slab's path when entered at (0, 0): the last even row, at the side its parity leaves it on
    rows = (n + 1) // 2
    last_y = 2 * (rows - 1)
    end_x = n - 1 if rows % 2 == 1 else 0
    for z in range(1, n, 2):
        b[z] = True
        if (z // 2) % 2 == 0:
            b[z, last_y, end_x] = False
        else:
            b[z, 0, 0] = False
    return b
