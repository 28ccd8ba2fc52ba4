"""Ground truth of mlm_export_mesh in plain numpy, written from the contract in include/mlmap_hip.h, and three properties a mesh
must have whatever produced it.

Classes: occ 0 OCCUPIED, 1 FREE, -1 UNKNOWN; infl 0 OCCUPIED, else -1 (what mlm_export_window's channels return), arrays [z][y][x]."""
import numpy as np

OCC, INFL, UNKNOWN, SEEN, CLOSED = 1, 2, 4, 16, 32
ROW = 12
E = np.eye(3, dtype=np.int64)  # e_x, e_y, e_z as (x, y, z)


def corners(v, a):
    """the four lattice points (x, y, z) of face a of voxel v, counter-clockwise seen from the open side"""
    u = a >> 1
    p, q = (u + 1) % 3, (u + 2) % 3
    b = np.asarray(v, dtype=np.int64) + (a & 1) * E[u]
    return [b, b + E[p], b + E[p] + E[q], b + E[q]] if a & 1 else [b, b + E[q], b + E[p] + E[q], b + E[p]]


def normal(a):
    return (1 if a & 1 else -1) * E[a >> 1]


def mesh(occ, infl, lo, flags, n=10, d=0.1):
    """every output of mlm_export_mesh for the box whose grown-by-one-voxel classes are occ / infl ([D2 + 2][D1 + 2][D0 + 2]) at
    origin lo (the box's, not the grown box's); n, d: subbox_n, subbox_d_xyz of the map"""
    occ, infl = np.asarray(occ), np.asarray(infl)
    D = [occ.shape[2] - 2, occ.shape[1] - 2, occ.shape[0] - 2]
    obstacle = np.zeros(occ.shape, dtype=bool)
    if flags & OCC:
        obstacle |= occ == 0
    if flags & INFL:
        obstacle |= infl == 0
    if flags & UNKNOWN:
        obstacle |= occ == -1
    is_open = ~obstacle
    if flags & SEEN:
        is_open &= occ == 1
    inside = np.zeros(occ.shape, dtype=bool)
    inside[1:-1, 1:-1, 1:-1] = True
    if flags & CLOSED:
        obstacle &= inside
        is_open |= ~inside
    # face (v, a): v in the box, O(v), open(v + e_a); has[z][y][x][a], so that its flat index is linear(v) * 6 + a
    core = obstacle[1:-1, 1:-1, 1:-1]
    sl = [slice(0, -2), slice(1, -1), slice(2, None)]  # neighbour at -1, 0, +1 in grown coordinates
    has = np.zeros(core.shape + (6,), dtype=bool)
    for a in range(6):
        dx, dy, dz = normal(a)
        has[..., a] = core & is_open[sl[dz + 1], sl[dy + 1], sl[dx + 1]]
    summary = np.zeros(ROW, dtype=np.int64)
    summary[2] = core.sum()
    summary[3] = has.any(axis=-1).sum()
    summary[4:10] = has.reshape(-1, 6).sum(axis=0)
    faces = []  # (linear(v) * 6 + a, x, y, z, a), box coordinates, ascending
    for key in np.flatnonzero(has):
        a, lin = int(key % 6), int(key // 6)
        x, y, z = lin % D[0], lin // D[0] % D[1], lin // (D[0] * D[1])
        faces.append((int(key), x, y, z, a))
        ux, uy, uz = np.array([x, y, z]) + normal(a)
        summary[10] += not (0 <= ux < D[0] and 0 <= uy < D[1] and 0 <= uz < D[2])
    F = len(faces)
    lat = {}  # lattice linear index -> normal sum
    quad_lat = np.zeros((F, 4), dtype=np.int64)
    for f, (_, x, y, z, a) in enumerate(faces):
        for i, k in enumerate(corners((x, y, z), a)):
            L = (k[2] * (D[1] + 1) + k[1]) * (D[0] + 1) + k[0]
            quad_lat[f, i] = L
            lat[L] = lat.get(L, np.zeros(3, dtype=np.int64)) + normal(a)
    order = np.array(sorted(lat), dtype=np.int64)
    V = len(order)
    quads = np.searchsorted(order, quad_lat).astype(np.int32).reshape(F, 4)
    face4 = np.array([[lo[0] + x, lo[1] + y, lo[2] + z, a] for _, x, y, z, a in faces], dtype=np.int32).reshape(F, 4)
    k = np.stack([order % (D[0] + 1), order // (D[0] + 1) % (D[1] + 1), order // ((D[0] + 1) * (D[1] + 1))], axis=1).reshape(V, 3)
    k = k + np.asarray(lo, dtype=np.int64)
    g = np.floor_divide(k, n)
    xyz = (g.astype(np.float64) * (d * n) + (k - g * n).astype(np.float64) * d).astype(np.float32)
    n3 = np.array([lat[L] for L in order], dtype=np.int8).reshape(V, 3)
    summary[0], summary[1] = F, V
    return {"quads": quads, "faces": face4, "verts": k.astype(np.int32), "xyz": xyz, "normals": n3, "summary": summary}


# ---- properties of any mesh ---------------------------------------------------------------------------------------------------
def quad_normals(m):
    """(c1 - c0) x (c3 - c0) of every quad, from the lattice coordinates of its vertices"""
    c = m["verts"].astype(np.int64)[m["quads"]]
    return np.cross(c[:, 1] - c[:, 0], c[:, 3] - c[:, 0])


def face_normals(m):
    a = m["faces"][:, 3]
    out = np.zeros((len(a), 3), dtype=np.int64)
    out[np.arange(len(a)), a >> 1] = np.where(a & 1, 1, -1)
    return out


def enclosed_voxels(m):
    """the divergence theorem on the x faces: sum of the planes of the +x faces minus that of the -x faces"""
    f = m["faces"].astype(np.int64)
    return int((f[f[:, 3] == 1, 0] + 1).sum() - f[f[:, 3] == 0, 0].sum())


def odd_edges(m):
    """lattice edges used by an odd number of faces (none on a closed surface)"""
    q = m["quads"].astype(np.int64)
    e = np.concatenate([np.stack([q[:, i], q[:, (i + 1) % 4]], axis=1) for i in range(4)])
    e.sort(axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True) if len(e) else (None, np.zeros(0, dtype=np.int64))
    return int((cnt % 2).sum())


def check_properties(m, flags):
    """every quad's normal is its face's direction; a CLOSED mesh encloses exactly the obstacle voxels and uses every lattice edge an
    even number of times (not with SEEN, which leaves the surface open towards voxels inside the box that are not FREE)"""
    assert np.array_equal(quad_normals(m), face_normals(m))
    if flags & CLOSED and not flags & SEEN:
        assert enclosed_voxels(m) == m["summary"][2]
        assert odd_edges(m) == 0


def vertex_normals_from_faces(m):
    """the normal sums rebuilt from quads and faces"""
    out = np.zeros((len(m["verts"]), 3), dtype=np.int64)
    fn = face_normals(m)
    for i in range(4):
        np.add.at(out, m["quads"][:, i], fn)
    return out
