"""Ground truth of mlm_query_views (include/mlmap_hip.h) for tests/test_view_plan.py and tests/test_gpu_views.py: the sets of the
header's contract as plain Python sets over the walk of tests/raywalk_ref.py (valid / path) and voxel classes from a block dump
(raywalk_ref.block_classes) or any other callable; a generator of pinhole fans at random poses in free space.  Nothing here calls the
code under test."""
import numpy as np

from tests import raywalk_ref as rw

ROW = 8
LIMIT = 2 ** 31 - 1


def walk(p0, p1, view_begin, d, classes):
    """the paths of all rays, walked once for every flag set: per view a list of None (invalid ray) or (voxels [K, 3] int64, class
    bits [K])"""
    vb = [int(x) for x in view_begin]
    out = []
    for k in range(len(vb) - 1):
        rays = []
        for i in range(vb[k], vb[k + 1]):
            Q = rw.valid(p0[i], p1[i], d)
            if Q is None:
                rays.append(None)
                continue
            pth, _ = rw.path(*Q)
            vox = np.array([v for v, _ in pth], dtype=np.int64)
            rays.append((vox, classes(vox)))
        out.append(rays)
    return out


def account(walked, flags, box=None, exclude=None, mark=None):
    """(table int64 [n_views, 8], mark) of the walked views: box = (lo, dims) or None, exclude / mark uint8 (dz, dy, dx) of the box
    or None; mark is updated in place and returned"""
    table = np.zeros((len(walked), ROW), dtype=np.int64)
    if box is not None:
        lo, dims = [int(x) for x in box[0]], [int(x) for x in box[1]]
    inside = (lambda v: all(lo[a] <= v[a] < lo[a] + dims[a] for a in range(3))) if box is not None else (lambda v: True)
    at = lambda v: (v[2] - lo[2], v[1] - lo[1], v[0] - lo[0])
    for k, rays in enumerate(walked):
        A, S, cls = set(), set(), {}
        stopped = invalid = steps = 0
        b_lo, b_hi = None, None
        for r in rays:
            if r is None:
                invalid += 1
                continue
            vox, bits = r
            hit = np.flatnonzero(bits & flags)
            n_steps = int(hit[0]) if hit.size else len(vox)
            tv = [tuple(v) for v in vox[:n_steps + 1].tolist()]
            for v, c in zip(tv, bits[:n_steps + 1].tolist()):
                cls[v] = c
            A.update(tv[:n_steps])
            if hit.size:
                S.add(tv[n_steps])
                stopped += 1
            steps += n_steps
            ends = np.stack([vox[0], vox[-1]])
            b_lo = ends.min(0) if b_lo is None else np.minimum(b_lo, ends.min(0))
            b_hi = ends.max(0) if b_hi is None else np.maximum(b_hi, ends.max(0))
        assert not (A & S)  # (the stop predicate is a function of the voxel alone)
        if b_lo is not None:  # the bounding box of the start and end voxels, cut to the box: refused beyond 2^31 - 1 voxels
            l, h = [int(x) for x in b_lo], [int(x) for x in b_hi]
            if box is not None:
                l, h = [max(l[a], lo[a]) for a in range(3)], [min(h[a], lo[a] + dims[a] - 1) for a in range(3)]
            if all(h[a] >= l[a] for a in range(3)) and (h[0] - l[0] + 1) * (h[1] - l[1] + 1) * (h[2] - l[2] + 1) > LIMIT:
                table[k, 7] = 1
                continue
        A = {v for v in A if inside(v)}
        S = {v for v in S if inside(v)}
        if mark is not None:
            for v in A:
                mark[at(v)] |= 1
            for v in S:
                mark[at(v)] |= 2
        if exclude is not None:
            A = {v for v in A if not exclude[at(v)]}
            S = {v for v in S if not exclude[at(v)]}
        table[k, 0] = len(A)
        table[k, 1] = sum(1 for v in A if cls[v] & rw.UNKNOWN)
        table[k, 2] = sum(1 for v in A if not cls[v] & (rw.UNKNOWN | rw.OCC))
        table[k, 3] = len(S)
        table[k, 4], table[k, 5], table[k, 6] = stopped, invalid, steps
    return table, mark


def views(p0, p1, view_begin, d, classes, flags, box=None, exclude=None, mark=None):
    return account(walk(p0, p1, view_begin, d, classes), flags, box, exclude, mark)


def assert_equal(got_table, exp_table, got_mark=None, exp_mark=None, what=""):
    g, e = np.asarray(got_table), np.asarray(exp_table)
    assert g.shape == e.shape and g.dtype == np.int64, (what, g.shape, g.dtype, e.shape)
    bad = np.flatnonzero((g != e).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(g)} rows differ, first #{bad[0]}: {g[bad[0]].tolist()} vs {e[bad[0]].tolist()}"
    if exp_mark is not None:
        gm, em = np.asarray(got_mark), np.asarray(exp_mark)
        assert gm.shape == em.shape and gm.dtype == np.uint8, (what, gm.shape, gm.dtype, em.shape)
        assert np.array_equal(gm, em), f"{what}: {(gm != em).sum()} mark bytes differ"


def non_vacuous(table):
    """over views of 64 x 48 fans of 4 m at d = 0.1, walked with OCC: a library that sums instead of de-duplicating cannot pass, and
    gains and surfaces are there to be counted"""
    t = np.asarray(table)
    seen = t[:, 0] + t[:, 3]
    assert (t[:, 6] >= 2 * seen).sum() * 2 >= len(t), (t[:, 6] / np.maximum(seen, 1)).tolist()
    assert ((t[:, 1] > 0) & (t[:, 3] > 0)).sum() * 3 >= len(t), t[:, [1, 3]].tolist()


# ---- fans -------------------------------------------------------------------------------------------------------------------------
def fan(width, height, hfov, vfov, max_range):
    """end points of a pinhole camera's pixel-centre rays in the sensor frame (x right, y down, z forward), each max_range long"""
    fx, fy = 0.5 * width / np.tan(0.5 * hfov), 0.5 * height / np.tan(0.5 * vfov)
    u, v = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    dirs = np.stack([(u - 0.5 * width) / fx, (v - 0.5 * height) / fy, np.ones(u.shape)], axis=-1).reshape(-1, 3)
    return dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * max_range


def rotation(yaw, pitch):
    """sensor to world: the optical axis at yaw about z and pitch up from the horizontal, x to the right, y down"""
    fwd = np.array([np.cos(yaw) * np.cos(pitch), np.sin(yaw) * np.cos(pitch), np.sin(pitch)])
    right = np.array([np.sin(yaw), -np.cos(yaw), 0.0])
    return np.stack([right, np.cross(fwd, right), fwd], axis=1)


def free_origins(rng, b, cfg, count):
    """positions inside FREE voxels of the block dump (not released blocks), away from the voxel faces"""
    n, d = cfg.subbox_n, cfg.subbox_d_xyz
    live = np.flatnonzero(~np.asarray(b["collapsed"]).astype(bool))
    blk, cid = np.nonzero(np.asarray(b["occ"])[live] == ord("f"))
    assert len(blk) >= count
    pick = rng.choice(len(blk), count, replace=False)
    g = np.asarray(b["keys"], dtype=np.int64)[live[blk[pick]]]
    c = np.stack([cid[pick] % n, (cid[pick] // n) % n, cid[pick] // (n * n)], axis=1)
    return (g * n + c + rng.uniform(0.2, 0.8, size=(count, 3))) * d


def random_fans(rng, b, cfg, count, width, height, max_range, hfov=np.deg2rad(90.0), vfov=np.deg2rad(70.0)):
    """(p0, p1, view_begin, origins, rotations, fan): `count` views of one fan from random origins in free space, any yaw, pitch
    within +-0.5 rad"""
    f = fan(width, height, hfov, vfov, max_range)
    org = free_origins(rng, b, cfg, count)
    R = np.stack([rotation(rng.uniform(-np.pi, np.pi), rng.uniform(-0.5, 0.5)) for _ in range(count)]) if count else np.zeros((0, 3, 3))
    p1 = org[:, None, :] + np.einsum("kij,mj->kmi", R, f)
    p0 = np.broadcast_to(org[:, None, :], p1.shape)
    vb = (np.arange(count + 1) * len(f)).astype(np.int32)
    return np.ascontiguousarray(p0).reshape(-1, 3), np.ascontiguousarray(p1).reshape(-1, 3), vb, org, R, f
