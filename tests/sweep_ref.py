"""Ground truth of mlm_query_sweeps (include/mlmap_hip.h) for tests/test_sweep_plan.py and tests/test_gpu_sweeps.py: the contract in
plain Python integers on top of tests/raywalk_ref.py (its path and its block classes).  The full ball is tested at every path voxel:
nothing here knows of caps, of column tables or of the search of mlm_nearest.h, and nothing calls the code under test.  (The classes of
a stretch of the path and its balls are looked up once, on the dense box around them: a cache, not a rule.)"""
import functools

import numpy as np

from tests import raywalk_ref as rw

OCC, INFL, UNKNOWN = rw.OCC, rw.INFL, rw.UNKNOWN
FLAG_SETS = rw.FLAG_SETS
OUTPUTS = ("status", "voxel", "t", "n_steps", "n_unknown", "hit", "hit_sq")
NONE = -1
MAX_RADIUS = 16
CHUNK = 32  # path voxels whose balls share one dense box of classes


@functools.lru_cache(maxsize=None)
def ball(r):
    """the offsets o with |o|^2 <= r^2, sorted by (|o|^2, z, y, x): ([B, 3] as x, y, z; [B] squared lengths)"""
    a = np.arange(-r, r + 1)
    z, y, x = np.meshgrid(a, a, a, indexing="ij")
    off = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.int64)
    sq = (off * off).sum(axis=1)
    keep = sq <= r * r
    off, sq = off[keep], sq[keep]
    order = np.lexsort((off[:, 0], off[:, 1], off[:, 2], sq))
    return off[order], sq[order]


def columns(r):
    """L(r): the (p, q) with p^2 + q^2 <= r^2"""
    return sum(1 for p in range(-r, r + 1) for q in range(-r, r + 1) if p * p + q * q <= r * r)


def _ball_bits(classes, vox, off, r):
    """[K, B] classes of vox[k] + off[j]"""
    lo = vox.min(axis=0) - r
    dims = vox.max(axis=0) + r - lo + 1
    z, y, x = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    grid = classes(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1) + lo).reshape(dims[2], dims[1], dims[0])
    at = vox[:, None, :] + off[None, :, :] - lo
    return grid[at[..., 2], at[..., 1], at[..., 0]]


def sweep(p0, p1, d, r, classes, flag_sets=FLAG_SETS):
    """{flags: (status, voxel, t, n_steps, n_unknown, hit, hit_sq)} of one segment and {flags: axis on which a tie between the two
    smallest hits was resolved (0 z, 1 y, 2 x) or None}; classes(voxels [K, 3] int64) -> the class bits that hold at each voxel"""
    Q = rw.valid(p0, p1, d)
    if Q is None:
        return {f: (-1, (0, 0, 0), 0.0, 0, 0, (0, 0, 0), NONE) for f in flag_sets}, {f: None for f in flag_sets}
    pth, _ = rw.path(*Q)
    vox = np.array([v for v, _ in pth], dtype=np.int64)
    unk = np.concatenate([[0], np.cumsum((classes(vox) & UNKNOWN) != 0)])  # unk[k]: UNKNOWN centre voxels among path indices 0 .. k-1
    off, sq = ball(r)
    out, ties = {}, {}
    todo = [f for f in flag_sets if f]
    for k0 in range(0, len(vox), CHUNK):
        if not todo:
            break
        bits = _ball_bits(classes, vox[k0:k0 + CHUNK], off, r)
        for f in list(todo):
            m = (bits & f) != 0
            rows = np.flatnonzero(m.any(axis=1))
            if not rows.size:
                continue
            k = k0 + int(rows[0])
            js = np.flatnonzero(m[rows[0]])  # (sorted by the tuple: the first is the hit)
            j = int(js[0])
            mm, ad = pth[k][1]
            hit = tuple(int(v) for v in vox[k] + off[j])
            out[f] = (1, pth[k][0], mm / ad, k, int(unk[k]), hit, int(sq[j]))
            ties[f] = None
            if len(js) > 1 and sq[js[1]] == sq[j]:
                a, b = off[j], off[js[1]]
                ties[f] = 0 if a[2] != b[2] else (1 if a[1] != b[1] else 2)
            todo.remove(f)
    for f in flag_sets:
        if f not in out:
            out[f] = (0, pth[-1][0], 1.0, len(pth), int(unk[-1]), pth[-1][0], NONE)
            ties[f] = None
    return out, ties


def path_len(p0, p1, d):
    """N + 1 of a valid segment, 0 of an invalid one"""
    Q = rw.valid(p0, p1, d)
    return 0 if Q is None else 1 + sum(abs((Q[1][a] >> 10) - (Q[0][a] >> 10)) for a in range(3))


def sweep_all(p0, p1, d, r, classes, flag_sets=FLAG_SETS):
    """{flags: {name: array}} with mlm_query_sweeps' types, and {flags: [tie axis or None per ray]}"""
    n = len(p0)
    res = {f: {"status": np.empty(n, np.int8), "voxel": np.empty((n, 3), np.int32), "t": np.empty(n, np.float64), "n_steps": np.empty(n, np.int32),
               "n_unknown": np.empty(n, np.int32), "hit": np.empty((n, 3), np.int32), "hit_sq": np.empty(n, np.int32)} for f in flag_sets}
    ties = {f: [] for f in flag_sets}
    for i in range(n):
        o, tie = sweep(p0[i], p1[i], d, r, classes, flag_sets)
        for f in flag_sets:
            q = res[f]
            q["status"][i], q["voxel"][i], q["t"][i], q["n_steps"][i], q["n_unknown"][i], q["hit"][i], q["hit_sq"][i] = o[f]
            ties[f].append(tie[f])
    return res, ties


def assert_equal(got, exp, what=""):
    """every output present in `got` equal: integers exactly, t by its 64 bits"""
    for k in OUTPUTS:
        if k not in got:
            continue
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, g.dtype, e.shape, e.dtype)
        bad = (g.view(np.uint64) != e.view(np.uint64)) if k == "t" else (g != e)
        bad = np.flatnonzero(bad.reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{what} {k}: {bad.size} of {len(g)} rays differ, first #{bad[0]}: {g[bad[0]]!r} vs {e[bad[0]]!r}"


def check_properties(p0, p1, d, r, classes, f, res):
    """a stopped ray's hit has O, lies in the ball, no ball voxel with O has a smaller tuple, and no earlier path voxel is blocked —
    each evaluated voxel by voxel, without ball(); returns the status"""
    st, voxel, _, k, _, hit, hit_sq = res
    Q = rw.valid(p0, p1, d)
    if Q is None:
        assert res == (-1, (0, 0, 0), 0.0, 0, 0, (0, 0, 0), NONE)
        return -1
    pth, _ = rw.path(*Q)
    rng = range(-r, r + 1)
    cube = np.array([(x, y, z) for z in rng for y in rng for x in rng], dtype=np.int64)
    inside = (cube * cube).sum(axis=1) <= r * r

    def blockers(v):
        c = cube[inside] + np.asarray(v, dtype=np.int64)
        return c[(classes(c) & f) != 0]

    last = k if st == 1 else len(pth)
    for j in range(last):
        assert len(blockers(pth[j][0])) == 0, (p0, p1, j)
    if st == 0:
        assert k == len(pth) and voxel == pth[-1][0] and hit == voxel and hit_sq == NONE
        return 0
    assert voxel == pth[k][0]
    b = blockers(voxel)
    assert len(b) > 0
    tup = sorted((int(((o - voxel) ** 2).sum()), int(o[2]), int(o[1]), int(o[0])) for o in b)[0]
    assert tup == (hit_sq, hit[2], hit[1], hit[0]) and hit_sq <= r * r, (tup, hit, hit_sq)
    return 1
