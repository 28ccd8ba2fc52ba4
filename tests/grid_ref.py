"""Ground truth of mlm_export_grid2d (include/mlmap_hip.h) in plain numpy, kept apart from the code under test.

Two independent parts: columns() reduces dense occ / infl arrays of the slab ([dz][dy][dx], the classes mlm_export_window returns) to
the grid, the eight column words and the summary, by whole-array reductions along z (no walk); the distance comes either from the
definition taken literally over a list of obstacle cells of the plane (dist_brute, small planes) or from a separable truncated
transform of the mask P of the plane grown by C per side (dist_separable, any plane).  dist_channels() applies the header's float32
formula."""
import numpy as np

OCC, INFL, UNKNOWN, DIST_UNOBSERVED = 1, 2, 4, 16


def predicate(occ, infl, flags):
    m = np.zeros(occ.shape, dtype=bool)
    if flags & OCC:
        m |= occ == 0
    if flags & INFL:
        m |= infl == 0
    if flags & UNKNOWN:
        m |= occ == -1
    return m


def columns(occ, infl, lo_z, flags, min_free=0, z_ref=None):
    """{"grid", "cols", "summary"} of a slab whose classes are occ / infl ([dz][dy][dx]); z_ref absolute, None: the middle layer"""
    occ, infl = np.asarray(occ).astype(np.int64), np.asarray(infl).astype(np.int64)
    dz = occ.shape[0]
    hi_z = lo_z + dz
    z_ref = lo_z + dz // 2 if z_ref is None else z_ref
    O = predicate(occ, infl, flags)
    unk = occ == -1
    z = (lo_z + np.arange(dz, dtype=np.int64))[:, None, None]
    n_obs, n_unk, n_free = O.sum(0), unk.sum(0), (occ == 1).sum(0)
    zmin = np.where(O, z, hi_z).min(0)
    zmax = np.where(O, z, lo_z - 1).max(0)
    below = np.where(O & (z <= z_ref), z, lo_z - 1).max(0)
    above = np.where(O & (z >= z_ref), z, hi_z).min(0)
    gap = (unk & (z > below[None]) & (z < above[None])).sum(0)
    cols = np.stack([n_obs, n_unk, n_free, zmin, zmax, below, above, gap], axis=-1).astype(np.int32)
    grid = np.where(n_obs > 0, 100, np.where(n_free < min_free, -1, 0)).astype(np.int8)
    summary = np.array([(grid == 100).sum(), (grid == 0).sum(), (grid == -1).sum(), n_obs.sum(), n_unk.sum(), n_free.sum()], dtype=np.int64)
    return {"grid": grid, "cols": cols, "summary": summary}


def plane_mask(grid, flags):
    """P of the distance field from a grid"""
    return (grid != 0) if flags & DIST_UNOBSERVED else (grid == 100)


def dist_separable(mask, C):
    """min(C^2, squared distance to the nearest True cell) of the plane inside `mask`, the mask of the plane grown by C per side
    ([dy + 2C][dx + 2C]), by two 1-D truncated passes"""
    C2 = C * C
    f = np.where(mask, 0, C2).astype(np.int64)
    for axis in (1, 0):
        g = f.copy()
        for k in range(1, C):
            a, b = [slice(None)] * 2, [slice(None)] * 2
            a[axis], b[axis] = slice(0, -k), slice(k, None)
            a, b = tuple(a), tuple(b)
            np.minimum(g[a], f[b] + k * k, out=g[a])
            np.minimum(g[b], f[a] + k * k, out=g[b])
        f = g
    return np.minimum(f, C2)[C:-C, C:-C].astype(np.int32)


def dist_brute(cells, lo, dims, C):
    """the definition literally: min over the obstacle cells (K x 2, x y, anywhere in the plane) of the squared distance, clamped at
    C^2, for the plane lo[:2] .. lo[:2] + dims[:2] ([dy][dx])"""
    iy, ix = np.unravel_index(np.arange(dims[0] * dims[1]), (dims[1], dims[0]))
    tgt = np.stack([lo[0] + ix, lo[1] + iy], axis=1).astype(np.int64)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    out = np.full(len(tgt), C * C, dtype=np.int64)
    if len(cells):
        out = np.minimum(out, ((tgt[:, None, :] - cells[None, :, :]) ** 2).sum(-1).min(1))
    return out.reshape(dims[1], dims[0]).astype(np.int32)


def dist_channels(sq, d):
    """{"sqdist", "dist"}: dist = (float)d * sqrtf((float)sqdist), one float32 square root and one float32 multiply"""
    return {"sqdist": sq.astype(np.int32), "dist": (np.float32(d) * np.sqrt(sq.astype(np.float32))).astype(np.float32)}


def grown2(lo, dims, C):
    """the slab grown by C cells per side in x and y"""
    return [lo[0] - C, lo[1] - C, lo[2]], [dims[0] + 2 * C, dims[1] + 2 * C, dims[2]]


def compare(got, exp, what=""):
    """word for word; dist as float32 bits"""
    for k, v in got.items():
        e = exp[k]
        assert v.shape == e.shape and v.dtype == e.dtype, (what, k, v.shape, e.shape, v.dtype, e.dtype)
        a, b = (v.view(np.uint32), e.view(np.uint32)) if v.dtype == np.float32 else (v, e)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what} {k}: {len(bad)} differ, first at {bad[0]}: {v[tuple(bad[0])]} vs {e[tuple(bad[0])]}"
