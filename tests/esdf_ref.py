"""Ground truth of mlm_export_esdf (include/mlmap_hip.h) in plain numpy, kept apart from the code under test.

Two forms of the field: the definition taken literally (edt_brute: min over every obstacle voxel of the map) for small boxes, and a
separable truncated transform of the obstacle mask of the box grown by C (edt_separable) for any box; channels() turns squared
distances into the header's sqdist / dist / grad channels in float32; expected() / expected_brute() put the two together.  grown(),
centres(), classes_mask() and _code() build the boxes, the voxel centres of a configuration, obstacle masks from occ / infl classes
and one int64 per index triple."""
import numpy as np

OCC, INFL, UNKNOWN, SIGNED = 1, 2, 4, 8


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


def edt_brute(obs, lo, dims, C):
    """the definition literally, over the box lo .. lo + dims ([z][y][x]): min over every obstacle voxel o of the map (obs [K,3],
    x y z) of |v - o|^2, clamped at C^2"""
    iz, iy, ix = np.unravel_index(np.arange(dims[0] * dims[1] * dims[2]), (dims[2], dims[1], dims[0]))
    tgt = np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)
    obs = np.asarray(obs, dtype=np.int64).reshape(-1, 3)
    out = np.full(len(tgt), C * C, dtype=np.int64)
    step = max(1, 20_000_000 // max(1, len(obs)))
    for i in range(0, len(tgt) if len(obs) else 0, step):
        d2 = ((tgt[i:i + step, None, :] - obs[None, :, :]) ** 2).sum(-1).min(1)
        out[i:i + step] = np.minimum(out[i:i + step], d2)
    return out.reshape(dims[2], dims[1], dims[0]).astype(np.int32)


def channels(dout, din, d):
    """sqdist, dist and gradients of the window from D_out (and D_in: signed) over the window +- 1"""
    sq = dout if din is None else np.where(dout == 0, -din, dout).astype(np.int32)
    df = np.float32(d)
    mag = df * np.sqrt(np.abs(sq).astype(np.float32))
    dist = np.where(sq < 0, -mag, mag).astype(np.float32)
    inv = np.float32(0.5 / d)
    grad = np.stack([(dist[1:-1, 1:-1, 2:] - dist[1:-1, 1:-1, :-2]) * inv, (dist[1:-1, 2:, 1:-1] - dist[1:-1, :-2, 1:-1]) * inv,
                     (dist[2:, 1:-1, 1:-1] - dist[:-2, 1:-1, 1:-1]) * inv], axis=-1).astype(np.float32)
    return {"sqdist": sq[1:-1, 1:-1, 1:-1], "dist": dist[1:-1, 1:-1, 1:-1], "grad": grad}


def expected(mask, C, signed, d):
    """channels of the window from the obstacle mask of the window grown by C per side ([z][y][x]), separable form"""
    crop = tuple(slice(C - 1, s - C + 1) for s in mask.shape)  # window +- 1
    return channels(edt_separable(mask, C)[crop], edt_separable(~mask, C)[crop] if signed else None, d)


def expected_brute(obs, lo, dims, C, d):
    """channels of an unsigned field from the map's obstacle voxels, the definition literally"""
    return channels(edt_brute(obs, [v - 1 for v in lo], [v + 2 for v in dims], C), None, d)


def grown(lo, dims, C):
    return [v - C for v in lo], [v + 2 * C for v in dims]


def centres(cfg, lo, dims):
    n, d = cfg.subbox_n, cfg.subbox_d_xyz
    iz, iy, ix = np.unravel_index(np.arange(dims[0] * dims[1] * dims[2]), (dims[2], dims[1], dims[0]))
    v = np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)
    g = np.floor_divide(v, n)
    return g.astype(np.float64) * (d * n) + (v - g * n).astype(np.float64) * d + d * 0.5


def classes_mask(occ, infl, flags):
    m = np.zeros(occ.shape, dtype=bool)
    if flags & OCC:
        m |= occ == 0
    if flags & INFL:
        m |= infl == 0
    if flags & UNKNOWN:
        m |= occ == -1
    return m


def _code(v):
    """one int64 per voxel / block index triple (|coordinates| < 2^20)"""
    v = np.asarray(v, dtype=np.int64).reshape(-1, 3) + (1 << 20)
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]
