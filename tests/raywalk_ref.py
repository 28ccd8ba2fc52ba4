"""Ground truth of mlm_query_rays (include/mlmap_hip.h) for tests/test_ray_walk.py and tests/test_gpu_rays.py: the walk of the
header's contract written in plain Python integers and fractions.Fraction, over voxel classes taken from a block dump
(OracleMap.export_blocks() / MLMap.export_blocks()) or from any other callable; checks of the walk against geometry; generators of
the rays the tests cast.  Nothing here calls the code under test."""
from fractions import Fraction

import numpy as np

OCC, INFL, UNKNOWN = 1, 2, 4
FLAG_SETS = (0, OCC, OCC | INFL, UNKNOWN, OCC | INFL | UNKNOWN)
OUTPUTS = ("status", "voxel", "t", "n_steps", "n_unknown")


# ---- the walk ---------------------------------------------------------------------------------------------------------------------
def lattice(p, d):
    """the three lattice coordinates floor((x / d) * 1024) of a position as Python ints; None: not finite or |q| >= 2^40"""
    with np.errstate(all="ignore"):
        q = np.floor((np.asarray(p, dtype=np.float64) / np.float64(d)) * 1024.0)
    if not np.all(np.isfinite(q)) or np.any(np.abs(q) >= 2.0 ** 40):
        return None
    return [int(v) for v in q]


def path(Q0, Q1):
    """[(voxel, (m, |D|))] of the N + 1 voxels of the ray Q0 -> Q1 ((0, 1) for the start voxel), and the number of tie steps"""
    D = [Q1[a] - Q0[a] for a in range(3)]
    v = [q >> 10 for q in Q0]
    e = [q >> 10 for q in Q1]
    N = sum(abs(e[a] - v[a]) for a in range(3))
    s = [(x > 0) - (x < 0) for x in D]
    m = [0, 0, 0]
    for a in range(3):
        if D[a]:
            m[a] = ((v[a] + 1) << 10) - Q0[a] if s[a] > 0 else Q0[a] - (v[a] << 10)
    out = [(tuple(v), (0, 1))]
    ties = 0
    for _ in range(N):
        best = None
        tie = False
        for a in range(3):
            if v[a] != e[a]:
                if best is None or m[a] * abs(D[best]) < m[best] * abs(D[a]):
                    best, tie = a, False
                elif m[a] * abs(D[best]) == m[best] * abs(D[a]):
                    tie = True
        ties += tie
        ent = (m[best], abs(D[best]))
        v[best] += s[best]
        m[best] += 1024
        out.append((tuple(v), ent))
    assert v == e
    return out, ties


def valid(p0, p1, d):
    """(Q0, Q1) of a valid ray, else None"""
    Q0, Q1 = lattice(p0, d), lattice(p1, d)
    if Q0 is None or Q1 is None or any(abs(Q1[a] - Q0[a]) > 2 ** 25 for a in range(3)):
        return None
    return Q0, Q1


def cast(p0, p1, d, classes, flag_sets=FLAG_SETS):
    """{flags: (status, voxel, t, n_steps, n_unknown)} of one ray, and its tie steps; classes(voxels [K,3] int64) -> the MLM_RAY_*
    bits that hold at each voxel"""
    Q = valid(p0, p1, d)
    if Q is None:
        return {f: (-1, (0, 0, 0), 0.0, 0, 0) for f in flag_sets}, 0
    pth, ties = path(*Q)
    bits = classes(np.array([v for v, _ in pth], dtype=np.int64))
    unk = np.concatenate([[0], np.cumsum((bits & UNKNOWN) != 0)])  # unk[k]: UNKNOWN voxels among path indices 0 .. k-1
    out = {}
    for f in flag_sets:
        hit = np.flatnonzero(bits & f)
        if hit.size:
            k = int(hit[0])
            m, ad = pth[k][1]
            out[f] = (1, pth[k][0], m / ad, k, int(unk[k]))  # (int / int: correctly rounded, as the IEEE division of the two doubles)
        else:
            out[f] = (0, pth[-1][0], 1.0, len(pth), int(unk[-1]))
    return out, ties


def cast_all(p0, p1, d, classes, flag_sets=FLAG_SETS):
    """{flags: {"status", "voxel", "t", "n_steps", "n_unknown"}} as arrays with mlm_query_rays' types, and the tie steps per ray"""
    n = len(p0)
    res = {f: {"status": np.empty(n, np.int8), "voxel": np.empty((n, 3), np.int32), "t": np.empty(n, np.float64),
               "n_steps": np.empty(n, np.int32), "n_unknown": np.empty(n, np.int32)} for f in flag_sets}
    ties = np.zeros(n, dtype=np.int64)
    for i in range(n):
        o, ties[i] = cast(p0[i], p1[i], d, classes, flag_sets)
        for f in flag_sets:
            r = res[f]
            r["status"][i], r["voxel"][i], r["t"][i], r["n_steps"][i], r["n_unknown"][i] = o[f]
    return res, ties


def assert_equal(got, exp, what=""):
    """every output equal: integers exactly, t by its 64 bits"""
    for k in OUTPUTS:
        if k not in got:
            continue
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, g.dtype, e.shape, e.dtype)
        bad = (g.view(np.uint64) != e.view(np.uint64)) if k == "t" else (g != e)
        bad = np.flatnonzero(bad.reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{what} {k}: {bad.size} of {len(g)} rays differ, first #{bad[0]}: {g[bad[0]]!r} vs {e[bad[0]]!r}"


def non_vacuous(res, ties, n_random):
    """the conditions that keep a comparison from passing vacuously, over the first n_random (the uniformly drawn) rays"""
    r = res[OCC]
    st, nu, ns = r["status"][:n_random], r["n_unknown"][:n_random], r["n_steps"][:n_random]
    lim = n_random // 10
    assert (st == 1).sum() >= lim and (st == 0).sum() >= lim, ((st == 1).sum(), (st == 0).sum())
    assert (nu > 0).sum() >= lim and ((nu > 0) & (nu < ns)).sum() >= lim, ((nu > 0).sum(), ((nu > 0) & (nu < ns)).sum())
    assert (ties > 0).sum() >= 50, (ties > 0).sum()


# ---- the walk against geometry ----------------------------------------------------------------------------------------------------
def touches(vox, Q0, Q1):
    """the closed cube of voxel vox meets the closed segment Q0 -> Q1 (lattice units; slab clipping in rationals)"""
    lo, hi = Fraction(0), Fraction(1)
    for a in range(3):
        dq = Q1[a] - Q0[a]
        l, u = vox[a] * 1024, vox[a] * 1024 + 1024
        if dq == 0:
            if not l <= Q0[a] <= u:
                return False
        else:
            t1, t2 = Fraction(l - Q0[a], dq), Fraction(u - Q0[a], dq)
            if t1 > t2:
                t1, t2 = t2, t1
            lo, hi = max(lo, t1), min(hi, t2)
    return lo <= hi


def check_geometry(Q0, Q1):
    """the four properties of the contract and t non-decreasing and <= 1; returns the tie steps"""
    pth, ties = path(Q0, Q1)
    e = tuple(q >> 10 for q in Q1)
    assert len(pth) == 1 + sum(abs((Q1[a] >> 10) - (Q0[a] >> 10)) for a in range(3)) and pth[-1][0] == e and pth[0][0] == tuple(q >> 10 for q in Q0)
    last = Fraction(0)
    for j, (v, (m, ad)) in enumerate(pth):
        assert touches(v, Q0, Q1), (Q0, Q1, v)
        t = Fraction(m, ad)
        assert last <= t <= 1, (Q0, Q1, v, t)
        last = t
        if j:
            assert sum(abs(v[a] - pth[j - 1][0][a]) for a in range(3)) == 1, (Q0, Q1, v)
    return ties


# ---- classes ----------------------------------------------------------------------------------------------------------------------
def _code(v):
    v = np.asarray(v, dtype=np.int64).reshape(-1, 3) + (1 << 20)
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]


def block_classes(b, n):
    """classes(voxels) from a block dump {"keys", "collapsed", "occ", "infl"} (sorted by key or not): bit 1 getOccupancy == OCCUPIED,
    2 getInflateOccupancy == OCCUPIED, 4 getOccupancy == UNKNOWN at the voxel, as mlm_export_window's occ / infl channels return
    them — an absent block or one beyond the key range is UNKNOWN, a released block answers from element 0 (inflated: UNKNOWN)"""
    keys = np.asarray(b["keys"], dtype=np.int64).reshape(-1, 3)
    codes = _code(keys)
    order = np.argsort(codes)
    codes = codes[order]
    occ, infl = np.asarray(b["occ"]), np.asarray(b["infl"])
    col = np.asarray(b["collapsed"]).astype(bool) if "collapsed" in b else np.zeros(len(keys), dtype=bool)

    def classes(vox):
        vox = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
        g = np.floor_divide(vox, n)
        c = vox - g * n
        bits = np.full(len(vox), UNKNOWN, dtype=np.int64)
        if not len(codes):
            return bits
        in_range = (np.abs(g) < (1 << 20)).all(axis=1)
        code = _code(np.where(in_range[:, None], g, 0))
        pos = np.minimum(np.searchsorted(codes, code), len(codes) - 1)
        have = in_range & (codes[pos] == code)
        blk = order[pos[have]]
        cid = np.where(col[blk], 0, (c[have, 2] * n + c[have, 1]) * n + c[have, 0])
        o = occ[blk, cid]
        r = np.where(o == ord("o"), OCC, np.where(o == ord("f"), 0, UNKNOWN))
        r = r | np.where(~col[blk] & (infl[blk, cid] == ord("o")), INFL, 0)
        bits[have] = r
        return bits

    return classes


def centres(vox, cfg):
    """world centres of voxels (subbox_id2xyz_glb_vec, map_local.h:208-213)"""
    n, d = cfg.subbox_n, cfg.subbox_d_xyz
    vox = np.asarray(vox, dtype=np.int64).reshape(-1, 3)
    g = np.floor_divide(vox, n)
    return g.astype(np.float64) * (d * n) + (vox - g * n).astype(np.float64) * d + d * 0.5


def query_classes(get_occ, get_infl, cfg):
    """classes(voxels) from point queries at the voxel centres (the oracle's getOccupancy / getInflateOccupancy)"""
    def classes(vox):
        p = centres(vox, cfg)
        o, i = np.asarray(get_occ(p)), np.asarray(get_infl(p))
        return np.where(o == 0, OCC, np.where(o == -1, UNKNOWN, 0)) | np.where(i == 0, INFL, 0)

    return classes


# ---- rays -------------------------------------------------------------------------------------------------------------------------
def uniform_rays(rng, lo, hi, count, short=None):
    """both end points uniform in the box lo .. hi; with `short`, every other ray ends within `short` (per axis) of its start"""
    p0, p1 = rng.uniform(lo, hi, size=(count, 3)), rng.uniform(lo, hi, size=(count, 3))
    if short is not None:
        p1[1::2] = p0[1::2] + rng.uniform(-short, short, size=p1[1::2].shape)
    return p0, p1


def special_rays(rng, lo, hi, d, count=600):
    """axis-aligned and zero-length rays; end points exactly on lattice, face, edge and corner positions (k * d and nextafter both
    ways) travelling in all eight sign octants (every tie branch, the m = 0 start); diagonals through corners"""
    a, b = [], []
    p, q = uniform_rays(rng, lo, hi, count)
    for i in range(count):  # axis aligned (one, two or all three coordinates kept) and zero length
        keep = rng.random(3) < 0.6
        q[i, keep] = p[i, keep]
    a.append(p), b.append(q)
    k0 = np.round(rng.uniform(lo, hi, size=(count, 3)) / d)
    span = rng.integers(0, 25, size=(count, 3))
    for octant in range(8):
        sgn = np.array([1 if octant & 1 else -1, 1 if octant & 2 else -1, 1 if octant & 4 else -1])
        k1 = k0 + sgn * span
        # equal spans on two or three axes: exact edge and corner crossings
        same = rng.random(count) < 0.5
        k1[same] = k0[same] + sgn * span[same, :1]
        p, q = k0 * d, k1 * d
        for arr in (p, q):
            nudge = rng.integers(0, 4, size=arr.shape)  # 0, 1: exact; 2: one ulp down; 3: one ulp up
            arr[nudge == 2] = np.nextafter(arr[nudge == 2], -np.inf)
            arr[nudge == 3] = np.nextafter(arr[nudge == 3], np.inf)
            half = rng.random(arr.shape) < 0.15  # some coordinates mid-voxel: faces and edges, not only corners
            arr[half] += d * 0.5
        a.append(p), b.append(q)
    return np.concatenate(a), np.concatenate(b)


def weird_rays(d):
    """NaN, infinities, 1e300, beyond the lattice; a ray of exactly 32 768 voxels on one axis (valid) and one lattice unit longer
    (invalid)"""
    u = d / 1024.0
    rows = [([np.nan, 0, 0], [1, 1, 1]), ([0, 0, 0], [0, np.nan, 0]), ([np.inf, 0, 0], [1, 1, 1]), ([0, 0, 0], [0, 0, -np.inf]),
            ([1e300, 0, 0], [1e300, 0, 0]), ([0, -1e300, 0], [0, 1, 0]), ([2.0 ** 31 * d, 0, 0], [2.0 ** 31 * d, 1, 0]),
            ([0.25 * u, 0.5 * d, 0.5 * d], [(2 ** 25 + 0.5) * u, 0.5 * d, 0.5 * d]),
            ([0.25 * u, 0.5 * d, 0.5 * d], [(2 ** 25 + 1.5) * u, 0.5 * d, 0.5 * d]),
            ([0.5 * d, 0.5 * d, -0.25 * u], [0.5 * d, 0.5 * d, -(2 ** 25 + 0.5) * u]),
            ([0.5 * d, 0.5 * d, -0.25 * u], [0.5 * d, 0.5 * d, -(2 ** 25 + 1.5) * u])]
    p0, p1 = np.array([r[0] for r in rows], dtype=np.float64), np.array([r[1] for r in rows], dtype=np.float64)
    # (the two long rays are what they are meant to be whatever the rounding of u)
    for i, span in ((7, 2 ** 25), (8, 2 ** 25 + 1), (9, 2 ** 25), (10, 2 ** 25 + 1)):
        Q0, Q1 = lattice(p0[i], d), lattice(p1[i], d)
        assert max(abs(Q1[a] - Q0[a]) for a in range(3)) == span, (i, Q0, Q1)
    return p0, p1
