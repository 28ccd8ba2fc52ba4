"""mlm_export_grid2d: the map projected onto the ground plane (include/mlmap_hip.h), word for word against plain numpy
(tests/grid_ref.py): grid, the eight column words and the summary from whole-array reductions of the slab's occ / infl classes,
sqdist / dist from the definition over obstacle cells (small planes) and from a separable transform of the grown plane's mask.

The classes come from maps built voxel by voxel (import_blocks), from the CPU oracle's getOccupancy / getInflateOccupancy at the voxel
centres, and from the GPU's own export_window."""
import ctypes
import os

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests.esdf_ref import centres
from tests.grid_ref import (DIST_UNOBSERVED, INFL, OCC, UNKNOWN, columns, compare, dist_brute, dist_channels, dist_separable, grown2, plane_mask,
                            predicate)

pytestmark = pytest.mark.gpu

N = S1.subbox_n
EXTRA = [int(x) for x in os.environ.get("MLM_STRESS_SEEDS", "").split(",") if x]  # more seeds for a longer soak
SEEDS = [5]


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


# ---- calls and references ------------------------------------------------------------------------------------------------------
def flag_args(flags):
    return dict(occ=bool(flags & OCC), infl=bool(flags & INFL), unknown=bool(flags & UNKNOWN), dist_unobserved=bool(flags & DIST_UNOBSERVED))


def grid2d(gpu, lo, dims, flags, min_free=0, z_ref=None, C=None, **ch):
    ch = ch or dict(grid=True, cols=True, sqdist=C is not None, dist=C is not None)
    return gpu.export_grid2d(lo, dims, min_free=min_free, z_ref=z_ref, max_dist=C, **flag_args(flags), **ch)


def grid2d_dev(gpu, lo, dims, flags, min_free=0, z_ref=None, C=None, guard=3):
    """the same into device tensors with guard elements on both sides of every output, which must stay as they were"""
    import torch

    cells = dims[0] * dims[1]
    shape = (dims[1], dims[0])
    spec = {"grid": (torch.int8, 1), "cols": (torch.int32, 8)}
    if C is not None:
        spec.update({"sqdist": (torch.int32, 1), "dist": (torch.float32, 1)})
    buf = {k: torch.full((cells * w + 2 * guard * w,), 77, dtype=dt, device="cuda") for k, (dt, w) in spec.items()}
    ptr = {k: v[guard * spec[k][1]:].data_ptr() for k, v in buf.items()}
    summary = gpu.export_grid2d_dev(lo, dims, min_free=min_free, z_ref=z_ref, max_dist=C, **flag_args(flags), **ptr)
    out = {"summary": summary}
    for k, v in buf.items():
        w = spec[k][1]
        a = v.cpu().numpy()
        assert (a[:guard * w] == 77).all() and (a[-guard * w:] == 77).all(), f"{k}: guard words overwritten"
        out[k] = a[guard * w:-guard * w].reshape(shape + ((8,) if w == 8 else ()))
    return out


def window_classes(gpu, lo, dims):
    w = gpu.export_window(lo, dims, odds=False, occ=True, infl=True)
    return w["occ"], w["infl"]


def reference(classes, lo, dims, flags, min_free=0, z_ref=None, C=None):
    """every output from `classes(lo, dims) -> (occ, infl)`; the distance from the mask of the plane grown by C"""
    occ, infl = classes(lo, dims)
    exp = columns(occ, infl, lo[2], flags & 7, min_free, z_ref)
    if C is not None:
        glo, gd = grown2(lo, dims, C)
        g = columns(*classes(glo, gd), lo[2], flags & 7, min_free, z_ref)["grid"]
        exp.update(dist_channels(dist_separable(plane_mask(g, flags), C), S1.subbox_d_xyz))
    return exp


# ---- maps built voxel by voxel ---------------------------------------------------------------------------------------------------
class Crafted:
    """blocks imported cell by cell: `blocks` are present and FREE / infl 'u' except the voxels listed as occupied, unknown or
    inflated; voxels of other blocks are UNKNOWN / UNKNOWN"""

    def __init__(self, MLMap, blocks, occupied=(), unknown=(), inflated=(), cfg=S1):
        n = cfg.subbox_n
        vox = [np.asarray(v, dtype=np.int64).reshape(-1, 3) for v in (occupied, unknown, inflated)]
        keys = np.unique(np.concatenate([np.asarray(blocks, dtype=np.int64).reshape(-1, 3)] + [np.floor_divide(v, n) for v in vox]), axis=0)
        self.n, self.keys = n, keys
        self.kidx = {tuple(k): i for i, k in enumerate(keys.tolist())}
        self.occ = np.full((len(keys), n ** 3), ord("f"), dtype=np.uint8)
        self.infl = np.full((len(keys), n ** 3), ord("u"), dtype=np.uint8)
        for plane, v, c in ((self.occ, vox[0], "o"), (self.occ, vox[1], "u"), (self.infl, vox[2], "o")):
            g = np.floor_divide(v, n)
            cell = v - g * n
            for gi, ci in zip(g.tolist(), cell.tolist()):
                plane[self.kidx[tuple(gi)], ci[2] * n * n + ci[1] * n + ci[0]] = ord(c)
        self.gpu = MLMap(cfg, max_blocks=4096)
        self.gpu.import_blocks(keys.astype(np.int32), np.zeros(self.occ.shape, np.float32), self.occ, self.infl, np.zeros(len(keys), np.uint8))

    def classes(self, lo, dims):
        """occ / infl of a box ([dz][dy][dx]) straight from the imported planes"""
        n = self.n
        iz, iy, ix = np.unravel_index(np.arange(dims[0] * dims[1] * dims[2]), (dims[2], dims[1], dims[0]))
        v = np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)
        g = np.floor_divide(v, n)
        c = v - g * n
        cid = c[:, 2] * n * n + c[:, 1] * n + c[:, 0]
        slot = np.array([self.kidx.get(tuple(k), -1) for k in g.tolist()])
        have = slot >= 0
        o = np.where(have, self.occ[np.maximum(slot, 0), cid], ord("u"))
        i = np.where(have, self.infl[np.maximum(slot, 0), cid], ord("u"))
        occ = np.where(o == ord("o"), 0, np.where(o == ord("f"), 1, -1)).astype(np.int8)
        infl = np.where(i == ord("o"), 0, -1).astype(np.int8)
        shape = (dims[2], dims[1], dims[0])
        return occ.reshape(shape), infl.reshape(shape)


LO, DIMS = [-7, -3, -13], [23, 22, 27]  # x in [-7, 16), y in [-3, 19): block seams at 0 and 10; z in [-13, 14): two partial bricks


@pytest.fixture(scope="module")
def band_map(mods):
    MLMap, _ = mods
    rng = np.random.default_rng(11)
    # stacks (gx, gy) of blocks gz = -2 .. 1: (1, 1) absent altogether, (0, 0) without gz = -1, (-1, 1) only gz = 1
    blocks = [(gx, gy, gz) for gx in (-1, 0, 1) for gy in (-1, 0, 1) for gz in (-2, -1, 0, 1)
              if (gx, gy) != (1, 1) and (gx, gy, gz) != (0, 0, -1) and ((gx, gy) != (-1, 1) or gz == 1)]
    zlo, zhi = LO[2], LO[2] + DIMS[2] - 1
    occupied = [(-5, -2, zlo), (-5, -1, zhi), (3, 4, zlo), (3, 4, zhi),  # the first and the last layer of the slab
                (-4, -2, zlo - 1), (-4, -1, zhi + 1), (12, 5, zlo - 1), (12, 5, zhi + 1),  # one layer outside: must not count
                (2, 2, 0), (2, 2, 1), (2, 3, 0), (15, -3, 5), (-7, 9, -1), (9, 9, -10), (9, 9, 9), (0, 0, 0), (-1, -1, -1)]
    present = np.array([b for b in blocks], dtype=np.int64)
    pick = present[rng.integers(0, len(present), 400)] * N + rng.integers(0, N, (400, 3))
    pick = pick[~((pick[:, 0] == -4) & (pick[:, 1] == -2))]  # (the column the test expects to be empty)
    occupied += pick[:120].tolist()
    m = Crafted(MLMap, blocks, occupied, unknown=pick[120:300], inflated=pick[260:400])
    yield m
    m.gpu.close()


def test_band_against_blocks(band_map):
    """a slab through partial bricks and negative indices, absent and partly absent stacks, obstacles on the slab's first and last
    layer and one layer outside it: every class-bit combination, min_free and z_ref, into host arrays and device tensors"""
    m = band_map
    occ, infl = m.classes(LO, DIMS)
    w_occ, w_infl = window_classes(m.gpu, LO, DIMS)
    assert np.array_equal(occ, w_occ) and np.array_equal(infl, w_infl)
    on_obstacle = 0  # (2, 2, 0) is occupied
    n_calls = 0
    for flags in range(1, 8):
        for min_free in (0, 1, DIMS[2]):
            for z_ref in (LO[2], LO[2] + DIMS[2] - 1, on_obstacle):
                exp = columns(occ, infl, LO[2], flags, min_free, z_ref)
                got = grid2d(m.gpu, LO, DIMS, flags, min_free, z_ref)
                compare(got, exp, f"flags={flags} min_free={min_free} z_ref={z_ref}")
                if n_calls % 9 == 4:
                    compare(grid2d_dev(m.gpu, LO, DIMS, flags, min_free, z_ref), exp, f"device flags={flags}")
                n_calls += 1
    exp = columns(occ, infl, LO[2], OCC, 1, on_obstacle)
    c = exp["cols"]
    assert (c[..., 0] > 0).any() and (c[..., 0] == 0).any() and (exp["grid"] == -1).any() and (exp["grid"] == 0).any()
    assert (c[..., 1] == DIMS[2]).any() and ((c[..., 1] > 0) & (c[..., 1] < DIMS[2])).any()  # absent and partly absent stacks
    assert c[2 - LO[1], 2 - LO[0], 5] == 0 and c[2 - LO[1], 2 - LO[0], 6] == 0  # z_ref on an obstacle: free height -1
    assert c[-2 - LO[1], -4 - LO[0], 0] == 0 and c[-2 - LO[1], -5 - LO[0], 3] == LO[2]  # outside the slab / on its first layer
    assert (c[..., 7] > 0).any()
    # the default z_ref is the middle layer
    compare(grid2d(m.gpu, LO, DIMS, OCC | UNKNOWN), columns(occ, infl, LO[2], OCC | UNKNOWN, 0, LO[2] + DIMS[2] // 2), "default z_ref")


def test_degenerate_slabs(band_map):
    """dims[2] == 1: the words are the window's classes of that layer; a 1 x 1 plane: one column"""
    m = band_map
    for lo, dims in (([-7, -3, 0], [23, 22, 1]), ([-7, -3, -13], [23, 22, 1]), ([2, 2, -13], [1, 1, 27]), ([12, 12, -3], [1, 1, 9]),
                     ([2, 2, 0], [1, 1, 1]), ([-5, -2, -13], [1, 1, 1])):
        occ, infl = window_classes(m.gpu, lo, dims)
        for flags in (OCC, INFL | UNKNOWN, OCC | INFL | UNKNOWN):
            for min_free in (0, dims[2]):
                got = grid2d(m.gpu, lo, dims, flags, min_free, lo[2], C=3)
                compare(got, reference(lambda l, d: window_classes(m.gpu, l, d), lo, dims, flags, min_free, lo[2], C=3), f"{lo} {dims} {flags}")
                if dims[2] == 1:
                    O = predicate(occ[0].astype(np.int64), infl[0].astype(np.int64), flags)
                    assert np.array_equal(got["grid"] == 100, O)
                    assert np.array_equal(got["cols"][..., 1], (occ[0] == -1).astype(np.int32))
                    assert np.array_equal(got["cols"][..., 2], (occ[0] == 1).astype(np.int32))
                    assert np.array_equal(got["cols"][..., 6] - got["cols"][..., 5] - 1, np.where(O, -1, 1))


@pytest.mark.parametrize("C", [1, 5, 64])
def test_halo_edge(mods, C):
    """one obstacle column k cells beyond a face of the plane, k = 1 .. C + 1: the facing cell reads min(k^2, C^2); one at offsets
    (C - 1, 1) beyond a corner reads min(C^2, (C - 1)^2 + 1); an obstacle nearer in the plane but outside the z band changes nothing;
    with MLM_GRID_DIST_UNOBSERVED an absent block beyond the face is an obstacle"""
    MLMap, _ = mods
    dims = [5, 4, 3]
    sp = 3 * C + 20  # planes far enough apart not to see each other's obstacles
    cases, outside = [], []
    for k in range(1, C + 2):
        lo = [-7 + sp * k, -3, -2]
        side = k % 2  # beyond the +x face, or beyond the -x face
        fx = lo[0] + dims[0] - 1 if side else lo[0]
        cases.append((lo, (fx + k if side else fx - k, lo[1] + 1, lo[2] + (k % 3)), (fx, lo[1] + 1), min(k * k, C * C)))
        outside.append((fx + 1 if side else fx - 1, lo[1] + 2, lo[2] + dims[2] if k % 2 else lo[2] - 1))  # one cell away, outside the band
    lo = [-7 - sp, 11, 4]  # the diagonal one, beyond the (+x, +y) corner
    cx, cy = lo[0] + dims[0] - 1, lo[1] + dims[1] - 1
    cases.append((lo, (cx + C - 1, cy + 1, lo[2]), (cx, cy), min(C * C, (C - 1) ** 2 + 1)))
    m = Crafted(MLMap, [], [c[1] for c in cases] + outside)
    for lo, ob, face, val in cases:
        got = grid2d(m.gpu, lo, dims, OCC, C=C, grid=True, sqdist=True, dist=True)
        assert got["sqdist"][face[1] - lo[1], face[0] - lo[0]] == val, (C, lo, ob)
        cells = [c[1][:2] for c in cases if lo[2] <= c[1][2] < lo[2] + dims[2]]
        exp = dist_channels(dist_brute(cells, lo, dims, C), S1.subbox_d_xyz)
        compare({k: got[k] for k in exp}, exp, f"C={C} {lo}")
        assert not got["grid"].any()
    m.gpu.close()

    # unobserved cells as obstacles: FREE blocks x, y in [-10, 30), the plane's +x face 4 cells from the first absent block
    m = Crafted(MLMap, [(gx, gy, 0) for gx in range(-1, 3) for gy in range(-1, 3)], [(18, 8, 3)])
    lo, dims = [22, 8, 2], [5, 4, 3]
    cl = m.classes
    for flags, val in ((OCC, min(C * C, 8 * 8 + 1)), (OCC | DIST_UNOBSERVED, min(C * C, 16))):
        got = grid2d(m.gpu, lo, dims, flags, min_free=dims[2], z_ref=lo[2], C=C)
        compare(got, reference(cl, lo, dims, flags, dims[2], lo[2], C), f"unobserved C={C} flags={flags}")
        assert got["sqdist"][1, 4] == val and not got["grid"].any()  # (the cell (26, 9): 4 from x = 30; (8, 1) from the obstacle)
    m.gpu.close()


def test_tile_seams(mods, knobs):
    """a 70 x 45 plane at C = 5 with the default plan (one tile) and with grid_tile at its smallest (a tile per cell, each grown by
    4): identical bytes, into host arrays and device tensors"""
    MLMap, _ = mods
    rng = np.random.default_rng(3)
    blocks = [(gx, gy, gz) for gx in range(-3, 6) for gy in range(-2, 5) for gz in (-1, 0) if rng.random() < 0.8]
    pick = np.array(blocks)[rng.integers(0, len(blocks), 300)] * N + rng.integers(0, N, (300, 3))
    m = Crafted(MLMap, blocks, pick[:60], unknown=pick[60:200], inflated=pick[200:])
    lo, dims, C = [-23, -11, -4], [70, 45, 9], 5
    for flags, min_free in ((OCC, 0), (OCC | INFL | DIST_UNOBSERVED, 4)):
        ref = grid2d(m.gpu, lo, dims, flags, min_free, 1, C)
        compare(ref, reference(m.classes, lo, dims, flags, min_free, 1, C), f"one tile flags={flags}")
        assert (ref["sqdist"] == C * C).any() and (ref["sqdist"] == 0).any() and ((ref["sqdist"] > 0) & (ref["sqdist"] < C * C)).any()
        knobs.set("grid_tile", 1)
        got = grid2d(m.gpu, lo, dims, flags, min_free, 1, C)
        dev = grid2d_dev(m.gpu, lo, dims, flags, min_free, 1, C)
        knobs.set("grid_tile", 50)  # pieces of one row: 50 + 20
        rows = grid2d(m.gpu, lo, dims, flags, min_free, 1, C)
        knobs.set("grid_tile", 1 << 20)
        for other in (got, dev, rows):
            for k, v in ref.items():
                assert np.array_equal(other[k].view(np.uint8), v.view(np.uint8)), (flags, k)
    m.gpu.close()


# ---- integrated maps -------------------------------------------------------------------------------------------------------------
def test_frontier_mode(mods):
    """released blocks answer from element 0 (infl UNKNOWN): the columns through them equal the reference on export_window's classes"""
    MLMap, _ = mods
    cfg = S1.with_(use_exploration_frontiers=True, subbox_n=5)
    gpu = MLMap(cfg, max_blocks=16384, max_batch=2)
    for k, (img, (q, t)) in enumerate(syn.stream(cfg, "room_jitter", "smooth", 8)):
        gpu.update_map(img, q, t)
        if k in (3, 6):
            gpu.inflate_map(t)
    b = gpu.export_blocks()
    assert b["collapsed"].sum() > 20
    n = cfg.subbox_n
    rel = b["keys"][b["collapsed"] != 0].astype(np.int64)
    lo = [int(v) for v in rel.min(0) * n - 3]
    dims = [min(int(v), 90) for v in (rel.max(0) + 1) * n + 3 - np.array(lo)]
    cl = lambda l, d: window_classes(gpu, l, d)  # noqa: E731
    for flags, C in ((OCC | INFL, 7), (UNKNOWN, None), (OCC | INFL | UNKNOWN | DIST_UNOBSERVED, 7)):
        exp = reference(cl, lo, dims, flags, 2, None, C)
        compare(grid2d(gpu, lo, dims, flags, 2, None, C), exp, f"frontier flags={flags}")
    assert (exp["cols"][..., 0] > 0).any()
    gpu.close()


def test_oracle_leg(mods):
    """a 40 x 40 x 12 slab of an integrated S1 map: grid and cols equal the reference on the CPU oracle's classes at the voxel centres"""
    MLMap, OracleMap = mods
    gpu, cpu = MLMap(S1, max_blocks=8192), OracleMap(S1)
    for k, (img, (q, t)) in enumerate(syn.stream(S1, "room_jitter", "smooth", 6)):
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
        if k in (2, 4):
            gpu.inflate_map(t)
            cpu.inflate_map(t)
    b = cpu.export_blocks()
    blk, cid = np.nonzero(b["occ"] == ord("o"))
    ov = b["keys"][blk].astype(np.int64) * N + np.stack([cid % N, (cid // N) % N, cid // (N * N)], axis=1)
    mid = ov[len(ov) // 2]  # an occupied voxel in the middle of the sorted blocks
    lo, dims = [int(mid[0]) - 20, int(mid[1]) - 20, int(mid[2]) - 6], [40, 40, 12]
    p = centres(S1, lo, dims)
    shape = (dims[2], dims[1], dims[0])
    occ, infl = cpu.getOccupancy(p).reshape(shape), cpu.getInflateOccupancy(p).reshape(shape)
    assert (occ == 0).any() and (occ == 1).any() and (occ == -1).any()
    for flags in (OCC, OCC | INFL, UNKNOWN):
        for z_ref in (None, lo[2] + 2):
            got = grid2d(gpu, lo, dims, flags, 3, z_ref)
            compare(got, columns(occ, infl, lo[2], flags, 3, z_ref), f"oracle flags={flags}")
    gpu.close()


@pytest.mark.parametrize("seed", SEEDS + EXTRA)
def test_sequences(mods, seed):
    """about 20 random steps of integrate / set_free_in_bound / inflate_map / import_blocks; after each, a random small slab against
    the reference on export_window of the same slab (and of the grown plane for the distance), and summary against the arrays"""
    MLMap, _ = mods
    rng = np.random.default_rng(seed)
    gpu = MLMap(S1, max_blocks=8192)
    frames = list(syn.stream(S1, "room_jitter", "smooth", 10))
    cl = lambda l, d: window_classes(gpu, l, d)  # noqa: E731
    k = 0
    t_last = np.zeros(3)
    for step in range(20):
        op = rng.integers(0, 4) if step else 0
        if op == 0 or k == 0:
            img, (q, t_last) = frames[k % len(frames)]
            gpu.update_map(img, q, t_last)
            k += 1
        elif op == 1:
            c = t_last + rng.uniform(-1, 1, 3)
            gpu.setFree_map_in_bound(c - rng.uniform(0.2, 0.8, 3), c + rng.uniform(0.2, 0.8, 3))
        elif op == 2:
            gpu.inflate_map(t_last)
        else:
            keys = rng.integers(-3, 4, (3, 3)).astype(np.int32)
            keys = np.unique(keys, axis=0)
            occ = rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), (len(keys), N ** 3))
            infl = rng.choice(np.frombuffer(b"uo", dtype=np.uint8), (len(keys), N ** 3), p=[0.9, 0.1])
            gpu.import_blocks(keys, np.zeros(occ.shape, np.float32), occ, infl, np.zeros(len(keys), np.uint8))
        centre = np.floor(t_last / S1.subbox_d_xyz).astype(np.int64) + rng.integers(-25, 25, 3)
        dims = [int(v) for v in rng.integers(1, (45, 45, 20))]
        lo = [int(centre[a]) - dims[a] // 2 for a in range(3)]
        flags = int(rng.integers(1, 8)) | (DIST_UNOBSERVED if rng.random() < 0.5 else 0)
        min_free = int(rng.integers(0, dims[2] + 1))
        z_ref = lo[2] + int(rng.integers(0, dims[2]))
        C = int(rng.choice([1, 2, 6, 17]))
        got = grid2d(gpu, lo, dims, flags, min_free, z_ref, C)
        compare(got, reference(cl, lo, dims, flags, min_free, z_ref, C), f"seed {seed} step {step} op {op} {lo} {dims} flags={flags} C={C}")
        s, c = got["summary"], got["cols"].astype(np.int64)
        assert s[:3].sum() == dims[0] * dims[1]
        assert s.tolist() == [(got["grid"] == 100).sum(), (got["grid"] == 0).sum(), (got["grid"] == -1).sum(), c[..., 0].sum(), c[..., 1].sum(),
                              c[..., 2].sum()]
    gpu.close()


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_and_null_channels(band_map):
    """each refused argument gives MLM_ERR_INVALID and leaves the handle usable; NULL channels are skipped; nothing is written beyond
    an output (guard words around host buffers here, around device buffers in grid2d_dev)"""
    gpu = band_map.gpu
    L, h = gpu._L, gpu._h
    G = 16
    cells = DIMS[0] * DIMS[1]
    host = {"grid": np.full(cells + 2 * G, 77, np.int8), "cols": np.full(8 * cells + 2 * G, 77, np.int32), "sqdist": np.full(cells + 2 * G, 77, np.int32),
            "dist": np.full(cells + 2 * G, 77, np.float32), "summary": np.full(6 + 2 * G, 77, np.int64)}
    ptr = {k: ctypes.c_void_p(v.ctypes.data + G * v.itemsize) for k, v in host.items()}
    NAMES = ("grid", "cols", "sqdist", "dist", "summary")

    def call(lo=LO, dims=DIMS, flags=OCC, min_free=0, z_ref=0, C=5, outs=NAMES):
        lo_a, dims_a = np.array(lo, dtype=np.int32), np.array(dims, dtype=np.int32)
        return L.mlm_export_grid2d(h, lo_a.ctypes.data_as(ctypes.c_void_p), dims_a.ctypes.data_as(ctypes.c_void_p), flags, min_free, z_ref, C,
                                   *[ptr[k] if k in outs else None for k in NAMES])

    bad = [dict(dims=[0, 4, 4]), dict(dims=[4, -1, 4]), dict(dims=[4, 4, 0]), dict(dims=[2048, 2048, 1024]), dict(lo=[2 ** 31 - 10, 0, 0], dims=[20, 1, 1]),
           dict(lo=[0, 0, 2 ** 31 - 1], dims=[1, 1, 1]), dict(lo=[0, 0, -2 ** 31], dims=[2, 2, 2], z_ref=-2 ** 31),
           dict(flags=0), dict(flags=DIST_UNOBSERVED), dict(flags=OCC | 8), dict(flags=OCC | 32), dict(flags=-1),
           dict(min_free=-1), dict(min_free=DIMS[2] + 1),
           dict(z_ref=LO[2] - 1), dict(z_ref=LO[2] + DIMS[2]),
           dict(C=0), dict(C=65), dict(C=-3), dict(C=0, outs=("dist",)), dict(C=65, outs=("sqdist",)),
           dict(outs=())]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert call() == 0
    for v in host.values():
        assert (v[:G] == 77).all() and (v[-G:] == 77).all()
    full = {k: host[k][G:-G].copy() for k in NAMES}
    occ, infl = band_map.classes(LO, DIMS)
    exp = columns(occ, infl, LO[2], OCC, 0, 0)
    assert np.array_equal(full["grid"].reshape(DIMS[1], DIMS[0]), exp["grid"]) and np.array_equal(full["summary"], exp["summary"])
    assert np.array_equal(full["cols"].reshape(DIMS[1], DIMS[0], 8), exp["cols"])
    # z_ref and max_dist are looked at only with the channels that need them; NULL channels stay untouched
    for v in host.values():
        v[:] = 77
    assert call(z_ref=10 ** 6, C=0, outs=("grid",)) == 0
    assert call(z_ref=10 ** 6, C=7, outs=("sqdist", "summary")) == 0
    assert call(z_ref=0, C=1000, outs=("cols",)) == 0
    for k in ("grid", "cols", "sqdist", "summary"):
        assert np.array_equal(host[k][G:-G], full[k] if k != "sqdist" else host[k][G:-G]) and (host[k][:G] == 77).all() and (host[k][-G:] == 77).all(), k
    assert (host["dist"] == 77).all()
    assert np.array_equal(host["sqdist"][G:-G].reshape(DIMS[1], DIMS[0]), reference(band_map.classes, LO, DIMS, OCC, 0, 0, 7)["sqdist"])
    # the int32 extremes are absent blocks; the scratch is kept by the handle and counted
    w = gpu.export_grid2d([2 ** 31 - 11, -2 ** 31, -2 ** 31 + 1], [10, 3, 2], occ=True, unknown=True, cols=True, sqdist=True, max_dist=64, min_free=1)
    assert (w["grid"] == 100).all() and (w["sqdist"] == 0).all() and w["summary"].tolist() == [30, 0, 0, 60, 60, 0]
    w = gpu.export_grid2d([2 ** 31 - 11, -2 ** 31, -2 ** 31 + 1], [10, 3, 2], cols=True, sqdist=True, dist_unobserved=True, max_dist=64, min_free=1)
    assert (w["grid"] == -1).all() and (w["sqdist"] == 0).all() and (w["cols"][..., 7] == 2).all()
    before = gpu.frame_stats()["device_bytes"]
    grid2d(gpu, LO, DIMS, OCC, C=5)
    assert gpu.frame_stats()["device_bytes"] == before
