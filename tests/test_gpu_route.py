"""mlm_export_route: the clearance-weighted cost field with face, edge and corner moves through the free space of a voxel box
(include/mlmap_hip.h), checked bit for bit against the numpy reference (tests/route_ref.py): every cost and parent value and the
three pinned summary counters.

The obstacle masks come from maps built voxel by voxel (import_blocks) and from the CPU oracle's getOccupancy /
getInflateOccupancy at the voxel centres; the class bytes (blocked, rings) from the exact squared-distance transform of the
obstacle mask of the box grown by clearance + n_penalty + 1."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import reach_ref
from tests import route_ref as ref

pytestmark = pytest.mark.gpu

OCC, INFL, UNKNOWN = 1, 2, 4
COSTS = (10, 14, 17)


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


def pack(t):
    return t[0] | t[1] << 8 | t[2] << 16


# ---- ground truth -------------------------------------------------------------------------------------------------------------
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


def oracle_mask(cpu, cfg, lo, dims, flags):
    """the obstacle mask from the CPU oracle's queries at the voxel centres"""
    p = centres(cfg, lo, dims)
    shape = (dims[2], dims[1], dims[0])
    return classes_mask(cpu.getOccupancy(p).reshape(shape), cpu.getInflateOccupancy(p).reshape(shape), flags)


def classes(mask_of, lo, dims, flags, r, n_pen):
    """class bytes of the box from an obstacle mask function (lo, dims, flags) -> [z][y][x], looked up r + n_pen + 1 voxels beyond the box"""
    g = r + n_pen + 1
    return ref.classes(mask_of([v - g for v in lo], [v + 2 * g for v in dims], flags), r, n_pen)


def rel(seeds, lo):
    return np.asarray(seeds, dtype=np.int64).reshape(-1, 3) - np.asarray(lo, dtype=np.int64)


def route(gpu, lo, dims, seeds, flags, r=0, conn=26, costs=COSTS, pen=(), max_cost=None, **ch):
    return gpu.export_route(lo, dims, seeds, occ=bool(flags & OCC), infl=bool(flags & INFL), unknown=bool(flags & UNKNOWN), clearance=r,
                            connectivity=conn, move_cost=costs, penalty=pen, max_cost=max_cost, **(ch or dict(cost=True, parent=True)))


def check(got, exp, what=""):
    for k in ("cost", "parent"):
        if k in got:
            bad = np.argwhere(got[k] != exp[k])
            assert got[k].shape == exp[k].shape and got[k].dtype == exp[k].dtype, (what, k)
            assert len(bad) == 0, f"{what} {k}: {len(bad)} differ, first at {bad[0]}: {got[k][tuple(bad[0])]} vs {exp[k][tuple(bad[0])]}"
    assert np.array_equal(got["summary"][:3], exp["summary"]), (what, got["summary"], exp["summary"])
    assert got["summary"][3] >= 1


def nearest_traversable(T, lo, v):
    """the traversable voxel nearest v (absolute; squared index distance, ties: lowest linear index), absolute"""
    iz, iy, ix = np.nonzero(T)
    d2 = (ix + lo[0] - v[0]) ** 2 + (iy + lo[1] - v[1]) ** 2 + (iz + lo[2] - v[2]) ** 2
    k = int(np.argmin(d2))  # (np.nonzero is in linear-index order, argmin takes the first)
    return [int(ix[k] + lo[0]), int(iy[k] + lo[1]), int(iz[k] + lo[2])]


# ---- maps built voxel by voxel ------------------------------------------------------------------------------------------------
def _code(v):
    v = np.asarray(v, dtype=np.int64).reshape(-1, 3) + (1 << 20)
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]


class Crafted:
    """obstacle voxels imported as OCCUPIED cells of otherwise FREE blocks; voxels of blocks not imported are UNKNOWN"""

    def __init__(self, MLMap, obstacles, free_blocks=()):
        n = S1.subbox_n
        obs = np.asarray(obstacles, dtype=np.int64).reshape(-1, 3)
        keys = np.unique(np.concatenate([np.floor_divide(obs, n), np.asarray(free_blocks, dtype=np.int64).reshape(-1, 3)]), axis=0)
        occ = np.full((len(keys), n ** 3), ord("f"), dtype=np.uint8)
        g = np.floor_divide(obs, n)
        c = obs - g * n
        row = np.searchsorted(np.sort(_code(keys)), _code(g))  # (np.unique sorts rows as _code orders them)
        assert np.array_equal(_code(keys), np.sort(_code(keys)))
        occ[row, c[:, 2] * n * n + c[:, 1] * n + c[:, 0]] = ord("o")
        self.obs, self.keys = _code(obs), _code(keys)
        self.gpu = MLMap(S1, max_blocks=4096)
        if len(keys):
            self.gpu.import_blocks(keys.astype(np.int32), np.zeros(occ.shape, np.float32), occ, np.full(occ.shape, ord("u"), np.uint8),
                                   np.zeros(len(keys), np.uint8))

    def mask(self, lo, dims, flags):
        n = S1.subbox_n
        iz, iy, ix = np.unravel_index(np.arange(dims[0] * dims[1] * dims[2]), (dims[2], dims[1], dims[0]))
        v = np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)
        is_obs = np.isin(_code(v), self.obs)
        known = np.isin(_code(np.floor_divide(v, n)), self.keys)
        occ = np.where(is_obs, 0, np.where(known, 1, -1)).reshape(dims[2], dims[1], dims[0])
        return classes_mask(occ, np.full(occ.shape, -1), flags)


def blocks_over(lo, dims, margin=0):
    """keys of the blocks that cover the box grown by margin"""
    n = S1.subbox_n
    r = [np.arange((lo[a] - margin) // n, (lo[a] + dims[a] - 1 + margin) // n + 1) for a in range(3)]
    return np.stack(np.meshgrid(*r, indexing="ij"), -1).reshape(-1, 3)


def from_blocked(MLMap, blocked, lo, margin=0):
    """a crafted map whose OCCUPIED voxels are the True voxels of blocked ([z][y][x]) placed at lo"""
    z, y, x = np.nonzero(blocked)
    dims = list(blocked.shape[::-1])
    return Crafted(MLMap, np.stack([x + lo[0], y + lo[1], z + lo[2]], axis=1), blocks_over(lo, dims, margin)), dims


def test_empty_map(mods):
    """no obstacles selected: 10 a + 4 b + 3 c over the sorted absolute offsets from the seed; with UNKNOWN nothing is traversable"""
    MLMap, _ = mods
    gpu = MLMap(S1, max_blocks=1024)
    lo, dims, seed = [-13, -5, -9], [37, 23, 11], [3, 4, -2]
    got = route(gpu, lo, dims, [seed], 0)
    z, y, x = np.indices(dims[::-1])
    s = rel(seed, lo)[0]
    d = np.sort(np.stack([abs(x - s[0]), abs(y - s[1]), abs(z - s[2])]), axis=0)
    assert np.array_equal(got["cost"], 10 * d[2] + 4 * d[1] + 3 * d[0])
    open_cls = np.zeros(dims[::-1], dtype=np.uint8)
    check(got, ref.route(open_cls, [s]), "empty")
    for flags in (OCC, OCC | INFL):  # (an empty map holds nothing OCCUPIED)
        check(route(gpu, lo, dims, [seed], flags, r=2, pen=(5, 3)), ref.route(np.full(dims[::-1], 2, dtype=np.uint8), [s], penalty=(5, 3)),
              f"empty flags={flags}")
    got = route(gpu, lo, dims, [seed], UNKNOWN)
    assert (got["cost"] == -1).all() and (got["parent"] == 255).all()
    assert tuple(got["summary"][:3]) == (0, 0, -1)
    gpu.close()


def test_walls_and_doors(mods):
    """two walls with a one-voxel door each, in windows that are not block aligned, negative, one voxel thick and a single voxel;
    several seeds, seeds on obstacles, outside the box and duplicated; the three connectivities"""
    MLMap, _ = mods
    lo, dims = [-23, -17, -9], [41, 36, 13]
    blocked = np.zeros(dims[::-1], dtype=bool)
    blocked[:, :, 12] = True
    blocked[3, 30, 12] = False
    blocked[:, 20, 12:] = True
    blocked[9, 20, 33] = False
    m, _ = from_blocked(MLMap, blocked, lo, margin=12)
    seeds = [[-20, -15, -8], [-20, -15, -8], [-11, 0, 0], [100, 0, 0], [-24, -17, -9]]  # (the third sits on the first wall)
    for conn in (6, 18, 26):
        for wlo, wd in [(lo, dims), ([-23, -17, -6], [41, 36, 1]), ([-11, -17, -9], [1, 36, 13]), ([-21, 2, -9], [30, 1, 13]), ([-20, -15, -8], [1, 1, 1])]:
            exp = ref.route(classes(m.mask, wlo, wd, OCC, 0, 0), rel(seeds, wlo), conn)
            check(route(m.gpu, wlo, wd, seeds, OCC, conn=conn), exp, f"doors {conn} {wlo} {wd}")
    exp = ref.route(np.where(blocked, ref.BLOCKED, 0).astype(np.uint8), rel(seeds, lo))
    assert exp["summary"][0] == exp["summary"][1] and exp["cost"][0, 35, 40] > 10 * 37 + 4 * 33 + 3  # (all reached, by a detour through a door)
    check(route(m.gpu, lo, dims, seeds, OCC, pen=(25, 6), costs=(3, 4, 5)), ref.route(classes(m.mask, lo, dims, OCC, 0, 2), rel(seeds, lo), 26, (3, 4, 5), (25, 6)),
          "doors with rings")
    m.gpu.close()


def test_corner_cutting(mods):
    """two obstacles at (x, y) and (x + 1, y + 1) of a slab one voxel thick stop the diagonal move between (x + 1, y) and
    (x, y + 1); a diagonal wall of such obstacles is impassable at every connectivity"""
    MLMap, _ = mods
    lo = [-3, 6, 1]
    pair = np.zeros((1, 8, 9), dtype=bool)
    pair[0, 3, 4] = pair[0, 4, 5] = True
    m, dims = from_blocked(MLMap, pair, lo)
    for conn in (18, 26):
        got = route(m.gpu, lo, dims, [[lo[0] + 5, lo[1] + 3, lo[2]]], OCC, conn=conn)
        check(got, ref.route(classes(m.mask, lo, dims, OCC, 0, 0), [[5, 3, 0]], conn), f"pair {conn}")
        assert got["cost"][0, 4, 4] > 2 * 14 and got["cost"][0, 2, 6] == 14
    m.gpu.close()
    n = 12
    wall = np.zeros((1, n, n), dtype=bool)
    wall[0, np.arange(n), np.arange(n)] = True
    m, dims = from_blocked(MLMap, wall, lo)
    y, x = np.indices((n, n))
    for conn in (6, 18, 26):
        got = route(m.gpu, lo, dims, [[lo[0] + 7, lo[1] + 2, lo[2]]], OCC, conn=conn)
        check(got, ref.route(classes(m.mask, lo, dims, OCC, 0, 0), [[7, 2, 0]], conn), f"wall {conn}")
        assert ((got["cost"][0] >= 0) == (x > y)).all()
    m.gpu.close()


def test_penalty_pulls_path_to_the_middle(mods):
    """a corridor 7 wide: with penalties the path from the far end keeps to the centre line; the clearances 0..3 with the penalty;
    an obstacle one voxel outside the box raises the ring class of voxels inside it"""
    MLMap, _ = mods
    lo, dims = [0, 0, 0], [30, 9, 1]
    obs = [(x, y, 0) for x in range(-8, 38) for y in (0, 8)]
    m = Crafted(MLMap, obs, blocks_over([-8, -8, -8], [46, 24, 16]))
    seed, pen = [1, 4, 0], (50, 20, 5)
    exp = ref.route(classes(m.mask, lo, dims, OCC, 0, 3), [seed], 18, COSTS, pen)
    got = route(m.gpu, lo, dims, [seed], OCC, conn=18, pen=pen)
    check(got, exp, "corridor")
    assert all(p[1] == 4 for p in ref.walk(got["parent"], (29, 4, 0)))
    plain = route(m.gpu, lo, dims, [seed], OCC, conn=18)
    check(plain, ref.route(classes(m.mask, lo, dims, OCC, 0, 0), [seed], 18), "corridor, no penalty")
    assert not np.array_equal(plain["cost"], got["cost"])
    for r in range(0, 4):
        cls = classes(m.mask, lo, dims, OCC, r, 3)
        check(route(m.gpu, lo, dims, [seed], OCC, r=r, conn=18, pen=pen), ref.route(cls, [seed], 18, COSTS, pen), f"corridor r={r}")
        assert (cls[0, 4, 15] != ref.BLOCKED) == (r <= 3)
    m.gpu.close()
    # the obstacle (-1, 4, 0), one voxel beyond the -x face
    m = Crafted(MLMap, obs + [(-1, 4, 0)], blocks_over([-8, -8, -8], [46, 24, 16]))
    cls = classes(m.mask, lo, dims, OCC, 0, 3)
    assert cls[0, 4, 0] == 0 and cls[0, 4, 1] == 1 and exp["cost"][0, 4, 0] != -1
    got = route(m.gpu, lo, dims, [seed], OCC, conn=18, pen=pen)
    check(got, ref.route(cls, [seed], 18, COSTS, pen), "obstacle outside the box")
    assert got["cost"][0, 4, 0] == exp["cost"][0, 4, 0] + 50  # (ring 0 instead of the free centre line, four voxels from either wall)
    m.gpu.close()


def test_serpentine_slab(mods, knobs):
    """optimal paths many times the box edge: hundreds of sweeps, every tile entered again and again; the same bytes under other
    tiles and sweep groups"""
    MLMap, _ = mods
    lo = [-30, 5, 2]
    m, dims = from_blocked(MLMap, reach_ref.serpentine_slab(64, 64), lo)
    cls = classes(m.mask, lo, dims, OCC, 0, 0)
    base = {}
    for conn in (6, 26):
        exp = ref.route(cls, [[0, 0, 0]], conn)
        assert exp["summary"][2] >= 10 * 20 * 64 and exp["summary"][1] == exp["summary"][0]
        base[conn] = route(m.gpu, lo, dims, [lo], OCC, conn=conn)
        check(base[conn], exp, f"slab {conn}")
    for name, v in (("route_group", 1), ("route_group", 64), ("route_tile", pack((1, 1, 1))), ("route_tile", pack((5, 3, 2)))):
        knobs.set(name, v)
        for conn in (6, 26):
            again = route(m.gpu, lo, dims, [lo], OCC, conn=conn)
            for k in ("cost", "parent"):
                assert again[k].tobytes() == base[conn][k].tobytes(), (name, v, conn, k)
            assert np.array_equal(again["summary"][:3], base[conn]["summary"][:3])
    m.gpu.close()


# ---- real maps ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s1_maps(mods):
    """S1 after six room_jitter frames, inflate_map after the third and the fifth, on the GPU and in the oracle; the last position"""
    MLMap, OracleMap = mods
    gpu, cpu = MLMap(S1, max_blocks=8192), OracleMap(S1)
    for k, (img, (q, t)) in enumerate(syn.stream(S1, "room_jitter", "smooth", 6)):
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
        if k in (2, 4):
            gpu.inflate_map(t)
            cpu.inflate_map(t)
    yield gpu, cpu, [int(np.floor(v / S1.subbox_d_xyz)) for v in t]
    gpu.close()


def vehicle_window(vehicle):
    return [vehicle[0] - 30, vehicle[1] - 25, vehicle[2] - 8], [61, 47, 17]


@pytest.mark.parametrize("flags", [OCC, OCC | INFL, OCC | UNKNOWN])
def test_equals_export_reach(s1_maps, flags):
    """connectivity 6, unit cost, no penalty: export_reach's steps and parent, the seed code 26 in place of 6"""
    gpu, cpu, vehicle = s1_maps
    lo, dims = vehicle_window(vehicle)
    f = dict(occ=bool(flags & OCC), infl=bool(flags & INFL), unknown=bool(flags & UNKNOWN))
    for r, ms in ((0, None), (0, 25), (2, None)):
        seed = nearest_traversable(classes(lambda l, d, g: oracle_mask(cpu, S1, l, d, g), lo, dims, flags, r, 0) != ref.BLOCKED, lo, vehicle)
        a = gpu.export_reach(lo, dims, [seed], clearance=r, max_steps=ms, steps=True, parent=True, **f)
        b = gpu.export_route(lo, dims, [seed], clearance=r, connectivity=6, move_cost=(1, 1, 1), max_cost=ms, cost=True, parent=True, **f)
        print(f"flags={flags} r={r} max_steps={ms}: reached {a['summary'][1]}")
        assert ms is not None or a["summary"][1] > 500
        assert np.array_equal(b["cost"], a["steps"]), (flags, r, ms)
        assert np.array_equal(b["parent"], np.where(a["parent"] == 6, 26, a["parent"])), (flags, r, ms)
        assert np.array_equal(b["summary"][:3], a["summary"][:3])


def test_real_map_against_oracle(s1_maps, knobs):
    """the window around the vehicle, class bytes from the oracle's classes at the voxel centres, connectivity 26, clearance 1,
    two rings; max_cost at two values; the same bytes from a tile whose LDS goes beyond 64 KB"""
    gpu, cpu, vehicle = s1_maps
    lo, dims = vehicle_window(vehicle)
    flags, r, pen = OCC | UNKNOWN, 1, (30, 10)
    cls = classes(lambda l, d, f: oracle_mask(cpu, S1, l, d, f), lo, dims, flags, r, len(pen))
    seed = nearest_traversable(cls != ref.BLOCKED, lo, vehicle)
    exp = ref.route(cls, rel(seed, lo), 26, COSTS, pen)
    print(f"window {lo} {dims}: summary {exp['summary']}, ring voxels {[int((cls == k).sum()) for k in range(3)]}")
    reached = exp["cost"] >= 0
    assert exp["summary"][1] > 500 and all((reached & (cls == k)).any() for k in range(len(pen) + 1))  # (not vacuous: every ring is entered)
    got = route(gpu, lo, dims, [seed], flags, r=r, pen=pen)
    print(f"  sweeps {got['summary'][3]}")
    check(got, exp, "real map")
    top = int(exp["summary"][2])
    for mc in (top // 4, top // 2):
        cut = route(gpu, lo, dims, [seed], flags, r=r, pen=pen, max_cost=mc)
        check(cut, ref.truncate(exp, mc), f"max_cost={mc}")
        assert np.array_equal(cut["cost"] >= 0, reached & (exp["cost"] <= mc))
    knobs.set("route_tile", pack((23, 23, 22)))  # (4 * 25 * 25 * 24 + 2 * 23 * 23 * 22 = 83 276 B of LDS)
    big = route(gpu, lo, dims, [seed], flags, r=r, pen=pen)
    for k in ("cost", "parent"):
        assert big[k].tobytes() == got[k].tobytes(), k


def test_frontier_mode(mods):
    """frontier mode with subbox_n = 5 (released blocks answer from element 0, infl UNKNOWN) against the oracle's classes"""
    MLMap, OracleMap = mods
    cfg = S1.with_(use_exploration_frontiers=True, subbox_n=5)
    gpu, cpu = MLMap(cfg, max_blocks=16384, max_batch=2), OracleMap(cfg)
    for img, (q, t) in syn.stream(cfg, "room_jitter", "smooth", 8):
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
    assert cpu.export_blocks()["collapsed"].sum() > 20
    vehicle = [int(np.floor(v / cfg.subbox_d_xyz)) for v in t]
    lo, dims = [vehicle[0] - 28, vehicle[1] - 30, vehicle[2] - 7], [57, 55, 15]
    for flags, r, pen in ((OCC | UNKNOWN, 1, (12,)), (OCC | INFL | UNKNOWN, 0, (12, 4))):
        cls = classes(lambda l, d, f: oracle_mask(cpu, cfg, l, d, f), lo, dims, flags, r, len(pen))
        seed = nearest_traversable(cls != ref.BLOCKED, lo, vehicle)
        exp = ref.route(cls, rel(seed, lo), 26, COSTS, pen)
        assert exp["summary"][1] > 500
        check(route(gpu, lo, dims, [seed], flags, r=r, pen=pen), exp, f"frontier flags={flags}")
    gpu.close()


# ---- destinations, modes, arguments ------------------------------------------------------------------------------------------
def test_async_stream_and_device_destinations(mods):
    """async mode: the field sees every submitted frame; the caller's stream, device seeds and device tensors give the host result;
    the scratch grows at the first call and stays"""
    import torch

    MLMap, OracleMap = mods
    nf = 8
    frames = np.stack([img for img, _ in syn.stream(S1, "room_jitter", "smooth", nf)])
    poses = syn.smooth_trajectory(nf, 42)
    q, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    gpu, cpu = MLMap(S1, max_blocks=8192, max_batch=4), OracleMap(S1)
    for k in range(nf):
        cpu.update_depth(frames[k], q[k], t[k])
    before = gpu.frame_stats()["device_bytes"]
    gpu.set_async(True)
    gpu.update_map_batch(frames, q, t)  # no sync()
    vehicle = [int(np.floor(v / S1.subbox_d_xyz)) for v in t[-1]]
    lo, dims = vehicle_window(vehicle)
    flags, r, pen = OCC | UNKNOWN, 1, (9, 4)
    cls = classes(lambda l, d, f: oracle_mask(cpu, S1, l, d, f), lo, dims, flags, r, len(pen))
    seed = nearest_traversable(cls != ref.BLOCKED, lo, vehicle)
    exp = ref.route(cls, rel(seed, lo), 26, COSTS, pen)
    assert exp["summary"][1] > 500
    w = route(gpu, lo, dims, [seed], flags, r=r, pen=pen)
    check(w, exp, "async")
    grown_bytes = gpu.frame_stats()["device_bytes"]
    assert grown_bytes > before
    route(gpu, lo, dims, [seed], flags, r=r, pen=pen)
    assert gpu.frame_stats()["device_bytes"] == grown_bytes

    s = torch.cuda.Stream()
    gpu.set_stream(s.cuda_stream)
    shape = (dims[2], dims[1], dims[0])
    dev = {"cost": torch.empty(shape, dtype=torch.int32, device="cuda"), "parent": torch.empty(shape, dtype=torch.uint8, device="cuda")}
    seeds_dev = torch.tensor([seed, seed], dtype=torch.int32, device="cuda")
    junk = torch.ones(1 << 26, device="cuda")
    with torch.cuda.stream(s):
        for _ in range(50):  # (keeps the caller's stream busy: the field is written behind this work)
            junk.mul_(1.0001)
        for v in dev.values():
            v.fill_(7)
    torch.cuda.current_stream().synchronize()  # (seeds_dev is written)
    kw = dict(occ=True, unknown=True, clearance=r, penalty=pen)
    sm = gpu.export_route_dev(lo, dims, seeds_dev.data_ptr(), 2, summary=True, **kw, **{k: v.data_ptr() for k, v in dev.items()})
    for k, v in dev.items():
        assert np.array_equal(v.cpu().numpy(), w[k]), k
    assert np.array_equal(sm[:3], exp["summary"])
    assert gpu.export_route_dev(lo, dims, seeds_dev.data_ptr(), 2, cost=dev["cost"].data_ptr(), **kw) is None
    assert gpu.frame_stats()["device_bytes"] == grown_bytes
    only = gpu.export_route(lo, dims, [seed], cost=False, parent=False, **kw)  # the summary alone
    assert set(only) == {"summary"} and np.array_equal(only["summary"][:3], exp["summary"])
    gpu.close()


def test_invalid_arguments(mods):
    """each refused argument gives MLM_ERR_INVALID and leaves the handle usable"""
    MLMap, _ = mods
    gpu = MLMap(S1, max_blocks=1024)
    L, h = gpu._L, gpu._h
    buf = np.zeros(1 << 16, dtype=np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    seed = np.zeros(3, dtype=np.int32)
    sp = seed.ctypes.data_as(ctypes.c_void_p)
    sm = np.zeros(4, dtype=np.int64)
    none = object()

    def call(lo=(0, 0, 0), dims=(4, 4, 4), seeds=sp, n=1, flags=0, r=0, conn=6, mc=(1, 1, 1), pen=(), npen=None, ms=100, outs=(p, None, None)):
        lo_a, dims_a = np.array(lo, dtype=np.int32), np.array(dims, dtype=np.int32)
        mc_a = None if mc is none else np.array(mc, dtype=np.int32)
        pen_a = None if pen is none or len(pen) == 0 else np.array(pen, dtype=np.int32)
        return L.mlm_export_route(h, lo_a.ctypes.data_as(ctypes.c_void_p), dims_a.ctypes.data_as(ctypes.c_void_p), seeds, n, flags, r, conn,
                                  None if mc_a is None else mc_a.ctypes.data_as(ctypes.c_void_p),
                                  None if pen_a is None else pen_a.ctypes.data_as(ctypes.c_void_p),
                                  (0 if pen_a is None else len(pen_a)) if npen is None else npen, ms, *outs)

    bad = [dict(dims=(0, 4, 4)), dict(dims=(4, -1, 4)), dict(dims=(4, 4, 0)), dict(dims=(2048, 2048, 1024)), dict(dims=(65536, 32768, 1)),
           dict(lo=(2 ** 31 - 10, 0, 0), dims=(20, 1, 1)), dict(lo=(0, 0, 2 ** 31 - 1), dims=(1, 1, 1)),
           dict(n=0), dict(n=-1), dict(seeds=None), dict(flags=8), dict(flags=OCC | 16), dict(flags=-1), dict(flags=1 << 30),
           dict(r=-1), dict(r=64), dict(r=1 << 20), dict(conn=0), dict(conn=4), dict(conn=7), dict(conn=27), dict(conn=-6),
           dict(mc=none), dict(mc=(0, 1, 1)), dict(conn=18, mc=(1, 65536, 1)), dict(conn=26, mc=(1, 1, -3)), dict(conn=18, mc=(1, 0, 1)),
           dict(npen=-1), dict(pen=(1,) * 64), dict(r=60, pen=(1, 1, 1, 1)), dict(pen=none, npen=2), dict(pen=(5, -1)), dict(pen=(65536,)),
           dict(ms=0), dict(ms=-5), dict(outs=(None, None, None))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert call() == 0
    assert call(conn=6, mc=(1, 0, -7)) == 0 and call(conn=18, mc=(1, 1, 1 << 20)) == 0  # (entries of excluded move kinds are ignored)
    assert call() == 0
    assert (buf[:64].reshape(4, 4, 4) == np.add.outer(np.add.outer(np.arange(4), np.arange(4)), np.arange(4))).all()
    assert call(r=60, pen=(1, 2, 3), flags=7, conn=26, mc=(65535, 65535, 65535), ms=2 ** 31 - 1, outs=(None, None, sm.ctypes.data_as(ctypes.c_void_p))) == 0
    assert tuple(sm[:3]) == (0, 0, -1)  # (an empty map: every voxel UNKNOWN)
    w = gpu.export_route([2 ** 31 - 11, -2 ** 31, 0], [10, 3, 2], [[2 ** 31 - 11, -2 ** 31, 0]], occ=True, clearance=60, penalty=(7, 7, 7), parent=True)
    assert w["cost"].max() == 10 * 9 + 4 * 2 + 3 and tuple(w["summary"][:3]) == (60, 60, 101)  # the int32 extremes: absent blocks, nothing OCCUPIED
    assert w["parent"][1, 2, 9] == 0 and w["parent"][1, 1, 1] == 18 and w["parent"][0, 0, 0] == 26  # (face moves win ties)
    gpu.close()
