"""mlm_export_clusters: connected components of a voxel set of a box with per-component statistics (include/mlmap_hip.h), checked
bit for bit against the breadth-first ground truth in plain numpy (tests/cluster_ref.py): every label, every table row and
summary[0..4].

The sets come from maps built voxel by voxel (import_blocks) and from the CPU oracle's getOccupancy / getInflateOccupancy at the
voxel centres of the box grown by one voxel."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import cluster_ref as ref

pytestmark = pytest.mark.gpu

OCC, INFL, UNKNOWN, FRONTIER = 1, 2, 4, 16
CONNS = (6, 18, 26)
TILES = [(32, 8, 8), (1, 5, 3), (4, 4, 4), (7, 1, 2), (64, 2, 1)]


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


def oracle_classes(cpu, cfg, lo, dims):
    """(occ, infl) [z][y][x] from the CPU oracle's queries at the voxel centres"""
    p = centres(cfg, lo, dims)
    shape = (dims[2], dims[1], dims[0])
    return cpu.getOccupancy(p).reshape(shape).astype(np.int32), cpu.getInflateOccupancy(p).reshape(shape).astype(np.int32)


def set_of(classes_of, lo, dims, flags):
    """S of the box from a function (lo, dims) -> (occ, infl); the frontier looks one voxel beyond the box"""
    if flags == FRONTIER:
        occ, _ = classes_of([v - 1 for v in lo], [v + 2 for v in dims])
        return ref.frontier_set(occ)
    occ, infl = classes_of(lo, dims)
    return ref.class_set(occ, infl, bool(flags & OCC), bool(flags & INFL), bool(flags & UNKNOWN))


def clusters(gpu, lo, dims, flags, conn=26, min_size=1, **kw):
    return gpu.export_clusters(lo, dims, frontier=bool(flags & FRONTIER), occ=bool(flags & OCC), infl=bool(flags & INFL),
                               unknown=bool(flags & UNKNOWN), connectivity=conn, min_size=min_size, **kw)


def check(got, exp, what=""):
    if "labels" in got:
        assert got["labels"].shape == exp["labels"].shape and got["labels"].dtype == exp["labels"].dtype, what
        bad = np.argwhere(got["labels"] != exp["labels"])
        assert len(bad) == 0, f"{what} labels: {len(bad)} differ, first at {bad[0]}: {got['labels'][tuple(bad[0])]} vs {exp['labels'][tuple(bad[0])]}"
    assert np.array_equal(got["summary"][:5], exp["summary"]), (what, got["summary"], exp["summary"])
    assert (got["summary"][5] >= 1) == (exp["summary"][0] > 0), (what, got["summary"])
    if "table" in got:
        rows = len(got["table"])
        assert rows <= len(exp["table"]) and np.array_equal(got["table"], exp["table"][:rows]), what


def check_all(gpu, S, lo, dims, flags, what, conns=CONNS, min_sizes=(1, 8)):
    out = None
    for conn in conns:
        for ms in min_sizes:
            exp = ref.clusters(S, conn, ms, None, lo)
            K = int(exp["summary"][2])
            got = clusters(gpu, lo, dims, flags, conn, ms, cap=K + 1)
            assert len(got["table"]) == K
            check(got, exp, f"{what} conn={conn} min_size={ms}")
            out = out or exp
    return out


# ---- maps built voxel by voxel ------------------------------------------------------------------------------------------------
def _code(v):
    v = np.asarray(v, dtype=np.int64).reshape(-1, 3) + (1 << 20)
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]


class Crafted:
    """voxels imported as OCCUPIED cells of otherwise FREE blocks; voxels of blocks not imported are UNKNOWN (the pattern of
    tests/test_gpu_reach.py, answering with the classes instead of a mask)"""

    def __init__(self, MLMap, occupied, free_blocks=()):
        n = S1.subbox_n
        obs = np.asarray(occupied, dtype=np.int64).reshape(-1, 3)
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

    def classes(self, lo, dims):
        n = S1.subbox_n
        iz, iy, ix = np.unravel_index(np.arange(dims[0] * dims[1] * dims[2]), (dims[2], dims[1], dims[0]))
        v = np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)
        is_obs = np.isin(_code(v), self.obs)
        inside = (np.abs(np.floor_divide(v, n)) < (1 << 20)).all(1)  # (beyond the key range no block exists)
        known = inside & np.isin(_code(np.where(inside[:, None], np.floor_divide(v, n), 0)), self.keys)
        occ = np.where(is_obs, 0, np.where(known, 1, -1)).reshape(dims[2], dims[1], dims[0])
        return occ, np.full(occ.shape, -1)


def blocks_over(lo, dims, margin=0):
    n = S1.subbox_n
    r = [np.arange((lo[a] - margin) // n, (lo[a] + dims[a] - 1 + margin) // n + 1) for a in range(3)]
    return np.stack(np.meshgrid(*r, indexing="ij"), -1).reshape(-1, 3)


def from_mask(MLMap, S, lo):
    """a crafted map whose OCCUPIED voxels are the True voxels of S ([z][y][x]) placed at lo, FREE around them"""
    z, y, x = np.nonzero(S)
    dims = list(S.shape[::-1])
    return Crafted(MLMap, np.stack([x + lo[0], y + lo[1], z + lo[2]], axis=1), blocks_over(lo, dims, 1)), dims


def crafted_masks():
    rng = np.random.default_rng(8)
    shape = (13, 27, 45)  # no multiple of the default tile
    for density in (0.1, 0.3, 0.5, 0.9):
        yield f"random {density}", rng.random(shape) < density
    yield "serpentine", ~ref.serpentine_3d(32)
    yield "serpentine walls", ref.serpentine_3d(24)
    yield "checkerboard", ref.checkerboard((9, 17, 35))
    corner = np.zeros((17, 17, 65), dtype=bool)
    corner[7, 7, 31] = corner[8, 8, 32] = True  # either side of a corner of the default tile
    yield "corner", corner
    yield "empty", np.zeros((3, 9, 40), dtype=bool)
    yield "full", np.ones((9, 10, 35), dtype=bool)
    yield "one voxel", np.ones((1, 1, 1), dtype=bool)


def test_crafted_masks_as_occupied(mods):
    """the masks of the CPU test as OCCUPIED voxels at a negative origin that is no multiple of the block edge"""
    MLMap, _ = mods
    lo = [-29, -13, 3]
    for name, S in crafted_masks():
        m, dims = from_mask(MLMap, S, lo)
        assert np.array_equal(set_of(m.classes, lo, dims, OCC), S)
        exp = check_all(m.gpu, S, lo, dims, OCC, name, min_sizes=(1, 8) if S.size > 1 else (1,))
        if name == "serpentine":
            assert tuple(ref.clusters(S, 6)["summary"]) == (S.sum(), 1, 1, S.sum(), S.sum())
        if name == "corner":
            assert exp["summary"][1] == 2 and ref.clusters(S, 26)["summary"][1] == 1
        m.gpu.close()


def test_class_sets_and_frontier_on_a_crafted_map(mods):
    """OCC, UNKNOWN, OCC | UNKNOWN and the frontier where only some blocks exist; boxes that reach beyond them"""
    MLMap, _ = mods
    rng = np.random.default_rng(4)
    n = S1.subbox_n
    blocks = np.argwhere(rng.random((5, 4, 3)) < 0.6) - [2, 2, 1]
    occupied = np.concatenate([b * n + rng.integers(0, n, size=(40, 3)) for b in blocks])
    m = Crafted(MLMap, occupied, blocks)
    for lo, dims in [([-2 * n - 3, -2 * n - 1, -n - 2], [5 * n + 7, 4 * n + 3, 3 * n + 5]), ([-5, -7, 1], [33, 9, 9]), ([3, -9, 0], [1, 30, 11])]:
        for flags in (OCC, UNKNOWN, OCC | UNKNOWN, FRONTIER):
            S = set_of(m.classes, lo, dims, flags)
            assert flags == OCC and dims[0] == 1 or S.any()
            check_all(m.gpu, S, lo, dims, flags, f"crafted {lo} {dims} flags={flags}")
    m.gpu.close()


def test_frontier_looks_beyond_the_box(mods):
    """a box that holds FREE voxels only: its frontier is the shell whose UNKNOWN neighbours lie outside the box; and a box at the
    int32 edge, where the neighbours' indices leave int32"""
    MLMap, _ = mods
    n = S1.subbox_n
    lo, dims = [-n, 2 * n, 0], [2 * n, n, n]
    m = Crafted(MLMap, np.zeros((0, 3)), blocks_over(lo, dims))
    S = set_of(m.classes, lo, dims, FRONTIER)
    shell = np.ones(dims[::-1], dtype=bool)
    shell[1:-1, 1:-1, 1:-1] = False
    assert np.array_equal(S, shell)
    check_all(m.gpu, S, lo, dims, FRONTIER, "shell")
    inner_lo, inner = [lo[0] + 1, lo[1] + 1, lo[2] + 1], [dims[0] - 2, dims[1] - 2, dims[2] - 2]
    got = clusters(m.gpu, inner_lo, inner, FRONTIER)
    assert not got["summary"].any() and (got["labels"] == ref.NONE).all() and len(got["table"]) == 0
    # one face of the box on the border of the known blocks: the UNKNOWN neighbours are all outside the box
    face_lo, face = [lo[0], lo[1] + 2, lo[2] + 2], [3, dims[1] - 4, dims[2] - 4]
    S = set_of(m.classes, face_lo, face, FRONTIER)
    assert S[:, :, 0].all() and not S[:, :, 1:].any()
    check_all(m.gpu, S, face_lo, face, FRONTIER, "face")
    for elo, ed in [([2 ** 31 - 11, -2 ** 31, 0], [10, 3, 2]), ([-2 ** 31, 2 ** 31 - 4, -2 ** 31], [2, 3, 4])]:
        for flags in (FRONTIER, UNKNOWN, OCC):
            S = set_of(m.classes, elo, ed, flags)
            assert S.all() if flags == UNKNOWN else not S.any()
            check_all(m.gpu, S, elo, ed, flags, f"int32 edge {elo} flags={flags}")
    m.gpu.close()


# ---- real maps ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s1_maps(mods):
    """S1 after 64 room_jitter frames, inflate_map every 16th, on the GPU and in the oracle; the last position"""
    MLMap, OracleMap = mods
    gpu, cpu = MLMap(S1, max_blocks=16384), OracleMap(S1)
    for k, (img, (q, t)) in enumerate(syn.stream(S1, "room_jitter", "smooth", 64)):
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
        if k % 16 == 15:
            gpu.inflate_map(t)
            cpu.inflate_map(t)
    yield gpu, cpu, [int(np.floor(v / S1.subbox_d_xyz)) for v in t]
    gpu.close()


def window_classes(gpu):
    def f(lo, dims):
        w = gpu.export_window(lo, dims, odds=False, occ=True, infl=True)
        return w["occ"].astype(np.int32), w["infl"].astype(np.int32)

    return f


def room_invariants(gpu, lo, dims, got, flags):
    """what holds without any reference"""
    t, sm = got["table"], got["summary"]
    assert sm[3] == t[:, 0].sum() and sm[2] == len(t) and (sm[4] >= t[:, 0]).all()
    lin = ((t[:, 3] - lo[2]) * dims[1] + (t[:, 2] - lo[1])) * dims[0] + (t[:, 1] - lo[0])
    assert (np.diff(lin) > 0).all()  # rows are sorted by root
    assert (t[:, 4:7] <= t[:, 1:4]).all() and (t[:, 1:4] <= t[:, 7:10]).all()
    cen = np.asarray(lo) + t[:, 10:13] / t[:, :1]
    assert (t[:, 4:7] <= cen).all() and (cen <= t[:, 7:10]).all()
    assert not t[:, 14:].any()
    if flags == FRONTIER:
        occ = gpu.export_window(lo, dims, odds=False, occ=True)["occ"]
        assert (occ[got["labels"] != ref.NONE] == 1).all()


@pytest.mark.parametrize("flags", [FRONTIER, OCC | INFL])
def test_room_map_against_oracle(s1_maps, flags):
    """a window on the room map: S from the oracle's classes at the centres of the (grown) box, and the same S rebuilt from this
    library's own export_window"""
    gpu, cpu, vehicle = s1_maps
    lo, dims = [vehicle[0] - 50, vehicle[1] - 60, vehicle[2] - 14], [117, 121, 29]
    S = set_of(lambda l, d: oracle_classes(cpu, S1, l, d), lo, dims, flags)
    assert np.array_equal(S, set_of(window_classes(gpu), lo, dims, flags))
    exp = check_all(gpu, S, lo, dims, flags, f"room flags={flags}")
    print(f"flags={flags} window {lo} {dims}: summary at 6 / min_size 1 {exp['summary']}")
    assert exp["summary"][0] > 2000 and exp["summary"][1] > 3  # (the test does not pass on an empty or trivial set)
    for ms in (1, 8):
        room_invariants(gpu, lo, dims, clusters(gpu, lo, dims, flags, 26, ms), flags)


def test_frontier_mode_with_inflation(mods):
    """a frontier-mode handle with inflation, as the shipped real-data configuration runs: released blocks answer from element 0;
    the class-defined frontier does not depend on the mode's bookkeeping"""
    MLMap, OracleMap = mods
    cfg = S1.with_(use_exploration_frontiers=True, subbox_n=5)
    gpu, cpu = MLMap(cfg, max_blocks=16384, max_batch=2), OracleMap(cfg)
    for k, (img, (q, t)) in enumerate(syn.stream(cfg, "room_jitter", "smooth", 8)):
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
        if k in (3, 6):
            gpu.inflate_map(t)
            cpu.inflate_map(t)
    b = cpu.export_blocks()
    assert b["collapsed"].sum() > 20
    n = cfg.subbox_n
    lo = [int(v) for v in b["keys"].min(0) * n - 7]
    dims = [min(int(v), 120) for v in (b["keys"].max(0) + 2) * n - 4 - np.array(lo)]
    for flags in (FRONTIER, OCC | INFL):
        S = set_of(lambda l, d: oracle_classes(cpu, cfg, l, d), lo, dims, flags)
        assert S.sum() > 500
        assert np.array_equal(S, set_of(window_classes(gpu), lo, dims, flags))
        check_all(gpu, S, lo, dims, flags, f"frontier mode flags={flags}")
        room_invariants(gpu, lo, dims, clusters(gpu, lo, dims, flags, 26, 8), flags)
    gpu.close()


def test_large_window(s1_maps):
    """512 x 512 x 64 around the room, frontier at 26, against the ground truth on this library's own classes"""
    gpu, _, _ = s1_maps
    lo, dims = [-250, -240, -20], [512, 512, 64]
    S = set_of(window_classes(gpu), lo, dims, FRONTIER)
    exp = ref.clusters(S, 26, 8, None, lo)
    assert exp["summary"][0] > 1000  # (the room's frontier: a few thousand voxels)
    got = clusters(gpu, lo, dims, FRONTIER, 26, 8, cap=int(exp["summary"][2]))
    print(f"large window: summary {got['summary']}")
    check(got, exp, "large")
    room_invariants(gpu, lo, dims, got, FRONTIER)


# ---- destinations, geometries, modes, arguments -------------------------------------------------------------------------------
def test_destinations_and_cap(s1_maps):
    """host and device destinations give identical bytes; each output alone; K > cap"""
    import torch

    gpu, _, vehicle = s1_maps
    lo, dims = [vehicle[0] - 50, vehicle[1] - 60, vehicle[2] - 14], [117, 121, 29]  # (6-connected, the room's frontier falls into dozens of pieces here)
    host = clusters(gpu, lo, dims, FRONTIER, 6, 1, cap=1 << 16)
    K = int(host["summary"][2])
    assert 8 < K <= 1 << 16 and len(host["table"]) == K
    check(host, ref.clusters(set_of(window_classes(gpu), lo, dims, FRONTIER), 6, 1, None, lo), "host")
    shape = (dims[2], dims[1], dims[0])
    lab = torch.full(shape, 7, dtype=torch.int32, device="cuda")
    tab = torch.full((K + 3, 16), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    sm = gpu.export_clusters_dev(lo, dims, frontier=True, connectivity=6, labels=lab.data_ptr(), table=tab.data_ptr(), cap=K + 3, summary=True)
    assert np.array_equal(lab.cpu().numpy(), host["labels"]) and np.array_equal(tab[:K].cpu().numpy(), host["table"])
    assert (tab[K:] == 7).all() and np.array_equal(sm[:5], host["summary"][:5])
    # each output alone
    only = clusters(gpu, lo, dims, FRONTIER, 6, 1, labels=True, cap=0)
    assert set(only) == {"labels", "summary"} and np.array_equal(only["labels"], host["labels"])
    only = clusters(gpu, lo, dims, FRONTIER, 6, 1, labels=False, cap=1 << 16)
    assert set(only) == {"table", "summary"} and np.array_equal(only["table"], host["table"])
    only = clusters(gpu, lo, dims, FRONTIER, 6, 1, labels=False, cap=0)
    assert set(only) == {"summary"} and np.array_equal(only["summary"][:5], host["summary"][:5])
    lab.fill_(7)
    torch.cuda.synchronize()
    assert gpu.export_clusters_dev(lo, dims, frontier=True, connectivity=6, labels=lab.data_ptr()) is None
    assert np.array_equal(lab.cpu().numpy(), host["labels"])
    tab.fill_(7)
    torch.cuda.synchronize()
    gpu.export_clusters_dev(lo, dims, frontier=True, connectivity=6, table=tab.data_ptr(), cap=K)
    assert np.array_equal(tab[:K].cpu().numpy(), host["table"]) and (tab[K:] == 7).all()
    # K > cap: the first rows, labels complete
    few = clusters(gpu, lo, dims, FRONTIER, 6, 1, cap=5)
    assert few["summary"][2] == K and np.array_equal(few["table"], host["table"][:5]) and np.array_equal(few["labels"], host["labels"])
    tab.fill_(7)
    torch.cuda.synchronize()
    gpu.export_clusters_dev(lo, dims, frontier=True, connectivity=6, table=tab.data_ptr(), cap=5)
    assert np.array_equal(tab[:5].cpu().numpy(), host["table"][:5]) and (tab[5:] == 7).all()


def test_forced_tiles(s1_maps, knobs):
    """every tile geometry gives the default's bytes (only summary[5] may differ)"""
    gpu, _, vehicle = s1_maps
    lo, dims = [vehicle[0] - 50, vehicle[1] - 60, vehicle[2] - 14], [117, 121, 29]  # (the window of test_room_map_against_oracle)
    for flags, conn in ((FRONTIER, 6), (OCC | INFL, 26), (UNKNOWN, 18)):
        base = clusters(gpu, lo, dims, flags, conn, 2)
        assert base["summary"][1] >= 1
        for T in TILES[1:] + [(1, 1, 1), (64, 13, 13)]:
            knobs.set("cluster_tile", pack(T))
            got = clusters(gpu, lo, dims, flags, conn, 2)
            assert np.array_equal(got["labels"], base["labels"]) and np.array_equal(got["table"], base["table"]), (flags, T)
            assert np.array_equal(got["summary"][:5], base["summary"][:5]), (flags, T)
        knobs.set("cluster_tile", pack(TILES[0]))


def test_async_stream_and_scratch(mods):
    """async mode: the call sees every submitted frame; the caller's stream gives the same bytes; the scratch grows at the first
    call and stays"""
    import torch

    MLMap, _ = mods
    nf = 8
    frames = np.stack([img for img, _ in syn.stream(S1, "room_jitter", "smooth", nf)])
    poses = syn.smooth_trajectory(nf, 42)
    q, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    sync = MLMap(S1, max_blocks=8192, max_batch=4)
    sync.update_map_batch(frames, q, t)
    sync.sync()
    v = [int(np.floor(x / S1.subbox_d_xyz)) for x in t[-1]]
    lo, dims = [v[0] - 45, v[1] - 45, v[2] - 12], [91, 93, 25]
    exp = clusters(sync, lo, dims, FRONTIER, 26, 2)
    assert exp["summary"][0] > 500
    check(exp, ref.clusters(set_of(window_classes(sync), lo, dims, FRONTIER), 26, 2, None, lo), "synced")
    sync.close()

    gpu = MLMap(S1, max_blocks=8192, max_batch=4)
    before = gpu.frame_stats()["device_bytes"]
    gpu.set_async(True)
    gpu.update_map_batch(frames, q, t)  # no sync()
    got = clusters(gpu, lo, dims, FRONTIER, 26, 2)
    for k in ("labels", "table"):
        assert np.array_equal(got[k], exp[k]), k
    assert np.array_equal(got["summary"][:5], exp["summary"][:5])
    grown = gpu.frame_stats()["device_bytes"]
    nvox = dims[0] * dims[1] * dims[2]
    assert grown - before >= 9 * nvox + (dims[0] + 2) * (dims[1] + 2) * (dims[2] + 2)
    clusters(gpu, lo, dims, FRONTIER, 26, 2)
    assert gpu.frame_stats()["device_bytes"] == grown

    s = torch.cuda.Stream()
    gpu.set_stream(s.cuda_stream)
    lab = torch.empty((dims[2], dims[1], dims[0]), dtype=torch.int32, device="cuda")
    tab = torch.zeros((len(exp["table"]) + 1, 16), dtype=torch.int64, device="cuda")
    junk = torch.ones(1 << 26, device="cuda")
    with torch.cuda.stream(s):
        for _ in range(50):  # (keeps the caller's stream busy: the outputs are written behind this work)
            junk.mul_(1.0001)
        lab.fill_(7)
    sm = gpu.export_clusters_dev(lo, dims, frontier=True, min_size=2, labels=lab.data_ptr(), table=tab.data_ptr(), cap=len(tab), summary=True)
    assert np.array_equal(lab.cpu().numpy(), exp["labels"]) and np.array_equal(tab[:-1].cpu().numpy(), exp["table"])
    assert np.array_equal(sm[:5], exp["summary"][:5])
    gpu.close()


def test_invalid_arguments(mods):
    """each refused argument gives MLM_ERR_INVALID and leaves the handle usable"""
    MLMap, _ = mods
    gpu = MLMap(S1, max_blocks=1024)
    L, h = gpu._L, gpu._h
    buf = np.zeros(1 << 16, dtype=np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    tab = np.zeros((4, 16), dtype=np.int64)
    tp = tab.ctypes.data_as(ctypes.c_void_p)
    sm = np.zeros(6, dtype=np.int64)
    sp = sm.ctypes.data_as(ctypes.c_void_p)

    def call(lo=(0, 0, 0), dims=(4, 4, 4), flags=UNKNOWN, conn=26, ms=1, labels=p, table=None, cap=0, summary=sp):
        lo_a, dims_a = np.array(lo, dtype=np.int32), np.array(dims, dtype=np.int32)
        return L.mlm_export_clusters(h, lo_a.ctypes.data_as(ctypes.c_void_p), dims_a.ctypes.data_as(ctypes.c_void_p), flags, conn, ms, labels, table,
                                     cap, summary)

    bad = [dict(dims=(0, 4, 4)), dict(dims=(4, -1, 4)), dict(dims=(4, 4, 0)), dict(dims=(2048, 2048, 1024)), dict(dims=(65536, 32768, 1)),
           dict(lo=(2 ** 31 - 10, 0, 0), dims=(20, 1, 1)), dict(lo=(0, 0, 2 ** 31 - 1), dims=(1, 1, 1)),
           dict(flags=0), dict(flags=8), dict(flags=FRONTIER | OCC), dict(flags=FRONTIER | 8), dict(flags=32), dict(flags=-1), dict(flags=1 << 30),
           dict(conn=0), dict(conn=4), dict(conn=8), dict(conn=27), dict(conn=-6), dict(ms=0), dict(ms=-3),
           dict(cap=-1), dict(cap=4), dict(table=tp), dict(table=tp, cap=-4), dict(labels=None, summary=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert call() == 0
        assert tuple(sm[:5]) == (64, 1, 1, 64, 64)  # (an empty map: every voxel UNKNOWN, one component)
    assert (buf[:64] == 0).all()
    assert call(flags=7, conn=6, ms=2 ** 31 - 1, labels=None, table=tp, cap=4) == 0
    assert tuple(sm[:5]) == (64, 1, 0, 0, 64) and not tab.any()
    assert call(flags=FRONTIER, conn=18, ms=65, table=tp, cap=4) == 0
    assert not sm.any() and (buf[:64] == -1).all()
    gpu.close()
