"""mlm_export_mesh: the exact indexed surface mesh of a voxel box (include/mlmap_hip.h), checked byte for byte against the numpy
ground truth (tests/mesh_ref.py): quads, faces, vertices, positions, normal sums and the summary.

The classes come from maps built voxel by voxel (import_blocks, the Crafted maps of tests/test_gpu_clusters.py) and from the CPU
oracle's getOccupancy / getInflateOccupancy at the voxel centres of the box grown by one voxel."""
import ctypes
import os

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import mesh_ref as ref
from tests.test_gpu_clusters import Crafted, blocks_over, oracle_classes
from tests.test_gpu_query_ops import config as geometry_config

pytestmark = pytest.mark.gpu

OCC, INFL, UNKNOWN, SEEN, CLOSED = ref.OCC, ref.INFL, ref.UNKNOWN, ref.SEEN, ref.CLOSED
KEYS = ("quads", "faces", "verts", "xyz", "normals")
EXTRA = [int(x) for x in os.environ.get("MLM_STRESS_SEEDS", "").split(",") if x]  # more seeds for a longer soak


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


def kw(flags):
    return dict(occ=bool(flags & OCC), infl=bool(flags & INFL), unknown=bool(flags & UNKNOWN), seen=bool(flags & SEEN), closed=bool(flags & CLOSED))


def expected(classes_of, lo, dims, flags, cfg=S1):
    occ, infl = classes_of([v - 1 for v in lo], [v + 2 for v in dims])
    return ref.mesh(occ, infl, lo, flags, cfg.subbox_n, cfg.subbox_d_xyz)


def same(got, exp, what=""):
    assert np.array_equal(got["summary"], exp["summary"]), (what, got["summary"], exp["summary"])
    for k in KEYS:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


def check(gpu, classes_of, lo, dims, flags, cfg=S1, what=""):
    exp = expected(classes_of, lo, dims, flags, cfg)
    got = gpu.export_mesh(lo, dims, **kw(flags))
    same(got, exp, f"{what} lo={lo} dims={dims} flags={flags}")
    return got


# ---- maps built voxel by voxel ------------------------------------------------------------------------------------------------
def test_single_voxel_and_empty_set(mods):
    MLMap, _ = mods
    v = [-13, 4, 27]
    m = Crafted(MLMap, [v], blocks_over(v, [1, 1, 1], 2))
    for lo, dims in (([-15, 2, 25], [5, 5, 5]), (v, [1, 1, 1])):
        for flags in (OCC, OCC | SEEN, OCC | CLOSED):
            got = check(m.gpu, m.classes, lo, dims, flags, what="single voxel")
            assert list(got["summary"][:4]) == [6, 8, 1, 1] and np.array_equal(got["faces"], [v + [a] for a in range(6)])
            assert np.array_equal(np.abs(got["normals"]), np.ones((8, 3)))
    # a box without an obstacle: F = V = 0, and nothing is written
    import torch

    lo, dims = [-12, 6, 20], [7, 3, 4]
    got = check(m.gpu, m.classes, lo, dims, OCC, what="empty")
    assert not got["summary"].any() and all(len(got[k]) == 0 for k in KEYS)
    q = torch.full((4, 4), 7, dtype=torch.int32, device="cuda")
    x = torch.full((4, 3), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    sm = m.gpu.export_mesh_dev(lo, dims, quads=q.data_ptr(), cap_faces=4, xyz=x.data_ptr(), cap_verts=4)
    assert not sm.any() and (q == 7).all() and (x == 7.0).all()
    m.gpu.close()


def test_cube_with_a_hole_and_pinches(mods):
    MLMap, _ = mods
    lo = [-12, -3, 7]  # (the cube straddles the blocks' borders at x = -10 and z = 10)
    cube = np.ones((3, 3, 3), dtype=bool)
    cube[1, 1, 1] = False
    z, y, x = np.nonzero(cube)
    m = Crafted(MLMap, np.stack([x + lo[0], y + lo[1], z + lo[2]], axis=1), blocks_over(lo, [3, 3, 3], 2))
    for flags in (OCC, OCC | CLOSED, OCC | SEEN):
        got = check(m.gpu, m.classes, [lo[0] - 1, lo[1] - 1, lo[2] - 1], [5, 5, 5], flags, what="cube with a hole")
        assert got["summary"][0] == 54 + 6 and got["summary"][1] == 64 and got["summary"][2] == 26 and got["summary"][10] == 0
        ref.check_properties(got, flags)
    got = check(m.gpu, m.classes, lo, [3, 3, 3], OCC | CLOSED, what="the cube's own box")
    assert got["summary"][10] == 54
    m.gpu.close()
    # two voxels that touch at an edge, two that touch at a corner: shared vertices, a normal sum that cancels at the pinch
    a = np.array([3, -8, 9])
    m = Crafted(MLMap, [a, a + [1, 1, 0], a + [5, 0, 0], a + [6, 1, 1]], blocks_over([0, -10, 5], [12, 5, 8], 2))
    got = check(m.gpu, m.classes, [1, -10, 7], [11, 5, 5], OCC, what="pinches")
    assert got["summary"][0] == 24 and got["summary"][1] == 14 + 15
    edge = [i for i, k in enumerate(got["verts"].tolist()) if k[:2] == [4, -7]]
    corner = [i for i, k in enumerate(got["verts"].tolist()) if k == [9, -7, 10]]
    assert len(edge) == 2 and not got["normals"][edge][:, :2].any() and len(corner) == 1 and not got["normals"][corner].any()
    assert np.array_equal(ref.vertex_normals_from_faces(got), got["normals"])
    ref.check_properties(got, OCC)
    m.gpu.close()


def test_obstacles_on_the_six_sides_of_the_box(mods):
    """an obstacle on each side of the box, the neighbour outside the box in turn an obstacle, FREE, and in an absent block"""
    MLMap, _ = mods
    n = S1.subbox_n
    lo, dims = [0, 0, 0], [n, n, n]  # (the block 0 0 0)
    h = n // 2
    inner = np.array([[0, h, h], [n - 1, h, h], [h, 0, h], [h, n - 1, h], [h, h, 0], [h, h, n - 1]])
    outer = np.array([[-1, h, h], [n, h, h], [h, -1, h], [h, n, h], [h, h, -1], [h, h, n]])
    around = blocks_over(lo, dims, 1)
    rim = {}  # summary[10] by (neighbour, flags)
    for name, m in (("obstacle", Crafted(MLMap, np.concatenate([inner, outer]), around)), ("free", Crafted(MLMap, inner, around)),
                    ("absent", Crafted(MLMap, inner, [[0, 0, 0]]))):
        for flags in (OCC, OCC | SEEN, OCC | CLOSED, OCC | SEEN | CLOSED):
            got = check(m.gpu, m.classes, lo, dims, flags, what=f"six sides, neighbour {name}")
            assert got["summary"][2] == 6
            rim[name, flags] = int(got["summary"][10])
        m.gpu.close()
    for flags in (OCC, OCC | SEEN):
        assert rim["obstacle", flags] == 0 and rim["obstacle", flags | CLOSED] == 6 and rim["free", flags] == 6 and rim["free", flags | CLOSED] == 6
    assert rim["absent", OCC] == 6 and rim["absent", OCC | SEEN] == 0 and rim["absent", OCC | SEEN | CLOSED] == 6


def test_straddling_box_and_the_edges_of_the_index_range(mods):
    MLMap, _ = mods
    rng = np.random.default_rng(5)
    lo, dims = [-41, -3, -2], [67, 5, 7]  # negative origin, no multiple of the block edge; two chunks of 2048, x no multiple of 64
    blocks = blocks_over(lo, dims, 1)
    blocks = blocks[rng.random(len(blocks)) < 0.8]  # (some blocks absent)
    occupied = np.concatenate([b * S1.subbox_n + rng.integers(0, S1.subbox_n, size=(150, 3)) for b in blocks])
    m = Crafted(MLMap, occupied, blocks)
    for flags in (OCC, UNKNOWN, OCC | UNKNOWN, OCC | SEEN, OCC | UNKNOWN | CLOSED, UNKNOWN | SEEN | CLOSED):
        got = check(m.gpu, m.classes, lo, dims, flags, what="straddling")
        assert got["summary"][0] > (200 if flags & OCC else 0)
        ref.check_properties(got, flags)
    m.gpu.close()
    # the last block of the key range: voxels beyond it are UNKNOWN, inside or outside the box
    n = S1.subbox_n
    last = (1 << 20) - 1
    m = Crafted(MLMap, [[last * n + n - 1, 3, 4], [last * n + n - 2, 3, 5]], [[last, 0, 0]])
    for lo, dims in (([last * n + n - 5, 1, 2], [9, 5, 5]), ([last * n + n - 5, 1, 2], [5, 5, 5])):
        for flags in (OCC, UNKNOWN, OCC | UNKNOWN, OCC | SEEN, OCC | CLOSED):
            got = check(m.gpu, m.classes, lo, dims, flags, what="key range")
            assert got["summary"][0] > 0 or not flags & OCC
    m.gpu.close()
    # the edge of int32: the neighbours' indices leave it
    m = Crafted(MLMap, np.zeros((0, 3)), [[0, 0, 0]])
    for elo, ed in [([2 ** 31 - 11, -2 ** 31, 0], [10, 3, 2]), ([-2 ** 31, 2 ** 31 - 4, -2 ** 31], [2, 3, 4])]:
        got = check(m.gpu, m.classes, elo, ed, UNKNOWN, what="int32 edge")
        assert got["summary"][0] == 0 and got["summary"][2] == ed[0] * ed[1] * ed[2]  # (UNKNOWN all around: no open voxel)
        got = check(m.gpu, m.classes, elo, ed, UNKNOWN | CLOSED, what="int32 edge, closed")
        assert got["summary"][0] == 2 * (ed[0] * ed[1] + ed[0] * ed[2] + ed[1] * ed[2])
        ref.check_properties(got, UNKNOWN | CLOSED)
        assert not check(m.gpu, m.classes, elo, ed, OCC, what="int32 edge, no obstacle")["summary"].any()
    m.gpu.close()


# ---- real maps ----------------------------------------------------------------------------------------------------------------
def mapped(MLMap, OracleMap, cfg, frames=4):
    gpu, cpu = MLMap(cfg, max_blocks=16384), OracleMap(cfg)
    t = None
    for img, (q, t) in syn.stream(cfg, "room_jitter", "smooth", frames):
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
    d = cfg.subbox_d_xyz
    for m in (gpu, cpu):
        m.setFree_map_in_bound(np.asarray(t) - 3 * d, np.asarray(t) + 3 * d)
        m.inflate_map(t)
    # a box round an inflated voxel (an OCCUPIED one where nothing was inflated) from the middle of the list
    b = cpu.export_blocks()
    n = cfg.subbox_n
    blk, cell = np.nonzero(b["infl"] == ord("o"))
    if len(blk) == 0:
        blk, cell = np.nonzero(b["occ"] == ord("o"))
    pick = len(blk) // 2
    c = cell[pick]
    centre = b["keys"][blk[pick]].astype(np.int64) * n + [c % n, c // n % n, c // (n * n)]
    return gpu, cpu, [int(v) for v in centre]


@pytest.fixture(scope="module")
def s1_scene(mods):
    gpu, cpu, centre = mapped(*mods, S1)
    yield gpu, cpu, centre
    gpu.close()


@pytest.fixture(scope="module")
def s1_host(s1_scene):
    """the mesh of the scene's box into host memory, OCC | INFL"""
    gpu, cpu, c = s1_scene
    lo, dims = [c[0] - 20, c[1] - 19, c[2] - 9], [41, 39, 19]
    got = check(gpu, lambda l, d: oracle_classes(cpu, S1, l, d), lo, dims, OCC | INFL, what="scene")
    return lo, dims, got


@pytest.mark.parametrize("flags", [OCC, OCC | SEEN])
def test_mapped_scene_against_oracle(s1_scene, s1_host, flags):
    gpu, cpu, _ = s1_scene
    lo, dims, both = s1_host
    got = check(gpu, lambda l, d: oracle_classes(cpu, S1, l, d), lo, dims, flags, what="scene")
    print(f"flags={flags} box {lo} {dims}: summary {got['summary']}; OCC | INFL {both['summary']}")
    assert got["summary"][0] > 100 and both["summary"][2] > got["summary"][2] > 20  # (neither empty nor trivial; inflation adds obstacles)
    assert np.array_equal(ref.vertex_normals_from_faces(got), got["normals"])


def test_block_of_fewer_cells_than_a_wave(mods):
    MLMap, OracleMap = mods
    cfg = geometry_config(3, 0.15, False)
    gpu, cpu, c = mapped(MLMap, OracleMap, cfg)
    lo, dims = [c[0] - 16, c[1] - 15, c[2] - 8], [33, 31, 17]
    for flags in (OCC | INFL, OCC | UNKNOWN | SEEN):
        got = check(gpu, lambda l, d: oracle_classes(cpu, cfg, l, d), lo, dims, flags, cfg, what="subbox_n 3")
        assert got["summary"][0] > 50
    gpu.close()


def test_closed_mesh_properties_on_the_gpu_output(s1_scene, s1_host):
    """the normal of every quad, the enclosed volume and the even edge use, on what the GPU wrote: no reference involved"""
    gpu, _, _ = s1_scene
    lo, dims, _ = s1_host
    for flags in (OCC | CLOSED, OCC | INFL | UNKNOWN | CLOSED):
        got = gpu.export_mesh(lo, dims, **kw(flags))
        assert got["summary"][0] > 100 and len(got["quads"]) == got["summary"][0] and len(got["verts"]) == got["summary"][1]
        assert np.array_equal(ref.quad_normals(got), ref.face_normals(got))
        assert ref.enclosed_voxels(got) == got["summary"][2] and ref.odd_edges(got) == 0
        assert got["summary"][4:10].sum() == got["summary"][0] and got["summary"][3] <= got["summary"][2]


def test_destinations_caps_and_sizing(s1_scene, s1_host):
    """host and device destinations give the same bytes; caps below F / V leave the rows beyond untouched; a summary alone sizes"""
    import torch

    gpu, _, _ = s1_scene
    lo, dims, host = s1_host
    F, V = int(host["summary"][0]), int(host["summary"][1])
    flags = kw(OCC | INFL)
    assert np.array_equal(gpu.export_mesh_dev(lo, dims, **flags), host["summary"])  # sizing: no array at all
    without = gpu.export_mesh(lo, dims, normals=False, **flags)
    assert "normals" not in without and all(without[k].tobytes() == host[k].tobytes() for k in KEYS[:4])

    def buffers(rows_f, rows_v):
        t = {"quads": torch.full((rows_f, 4), 7, dtype=torch.int32, device="cuda"), "faces": torch.full((rows_f, 4), 7, dtype=torch.int32, device="cuda"),
             "verts": torch.full((rows_v, 3), 7, dtype=torch.int32, device="cuda"), "xyz": torch.full((rows_v, 3), 7.0, dtype=torch.float32, device="cuda"),
             "normals": torch.full((rows_v, 3), 7, dtype=torch.int8, device="cuda")}
        torch.cuda.synchronize()
        return t

    for cap_f, cap_v in ((F + 3, V + 3), (F, V), (F - 1, V - 1), (5, V + 3), (F + 3, 64), (1, 1)):
        t = buffers(F + 3, V + 3)
        sm = gpu.export_mesh_dev(lo, dims, quads=t["quads"].data_ptr(), faces=t["faces"].data_ptr(), cap_faces=cap_f, verts=t["verts"].data_ptr(),
                                 xyz=t["xyz"].data_ptr(), normals=t["normals"].data_ptr(), cap_verts=cap_v, **flags)
        assert np.array_equal(sm, host["summary"]), (cap_f, cap_v)
        for k in KEYS:
            rows = min(F, cap_f) if k in ("quads", "faces") else min(V, cap_v)
            g = t[k].cpu().numpy()
            assert g[:rows].tobytes() == host[k][:rows].tobytes(), (k, cap_f, cap_v)
            assert (g[rows:] == 7).all(), (k, cap_f, cap_v, "rows beyond the cap were written")
    # each group alone, and single arrays; quads carry the true vertex numbers without any vertex array
    t = buffers(F, V)
    assert gpu.export_mesh_dev(lo, dims, quads=t["quads"].data_ptr(), cap_faces=F, summary=False, **flags) is None
    assert np.array_equal(t["quads"].cpu().numpy(), host["quads"]) and (t["faces"] == 7).all() and (t["verts"] == 7).all()
    gpu.export_mesh_dev(lo, dims, normals=t["normals"].data_ptr(), xyz=t["xyz"].data_ptr(), cap_verts=V, **flags)
    assert np.array_equal(t["normals"].cpu().numpy(), host["normals"]) and t["xyz"].cpu().numpy().tobytes() == host["xyz"].tobytes()
    # host arrays through the C interface with caps below F / V
    q = np.full((F, 4), 7, dtype=np.int32)
    v3 = np.full((V, 3), 7, dtype=np.int32)
    sm = np.zeros(12, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lo_a, dims_a = np.array(lo, dtype=np.int32), np.array(dims, dtype=np.int32)
    assert gpu._L.mlm_export_mesh(gpu._h, p(lo_a), p(dims_a), OCC | INFL, p(q), None, F - 2, p(v3), None, None, 3, p(sm)) == 0
    assert np.array_equal(sm, host["summary"]) and np.array_equal(q[:F - 2], host["quads"][:F - 2]) and (q[F - 2:] == 7).all()
    assert np.array_equal(v3[:3], host["verts"][:3]) and (v3[3:] == 7).all()


def test_staged_ranges_and_scratch(mods, s1_scene, s1_host, knobs):
    """host destinations staged in ranges of 100 and of 1 row give the bytes of one range; the scratch grows at the first call and
    stays"""
    MLMap, _ = mods
    gpu, _, _ = s1_scene
    lo, dims, host = s1_host
    assert host["summary"][0] > 300 and host["summary"][1] > 300
    for rows in (100, 1 << 20, 257):
        knobs.set("mesh_stage_rows", rows)
        same(gpu.export_mesh(lo, dims, **kw(OCC | INFL)), host, f"ranges of {rows} rows")
    small_lo, small = [lo[0] + 15, lo[1] + 15, lo[2] + 5], [9, 9, 9]
    one = gpu.export_mesh(small_lo, small, **kw(OCC | INFL))
    knobs.set("mesh_stage_rows", 1)
    same(gpu.export_mesh(small_lo, small, **kw(OCC | INFL)), one, "ranges of one row")
    fresh = MLMap(S1, max_blocks=64)
    before = fresh.frame_stats()["device_bytes"]
    box = [128, 128, 128]  # an empty map: every voxel UNKNOWN; CLOSED: the six sides of the box
    sm = fresh.export_mesh_dev([0, 0, 0], box, occ=False, unknown=True, closed=True)
    side = 128 * 128
    assert list(sm) == [6 * side, 6 * side + 2, 128 ** 3, 6 * side - 12 * 128 + 8] + [side] * 6 + [6 * side, 0]
    grown = fresh.frame_stats()["device_bytes"]
    assert grown - before >= 128 ** 3 + 130 ** 3 + 129 ** 3 * 3 // 16
    fresh.export_mesh_dev([0, 0, 0], box, occ=False, unknown=True, closed=True)
    assert fresh.frame_stats()["device_bytes"] == grown
    fresh.close()


def test_async_mode_and_the_callers_stream(mods):
    """async mode: the call sees every submitted frame; on the caller's stream the rows land behind the work queued there"""
    import torch

    MLMap, _ = mods
    nf = 8
    frames = np.stack([img for img, _ in syn.stream(S1, "room_jitter", "smooth", nf)])
    poses = syn.smooth_trajectory(nf, 42)
    q, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    synced = MLMap(S1, max_blocks=8192, max_batch=4)
    synced.update_map_batch(frames, q, t)
    synced.sync()
    v = [int(np.floor(x / S1.subbox_d_xyz)) for x in t[-1]]
    lo, dims = [v[0] - 30, v[1] - 30, v[2] - 10], [61, 63, 21]
    w = synced.export_window([c - 1 for c in lo], [c + 2 for c in dims], odds=False, occ=True, infl=True)
    exp = ref.mesh(w["occ"], w["infl"], lo, OCC | UNKNOWN, S1.subbox_n, S1.subbox_d_xyz)
    assert exp["summary"][0] > 500
    same(synced.export_mesh(lo, dims, **kw(OCC | UNKNOWN)), exp, "synced")
    synced.close()

    gpu = MLMap(S1, max_blocks=8192, max_batch=4)
    gpu.set_async(True)
    gpu.update_map_batch(frames, q, t)  # no sync()
    same(gpu.export_mesh(lo, dims, **kw(OCC | UNKNOWN)), exp, "async")
    F, V = int(exp["summary"][0]), int(exp["summary"][1])
    s = torch.cuda.Stream()
    gpu.set_stream(s.cuda_stream)
    quads = torch.empty((F, 4), dtype=torch.int32, device="cuda")
    xyz = torch.empty((V, 3), dtype=torch.float32, device="cuda")
    junk = torch.ones(1 << 26, device="cuda")
    with torch.cuda.stream(s):
        for _ in range(50):  # (keeps the caller's stream busy: the rows are written behind this work)
            junk.mul_(1.0001)
        quads.fill_(7)
        xyz.fill_(7.0)
    sm = gpu.export_mesh_dev(lo, dims, quads=quads.data_ptr(), cap_faces=F, xyz=xyz.data_ptr(), cap_verts=V, **kw(OCC | UNKNOWN))
    assert np.array_equal(sm, exp["summary"])
    assert np.array_equal(quads.cpu().numpy(), exp["quads"]) and xyz.cpu().numpy().tobytes() == exp["xyz"].tobytes()
    gpu.close()


def test_invalid_arguments(mods):
    """each refused argument gives MLM_ERR_INVALID and leaves the handle usable"""
    MLMap, _ = mods
    gpu = MLMap(S1, max_blocks=64)
    L, h = gpu._L, gpu._h
    q = np.zeros((512, 4), dtype=np.int32)
    v = np.zeros((512, 3), dtype=np.int32)
    sm = np.zeros(12, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def call(lo=(0, 0, 0), dims=(4, 4, 4), flags=UNKNOWN | CLOSED, quads=p(q), face4=None, cap_f=512, vert3=p(v), xyz=None, n3=None, cap_v=512,
             summary=p(sm)):
        lo_a, dims_a = np.array(lo, dtype=np.int32), np.array(dims, dtype=np.int32)
        return L.mlm_export_mesh(h, p(lo_a), p(dims_a), flags, quads, face4, cap_f, vert3, xyz, n3, cap_v, summary)

    bad = [dict(dims=(0, 4, 4)), dict(dims=(4, -1, 4)), dict(dims=(4, 4, 0)), dict(dims=(2048, 2048, 1024)), dict(dims=(65536, 32768, 1)),
           dict(lo=(2 ** 31 - 10, 0, 0), dims=(20, 1, 1)), dict(lo=(0, 0, 2 ** 31 - 1), dims=(1, 1, 1)),
           dict(dims=(2 ** 30, 1, 1)), dict(dims=(1290, 1290, 1290)),  # more than 2^31 - 1 lattice points, the voxels fit
           dict(flags=0), dict(flags=SEEN), dict(flags=CLOSED | SEEN), dict(flags=OCC | 8), dict(flags=OCC | 64), dict(flags=-1), dict(flags=OCC | 1 << 30),
           dict(cap_f=-1), dict(cap_v=-1), dict(cap_f=0), dict(cap_v=0), dict(quads=None), dict(vert3=None), dict(quads=None, cap_f=-3),
           dict(quads=None, cap_f=0, vert3=None, cap_v=0, summary=None)]
    for kwargs in bad:
        sm[:] = -5
        assert call(**kwargs) == -1, kwargs
        assert (sm == -5).all() and not q.any() and not v.any(), kwargs
        assert call() == 0
        assert list(sm[:4]) == [96, 98, 64, 56] and q[:96].any()  # (an empty map: the closed 4 x 4 x 4 box of UNKNOWN voxels)
        q[:] = 0
        v[:] = 0
    assert call(quads=None, cap_f=0, vert3=None, cap_v=0) == 0 and list(sm[:2]) == [96, 98]
    assert call(quads=None, face4=p(q), summary=None) == 0 and (q[:96, 3] < 6).all()
    gpu.close()


# ---- random sequences ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3] + EXTRA)
def test_random_sequence(mods, seed):
    """integrate, setFree_map_in_bound and inflate_map mixed with export_mesh at random flags and boxes, each checked against the
    oracle's classes of that moment"""
    MLMap, OracleMap = mods
    rng = np.random.default_rng(seed)
    n, d = [(3, 0.15), (7, 0.05), (10, 0.1), (16, 0.15)][seed % 4]
    cfg = geometry_config(n, d, bool(seed & 1))
    gpu, cpu = MLMap(cfg, max_blocks=16384), OracleMap(cfg)
    frames = syn.stream(cfg, "room_jitter", "smooth", 12)
    t = np.zeros(3)
    meshes = faces = 0
    for step in range(14):
        op = "frame" if step < 2 else rng.choice(["frame", "free", "inflate", "mesh", "mesh"])
        if op == "frame":
            img, (q, t) = next(frames)
            gpu.update_map(img, q, t)
            cpu.update_depth(img, q, t)
            continue
        if op == "free":
            c = np.asarray(t) + rng.uniform(-1.0, 1.0, 3)
            for m in (gpu, cpu):
                m.setFree_map_in_bound(c - 4 * d, c + 4 * d)
            continue
        if op == "inflate":
            for m in (gpu, cpu):
                m.inflate_map(t)
            continue
        b = cpu.export_blocks()
        blk, cell = np.nonzero(b["occ"] == ord("o"))
        pick = int(rng.integers(0, len(blk)))
        c = int(cell[pick])
        centre = b["keys"][blk[pick]].astype(np.int64) * n + [c % n, c // n % n, c // (n * n)]
        dims = [int(v) for v in rng.integers(1, 23, 3)]
        lo = [int(centre[a] - rng.integers(0, dims[a])) for a in range(3)]
        flags = int(rng.integers(1, 8)) | (SEEN if rng.random() < 0.4 else 0) | (CLOSED if rng.random() < 0.4 else 0)
        got = check(gpu, lambda l, s: oracle_classes(cpu, cfg, l, s), lo, dims, flags, cfg, what=f"seed {seed} step {step}")
        ref.check_properties(got, flags)
        meshes += 1
        faces += int(got["summary"][0])
    assert meshes >= 3 and faces > 0, (meshes, faces)
    gpu.close()
