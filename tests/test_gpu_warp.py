"""mlm_warp_blocks on the GPU: crafted maps of every block geometry under the identity, a whole-voxel shift, a yaw and a general rigid
transform, into host and into device memory, with every output left out in turn, byte for byte against the contract in numpy
(tests/warp_ref.py); atomicity of the failing calls; MLM_WARP_REPLACE against its definition (warp into device buffers, crop everything,
import) with integration on both sides of it; frontier mode; an integrated corridor map; reanchor there and back."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import warp_ref as ref

pytestmark = pytest.mark.gpu
PLANES = ("keys", "log_odds", "occ", "infl")
WHOLE = ([ref.KEY_MIN] * 3, [1 << 21] * 3)
GENERAL = ref.make_T(ref.rot(30.0, 7.0, -3.0), (0.23, -0.41, 0.17))
TRANSFORMS = {"identity": ref.make_T(), "shift": ref.make_T(None, (0.3, -0.7, 1.1)), "yaw30": ref.make_T(ref.rot(30.0)), "general": GENERAL}


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap, MlmError, invert_T

    return MLMap, MlmError, invert_T


def small_cfg(n, explore=False):
    return S1.with_(subbox_n=n, subbox_d_xyz=0.1, use_exploration_frontiers=explore, width=320, height=240, cam_cx=160.0, cam_cy=120.0,
                    cam_fx=192.5, cam_fy=192.5)


def same(a, b, what):
    for k in PLANES:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {k}"


def same_counts(got, want, what):
    """summary [0], [2] .. [7]; [1] is an implementation count >= [2]"""
    g, w = np.asarray(got), np.asarray(want)
    assert g[0] == w[0] and g[2:].tolist() == w[2:].tolist() and g[1] >= g[2], (what, g.tolist(), w.tolist())


def craft(rng, n, count, explore=False):
    """count blocks of a cube of keys around zero: distinct log-odds, random classes, a few blocks nothing has seen"""
    C = n ** 3
    side = max(2, int(np.ceil((2.5 * count) ** (1 / 3))))
    flat = rng.choice(side ** 3, count, replace=False)
    keys = (np.stack([flat % side, (flat // side) % side, flat // (side * side)], axis=1) - side // 2)[rng.permutation(count)].astype(np.int32)
    lo = (np.float32(-2.0) + rng.permutation(count * C).astype(np.float32) * np.float32(6.0 / (count * C))).reshape(count, C)
    b = {"keys": keys.reshape(count, 3), "log_odds": lo, "occ": rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(count, C)),
         "infl": rng.choice(np.frombuffer(b"uo", dtype=np.uint8), size=(count, C)),
         "collapsed": (rng.random(count) < 0.2).astype(np.uint8) if explore else np.zeros(count, dtype=np.uint8)}
    blank = rng.random(count) < 0.15
    b["occ"][blank] = ref.U
    b["infl"][blank] = ref.U
    return b


def load(m, b):
    if len(b["keys"]):
        m.import_blocks(b["keys"], b["log_odds"], b["occ"], b["infl"], b["collapsed"] if b["collapsed"].any() else None)


def empty(m):
    m.crop_blocks(*WHOLE, inside=True)
    assert m.block_count() == 0


def raw_call(gpu, T, lo, dims, flags, cap, outs):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    T_a = None if T is None else np.ascontiguousarray(T, dtype=np.float64)
    lo_a = None if lo is None else np.asarray(lo, dtype=np.int32)
    dims_a = None if dims is None else np.asarray(dims, dtype=np.int32)
    sm = np.full(ref.ROW, -9, dtype=np.int64)
    rc = gpu._L.mlm_warp_blocks(gpu._h, p(T_a), p(lo_a), p(dims_a), flags, cap, *[None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in outs],
                                sm.ctypes.data_as(ctypes.c_void_p))
    return rc, sm, gpu._L.mlm_last_error(gpu._h).decode()


def out_arrays(cap, C):
    return [np.full((cap, 3), 7, dtype=np.int32), np.full((cap, C), 7, dtype=np.float32), np.full((cap, C), 7, dtype=np.uint8),
            np.full((cap, C), 7, dtype=np.uint8)]


def device_call(gpu, T, E, C, skip=None, **kw):
    """the call into torch device tensors with one row to spare (which must stay as it was); skip: the output left out"""
    import torch

    dev = {"keys": torch.full((E + 1, 3), 7, dtype=torch.int32, device="cuda"), "log_odds": torch.full((E + 1, C), 7, dtype=torch.float32, device="cuda"),
           "occ": torch.full((E + 1, C), 7, dtype=torch.uint8, device="cuda"), "infl": torch.full((E + 1, C), 7, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    res = gpu.warp_blocks(T, out={"cap": E + 1, **{k: v.data_ptr() for k, v in dev.items() if k != skip}}, **kw)
    got = {k: v.cpu().numpy() for k, v in dev.items()}
    assert all(np.all(v[E:] == 7) for v in got.values())
    return res, {k: v[:E] for k, v in got.items()}, dev


COUNTS = {2: [1, 65, 300], 3: [1, 65, 300], 4: [1, 65, 300], 7: [1, 65, 300], 8: [1, 65, 300], 16: [1, 65, 300]}


@pytest.mark.parametrize("n", [2, 3, 4, 7, 8, 16])
def test_crafted_maps(mods, knobs, n):
    """one handle per geometry; every case empties it and loads the next crafted map.  Host outputs are staged in rounds of 50 blocks."""
    MLMap, _, _ = mods
    knobs.set("crop_stage_rows", 50)
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(2000 + n)
    C = n ** 3
    for count in COUNTS[n]:
        empty(gpu)
        src = craft(rng, n, count)
        load(gpu, src)
        before = gpu.export_blocks(raw=True)
        names = list(TRANSFORMS) if (n < 16 or count < 300) else ["general"]  # (the numpy rule over 300 blocks of 4096 cells takes seconds per transform)
        for name in names:
            T = TRANSFORMS[name]
            what = f"n {n} count {count} {name}"
            want = ref.warp(src, T, n, 0.1)
            E = len(want["keys"])
            assert E >= count * (name == "identity")
            # dry, then host arrays
            dry = gpu.warp_blocks(T, dry=True)
            same_counts(dry["summary"], np.where(np.arange(8) == 3, 0, want["summary"]), what + " dry")
            res = gpu.warp_blocks(T, out=True)
            same(res, want, what + " host")
            same_counts(res["summary"], want["summary"], what + " host")
            # device tensors, and every output left out in turn
            res, got, _ = device_call(gpu, T, E, C)
            same(got, want, what + " device")
            same_counts(res["summary"], want["summary"], what + " device")
            if count == 65:
                for skip in PLANES:
                    outs = out_arrays(E, C)
                    outs[PLANES.index(skip)] = None
                    rc, sm, err = raw_call(gpu, T, None, None, 0, E, outs)
                    assert rc == ref.OK, err
                    for k, a in zip(PLANES, outs):
                        assert a is None or a.tobytes() == want[k].tobytes(), f"{what} host without {skip}: {k}"
                    same_counts(sm, want["summary"], what + " without " + skip)
                    _, got, _ = device_call(gpu, T, E, C, skip=skip)
                    assert np.all(got[skip] == 7)
                    assert all(got[k].tobytes() == want[k].tobytes() for k in PLANES if k != skip), f"{what} device without {skip}"
                # MLM_WARP_SEEN and a key box
                seen = ref.warp(src, T, n, 0.1, seen=True)
                res = gpu.warp_blocks(T, seen=True, out=True)
                same(res, seen, what + " seen")
                same_counts(res["summary"], seen["summary"], what + " seen")
                lo, dims = [0, -50, -1], [2, 100, 3]
                boxed = ref.warp(src, T, n, 0.1, lo, dims)
                res = gpu.warp_blocks(T, lo, dims, out=True)
                same(res, boxed, what + " box")
                same_counts(res["summary"], boxed["summary"], what + " box")
        after = gpu.export_blocks(raw=True)
        assert all(after[k].tobytes() == before[k].tobytes() for k in before), "a call without MLM_WARP_REPLACE changed the map"
    gpu.close()


def test_failing_calls_leave_the_map_alone(mods):
    MLMap, MlmError, _ = mods
    n, C = 4, 64
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(4)
    src = craft(rng, n, 120)
    load(gpu, src)
    before = gpu.export_blocks(raw=True)
    want = ref.warp(src, GENERAL, n, 0.1)
    E = len(want["keys"])
    exp = want["summary"].copy()
    exp[3] = 0
    for flags in (0, ref.REPLACE, ref.SEEN | ref.REPLACE):
        w = ref.warp(src, GENERAL, n, 0.1, seen=bool(flags & ref.SEEN))
        e = w["summary"].copy()
        e[3] = 0
        for cap, outs in ((len(w["keys"]) - 1, out_arrays(len(w["keys"]) - 1, C)), (0, out_arrays(1, C)), (3, [None, None, np.full((3, C), 7, np.uint8), None])):
            rc, sm, err = raw_call(gpu, GENERAL, None, None, flags, cap, outs)
            assert rc == ref.ERR_CAPACITY and "emitted" in err, (rc, err)
            same_counts(sm, e, f"capacity, flags {flags}")
            assert all(a is None or np.all(a == 7) for a in outs), "an output was written"
            assert all(gpu.export_blocks(raw=True)[k].tobytes() == before[k].tobytes() for k in before)
    sheared = ref.make_T([[1, 1e-3, 0], [0, 1, 0], [0, 0, 1]])
    cases = [(None, None, None, 0, 0), (ref.make_T(None, (np.nan, 0, 0)), None, None, 0, 0), (ref.make_T(None, (0, 0, -np.inf)), None, None, ref.REPLACE, 0),
             (ref.make_T(np.eye(3) * 1.001), None, None, ref.REPLACE, 0), (sheared, None, None, 0, 0), (GENERAL, [0, 0, 0], None, 0, 0),
             (GENERAL, None, [1, 1, 1], ref.REPLACE, 0), (GENERAL, [0, 0, 0], [1, 0, 1], 0, 0), (GENERAL, [ref.I32_MAX, 0, 0], [1, 1, 1], ref.REPLACE, 0),
             (GENERAL, None, None, 8, 0), (GENERAL, None, None, -1, 0), (GENERAL, None, None, ref.REPLACE | 32, 0), (GENERAL, None, None, ref.REPLACE, -1)]
    for T, lo, dims, flags, cap in cases:
        outs = out_arrays(E, C)
        rc, sm, err = raw_call(gpu, T, lo, dims, flags, cap, outs)
        assert rc == ref.ERR_INVALID and err.startswith("mlm_warp_blocks: ") and len(err) > 25, (flags, cap, rc, err)
        assert ref.check_args(T, lo, dims, flags, cap) != 0
        assert np.all(sm == -9) and all(np.all(a == 7) for a in outs)
        assert all(gpu.export_blocks(raw=True)[k].tobytes() == before[k].tobytes() for k in before), "map after an invalid call"
    with pytest.raises(MlmError):
        gpu.warp_blocks(sheared, replace=True)
    res = gpu.warp_blocks(GENERAL, out=True)  # the handle stays usable
    same(res, want, "after the failing calls")
    gpu.close()


def classes_at(dump, n, pos, d=0.1):
    """getOccupancy's answer (FREE 1, OCCUPIED 0, UNKNOWN -1) from a dump, at positions"""
    v = np.floor(pos / d).astype(np.int64)
    g = v // n
    c = v - g * n
    row = {tuple(k): i for i, k in enumerate(dump["keys"].tolist())}
    r = np.array([row.get(tuple(k), -1) for k in g.tolist()])
    occ = np.where(r >= 0, dump["occ"][np.maximum(r, 0), (c[:, 2] * n + c[:, 1]) * n + c[:, 0]], ref.U)
    return np.where(occ == ref.O, 0, np.where(occ == ref.F, 1, -1)).astype(np.int8)


@pytest.mark.parametrize("n,count,mirror", [(3, 300, False), (8, 65, True), (16, 20, False)])
def test_replace_is_the_dump_imported(mods, knobs, n, count, mirror):
    """300 blocks into a pool of 64: the emitted blocks outgrow the pool before the first write"""
    MLMap, _, _ = mods
    if mirror:
        knobs.set("mirror_max", 1 << 20)
    else:
        knobs.set("mirror", 0)
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(70 + n)
    src = craft(rng, n, count)
    load(gpu, src)
    for name in ("general", "shift"):
        T = TRANSFORMS[name]
        cur = gpu.export_blocks()
        pos0 = (cur["keys"][:40].astype(np.float64) * n + rng.integers(0, n, (min(40, len(cur["keys"])), 3)) + 0.5) * 0.1
        gpu.getOccupancy(pos0[:1]), gpu.getOccupancy(pos0)  # (a mirror that knows the map as it was)
        dump = gpu.warp_blocks(T, out=True)
        same(dump, ref.warp(cur, T, n, 0.1), f"{name}: dump")
        res = gpu.warp_blocks(T, replace=True)
        same_counts(res["summary"], np.where(np.arange(8) == 3, 0, dump["summary"]), name)
        after = gpu.export_blocks()
        same(after, dump, f"{name}: export after MLM_WARP_REPLACE")
        assert not after["collapsed"].any() and gpu.block_count() == len(dump["keys"]) == gpu.frame_stats()["n_blocks"]
        pick = rng.integers(0, len(dump["keys"]), 300)
        keys = dump["keys"][pick].astype(np.int64) + (rng.random((300, 3)) < 0.2) * rng.integers(-1, 2, (300, 3))
        pos = (keys * n + rng.integers(0, n, (300, 3)) + 0.5) * 0.1
        assert np.array_equal(gpu.getOccupancy(pos[:1]), classes_at(dump, n, pos[:1]))
        assert np.array_equal(gpu.getOccupancy(pos), classes_at(dump, n, pos)), f"{name}: getOccupancy at destination centres"
        assert np.array_equal(gpu.getOccupancy(pos0), classes_at(dump, n, pos0))
    gpu.close()


def test_replace_equals_warp_crop_import_with_integration(mods):
    """handle A: frames, MLM_WARP_REPLACE, a frame; handle B: the same frames, the call into device buffers, a crop of everything,
    import_blocks, the same frame — identical sorted exports, float bits included"""
    MLMap, _, _ = mods
    cfg = small_cfg(8)
    frames = list(syn.stream(cfg, "room_jitter", "smooth", 5))
    a, b = MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64)
    for m in (a, b):
        for img, (q, t) in frames[:4]:
            m.update_map(img, q, t)
    T = ref.make_T(ref.rot(1.0), (0.1, -0.2, 0.0))  # a correction as match_pose finds it: a degree and a voxel or two
    ra = a.warp_blocks(T, replace=True)
    E, C = int(ra["summary"][2]), cfg.cells_per_block
    assert E > 20 and ra["summary"][0] == b.block_count()
    rb, _, dev = device_call(b, T, E, C)
    same_counts(rb["summary"], np.where(np.arange(8) == 3, E, ra["summary"]), "both handles")
    empty(b)
    b.import_blocks((dev["keys"].data_ptr(), E), dev["log_odds"].data_ptr(), dev["occ"].data_ptr(), dev["infl"].data_ptr())
    same(a.export_blocks(), b.export_blocks(), "right after")
    g0 = a.frame_stats()["n_graph_launches"]
    for m in (a, b):
        img, (q, t) = frames[4]
        m.update_map(img, q, t)
    ea, eb = a.export_blocks(), b.export_blocks()
    same(ea, eb, "one frame later")
    assert len(ea["keys"]) >= E and a.frame_stats()["n_graph_launches"] > g0, "the graphs did not survive the call"
    a.close(), b.close()


def test_frontier_mode(mods):
    MLMap, MlmError, _ = mods
    n = 5
    gpu = MLMap(small_cfg(n, True), max_blocks=64)
    rng = np.random.default_rng(9)
    src = craft(rng, n, 150, explore=True)
    assert src["collapsed"].sum() > 10
    load(gpu, src)
    before = gpu.export_blocks(raw=True)
    for flags in (ref.REPLACE, ref.REPLACE | ref.DRY, ref.REPLACE | ref.SEEN):
        rc, sm, err = raw_call(gpu, GENERAL, None, None, flags, 0, [None] * 4)
        assert rc == ref.ERR_INVALID and "frontier" in err and np.all(sm == -9), (rc, err)
    with pytest.raises(MlmError):
        gpu.reanchor(GENERAL)
    assert all(gpu.export_blocks(raw=True)[k].tobytes() == before[k].tobytes() for k in before)
    for name, T in TRANSFORMS.items():
        for seen in (False, True):
            want = ref.warp(src, T, n, 0.1, seen=seen)
            res = gpu.warp_blocks(T, seen=seen, out=True)
            same(res, want, f"frontier mode, {name}, seen {seen}")
            same_counts(res["summary"], want["summary"], name)
    assert all(gpu.export_blocks(raw=True)[k].tobytes() == before[k].tobytes() for k in before)
    gpu.close()


def test_integrated_corridor_map(mods):
    """S1 at 0.1 m, a few corridor frames, yaw 30 degrees plus a translation"""
    MLMap, _, _ = mods
    gpu = MLMap(S1, max_blocks=2048)
    for img, (q, t) in syn.stream(S1, "corridor", "smooth", 4):
        gpu.update_map(img, q, t)
    src = gpu.export_blocks()
    assert len(src["keys"]) > 50
    T = ref.make_T(ref.rot(30.0), (0.37, -1.21, 0.05))
    want = ref.warp(src, T, S1.subbox_n, S1.subbox_d_xyz)
    res = gpu.warp_blocks(T, out=True)
    same(res, want, "corridor")
    same_counts(res["summary"], want["summary"], "corridor")
    seen = gpu.warp_blocks(T, seen=True, out=True)
    same(seen, ref.warp(src, T, S1.subbox_n, S1.subbox_d_xyz, seen=True), "corridor, seen")
    assert 0 < seen["summary"][4] < res["summary"][4]
    gpu.close()


def test_reanchor_there_and_back(mods):
    """a translation by whole blocks and back returns the original sorted export.  A translation by whole voxels that is no multiple of
    subbox_n returns it too — on the original's blocks; the blocks the shifted map straddled come back as well, holding nothing but what
    allocate_ram leaves (their voxels are present in the shifted map, hence live)"""
    MLMap, _, invert_T = mods
    n = 7
    gpu = MLMap(small_cfg(n), max_blocks=64)
    src = craft(np.random.default_rng(12), n, 200)
    load(gpu, src)
    orig = gpu.export_blocks()
    for t, exact in (((n, -2 * n, 3 * n), True), ((3, -11, 8), False)):
        T = ref.make_T(None, np.asarray(t, dtype=np.float64) * 0.1)
        gpu.reanchor(T)
        moved = gpu.export_blocks()
        same(moved, ref.warp(orig, ref.invert(T), n, 0.1), f"reanchor by {t}")
        assert moved["keys"].tobytes() != orig["keys"].tobytes() and (len(moved["keys"]) == len(orig["keys"])) == exact
        gpu.reanchor(invert_T(T))
        back = gpu.export_blocks()
        row = {tuple(k): i for i, k in enumerate(back["keys"].tolist())}
        rows = np.array([row[tuple(k)] for k in orig["keys"].tolist()])
        same({k: back[k][rows] for k in PLANES}, orig, f"there and back by {t}")
        extra = np.setdiff1d(np.arange(len(back["keys"])), rows)
        assert (len(extra) == 0) == exact
        assert not back["log_odds"][extra].any() and np.all(back["occ"][extra] == ref.U) and np.all(back["infl"][extra] == ref.U)
        if not exact:  # (back to the original for the next round)
            empty(gpu)
            load(gpu, src)
            same(gpu.export_blocks(), orig, "reloaded")
    gpu.close()
