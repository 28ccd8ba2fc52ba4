"""mlm_crop_blocks on the GPU: crafted maps of every block geometry through every kind of box against the rule in numpy
(tests/crop_ref.py) and against an oracle that only ever saw the kept blocks; atomicity of the failing and the dry call; the page-out /
import round trip; integration, frontier mode and random operation sequences across a crop, mirrored on the oracle (which cannot drop a
block: there a crop is the dropped keys reset to what allocate_ram leaves, so a block the GPU lacks must be pristine in the oracle)."""
import ctypes
import os

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import crop_ref as ref
from tests.test_gpu_window import check_oracle, window_voxels
from tests.util import assert_same_bits, compare_maps

pytestmark = pytest.mark.gpu
EXTRA = [int(x) for x in os.environ.get("MLM_STRESS_SEEDS", "").split(",") if x]  # more seeds for a longer soak: MLM_STRESS_SEEDS=21,22,...
SEEDS = [3, 8, 10]
SEQ_N = {3: 3, 8: 8, 10: 10}
PLANES = ("keys", "log_odds", "occ", "infl", "collapsed")
WHOLE = ([ref.KEY_MIN] * 3, [1 << 21] * 3)
FAR_X = 1000  # blocks imported in a call of their own, far from the cube: the last slots of the pool


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap, MlmError
    from oracle.binding import OracleMap

    return MLMap, OracleMap, MlmError


def small_cfg(n, explore=False):
    return S1.with_(subbox_n=n, subbox_d_xyz=0.1, use_exploration_frontiers=explore, width=320, height=240, cam_cx=160.0, cam_cy=120.0,
                    cam_fx=192.5, cam_fy=192.5)


def same(a, b, what):
    for k in PLANES:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {k}"


def craft(rng, n, count, explore, side, edges=True):
    """count blocks: random keys of the cube [0, side)^3 plus both ends of the key range, distinct log-odds, random classes"""
    C = n ** 3
    edge = [[ref.KEY_MIN] * 3, [ref.KEY_MAX] * 3][:max(0, min(2, count - 1)) if edges else 0]
    flat = rng.choice(side ** 3, count - len(edge), replace=False)
    keys = np.concatenate([np.stack([flat % side, (flat // side) % side, flat // (side * side)], axis=1), np.array(edge, dtype=np.int64).reshape(-1, 3)])
    keys = keys[rng.permutation(count)].astype(np.int32)
    lo = (np.float32(-2.0) + rng.permutation(count * C).astype(np.float32) * np.float32(6.0 / (count * C))).reshape(count, C)
    return {"keys": keys, "log_odds": lo, "occ": rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(count, C)),
            "infl": rng.choice(np.frombuffer(b"uo", dtype=np.uint8), size=(count, C)),
            "collapsed": (rng.random(count) < 0.2).astype(np.uint8) if explore else np.zeros(count, dtype=np.uint8)}


def far_blocks(rng, n, m, explore):
    b = craft(rng, n, m, explore, 4, edges=False)
    b["keys"] = b["keys"] + np.array([FAR_X, 0, 0], dtype=np.int32)
    return b


def load(m, b):
    if len(b["keys"]):
        m.import_blocks(b["keys"], b["log_odds"], b["occ"], b["infl"], b["collapsed"] if b["collapsed"].any() else None)


def positions(rng, cfg, kept_keys, dropped_keys, k=60):
    """voxel centres of kept, dropped and neighbouring blocks (inside the key range's interior)"""
    n, d = cfg.subbox_n, cfg.subbox_d_xyz
    pick = lambda keys: keys[rng.integers(0, len(keys), k)] if len(keys) else np.zeros((0, 3), dtype=np.int64)
    inner = lambda keys: keys[(np.abs(keys) < (1 << 19)).all(axis=1)].astype(np.int64)
    a, b = pick(inner(kept_keys)), pick(inner(dropped_keys))
    near = np.concatenate([a, b]) + rng.integers(-1, 2, size=(len(a) + len(b), 3))
    keys = np.concatenate([a, b, near])
    cc = rng.integers(0, n, size=keys.shape)
    return keys.astype(np.float64) * (d * n) + cc * d + d * 0.5


def check_queries(gpu, cpu, pos, what):
    """every query kind against the oracle, bit for bit (a single position first: a host-mirror handle refreshes its mirror for a small
    batch only, and answers the batches behind it from the mirror)"""
    assert np.array_equal(gpu.getOccupancy(pos[:1]), cpu.getOccupancy(pos[:1])), what
    assert np.array_equal(gpu.getOccupancy(pos), cpu.getOccupancy(pos)), what
    assert np.array_equal(gpu.getInflateOccupancy(pos), cpu.getInflateOccupancy(pos)), what
    assert_same_bits(gpu.getOdd(pos), cpu.getOdd(pos), f"{what}: getOdd")
    assert np.array_equal(gpu.getOccupancy(pos, inflate=0.15), cpu.getOccupancy(pos, inflate=0.15)), what
    assert_same_bits(gpu.getOddGrad(pos, 5), cpu.getOddGrad(pos, 5), f"{what}: getOddGrad")


def check_window_across(gpu, cpu, cfg, lo_key, dims_key, what):
    """export_window over a few voxels either side of the box's low x face, against the oracle's queries"""
    n = cfg.subbox_n
    x0 = int(lo_key[0]) if abs(int(lo_key[0])) < (1 << 19) else 0  # (inside the key range's interior)
    lo, dims = [x0 * n - 3, 0, 0], [7, min(2 * n, 9), min(n, 5)]
    w = gpu.export_window(lo, dims, odds=True, occ=True, infl=True)
    keys, cid, cen = window_voxels(cfg, lo, dims)
    check_oracle(cpu, w, keys, cid, cen, 5)


def boxes(side):
    """(name, key_lo, key_dims, inside): nothing dropped, everything dropped, only the far (last) slots dropped, ~10 / 50 / 90 % both ways"""
    out = [("D0", *WHOLE, False), ("K0", *WHOLE, True), ("H0", [FAR_X, -8, -8], [64, 64, 64], True)]
    for pct in (10, 50, 90):
        w = max(1, round(side * pct / 100))
        out.append((f"in{pct}", [0, -4, -4], [w, side + 8, side + 8], True))
        out.append((f"out{pct}", [w, -4, -4], [side, side + 8, side + 8], False))
    return out


COUNTS = {2: [1, 63, 65, 257, 1000, 70000], 3: [1, 63, 65, 257, 1000], 4: [1, 63, 65, 257, 1000], 5: [1, 63, 65, 257, 1000],
          8: [1, 63, 65, 257, 1000], 16: [1, 63, 65, 257, 1000]}


@pytest.mark.parametrize("variant", ["kernel", "mirror"])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 16])
def test_crafted_maps(mods, knobs, n, variant):
    """one handle per geometry and query path; every case empties it (a crop of everything) and loads the next crafted map"""
    MLMap, OracleMap, _ = mods
    explore = (n % 2 == 1) != (variant == "mirror")
    cfg = small_cfg(n, explore)
    if variant == "kernel":
        knobs.set("mirror", 0)
    else:
        knobs.set("mirror_max", 1 << 20)
    gpu = MLMap(cfg, max_blocks=64)
    rng = np.random.default_rng(1000 * n + (variant == "mirror"))
    seen = set()
    for count in COUNTS[n]:
        side = max(3, int(np.ceil((2.5 * count) ** (1 / 3))))
        for name, lo, dims, inside in boxes(side):
            if count == 70000 and name not in ("in50", "out10", "H0"):
                continue
            what = f"n {n} {variant} count {count} box {name}"
            gpu.crop_blocks(*WHOLE, inside=True)
            assert gpu.block_count() == 0 and gpu.frame_stats()["n_blocks"] == 0, what
            src, far = craft(rng, n, count, explore, side), far_blocks(rng, n, 5, explore)
            load(gpu, src)
            load(gpu, far)
            before = gpu.export_blocks(raw=True)
            assert sorted(map(tuple, before["keys"])) == sorted(map(tuple, np.concatenate([src["keys"], far["keys"]]))), what
            oracle_too = count <= 257 or name == "in50"
            if oracle_too:
                full = OracleMap(cfg)
                load(full, {k: v for k, v in before.items()})
                drop0 = ref.drops(before["keys"], lo, dims, inside)
                pos = positions(rng, cfg, before["keys"][~drop0], before["keys"][drop0])
                check_queries(gpu, full, pos, what + " before")
                full.close()
            s0 = gpu.frame_stats()
            res = gpu.crop_blocks(lo, dims, inside=inside, out=True)
            kept, rows, p = ref.crop(before, lo, dims, inside)
            seen.add((p["D"] == 0, p["K"] == 0, p["H"] == 0))
            after, s1 = gpu.export_blocks(raw=True), gpu.frame_stats()
            same(after, kept, what + " raw order")
            same(res, rows, what + " rows")
            sm = res["summary"]
            assert sm[:4].tolist() == [len(before["keys"]), p["K"], p["D"], p["D"]] and sm[4] == sm[5] == s1["block_capacity"], (what, sm)
            # (the sizing call of out=True may have enlarged the scratch the handle keeps: 4 bytes per block)
            assert s0["device_bytes"] <= sm[6] <= sm[7] == s1["device_bytes"] and sm[6] - s0["device_bytes"] <= 4 * len(before["keys"]) + 8192, (what, sm)
            assert gpu.block_count() == p["K"] and s1["n_blocks"] == p["K"], what
            if name == "H0":
                assert p["H"] == 0 and p["D"] == 5, what
            if oracle_too:
                cpu = OracleMap(cfg)
                load(cpu, kept)
                check_queries(gpu, cpu, pos, what + " after")
                check_window_across(gpu, cpu, cfg, lo, dims, what)
                h = gpu.frame_stats()["n_host_queries"]
                assert (h == 0) if variant == "kernel" else (h >= s0["n_host_queries"] + 5 * len(pos)), what
                cpu.close()
    assert {(True, False, True), (False, True, True), (False, False, True), (False, False, False)} <= seen, seen
    gpu.close()


def raw_call(gpu, lo, dims, flags, cap, outs):
    lo_a = np.asarray([0, 0, 0] if lo is None else lo, dtype=np.int32)
    dims_a = np.asarray([1, 1, 1] if dims is None else dims, dtype=np.int32)
    sm = np.zeros(ref.ROW, dtype=np.int64)
    ptr = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in outs]
    rc = gpu._L.mlm_crop_blocks(gpu._h, lo_a.ctypes.data_as(ctypes.c_void_p) if lo is not None else None,
                                dims_a.ctypes.data_as(ctypes.c_void_p) if dims is not None else None, flags, cap, *ptr,
                                sm.ctypes.data_as(ctypes.c_void_p))
    return rc, sm, gpu._L.mlm_last_error(gpu._h).decode()


def out_arrays(cap, C):
    return [np.full((cap, 3), 7, dtype=np.int32), np.full((cap, C), 7, dtype=np.float32), np.full((cap, C), 7, dtype=np.uint8),
            np.full((cap, C), 7, dtype=np.uint8), np.full(cap, 7, dtype=np.uint8)]


def test_failing_and_dry_calls_leave_the_map_alone(mods, knobs):
    MLMap, _, _ = mods
    knobs.set("mirror_max", 1 << 20)
    cfg = small_cfg(5, True)
    gpu = MLMap(cfg, max_blocks=64)
    rng = np.random.default_rng(4)
    load(gpu, craft(rng, 5, 300, True, 9))
    before = gpu.export_blocks(raw=True)
    lo, dims = [0, -4, -4], [4, 20, 20]
    D = int(ref.drops(before["keys"], lo, dims, True).sum())
    assert 60 < D < 240
    cap0 = int(gpu.crop_blocks(lo, dims, inside=True, dry=True)["summary"][4])
    assert cap0 >= 300
    for flags, cap, outs, want in ((ref.INSIDE, D - 1, out_arrays(D - 1, 125), ref.ERR_CAPACITY), (ref.INSIDE, 0, out_arrays(1, 125), ref.ERR_CAPACITY),
                                   (ref.INSIDE, D - 1, [None, None, None, None, np.zeros(D, np.uint8)], ref.ERR_CAPACITY),
                                   (ref.INSIDE | ref.DRY, D, out_arrays(D, 125), ref.OK), (ref.INSIDE | ref.DRY | ref.SHRINK, 0, [None] * 5, ref.OK)):
        rc, sm, err = raw_call(gpu, lo, dims, flags, cap, outs)
        assert rc == want and (rc == ref.OK or "dropped" in err), (rc, err)
        assert sm.tolist()[:6] == [300, 300 - D, D, 0, cap0, cap0] and sm[6] == sm[7], sm
        if outs[0] is not None:
            assert all(np.all(a == 7) for a in outs), "an output was written"
        same(gpu.export_blocks(raw=True), before, "map after a failing / dry call")
    # D == 0: a no-op that leaves the mirror what it was
    pos = positions(rng, cfg, before["keys"], before["keys"])
    gpu.getOdd(pos[:8])
    s0 = gpu.frame_stats()
    res = gpu.crop_blocks(*WHOLE, inside=False, out=True, shrink=True)
    assert res["summary"][:4].tolist() == [300, 300, 0, 0] and len(res["keys"]) == 0
    gpu.getOdd(pos[:8])
    s1 = gpu.frame_stats()
    assert s1["n_mirror_refreshes"] == s0["n_mirror_refreshes"] and s1["n_host_queries"] == s0["n_host_queries"] + 8
    same(gpu.export_blocks(raw=True), before, "map after D == 0")
    gpu.close()


@pytest.mark.parametrize("n,explore,stage_rows", [(3, True, 1), (8, False, 7), (10, True, None)])
def test_page_out_and_import_round_trip(mods, knobs, n, explore, stage_rows):
    """stage_rows: host destinations staged in rounds of so many blocks (None: the call's own 64 MB rounds, one here)"""
    import torch

    MLMap, _, _ = mods
    if stage_rows:
        knobs.set("crop_stage_rows", stage_rows)
    cfg = small_cfg(n, explore)
    gpu = MLMap(cfg, max_blocks=64)
    rng = np.random.default_rng(n)
    load(gpu, craft(rng, n, 400, explore, 10))
    orig = gpu.export_blocks()
    lo, dims = [2, -4, -4], [5, 30, 30]
    # host arrays
    res = gpu.crop_blocks(lo, dims, inside=True, out=True)
    D = int(res["summary"][2])
    assert 100 < D < 300 and gpu.block_count() == 400 - D
    assert ref.drops(res["keys"], lo, dims, True).all() and not ref.drops(gpu.export_blocks()["keys"], lo, dims, True).any()
    gpu.import_blocks(res["keys"], res["log_odds"], res["occ"], res["infl"], res["collapsed"])
    same(gpu.export_blocks(), orig, "round trip through host arrays")
    # torch device tensors (one row to spare, which must stay as it was)
    C = n ** 3
    dev = {"keys": torch.full((D + 1, 3), 7, dtype=torch.int32, device="cuda"), "log_odds": torch.full((D + 1, C), 7, dtype=torch.float32, device="cuda"),
           "occ": torch.full((D + 1, C), 7, dtype=torch.uint8, device="cuda"), "infl": torch.full((D + 1, C), 7, dtype=torch.uint8, device="cuda"),
           "collapsed": torch.full((D + 1,), 7, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()
    before = gpu.export_blocks(raw=True)
    res2 = gpu.crop_blocks(lo, dims, inside=True, out={"cap": D + 1, **{k: v.data_ptr() for k, v in dev.items()}})
    assert res2["summary"][:4].tolist() == [400, 400 - D, D, D]
    got = {k: v.cpu().numpy() for k, v in dev.items()}
    assert all(np.all(v[D:] == 7) for v in got.values())
    _, rows, _ = ref.crop(before, lo, dims, True)
    same({k: v[:D] for k, v in got.items()}, rows, "device rows")
    gpu.import_blocks((dev["keys"].data_ptr(), D), dev["log_odds"].data_ptr(), dev["occ"].data_ptr(), dev["infl"].data_ptr(), dev["collapsed"].data_ptr())
    same(gpu.export_blocks(), orig, "round trip through device tensors")
    gpu.close()


def pristine(b, rows):
    return not b["log_odds"][rows].any() and np.all(b["occ"][rows] == ord("u")) and np.all(b["infl"][rows] == ord("u")) and not b["collapsed"][rows].any()


def compare_after_crop(gpu, cpu, what):
    """every block the GPU holds equals the oracle's bit for bit; every oracle block the GPU lacks is pristine.  Returns the keys the GPU lacks."""
    g, c = gpu.export_blocks(), cpu.export_blocks()
    ck = {tuple(k): i for i, k in enumerate(c["keys"])}
    idx = np.array([ck.get(tuple(k), -1) for k in g["keys"]], dtype=np.int64)
    assert (idx >= 0).all(), f"{what}: the GPU holds blocks the oracle lacks"
    compare_maps(g, {k: v[idx] for k, v in c.items()}, what)
    lacks = np.setdiff1d(np.arange(len(c["keys"])), idx)
    assert pristine(c, lacks), f"{what}: a block the GPU lacks is not pristine in the oracle"
    return c["keys"][lacks]


def reset_in_oracle(cpu, keys):
    if len(keys):
        C = cpu.cells
        cpu.import_blocks(keys, np.zeros((len(keys), C), np.float32), np.full((len(keys), C), ord("u"), np.uint8),
                          np.full((len(keys), C), ord("u"), np.uint8), np.zeros(len(keys), np.uint8))


def middle_box(keys):
    """a box through the middle of the blocks: everything from the median x on"""
    k = np.asarray(keys, dtype=np.int64)
    mx = int(np.median(k[:, 0]))
    lo = [mx, int(k[:, 1].min()), int(k[:, 2].min())]
    return lo, [int(k[:, 0].max()) - mx + 1, int(k[:, 1].max() - k[:, 1].min()) + 1, int(k[:, 2].max() - k[:, 2].min()) + 1]


@pytest.mark.parametrize("use_async", [False, True])
def test_integration_after_a_crop(mods, use_async):
    MLMap, OracleMap, _ = mods
    gpu, cpu = MLMap(S1, max_blocks=64, max_batch=3), OracleMap(S1)
    frames = list(syn.stream(S1, "room_jitter", "smooth", 12))
    gpu.set_async(use_async)

    def run(part):
        if use_async:
            for b in range(0, len(part), 3):
                gpu.update_map_batch(np.stack([f for f, _ in part[b:b + 3]]), np.stack([q for _, (q, _) in part[b:b + 3]]),
                                     np.stack([t for _, (_, t) in part[b:b + 3]]))
        else:
            for img, (q, t) in part:
                gpu.update_map(img, q, t)
        for img, (q, t) in part:
            cpu.update_depth(img, q, t)

    g0 = gpu.frame_stats()["n_graph_launches"]
    run(frames[:6])
    lo, dims = middle_box(cpu.export_blocks()["keys"])
    res = gpu.crop_blocks(lo, dims, inside=True, shrink=True, out=True)  # (async: straight behind the submit, no sync)
    sm, s1 = res["summary"], gpu.frame_stats()
    print("crop summary", sm.tolist(), "pool grows", s1["n_pool_grows"])
    nb0 = cpu.block_count()
    assert sm[0] == nb0 and 0 < sm[2] < nb0 and sm[4] > 64 and s1["n_pool_grows"] >= 1
    assert ref.drops(res["keys"], lo, dims, True).all() and len(res["keys"]) == sm[2]
    target = ref.shrink_target(64, int(sm[4]), int(sm[1]))
    assert sm[5] == (target or sm[4]) == s1["block_capacity"] and s1["n_blocks"] == sm[1]
    assert target and sm[7] < sm[6] and sm[7] == s1["device_bytes"], "the pool did not shrink"
    if not use_async:
        assert s1["n_graph_launches"] > g0, "single frames do not run as graphs"
    reset_in_oracle(cpu, res["keys"])
    compare_after_crop(gpu, cpu, "right after the crop")
    run(frames[6:])
    gpu.sync()
    s2 = gpu.frame_stats()
    lacks = compare_after_crop(gpu, cpu, "six frames after the crop")
    print("after", s2["n_blocks"], "capacity", s2["block_capacity"], "pool grows", s2["n_pool_grows"], "lacks", len(lacks))
    assert s2["n_blocks"] > sm[1], "the later frames created no block afresh"
    if not use_async:
        assert s2["n_graph_launches"] > s1["n_graph_launches"], "the graphs did not survive the crop"
    assert s2["n_pool_grows"] > s1["n_pool_grows"] and s2["block_capacity"] > sm[5], "the pool did not grow again"
    gpu.close()


def test_frontier_mode(mods):
    MLMap, OracleMap, _ = mods
    cfg = S1.with_(use_exploration_frontiers=True)
    gpu, cpu = MLMap(cfg, max_blocks=64), OracleMap(cfg)
    frames = list(syn.stream(cfg, "room_jitter", "smooth", 12))
    reach = int(np.ceil(cfg.am_n_Rho * cfg.am_d_Rho / (cfg.subbox_n * cfg.subbox_d_xyz))) + 2
    far = craft(np.random.default_rng(6), 10, 40, True, 4, edges=False)
    far["keys"] = far["keys"] + np.array([reach + 3, 0, 0], dtype=np.int32)  # (farther from every pose than the awareness range plus two blocks)
    load(gpu, far), load(cpu, far)  # (first: the lowest slots, so that the crop has holes to fill)
    for img, (q, t) in frames[:6]:
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
    compare_maps(gpu.export_blocks(), {k: v for k, v in cpu.export_blocks().items() if k != "frontier_cnt"}, "before the crop")
    lo, dims = [reach + 2, -reach - 8, -reach - 8], [16, 2 * reach + 16, 2 * reach + 16]
    before = gpu.export_blocks(raw=True)
    res = gpu.crop_blocks(lo, dims, inside=True, out=True)
    _, rows, p = ref.crop(before, lo, dims, True)
    same(res, rows, "dropped rows")
    assert p["D"] == len(far["keys"]) and p["H"] > 0 and res["summary"][:3].tolist() == [len(before["keys"]), p["K"], p["D"]]
    for img, (q, t) in frames[6:]:
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
    c = cpu.export_blocks()
    keep = ~ref.drops(c["keys"], lo, dims, True)
    compare_maps(gpu.export_blocks(), {k: v[keep] for k, v in c.items() if k != "frontier_cnt"}, "six frames after the crop")
    cf = cpu.export_frontier()
    cf = cf[~ref.drops(cf[:, :3], lo, dims, True)]
    gf = gpu.export_frontier()
    assert len(cf) > 0 and np.array_equal(gf, cf), "frontier sets differ"
    gpu.close()


@pytest.mark.parametrize("seed", SEEDS + EXTRA)
def test_random_sequences(mods, seed):
    MLMap, OracleMap, _ = mods
    n = SEQ_N.get(seed, (3, 8, 10)[seed % 3])
    cfg = small_cfg(n)
    rng = np.random.default_rng(100 * seed)
    gpu, cpu = MLMap(cfg, max_blocks=64), OracleMap(cfg)
    base, traj = syn.room_depth(cfg), syn.smooth_trajectory(64, seed)
    d_glb, k, log, crops = n * cfg.subbox_d_xyz, 0, [], 0
    ops = ["integrate", "integrate", "crop", "set_free", "inflate", "import", "integrate", "crop"] + list(rng.choice(
        ["integrate", "set_free", "inflate", "import", "crop"], size=12, p=[0.35, 0.15, 0.1, 0.15, 0.25]))
    for step, op in enumerate(ops):
        log.append(op)
        what = f"seed {seed}, n {n}, step {step}: {log}"
        q, t = traj[k]
        if op == "integrate":
            img = syn.jitter_depth(base, k, seed=seed)
            gpu.update_map(img, q, t)
            cpu.update_depth(img, q, t)
            k += 1
        elif op == "set_free":
            held = gpu.export_blocks()["keys"]
            if len(held):  # a box inside one block the GPU holds (the oracle's stand-in blocks must stay pristine)
                key = held[rng.integers(0, len(held))].astype(np.float64)
                lo = key * d_glb + rng.uniform(0.1, 0.4, 3) * d_glb
                hi = lo + rng.uniform(0.1, 0.5, 3) * d_glb
                gpu.setFree_map_in_bound(lo, hi)
                cpu.setFree_map_in_bound(lo, hi)
        elif op == "inflate":
            gpu.inflate_map(t)
            cpu.inflate_map(t)
        elif op == "import":
            b = craft(rng, n, 6, False, 3, edges=False)
            b["keys"] = (b["keys"] + np.floor(t / d_glb).astype(np.int32) + rng.integers(-2, 3, 3)).astype(np.int32)
            _, first = np.unique(b["keys"], axis=0, return_index=True)
            b = {kk: v[np.sort(first)] for kk, v in b.items()}
            load(gpu, b), load(cpu, b)
        else:
            c = np.floor(t / d_glb).astype(np.int64) + rng.integers(-2, 3, 3)
            w = rng.integers(1, 5, 3)
            inside = bool(rng.random() < 0.5)
            lo, dims = (c - w, 2 * w + 1) if not inside else (c - np.array([0, 30, 30]), np.array([int(w[0]), 60, 60]))
            before = gpu.export_blocks(raw=True)
            res = gpu.crop_blocks(lo, dims, inside=inside, shrink=bool(rng.random() < 0.5), out=True)
            kept, rows, p = ref.crop(before, lo, dims, inside)
            same(res, rows, what + " rows")
            same(gpu.export_blocks(raw=True), kept, what + " raw order")
            reset_in_oracle(cpu, res["keys"])
            crops += p["D"] > 0 and p["K"] > 0
        compare_after_crop(gpu, cpu, what)
    assert crops >= 2 and k >= 3, (crops, log)
    assert gpu.frame_stats()["n_pool_grows"] >= 1
    gpu.close()


def test_invalid_arguments(mods):
    MLMap, _, MlmError = mods
    cfg = small_cfg(4)
    gpu = MLMap(cfg, max_blocks=64)
    load(gpu, craft(np.random.default_rng(0), 4, 50, False, 5))
    before = gpu.export_blocks(raw=True)
    none5 = [None] * 5
    cases = [(None, [1, 1, 1], 0, 0), ([0, 0, 0], None, 0, 0), ([0, 0, 0], [0, 1, 1], 0, 0), ([0, 0, 0], [1, 1, -3], 1, 0),
             ([ref.I32_MAX, 0, 0], [1, 1, 1], 0, 0), ([0, 5, 0], [1, ref.I32_MAX - 4, 1], 1, 0), ([0, 0, 0], [1, 1, 1], 8, 0),
             ([0, 0, 0], [1, 1, 1], -1, 0), ([0, 0, 0], [1, 1, 1], 1 | 64, 0), ([0, 0, 0], [1, 1, 1], 0, -1), ([0, 0, 0], [1, 1, 1], 2, -7)]
    for lo, dims, flags, cap in cases:
        rc, _, err = raw_call(gpu, lo, dims, flags, cap, none5)
        assert rc == ref.ERR_INVALID and err.startswith("mlm_crop_blocks: ") and len(err) > 25, (lo, dims, flags, cap, rc, err)
        if lo is not None and dims is not None:
            assert ref.check_args(lo, dims, flags, cap) != 0
    with pytest.raises(MlmError):
        gpu.crop_blocks([0, 0, 0], [0, 0, 0])
    same(gpu.export_blocks(raw=True), before, "map after invalid calls")
    res = gpu.crop_blocks([0, 0, 0], [2, 9, 9], inside=True)  # the handle stays usable
    assert res["summary"][2] > 0 and gpu.block_count() == 50 - res["summary"][2]
    lo, dims = ref.retain_box([0.2, 0.2, 0.2], 0.5, 4 * 0.1)
    res = gpu.retain_around([0.2, 0.2, 0.2], 0.5)
    assert not ref.drops(gpu.export_blocks()["keys"], lo, dims, False).any() and res["summary"][1] == gpu.block_count()
    gpu.close()
