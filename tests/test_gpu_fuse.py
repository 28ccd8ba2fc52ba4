"""mlm_fuse_blocks on the GPU: crafted maps of every block geometry fused with crafted dumps in every mode, from host and from device
memory, with infl, per_row and summary left out in turn, byte for byte against the contract in numpy (tests/fuse_ref.py) in raw slot
order; unaligned device sources; atomicity of the failing calls; MLM_FUSE_DRY; frontier mode; the host mirror; integration on both
sides of a fuse against a twin that fuses by the definition; fuse_from against warp_ref followed by fuse_ref."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from tests import fuse_ref as ref
from tests import warp_ref
from tests.test_gpu_warp import craft, empty, load, small_cfg

pytestmark = pytest.mark.gpu
PLANES = ("keys", "log_odds", "occ", "infl")
MODES = ("add", "max", "take", "fill")


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap, MlmError

    return MLMap, MlmError


def same(a, b, what):
    for k in PLANES:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {k}"


def craft_pair(rng, n, held, rows, explore=False):
    """a map of `held` blocks and a dump of `rows` rows, about half of whose keys the map holds; the dump has rows nothing has seen
    (craft's blank ones), rows with only infl, and log-odds beyond the clamp range"""
    pool = craft(rng, n, held + rows, explore)
    m = {k: v[:held] for k, v in pool.items()}
    d = craft(rng, n, rows)
    k_own = min(held, rows // 2)
    d["keys"] = np.concatenate([m["keys"][rng.permutation(held)[:k_own]], pool["keys"][held:held + rows - k_own]])[rng.permutation(rows)].astype(np.int32)
    d["occ"][rng.random(rows) < 0.15] = ref.U
    d["log_odds"] = (d["log_odds"] * np.float32(1.5)).astype(np.float32)
    return m, {k: d[k] for k in PLANES}


def to_device(rows, offset=False):
    """the dump in torch device tensors; offset: the float plane starts one element, the byte planes one byte into their allocation"""
    import torch

    keep, ptr = [], {}
    for k in PLANES:
        a = np.ascontiguousarray(rows[k])
        flat = torch.from_numpy(a.reshape(-1).copy())
        o = 1 if offset and k != "keys" else 0
        t = torch.zeros(flat.numel() + o, dtype=flat.dtype, device="cuda")
        t[o:] = flat.cuda()
        keep.append(t)
        ptr[k] = t.data_ptr() + o * t.element_size()
    torch.cuda.synchronize()
    return keep, ptr


def raw_call(gpu, n, ptr, mode, flags, per_row, summary):
    vp = lambda a: None if a is None else ctypes.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(ctypes.c_void_p)
    rc = gpu._L.mlm_fuse_blocks(gpu._h, n, vp(ptr["keys"]), vp(ptr["log_odds"]), vp(ptr["occ"]), vp(ptr.get("infl")), mode, flags, vp(per_row), vp(summary))
    return rc, gpu._L.mlm_last_error(gpu._h).decode()


COMBOS = [(0, 1), (1, 65), (65, 300), (300, 65), (0, 300), (300, 1)]


@pytest.mark.parametrize("n", [2, 3, 4, 7, 8, 16])
def test_crafted_maps(mods, n):
    """one handle per geometry, created with room for 64 blocks: the pool grows inside a fuse.  Per case the four modes, each on the
    freshly loaded map: ADD from host arrays, MAX from device tensors, TAKE without infl, FILL from device tensors without per_row —
    and a call without summary with per_row in device memory."""
    import torch

    MLMap, _ = mods
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(3000 + n)
    grew = 0
    for held, rows_n in COMBOS:
        m, rows = craft_pair(rng, n, held, rows_n)
        for mode in MODES:
            what = f"n {n} held {held} rows {rows_n} {mode}"
            empty(gpu)
            load(gpu, dict(m, collapsed=np.zeros(held, np.uint8)))
            before = gpu.export_blocks(raw=True)
            infl_given = mode != "take"
            want, sm, pr = ref.fuse(before, rows, mode, infl_given=infl_given)
            cap0, nb0 = gpu.frame_stats()["block_capacity"], gpu.block_count()
            keep, ptr = to_device(rows) if mode in ("max", "fill") else (None, None)
            src = (rows["keys"], rows["log_odds"], rows["occ"], rows["infl"] if infl_given else None) if ptr is None else (
                (ptr["keys"], rows_n), ptr["log_odds"], ptr["occ"], ptr["infl"])
            dry = gpu.fuse_blocks(*src, mode=mode, dry=True, per_row=True)
            assert dry["summary"].tolist() == sm.tolist() and dry["per_row"].tolist() == pr.tolist(), what + " dry"
            assert gpu.block_count() == nb0 and gpu.frame_stats()["block_capacity"] == cap0
            same(gpu.export_blocks(raw=True), before, what + " dry")
            res = gpu.fuse_blocks(*src, mode=mode, per_row=mode != "fill")
            assert res["summary"].tolist() == sm.tolist(), (what, res["summary"].tolist(), sm.tolist())
            assert res["per_row"] is None if mode == "fill" else res["per_row"].tolist() == pr.tolist(), what
            after = gpu.export_blocks(raw=True)
            same(after, want, what)
            st = gpu.frame_stats()
            assert gpu.block_count() == len(want["keys"]) == st["n_blocks"] == nb0 + sm[2] and st["block_capacity"] >= st["n_blocks"]
            grew += st["block_capacity"] > cap0
            del keep
    assert grew >= 1
    # no summary, per_row in device memory, on top of what the last case left
    m, rows = craft_pair(rng, n, 0, 65)
    before = gpu.export_blocks(raw=True)
    want, sm, pr = ref.fuse(before, rows, ref.ADD)
    keep, ptr = to_device(rows)
    d_pr = torch.full((65, 4), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc, err = raw_call(gpu, 65, ptr, ref.ADD, 0, d_pr.data_ptr(), None)
    assert rc == 0, err
    assert d_pr.cpu().numpy().tolist() == pr.tolist()
    same(gpu.export_blocks(raw=True), want, f"n {n} without summary")
    gpu.close()


@pytest.mark.parametrize("n", [4, 8])
def test_unaligned_device_sources(mods, n):
    """a float plane one element and byte planes one byte into their allocations: the narrow lane paths, the same answers"""
    MLMap, _ = mods
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(3100 + n)
    m, rows = craft_pair(rng, n, 65, 65)
    for mode in MODES:
        empty(gpu)
        load(gpu, dict(m, collapsed=np.zeros(65, np.uint8)))
        before = gpu.export_blocks(raw=True)
        want, sm, pr = ref.fuse(before, rows, mode)
        keep, ptr = to_device(rows, offset=True)
        assert ptr["log_odds"] % 16 == 4 and ptr["occ"] % 4 == 1
        res = gpu.fuse_blocks((ptr["keys"], 65), ptr["log_odds"], ptr["occ"], ptr["infl"], mode=mode, per_row=True)
        assert res["summary"].tolist() == sm.tolist() and res["per_row"].tolist() == pr.tolist(), mode
        same(gpu.export_blocks(raw=True), want, f"unaligned n {n} {mode}")
    gpu.close()


def test_failing_calls_leave_the_map_untouched(mods, knobs):
    MLMap, MlmError = mods
    n = 4
    knobs.set("pool_grow", 0)
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(3200)
    m, rows = craft_pair(rng, n, 50, 65)
    load(gpu, dict(m, collapsed=np.zeros(50, np.uint8)))
    before = gpu.export_blocks(raw=True)
    want, sm, pr = ref.fuse(before, rows, ref.ADD)
    assert 50 + sm[2] > 64
    dup = {k: v.copy() for k, v in rows.items()}
    dup["keys"][50] = dup["keys"][7]
    far = {k: v.copy() for k, v in rows.items()}
    far["keys"][64] = [0, 0, ref.KEY_MAX + 1]
    keep, far_dev = to_device(far)
    cases = [(dup, "MLM_ERR_INVALID", "same block key"), (far, "MLM_ERR_INVALID", "21-bit"), (rows, "MLM_ERR_CAPACITY", "created blocks")]
    for mode in ("add", "fill"):
        for dry in (False, True):
            for bad, status, text in cases:
                if dry and status == "MLM_ERR_CAPACITY":
                    continue  # (a diff needs no room: below)
                with pytest.raises(MlmError) as e:
                    gpu.fuse_blocks(bad["keys"], bad["log_odds"], bad["occ"], bad["infl"], mode=mode, dry=dry)
                assert status in str(e.value) and text in str(e.value), str(e.value)
                same(gpu.export_blocks(raw=True), before, f"{text} {mode}")
                assert gpu.block_count() == 50
    with pytest.raises(MlmError) as e:
        gpu.fuse_blocks((far_dev["keys"], 65), far_dev["log_odds"], far_dev["occ"], far_dev["infl"])
    assert "21-bit" in str(e.value)
    for bad_mode, bad_flags, text in ((4, 0, "mode"), (0, 2, "flag")):
        rc, err = raw_call(gpu, 65, rows, bad_mode, bad_flags, None, None)
        assert rc == ref.ERR_INVALID and text in err
    rc, err = raw_call(gpu, -1, rows, 0, 0, None, None)
    assert rc == ref.ERR_INVALID
    rc, err = raw_call(gpu, 5, dict(rows, occ=None), 0, 0, None, None)
    assert rc == ref.ERR_INVALID
    sm0 = np.full(ref.ROW, -9, dtype=np.int64)
    rc, err = raw_call(gpu, 0, {"keys": None, "log_odds": None, "occ": None}, 0, 0, None, sm0)
    assert rc == ref.OK and not sm0.any()
    same(gpu.export_blocks(raw=True), before, "invalid arguments")
    # the diff of the dump that does not fit works, and so does the next valid call
    res = gpu.fuse_blocks(rows["keys"], rows["log_odds"], rows["occ"], rows["infl"], dry=True, per_row=True)
    assert res["summary"].tolist() == sm.tolist() and res["per_row"].tolist() == pr.tolist()
    few = {k: v[:12] for k, v in rows.items()}
    want, sm, pr = ref.fuse(before, few, ref.ADD)
    assert 50 + sm[2] <= 64
    res = gpu.fuse_blocks(few["keys"], few["log_odds"], few["occ"], few["infl"], per_row=True)
    assert res["summary"].tolist() == sm.tolist() and res["per_row"].tolist() == pr.tolist()
    same(gpu.export_blocks(raw=True), want, "the next valid call")
    gpu.close()


@pytest.mark.parametrize("n", [3, 4])
def test_frontier_mode(mods, n):
    """the fuse itself is refused; the diff reads a released block from element 0 with infl 'u'"""
    MLMap, MlmError = mods
    gpu = MLMap(small_cfg(n, explore=True), max_blocks=64)
    rng = np.random.default_rng(3300 + n)
    m, rows = craft_pair(rng, n, 65, 65, explore=True)
    assert m["collapsed"].any()
    load(gpu, m)
    before = gpu.export_blocks(raw=True)
    assert before["collapsed"].any()
    for mode in MODES:
        with pytest.raises(MlmError) as e:
            gpu.fuse_blocks(rows["keys"], rows["log_odds"], rows["occ"], rows["infl"], mode=mode)
        assert "MLM_ERR_INVALID" in str(e.value) and "frontier" in str(e.value)
        _, sm, pr = ref.fuse(ref.expanded(before), rows, mode, dry=True)
        res = gpu.fuse_blocks(rows["keys"], rows["log_odds"], rows["occ"], rows["infl"], mode=mode, dry=True, per_row=True)
        assert res["summary"].tolist() == sm.tolist() and res["per_row"].tolist() == pr.tolist(), mode
        after = gpu.export_blocks(raw=True)
        same(after, before, f"frontier {mode}")
        assert np.array_equal(after["collapsed"], before["collapsed"])
    gpu.close()


def test_host_mirror_follows_a_fuse(mods):
    """small host batches are answered from the host mirror: after a fuse they answer from the new content"""
    MLMap, _ = mods
    n, d = 4, 0.1
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(3400)
    m, rows = craft_pair(rng, n, 40, 40)
    load(gpu, dict(m, collapsed=np.zeros(40, np.uint8)))
    r, c = np.nonzero((rows["occ"] != ref.U))
    pick = rng.permutation(len(r))[:48]
    r, c = r[pick], c[pick]
    cell = np.stack([c % n, (c // n) % n, c // (n * n)], axis=1)
    pos = (rows["keys"][r].astype(np.float64) * n + cell + 0.5) * d

    def classes(b):
        at = {tuple(k): i for i, k in enumerate(b["keys"].tolist())}
        occ = np.array([b["occ"][at[tuple(k)], ci] if tuple(k) in at else ref.U for k, ci in zip(rows["keys"][r].tolist(), c)])
        return np.where(occ == ref.O, MLMap.OCCUPIED, np.where(occ == ref.F, MLMap.FREE, MLMap.UNKNOWN))

    before = gpu.export_blocks(raw=True)
    odd0 = gpu.getOdd(pos)
    assert np.array_equal(gpu.getOccupancy(pos), classes(before))
    want, sm, _ = ref.fuse(before, rows, ref.ADD)
    gpu.fuse_blocks(rows["keys"], rows["log_odds"], rows["occ"], rows["infl"])
    twin = MLMap(small_cfg(n), max_blocks=128)  # the same queries of a handle that was given the fused map whole
    load(twin, dict(want, collapsed=np.zeros(len(want["keys"]), np.uint8)))
    odd1 = gpu.getOdd(pos)
    assert (odd1 != odd0).sum() > 20 and (classes(want) != MLMap.UNKNOWN).all()
    assert np.array_equal(odd1.view(np.uint32), twin.getOdd(pos).view(np.uint32)) and np.array_equal(gpu.getOccupancy(pos), classes(want))
    twin.close()
    gpu.close()


def frames(cfg, seed, count):
    base, traj = syn.room_depth(cfg), syn.smooth_trajectory(32, seed)
    return [(syn.jitter_depth(base, k, seed=seed), *traj[k]) for k in range(count)]


def fuse_by_definition(b, rows, mode, infl_given=True):
    """export, the numpy rule, a crop of everything, import_blocks"""
    want, sm, _ = ref.fuse(b.export_blocks(raw=True), rows, mode, infl_given=infl_given)
    empty(b)
    if len(want["keys"]):
        b.import_blocks(want["keys"], want["log_odds"], want["occ"], want["infl"])
    return sm


@pytest.mark.parametrize("n", [4, 9])
def test_integration_on_both_sides(mods, n):
    MLMap, _ = mods
    cfg = small_cfg(n)
    a, b, c = MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64)
    for img, q, t in frames(cfg, 11, 3):
        c.update_map(img, q, t)
    rows = c.export_blocks()
    assert len(rows["keys"]) > 4
    fr = frames(cfg, 5, 6)
    for step, mode in enumerate(MODES):
        for img, q, t in fr[step:step + 2]:
            a.update_map(img, q, t), b.update_map(img, q, t)
        same(a.export_blocks(), b.export_blocks(), f"n {n} step {step} before")
        res = a.fuse_blocks(rows["keys"], rows["log_odds"], rows["occ"], rows["infl"], mode=mode)
        sm = fuse_by_definition(b, rows, mode)
        assert res["summary"].tolist() == sm.tolist()
        same(a.export_blocks(), b.export_blocks(), f"n {n} step {step} {mode}")
    for img, q, t in fr[4:6]:
        a.update_map(img, q, t), b.update_map(img, q, t)
    ea = a.export_blocks()
    same(ea, b.export_blocks(), f"n {n} after")
    assert a.block_count() == len(ea["keys"]) == a.frame_stats()["n_blocks"]
    for m in (a, b, c):
        m.close()


@pytest.mark.parametrize("mode", ["add", "fill"])
def test_fuse_from_another_handle(mods, mode):
    """fuse_from(other, T) is warp_ref.warp(other, T, seen) followed by fuse_ref.fuse, the dump never leaving the device"""
    MLMap, _ = mods
    n = 4
    cfg = small_cfg(n)
    a, other = MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64)
    for img, q, t in frames(cfg, 5, 3):
        a.update_map(img, q, t)
    for img, q, t in frames(cfg, 11, 3):
        other.update_map(img, q, t)
    for T in (None, warp_ref.make_T(warp_ref.rot(2.0, -0.5, 0.7), (0.13, -0.21, 0.08))):
        before = a.export_blocks(raw=True)
        dump = warp_ref.warp(other.export_blocks(), warp_ref.make_T() if T is None else T, n, cfg.subbox_d_xyz, seen=True)
        want, sm, _ = ref.fuse(before, dump, mode)
        dry = a.fuse_from(other, T, mode=mode, dry=True)
        assert dry["summary"].tolist() == sm.tolist()
        same(a.export_blocks(raw=True), before, "fuse_from dry")
        res = a.fuse_from(other, T, mode=mode)
        assert res["summary"].tolist() == sm.tolist() and sm[4] > 0
        same(a.export_blocks(raw=True), want, f"fuse_from {mode}")
    a.close(), other.close()
