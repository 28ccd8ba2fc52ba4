"""mlm_age_blocks on the GPU: crafted maps of every block geometry (imported, never the workload's own) aged in both modes, over a key
box, outside it and with no box, with MLM_AGE_FORGET, MLM_AGE_DROP and MLM_AGE_CLEAR_INFL alone and together, summary and per_block
given and left out, per_block in host and in device memory — the dry call first, then the wet one, byte for byte in raw slot order against
the contract in numpy (tests/age_ref.py); MLM_AGE_DROP against a twin that drops by the definition, with integration on both sides;
the refused calls; frontier mode; zero blocks; the host mirror; age_outside."""
import ctypes

import numpy as np
import pytest

from tests import age_ref as ref
from tests import crop_ref
from tests.test_age_plan import AMOUNT, BOX, FORGET, cube_keys, wild
from tests.test_gpu_fuse import frames
from tests.test_gpu_warp import empty, small_cfg

pytestmark = pytest.mark.gpu
PLANES = ("keys", "log_odds", "occ", "infl")


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap, MlmError

    return MLMap, MlmError


def same(a, b, what):
    for k in PLANES:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {k}"


def load(gpu, b):
    if len(b["keys"]):
        gpu.import_blocks(b["keys"], b["log_odds"], b["occ"], b["infl"])


def raw_call(gpu, key_lo, key_dims, mode, amount, forget, flags, per_block, summary):
    vp = lambda a: None if a is None else ctypes.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(ctypes.c_void_p)
    lo_a = None if key_lo is None else np.asarray(key_lo, dtype=np.int32)
    dims_a = None if key_dims is None else np.asarray(key_dims, dtype=np.int32)
    rc = gpu._L.mlm_age_blocks(gpu._h, vp(lo_a), vp(dims_a), mode, float(amount), float(forget), flags, vp(per_block), vp(summary))
    return rc, gpu._L.mlm_last_error(gpu._h).decode()


# (mode, box, outside, forget, drop, clear_infl): both modes; box / OUTSIDE / no box; the three flags alone and together
CASES = [("scale", True, False, False, False, False), ("step", False, False, True, False, False), ("scale", True, True, False, True, False),
         ("step", True, False, False, False, True), ("scale", False, False, True, True, True), ("step", True, True, True, True, False),
         ("scale", True, False, True, True, True), ("step", False, False, False, True, False)]


@pytest.mark.parametrize("n", [2, 3, 4, 8, 16])
def test_crafted_maps(mods, n):
    """one handle per geometry.  Per block count and case: the dry call (map and mirror answers unchanged), then the wet one — through
    the binding with per_block in host memory, or raw with per_block in device memory or left out and the summary left out in turn"""
    import torch

    MLMap, _ = mods
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(4000 + n)
    C = n ** 3
    dropped = forgot = 0
    for count in [1, 65, 257] + ([4097] if n == 2 else []):  # (4 097: the 2 048-slot chunk of the prefix crossed twice)
        m = wild(rng, cube_keys(rng, count, bounds=False), C)
        probe = (m["keys"][:8].astype(np.float64) * n + 0.5) * 0.1
        for ci, (mode, box, outside, forget, drop, clear_infl) in enumerate(CASES if count != 4097 else CASES[4:7]):
            what = f"n {n} blocks {count} case {ci}"
            empty(gpu)
            load(gpu, m)
            before = gpu.export_blocks(raw=True)
            assert len(before["keys"]) == count
            kw = dict(key_lo=BOX[0] if box else None, key_dims=BOX[1] if box else None, mode=mode, amount=AMOUNT[ref.MODES[mode]], forget=FORGET if forget else None,
                      outside=outside, drop=drop, clear_infl=clear_infl)
            want, sm, pr = ref.age(before, **kw)
            odd0 = gpu.getOdd(probe)
            dry = gpu.age_blocks(dry=True, per_block=True, **kw)
            assert dry["summary"].tolist() == sm.tolist(), (what, dry["summary"].tolist(), sm.tolist())
            assert dry["per_block"].tolist() == pr.tolist(), what + " dry"
            assert gpu.block_count() == count and np.array_equal(gpu.getOdd(probe).view(np.uint32), odd0.view(np.uint32))
            same(gpu.export_blocks(raw=True), before, what + " dry")
            flags = (ref.OUTSIDE if outside else 0) | (ref.FORGET if forget else 0) | (ref.DROP if drop else 0) | (ref.CLEAR_INFL if clear_infl else 0)
            if ci % 3 == 0:  # the binding: summary and per_block in host memory
                res = gpu.age_blocks(per_block=True, **kw)
                assert res["summary"].tolist() == sm.tolist() and res["per_block"].tolist() == pr.tolist(), what
            elif ci % 3 == 1:  # per_block in device memory, no summary
                d_pb = torch.full((count, 4), -7, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                rc, err = raw_call(gpu, kw["key_lo"], kw["key_dims"], ref.MODES[mode], kw["amount"], FORGET, flags, d_pb.data_ptr(), None)
                assert rc == 0, err
                assert d_pb.cpu().numpy().tolist() == pr.tolist(), what
            else:  # the summary alone
                got_sm = np.full(ref.ROW, -9, dtype=np.int64)
                rc, err = raw_call(gpu, kw["key_lo"], kw["key_dims"], ref.MODES[mode], kw["amount"], FORGET, flags, None, got_sm)
                assert rc == 0, err
                assert got_sm.tolist() == sm.tolist(), what
            same(gpu.export_blocks(raw=True), want, what)
            st = gpu.frame_stats()
            assert gpu.block_count() == len(want["keys"]) == st["n_blocks"] == sm[3], what
            dropped += int(sm[2])
            forgot += int(sm[6])
    assert dropped > 0 and forgot > 0
    gpu.close()


@pytest.mark.parametrize("n", [4, 9])
def test_drop_is_the_definition_with_integration_on_both_sides(mods, n):
    """a twin drops by the definition: age without DROP, export, the empty selected blocks filtered in numpy, a crop of everything, import.
    Frames integrated into both before, between and afterwards give the same float bits"""
    MLMap, _ = mods
    cfg = small_cfg(n)
    a, b = MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64)
    fr = frames(cfg, 5, 6)
    total = 0
    for step in range(2):
        for img, q, t in fr[2 * step:2 * step + 2]:
            a.update_map(img, q, t), b.update_map(img, q, t)
        same(a.export_blocks(), b.export_blocks(), f"n {n} step {step} before")
        # mild everywhere first; then everything outside one block's box scaled to nothing: every block there empties out
        key0 = a.export_blocks()["keys"][0]
        kw = dict(mode="step", amount=0.3, forget=0.4) if step == 0 else dict(key_lo=key0, key_dims=[1, 1, 1], outside=True, mode="scale", amount=0.0, forget=0.0)
        nb0 = a.block_count()
        res = a.age_blocks(drop=True, per_block=True, **kw)
        b.age_blocks(**kw)
        e = b.export_blocks(raw=True)
        sel = ref.selected(e["keys"], kw.get("key_lo"), kw.get("key_dims"), kw.get("outside", False))
        keep = ~(sel & ref.empty_blocks(e))
        empty(b)
        if keep.any():
            b.import_blocks(e["keys"][keep], e["log_odds"][keep], e["occ"][keep], e["infl"][keep])
        sm = res["summary"]
        assert sm[0] == nb0 and sm[2] == int((~keep).sum()) == int((res["per_block"][:, 3] == 2).sum()) and sm[3] == a.block_count() == b.block_count()
        same(a.export_blocks(), b.export_blocks(), f"n {n} step {step} aged")
        total += int(sm[2])
        if step == 1:
            assert sm[2] == nb0 - 1 and a.block_count() == 1
    for img, q, t in fr[4:6]:
        a.update_map(img, q, t), b.update_map(img, q, t)
    ea = a.export_blocks()
    same(ea, b.export_blocks(), f"n {n} after")
    assert a.block_count() == len(ea["keys"]) == a.frame_stats()["n_blocks"] and total > 0
    a.close(), b.close()


def test_refused_calls_leave_the_map_untouched(mods):
    MLMap, MlmError = mods
    n = 4
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(4200)
    m = wild(rng, cube_keys(rng, 65, bounds=False), n ** 3)
    load(gpu, m)
    before = gpu.export_blocks(raw=True)
    lo, dims = BOX
    bad = [((lo, None, 0, 0.5, 0.0, 0), 1), ((None, dims, 0, 0.5, 0.0, 0), 1), ((lo, [1, 0, 1], 0, 0.5, 0.0, 0), 2), (([0, (1 << 31) - 2, 0], [1, 2, 1], 0, 0.5, 0.0, 0), 3),
           ((lo, dims, 0, 0.5, 0.0, 32), 4), ((lo, dims, 2, 0.5, 0.0, 0), 5), ((lo, dims, -1, 0.5, 0.0, 0), 5), ((lo, dims, 0, np.nan, 0.0, 0), 6),
           ((lo, dims, 1, np.inf, 0.0, 0), 6), ((lo, dims, 0, 1.5, 0.0, 0), 7), ((lo, dims, 0, -0.5, 0.0, 0), 7), ((lo, dims, 1, -0.5, 0.0, 0), 8),
           ((lo, dims, 0, 0.5, -1.0, ref.FORGET), 9), ((lo, dims, 0, 0.5, np.nan, ref.FORGET | ref.DROP), 9), ((None, None, 1, 0.5, np.inf, ref.FORGET), 9)]
    for args, code in bad:
        for extra in (0, ref.DRY):
            sm = np.full(ref.ROW, -9, dtype=np.int64)
            rc, err = raw_call(gpu, *args[:5], args[5] | extra, None, sm)
            assert rc == ref.ERR_INVALID and err == "mlm_age_blocks: " + ref.TEXTS[code], (args, err)
            assert ref.check_args(args[0], args[1], args[2], args[3], args[4], args[5] | extra) == code
        same(gpu.export_blocks(raw=True), before, str(args))
        assert gpu.block_count() == 65
    with pytest.raises(MlmError) as e:
        gpu.age_blocks(lo, dims, mode="scale", amount=2.0)
    assert "MLM_ERR_INVALID" in str(e.value) and "[0, 1]" in str(e.value)
    # without MLM_AGE_FORGET forget is ignored, whatever it is; and the next valid call works
    want, sm, pr = ref.age(before, lo, dims, mode=ref.STEP, amount=0.375)
    got = np.zeros(ref.ROW, dtype=np.int64)
    rc, err = raw_call(gpu, lo, dims, ref.STEP, 0.375, np.nan, 0, None, got)
    assert rc == 0 and got.tolist() == sm.tolist(), err
    same(gpu.export_blocks(raw=True), want, "the next valid call")
    gpu.close()


@pytest.mark.parametrize("n", [3, 4])
def test_frontier_mode_is_refused(mods, n):
    from tests.test_gpu_warp import craft
    from tests.test_gpu_warp import load as load_flags

    MLMap, MlmError = mods
    gpu = MLMap(small_cfg(n, explore=True), max_blocks=64)
    m = craft(np.random.default_rng(4300 + n), n, 65, True)
    load_flags(gpu, m)
    before = gpu.export_blocks(raw=True)
    for dry in (False, True):
        with pytest.raises(MlmError) as e:
            gpu.age_blocks(mode="scale", amount=0.5, forget=0.1, drop=True, dry=dry)
        assert "MLM_ERR_INVALID" in str(e.value) and "frontier" in str(e.value)
    after = gpu.export_blocks(raw=True)
    same(after, before, "frontier")
    assert np.array_equal(after["collapsed"], before["collapsed"])
    gpu.close()


def test_zero_blocks(mods):
    MLMap, _ = mods
    gpu = MLMap(small_cfg(4), max_blocks=64)
    for kw in (dict(), dict(dry=True), dict(key_lo=BOX[0], key_dims=BOX[1], outside=True)):
        res = gpu.age_blocks(mode="step", amount=0.5, forget=0.1, drop=True, per_block=True, **kw)
        assert not res["summary"].any() and res["per_block"].shape == (0, 4)
    sm = np.full(ref.ROW, -9, dtype=np.int64)
    rc, err = raw_call(gpu, None, None, 0, 0.5, 0.0, ref.DROP, None, sm)
    assert rc == 0 and not sm.any() and gpu.block_count() == 0
    gpu.close()


def test_host_mirror_follows_an_aging(mods):
    """small host batches are answered from the host mirror: after a wet call that drops blocks they answer from the new content"""
    MLMap, _ = mods
    n, d = 4, 0.1
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(4400)
    m = wild(rng, cube_keys(rng, 40, bounds=False), n ** 3)
    load(gpu, m)
    r, c = np.nonzero(m["occ"] != ref.U)
    pick = rng.permutation(len(r))[:48]
    r, c = r[pick], c[pick]
    cell = np.stack([c % n, (c // n) % n, c // (n * n)], axis=1)
    pos = (m["keys"][r].astype(np.float64) * n + cell + 0.5) * d

    def classes(b):
        at = {tuple(k): i for i, k in enumerate(b["keys"].tolist())}
        occ = np.array([b["occ"][at[tuple(k)], ci] if tuple(k) in at else ref.U for k, ci in zip(m["keys"][r].tolist(), c)])
        return np.where(occ == ref.O, MLMap.OCCUPIED, np.where(occ == ref.F, MLMap.FREE, MLMap.UNKNOWN))

    before = gpu.export_blocks(raw=True)
    odd0 = gpu.getOdd(pos)
    assert np.array_equal(gpu.getOccupancy(pos), classes(before))
    kw = dict(mode="scale", amount=0.5, forget=FORGET, drop=True)
    want, sm, _ = ref.age(before, **kw)
    res = gpu.age_blocks(**kw)
    assert res["summary"].tolist() == sm.tolist() and sm[2] > 0 and sm[6] > 0
    twin = MLMap(small_cfg(n), max_blocks=128)  # the same queries of a handle that was given the aged map whole
    load(twin, want)
    odd1 = gpu.getOdd(pos)
    assert (odd1 != odd0).sum() > 20
    assert np.array_equal(odd1.view(np.uint32), twin.getOdd(pos).view(np.uint32)) and np.array_equal(gpu.getOccupancy(pos), classes(want))
    assert (classes(want) != classes(before)).any()
    twin.close()
    gpu.close()


def test_age_outside_is_age_blocks_with_retain_arounds_box(mods):
    MLMap, _ = mods
    n = 4
    cfg = small_cfg(n)
    gpu = MLMap(cfg, max_blocks=64)
    rng = np.random.default_rng(4500)
    m = wild(rng, cube_keys(rng, 257, bounds=False), n ** 3)
    load(gpu, m)
    before = gpu.export_blocks(raw=True)
    t, radius = np.array([0.13, -0.21, 0.3]), 0.55
    lo, dims = crop_ref.retain_box(t, radius, n * cfg.subbox_d_xyz)
    got_lo, got_dims = gpu.retain_box(t, radius)
    assert np.array_equal(got_lo, lo) and np.array_equal(got_dims, dims)
    want, sm, pr = ref.age(before, lo, dims, mode=ref.STEP, amount=0.375, forget=FORGET, outside=True, drop=True)
    res = gpu.age_outside(t, radius, mode="step", amount=0.375, forget=FORGET, drop=True, per_block=True)
    assert res["summary"].tolist() == sm.tolist() and res["per_block"].tolist() == pr.tolist() and 0 < sm[1] < 257 and sm[2] > 0
    same(gpu.export_blocks(raw=True), want, "age_outside")
    kept = gpu.retain_around(t, radius)["summary"]  # (retain_around still crops by the same box)
    assert kept[1] == int((~crop_ref.drops(want["keys"], lo, dims, inside=False)).sum())
    gpu.close()
