"""mlm_delta_blocks on the GPU: crafted maps of every block geometry (imported, never the workload's own), a first call, the map changed
through the public calls — one log-odds bit, one occ byte, one infl byte, a block imported, a block cropped away — and the next call
byte for byte against the contract in numpy (tests/delta_ref.py), in its order; host and device memory per pointer, unaligned device
destinations, every output left out in turn, MLM_DELTA_DRY; two schedules of the digest kernel; the refused calls; frontier mode; a
replica that follows a map through integration, set-free, inflation, aging and a crop."""
import ctypes

import numpy as np
import pytest

from tests import delta_ref as ref
from tests.test_gpu_fuse import frames
from tests.test_gpu_warp import craft, empty, load, small_cfg

pytestmark = pytest.mark.gpu
PLANES = ("keys", "log_odds", "occ", "infl")
OUTS = ("table_keys", "table_digest", "keys", "log_odds", "occ", "infl", "kind", "gone")
DTYPES = {"table_keys": np.int32, "table_digest": np.uint64, "keys": np.int32, "log_odds": np.float32, "occ": np.uint8, "infl": np.uint8, "kind": np.uint8, "gone": np.int32}
BOX = ([-1, -2, -1], [3, 5, 4])


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap, MlmError

    return MLMap, MlmError


def cols(name, C):
    return {"table_keys": 3, "table_digest": 2, "keys": 3, "kind": 1, "gone": 3}.get(name, C)


def raw_call(gpu, prev=None, box=None, flags=0, caps=(0, 0, 0), outs=None, summary=True, n_prev=None):
    """the C call; prev: (keys, digest) as numpy arrays or device pointers (ints); outs: name -> numpy array, device pointer or None"""
    keep = []

    def vp(a, dt=None):
        if a is None:
            return None
        if isinstance(a, int):
            return ctypes.c_void_p(a)
        arr = a if dt is None else np.ascontiguousarray(a, dtype=dt)
        keep.append(arr)
        return arr.ctypes.data_as(ctypes.c_void_p)
    outs = outs or {}
    lo_a, dims_a = (None, None) if box is None else (None if box[0] is None else np.asarray(box[0], dtype=np.int32), None if box[1] is None else np.asarray(box[1], dtype=np.int32))
    if n_prev is None:
        n_prev = 0 if prev is None else len(prev[0]) if not isinstance(prev[0], int) else prev[2]
    pk, pd = (None, None) if prev is None else (vp(prev[0], np.int32), vp(prev[1], np.uint64))
    sm = np.full(ref.ROW, -9, dtype=np.int64)
    o = [vp(outs.get(k)) for k in OUTS]
    rc = gpu._L.mlm_delta_blocks(gpu._h, vp(lo_a), vp(dims_a), n_prev, pk, pd, flags, caps[0], o[0], o[1], caps[1], o[2], o[3], o[4], o[5], o[6], caps[2], o[7],
                                 vp(sm) if summary else None)
    return rc, sm, gpu._L.mlm_last_error(gpu._h).decode()


def host_outs(caps, C, skip=()):
    rows = {"table_keys": caps[0], "table_digest": caps[0], "gone": caps[2]}
    return {k: np.full((rows.get(k, caps[1]), cols(k, C) * np.dtype(DTYPES[k]).itemsize), 7, dtype=np.uint8).view(DTYPES[k]) for k in OUTS if k not in skip}


def check(got, want, what, names=OUTS):
    """got: name -> array with at least the contract's rows; the rows beyond them untouched (every byte 7)"""
    for k in names:
        w = np.ascontiguousarray(want["table"][0] if k == "table_keys" else want["table"][1] if k == "table_digest" else want[k])
        g = np.ascontiguousarray(got[k])
        assert len(g) >= len(w) and g[:len(w)].tobytes() == w.tobytes(), f"{what}: {k}"
        assert (g[len(w):].view(np.uint8) == 7).all(), f"{what}: {k} beyond its rows"


def check_delta(d, want, what):
    """a Delta of the binding against the contract"""
    got = {"table_keys": d.table[0], "table_digest": d.table[1], **{k: getattr(d, k) for k in OUTS[2:]}}
    got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    got["table_digest"] = got["table_digest"].view(np.uint64)
    for k in OUTS:
        w = want["table"][0] if k == "table_keys" else want["table"][1] if k == "table_digest" else want[k]
        assert len(got[k]) == len(w), f"{what}: rows of {k}"
    check(got, want, what)
    assert d.summary.tolist() == want["summary"].tolist(), (what, d.summary.tolist(), want["summary"].tolist())


def change(gpu, rng, n):
    """the five changes through the public calls, as far as the map has blocks for them; returns how many of each kind were made"""
    e = gpu.export_blocks(raw=True)
    nb, C = len(e["keys"]), n ** 3
    pick = rng.permutation(nb)[:4]
    made = {"changed": 0, "new": 1, "gone": 0}
    rows = {k: e[k][pick[:3]].copy() for k in PLANES}
    for j in range(min(3, len(pick))):
        c = int(rng.integers(C))
        if j == 0:
            rows["log_odds"].view(np.uint32)[j, c] ^= np.uint32(1) << np.uint32(rng.integers(32))
        elif j == 1:
            rows["occ"][j, c] = ref.O if rows["occ"][j, c] != ref.O else ref.F
        else:
            rows["infl"][j, c] = ref.O if rows["infl"][j, c] != ref.O else ref.U
        made["changed"] += 1
    if len(pick):
        gpu.import_blocks(rows["keys"], rows["log_odds"], rows["occ"], rows["infl"])
    fresh = craft(rng, n, 1)
    fresh["keys"][:] = [77, -77, 7]
    gpu.import_blocks(fresh["keys"], fresh["log_odds"], fresh["occ"], fresh["infl"])
    if len(pick) == 4:
        gpu.crop_blocks(e["keys"][pick[3]], [1, 1, 1], inside=True)
        made["gone"] = 1
    return made


@pytest.mark.parametrize("n", [2, 3, 4, 7, 8, 16])
def test_crafted_maps(mods, knobs, n):
    """one handle per geometry, created with room for 64 blocks.  Host outputs of the emitted blocks are staged in rounds of 50 blocks."""
    import torch

    MLMap, _ = mods
    knobs.set("crop_stage_rows", 50)
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(6000 + n)
    C = n ** 3
    for count in (0, 1, 65, 300):
        what = f"n {n} count {count}"
        empty(gpu)
        if count:
            load(gpu, craft(rng, n, count))
        before = gpu.export_blocks(raw=True)
        want0 = ref.delta(before)
        d0 = gpu.delta()
        check_delta(d0, want0, what + " first")
        assert d0.summary[6] == count == d0.summary[1] and not d0.summary[[4, 5, 7]].any()
        # nothing in between: nothing changed, new or gone, and the same table again
        d_same = gpu.delta(prev=d0)
        assert d_same.summary[4] == count and not d_same.summary[5:9].any() and d_same.table[1].tobytes() == d0.table[1].tobytes(), what
        made = change(gpu, rng, n)
        after = gpu.export_blocks(raw=True)
        same_map = {k: after[k].copy() for k in PLANES}
        want = ref.delta(after, d0.table)
        sm = want["summary"]
        assert (sm[5], sm[6], sm[7]) == (made["changed"], made["new"], made["gone"]), (what, sm.tolist(), made)
        check_delta(gpu.delta(prev=d0), want, what + " host")
        check_delta(gpu.delta(prev=(torch.from_numpy(d0.table[0]).cuda(), torch.from_numpy(d0.table[1].view(np.int64)).cuda()), device=True), want, what + " device")
        for box, no_infl in ((BOX, False), (None, True), (BOX, True)):
            prev = ref.delta(before, None, None, None, no_infl)["table"]
            w = ref.delta(after, prev, *(box or (None, None)), no_infl)
            check_delta(gpu.delta(prev=prev, box=box, no_infl=no_infl), w, f"{what} box {box} no_infl {no_infl}")
        if count == 65:
            per_pointer(gpu, d0.table, want, C, what)
        for k in PLANES:
            assert gpu.export_blocks(raw=True)[k].tobytes() == same_map[k].tobytes(), what + ": the call only reads"
    gpu.close()


def per_pointer(gpu, prev, want, C, what):
    """host and device memory per pointer, unaligned device destinations, every output left out in turn, the dry call"""
    import torch

    sm = want["summary"]
    S, E, G = int(sm[1]), int(sm[5] + sm[6]), int(sm[7])
    caps = (S + 1, E + 1, G + 1)
    d_prev = (torch.from_numpy(np.ascontiguousarray(prev[0])).cuda(), torch.from_numpy(np.ascontiguousarray(prev[1]).view(np.int64)).cuda())

    def device_out(name, offset):
        """a device array of the output's cap, every byte 7; offset: it starts one element into its allocation"""
        rows = caps[0] if name.startswith("table") else caps[2] if name == "gone" else caps[1]
        count, dt = rows * cols(name, C), np.dtype(DTYPES[name])
        t = torch.full(((count + 1) * dt.itemsize,), 7, dtype=torch.uint8, device="cuda")
        o = dt.itemsize if offset and name in ("log_odds", "occ", "infl", "kind") else 0
        return t, t.data_ptr() + o, o, count * dt.itemsize, rows

    torch.cuda.synchronize()
    for variant in range(3):  # 0: everything on the device, planes unaligned; 1: the table in, host out; 2: host in, host and device alternating
        outs, dev = {}, {}
        host = host_outs(caps, C)
        for i, k in enumerate(OUTS):
            if variant == 0 or (variant == 2 and i % 2 == 0):
                dev[k] = device_out(k, offset=variant == 0)
                outs[k] = dev[k][1]
            else:
                outs[k] = host[k]
        torch.cuda.synchronize()
        p = prev if variant == 2 else (d_prev[0].data_ptr(), d_prev[1].data_ptr(), len(prev[0]))
        rc, got_sm, err = raw_call(gpu, p, None, 0, caps, outs)
        assert rc == 0, err
        torch.cuda.synchronize()
        got = {k: (dev[k][0].cpu().numpy()[dev[k][2]:dev[k][2] + dev[k][3]].copy().view(DTYPES[k]).reshape(dev[k][4], -1) if k in dev else host[k]) for k in OUTS}
        check(got, want, f"{what} variant {variant}")
        for k in dev:  # the bytes in front of an offset output stay
            assert (dev[k][0].cpu().numpy()[:dev[k][2]] == 7).all()
        assert got_sm.tolist() == sm.tolist(), (what, variant)
    for skip in OUTS:  # every output left out in turn; no summary once
        host = host_outs(caps, C, skip=(skip,))
        rc, got_sm, err = raw_call(gpu, prev, None, 0, caps, host, summary=skip != "kind")
        assert rc == 0, err
        check(host, want, f"{what} without {skip}", names=[k for k in OUTS if k != skip])
    # the caps of outputs that are not given do not count
    rc, got_sm, err = raw_call(gpu, prev, None, 0, (0, 0, 0), {})
    assert rc == 0 and got_sm[:8].tolist() == sm[:8].tolist() and not got_sm[8:11].any(), err
    # dry: the counts and nothing else
    host = host_outs(caps, C)
    rc, got_sm, err = raw_call(gpu, prev, None, ref.DRY, caps, host)
    assert rc == 0 and got_sm[:8].tolist() == sm[:8].tolist() and not got_sm[8:11].any() and got_sm[11] == sm[11], err
    assert all((v.view(np.uint8) == 7).all() for v in host.values())


@pytest.mark.parametrize("n", [3, 8])
def test_two_schedules_give_the_same_bytes(mods, knobs, n):
    """the digest kernel under its default grid cap and with one workgroup (knob delta_grid): more than a thousand blocks per wave"""
    MLMap, _ = mods
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(6100 + n)
    load(gpu, craft(rng, n, 300))
    a0 = gpu.delta()
    change(gpu, rng, n)
    a1 = gpu.delta(prev=a0, box=BOX)
    knobs.set("delta_grid", 1)
    b1 = gpu.delta(prev=a0, box=BOX)
    for x, y in zip((a1.table[0], a1.table[1], a1.keys, a1.log_odds, a1.occ, a1.infl, a1.kind, a1.gone, a1.summary),
                    (b1.table[0], b1.table[1], b1.keys, b1.log_odds, b1.occ, b1.infl, b1.kind, b1.gone, b1.summary)):
        assert x.tobytes() == y.tobytes()
    assert gpu.delta().table[1].tobytes() == ref.delta(gpu.export_blocks(raw=True))["table"][1].tobytes()
    gpu.close()


def test_refused_calls_leave_everything_untouched(mods):
    MLMap, MlmError = mods
    n, C = 4, 64
    gpu = MLMap(small_cfg(n), max_blocks=64)
    rng = np.random.default_rng(6200)
    load(gpu, craft(rng, n, 65))
    d0 = gpu.delta()
    change(gpu, rng, n)
    before = gpu.export_blocks(raw=True)
    prev = d0.table
    want = ref.delta(before, prev)
    sm = want["summary"]
    S, E, G = int(sm[1]), int(sm[5] + sm[6]), int(sm[7])
    assert E == 4 and G == 1
    lo, dims = BOX
    big = 1 << 20
    out_of_range = (np.concatenate([prev[0], [[big, 0, 0]]]).astype(np.int32), np.concatenate([prev[1], [[1, 2]]]).astype(np.uint64))
    swapped = (prev[0][::-1].copy(), prev[1][::-1].copy())
    twice = (np.concatenate([prev[0][:1], prev[0]]), np.concatenate([prev[1][:1], prev[1]]))
    full = (S, E, G)
    bad = [(dict(box=(lo, None)), 1), (dict(box=(None, dims)), 1), (dict(box=(lo, [1, 0, 1])), 2), (dict(box=([0, (1 << 31) - 2, 0], [1, 2, 1])), 3), (dict(flags=4), 4),
           (dict(flags=-1), 4), (dict(caps=(-1, E, G)), 5), (dict(caps=(S, -1, G)), 5), (dict(caps=(S, E, -1)), 5), (dict(n_prev=-1), 5), (dict(prev=None, n_prev=3), 6),
           (dict(prev=out_of_range), 7), (dict(prev=swapped), 8), (dict(prev=twice), 8)]
    for case, code in bad:
        for extra in (0, ref.DRY):
            kw = dict(prev=prev, caps=full)
            kw.update(case)
            kw["flags"] = kw.get("flags", 0) | extra
            host = host_outs((S + 1, E + 1, G + 2), C)
            rc, got_sm, err = raw_call(gpu, outs=host, **kw)
            assert rc == ref.ERR_INVALID and err == "mlm_delta_blocks: " + ref.TEXTS[code], (case, err)
            assert all((v.view(np.uint8) == 7).all() for v in host.values()) and (got_sm == -9).all(), case
    for caps in ((S - 1, E, G), (S, E - 1, G), (S, E, G - 1)):
        host = host_outs((S + 1, E + 1, G + 1), C)
        rc, got_sm, err = raw_call(gpu, prev, None, 0, caps, host)
        assert rc == ref.ERR_CAPACITY and "would be written, the outputs hold" in err, (caps, err)
        assert all((v.view(np.uint8) == 7).all() for v in host.values()), caps
        assert got_sm[:8].tolist() == sm[:8].tolist() and not got_sm[8:11].any() and got_sm[11] == sm[11], caps
    after = gpu.export_blocks(raw=True)
    for k in PLANES:
        assert after[k].tobytes() == before[k].tobytes()
    with pytest.raises(MlmError) as e:
        gpu.delta(prev=swapped)
    assert "MLM_ERR_INVALID" in str(e.value) and "ascending" in str(e.value)
    check_delta(gpu.delta(prev=prev), want, "the next valid call")
    gpu.close()


@pytest.mark.parametrize("n", [3, 4])
def test_frontier_mode(mods, n):
    """the call succeeds on a frontier-mode handle; a released block's digest and emitted planes are those of its expanded view"""
    MLMap, _ = mods
    gpu = MLMap(small_cfg(n, explore=True), max_blocks=64)
    m = craft(np.random.default_rng(6300 + n), n, 65, True)
    load(gpu, m)
    before = gpu.export_blocks(raw=True)
    assert before["collapsed"].sum() > 3
    want = ref.delta(before)
    d0 = gpu.delta()
    check_delta(d0, want, f"frontier n {n}")
    col = before["collapsed"][ref.order(before["keys"])].astype(bool)
    assert (d0.infl[col] == ref.U).all() and (d0.log_odds[col] == d0.log_odds[col][:, :1]).all() and (d0.occ[col] == d0.occ[col][:, :1]).all()
    flat = {k: v.copy() for k, v in before.items()}
    flat["log_odds"], flat["occ"], flat["infl"] = ref.view(before)
    flat["collapsed"][:] = 0
    assert ref.delta(flat)["table"][1].tobytes() == d0.table[1].tobytes()
    check_delta(gpu.delta(prev=d0, box=BOX, no_infl=False), ref.delta(before, d0.table, *BOX), f"frontier n {n} again")
    after = gpu.export_blocks(raw=True)
    assert all(after[k].tobytes() == before[k].tobytes() for k in PLANES) and np.array_equal(after["collapsed"], before["collapsed"])
    gpu.close()


def test_replica_round_trip(mods):
    """B follows A by deltas alone through integration, set-free, inflation, an aging that forgets and drops, and a crop"""
    MLMap, _ = mods
    n = 4
    cfg = small_cfg(n)
    a, b = MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64)
    d_glb = n * cfg.subbox_d_xyz
    prev, fewer, gone, steps = None, 0, 0, 0

    def follow(what):
        nonlocal prev, fewer, gone, steps
        d = a.delta(prev=prev, device=steps % 2 == 1)
        b.apply_delta(d)
        prev = d
        ea, eb = a.export_blocks(), b.export_blocks()
        for k in PLANES:
            assert ea[k].tobytes() == eb[k].tobytes(), f"{what}: {k}"
        assert d.summary[8] == d.summary[5] + d.summary[6] and d.summary[1] == len(ea["keys"])
        fewer += int(0 < d.summary[8] < d.summary[1])
        gone += int(d.summary[7])
        steps += 1

    for k, (img, q, t) in enumerate(frames(cfg, 5, 6)):
        a.update_map(img, q, t)
        follow(f"frame {k}")
        if k == 1:
            held = a.export_blocks()["keys"]
            lo = held[len(held) // 2].astype(np.float64) * d_glb + 0.1 * d_glb
            a.setFree_map_in_bound(lo, lo + 0.5 * d_glb)
            follow("set free")
        elif k == 2:
            a.inflate_map(t)
            follow("inflate")
        elif k == 3:
            a.age_blocks(mode="step", amount=0.6, forget=0.7, drop=True)
            follow("age")
        elif k == 4:
            ctr = np.floor(t / d_glb).astype(np.int64)
            a.crop_blocks(ctr - 2, [5, 5, 5])
            follow("crop")
    assert fewer >= 1 and gone >= 1 and steps == 10, (fewer, gone, steps)
    a.close(), b.close()
