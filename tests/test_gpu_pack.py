"""mlm_pack_blocks / mlm_unpack_blocks on the GPU: crafted maps of every block geometry (imported, never the workload's own) — fewer
cells than a wave has lanes (8, 27), exactly one word (64), a ragged last word (343), many steps (4096) — packed from the live map and
from rows, byte for byte against the contract in numpy (tests/pack_ref.py); host and device memory per pointer, host staging in rounds
of 50 rows, two schedules, the refused calls, crafted corrupt streams inside a buffer with slack, frontier mode, and save / load and a
replica that follows by packed deltas."""
import ctypes
import struct

import numpy as np
import pytest

from tests import delta_ref
from tests import pack_ref as ref
from tests.test_gpu_fuse import frames
from tests.test_gpu_warp import craft, empty, load, small_cfg

pytestmark = pytest.mark.gpu
PLANES = ("keys", "log_odds", "occ", "infl")
DTYPES = {"keys": np.int32, "log_odds": np.float32, "occ": np.uint8, "infl": np.uint8}
BOX = ([-1, -2, -1], [3, 5, 4])


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap, MlmError

    return MLMap, MlmError


def clamps(cfg):
    return np.float32(cfg.lm_log_odds_min), np.float32(cfg.lm_log_odds_max)


def regular(rng, n, count, cfg, explore=False):
    """craft's blocks made as regular as a real map: voxels on the clamps, unseen voxels, blank blocks, a block blank but for a -0.0f"""
    b = craft(rng, n, count, explore)
    lo_min, lo_max = clamps(cfg)
    pick = rng.integers(0, 6, size=b["log_odds"].shape)
    b["log_odds"][pick == 1], b["log_odds"][pick == 2], b["log_odds"][pick >= 4] = lo_min, lo_max, 0.0
    blank = rng.random(count) < 0.2
    b["log_odds"][blank], b["occ"][blank], b["infl"][blank] = 0.0, ref.U, ref.U
    if count > 2:
        b["log_odds"][1], b["occ"][1], b["infl"][1] = 0.0, ref.U, ref.U
        b["log_odds"][1, -1] = -0.0
    return b


def vp(a):
    return None if a is None else ctypes.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(ctypes.c_void_p)


def raw_pack(gpu, box=None, rows=None, n=0, flags=0, cap=0, stream=None):
    """the C call; rows: four numpy arrays / device pointers / None; stream: numpy array or device pointer"""
    lo_a, dims_a = (None, None) if box is None else (None if box[0] is None else np.asarray(box[0], dtype=np.int32), None if box[1] is None else np.asarray(box[1], dtype=np.int32))
    src = (None,) * 4 if rows is None else rows
    sm = np.full(ref.ROW, -9, dtype=np.int64)
    rc = gpu._L.mlm_pack_blocks(gpu._h, vp(lo_a), vp(dims_a), n, *[vp(a) for a in src], flags, cap, vp(stream), vp(sm))
    return rc, sm, gpu._L.mlm_last_error(gpu._h).decode()


def raw_unpack(gpu, stream, nbytes, cap, outs, flags=0):
    sm = np.full(ref.ROW, -9, dtype=np.int64)
    rc = gpu._L.mlm_unpack_blocks(gpu._h, vp(stream), nbytes, flags, cap, *[vp(outs.get(k)) for k in PLANES], vp(sm))
    return rc, sm, gpu._L.mlm_last_error(gpu._h).decode()


def sorted_view(e, no_infl=False):
    """the rows a stream of the whole map decodes to"""
    lo, occ, infl = delta_ref.view(e, no_infl)
    o = delta_ref.order(e["keys"])
    return {"keys": e["keys"][o], "log_odds": lo[o], "occ": occ[o], "infl": infl[o]}


def same_rows(got, want, what):
    for k in PLANES:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        assert g.shape == want[k].shape and g.tobytes() == np.ascontiguousarray(want[k]).tobytes(), f"{what}: {k}"


@pytest.mark.parametrize("n", [2, 3, 4, 7, 8, 16])
def test_crafted_maps(mods, knobs, n):
    """one handle per geometry, created with room for 64 blocks; host rows and host outputs are staged in rounds of 50 blocks"""
    import torch

    MLMap, _ = mods
    knobs.set("crop_stage_rows", 50)
    cfg = small_cfg(n)
    lo_min, lo_max = clamps(cfg)
    gpu = MLMap(cfg, max_blocks=64)
    rng = np.random.default_rng(7000 + n)
    C = n ** 3
    for count in (0, 1, 65, 300):
        what = f"n {n} count {count}"
        empty(gpu)
        if count:
            load(gpu, regular(rng, n, count, cfg))
        e = gpu.export_blocks(raw=True)
        want = ref.pack_map(e, n, lo_min, lo_max)
        s = gpu.pack()
        assert s.tobytes() == want["stream"], what
        assert gpu.pack_summary.tolist() == want["summary"].tolist(), (what, gpu.pack_summary.tolist(), want["summary"].tolist())
        total = len(want["stream"])
        assert gpu.pack(device=True).cpu().numpy().tobytes() == want["stream"], what + " device"
        for box, no_infl in ((BOX, False), (None, True), (BOX, True)):
            w = ref.pack_map(e, n, lo_min, lo_max, *(box or (None, None)), no_infl)
            assert gpu.pack(box=box, no_infl=no_infl).tobytes() == w["stream"], f"{what} box {box} no_infl {no_infl}"
            assert gpu.pack_summary.tolist() == w["summary"].tolist()
        # the rows source, in the pool's order: host memory, device memory, alternating per pointer, infl left out
        rows = [np.ascontiguousarray(e[k]) for k in PLANES]
        wr = ref.pack_rows(*rows, n, lo_min, lo_max)
        dev = [torch.from_numpy(a).cuda() for a in rows]
        assert gpu.pack(rows=rows).tobytes() == wr["stream"], what + " host rows"
        assert gpu.pack(rows=dev, device=True).cpu().numpy().tobytes() == wr["stream"], what + " device rows"
        assert gpu.pack(rows=(dev[0], rows[1], dev[2], rows[3])).tobytes() == wr["stream"] == gpu.pack(rows=(rows[0], dev[1], rows[2], dev[3])).tobytes(), what + " mixed"
        assert gpu.pack(rows=(rows[0], dev[1], rows[2], None)).tobytes() == ref.pack_rows(rows[0], rows[1], rows[2], None, n, lo_min, lo_max)["stream"], what + " no infl plane"
        assert gpu.pack(rows=rows, no_infl=True).tobytes() == ref.pack_rows(*rows, n, lo_min, lo_max, True)["stream"]
        # bytes beyond summary[7] stay untouched, in host and in device memory
        host = np.full(total + 64, 7, dtype=np.uint8)
        rc, sm, err = raw_pack(gpu, cap=len(host), stream=host)
        assert rc == 0 and sm[7] == total and host[:total].tobytes() == want["stream"] and (host[total:] == 7).all(), (what, err)
        d = torch.full((total + 64,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc, sm, err = raw_pack(gpu, cap=total + 64, stream=d.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0 and sm.tolist() == want["summary"].tolist() and d.cpu().numpy()[:total].tobytes() == want["stream"] and (d.cpu().numpy()[total:] == 7).all(), (what, err)
        # unpack: host and device outputs, the summary, rows beyond n untouched, each output left out in turn
        rows_want = sorted_view(e)
        same_rows(gpu.unpack(s), rows_want, what + " unpack")
        same_rows(gpu.unpack(torch.from_numpy(s).cuda(), device=True), rows_want, what + " unpack device")
        assert gpu.unpack(s)["summary"].tolist() == ref.unpack(want["stream"], n)["summary"].tolist()
        if count == 65:
            for skip in (None,) + PLANES:
                outs = {k: np.full((count + 1, (3 if k == "keys" else C) * np.dtype(DTYPES[k]).itemsize), 7, dtype=np.uint8).view(DTYPES[k]) for k in PLANES if k != skip}
                rc, sm, err = raw_unpack(gpu, s, len(s), count + 1, outs)
                assert rc == 0, err
                for k in outs:
                    assert outs[k][:count].tobytes() == np.ascontiguousarray(rows_want[k]).tobytes() and (outs[k][count:].view(np.uint8) == 7).all(), (what, skip, k)
        after = gpu.export_blocks(raw=True)
        assert all(after[k].tobytes() == e[k].tobytes() for k in PLANES), what + ": the calls only read"
    gpu.close()


@pytest.mark.parametrize("n", [3, 8])
def test_two_schedules_give_the_same_bytes(mods, knobs, n):
    """the pack and unpack kernels under their default grid cap and with one workgroup (knob pack_grid): 75 rows per wave"""
    MLMap, _ = mods
    cfg = small_cfg(n)
    gpu = MLMap(cfg, max_blocks=64)
    load(gpu, regular(np.random.default_rng(7100 + n), n, 300, cfg))
    a, a_box = gpu.pack(), gpu.pack(box=BOX)
    ua = gpu.unpack(a)
    knobs.set("pack_grid", 1)
    b, b_box = gpu.pack(), gpu.pack(box=BOX)
    ub = gpu.unpack(a)
    assert a.tobytes() == b.tobytes() == ref.pack_map(gpu.export_blocks(raw=True), n, *clamps(cfg))["stream"] and a_box.tobytes() == b_box.tobytes()
    same_rows(ua, ub, "schedules")
    gpu.close()


def test_refused_calls_leave_everything_untouched(mods):
    import torch

    MLMap, MlmError = mods
    n, C = 4, 64
    cfg = small_cfg(n)
    gpu = MLMap(cfg, max_blocks=64)
    rng = np.random.default_rng(7200)
    load(gpu, regular(rng, n, 65, cfg))
    before = gpu.export_blocks(raw=True)
    want = ref.pack_map(before, n, *clamps(cfg))
    total = len(want["stream"])
    rows = [np.ascontiguousarray(before[k]) for k in PLANES]
    lo, dims = BOX
    d = torch.full((total + 16,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bad = [(dict(box=(lo, None)), 1), (dict(box=(None, dims)), 1), (dict(box=(lo, [1, 0, 1])), 2), (dict(box=([0, (1 << 31) - 2, 0], [1, 2, 1])), 3), (dict(flags=4), 4),
           (dict(flags=-1), 4), (dict(box=BOX, rows=rows, n=65), 5), (dict(rows=rows, n=-1), 6), (dict(rows=(rows[0], None, rows[2], rows[3]), n=65), 7),
           (dict(rows=(rows[0], rows[1], None, rows[3]), n=65), 7), (dict(stream=d.data_ptr() + 4), 8)]
    for case, code in bad:
        host = np.full(total + 8, 7, dtype=np.uint8)
        kw = dict(cap=total, stream=host)
        kw.update(case)
        rc, sm, err = raw_pack(gpu, **kw)
        assert rc == ref.ERR_INVALID and err == "mlm_pack_blocks: " + ref.PACK_TEXTS[code], (case, err)
        assert (host == 7).all() and (sm == -9).all(), case
    # a byte outside 'u' 'f' 'o': found on the device, the row named
    for plane, row in ((2, 40), (3, 7)):
        wrong = [a.copy() for a in rows]
        wrong[plane][row, C - 1] = ord("x")
        wrong[plane][60, 3] = 0
        host = np.full(total + 8, 7, dtype=np.uint8)
        rc, sm, err = raw_pack(gpu, rows=wrong, n=65, cap=total + 8, stream=host)
        assert rc == ref.ERR_INVALID and err == f"mlm_pack_blocks: {ref.PACK_TEXTS[9]} (row {row})", err
        assert (host == 7).all() and (sm == -9).all()
    # the capacity one byte short: the summary filled, nothing written
    for stream in (np.full(total + 8, 7, dtype=np.uint8), d.data_ptr()):
        rc, sm, err = raw_pack(gpu, cap=total - 1, stream=stream)
        assert rc == ref.ERR_CAPACITY and "would be written, the stream holds" in err and sm[:7].tolist() == want["summary"][:7].tolist() and sm[7] == 0, err
        torch.cuda.synchronize()
        assert ((stream if isinstance(stream, np.ndarray) else d.cpu().numpy()) == 7).all()
    # dry, and a null stream: the sizes only
    host = np.full(total + 8, 7, dtype=np.uint8)
    for kw in (dict(flags=ref.DRY, cap=total + 8, stream=host), dict(cap=0, stream=None)):
        rc, sm, err = raw_pack(gpu, **kw)
        assert rc == 0 and sm[:7].tolist() == want["summary"][:7].tolist() and sm[7] == 0 and (host == 7).all(), err
    # unpack: the arguments, the cap one short
    s = np.frombuffer(want["stream"], dtype=np.uint8).copy()
    ds = torch.zeros(total + 8, dtype=torch.uint8, device="cuda")
    ds[4:4 + total] = torch.from_numpy(s).cuda()
    torch.cuda.synchronize()
    outs = {k: np.full((66, 3 if k == "keys" else C), 7, dtype=DTYPES[k]) for k in PLANES}
    for kw, code in ((dict(stream=None), 11), (dict(flags=1), 12), (dict(cap=-1), 13), (dict(stream=ds.data_ptr() + 4), 14)):
        args = dict(stream=s, nbytes=total, cap=66, outs=outs)
        args.update(kw)
        rc, sm, err = raw_unpack(gpu, **args)
        assert rc == ref.ERR_INVALID and err == "mlm_unpack_blocks: " + ref.UNPACK_TEXTS[code] and (sm == -9).all(), (kw, err)
    rc, sm, err = raw_unpack(gpu, s, total, 64, outs)
    assert rc == ref.ERR_CAPACITY and sm[0] == 65 and sm[7] == 0, err
    assert all((v == 7).all() for v in outs.values())
    rc, sm, err = raw_unpack(gpu, s, total, 0, {})
    assert rc == 0 and sm[0] == 65 and sm[1] == total, err
    after = gpu.export_blocks(raw=True)
    assert all(after[k].tobytes() == before[k].tobytes() for k in PLANES)
    with pytest.raises(MlmError) as ei:
        gpu.unpack(s[:100])
    assert "MLM_ERR_INVALID" in str(ei.value) and "check 4" in str(ei.value)
    assert gpu.pack().tobytes() == want["stream"]
    gpu.close()


def test_corrupt_streams(mods):
    """bad magic, wrong C, total above bytes, n_lit off by one, an offset off by one, an occ code 3, a tail bit set — each in a buffer with
    one maximal record of slack, in host and in device memory: the reference's check number and block, nothing written"""
    import torch

    MLMap, _ = mods
    n, C = 3, 27
    cfg = small_cfg(n)
    gpu = MLMap(cfg, max_blocks=64)
    rng = np.random.default_rng(7300)
    m = regular(rng, n, 9, cfg)
    m["occ"][4] = np.frombuffer(b"ufo", dtype=np.uint8)[np.arange(C) % 3]  # block 4 has both occ planes and a free cell
    m["log_odds"][4] = np.linspace(0.1, 1.0, C, dtype=np.float32)
    rows = [np.ascontiguousarray(m[k]) for k in PLANES]
    s = ref.pack_rows(*rows, n, *clamps(cfg))["stream"]
    assert gpu.pack(rows=rows).tobytes() == s
    offs = [struct.unpack_from("<I", s, ref.HEADER + ref.DIR * i + 12)[0] for i in range(9)]
    pres, n_lit = struct.unpack_from("<II", s, 8 * offs[4])
    assert pres & 3 == 3 and n_lit == C
    occ0, occ1 = struct.unpack_from("<QQ", s, 8 * offs[4] + 8)
    slack = ref.record_bytes(ref.words(C), 63, C)

    def edit(at, fmt, *v):
        b = bytearray(s)
        struct.pack_into(fmt, b, at, *v)
        return bytes(b)
    cases = [("magic", edit(0, "<B", ord("m")), len(s)), ("C", edit(8, "<I", 64), len(s)), ("total", edit(32, "<Q", len(s) + 8), len(s)),
             ("n_lit", edit(8 * offs[4] + 4, "<I", C - 1), len(s)), ("offset", edit(ref.HEADER + ref.DIR * 5 + 12, "<I", offs[5] + 1), len(s)),
             ("code 3", edit(8 * offs[4] + 8, "<QQ", occ0 | 1, occ1 | 1), len(s)), ("tail", edit(8 * offs[4] + 16, "<Q", occ1 | 1 << 27), len(s))]
    expect = {"magic": (2, -1), "C": (3, -1), "total": (4, -1), "n_lit": (9, 4), "offset": (5, 5), "code 3": (8, 4), "tail": (7, 4)}
    for name, bad, nbytes in cases:
        want = ref.unpack(bad[:nbytes], n)
        assert (want["code"], want["block"]) == expect[name], (name, want)
        text = "mlm_unpack_blocks: " + ref.UNPACK_TEXTS[want["code"]] + (f" (block {want['block']})" if want["block"] >= 0 else "")
        padded = np.frombuffer(bad + b"\0" * slack, dtype=np.uint8).copy()
        dev = torch.from_numpy(padded).cuda()
        torch.cuda.synchronize()
        for stream in (padded, dev.data_ptr()):
            outs = {k: np.full((10, 3 if k == "keys" else C), 7, dtype=DTYPES[k]) for k in PLANES}
            rc, sm, err = raw_unpack(gpu, stream, nbytes, 10, outs)
            assert rc == ref.ERR_INVALID and err == text, (name, err, text)
            assert all((v == 7).all() for v in outs.values()) and (sm == -9).all(), name
    same_rows(gpu.unpack(s), {k: m[k] for k in PLANES}, "the valid stream")
    gpu.close()


@pytest.mark.parametrize("n", [3, 4])
def test_frontier_mode(mods, n):
    """a frontier-mode handle is accepted; a released block packs as its expanded view"""
    MLMap, _ = mods
    cfg = small_cfg(n, explore=True)
    gpu = MLMap(cfg, max_blocks=64)
    load(gpu, regular(np.random.default_rng(7400 + n), n, 65, cfg, True))
    before = gpu.export_blocks(raw=True)
    assert before["collapsed"].sum() > 3
    s = gpu.pack()
    assert s.tobytes() == ref.pack_map(before, n, *clamps(cfg))["stream"]
    assert gpu.pack(box=BOX, no_infl=True).tobytes() == ref.pack_map(before, n, *clamps(cfg), *BOX, True)["stream"]
    rows = gpu.unpack(s)
    same_rows(rows, sorted_view(before), f"frontier n {n}")
    col = before["collapsed"][delta_ref.order(before["keys"])].astype(bool)
    assert (rows["infl"][col] == ref.U).all() and (rows["occ"][col] == rows["occ"][col][:, :1]).all()
    after = gpu.export_blocks(raw=True)
    assert all(after[k].tobytes() == before[k].tobytes() for k in PLANES) and np.array_equal(after["collapsed"], before["collapsed"])
    gpu.close()


@pytest.mark.parametrize("n", [4, 10])
def test_save_load_and_packed_replica(mods, tmp_path, n):
    """a map built through the public calls: save -> load into a fresh handle gives export_blocks byte for byte; a replica follows by
    delta(packed=True) / apply_delta across integration, set-free, inflation, aging and a crop"""
    MLMap, _ = mods
    cfg = small_cfg(n)
    a, b = MLMap(cfg, max_blocks=64), MLMap(cfg, max_blocks=64)
    d_glb = n * cfg.subbox_d_xyz
    prev, steps, smaller = None, 0, 0

    def follow(what):
        nonlocal prev, steps, smaller
        d = a.delta(prev=prev, packed=True, device=steps % 2 == 1)
        if steps % 2 == 0:
            assert d.keys is None and isinstance(d.stream, np.ndarray)
        else:  # a Delta that carries only the stream
            d.keys = d.log_odds = d.occ = d.infl = None
        b.apply_delta(d)
        prev = d
        ea, eb = a.export_blocks(), b.export_blocks()
        for k in PLANES:
            assert ea[k].tobytes() == eb[k].tobytes(), f"{what}: {k}"
        E = int(d.summary[5] + d.summary[6])
        smaller += int(E > 0 and int(d.stream.shape[0]) < E * (12 + 6 * n ** 3))
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
    assert steps == 10 and smaller >= 5, (steps, smaller)
    path = str(tmp_path / "map.mlmpack")
    size = a.save(path)
    ea = a.export_blocks()
    assert 0 < size < len(ea["keys"]) * (12 + 6 * n ** 3)
    c = MLMap(cfg, max_blocks=64)
    res = c.load(path)
    ec = c.export_blocks()
    assert res["summary"][0] == len(ea["keys"]) and all(ea[k].tobytes() == ec[k].tobytes() for k in PLANES)
    # load with a fuse mode: every row finds its block, none is created
    fused = c.load(path, fuse="take")["fuse"]["summary"]
    assert fused[0] == fused[1] == len(ea["keys"]) and fused[2] == 0 and c.block_count() == len(ea["keys"])
    a.close(), b.close(), c.close()
