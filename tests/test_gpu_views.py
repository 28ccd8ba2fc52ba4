"""mlm_query_views: distinct-voxel accounting of grouped ray fans (include/mlmap_hip.h), every table word and every mark byte held to
plain Python sets over the Python walk (tests/view_ref.py) on the CPU oracle's block dump: room map and frontier-mode map with
released blocks, fans of 64 x 48 and 16 x 16 rays, the LDS path and the global path (forced by the knob "view_lds_bits"; both must
give the same answers), a box smaller than the fans, exclude and mark, host and device memory mixed, a caller's stream, a call right
behind an async batch, the greedy loop of three picks, and the refused arguments."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import raywalk_ref as rw
from tests import view_ref as vr

pytestmark = pytest.mark.gpu

OCC, INFL, UNKNOWN = rw.OCC, rw.INFL, rw.UNKNOWN
LDS_BITS = (64 * 1024 - 64) * 8


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


def real_map(mods, frontier):
    MLMap, OracleMap = mods
    if frontier:
        cfg = S1.with_(use_exploration_frontiers=True, subbox_n=5)
        gpu, cpu = MLMap(cfg, max_blocks=16384, max_batch=2), OracleMap(cfg)
        for img, (q, t) in syn.stream(cfg, "room_jitter", "smooth", 8):
            gpu.update_map(img, q, t)
            cpu.update_depth(img, q, t)
    else:
        cfg = S1
        gpu, cpu = MLMap(cfg, max_blocks=8192), OracleMap(cfg)
        for k, (img, (q, t)) in enumerate(syn.stream(cfg, "room_jitter", "smooth", 6)):
            gpu.update_map(img, q, t)
            cpu.update_depth(img, q, t)
            if k in (2, 4):
                gpu.inflate_map(t)
                cpu.inflate_map(t)
    return cfg, gpu, cpu


def flag_kw(flags):
    return {"occ": bool(flags & OCC), "infl": bool(flags & INFL), "unknown": bool(flags & UNKNOWN)}


def make_views(b, cfg, seed, n_big, n_small, extras=True):
    """n_big 64 x 48 fans of 4 m, n_small 16 x 16 fans of 8 m; with extras an empty view, one of invalid rays only, ties and
    grazed corners, one to be refused, an empty view"""
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    rng = np.random.default_rng(seed)
    big = vr.random_fans(rng, b, cfg, n_big, 64, 48, 4.0)
    small = vr.random_fans(rng, b, cfg, n_small, 16, 16, 8.0)
    groups = [(big[0][i * 3072:(i + 1) * 3072], big[1][i * 3072:(i + 1) * 3072]) for i in range(n_big)]
    groups += [(small[0][i * 256:(i + 1) * 256], small[1][i * 256:(i + 1) * 256]) for i in range(n_small)]
    if extras:
        w0, w1 = rw.weird_rays(d)
        bad = np.array([rw.valid(a, e, d) is None for a, e in zip(w0, w1)])
        lo_w, hi_w = b["keys"].min(0) * d * n - 0.5, (b["keys"].max(0) + 1) * d * n + 0.5
        s0, s1 = rw.special_rays(rng, lo_w, hi_w, d, count=30)
        c = lambda *v: [(x + 0.5) * d for x in v]
        far0, far1 = np.array([c(0, 0, 0), c(2000, 2000, 2000)]), np.array([c(3, 1, 0), c(2002, 2001, 2000)])
        groups += [(w0[:0], w1[:0]), (w0[bad], w1[bad]), (s0, s1), (far0, far1), (w0[:0], w1[:0])]
    p0, p1 = np.concatenate([g[0] for g in groups]), np.concatenate([g[1] for g in groups])
    vb = np.concatenate([[0], np.cumsum([len(g[0]) for g in groups])]).astype(np.int32)
    return p0, p1, vb


def small_box(b, cfg):
    full = (b["occ"] == ord("o")).any(axis=1)
    mid = (np.median(b["keys"][full], axis=0) * cfg.subbox_n).astype(int)
    return [int(mid[0]) - 12, int(mid[1]) - 14, int(mid[2]) - 6], [31, 29, 17]  # smaller than the fans


@pytest.mark.parametrize("frontier", [False, True], ids=["S1", "S1 frontier n5"])
def test_views_against_the_sets(mods, knobs, frontier):
    """every flag set, without a box and with box + exclude + mark, on the default plan, with every bitset in global scratch and
    with a small LDS limit that splits the views between the paths"""
    cfg, gpu, cpu = real_map(mods, frontier)
    b = cpu.export_blocks()
    if frontier:
        assert b["collapsed"].sum() > 20
    p0, p1, vb = make_views(b, cfg, 23 + frontier, 4, 3)
    walked = vr.walk(p0, p1, vb, cfg.subbox_d_xyz, rw.block_classes(b, cfg.subbox_n))
    ref, _ = vr.account(walked[:4], OCC)
    print("64 x 48 fans, OCC:", ref.tolist())
    vr.non_vacuous(ref)
    box = small_box(b, cfg)
    shape = box[1][::-1]
    rng = np.random.default_rng(3)
    exclude = (rng.random(shape) < 0.3).astype(np.uint8) * 7
    mark0 = rng.choice(np.array([0, 0, 1, 2, 4, 128], dtype=np.uint8), size=shape)
    exps = {f: (vr.account(walked, f)[0], vr.account(walked, f, box=box, exclude=exclude, mark=mark0.copy())) for f in rw.FLAG_SETS}
    for lds_bits in (LDS_BITS, 0, 100000):
        knobs.set("view_lds_bits", lds_bits)
        for f in rw.FLAG_SETS:
            exp, (exp_b, exp_m) = exps[f]
            got = gpu.query_views(p0, p1, vb, **flag_kw(f))
            vr.assert_equal(got["table"], exp, what=f"frontier={frontier} flags={f} lds_bits={lds_bits}")
            assert "mark" not in got
            got = gpu.query_views(p0, p1, vb, box=box, exclude=exclude, mark=mark0.copy(), **flag_kw(f))
            vr.assert_equal(got["table"], exp_b, got["mark"], exp_m, what=f"frontier={frontier} flags={f} lds_bits={lds_bits} box")
            if f == OCC:
                assert ((exp_m & 1) != (mark0 & 1)).any() and ((exp_m & 2) != (mark0 & 2)).any() and exp_b[:4, 0].sum() > 0
    gpu.close()


def test_destinations_stream_and_async(mods):
    """device inputs and outputs on a caller's stream behind queued work; host and device pointers mixed; mark alone; a call right
    behind an async batch sees every submitted frame; the scratch grows at the first call and then stays"""
    import torch

    MLMap, OracleMap = mods
    nf = 8
    frames = np.stack([img for img, _ in syn.stream(S1, "room_jitter", "smooth", nf)])
    poses = syn.smooth_trajectory(nf, 42)
    q, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    gpu, cpu = MLMap(S1, max_blocks=8192, max_batch=4), OracleMap(S1)
    for k in range(nf):
        cpu.update_depth(frames[k], q[k], t[k])
    b = cpu.export_blocks()
    p0, p1, vb = make_views(b, S1, 31, 3, 2)
    walked = vr.walk(p0, p1, vb, S1.subbox_d_xyz, rw.block_classes(b, S1.subbox_n))
    box = small_box(b, S1)
    shape = box[1][::-1]
    exclude = (np.random.default_rng(8).random(shape) < 0.25).astype(np.uint8)
    exp, exp_m = vr.account(walked, OCC | INFL, box=box, exclude=exclude, mark=np.zeros(shape, np.uint8))
    assert exp[:3, 0].sum() > 0 and exp_m.any()
    gpu.set_async(True)
    gpu.update_map_batch(frames, q, t)  # no sync()
    got = gpu.query_views(p0, p1, vb, infl=True, box=box, exclude=exclude, mark=True)
    vr.assert_equal(got["table"], exp, got["mark"], exp_m, "async")
    grown = gpu.frame_stats()["device_bytes"]
    gpu.query_views(p0, p1, vb, infl=True, box=box, exclude=exclude, mark=True)
    assert gpu.frame_stats()["device_bytes"] == grown

    s = torch.cuda.Stream()
    gpu.set_stream(s.cuda_stream)
    nv = len(vb) - 1
    junk = torch.ones(1 << 26, device="cuda")
    h0, h1 = torch.from_numpy(p0).pin_memory(), torch.from_numpy(p1).pin_memory()
    with torch.cuda.stream(s):
        for _ in range(50):  # (keeps the caller's stream busy: the inputs arrive, and the answers are written, behind this work)
            junk.mul_(1.0001)
        d0, d1 = h0.to("cuda", non_blocking=True), h1.to("cuda", non_blocking=True)
        dvb = torch.from_numpy(vb).pin_memory().to("cuda", non_blocking=True)
        dex = torch.from_numpy(exclude).pin_memory().to("cuda", non_blocking=True)
        dmark = torch.zeros(shape, dtype=torch.uint8, device="cuda")
        dtab = torch.full((nv, 8), 7, dtype=torch.int64, device="cuda")
    gpu.query_views_dev(d0.data_ptr(), d1.data_ptr(), dvb.data_ptr(), nv, occ=True, infl=True, box=box, exclude=dex.data_ptr(),
                        mark=dmark.data_ptr(), table=dtab.data_ptr())
    vr.assert_equal(dtab.cpu().numpy(), exp, dmark.cpu().numpy(), exp_m, "device")
    # mixed: device rays and exclude, host view_begin, table and mark; then host rays, device table, no mark; then mark alone
    tab, mk = np.full((nv, 8), 9, np.int64), np.zeros(shape, np.uint8)
    gpu.query_views_dev(d0.data_ptr(), d1.data_ptr(), vb.ctypes.data, nv, occ=True, infl=True, box=box, exclude=dex.data_ptr(),
                        mark=mk.ctypes.data, table=tab.ctypes.data)
    vr.assert_equal(tab, exp, mk, exp_m, "mixed 1")
    dtab.fill_(5)
    gpu.query_views_dev(p0.ctypes.data, d1.data_ptr(), dvb.data_ptr(), nv, occ=True, infl=True, box=box, exclude=exclude.ctypes.data,
                        table=dtab.data_ptr())
    vr.assert_equal(dtab.cpu().numpy(), exp, what="mixed 2")
    mk[...] = 0
    gpu.query_views_dev(p0.ctypes.data, p1.ctypes.data, vb.ctypes.data, nv, occ=True, infl=True, box=box, mark=mk.ctypes.data)
    assert np.array_equal(mk, exp_m)
    gpu.close()


def test_greedy_three_picks(mods, knobs):
    """score all, mark the winner, score again with exclude — three picks, against the same loop on the reference; on both paths"""
    cfg, gpu, cpu = real_map(mods, False)
    b = cpu.export_blocks()
    p0, p1, vb = make_views(b, cfg, 41, 6, 0, extras=False)
    walked = vr.walk(p0, p1, vb, cfg.subbox_d_xyz, rw.block_classes(b, cfg.subbox_n))
    lo_v, hi_v = b["keys"].min(0) * cfg.subbox_n - 20, (b["keys"].max(0) + 1) * cfg.subbox_n + 20
    box = ([int(x) for x in lo_v], [int(x) for x in hi_v - lo_v])
    shape = box[1][::-1]

    def greedy(score, mark_one):
        seen, picks, gains = np.zeros(shape, np.uint8), [], []
        for _ in range(3):
            t = score(seen)
            gains.append(t[:, 1].copy())
            k = int(np.argmax(t[:, 1]))  # (ties: the lowest index, in both loops)
            picks.append(k)
            seen = mark_one(k, seen)
        return picks, gains, seen

    ref = greedy(lambda seen: vr.account(walked, OCC, box=box, exclude=seen)[0],
                 lambda k, seen: vr.account(walked[k:k + 1], OCC, box=box, mark=seen.copy())[1])
    picks, gains, seen = ref
    assert len(set(picks)) == 3
    drop = (gains[1] < gains[0]) & (gains[1] > 0)
    assert drop.any(), (gains[0].tolist(), gains[1].tolist())  # with exclude from the winner some view's gain drops but stays positive
    one = lambda k: (p0[vb[k]:vb[k + 1]], p1[vb[k]:vb[k + 1]], np.array([0, vb[k + 1] - vb[k]], np.int32))
    for lds_bits in (LDS_BITS, 0):
        knobs.set("view_lds_bits", lds_bits)
        got = greedy(lambda seen: gpu.query_views(p0, p1, vb, box=box, exclude=seen)["table"],
                     lambda k, seen: gpu.query_views(*one(k), box=box, mark=seen.copy())["mark"])
        assert got[0] == picks and np.array_equal(got[2], seen)
        for a, e in zip(got[1], gains):
            assert np.array_equal(a, e)
    gpu.close()


def test_refused_arguments(mods):
    MLMap, _ = mods
    gpu = MLMap(S1, max_blocks=1024)
    L, h, vp = gpu._L, gpu._h, ctypes.c_void_p
    d = S1.subbox_d_xyz
    a = np.array([[0.05 * d, 0.5 * d, 0.5 * d], [np.nan, 0, 0], [0.5 * d, 0.5 * d, 0.5 * d]])
    e = np.array([[3.5 * d, 0.5 * d, 0.5 * d], [1, 1, 1], [0.5 * d, 2.5 * d, 0.5 * d]])
    vb = np.array([0, 2, 2, 3], np.int32)
    lo, dims = np.array([-2, -2, -2], np.int32), np.array([8, 8, 8], np.int32)
    tab, ex, mk = np.zeros((3, 8), np.int64), np.zeros((8, 8, 8), np.uint8), np.zeros((8, 8, 8), np.uint8)
    P = lambda x: None if x is None else x.ctypes.data_as(vp)
    call = lambda p0=a, p1=e, b=vb, nv=3, fl=OCC, l=lo, dm=dims, x=ex, m=mk, t=tab: L.mlm_query_views(h, P(p0), P(p1), P(b), nv, fl, P(l), P(dm), P(x), P(m), P(t))
    ok = lambda: call()
    bad = [lambda: call(b=np.array([0, 2, 1, 3], np.int32)), lambda: call(b=np.array([-1, 2, 2, 3], np.int32)), lambda: call(b=None),
           lambda: call(nv=-1), lambda: call(l=None, dm=None), lambda: call(l=None, dm=None, m=None),  # exclude / mark without a box
           lambda: call(l=None, dm=None, x=None), lambda: call(dm=None), lambda: call(m=ex), lambda: call(fl=8), lambda: call(fl=-1),
           lambda: call(m=None, t=None), lambda: call(p0=None), lambda: call(dm=np.array([8, 0, 8], np.int32)),
           lambda: call(l=np.array([2 ** 31 - 4, 0, 0], np.int32)), lambda: call(l=np.array([0, 0, 0], np.int32), dm=np.array([2048, 2048, 2048], np.int32), x=None, m=None)]
    for i, f in enumerate(bad):
        assert f() == -1, i
        assert ok() == 0, i
    assert call(b=None, nv=0) == 0 and call(p0=None, p1=None, b=np.array([5], np.int32), nv=0) == 0  # n_views == 0
    assert call(p0=None, p1=None, b=np.array([4, 4, 4, 4], np.int32)) == 0                                 # views without rays need no rays
    # an empty map: every voxel UNKNOWN.  View 0: ray 0 visits voxels (0..3, 0, 0), ray 1 is invalid; view 1 is empty; view 2:
    # (0, 0..2, 0) — voxel (0, 0, 0) is shared between the views, not within one
    mk[...] = 0
    assert ok() == 0
    assert tab.tolist() == [[4, 4, 0, 0, 0, 1, 4, 0], [0] * 8, [3, 3, 0, 0, 0, 0, 3, 0]]
    want = np.zeros((8, 8, 8), np.uint8)
    want[2, 2, 2:6] = 1
    want[2, 2:5, 2] = 1
    assert np.array_equal(mk, want)
    assert call(fl=UNKNOWN, x=None, m=None) == 0  # every ray stops in its start voxel
    assert tab.tolist() == [[0, 0, 0, 1, 1, 1, 0, 0], [0] * 8, [0, 0, 0, 1, 1, 0, 0, 0]]
    gpu.close()
