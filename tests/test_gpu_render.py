"""mlm_render_depth: the depth images the map predicts for a pinhole camera (include/mlmap_hip.h).  The kernel makes every pixel's
segment itself; here the same segments are made in numpy (tests/render_ref.py, the contract's arithmetic in float64) and cast by
mlm_query_rays, whose answers tests/test_gpu_rays.py holds to the Python walk: status, voxel and n_unknown must be equal, the depth
must be the contract's formula on the returned t, the table the numpy sums — for every flag set, image shapes with partial tiles on
both edges, host and device memory per pointer, calls of more than one chunk, and after every call that changes the map."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from mlmapping_amd.mlmap import compose_T_ws
from tests import raywalk_ref as rw
from tests import render_ref as rr

pytestmark = pytest.mark.gpu

OCC, INFL, UNKNOWN = rw.OCC, rw.INFL, rw.UNKNOWN
K_WIDE = (14.0, 20.0, 18.0, 10.0)  # a 37 x 21 image, 52 x 27 degrees to each side: wider than the camera that built the map
MM = 3900                          # ends in front of the room's far wall (4.0 .. 4.1 m): floor, ceiling and side walls stop rays
SHAPES = [(3, 37, 21), (1, 1, 1), (2, 64, 1), (2, 1, 64), (1, 130, 9)]  # (poses, width, height)
OUT = ("depth", "status", "voxel", "n_unknown", "table")
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap

    return MLMap


def build(MLMap, frontier, n_frames=None):
    """a handle after the room_jitter stream (as tests/test_gpu_rays.py builds it) and the camera poses of its frames"""
    cfg = S1.with_(use_exploration_frontiers=True, subbox_n=5) if frontier else S1
    gpu = MLMap(cfg, max_blocks=16384 if frontier else 8192, max_batch=2)
    poses = []
    for k, (img, (q, t)) in enumerate(syn.stream(cfg, "room_jitter", "smooth", n_frames or (8 if frontier else 6))):
        gpu.update_map(img, q, t)
        poses.append((q, t))
        if not frontier and k in (2, 4):
            gpu.inflate_map(t)
    T = compose_T_ws(np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses]), cfg.T_B_S)
    return cfg, gpu, T


@pytest.fixture(scope="module")
def maps(mods):
    out = {False: build(mods, False), True: build(mods, True)}
    yield out
    for _, gpu, _ in out.values():
        gpu.close()


def flags_kw(f):
    return {"occ": bool(f & OCC), "infl": bool(f & INFL), "unknown": bool(f & UNKNOWN)}


def expected(gpu, T, w, h, K, mm, f):
    """mlm_render_depth's outputs from mlm_query_rays over the numpy segments of the same pixels"""
    p0, p1 = rr.segments(T, w, h, K, mm)
    r = gpu.cast_rays(p0.reshape(-1, 3), p1.reshape(-1, 3), **flags_kw(f))
    return rr.from_rays(r, len(T), h, w, mm), r


def assert_same(got, exp, what):
    for k in OUT:
        if k in got:
            assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k, got[k].dtype, got[k].shape, exp[k].dtype, exp[k].shape)
            bad = np.flatnonzero((got[k] != exp[k]).reshape(-1))
            assert bad.size == 0, f"{what} {k}: {bad.size} of {got[k].size} differ, first #{bad[0]}: {got[k].reshape(-1)[bad[0]]} vs {exp[k].reshape(-1)[bad[0]]}"


@pytest.mark.parametrize("frontier", [False, True], ids=["S1 inflated", "S1 frontier n5 (released blocks)"])
def test_parity_with_query_rays(maps, frontier):
    cfg, gpu, T_all = maps[frontier]
    if frontier:
        assert gpu.export_blocks()["collapsed"].sum() > 20
    else:
        b = gpu.export_blocks()
        assert ((b["infl"] == ord("o")) & (b["occ"] != ord("o"))).sum() > 100  # (inflation applied: OCC | INFL differs from OCC)
    for n, w, h in SHAPES:
        T = T_all[[0, 2, 5][:n]]
        for f in rw.FLAG_SETS:
            exp, r = expected(gpu, T, w, h, K_WIDE, MM, f)
            got = gpu.render_depth(T_ws=T, width=w, height=h, K=K_WIDE, max_depth=MM / 1000.0, **flags_kw(f))
            assert_same(got, exp, f"{n} x {w} x {h} flags={f}")
            assert np.array_equal(got["depth"] == 0, got["status"] != 1)
            if (n, w, h) == SHAPES[0] and f == OCC:
                # from the reference's answers, so that the comparison cannot pass vacuously
                st, npx = r["status"], r["status"].size
                print(f"frontier={frontier}: stopped {(st == 1).sum()} / not {(st == 0).sum()} of {npx}, n_unknown > 0: {(r['n_unknown'] > 0).sum()}")
                assert (st == 1).sum() * 10 >= npx and (st == 0).sum() * 10 >= npx and (r["n_unknown"] > 0).any()
                assert len(np.unique(exp["depth"])) > 50 and (exp["table"][:, 0] != exp["table"][0, 0]).any()  # (poses differ)
            if f == OCC | INFL and not frontier and (n, w, h) == SHAPES[0]:
                assert not np.array_equal(got["depth"], gpu.render_depth(T_ws=T, width=w, height=h, K=K_WIDE, max_depth=MM / 1000.0)["depth"])
    # the handle's own camera (K = NULL) and the body poses (q_wb, t_wb) of the frames
    poses = [p for _, p in syn.stream(cfg, "room_jitter", "smooth", 2)]
    q, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    Kc = (cfg.cam_fx, cfg.cam_fy, cfg.cam_cx, cfg.cam_cy)
    got = gpu.render_depth(q_wb=q, t_wb=t, width=70, height=50, max_depth=6.0)
    exp, _ = expected(gpu, compose_T_ws(q, t, cfg.T_B_S), 70, 50, Kc, 6000, OCC)
    assert_same(got, exp, "K = NULL")


def test_pointer_matrix(maps):
    """T_ws and every output in host or in device memory, each on its own; each single output with the others NULL"""
    import torch

    cfg, gpu, T_all = maps[False]
    n, w, h = SHAPES[0]
    T = np.ascontiguousarray(T_all[[0, 2, 5]])
    ref = gpu.render_depth(T_ws=T, width=w, height=h, K=K_WIDE, max_depth=MM / 1000.0, infl=True)
    exp, _ = expected(gpu, T, w, h, K_WIDE, MM, OCC | INFL)
    assert_same(ref, exp, "all host")
    Kd = np.array(K_WIDE, dtype=np.float64)
    tdt = {"depth": torch.int16, "status": torch.int8, "voxel": torch.int32, "n_unknown": torch.int32, "table": torch.int64}
    T_dev = torch.from_numpy(T).cuda()

    def call(t_on_dev, on_dev, which):
        host = {k: np.full(ref[k].shape, 7, dtype=ref[k].dtype) for k in which}
        dev = {k: torch.full(ref[k].shape, 7, dtype=tdt[k], device="cuda") for k in which if on_dev[k]}
        ptr = [None if k not in which else vp(dev[k].data_ptr()) if on_dev[k] else host[k].ctypes.data_as(vp) for k in OUT]
        tp = vp(T_dev.data_ptr()) if t_on_dev else T.ctypes.data_as(vp)
        assert gpu._L.mlm_render_depth(gpu._h, tp, n, w, h, Kd.ctypes.data_as(vp), MM, OCC | INFL, *ptr) == 0
        return {k: (dev[k].cpu().numpy().view(ref[k].dtype) if on_dev[k] else host[k]) for k in which}

    for bits in range(64):
        on_dev = {k: bool(bits >> (i + 1) & 1) for i, k in enumerate(OUT)}
        assert_same(call(bool(bits & 1), on_dev, OUT), ref, f"pointer matrix {bits:06b}")
    for k in OUT:
        for d in (False, True):
            assert_same(call(d, {k: d}, (k,)), ref, f"{k} alone, device={d}")


def test_more_than_one_chunk(maps):
    """5 poses x 512 x 512 (1.3 M pixels: more than one chunk of 2^20), host depth + status only"""
    cfg, gpu, T_all = maps[False]
    n, w, h = 5, 512, 512
    T = np.ascontiguousarray(T_all[:5])
    K = (300.0, 300.0, 255.5, 250.0)
    depth, status = np.zeros((n, h, w), np.uint16), np.zeros((n, h, w), np.int8)
    Kd = np.array(K, dtype=np.float64)
    assert gpu._L.mlm_render_depth(gpu._h, T.ctypes.data_as(vp), n, w, h, Kd.ctypes.data_as(vp), 4050, OCC, depth.ctypes.data_as(vp),
                                   status.ctypes.data_as(vp), None, None, None) == 0
    exp, r = expected(gpu, T, w, h, K, 4050, OCC)
    assert_same({"depth": depth, "status": status}, exp, "1.3 M pixels")
    st = r["status"]
    print(f"1.3 M pixels: stopped {(st == 1).sum()}, not stopped {(st == 0).sum()}")
    assert (st == 1).any() and (st == 0).any() and len(np.unique(depth[4])) > 50  # (the last pose, in the second chunk, is an image too)


def test_render_follows_the_map(mods):
    """straight after (no sync) mlm_integrate_depth_u16, mlm_set_free_in_bound, mlm_inflate_map and mlm_import_blocks, once in async
    mode, and on a caller's stream: the image is what mlm_query_rays answers at that moment (and after the first two it has changed)"""
    import torch

    MLMap = mods
    cfg, gpu, T_all = build(MLMap, False, n_frames=3)
    frames = list(syn.stream(cfg, "room_jitter", "smooth", 8))
    T, (n, w, h) = np.ascontiguousarray(T_all[:2]), (2, 37, 21)
    seen = []

    def check(g, what, f=OCC | INFL, changed=True):
        got = g.render_depth(T_ws=T, width=w, height=h, K=K_WIDE, max_depth=4.3, **flags_kw(f))
        exp, _ = expected(g, T, w, h, K_WIDE, 4300, f)
        assert_same(got, exp, what)
        if seen:
            same = all(np.array_equal(got[k], seen[-1][k]) for k in OUT)
            print(f"{what}: {'the same image as' if same else 'differs from'} the one before")
            assert not (changed and same), what
        seen.append(got)
        return got

    check(gpu, "start")
    for img, (q, t) in frames[3:5]:
        gpu.update_map(img, q, t)
    check(gpu, "mlm_integrate_depth_u16")
    gpu.setFree_map_in_bound(T[0, 9:] + [-1.0, -1.0, -2.0], T[0, 9:] + [6.0, 6.0, 0.0])
    check(gpu, "mlm_set_free_in_bound")
    gpu.inflate_map(frames[4][1][1])
    check(gpu, "mlm_inflate_map", changed=False)
    gpu.set_async(True)
    gpu.update_map_batch(np.stack([f[0] for f in frames[5:8]]), np.stack([f[1][0] for f in frames[5:8]]), np.stack([f[1][1] for f in frames[5:8]]))
    last = check(gpu, "async mode, frames in flight", changed=False)
    gpu.set_async(False)
    # a second handle that gets the first one's blocks
    b = gpu.export_blocks()
    other = MLMap(cfg, max_blocks=8192)
    seen.clear()
    check(other, "empty map", f=UNKNOWN)
    other.import_blocks(b["keys"], b["log_odds"], b["occ"], b["infl"], b["collapsed"])
    got = check(other, "mlm_import_blocks", changed=False)
    assert_same(got, last, "the imported map renders as the exported one")
    other.close()
    # the caller's stream, behind queued work, device in and out
    s = torch.cuda.Stream()
    gpu.set_stream(s.cuda_stream)
    junk = torch.ones(1 << 26, device="cuda")
    hT = torch.from_numpy(T).pin_memory()
    with torch.cuda.stream(s):
        for _ in range(50):
            junk.mul_(1.0001)
        dT = hT.to("cuda", non_blocking=True)
        depth = torch.full((n, h, w), 7, dtype=torch.int16, device="cuda")
        table = torch.full((n, 4), 7, dtype=torch.int64, device="cuda")
    gpu.render_depth_dev(dT.data_ptr(), n, w, h, K=K_WIDE, max_depth=4.3, infl=True, depth=depth.data_ptr(), table=table.data_ptr())
    assert_same({"depth": depth.cpu().numpy().view(np.uint16), "table": table.cpu().numpy()}, last, "caller's stream")
    gpu.close()


def test_round_trip_of_a_wall(mods):
    """a flat wall 3 m in front of the camera, integrated five times from one pose and rendered from that pose with MLM_RAY_OCC and the
    handle's own camera: where both images are non-zero the rendered depth lies within two voxel diagonals of the measured one.  A
    sanity property of the pair integrate / render, not an exact one: the map quantises the wall into the awareness map's polar
    cells and then into voxels, and the render reports where a ray ENTERS the first occupied voxel."""
    MLMap = mods
    cfg = S1
    gpu = MLMap(cfg, max_blocks=8192)
    img = np.full((cfg.height, cfg.width), 3000, dtype=np.uint16)
    q, t = syn.static_pose()
    for _ in range(5):
        gpu.update_map(img, q, t)
    got = gpu.render_depth(q_wb=q[None], t_wb=t[None], width=cfg.width, height=cfg.height, max_depth=6.0)
    ren = got["depth"][0].astype(np.int64)
    both = (ren != 0) & (img != 0)
    err = np.abs(ren - img.astype(np.int64))[both]
    tol = 2.0 * np.sqrt(3.0) * cfg.subbox_d_xyz * 1000.0
    print(f"round trip: compared {both.sum()} of {img.size} wall pixels ({both.mean():.3f}), error max {err.max()} mm, mean {err.mean():.1f} mm, tolerance {tol:.0f} mm")
    assert both.sum() * 2 >= img.size
    assert err.max() <= tol
    gpu.close()


def test_errors_leave_the_handle_usable_and_the_staging_is_what_the_header_states(mods):
    MLMap = mods
    cfg, gpu, T_all = build(MLMap, False, n_frames=2)
    L, hnd = gpu._L, gpu._h
    n, w, h = SHAPES[0]
    T = np.ascontiguousarray(np.concatenate([T_all[:2], T_all[:1]]))
    Kd = np.array(K_WIDE, dtype=np.float64)
    outs = {"depth": np.zeros((n, h, w), np.uint16), "status": np.zeros((n, h, w), np.int8), "voxel": np.zeros((n, h, w, 3), np.int32),
            "n_unknown": np.zeros((n, h, w), np.int32), "table": np.zeros((n, 4), np.int64)}
    po = [outs[k].ctypes.data_as(vp) for k in OUT]
    Tp, Kp = T.ctypes.data_as(vp), Kd.ctypes.data_as(vp)

    def k_with(i, v):
        k = Kd.copy()
        k[i] = v
        return k

    before = gpu.frame_stats()["device_bytes"]
    assert L.mlm_render_depth(hnd, Tp, n, w, h, Kp, MM, OCC, *po) == 0
    ref = {k: v.copy() for k, v in outs.items()}
    r256 = lambda x: (x + 255) // 256 * 256
    px = n * w * h
    stated = r256(96 * n) + r256(2 * px) + r256(px) + r256(12 * px) + r256(4 * px) + r256(32 * n)
    grown = gpu.frame_stats()["device_bytes"]
    assert grown - before == stated, (grown - before, stated)
    bad_k = [k_with(0, 0.0), k_with(0, -1.0), k_with(0, np.nan), k_with(0, np.inf), k_with(1, 0.0), k_with(1, -np.inf), k_with(1, np.nan),
             k_with(2, np.nan), k_with(2, np.inf), k_with(3, np.nan), k_with(3, -np.inf)]
    bad = [lambda: L.mlm_render_depth(hnd, Tp, -1, w, h, Kp, MM, OCC, *po), lambda: L.mlm_render_depth(hnd, None, n, w, h, Kp, MM, OCC, *po),
           lambda: L.mlm_render_depth(hnd, Tp, n, 0, h, Kp, MM, OCC, *po), lambda: L.mlm_render_depth(hnd, Tp, n, -3, h, Kp, MM, OCC, *po),
           lambda: L.mlm_render_depth(hnd, Tp, n, 8193, h, Kp, MM, OCC, *po), lambda: L.mlm_render_depth(hnd, Tp, n, w, 0, Kp, MM, OCC, *po),
           lambda: L.mlm_render_depth(hnd, Tp, n, w, 8193, Kp, MM, OCC, *po),
           lambda: L.mlm_render_depth(hnd, Tp, 32, 8192, 8192, Kp, MM, OCC, *po),  # 2^31 pixels (refused before anything is read)
           lambda: L.mlm_render_depth(hnd, Tp, n, w, h, Kp, 0, OCC, *po), lambda: L.mlm_render_depth(hnd, Tp, n, w, h, Kp, -5, OCC, *po),
           lambda: L.mlm_render_depth(hnd, Tp, n, w, h, Kp, 65536, OCC, *po), lambda: L.mlm_render_depth(hnd, Tp, n, w, h, Kp, MM, 8, *po),
           lambda: L.mlm_render_depth(hnd, Tp, n, w, h, Kp, MM, -1, *po), lambda: L.mlm_render_depth(hnd, Tp, n, w, h, Kp, MM, OCC | 1 << 20, *po),
           lambda: L.mlm_render_depth(hnd, Tp, n, w, h, Kp, MM, OCC, None, None, None, None, None)]
    bad += [(lambda k=k: L.mlm_render_depth(hnd, Tp, n, w, h, k.ctypes.data_as(vp), MM, OCC, *po)) for k in bad_k]
    for i, call in enumerate(bad):
        assert call() == -1, i
        assert b"mlm_render_depth" in L.mlm_last_error(hnd)
        for v in outs.values():
            v[...] = 9
        assert L.mlm_render_depth(hnd, Tp, n, w, h, Kp, MM, OCC, *po) == 0
        assert_same(outs, ref, f"after refused call {i}")
    assert L.mlm_render_depth(hnd, None, 0, w, h, Kp, MM, OCC, *po) == 0  # n_poses == 0
    assert L.mlm_render_depth(hnd, Tp, 0, w, h, Kp, MM, OCC, *po) == 0
    assert_same(outs, ref, "n_poses == 0 writes nothing")
    assert gpu.frame_stats()["device_bytes"] == grown  # (no call since has needed more)
    # a non-finite pose is no error: its pixels are invalid, the other poses' are not touched by it
    T2 = T.copy()
    T2[1, 3] = np.nan
    assert L.mlm_render_depth(hnd, T2.ctypes.data_as(vp), n, w, h, Kp, MM, OCC, *po) == 0
    assert np.all(outs["status"][1] == -1) and np.all(outs["depth"][1] == 0) and outs["table"][1].tolist() == [0, 0, w * h, 0]
    assert np.array_equal(outs["depth"][[0, 2]], ref["depth"][[0, 2]]) and np.array_equal(outs["table"][[0, 2]], ref["table"][[0, 2]])
    assert gpu.frame_stats()["device_bytes"] == grown
    gpu.close()
