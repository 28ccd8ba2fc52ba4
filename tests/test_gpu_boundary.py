"""GPU tests of the drop-in boundary itself: the C++ facade used from a real C++ program, thread safety of the entry
points, caller-supplied streams, recovery after a capacity error, and the multi-GPU merge path over RCCL with the maps
taken from and loaded back into live device handles."""
import ctypes
import os
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1, SDEF, to_c
from tests.util import assert_same_bits, compare_maps, voxel_centres

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


def test_cpp_facade_client_process(mods, tmp_path):
    """include/mlmap_facade.hpp instantiated and used by a C++ program (g++, linked against libmlmap_hip.so only), run
    as a fresh child process: every template method is compiled and called, its answers must equal the oracle's."""
    MLMap, OracleMap = mods
    cfg = SDEF
    exe = tmp_path / "facade_client"
    lib_dir = os.path.join(ROOT, "mlmapping_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_client.cpp"), "-o", str(exe), "-L", lib_dir, "-lmlmap_hip",
                           f"-Wl,-rpath,{lib_dir}"])
    n_frames, n_pos = 4, 3000
    cpu = OracleMap(cfg)
    rng = np.random.default_rng(4)
    blob = bytearray(bytes(to_c(cfg)))
    blob += struct.pack("4i", n_frames, cfg.width, cfg.height, n_pos)
    for img, (q, t) in syn.stream(cfg, "room_jitter", "smooth", n_frames):
        blob += np.concatenate([q, t]).astype(np.float64).tobytes() + np.ascontiguousarray(img, dtype=np.uint16).tobytes()
        cpu.update_depth(img, q, t)
    cpu.inflate_map([0.0, 0.0, 1.5])
    pos = np.concatenate([rng.uniform([-2, -5, 0], [6, 5, 3], size=(n_pos - 1000, 3)), voxel_centres(cpu.export_blocks(), cfg, 1000)])
    blob += pos.astype(np.float64).tobytes()
    path = tmp_path / "in.bin"
    path.write_bytes(bytes(blob))
    out = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    rows = [ln.split() for ln in out[:n_pos]]
    occ = np.array([int(r[0]) for r in rows])
    occ_i = np.array([int(r[1]) for r in rows])
    infl = np.array([int(r[2]) for r in rows])
    odd = np.array([float.fromhex(r[3]) for r in rows], dtype=np.float32)
    grad = np.array([[float.fromhex(x) for x in r[4:7]] for r in rows])
    grad2 = np.array([[float.fromhex(x) for x in r[7:10]] for r in rows])
    assert np.array_equal(occ, cpu.getOccupancy(pos))
    assert np.array_equal(occ_i, cpu.getOccupancy(pos, inflate=0.15))
    assert np.array_equal(infl, cpu.getInflateOccupancy(pos))
    assert_same_bits(odd, cpu.getOdd(pos), "getOdd")
    for g, it in ((grad, 5), (grad2, 2)):
        cg = cpu.getOddGrad(pos, it)
        assert_same_bits(g, cg, f"getOddGrad({it})")
    at = [float.fromhex(x) for x in out[n_pos].split()[1:]]
    want = cpu.getOddAt(np.array([[0, 0, 1], [40, 40, 40]], dtype=np.int32), np.array([7, 0], dtype=np.int32))
    assert_same_bits(np.array(at, dtype=np.float32), want, "getOddAt")
    cpu.setFree_map_in_bound([0.5, -0.5, 1.0], [1.0, 0.5, 1.5])
    o_free = int(cpu.getOccupancy(np.array([[0.75, 0.0, 1.25]]))[0])
    assert out[n_pos + 1].split()[1:] == [str(o_free), str(int(o_free == 1))]
    # local_map_snapshot(): the visualisers' loops over observed_group_map (rviz_vis.cpp:280-321) give the oracle's sums
    snap = out[n_pos + 2].split()
    assert snap[0] == "snapshot"
    b = cpu.export_blocks()
    gm = cpu.global_map_points().astype(np.float64)
    assert [int(x) for x in snap[1:6]] == [b["keys"].shape[0], int((b["occ"] == ord("o")).sum()), int((b["occ"] == ord("f")).sum()), gm.shape[0],
                                           cpu.export_frontier().shape[0]]
    assert np.allclose([float.fromhex(x) for x in snap[6:9]], gm.sum(0), rtol=1e-9, atol=1e-6)
    assert abs(float.fromhex(snap[9]) - float(b["log_odds"].astype(np.float64).sum())) <= 1e-6 * max(1.0, abs(float(b["log_odds"].astype(np.float64).sum())))
    # and the same answers through the ctypes path
    gpu = MLMap(cfg, max_blocks=8192)
    for img, (q, t) in syn.stream(cfg, "room_jitter", "smooth", n_frames):
        gpu.update_map(img, q, t)
    gpu.inflate_map([0.0, 0.0, 1.5])
    assert np.array_equal(occ, gpu.getOccupancy(pos)) and np.array_equal(infl, gpu.getInflateOccupancy(pos))
    assert np.array_equal(odd.view(np.uint32), gpu.getOdd(pos).view(np.uint32))


def test_queries_from_a_second_thread(mods):
    """Planner thread vs depth callback (the reference runs both on an MT nodelet without locking): queries issued from a
    second thread while the first one integrates must neither crash nor corrupt anything; every answer must be one the
    map could give at some frame boundary, and the final map must equal the oracle's."""
    MLMap, OracleMap = mods
    cfg = SDEF
    n = 12
    frames = list(syn.stream(cfg, "room_jitter", "smooth", n))
    cpu = OracleMap(cfg)
    rng = np.random.default_rng(8)
    pos = rng.uniform([-2, -5, 0], [6, 5, 3], size=(4000, 3))
    states = [cpu.getOccupancy(pos).copy()]  # answers at every frame boundary
    for img, (q, t) in frames:
        cpu.update_depth(img, q, t)
        states.append(cpu.getOccupancy(pos).copy())
    states = np.stack(states)
    gpu = MLMap(cfg, max_blocks=8192, max_batch=4)
    errors, answers = [], []
    stop = threading.Event()

    def planner():
        try:
            while not stop.is_set():
                a = gpu.getOccupancy(pos)
                o = gpu.getOdd(pos[:500])
                assert np.isfinite(o).all()
                answers.append(a)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = threading.Thread(target=planner)
    th.start()
    for mode in (False, True):
        gpu.set_async(mode)
        for img, (q, t) in frames[: n // 2] if not mode else frames[n // 2:]:
            gpu.update_map(img, q, t)
    gpu.sync()
    stop.set()
    th.join()
    assert not errors, errors
    assert len(answers) >= 2
    for a in answers:  # a query observes a completed integrate call: the map at SOME frame boundary
        assert (states == a[None, :]).all(axis=1).any(), "a concurrent query saw a map no frame boundary produces"
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "after concurrent queries")


def test_caller_stream_orders_device_inputs(mods):
    """mlm_set_stream: a depth image produced by work enqueued on the caller's stream (here: a long chain of torch kernels
    ending in the copy that fills the image) is read only after that work — no host synchronisation by the caller."""
    import torch

    MLMap, OracleMap = mods
    cfg = S1
    gpu, cpu = MLMap(cfg, max_blocks=8192, max_batch=4), OracleMap(cfg)
    s = torch.cuda.Stream()
    gpu.set_stream(s.cuda_stream)
    frames = [img for img, _ in syn.stream(cfg, "room_jitter", "smooth", 6)]
    poses = syn.smooth_trajectory(6, 42)
    src = [torch.from_numpy(f.view(np.int16)).cuda() for f in frames]
    buf = torch.zeros((4, cfg.height, cfg.width), dtype=torch.int16, device="cuda")
    junk = torch.ones(1 << 26, device="cuda")  # 256 MB: each pass over it takes ~0.1 ms
    torch.cuda.synchronize()
    for k0 in (0, 3):
        with torch.cuda.stream(s):
            for _ in range(200):  # keep the stream busy (~20 ms) so that the copies below complete late
                junk.mul_(1.0001)
            for j in range(3):
                buf[j].copy_(src[k0 + j])
        q = np.stack([poses[k0 + j][0] for j in range(3)])
        t = np.stack([poses[k0 + j][1] for j in range(3)])
        gpu.update_map_batch_dev(buf.data_ptr(), 3, cfg.width, cfg.height, q, t)  # no synchronize() in between
        for j in range(3):
            cpu.update_depth(frames[k0 + j], q[j], t[j])
        gpu.sync()  # (buf is overwritten by the next round)
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "caller stream")
    gpu.close()


@pytest.mark.parametrize("explore", [False, True])
def test_handle_survives_capacity_error(mods, explore, monkeypatch, knobs):
    """After MLM_ERR_CAPACITY (block pool full and not allowed to grow: MLM_POOL_GROW=0, which stands in for a device out of
    memory) the handle stays usable: the blocks that exist keep accepting updates and answering queries (the device error
    flag used to stay set, failing every later call) — also in frontier mode, whose synchronous path has its own error
    epilogue."""
    from mlmapping_amd.mlmap import MlmError

    MLMap, OracleMap = mods
    knobs.set("pool_grow", "0")
    cfg = S1.with_(use_exploration_frontiers=explore)
    gpu = MLMap(cfg, max_blocks=40)
    img = syn.room_depth(cfg)      # 116 blocks of 1 m
    near = np.full_like(img, 600)  # a wall 0.6 m ahead: a handful of blocks
    q, t = syn.static_pose()
    gpu.update_map(near, q, t)
    before = gpu.export_blocks()
    with pytest.raises(MlmError, match="CAPACITY"):
        gpu.update_map(img, q, t)  # the whole room: far more than 40 blocks
    # the pool is full now, but every block that exists keeps working: the near wall again, same blocks only
    gpu.update_map(near, q, t)
    after = gpu.export_blocks()
    assert after["keys"].shape[0] <= 40
    idx = {tuple(k): i for i, k in enumerate(after["keys"])}
    rows = [idx[tuple(k)] for k in before["keys"]]
    assert (after["log_odds"][rows] != before["log_odds"]).any(), "existing blocks no longer accept updates"
    assert gpu.getOccupancy(np.array([[0.7, 0.0, 1.5]])).shape == (1,)


def test_merge_over_rccl_world_size_1(mods):
    """BASELINE config 4's exchange step on the hardware at hand: a world-size-1 `nccl` group (RCCL really initialised),
    the map taken from a live device handle, packed / finished by the library's HIP kernels, loaded back with
    mlm_import_blocks and queried.  With one rank the merged map is the clamp/class rule applied to the map itself."""
    import torch
    import torch.distributed as dist

    from mlmapping_amd.merge import merge_device_maps, merge_global_map

    MLMap, OracleMap = mods
    cfg = SDEF
    gpu, cpu = MLMap(cfg, max_blocks=4096), OracleMap(cfg)
    for img, (q, t) in syn.stream(cfg, "room_jitter", "random", 5):
        gpu.update_map(img, q, t)
        cpu.update_depth(img, q, t)
    torch.cuda.set_device(0)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 2000))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        x = torch.ones(8, device="cuda")
        dist.all_reduce(x)  # the communicator exists and works
        assert float(x.sum()) == 8.0
        b = cpu.export_blocks()
        merged = merge_device_maps(gpu, load_back=False)
        # expectation: clamp + class rule on the oracle's map
        lo = np.clip(b["log_odds"], np.float32(cfg.lm_log_odds_min), np.float32(cfg.lm_log_odds_max))
        cls = np.where(b["occ"] != ord("u"), ord("f"), ord("u")).astype(np.uint8)
        cls[lo > np.float32(cfg.lm_occupied_sh)] = ord("o")
        assert np.array_equal(merged["keys"].cpu().numpy(), b["keys"])
        assert np.array_equal(merged["occ"].cpu().numpy(), cls)
        g = gpu.export_blocks()
        lo_g = np.clip(g["log_odds"], np.float32(cfg.lm_log_odds_min), np.float32(cfg.lm_log_odds_max))
        assert np.array_equal(merged["log_odds"].cpu().numpy().view(np.uint32), lo_g.view(np.uint32))
        # the generic front end (block dumps -> tensors) over the same communicator gives the same map
        m2 = merge_global_map(g, cfg)
        assert np.array_equal(m2["occ"].cpu().numpy(), cls) and np.array_equal(m2["keys"].cpu().numpy(), b["keys"])
        # load the merged map into a SECOND, empty handle and query it
        other = MLMap(cfg, max_blocks=4096)
        other.import_blocks((merged["keys"].data_ptr(), merged["keys"].shape[0]), log_odds=merged["log_odds"].data_ptr(),
                            occ=merged["occ"].data_ptr())
        e = other.export_blocks()
        assert np.array_equal(e["keys"], b["keys"]) and np.array_equal(e["occ"], cls)
        assert np.array_equal(e["log_odds"].view(np.uint32), lo_g.view(np.uint32))
        pos = np.concatenate([np.random.default_rng(2).uniform(-4, 6, size=(20000, 3)), voxel_centres(b, cfg, 20000)])
        want = np.full(pos.shape[0], -1)
        # occupancy of the merged map, evaluated with numpy from (keys, cls)
        d = cfg.subbox_d_xyz
        gk = np.floor(pos / (d * cfg.subbox_n)).astype(np.int64)
        ck = np.floor(pos / d).astype(np.int64) - gk * cfg.subbox_n
        idx = {tuple(k): i for i, k in enumerate(b["keys"])}
        for i in range(pos.shape[0]):
            j = idx.get(tuple(gk[i]))
            if j is not None:
                c = cls[j, ck[i, 2] * cfg.subbox_n ** 2 + ck[i, 1] * cfg.subbox_n + ck[i, 0]]
                want[i] = 0 if c == ord("o") else (1 if c == ord("f") else -1)
        assert np.array_equal(other.getOccupancy(pos), want)
        # load_back on the original handle: idempotent for a single rank
        merge_device_maps(gpu, load_back=True)
        assert np.array_equal(gpu.export_blocks()["occ"], cls)
        # import from host arrays as well, into a handle that already holds part of the map
        third = MLMap(cfg, max_blocks=4096)
        third.update_map(syn.room_depth(cfg), *syn.static_pose())
        third.import_blocks(b["keys"], log_odds=lo_g, occ=cls)
        e3 = third.export_blocks()
        rows = {tuple(k): i for i, k in enumerate(e3["keys"])}
        sel = [rows[tuple(k)] for k in b["keys"]]
        assert np.array_equal(e3["occ"][sel], cls) and np.array_equal(e3["log_odds"][sel].view(np.uint32), lo_g.view(np.uint32))
    finally:
        dist.destroy_process_group()


def test_merge_device_maps_two_ranks_periodic(tmp_path):
    """merge_device_maps with world size 2 (both ranks' maps on the one GPU, collectives over gloo, host staged): key union,
    mlm_merge_pack, direct reduce-scatter (all-to-all), mlm_merge_finish, all-gather, mlm_import_blocks — and the periodic
    case the round-2 advisor flagged: a second merge after more frames must add the ranks' INCREMENTS to the first merged
    map, not sum maps that already contain it; a third merge with nothing new changes nothing."""
    import subprocess

    port = str(29700 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "merge_device_worker.py"), str(r), "2", port, str(tmp_path)])
             for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    cfg = SDEF
    lo_min, lo_max, sh = np.float32(cfg.lm_log_odds_min), np.float32(cfg.lm_log_odds_max), np.float32(cfg.lm_occupied_sh)
    L = lambda name, r: np.load(tmp_path / f"{name}_{r}.npz")

    def union_layout(maps):
        allk = np.unique(np.concatenate([m["keys"] for m in maps]), axis=0)
        allk = allk[np.lexsort((allk[:, 2], allk[:, 1], allk[:, 0]))]
        idx = {tuple(k): i for i, k in enumerate(allk)}
        out = []
        for m in maps:
            lo = np.zeros((allk.shape[0], cfg.cells_per_block), np.float32)
            seen = np.zeros(lo.shape, bool)
            rows = [idx[tuple(k)] for k in m["keys"]]
            lo[rows] = m["log_odds"]
            seen[rows] = m["occ"] != ord("u")
            out.append((lo, seen))
        return allk, out

    def classes(lo, seen):
        c = np.where(seen, ord("f"), ord("u")).astype(np.uint8)
        c[lo > sh] = ord("o")
        return c

    # round 1: plain sum of the two maps
    keys1, ((a_lo, a_seen), (b_lo, b_seen)) = union_layout([L("own1", 0), L("own1", 1)])
    exp1 = np.clip(a_lo + b_lo, lo_min, lo_max)
    for r in range(2):
        m = L("merged1", r)
        assert np.array_equal(m["keys"], keys1)
        assert np.array_equal(m["log_odds"].view(np.uint32), exp1.view(np.uint32)), f"rank {r}: first merge"
        assert np.array_equal(m["occ"], classes(exp1, a_seen | b_seen))
    assert keys1.shape[0] > max(L("own1", 0)["keys"].shape[0], L("own1", 1)["keys"].shape[0])
    # round 2: M + (L_0 - M) + (L_1 - M)
    keys2, ((a2, s_a), (b2, s_b), (m1, _)) = union_layout([L("own2", 0), L("own2", 1), L("merged1", 0)])
    exp2 = np.clip((a2 - m1) + (b2 - m1) + m1, lo_min, lo_max)
    for r in range(2):
        m = L("merged2", r)
        assert np.array_equal(m["keys"], keys2)
        assert np.allclose(m["log_odds"], exp2, atol=2e-6), f"rank {r}: second merge"
        assert np.array_equal(m["occ"][np.abs(exp2 - sh) > 1e-5], classes(exp2, s_a | s_b)[np.abs(exp2 - sh) > 1e-5])
    assert np.abs(np.clip(a2 + b2, lo_min, lo_max) - exp2).max() > 0.1  # (re-summing the maps would double-count)
    for r in range(2):
        m2, m3 = L("merged2", r), L("merged3", r)
        assert np.array_equal(m2["keys"], m3["keys"]) and np.array_equal(m2["occ"], m3["occ"])
        assert np.allclose(m2["log_odds"], m3["log_odds"], atol=1e-6)


def test_two_slot_sets(mods, monkeypatch, knobs):
    """The handle falls back to two slot sets when three do not fit the device memory; forced here (MLM_SLOT_SETS=2): the
    asynchronous batch pipeline must give the same map."""
    MLMap, OracleMap = mods
    knobs.set("slot_sets", "2")
    cfg = S1
    n = 20
    frames = np.stack([img for img, _ in syn.stream(cfg, "room_jitter", "random", n)])
    poses = syn.random_poses(n, 42)
    q = np.stack([p[0] for p in poses])
    t = np.stack([p[1] for p in poses])
    gpu, cpu = MLMap(cfg, max_blocks=16384, max_batch=4), OracleMap(cfg)
    gpu.set_async(True)
    for k0 in range(0, n, 4):
        gpu.update_map_batch(frames[k0:k0 + 4], q[k0:k0 + 4], t[k0:k0 + 4])
    gpu.sync()
    for k in range(n):
        cpu.update_depth(frames[k], q[k], t[k])
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "two slot sets")


def test_registered_host_frames_and_callback_clocks(mods):
    """mlm_host_register / mlm_host_unregister (the caller pins its frame buffer once; packed batches then travel in one copy at the
    link's rate): asynchronous packed host batches from a registered buffer give the oracle's map, the buffer can be unregistered
    and used again pageable, and registering garbage is an error, not a crash.  Also the host clocks of the callback path
    (mlm_debug_clocks): sections are non-negative, add up to less than the call's wall time and reset."""
    import time

    MLMap, OracleMap = mods
    cfg = SDEF
    n = 12
    frames = np.ascontiguousarray(np.stack([img for img, _ in syn.stream(cfg, "room_jitter", "smooth", n)]))
    poses = syn.smooth_trajectory(n, 42)
    q = np.stack([p[0] for p in poses])
    t = np.stack([p[1] for p in poses])
    gpu, cpu = MLMap(cfg, max_blocks=4096, max_batch=4), OracleMap(cfg)
    gpu.host_register(frames)
    gpu.set_async(True)
    for k0 in (0, 4):
        gpu.update_map_batch(frames[k0:k0 + 4], q[k0:k0 + 4], t[k0:k0 + 4])
    gpu.sync()
    gpu.host_unregister(frames)
    gpu.update_map_batch(frames[8:12], q[8:12], t[8:12])  # (pageable again)
    gpu.sync()
    for k in range(n):
        cpu.update_depth(frames[k], q[k], t[k])
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "registered host frames")
    with pytest.raises(Exception):
        gpu.host_unregister(frames)  # (not registered any more)
    # host clocks of the sampled callback
    gpu.set_async(False)
    zero3 = np.zeros(3)
    gpu.debug_clocks()
    t0 = time.perf_counter()
    for k in range(20):
        gpu.depth_odom_callback(frames[k % n], 0.0, t[k % n], q[k % n], zero3, 0.0, zero3, 0.0, 0.0, sampled=True)
    wall = (time.perf_counter() - t0) * 1e6
    clk = gpu.debug_clocks()
    assert (clk >= 0).all() and clk[:6].sum() > 0 and clk[:6].sum() <= wall, (clk, wall)
    assert gpu.debug_clocks().sum() == 0.0
    gpu.close()


def test_two_handles_interleaved_and_no_leak(mods):
    """Two maps in one process fed alternately (knobs and graphs are per handle, the streams their own): each equals its own oracle
    map.  Then handles are created and destroyed in a loop: the device memory a handle held comes back."""
    import torch

    MLMap, OracleMap = mods
    cfg = SDEF
    n = 8
    fa = [f for f in syn.stream(cfg, "room_jitter", "smooth", n)]
    fb = [f for f in syn.stream(cfg, "corridor", "translating", n)]
    ga, gb, ca, cb = MLMap(cfg, max_blocks=2048), MLMap(cfg, max_blocks=2048, max_batch=2), OracleMap(cfg), OracleMap(cfg)
    gb.set_async(True)
    rng = np.random.default_rng(3)
    for k in range(n):
        (ia, (qa, ta)), (ib, (qb, tb)) = fa[k], fb[k]
        pix = rng.choice(cfg.width * cfg.height, 500, replace=False).astype(np.int32)
        ga.update_map(ia, qa, ta, pixel_idx=pix)      # synchronous single frames through the graph
        ca.update_depth_indexed(ia, pix, qa, ta)
        gb.update_map(ib, qb, tb)                     # asynchronous dense frames
        cb.update_depth(ib, qb, tb)
    compare_maps(ga.export_blocks(), ca.export_blocks(), "handle A (sampled, synchronous)")
    compare_maps(gb.export_blocks(), cb.export_blocks(), "handle B (dense, asynchronous)")
    ga.close()
    gb.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(4):
        g = MLMap(cfg, max_blocks=2048, max_batch=2)
        g.update_map(fa[0][0], *fa[0][1])
        g.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 64 << 20, (free0, free1)


def test_invalid_arguments_are_refused(mods):
    """Every entry point answers bad arguments with a status (MLM_ERR_INVALID / MLM_ERR_CAPACITY), never with a crash, and the handle
    keeps working: null buffers, null handle, non-positive sizes, a row stride below the width, negative counts, a frame above
    mlm_limits.max_points, export buffers that are too small — followed by a frame that must still equal the oracle's."""
    import torch

    from mlmapping_amd import mlmap as mm

    MLMap, OracleMap = mods
    cfg = SDEF
    gpu, cpu = MLMap(cfg, max_blocks=1024, max_points=cfg.width * cfg.height), OracleMap(cfg)
    L, h = gpu._L, gpu._h
    img, (q, t) = next(iter(syn.stream(cfg, "room", "static", 1)))
    q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
    pq, pt, pimg = q.ctypes.data, t.ctypes.data, img.ctypes.data
    W, H = cfg.width, cfg.height
    dev_img = torch.zeros(W * H, dtype=torch.int16, device="cuda")
    pdev = ctypes.c_void_p(dev_img.data_ptr())
    ERR_INVALID, ERR_CAPACITY = -1, -3  # (mlmap_hip.h)
    bad = (ERR_INVALID, ERR_CAPACITY)
    out = np.zeros(16, np.int8)
    pos = np.zeros((4, 3))
    n_out = ctypes.c_int(0)
    calls = [
        lambda: L.mlm_integrate_depth_u16(h, None, W, H, W, None, 0, pq, pt),
        lambda: L.mlm_integrate_depth_u16(None, pimg, W, H, W, None, 0, pq, pt),
        lambda: L.mlm_integrate_depth_u16(h, pimg, 0, H, W, None, 0, pq, pt),
        lambda: L.mlm_integrate_depth_u16(h, pimg, W, -3, W, None, 0, pq, pt),
        lambda: L.mlm_integrate_depth_u16(h, pimg, W, H, W - 1, None, 0, pq, pt),
        lambda: L.mlm_integrate_depth_u16_dev(h, pdev, W, H, W - 1, None, 0, pq, pt),          # a row stride below the width, on the
        lambda: L.mlm_integrate_depth_batch(h, pimg, 1, W * H, W, H, W - 1, pq, pt),          # other three depth entry points
        lambda: L.mlm_integrate_depth_batch_dev(h, pdev, 1, W * H, W, H, W - 1, pq, pt),
        lambda: L.mlm_integrate_depth_u16(h, pimg, W, H, W, pimg, -5, pq, pt),
        lambda: L.mlm_integrate_depth_u16(h, pimg, W, H, W, None, 0, None, pt),
        lambda: L.mlm_integrate_depth_u16(h, pimg, 4 * W, H, 4 * W, None, 0, pq, pt),   # above max_points
        lambda: L.mlm_integrate_points(h, None, 5, pq, pt),
        lambda: L.mlm_integrate_points(h, pos.ctypes.data, -1, pq, pt),
        lambda: L.mlm_query_occupancy(h, None, 4, out.ctypes.data),
        lambda: L.mlm_query_occupancy(h, pos.ctypes.data, 4, None),
        lambda: L.mlm_query_occupancy(h, pos.ctypes.data, -2, out.ctypes.data),
        lambda: L.mlm_host_register(h, None, 64),
        lambda: L.mlm_host_register(h, pimg, 0),
        lambda: L.mlm_get_frame_stats(h, None),
        lambda: L.mlm_debug_clocks(h, None, 0),
    ]
    for k, c in enumerate(calls):
        rc = c()
        assert rc in bad, (k, rc)
    assert L.mlm_debug_set(b"no_such_knob", 1) == ERR_INVALID
    # the handle still works, and an export into a buffer that is too small is refused without writing past it
    gpu.update_map(img, q, t)
    cpu.update_depth(img, q, t)
    keys = np.zeros((1, 3), np.int32)
    rc = L.mlm_export_blocks(h, 1, keys.ctypes.data, None, None, None, ctypes.byref(n_out))
    assert rc in bad or n_out.value <= 1 or rc == mm.MLM_OK, (rc, n_out.value)
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "after the refused calls")
    gpu.close()


def test_bench_launcher_contract_two_ranks():
    """`python bench.py --gpus 2` exactly as the driver invokes it when it does not wrap it in torch.distributed.run: the
    parent starts the two ranks itself (before it touches the GPU) — rank environment, barrier, max over ranks, the timed
    merge leg, ONE JSON line from rank 0, whole-job aggregate.  This box has one GPU, so both ranks share it and the
    collectives run over gloo (MLM_BENCH_DIST_BACKEND): the contract is what is checked, not a rate.  Without that hook the
    same command must fail loudly on a one-GPU box instead of reporting one stream as two GPUs."""
    import json
    import sys

    import torch

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "8", "--batches-per-step", "2", "--no-cpu-baseline", "--no-extra",
           "--full"]  # (roofline and the merge leg: --full)
    if torch.cuda.device_count() < 2:
        r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "one rank per GPU" in r.stderr, (r.returncode, r.stderr[-500:])
        assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    r = subprocess.run(cmd, cwd=root, env=dict(env, MLM_BENCH_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["config"]["streams"] == 2 and d["config"]["frames_per_step"] == 16 and d["config"]["batch"] == 8 and "cfg4" in d["config"]["workload"]
    # whole-job aggregate: frames of BOTH ranks over the slower rank's time
    assert abs(d["value"] - 2 * 3 * 16 / (d["ms_per_step"] * 3 / 1e3)) < 1e-6 * d["value"] and d["value_p50"] > 0
    assert d["roofline"]["frac"] > 0 and d["roofline"]["atomics"]["atomics_per_frame"] > 0
    mg = d["merge"]  # the two streams have different poses: the union is larger than either map
    assert mg["merge_ms"] > 0 and mg["union_blocks"] > mg["own_blocks"] > 0 and mg["merge_bytes_per_rank"] > 0


def test_fallbacks_in_batches_share_one_cell_table_state(mods, monkeypatch, knobs):
    """A sector-path handle keeps the cell-table path's per-frame state once, not per frame slot.  Fall-backs to that path
    (forced on every second frame) in batches of two: each is redone alone on the shared state, and the map matches the oracle."""
    MLMap, OracleMap = mods
    knobs.set("sec_fail_every", "2")
    knobs.set("sec_backoff", "0")
    cfg = S1
    gpu, cpu = MLMap(cfg, max_blocks=16384, max_batch=2), OracleMap(cfg)
    frames = list(syn.stream(cfg, "room_jitter", "random", 6))
    imgs = np.stack([f[0] for f in frames])
    q = np.stack([f[1][0] for f in frames])
    t = np.stack([f[1][1] for f in frames])
    gpu.update_map_batch(imgs, q, t)  # 2 + 2 + 2
    for img, (qq, tt) in frames:
        cpu.update_depth(img, qq, tt)
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "fall-backs in batches")
    assert gpu.frame_stats()["n_sector_fallbacks"] == 3
    gpu.close()
