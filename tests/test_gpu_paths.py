"""mlm_query_paths on the GPU: paths through a parent field, traced and shortened (include/mlmap_hip.h).  The fields of
tests/path_cases.py — the ones the CPU driver runs in tests/test_path_plan.py — go as byte arrays into a handle with a small map (the
call reads no map state) three ways: device pointers for everything (the kernel k_paths), parent on the device with goals and
outputs in host memory (the kernel, staged), parent in host memory (the host branch).  All three must give tests/path_ref.py's bytes,
length by its 64 bits.  Then chunking by the scratch bound, one end-to-end run on a real map (export_route / export_reach into a
device tensor, paths on that pointer, reference on the downloaded field), the contract's refusals and the scratch's size."""
import ctypes

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import path_cases as pc
from tests import path_ref as ref

pytestmark = pytest.mark.gpu

SCRATCH_BOUND = 256 << 20  # include/mlmap_hip.h: "chunks of goals of at most 256 MiB"
ERR_INVALID = -1


@pytest.fixture(scope="module")
def gpu():
    from mlmapping_amd.mlmap import MLMap

    m = MLMap(S1, max_blocks=256)
    yield m
    m.close()


def to_numpy(out):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in out.items()}


def call(gpu, c, parent, goals, outs):
    """the C call on pointers: parent / goals / outs are numpy arrays (host memory) or torch device tensors"""
    def p(a):
        return None if a is None else a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()

    gpu.query_paths_dev(c["lo"], c["parent"].shape[::-1], p(parent), p(goals), len(c["goals"]), kind=c["kind"], lookahead=c["lookahead"],
                        max_moves=c["max_moves"], cap=c["cap"], status=p(outs["status"]), way=p(outs["way"]) if c["cap"] else None,
                        length=p(outs["length"]), table=p(outs["table"]))
    return to_numpy(outs)


def host_outs(c):
    n = len(c["goals"])
    return {"status": np.full(n, 77, np.int8), "way": c["fill"].copy(), "length": np.full(n, 7.0), "table": np.full((n, 8), 7, np.int64)}


def dev_outs(c):
    import torch

    return {k: torch.from_numpy(v).cuda() for k, v in host_outs(c).items()}


def three_ways(gpu, c):
    import torch

    exp = pc.answer(c)
    parent_dev, goals_dev = torch.from_numpy(c["parent"]).cuda(), torch.from_numpy(c["goals"]).cuda()
    pc.assert_same(call(gpu, c, parent_dev, goals_dev, dev_outs(c)), exp, (c["name"], "kernel"))
    pc.assert_same(call(gpu, c, parent_dev, c["goals"], host_outs(c)), exp, (c["name"], "kernel, staged"))
    pc.assert_same(call(gpu, c, c["parent"], c["goals"], host_outs(c)), exp, (c["name"], "host branch"))
    # mixed: host field with device goals and outputs; device field with host goals and device outputs
    pc.assert_same(call(gpu, c, c["parent"], goals_dev, dev_outs(c)), exp, (c["name"], "host branch, device outputs"))
    mixed = dev_outs(c)
    mixed["status"], mixed["table"] = host_outs(c)["status"], host_outs(c)["table"]
    pc.assert_same(call(gpu, c, parent_dev, c["goals"], mixed), exp, (c["name"], "kernel, mixed"))


@pytest.mark.parametrize("group", ["random", "maze", "slab", "hand", "cap"])
def test_three_ways_equal_reference(gpu, group):
    cases = [c for c in pc.build() if c["group"] == group]
    assert cases
    for c in cases:
        three_ways(gpu, c)


def test_binding_numpy_and_torch(gpu):
    """MLMap.query_paths: numpy in, numpy out; device tensors in, device tensors out; a subset of the outputs"""
    import torch

    c = next(c for c in pc.build() if c["name"].endswith("-L16") and c["kind"] == ref.ROUTE)
    exp = ref.query(c["parent"], c["kind"], c["lo"], c["goals"], 16, 4096, 5, pc.D_SUB)
    dims = c["parent"].shape[::-1]
    a = gpu.query_paths(c["lo"], dims, c["parent"], c["goals"], "route", 16, 4096, 5)
    assert all(isinstance(v, np.ndarray) for v in a.values())
    pc.assert_same(a, exp, "numpy")
    b = gpu.query_paths(c["lo"], dims, torch.from_numpy(c["parent"]).cuda(), torch.from_numpy(c["goals"]).cuda(), ref.ROUTE, 16, 4096, 5)
    assert all(v.is_cuda for v in b.values())
    pc.assert_same(to_numpy(b), exp, "torch")
    only = gpu.query_paths(c["lo"], dims, torch.from_numpy(c["parent"]).cuda(), c["goals"], lookahead=16, outputs=("length", "table"))
    assert sorted(only) == ["length", "table"]
    assert np.array_equal(only["table"], exp["table"]) and np.array_equal(only["length"].view(np.uint64), exp["length"].view(np.uint64))


def test_chunks_by_the_scratch_bound():
    """max_moves = 2^20: 12 MiB of path scratch per goal, so 64 goals run in chunks of 21 — same answers, scratch within the bound"""
    import torch

    from mlmapping_amd.mlmap import MLMap

    base = next(c for c in pc.build() if c["name"] == "slab-L64")
    rng = np.random.default_rng(4)
    goals = np.stack([rng.integers(200, size=64), rng.integers(70, size=64), rng.integers(2, size=64)], axis=1)
    c = pc.case("slab-chunks", "chunks", base["parent"], ref.ROUTE, (0, 0, 0), goals, 64, 1 << 20, cap=3)
    per_goal = 12 * ((1 << 20) + 1)
    assert 1 < SCRATCH_BOUND // per_goal < 64
    m = MLMap(S1, max_blocks=256)
    try:
        before = m.frame_stats()["device_bytes"]
        three_ways(m, c)
        grown = m.frame_stats()["device_bytes"] - before
        stage = 64 * (85 + 12 * 3) + 5 * 256  # (the staged channels of at most 64 goals, each rounded up to 256 bytes)
        print(f"device_bytes grew by {grown}")
        assert SCRATCH_BOUND - per_goal < grown <= SCRATCH_BOUND + stage
        small = pc.case("slab-chunks-small", "chunks", base["parent"], ref.ROUTE, (0, 0, 0), goals, 64, 4096, cap=3)
        pc.assert_same(call(m, small, torch.from_numpy(small["parent"]).cuda(), torch.from_numpy(small["goals"]).cuda(), dev_outs(small)),
                       pc.answer(c), "max_moves 4096")
        assert m.frame_stats()["device_bytes"] - before == grown  # (kept, not grown again)
    finally:
        m.close()


def test_scratch_growth_is_bounded():
    """a fresh handle: the first call takes 12 bytes x (max_moves + 1) per goal and nothing else with device pointers"""
    import torch

    from mlmapping_amd.mlmap import MLMap

    m = MLMap(S1, max_blocks=256)
    try:
        c = next(c for c in pc.build() if c["name"] == "slab-L64")
        before = m.frame_stats()["device_bytes"]
        pc.assert_same(call(m, c, torch.from_numpy(c["parent"]).cuda(), torch.from_numpy(c["goals"]).cuda(), dev_outs(c)), pc.answer(c), "fresh")
        grown = m.frame_stats()["device_bytes"] - before
        assert 0 < grown <= 12 * (c["max_moves"] + 1) * len(c["goals"])
        call(m, c, c["parent"], c["goals"], host_outs(c))  # the host branch takes no device memory
        assert m.frame_stats()["device_bytes"] - before == grown
    finally:
        m.close()


def test_real_map_end_to_end():
    """the synthetic corridor, a route field (26-connected, clearance 1, one penalty ring) and a reach field around the vehicle in
    device tensors, about 500 reached goals each, against the reference on the downloaded field; route_paths gives the same"""
    import torch

    from mlmapping_amd.mlmap import MLMap

    m = MLMap(S1, max_blocks=8192)
    try:
        for img, (q, t) in syn.stream(S1, "corridor", "smooth", 4):
            m.update_map(img, q, t)
        vehicle = np.array([int(np.floor(v / S1.subbox_d_xyz)) for v in t])
        lo, dims = vehicle - [48, 48, 8], (96, 96, 16)
        off = np.array([(x, y, z) for z in (-1, 0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1)])
        seeds = torch.from_numpy((vehicle + off).astype(np.int32)).cuda()  # (a seed that is not traversable contributes nothing)
        field = torch.empty(dims[::-1], dtype=torch.uint8, device="cuda")
        rng = np.random.default_rng(1)
        for kind, export in ((ref.ROUTE, lambda: m.export_route_dev(lo, dims, seeds.data_ptr(), 27, clearance=1, connectivity=26, penalty=(20,),
                                                                    parent=field.data_ptr(), summary=True)),
                             (ref.REACH, lambda: m.export_reach_dev(lo, dims, seeds.data_ptr(), 27, clearance=1, parent=field.data_ptr(), summary=True))):
            summary = export()
            parent = field.cpu().numpy()
            reached = np.argwhere(parent <= ref.seed_code(kind))[:, ::-1]
            print(f"kind {kind}: summary {summary}, reached {len(reached)}")
            assert len(reached) > 2000 and len(reached) == summary[1]
            goals = np.ascontiguousarray((reached[rng.choice(len(reached), size=500, replace=False)] + lo).astype(np.int32))
            exp = ref.query(parent, kind, lo, goals, 32, 4096, 16, S1.subbox_d_xyz)
            assert (exp["status"] == 1).all() and (exp["table"][:, 1] < exp["table"][:, 0]).sum() > 100  # (genuine field; many paths shortened)
            got = m.query_paths(lo, dims, field, torch.from_numpy(goals).cuda(), kind, 32, 4096, 16)
            pc.assert_same(to_numpy(got), exp, ("real map", kind))
            pc.assert_same(m.query_paths(lo, dims, parent, goals, kind, 32, 4096, 16), exp, ("real map, host branch", kind))
            if kind == ref.ROUTE:
                both = m.route_paths(lo, dims, seeds, torch.from_numpy(goals).cuda(), clearance=1, connectivity=26, penalty=(20,), lookahead=32,
                                     max_moves=4096, cap=16)
                assert np.array_equal(both.pop("summary")[:3], summary[:3])
                pc.assert_same(to_numpy(both), exp, "route_paths")
                again = m.route_paths(lo, dims, (vehicle + off), goals, clearance=1, connectivity=26, penalty=(20,), lookahead=32, max_moves=4096, cap=16)
                again.pop("summary")
                pc.assert_same(again, exp, "route_paths, numpy")
    finally:
        m.close()


def test_refusals_leave_the_handle_usable(gpu):
    import torch

    from mlmapping_amd.mlmap import MLM_OK, _p

    L, h = gpu._L, gpu._h
    c = next(c for c in pc.build() if c["name"] == "hand-tie2-open")
    lo, dims = c["lo"].copy(), np.array(c["parent"].shape[::-1], dtype=np.int32)
    par_h, goals_h = c["parent"], c["goals"]
    par_d, goals_d = torch.from_numpy(par_h).cuda(), torch.from_numpy(goals_h).cuda()
    n = len(goals_h)
    st, way, ln, tb = np.zeros(n, np.int8), np.zeros((n, 4, 3), np.int32), np.zeros(n), np.zeros((n, 8), np.int64)

    def q(lo_=lo, dims_=dims, parent=par_h, kind=1, goals=goals_h, n_=n, L_=8, mm=16, cap=4, status=st, way3=way, length=ln, table=tb):
        ptr = [None if a is None else _p(a) if isinstance(a, np.ndarray) else ctypes.c_void_p(a.data_ptr()) for a in (lo_, dims_, parent)]
        g = None if goals is None else _p(goals) if isinstance(goals, np.ndarray) else ctypes.c_void_p(goals.data_ptr())
        outs = [None if a is None else _p(a) for a in (status, way3, length, table)]
        return L.mlm_query_paths(h, *ptr, kind, g, n_, L_, mm, cap, *outs)

    big = np.array([2 ** 31 - 2, 0, 0], dtype=np.int32)
    bad = [dict(lo_=None), dict(dims_=None), dict(dims_=np.array([3, 0, 1], dtype=np.int32)), dict(dims_=np.array([3, 3, -1], dtype=np.int32)),
           dict(lo_=big), dict(dims_=np.array([2048, 2048, 2048], dtype=np.int32)), dict(parent=None), dict(kind=2), dict(kind=-1), dict(n_=-1),
           dict(goals=None), dict(L_=0), dict(L_=4097), dict(mm=0), dict(mm=(1 << 20) + 1), dict(cap=-1), dict(cap=0), dict(cap=4, way3=None),
           dict(status=None, way3=None, length=None, table=None, cap=0)]
    for parent in (par_h, par_d):
        for kw in bad:
            kw = dict(kw)
            kw.setdefault("parent", parent)
            assert q(**kw) == ERR_INVALID, kw
        assert q(parent=parent, n_=0) == MLM_OK and q(parent=parent, n_=0, goals=None) == MLM_OK
        assert q(parent=parent, L_=4096, mm=1 << 20) == MLM_OK
        assert q(parent=parent, cap=0, way3=None) == MLM_OK
    # the handle answers as before
    three_ways(gpu, c)
    exp = pc.answer(c)
    assert q(parent=par_d, goals=goals_d, cap=4) == MLM_OK and np.array_equal(st, exp["status"]) and np.array_equal(tb, exp["table"])
