"""mlm_query_clearance: exact segment casts through a distance field (include/mlmap_hip.h), every output held byte for byte to the
contract written in plain Python integers (tests/clearance_ref.py).  Every case runs three ways — a small batch in host memory (the
host branch: no launch), device tensors for every pointer (the kernels k_clearance / k_clearance_groups), and host memory again after
set_host_mirror_limit(0) (the kernels, staged) — and all three must give the reference's bytes; the kernel legs run with a look-ahead
of 1 and of 4 voxels (knob "clear_ahead").  Then agreement with the existing calls on real maps: with a field of mlm_export_esdf the
walk reproduces mlm_query_sweeps' and mlm_query_rays' stop bytes."""
import ctypes
import functools

import numpy as np
import pytest

from mlmapping_amd.config import S1
from tests import clearance_ref as cr
from tests.test_clearance_plan import BOXES, by_hand, centre, random_groups
from tests.test_gpu_nearest import CUBE3, dump, kw, load, to_numpy

pytestmark = pytest.mark.gpu

D, N = S1.subbox_d_xyz, S1.subbox_n
SX = S1.with_(use_exploration_frontiers=True)  # released blocks answer from element 0 only in frontier mode
S5 = SX.with_(subbox_n=5)
CHUNK = 1 << 18        # rays per launch when host memory is staged
HOST_RAYS, HOST_VOXELS = 64, 1 << 18  # the host branch's bounds
STOPS = ((-1, 64), (9, 64), (100, 9), (1 << 20, 1 << 20))  # sq_stop, sq_cap


@pytest.fixture(scope="module")
def MLMap():
    from mlmapping_amd.mlmap import MLMap

    return MLMap


def handles(MLMap, knobs, ahead, cfg=S1):
    """(a handle, a handle after set_host_mirror_limit(0)), both with the look-ahead `ahead`"""
    knobs.set("clear_ahead", ahead)
    a, b = MLMap(cfg, max_blocks=256), MLMap(cfg, max_blocks=256)
    b.set_host_mirror_limit(0)
    return a, b


def path_voxels(p0, p1, d=D):
    out = []
    for a, b in zip(p0, p1):
        Q = cr.rw.valid(a, b, d)
        out.append(0 if Q is None else 1 + sum(abs((Q[1][k] >> 10) - (Q[0][k] >> 10)) for k in range(3)))
    return out


def on_host(gpu, p0, p1, lo, dims, field, stop, cap, op, gb):
    """the batch in host memory: as one call with its groups where the host branch takes it whole, else in pieces it takes (at most 64
    rays and 2^18 path voxels), without groups; every piece must have been answered without a launch"""
    work = path_voxels(p0, p1)
    call = lambda i, j, g: gpu.query_clearance(p0[i:j], p1[i:j], lo, dims, field, stop, cap, op, g)
    if len(p0) <= HOST_RAYS and sum(work) <= HOST_VOXELS:
        before = gpu.frame_stats()["n_host_queries"]
        out = call(0, len(p0), gb)
        assert gpu.frame_stats()["n_host_queries"] == before + len(p0), "the batch was not answered on the host"
        return out
    parts, i = [], 0
    while i < len(p0):
        m, tot = 0, 0
        while i + m < len(p0) and m < HOST_RAYS and tot + work[i + m] <= HOST_VOXELS:
            tot += work[i + m]
            m += 1
        before = gpu.frame_stats()["n_host_queries"]
        parts.append(call(i, i + max(m, 1), None))
        assert gpu.frame_stats()["n_host_queries"] == before + m, "a piece was not answered on the host, or one beyond the bounds was"
        i += max(m, 1)
    return {k: np.concatenate([p[k] for p in parts]) for k in cr.OUTPUTS}


def three_ways(pair, p0, p1, lo, dims, field, stop, cap, op, gb, exp, what):
    import torch

    gpu, staged = pair
    p0, p1 = np.ascontiguousarray(p0, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(p1, dtype=np.float64).reshape(-1, 3)
    field = np.ascontiguousarray(field, dtype=np.int32)
    cr.assert_equal(on_host(gpu, p0, p1, lo, dims, field, stop, cap, op, gb), exp, f"host {what}")
    dev = gpu.query_clearance(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), lo, dims, torch.from_numpy(field).cuda(), stop, cap, op,
                              None if gb is None else torch.from_numpy(np.asarray(gb, dtype=np.int32)).cuda())
    assert gb is None or "table" in dev
    cr.assert_equal(to_numpy(dev), exp, f"device tensors {what}")
    before = staged.frame_stats()["n_host_queries"]
    got = staged.query_clearance(p0, p1, lo, dims, field, stop, cap, op, gb)
    assert staged.frame_stats()["n_host_queries"] == before
    assert gb is None or "table" in got
    cr.assert_equal(got, exp, f"staged kernel {what}")


def close(pair):
    for g in pair:
        g.close()


# ---- an answer written by hand ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ahead", [1, 4])
def test_by_hand(MLMap, knobs, ahead):
    """an 8 x 4 x 4 field, 50 everywhere but 9, 4, 0 at x = 3, 4, 5 of the row y = z = 1; a segment along x from voxel 1 to voxel 7 with
    sq_stop 0 and sq_cap 16: stopped at (5, 1, 1), entered at 3584 / 6144, 4 voxels passed with f = 16, 16, 9, 4"""
    lo, dims, f, a, b = by_hand(D)
    exp = {"status": np.array([1], np.int8), "voxel": np.array([[5, 1, 1]], np.int32), "t": np.array([3584 / 6144]), "n_steps": np.array([4], np.int32),
           "min_sq": np.array([0], np.int32), "min": np.array([[5, 1, 1]], np.int32), "cost": np.array([19], np.int64), "n_near": np.array([2], np.int32),
           "table": np.array([[1, 0, 1, 0, 0, 19, 4, 2]], np.int64)}
    pair = handles(MLMap, knobs, ahead)
    three_ways(pair, a, b, lo, dims, f, 0, 16, False, [0, 1], exp, "by hand")
    close(pair)


# ---- the shapes of the host test ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_cases(bi):
    """the field, the segments, the groups and the reference's answers of box bi, computed once"""
    lo, dims = BOXES[bi]
    rng = np.random.default_rng(100 + bi)
    field = cr.wild_field(rng, dims)
    p0, p1 = cr.segments(rng, lo, dims, D, 64)
    gb = random_groups(rng, len(p0))
    k = next(k for k in range(2, len(gb) - 1) if gb[k + 1] > gb[k])
    p0[gb[k]] = [np.nan, 0.0, 0.0]  # (a first segment that is invalid)
    cases = []
    for stop, cap in STOPS:
        for op in (False, True):
            exp = cr.clearance_all(p0, p1, D, lo, dims, field, stop, cap, op)
            exp["table"] = cr.group_rows(exp, gb)
            cases.append((stop, cap, op, exp))
    return lo, dims, field, p0, p1, gb, cases


@pytest.mark.parametrize("ahead", [1, 4])
@pytest.mark.parametrize("bi", range(len(BOXES)))
def test_shapes(MLMap, knobs, bi, ahead):
    """arbitrary int32 fields over boxes (1, 1, 1), (5, 3, 2), (8, 4, 4) and (13, 9, 6) with lo negative and across 0; segments that start
    outside, leave, pass through the outside, zero-length, grazing and invalid ones; sq_stop -1 and >= sq_cap; groups with an empty
    one, single segments, an invalid first segment and trailing rays in no group"""
    lo, dims, field, p0, p1, gb, cases = shape_cases(bi)
    pair = handles(MLMap, knobs, ahead)
    seen = set()
    for stop, cap, op, exp in cases:
        three_ways(pair, p0, p1, lo, dims, field, stop, cap, op, gb, exp, f"box {bi} sq_stop={stop} sq_cap={cap} outside_pass={op}")
        seen |= {int(s) for s in np.unique(exp["status"])}
    assert seen == {-1, 0, 1, 2}
    close(pair)


@pytest.mark.parametrize("ahead", [1, 4])
def test_batch_sizes(MLMap, knobs, ahead):
    """n = 1, 63, 64, 65 and 257 rays of one set: the host branch's bound, a partial wave, more than one workgroup"""
    lo, dims = (-6, -5, -4), (14, 11, 9)
    rng = np.random.default_rng(9)
    field = cr.wild_field(rng, dims)
    p0 = rng.uniform((np.array(lo) - 1) * D, (np.array(lo) + dims + 1) * D, size=(257, 3))
    p1 = rng.uniform((np.array(lo) - 1) * D, (np.array(lo) + dims + 1) * D, size=(257, 3))
    full = cr.clearance_all(p0, p1, D, lo, dims, field, 2, 64)
    assert {int(s) for s in np.unique(full["status"])} == {0, 1, 2}
    pair = handles(MLMap, knobs, ahead)
    for n in (1, 63, 64, 65, 257):
        exp = {k: v[:n] for k, v in full.items()}
        gb = [0, n] if n < 63 else [0, 3, 3, n // 2, n - 1]
        exp["table"] = cr.group_rows(exp, gb)
        three_ways(pair, p0[:n], p1[:n], lo, dims, field, 2, 64, False, gb, exp, f"n={n}")
    close(pair)


def test_two_chunks_and_a_group_across_the_boundary(MLMap, knobs):
    """2^18 + 1 zero-length segments in host memory, mirror limit 0: two launches; nothing stops a segment, so the group that begins
    three rays before the chunk boundary sums words of both chunks"""
    lo, dims = (-2, -1, 0), (5, 3, 2)
    field = np.arange(30, dtype=np.int32).reshape(2, 3, 5) - 4
    pts = np.concatenate([centre([(-2, -1, 0), (2, 1, 1), (0, 0, 1), (7, 7, 7)], D), [[np.nan, 0.0, 0.0]]])
    one = cr.clearance_all(pts, pts, D, lo, dims, field, -1, 20, True)
    assert one["status"].tolist() == [0, 0, 0, 0, -1] and one["cost"].tolist() == [20, 0, 2, 0, 0]
    n = CHUNK + 1
    idx = np.arange(n) % 4  # (the invalid one only in front: it would end a group's count)
    idx[0] = 4
    exp = {k: v[idx] for k, v in one.items()}
    gb = np.array([0, 1, 5, CHUNK - 3, n], dtype=np.int32)
    exp["table"] = cr.group_rows(exp, gb)
    assert exp["table"][0].tolist() == [1, 0, -1, -1, -1, 0, 0, 0] and exp["table"][3, :3].tolist() == [4, -1, 0] and exp["table"][3, 6] == 4
    assert exp["table"][2, 0] == CHUNK - 8 and exp["table"][2, 1] == -1 and exp["table"][2, 6] == CHUNK - 8
    p = np.ascontiguousarray(pts[idx])
    knobs.set("clear_ahead", 4)
    gpu = MLMap(S1, max_blocks=256)
    gpu.set_host_mirror_limit(0)
    before = gpu.frame_stats()["device_bytes"]
    got = gpu.query_clearance(p, p, lo, dims, field, -1, 20, True, gb)
    assert gpu.frame_stats()["device_bytes"] - before >= 101 * CHUNK + 21 * n  # (the staging of one chunk and the groups' scratch are counted)
    assert gpu.frame_stats()["n_host_queries"] == 0
    cr.assert_equal(got, exp, "two chunks")
    gpu.close()


def test_pointers_each_on_their_own(MLMap, knobs):
    """group_begin in device memory beside host rays; the field in host memory against the field in device memory; single outputs and
    the table alone: the same bytes every time"""
    import torch

    lo, dims, field, p0, p1, gb, cases = shape_cases(2)
    stop, cap, op, exp = cases[2]
    gpu = MLMap(S1, max_blocks=256)
    gbt = torch.from_numpy(gb).cuda()
    before = gpu.frame_stats()["n_host_queries"]
    a = gpu.query_clearance(p0, p1, lo, dims, field, stop, cap, op, gbt)  # host rays, field and table, device group_begin
    assert isinstance(a["table"], np.ndarray) and isinstance(a["status"], np.ndarray)
    cr.assert_equal(a, exp, "device group_begin")
    b = gpu.query_clearance(p0, p1, lo, dims, torch.from_numpy(field).cuda(), stop, cap, op, gb)  # device field, everything else host
    cr.assert_equal(b, exp, "device field")
    c = gpu.query_clearance(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), lo, dims, field, stop, cap, op, gbt)  # host field
    d = gpu.query_clearance(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), lo, dims, torch.from_numpy(field).cuda(), stop, cap, op, gbt)
    for k in cr.OUTPUTS + ("table",):
        assert c[k].cpu().numpy().tobytes() == d[k].cpu().numpy().tobytes() == exp[k].tobytes(), k
    assert gpu.frame_stats()["n_host_queries"] == before  # (none of these was all in host memory)
    for k in cr.OUTPUTS:  # one output, each in turn; then the table alone
        one = gpu.query_clearance(p0[:40], p1[:40], lo, dims, field, stop, cap, op, outputs=(k,))
        assert list(one) == [k] and one[k].tobytes() == exp[k][:40].tobytes(), k
    for pts in ((p0, p1), (torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda())):
        only = to_numpy(gpu.query_clearance(*pts, lo, dims, field, stop, cap, op, gb, outputs=()))
        assert list(only) == ["table"] and only["table"].tobytes() == exp["table"].tobytes()
    gpu.close()


def test_arguments(MLMap, knobs):
    """every MLM_ERR_INVALID of the contract, with the handle usable afterwards; n == 0"""
    lo_t, dims_t, f, a, b = by_hand(D)
    for mirror in (1, 0):
        knobs.set("mirror", mirror)
        gpu = MLMap(S1, max_blocks=256)
        L, h = gpu._L, gpu._h
        P = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
        p0, p1 = np.ascontiguousarray(np.tile(a, (3, 1))), np.ascontiguousarray(np.tile(b, (3, 1)))
        lo, dims = np.array(lo_t, np.int32), np.array(dims_t, np.int32)
        outs = [np.zeros(3, np.int8), np.zeros((3, 3), np.int32), np.zeros(3), np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros((3, 3), np.int32),
                np.zeros(3, np.int64), np.zeros(3, np.int32)]
        gb, table = np.array([0, 2, 3], np.int32), np.zeros((2, 8), np.int64)

        def call(a=p0, c=p1, n=3, lo=lo, dims=dims, f=f, stop=0, cap=16, flags=0, o=outs, gb=gb, ng=2, table=table):
            return L.mlm_query_clearance(h, P(a), P(c), n, P(lo), P(dims), P(f), stop, cap, flags, *[P(x) for x in o], P(gb), ng, P(table))

        i32 = lambda *v: np.array(v, np.int32)
        bad = [lambda: call(n=-1), lambda: call(a=None), lambda: call(c=None), lambda: call(lo=None), lambda: call(dims=None), lambda: call(f=None),
               lambda: call(dims=i32(8, 0, 4)), lambda: call(dims=i32(8, -1, 4)), lambda: call(lo=i32(2 ** 31 - 4, 0, 0)),
               lambda: call(dims=i32(2048, 2048, 2048)), lambda: call(stop=-2), lambda: call(stop=(1 << 20) + 1), lambda: call(cap=0),
               lambda: call(cap=(1 << 20) + 1), lambda: call(flags=2), lambda: call(flags=-1), lambda: call(flags=1 | 1 << 20),
               lambda: call(o=[None] * 8, gb=None, table=None), lambda: call(gb=None), lambda: call(table=None), lambda: call(ng=-1),
               lambda: call(gb=i32(-1, 2, 3)), lambda: call(gb=i32(0, 2, 1)), lambda: call(gb=i32(0, 2, 4))]
        for k, fn in enumerate(bad):
            assert fn() == -1, k
            assert b"mlm_query_clearance" in L.mlm_last_error(h), k
            assert call() == 0  # (the handle is usable afterwards)
        assert outs[0].tolist() == [1, 1, 1] and outs[3].tolist() == [4, 4, 4] and table.tolist() == [[2, 0, 1, 0, 0, 19, 4, 2], [1, 0, 1, 0, 0, 19, 4, 2]]
        assert call(a=None, c=None, n=0, gb=None, ng=0, table=None) == 0  # n == 0, no groups
        assert call(a=None, c=None, n=0, gb=i32(0), ng=0) == 0
        table[...] = 7
        assert call(a=None, c=None, n=0, gb=i32(0, 0, 0)) == 0 and table.tolist() == [[0, -1, 0, -1, -1, 0, 0, 0]] * 2  # (empty groups have rows)
        assert call(o=[None] * 8) == 0  # the table alone is an output
        assert gpu.frame_stats()["n_host_queries"] > 0 if mirror else gpu.frame_stats()["n_host_queries"] == 0
        gpu.close()


# ---- agreement with the existing calls on real maps ----------------------------------------------------------------------------
def real_map(which):
    """(block dump, config, box lo, box dims): 3 x 3 x 3 blocks written voxel by voxel — subbox_n 10, or subbox_n 5 in frontier mode with
    a released block whose element 0 is OCCUPIED and one whose element 0 is FREE"""
    rng = np.random.default_rng(60 + which)
    n = N if which == 0 else 5
    lo, hi = -n, 2 * n
    vox = lambda count: rng.integers(lo, hi, size=(count, 3))
    released = None if which == 0 else {(1, 0, -1): "o", (-1, 1, 0): "f"}
    free = [g for g in CUBE3 if not released or g not in released]
    b = dump(vox(60 if which == 0 else 12), free, inflated=vox(40 if which == 0 else 20), unknown=vox(120 if which == 0 else 30), released=released, n=n)
    return b, (S1 if which == 0 else S5), np.full(3, lo, np.int64), np.full(3, hi - lo, np.int64)


@pytest.mark.parametrize("which", [0, 1], ids=["n10", "n5 with released blocks"])
def test_agrees_with_sweeps_and_rays_on_a_map(MLMap, knobs, which):
    """both end points of every segment inside the exported box, so every path lies in it.  r in {1, 3}: export_esdf at max_dist r + 1,
    sq_stop r^2: status, voxel, t and n_steps are query_sweeps' bytes and min_sq at a stop is hit_sq.  r = 0: max_dist 1, sq_stop 0:
    they are cast_rays' bytes for OCC, OCC | INFL and UNKNOWN"""
    import torch

    b, cfg, lo, dims = real_map(which)
    d = cfg.subbox_d_xyz
    rng = np.random.default_rng(70 + which)
    p0, p1 = rng.uniform(lo * d, (lo + dims) * d, size=(300, 3)), rng.uniform(lo * d, (lo + dims) * d, size=(300, 3))
    p1[::3] = p0[::3] + rng.uniform(-4 * d, 4 * d, size=p1[::3].shape)  # (short edges too)
    p1 = np.clip(p1, lo * d + 1e-9, (lo + dims) * d - 1e-9)
    t0, t1 = torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda()
    same = ("status", "voxel", "t", "n_steps")
    for ahead in (1, 4):
        knobs.set("clear_ahead", ahead)
        gpu = load(MLMap, b, cfg)
        for r in (1, 3):
            field = torch.empty((int(dims[2]), int(dims[1]), int(dims[0])), dtype=torch.int32, device="cuda")
            gpu.export_esdf_dev(lo, dims, r + 1, sqdist=field.data_ptr())
            ref = to_numpy(gpu.query_sweeps(t0, t1, r))
            got = to_numpy(gpu.query_clearance(t0, t1, lo, dims, field, r * r, (r + 1) ** 2))
            host = gpu.query_clearance(p0[:64], p1[:64], lo, dims, field.cpu().numpy(), r * r, (r + 1) ** 2)
            for k in same:
                assert got[k].tobytes() == ref[k].tobytes(), (ahead, r, k)
                assert host[k].tobytes() == ref[k][:64].tobytes(), (ahead, r, k, "host")
            stop = ref["status"] == 1
            assert stop.sum() >= 5 and (~stop).sum() >= 5 and (stop & (ref["n_steps"] > 0)).sum() >= 5, (stop.sum(), (~stop).sum())
            assert np.array_equal(got["min_sq"][stop], ref["hit_sq"][stop]) and (got["min_sq"][~stop] > r * r).all()
            assert not (got["status"] == 2).any()
        for f in (1, 3, 4):
            field = torch.empty((int(dims[2]), int(dims[1]), int(dims[0])), dtype=torch.int32, device="cuda")
            gpu.export_esdf_dev(lo, dims, 1, sqdist=field.data_ptr(), **kw(f))
            ref = gpu.cast_rays(p0, p1, **kw(f))
            got = to_numpy(gpu.query_clearance(t0, t1, lo, dims, field, 0, 1))
            for k in same:
                assert got[k].tobytes() == ref[k].tobytes(), (ahead, f, k)
            assert (ref["status"] == 1).sum() >= 5 and (ref["status"] == 0).sum() >= 5, f
        gpu.close()


def test_check_edges(MLMap, knobs):
    """check_edges equals export_esdf over the end points' voxel box followed by query_clearance; it raises when the box is too large"""
    import torch

    b, cfg, lo, dims = real_map(0)
    rng = np.random.default_rng(5)
    p0, p1 = rng.uniform(lo * D, (lo + dims) * D, size=(200, 3)), rng.uniform(lo * D, (lo + dims) * D, size=(200, 3))
    p0[7] = [np.nan, 0.0, 0.0]  # (an invalid segment does not widen the box)
    gb = np.array([0, 16, 16, 100, 200], np.int32)
    gpu = load(MLMap, b, cfg)
    vox = np.floor(np.floor((np.concatenate([np.delete(p0, 7, axis=0), p1]) / D) * 1024.0) / 1024.0).astype(np.int64)
    blo, bdims = vox.min(0), vox.max(0) - vox.min(0) + 1
    for r, cap in ((2, None), (1, 40), (0, None)):
        out = gpu.check_edges(p0, p1, r, sq_cap=cap, group_begin=gb)
        assert np.array_equal(out["box"][0], blo) and np.array_equal(out["box"][1], bdims)
        c = (r + 1) ** 2 if cap is None else cap
        md = max(r + 1, int(np.ceil(np.sqrt(c))))
        field = gpu.export_esdf(blo, bdims, md)["sqdist"]
        two = gpu.query_clearance(p0, p1, blo, bdims, field, r * r, c, False, gb)
        for k in cr.OUTPUTS + ("table",):
            assert isinstance(out[k], np.ndarray) and out[k].tobytes() == two[k].tobytes(), (r, k)
        sw = gpu.query_sweeps(p0, p1, r)
        for k in ("status", "voxel", "t", "n_steps"):
            assert out[k].tobytes() == sw[k].tobytes(), (r, k)
        dev = gpu.check_edges(torch.from_numpy(p0).cuda(), torch.from_numpy(p1).cuda(), r, sq_cap=cap, group_begin=gb)
        assert all(dev[k].is_cuda and dev[k].cpu().numpy().tobytes() == two[k].tobytes() for k in cr.OUTPUTS + ("table",))
    with pytest.raises(ValueError, match=r"\d+ x \d+ x \d+ voxels"):
        gpu.check_edges(p0, p1, 1, max_voxels=int(bdims.prod()) - 1)
    gpu.close()
