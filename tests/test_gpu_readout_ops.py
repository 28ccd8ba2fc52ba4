"""Random sequences of map-changing calls and planner read-outs on one handle, in random map geometries, mirrored on the oracle.

The read-outs (export_window, export_esdf, cast_rays, export_reach, export_clusters) share scratch on the handle (the window
staging, the ESDF scratch of the clearance pass, ray staging, reach fields, cluster words), depend on drain(), on the host
mirror's dirty boxes and on pool growth moving the block planes, and cut voxel indices into block key and cell with subbox_n.
Their own test files run each alone, on a map that stands still, with subbox_n 10 (5 once).  Here one GPU handle and one
OracleMap follow the same random operation list; every read-out is compared where it is asked, with the truth built from the
oracle's block dump of that moment (raywalk_ref.block_classes) through the numpy references (esdf_ref, raywalk_ref, reach_ref,
cluster_ref) — the window from the oracle's own queries, which also pin the class function once per sequence.  Boxes are random,
unaligned, thin, straddle 0 and reach past the map; a third of the calls write into device memory; every sequence ends with the
largest box, the smallest and the largest again through every read-out (scratch that grows, shrinks and is reused).

`Sequence(..., gpu=None)` runs the oracle and the references alone: the conditions that keep the test from being vacuous were
checked that way for the fixed seeds."""
import ctypes
import os

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import cluster_ref, esdf_ref, reach_ref
from tests import raywalk_ref as rw
from tests.util import assert_same_bits, compare_maps

pytestmark = pytest.mark.gpu
EXTRA = [int(x) for x in os.environ.get("MLM_STRESS_SEEDS", "").split(",") if x]  # more seeds for a longer soak: MLM_STRESS_SEEDS=21,22,...
SEEDS = [2, 7, 12]  # subbox_n 3, 7, 16 and subbox_d_xyz 0.15, 0.05, 0.15 (geometry())
STEPS = 60
OCC, INFL, UNKNOWN, SIGNED = 1, 2, 4, 8  # (the same bits in mlm_export_esdf, mlm_export_reach, mlm_export_clusters, mlm_query_rays)
FRONTIER = 16
GEOM_N, GEOM_D = (2, 3, 4, 5, 7, 8, 10, 16), (0.05, 0.1, 0.15, 0.2, 0.25)
MAX_BLOCKS = 8  # the pool the handle starts with: every sequence outgrows it
EDGE = 22  # longest box edge, voxels


def geometry(seed):
    """(subbox_n, subbox_d_xyz) of a seed"""
    rng = np.random.default_rng(7000 + seed)
    return int(rng.choice(GEOM_N)), float(rng.choice(GEOM_D))


def config(seed, explore):
    """the awareness map and the thresholds of S1 on quarter-size frames, the local map's geometry drawn per seed"""
    n, d = geometry(seed)
    return S1.with_(subbox_n=n, subbox_d_xyz=d, use_exploration_frontiers=explore, width=320, height=240, cam_cx=160.0, cam_cy=120.0,
                    cam_fx=192.5, cam_fy=192.5)


def test_fixed_seeds_cover_new_geometries():
    geo = [geometry(s) for s in SEEDS]
    assert any(10 % n for n, _ in geo) and any(d not in (0.1, 0.2) for _, d in geo), geo


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


def grid(lo, dims):
    """voxel indices [N,3] (x, y, z) of the box in its (dz, dy, dx) order"""
    iz, iy, ix = np.unravel_index(np.arange(dims[0] * dims[1] * dims[2]), (dims[2], dims[1], dims[0]))
    return np.stack([lo[0] + ix, lo[1] + iy, lo[2] + iz], axis=1).astype(np.int64)


def grow(lo, dims, g):
    return [v - g for v in lo], [v + 2 * g for v in dims]


class Sequence:
    KINDS = ("window", "esdf", "rays", "reach", "clusters")  # (a subclass adds kinds, their methods and their weights in OPS)

    def __init__(self, cfg, seed, gpu, cpu):
        self.cfg, self.seed, self.gpu, self.cpu = cfg, seed, gpu, cpu
        self.n, self.d = cfg.subbox_n, cfg.subbox_d_xyz
        self.rng = np.random.default_rng(100 * seed + int(cfg.use_exploration_frontiers))
        self.base = syn.room_depth(cfg)
        self.traj = syn.smooth_trajectory(400, seed)
        self.k = 0  # frames integrated so far
        self.step, self.log = 0, []
        self.is_async, self.fresh, self.imports, self.stream_ops = False, False, 0, 0
        self.cap0 = MAX_BLOCKS if gpu is None else max(MAX_BLOCKS, gpu.frame_stats()["block_capacity"])
        self.dump = None  # the oracle's block dump and the class function of the map as it is
        self.noted = []  # every box of the sequence
        self.streams, self.on_stream = None, 0
        self.calls = {k: 0 for k in self.KINDS}
        self.unsynced = {k: 0 for k in self.KINDS}   # read-outs whose immediately preceding operation was a map change in async mode
        self.in_async = {k: 0 for k in self.KINDS}
        self.after_growth = {k: 0 for k in self.KINDS}
        self.rich = {k: 0 for k in self.KINDS}       # calls with a non-trivial answer
        self.grew_in_flight = 0                 # pool growth between the start of an async batch and the end of the read-out behind it
        self.host_rays = self.pinned = self.straddle = self.thin = self.absent = self.skipped = 0

    # ---- bookkeeping ----------------------------------------------------------------------------------------------------------
    def ctx(self, what=""):
        return f"seed {self.seed}, n {self.n}, d {self.d}, step {self.step}, {what}: {self.log}"

    def changed(self):
        self.dump, self.fresh = None, self.is_async

    def has_grown(self):
        """the map holds more blocks than the pool the handle was created with: the pool has grown, or will have when the next
        read-out answers (n_pool_grows itself is asserted at the end)"""
        return self.cpu.block_count() > self.cap0

    def truth(self):
        if self.dump is None:
            b = self.cpu.export_blocks()
            self.dump = (b, rw.block_classes(b, self.n))
        return self.dump

    def occupied(self):
        """voxel indices [K,3] of the OCCUPIED cells of the live blocks"""
        b, n = self.truth()[0], self.n
        blk, cid = np.nonzero((b["occ"] == ord("o")) & (b["collapsed"] == 0)[:, None])
        return b["keys"][blk].astype(np.int64) * n + np.stack([cid % n, (cid // n) % n, cid // (n * n)], axis=1)

    def bits(self, lo, dims):
        """class bits of the box, (dz, dy, dx)"""
        return self.truth()[1](grid(lo, dims)).reshape(dims[2], dims[1], dims[0])

    def count(self, kind, rich):
        self.calls[kind] += 1
        self.unsynced[kind] += self.fresh
        self.fresh = False
        self.in_async[kind] += self.is_async
        self.after_growth[kind] += self.has_grown()
        self.rich[kind] += bool(rich)

    def dev(self):
        pick = self.rng.random() < 1 / 3  # (drawn without a GPU as well: the oracle-only run sees the same sequence)
        return self.gpu is not None and pick

    # ---- frames and boxes -----------------------------------------------------------------------------------------------------
    def frame(self, jump=0.0):
        img = syn.jitter_depth(self.base, self.k, seed=self.seed)
        q, t = self.traj[self.k]
        t = t + np.array([0.03 * self.k + jump, -0.02 * self.k, 0.0])  # (the camera wanders: new blocks keep appearing)
        self.k += 1
        return img, q, t

    def box(self):
        """a random unaligned box around a block of the map: thin, straddling 0 or reaching past the map now and then"""
        rng, n = self.rng, self.n
        keys = self.truth()[0]["keys"]
        dims = [int(v) for v in rng.integers(2, EDGE + 1, 3)]
        if rng.random() < 0.3:
            dims[int(rng.integers(0, 3))] = 1
        anchor = keys[int(rng.integers(0, len(keys)))].astype(np.int64) * n if len(keys) else np.zeros(3, np.int64)
        lo = [int(anchor[a] + rng.integers(-dims[a], max(n, 2))) for a in range(3)]
        occupied = self.occupied()
        if len(occupied) and rng.random() < 0.6:  # (around an OCCUPIED voxel: surfaces, specks of noise, unknown space behind them)
            v = occupied[int(rng.integers(0, len(occupied)))]
            lo = [int(v[a] - rng.integers(0, dims[a])) for a in range(3)]
        if rng.random() < 0.25:
            a = int(rng.integers(0, 3))
            lo[a] = -int(rng.integers(0, dims[a]))  # (dims 1: lo 0 .. -0; else straddles 0)
        self.note(lo, dims)
        return lo, dims

    def note(self, lo, dims):
        self.noted.append((lo, dims))
        self.straddle += any(lo[a] < 0 < lo[a] + dims[a] for a in range(3))
        self.thin += 1 in dims
        g = np.unique(np.floor_divide(grid(lo, dims), self.n), axis=0)
        have = set(map(tuple, self.truth()[0]["keys"].tolist()))
        self.absent += any(tuple(k) not in have for k in g.tolist())

    def world(self, lo, dims):
        return np.array(lo) * self.d, (np.array(lo) + np.array(dims)) * self.d

    # ---- map-changing operations ----------------------------------------------------------------------------------------------
    def both(self, fn):
        if self.gpu is not None:
            fn(self.gpu)
        fn(self.cpu)

    def op_dense(self):
        img, q, t = self.frame()
        if self.gpu is not None:
            self.gpu.update_map(img, q, t)
        self.cpu.update_depth(img, q, t)
        self.changed()

    def op_sampled(self):
        img, q, t = self.frame()
        pix = (self.rng.integers(0, self.cfg.height, 500) * self.cfg.width + self.rng.integers(0, self.cfg.width, 500)).astype(np.int32)
        if self.gpu is not None:
            self.gpu.update_map(img, q, t, pixel_idx=pix)
        self.cpu.update_depth_indexed(img, pix, q, t)
        self.changed()

    def op_growbatch(self):
        """an asynchronous batch seen from somewhere else: new blocks, the pool grows while the batch is in flight"""
        if not self.is_async:
            self.is_async = True
            if self.gpu is not None:
                self.gpu.set_async(True)
        fr = [self.frame(jump=1.5) for _ in range(int(self.rng.integers(2, 5)))]
        if self.gpu is not None:
            self.gpu.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), np.stack([f[2] for f in fr]))
        for img, q, t in fr:
            self.cpu.update_depth(img, q, t)
        self.changed()

    def op_setfree(self):
        """setFree_map_in_bound around an OCCUPIED voxel, between two small ray batches through it: the first brings the host mirror
        up to date, the second must see the freed voxels"""
        occupied = self.occupied()
        v = occupied[int(self.rng.integers(0, len(occupied)))] if len(occupied) else np.zeros(3, np.int64)
        c = (v + 0.5) * self.d
        lo, dims = [int(x) - 3 for x in v], [7, 7, 7]
        self.note(lo, dims)
        self.rays(lo, dims, small=True, flags=OCC, through=c)
        lo_, hi_ = c - self.rng.uniform(0.5, 2.5, 3) * self.d, c + self.rng.uniform(0.5, 2.5, 3) * self.d
        self.both(lambda m: m.setFree_map_in_bound(lo_, hi_))
        self.changed()
        self.rays(lo, dims, small=True, flags=OCC, through=c)

    def op_inflate(self):
        c = self.traj[max(self.k - 1, 0)][1]
        self.both(lambda m: m.inflate_map(c))
        self.changed()

    def op_import(self):
        """a few crafted blocks: negative keys next to each other (one of them released in frontier mode) and one far from the rest"""
        rng, C = self.rng, self.cfg.cells_per_block
        self.imports += 1
        base = -(20 + 3 * self.imports)
        keys = np.array([[base, base, -1], [base + 1, base, -1], [base, base + 1, 0], [3000 + self.imports, -2000, 7]], dtype=np.int32)
        lo = rng.uniform(self.cfg.lm_log_odds_min, self.cfg.lm_log_odds_max, size=(4, C)).astype(np.float32)
        occ = rng.choice(np.frombuffer(b"ofu", dtype=np.uint8), size=(4, C), p=[0.15, 0.6, 0.25])
        infl = rng.choice(np.frombuffer(b"ofu", dtype=np.uint8), size=(4, C), p=[0.2, 0.5, 0.3])
        col = np.zeros(4, dtype=np.uint8)
        if self.cfg.use_exploration_frontiers:
            col[1] = 1
        self.both(lambda m: m.import_blocks(keys, lo, occ, infl, col))
        self.changed()

    def op_mode(self):
        self.is_async, self.fresh = not self.is_async, False
        if self.gpu is not None:
            self.gpu.set_async(self.is_async)

    def op_stream(self):
        """the handle moves to a stream of the caller, and back to the caller's other stream at the next call (mlm_set_stream gives
        up the handle's own stream for good: there is none to go back to)"""
        self.stream_ops += 1
        self.fresh = False
        if self.gpu is None:
            return
        import torch

        if self.streams is None:
            self.streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        self.on_stream ^= 1
        self.gpu.set_stream(self.streams[self.on_stream].cuda_stream)

    def op_sync(self):
        if self.gpu is not None:
            self.gpu.sync()
        self.fresh = False

    # ---- read-outs ------------------------------------------------------------------------------------------------------------
    def tensors(self, spec):
        """{name: tensor} on the device, pre-filled with a sentinel"""
        import torch

        out = {k: torch.full(shape, 7, dtype=dt, device="cuda") for k, (shape, dt) in spec.items()}
        torch.cuda.synchronize()
        return out

    def fetch(self, dev):
        import torch

        self.gpu.sync()
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in dev.items()}

    def window(self, lo, dims):
        import torch

        max_iter = int(self.rng.choice([0, 1, 5, 9]))
        v = grid(lo, dims)
        keys = np.floor_divide(v, self.n)
        cc = v - keys * self.n
        cid = ((cc[:, 2] * self.n + cc[:, 1]) * self.n + cc[:, 0]).astype(np.int32)
        cen = rw.centres(v, self.cfg)
        shape = (dims[2], dims[1], dims[0])
        exp = {"odds": self.cpu.getOddAt(keys.astype(np.int32), cid).reshape(shape), "occ": self.cpu.getOccupancy(cen).reshape(shape),
               "infl": self.cpu.getInflateOccupancy(cen).reshape(shape), "grad": self.cpu.getOddGrad(cen, max_iter).reshape(shape + (3,))}
        self.count("window", all((exp["occ"] == c).any() for c in (-1, 0, 1)))
        use_dev = self.dev()
        if self.gpu is None:
            return
        if use_dev:
            dev = self.tensors({"odds": (shape, torch.float32), "occ": (shape, torch.int8), "infl": (shape, torch.int8), "grad": (shape + (3,), torch.float64)})
            self.gpu.export_window_dev(lo, dims, max_iter, **{k: t.data_ptr() for k, t in dev.items()})
            got = self.fetch(dev)
        else:
            got = self.gpu.export_window(lo, dims, odds=True, occ=True, infl=True, grad=True, max_iter=max_iter)
        for k in ("odds", "grad"):
            assert_same_bits(got[k].reshape(len(v), -1), exp[k].reshape(len(v), -1), self.ctx(f"window {k} {lo} {dims} max_iter={max_iter} dev={use_dev}"))
        for k in ("occ", "infl"):
            assert_same_bits(got[k].reshape(-1).astype(np.int32), exp[k].reshape(-1), self.ctx(f"window {k} {lo} {dims} dev={use_dev}"))

    def esdf(self, lo, dims):
        import torch

        rng = self.rng
        C = int(rng.choice([1, 2, 5, 16, 33]))
        flags = int(rng.integers(1, 8)) | (SIGNED if rng.random() < 0.5 else 0)
        glo, gd = grow(lo, dims, C)
        mask = (self.bits(glo, gd) & flags) != 0
        exp = esdf_ref.expected(mask, C, bool(flags & SIGNED), self.d)
        self.count("esdf", ((exp["sqdist"] > 0) & (exp["sqdist"] < C * C)).any())
        use_dev = self.dev()
        if self.gpu is None:
            return
        kw = dict(occ=bool(flags & OCC), infl=bool(flags & INFL), unknown=bool(flags & UNKNOWN), signed=bool(flags & SIGNED))
        shape = (dims[2], dims[1], dims[0])
        if use_dev:
            dev = self.tensors({"sqdist": (shape, torch.int32), "dist": (shape, torch.float32), "grad": (shape + (3,), torch.float32)})
            self.gpu.export_esdf_dev(lo, dims, C, **kw, **{k: t.data_ptr() for k, t in dev.items()})
            got = self.fetch(dev)
        else:
            got = self.gpu.export_esdf(lo, dims, C, **kw, sqdist=True, dist=True, grad=True)
        what = self.ctx(f"esdf {lo} {dims} C={C} flags={flags} dev={use_dev}")
        assert np.array_equal(got["sqdist"], exp["sqdist"]), what
        for k in ("dist", "grad"):
            assert np.array_equal(got[k].view(np.uint32), exp[k].view(np.uint32)), (k, what)

    def rays(self, lo, dims, small, flags=None, through=None):
        import torch

        rng, d = self.rng, self.d
        flags = int(rng.integers(0, 8)) if flags is None else flags
        wlo, whi = self.world(lo, dims)
        if small:
            p0, p1 = rw.uniform_rays(rng, wlo, whi, 5)
            if through is not None:
                p1 = 2 * through - p0  # (every ray passes the voxel)
        else:
            a, b = rw.uniform_rays(rng, wlo - 2 * d, whi + 2 * d, 2200, short=6 * d)
            sa, sb = rw.special_rays(rng, wlo, whi, d, count=30)
            parts = [(a, b), (sa, sb)]
            if self.calls["rays"] % 4 == 0:
                parts.append(rw.weird_rays(d))
            p0, p1 = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        exp = rw.cast_all(p0, p1, d, self.truth()[1], (flags,))[0][flags]
        self.count("rays", (exp["status"] == 1).any() and (exp["status"] == 0).any())
        use_dev = not small and self.dev()
        if self.gpu is None:
            return
        kw = dict(occ=bool(flags & OCC), infl=bool(flags & INFL), unknown=bool(flags & UNKNOWN))
        n = len(p0)
        before = self.gpu.frame_stats()["n_host_queries"]  # (a counter of the handle: reading it waits for nothing)
        if use_dev:
            dev = self.tensors({"status": ((n,), torch.int8), "voxel": ((n, 3), torch.int32), "t": ((n,), torch.float64),
                                "n_steps": ((n,), torch.int32), "n_unknown": ((n,), torch.int32)})
            ends = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in (p0, p1)]
            torch.cuda.synchronize()
            self.gpu.cast_rays_dev(ends[0].data_ptr(), ends[1].data_ptr(), n, **kw, **{k: t.data_ptr() for k, t in dev.items()})
            got = self.fetch(dev)
        else:
            got = self.gpu.cast_rays(p0, p1, **kw)
        rw.assert_equal(got, exp, self.ctx(f"rays {lo} {dims} {'small' if small else 'large'} flags={flags} dev={use_dev}"))
        took = self.gpu.frame_stats()["n_host_queries"] - before  # the route: a handful of rays on the host mirror, thousands through the kernel
        assert took == (n if small else 0), self.ctx(f"rays: {took} of {n} answered on the host")
        self.host_rays += took

    def reach(self, lo, dims):
        import torch

        rng = self.rng
        for _ in range(1 if self.rich["reach"] else 5):  # (until one call had a non-trivial answer: up to five draws of the arguments)
            flags = int(rng.choice([0, OCC, OCC | INFL, OCC | UNKNOWN, UNKNOWN, OCC | INFL | UNKNOWN]))
            r = int(rng.choice([0, 1, 3]))
            glo, gd = grow(lo, dims, r + 1)
            T = ~reach_ref.blocked((self.bits(glo, gd) & flags) != 0, r)
            k = int(rng.integers(1, 5))
            seeds = np.stack([rng.integers(-2, dims[a] + 2, k) for a in range(3)], axis=1)  # (relative to the box; some outside)
            free = np.argwhere(T)
            if len(free) and rng.random() < 0.9:
                seeds[0] = free[int(rng.integers(0, len(free)))][::-1]
            max_steps = int(rng.integers(1, 6)) if rng.random() < 0.4 else None
            exp = reach_ref.reach(T, seeds, max_steps)
            if 0 < exp["summary"][1] < exp["summary"][0]:
                break
        self.count("reach", 0 < exp["summary"][1] < exp["summary"][0])
        use_dev = self.dev()
        if self.gpu is None:
            return
        kw = dict(occ=bool(flags & OCC), infl=bool(flags & INFL), unknown=bool(flags & UNKNOWN), clearance=r, max_steps=max_steps)
        sv = (seeds + np.array(lo)).astype(np.int32)
        shape = (dims[2], dims[1], dims[0])
        if use_dev:
            dev = self.tensors({"steps": (shape, torch.int32), "parent": (shape, torch.uint8)})
            sd = torch.from_numpy(np.ascontiguousarray(sv)).cuda()
            torch.cuda.synchronize()
            sm = self.gpu.export_reach_dev(lo, dims, sd.data_ptr(), k, **kw, steps=dev["steps"].data_ptr(), parent=dev["parent"].data_ptr(), summary=True)
            got = self.fetch(dev)
            got["summary"] = sm
        else:
            got = self.gpu.export_reach(lo, dims, sv, **kw, steps=True, parent=True)
        what = self.ctx(f"reach {lo} {dims} flags={flags} clearance={r} seeds={seeds.tolist()} max_steps={max_steps} dev={use_dev}")
        assert np.array_equal(got["steps"], exp["steps"]), what
        assert np.array_equal(got["parent"], exp["parent"]), what
        assert np.array_equal(got["summary"][:3], exp["summary"]), (got["summary"], exp["summary"], what)
        hit = np.argwhere(got["steps"] >= 0)
        for z, y, x in hit[rng.permutation(len(hit))[:20]]:  # the client's walk along `parent` ends at a seed in `steps` moves
            p = reach_ref.walk(got["parent"], (x, y, z))
            assert len(p) - 1 == got["steps"][z, y, x] and got["steps"][p[-1][2], p[-1][1], p[-1][0]] == 0, what

    def clusters(self, lo, dims):
        import torch

        rng = self.rng
        for _ in range(1 if self.rich["clusters"] else 5):  # (until one call had a non-trivial answer: up to five draws of the arguments)
            frontier = rng.random() < 0.4
            flags = FRONTIER if frontier else int(rng.choice([OCC, OCC | INFL, int(rng.integers(1, 8))]))  # (surfaces break into specks: more of them)
            conn, min_size = int(rng.choice([6, 18, 26])), int(rng.choice([1, 2, 9], p=[0.2, 0.4, 0.4]))
            cap = int(rng.choice([1, 2, 4, 512]))
            if frontier:
                glo, gd = grow(lo, dims, 1)
                b = self.bits(glo, gd)
                S = cluster_ref.frontier_set(np.where(b & OCC, 0, np.where(b & UNKNOWN, -1, 1)))
            else:
                S = (self.bits(lo, dims) & flags) != 0
            exp = cluster_ref.clusters(S, conn, min_size, cap, lo)
            if exp["summary"][2] >= 2 and exp["summary"][1] > exp["summary"][2]:
                break
        K = int(exp["summary"][2])
        self.count("clusters", K >= 2 and exp["summary"][1] > K)
        use_dev = self.dev()
        if self.gpu is None:
            return
        kw = dict(frontier=frontier, occ=bool(flags & OCC), infl=bool(flags & INFL), unknown=bool(flags & UNKNOWN), connectivity=conn, min_size=min_size)
        shape = (dims[2], dims[1], dims[0])
        if use_dev:
            dev = self.tensors({"labels": (shape, torch.int32), "table": ((cap, cluster_ref.ROW), torch.int64)})
            sm = self.gpu.export_clusters_dev(lo, dims, **kw, labels=dev["labels"].data_ptr(), table=dev["table"].data_ptr(), cap=cap, summary=True)
            got = self.fetch(dev)
        else:  # (the C call itself: the wrapper hands out the first min(K, cap) rows only)
            got = {"labels": np.full(shape, 7, dtype=np.int32), "table": np.full((cap, cluster_ref.ROW), 7, dtype=np.int64)}
            sm = np.zeros(6, dtype=np.int64)
            lo_a, dims_a = self.gpu._window_args(lo, dims)
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
            rc = self.gpu._L.mlm_export_clusters(self.gpu._h, p(lo_a), p(dims_a), self.gpu._cluster_flags(**{k: kw[k] for k in ("frontier", "occ", "infl", "unknown")}),
                                                 conn, min_size, p(got["labels"]), p(got["table"]), cap, p(sm))
            assert rc == 0, self.ctx(f"mlm_export_clusters: {rc}")
        what = self.ctx(f"clusters {lo} {dims} flags={flags} connectivity={conn} min_size={min_size} cap={cap} K={K} dev={use_dev}")
        assert np.array_equal(got["labels"], exp["labels"]), what
        rows = min(K, cap)
        assert np.array_equal(got["table"][:rows], exp["table"]), what
        assert (got["table"][rows:] == 7).all(), "rows from min(K, cap) on were written: " + what
        assert np.array_equal(sm[:5], exp["summary"]), (sm, exp["summary"], what)

    def pin_classes(self, lo, dims):
        """the class function of the block dump against the oracle's queries at the voxel centres"""
        v = grid(lo, dims)
        got = self.truth()[1](v)
        want = rw.query_classes(self.cpu.getOccupancy, self.cpu.getInflateOccupancy, self.cfg)(v)
        assert np.array_equal(got, want), self.ctx(f"block_classes against the oracle's queries {lo} {dims}")
        self.pinned += 1

    def behind_a_batch(self, kind):
        before = 0 if self.gpu is None else self.gpu.frame_stats()["n_pool_grows"]
        self.log.append("growbatch")
        self.op_growbatch()
        assert self.fresh
        self.readout(kind, *self.box())
        if self.gpu is not None:
            self.gpu.sync()  # (n_pool_grows is brought up to date when the frames are through)
            self.grew_in_flight += self.gpu.frame_stats()["n_pool_grows"] > before

    def readout(self, kind, lo, dims, small_rays=False):
        self.log.append(kind)
        if kind == "rays":
            self.rays(lo, dims, small_rays)
        else:
            getattr(self, kind)(lo, dims)

    # ---- the sequence ---------------------------------------------------------------------------------------------------------
    OPS = {"dense": 0.11, "sampled": 0.05, "growbatch": 0.06, "setfree": 0.05, "inflate": 0.06, "import": 0.04, "mode": 0.05, "stream": 0.03,
           "sync": 0.04, "window": 0.1, "esdf": 0.1, "rays": 0.06, "rays_small": 0.05, "reach": 0.1, "clusters": 0.1}

    def run(self, steps=STEPS):
        names, p = list(self.OPS), np.array(list(self.OPS.values()))
        # the first frames of the map arrive as an asynchronous batch, a read-out right behind it: the pool of MAX_BLOCKS blocks grows
        # while the batch is in flight, and the read-out must see the planes where they have moved
        self.behind_a_batch(self.KINDS[self.seed % len(self.KINDS)])
        for op in ("mode", "dense", "dense", "import"):
            self.log.append(op)
            getattr(self, "op_" + op)()
        for self.step in range(steps):
            op = str(self.rng.choice(names, p=p / p.sum()))
            if op in self.KINDS or op == "rays_small":
                self.readout("rays" if op == "rays_small" else op, *self.box(), small_rays=op == "rays_small")
            else:
                self.log.append(op)
                getattr(self, "op_" + op)()
            if self.step == steps // 2:
                self.pin_classes(*self.box())
        self.step = steps
        for kind in self.KINDS:  # every kind once directly behind an asynchronous batch
            self.behind_a_batch(kind)
        self.before_the_tail()
        # the tail: the largest box of the sequence through every read-out, the smallest ones, the largest again
        big = max(self.noted, key=lambda b: b[1][0] * b[1][1] * b[1][2])
        tiny = [(list(big[0]), [1, 1, 1]), ([big[0][0] + 1, big[0][1], big[0][2] + 2], [1, big[1][1], 1])]
        for i, (lo, dims) in enumerate([big] + tiny + [big]):
            if i == 3:
                self.log.append("stream")
                self.op_stream()
            self.note(lo, dims)
            for kind in self.KINDS:
                self.readout(kind, lo, dims, small_rays=dims[0] == 1)
        self.pin_classes(*big)

    def before_the_tail(self):
        """(a subclass's own fixed steps)"""

    def check_not_vacuous(self):
        for k in self.KINDS:
            assert self.calls[k] >= 4 and self.unsynced[k] >= 1 and self.in_async[k] >= 1 and self.after_growth[k] >= 1 and self.rich[k] >= 1, \
                self.ctx(f"{k}: calls {self.calls[k]}, unsynced {self.unsynced[k]}, async {self.in_async[k]}, after growth {self.after_growth[k]}, "
                         f"non-trivial {self.rich[k]}")
        assert self.pinned >= 2 and self.straddle >= 1 and self.thin >= 1 and self.absent >= 1 and self.imports >= 1 and self.stream_ops >= 1 and self.skipped == 0, \
            self.ctx(f"pinned {self.pinned}, straddling {self.straddle}, thin {self.thin}, absent {self.absent}, imports {self.imports}")


@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("seed", SEEDS + EXTRA)
def test_random_readout_sequences(mods, knobs, explore, seed):
    MLMap, OracleMap = mods
    cfg = config(seed, explore)
    knobs.set("pool_grow", 1)
    gpu, cpu = MLMap(cfg, max_blocks=MAX_BLOCKS, max_points=cfg.width * cfg.height, max_batch=4), OracleMap(cfg)
    s = Sequence(cfg, seed, gpu, cpu)
    s.run()
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), s.ctx("the maps at the end"))
    if explore:
        gf, cf = gpu.export_frontier(), cpu.export_frontier()
        assert gf.shape == cf.shape and np.array_equal(gf, cf), s.ctx("the frontier sets at the end")
    st = gpu.frame_stats()
    assert st["n_pool_grows"] >= 1 and s.grew_in_flight >= 1 and s.host_rays > 0, (st, s.grew_in_flight, s.ctx("pool growth, rays on the host mirror"))
    if seed in SEEDS:
        s.check_not_vacuous()
    gpu.close()
