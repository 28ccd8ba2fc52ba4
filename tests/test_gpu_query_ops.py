"""The nine later read-outs (export_grid2d, export_route, query_paths, render_depth, query_views, query_boxes, query_nearest,
query_sweeps, score_poses) in the random call sequences of tests/test_gpu_readout_ops.py, in explicit map geometries.

Their own test files run each call alone, on a map that stands still, with subbox_n 10 (5 once) and a pool that never grows.  Here one
GPU handle and one OracleMap follow the same random list of map changes (the parent's, unchanged) and read-outs, in the geometries at
which the kernels' control flow changes: subbox_n 2, 3, 4 and 7, whose largest radius with the block box in k_sweeps' slot cache is
2 n (the host's rule (2r - 1) / n + 2 <= 5) and which have fewer cells per block than a wave has lanes, and 8 and 16, where every radius
is cached; voxel sizes from 0.05 to 0.25.  The truth of every read-out is the plain-Python reference of its own test file over the
classes of the oracle's block dump of that moment; every comparison is byte for byte, the float channels included.

boxes, nearest, sweeps and score also have a `*_small` operation (op_setfree's shape): a batch small enough for the host mirror next to
an OCCUPIED voxel, setFree_map_in_bound around it, the same batch again: the second answer must show the change.  n_host_queries
shows that the mirror answered every small batch and no large one: a large batch in host memory carries invalid items behind its own up
to 65, one more than an up-to-date mirror takes (past_the_mirror), so boxes, nearest and sweeps reach their kernels in every call.

At the largest cached radius and the next one, six rays of every sweeps batch run past the blocks of the last op_import, alone in unknown
space, and stop on an OCCUPIED voxel in the last block layer of the block box around the ball (edge_rays); past the bound the box is six
blocks wide there, where a torus of five would hand out the first layer's entry.  edge_stopped counts such stops from the reference's answer.

`QuerySequence(..., gpu=None)` runs the oracle and the references alone: the conditions that keep the test from being vacuous
(check_not_vacuous) were established that way for the twelve fixed cases; the slowest of them (subbox_n 7 and 16 at 0.05 m) take 12.3 s there, the
existing file's slowest 14.1 s in the same measurement, most of it in the oracle and the references."""
import numpy as np
import pytest

from tests import box_ref, esdf_ref, grid_ref, nearest_ref, path_ref, reach_ref, render_ref, route_ref, score_ref, sweep_ref, view_ref
from tests import raywalk_ref as rw
from tests.test_gpu_readout_ops import EXTRA, MAX_BLOCKS, OCC, INFL, UNKNOWN, Sequence, grid, grow
from tests.test_gpu_readout_ops import config as parent_config
from tests.util import compare_maps

pytestmark = pytest.mark.gpu
GEOMETRIES = [(2, 0.25), (3, 0.15), (4, 0.1), (7, 0.05), (8, 0.15), (16, 0.05)]
SEED, CASE_SEED = 4, {(7, True): 6}  # the sequence of a fixed case: (subbox_n, frontier mode) -> seed, SEED for the others
STEPS = 30
SWEEP_NB = 5                    # kSweepNB (mlm_kernels_sweeps.h)
VIEW_LDS_BITS = (64 * 1024 - 64) * 8  # kViewLdsBits (mlm_views.h)
MIRROR_CLEAN = 64  # most items of a batch the host mirror answers when it is up to date: MlmMirror::max_clean / 4 (8 while it needs a refresh first)
COSTS = (10, 14, 17)
SMALL = ("boxes", "nearest", "sweeps", "score")


def config(n, d, explore):
    """the parent's configuration in an explicit geometry (mlm_inflate_map needs inflate_n < subbox_n: 1 at subbox_n 2, S1's 2 otherwise)"""
    cfg = parent_config(0, explore)
    return cfg.with_(subbox_n=n, subbox_d_xyz=d, inflate_n=min(cfg.inflate_n, n - 1))


def cached_radius(n):
    """the largest radius whose block box stays in k_sweeps' slot cache: (2r - 1) / n + 2 <= kSweepNB"""
    return max(r for r in range(1, sweep_ref.MAX_RADIUS + 1) if (2 * r - 1) // n + 2 <= SWEEP_NB)


def past_the_mirror(rows, filler):
    """the batch with copies of `filler`, an invalid item that costs the reference nothing, behind it: MIRROR_CLEAN + 1 rows, more than
    the host mirror answers in whatever state it is, so that a large batch in host memory runs as a kernel like one in device memory"""
    rows = np.asarray(rows)
    pad = np.tile(np.asarray(filler, dtype=rows.dtype), (max(0, MIRROR_CLEAN + 1 - len(rows)), 1))
    return np.concatenate([rows, pad])


def kw3(flags):
    return dict(occ=bool(flags & OCC), infl=bool(flags & INFL), unknown=bool(flags & UNKNOWN))


def same(got, exp, names, what):
    """the named outputs equal byte for byte"""
    for k in names:
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, g.dtype, e.shape, e.dtype)
        bad = np.flatnonzero((g.view(np.uint8).reshape(len(g), -1) != e.view(np.uint8).reshape(len(e), -1)).any(axis=1)) if len(g) else []
        assert len(bad) == 0, f"{what} {k}: {len(bad)} of {len(g)} rows differ, first #{bad[0]}: {g[bad[0]]!r} vs {e[bad[0]]!r}"


class QuerySequence(Sequence):
    KINDS = ("grid2d", "route", "paths", "render", "views", "boxes", "nearest", "sweeps", "score")
    OPS = {"dense": 0.1, "sampled": 0.04, "growbatch": 0.03, "setfree": 0.03, "inflate": 0.05, "import": 0.04, "mode": 0.05, "stream": 0.03, "sync": 0.03,
           "grid2d": 0.06, "route": 0.06, "paths": 0.06, "render": 0.05, "views": 0.05, "boxes": 0.06, "nearest": 0.06, "sweeps": 0.07, "score": 0.05,
           "boxes_small": 0.04, "nearest_small": 0.04, "sweeps_small": 0.04, "score_small": 0.04}

    def __init__(self, cfg, seed, gpu, cpu):
        super().__init__(cfg, seed, gpu, cpu)
        for c in (self.calls, self.unsynced, self.in_async, self.after_growth, self.rich):
            c["rays"] = 0  # (op_setfree's two small ray batches)
        self.r_c = cached_radius(self.n)
        self.small_calls = {k: 0 for k in SMALL}
        self.small_shown = {k: 0 for k in SMALL}  # second batches whose reference answer differs from the first's
        self.host_items = {k: 0 for k in SMALL}
        self.sweep_stops = {}                     # radius -> calls with a stop among the rays
        self.edge_stops = {}                      # radius -> stops decided in an outermost block layer of the ball's block box (edge_stopped)
        self.released_hit = 0                     # reference answers that lie in a released block
        self.lds_views = self.global_views = 0
        self.unit_routes = 0                      # routes held to reach_ref as well
        self.last = None

    # ---- helpers --------------------------------------------------------------------------------------------------------------
    def frame(self, jump=0.0):
        self.last = super().frame(jump)
        return self.last

    def classes(self):
        return self.truth()[1]

    def T_last(self, count=1, spread=0.05):
        """the pose of the last integrated frame, moved by a small random offset"""
        from mlmapping_amd.mlmap import compose_T_ws

        _, q, t = self.last
        t = np.asarray(t, dtype=np.float64)[None, :] + self.rng.uniform(-spread, spread, size=(count, 3))
        return compose_T_ws(np.tile(np.asarray(q, dtype=np.float64), (count, 1)), t, self.cfg.T_B_S)

    def occ_infl(self, lo, dims):
        """the classes of a box as export_window's occ / infl channels: 0 OCCUPIED, 1 FREE, -1 UNKNOWN"""
        b = self.bits(lo, dims)
        return np.where(b & OCC, 0, np.where(b & UNKNOWN, -1, 1)), np.where(b & INFL, 0, 1)

    def released(self):
        """keys of the released blocks, those whose element 0 is not FREE first"""
        b = self.truth()[0]
        idx = np.flatnonzero(b["collapsed"] != 0)
        return b["keys"][idx[np.argsort(b["occ"][idx, 0] == ord("f"), kind="stable")]].astype(np.int64)

    def to_dev(self, *arrays):
        import torch

        out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
        torch.cuda.synchronize()
        return out

    def host_took(self, n, fn, small, what):
        """fn() with the items the host mirror answered: all n of a small batch, none of a large one"""
        before = self.gpu.frame_stats()["n_host_queries"]
        got = fn()
        took = self.gpu.frame_stats()["n_host_queries"] - before
        assert took == (n if small else 0), self.ctx(f"{what}: {took} of {n} answered on the host")
        return got, took

    def count_small(self, kind, shown, took):
        self.small_calls[kind] += 1
        self.small_shown[kind] += bool(shown)
        self.host_items[kind] += took
        self.fresh = False

    def around_an_obstacle(self):
        """an OCCUPIED voxel, its centre and the box of op_setfree around it"""
        occupied = self.occupied()
        v = occupied[int(self.rng.integers(0, len(occupied)))] if len(occupied) else np.zeros(3, np.int64)
        lo, dims = [int(x) - 3 for x in v], [7, 7, 7]
        self.note(lo, dims)
        return v, (v + 0.5) * self.d

    def free_around(self, c):
        lo_, hi_ = c - self.rng.uniform(0.5, 2.5, 3) * self.d, c + self.rng.uniform(0.5, 2.5, 3) * self.d
        self.both(lambda m: m.setFree_map_in_bound(lo_, hi_))
        self.changed()

    # ---- grid2d ---------------------------------------------------------------------------------------------------------------
    def grid2d(self, lo, dims):
        import torch

        rng = self.rng
        for again in range(1 if self.rich["grid2d"] else 5):
            flags = int(rng.integers(1, 8))
            du = grid_ref.DIST_UNOBSERVED if rng.random() < 0.4 else 0
            min_free = min(int(rng.choice([0, 2])), dims[2])
            if again:  # (-1 needs min_free, and columns of UNKNOWN voxels that are no obstacles)
                flags, min_free = (flags & 3) or OCC, min(2, dims[2])
            z_ref = [None, lo[2] + int(rng.integers(0, dims[2])), lo[2] - 2, lo[2] + dims[2] + 1][int(rng.integers(0, 4))]
            C = int(rng.choice([1, 3, 9]))
            exp = grid_ref.columns(*self.occ_infl(lo, dims), lo[2], flags, min_free, z_ref)
            if all((exp["grid"] == c).any() for c in (100, 0, -1)):
                break
        g = grid_ref.columns(*self.occ_infl(*grid_ref.grown2(lo, dims, C)), lo[2], flags, min_free, z_ref)["grid"]
        exp.update(grid_ref.dist_channels(grid_ref.dist_separable(grid_ref.plane_mask(g, flags | du), C), self.d))
        self.count("grid2d", all((exp["grid"] == c).any() for c in (100, 0, -1)))
        use_dev = self.dev()
        if self.gpu is None:
            return
        kw = dict(min_free=min_free, z_ref=z_ref, max_dist=C, dist_unobserved=bool(du), **kw3(flags))
        shape = (dims[1], dims[0])
        cols = z_ref is None or lo[2] <= z_ref < lo[2] + dims[2]  # (a z_ref outside the slab is accepted without the column words only)
        if use_dev:
            dev = self.tensors({"grid": (shape, torch.int8), "sqdist": (shape, torch.int32), "dist": (shape, torch.float32),
                                **({"cols": (shape + (8,), torch.int32)} if cols else {})})
            sm = self.gpu.export_grid2d_dev(lo, dims, **kw, **{k: t.data_ptr() for k, t in dev.items()})
            got = self.fetch(dev)
            got["summary"] = sm
        else:
            got = self.gpu.export_grid2d(lo, dims, **kw, grid=True, cols=cols, sqdist=True, dist=True)
        grid_ref.compare(got, exp, self.ctx(f"grid2d {lo} {dims} flags={flags | du} min_free={min_free} z_ref={z_ref} C={C} dev={use_dev}"))

    # ---- route and paths ------------------------------------------------------------------------------------------------------
    def draw_route(self, lo, dims, rich):
        """arguments of export_route (box, seeds and clearance as reach draws them) and the reference's field"""
        rng = self.rng
        for _ in range(1 if rich else 5):
            a = dict(flags=int(rng.choice([0, OCC, OCC | INFL, OCC | UNKNOWN, UNKNOWN, OCC | INFL | UNKNOWN])), r=int(rng.choice([0, 1, 3])),
                     conn=int(rng.choice([6, 18, 26])), pen=(20, 7) if rng.random() < 0.5 else (), costs=COSTS)
            if self.unit_routes == 0 and self.calls["route"] > 0:  # (the second route of a sequence, if none before it: export_reach's rules)
                a["conn"], a["pen"] = 6, ()
            if a["conn"] == 6 and not a["pen"] and (rng.random() < 0.7 or self.unit_routes == 0):
                a["costs"] = (1, 1, 1)
            g = a["r"] + len(a["pen"]) + 1
            glo, gd = grow(lo, dims, g)
            a["cls"] = route_ref.classes((self.bits(glo, gd) & a["flags"]) != 0, a["r"], len(a["pen"]))
            T = a["cls"] != route_ref.BLOCKED
            k = int(rng.integers(1, 5))
            a["seeds"] = np.stack([rng.integers(-2, dims[x] + 2, k) for x in range(3)], axis=1)
            free = np.argwhere(T)
            if len(free) and rng.random() < 0.9:
                a["seeds"][0] = free[int(rng.integers(0, len(free)))][::-1]
            a["max_cost"] = int(rng.integers(1, 8)) * max(a["costs"]) if rng.random() < 0.4 else None
            a["exp"] = route_ref.route(a["cls"], a["seeds"], a["conn"], a["costs"], a["pen"], a["max_cost"])
            if 0 < a["exp"]["summary"][1] < a["exp"]["summary"][0]:
                break
        if a["costs"] == (1, 1, 1):  # unit cost, face moves, no penalty: export_reach's steps
            ref = reach_ref.reach(T, a["seeds"], a["max_cost"])
            assert np.array_equal(ref["steps"], a["exp"]["cost"]), self.ctx("route_ref against reach_ref")
            self.unit_routes += 1
        a["kw"] = dict(clearance=a["r"], connectivity=a["conn"], move_cost=a["costs"], penalty=a["pen"], max_cost=a["max_cost"], **kw3(a["flags"]))
        a["sv"] = (a["seeds"] + np.array(lo)).astype(np.int32)
        a["what"] = f"{lo} {dims} flags={a['flags']} clearance={a['r']} conn={a['conn']} costs={a['costs']} pen={a['pen']} seeds={a['seeds'].tolist()} max_cost={a['max_cost']}"
        return a

    def route(self, lo, dims):
        import torch

        a = self.draw_route(lo, dims, self.rich["route"])
        exp = a["exp"]
        self.count("route", 0 < exp["summary"][1] < exp["summary"][0])
        use_dev = self.dev()
        if self.gpu is None:
            return
        shape = (dims[2], dims[1], dims[0])
        if use_dev:
            dev = self.tensors({"cost": (shape, torch.int32), "parent": (shape, torch.uint8)})
            sd, = self.to_dev(a["sv"])
            sm = self.gpu.export_route_dev(lo, dims, sd.data_ptr(), len(a["sv"]), **a["kw"], cost=dev["cost"].data_ptr(), parent=dev["parent"].data_ptr(), summary=True)
            got = self.fetch(dev)
            got["summary"] = sm
        else:
            got = self.gpu.export_route(lo, dims, a["sv"], **a["kw"], cost=True, parent=True)
        what = self.ctx(f"route {a['what']} dev={use_dev}")
        assert got["cost"].dtype == np.int32 and np.array_equal(got["cost"], exp["cost"]), what
        assert got["parent"].dtype == np.uint8 and np.array_equal(got["parent"], exp["parent"]), what
        assert np.array_equal(got["summary"][:3], exp["summary"]), (got["summary"], exp["summary"], what)

    def paths(self, lo, dims):
        rng = self.rng
        a = self.draw_route(lo, dims, self.rich["paths"])
        field = a["exp"]
        reached = np.argwhere(field["cost"] >= 0)[:, ::-1]
        missed = np.argwhere(field["cost"] < 0)[:, ::-1]
        goals = [reached[i] for i in rng.permutation(len(reached))[:6]]
        if len(missed):
            goals.append(missed[int(rng.integers(0, len(missed)))])
        goals = (np.array(goals + [[-1, 0, dims[2]]], dtype=np.int64).reshape(-1, 3) + np.array(lo)).astype(np.int32)  # (the last one outside the box)
        L, cap = int(rng.choice([1, 3, 64])), int(rng.choice([1, 4, 64]))
        mm = max(1, min(2 ** 20, dims[0] * dims[1] * dims[2] - 1, 8 * sum(dims)))
        exp = path_ref.query(field["parent"], path_ref.ROUTE, lo, goals, L, mm, cap, self.d)
        ok = exp["status"] == 1
        self.count("paths", (ok & (exp["table"][:, 1] < exp["table"][:, 0] + 1)).any() and (exp["status"][:-1] == 0).any())
        use_dev = self.dev()
        if self.gpu is None:
            return
        names = ("status", "way", "length", "table")
        what = self.ctx(f"paths {a['what']} goals={goals.tolist()} lookahead={L} cap={cap} dev={use_dev}")
        if use_dev:  # the kernel on the reference's field
            par, gl = self.to_dev(field["parent"], goals)
            got = {k: v.cpu().numpy() for k, v in self.gpu.query_paths(lo, dims, par, gl, "route", L, None, cap).items()}
        else:        # the host branch
            got = self.gpu.query_paths(lo, dims, field["parent"], goals, "route", L, None, cap)
        same(got, exp, names, "query_paths " + what)
        both = self.gpu.route_paths(lo, dims, a["sv"], goals, **a["kw"], lookahead=L, cap=cap)  # the field of export_route, kept on the device
        assert np.array_equal(both["summary"][:3], field["summary"]), what
        same(both, exp, names, "route_paths " + what)

    # ---- render ---------------------------------------------------------------------------------------------------------------
    def render(self, lo, dims):
        import torch

        rng = self.rng
        for _ in range(1 if self.rich["render"] else 5):
            T = self.T_last(int(rng.integers(1, 3)))
            w, h = [(24, 16), (17, 9), (8, 5)][int(rng.integers(0, 3))]
            K = (0.6 * w, 0.6 * w, 0.5 * w, 0.5 * h)
            mm = int(rng.choice([1000, 4000], p=[0.75, 0.25] if w == 24 else [0.5, 0.5]))  # (the reference walks every pixel's ray in Python)
            flags = int(rng.integers(1, 8))
            exp = render_ref.render_all(T, w, h, K, mm, self.d, self.classes(), (flags,))[0][flags]
            if (exp["status"] == 1).any() and (exp["status"] == 0).any():
                break
        self.count("render", (exp["status"] == 1).any() and (exp["status"] == 0).any())
        use_dev = self.dev()
        if self.gpu is None:
            return
        n = len(T)
        if use_dev:
            dev = self.tensors({"depth": ((n, h, w), torch.int16), "status": ((n, h, w), torch.int8), "voxel": ((n, h, w, 3), torch.int32),
                                "n_unknown": ((n, h, w), torch.int32), "table": ((n, 4), torch.int64)})
            Td, = self.to_dev(T)
            self.gpu.render_depth_dev(Td.data_ptr(), n, w, h, K, mm / 1000.0, **kw3(flags), **{k: t.data_ptr() for k, t in dev.items()})
            got = self.fetch(dev)
            got["depth"] = got["depth"].view(np.uint16)
        else:
            got = self.gpu.render_depth(T_ws=T, width=w, height=h, K=K, max_depth=mm / 1000.0, **kw3(flags))
        what = self.ctx(f"render {n} poses {w} x {h} max_depth={mm} flags={flags} dev={use_dev}")
        flat = {"depth": got["depth"].reshape(-1), "status": got["status"].reshape(-1), "voxel": got["voxel"].reshape(-1, 3),
                "n_unknown": got["n_unknown"].reshape(-1), "table": got["table"]}
        same(flat, exp, ("depth", "status", "voxel", "n_unknown", "table"), what)

    # ---- views ----------------------------------------------------------------------------------------------------------------
    def views(self, lo, dims):
        import torch

        rng, d, b = self.rng, self.d, self.truth()[0]
        count = int(rng.integers(3, 7))
        near = max((count + 1) // 2, count - 2)  # (at most two of the wide fans: the reference walks 96 rays of 90 voxels and more for each)
        # narrow fans (20 x 15 degrees, 40 voxels) keep their bitset in LDS, meet their voxels many times over and cross unknown space
        # before they stop; a 90 x 70 degree fan of 90 voxels spans more than kViewLdsBits voxels however it lies
        parts = [view_ref.random_fans(rng, b, self.cfg, k, 12, 8, R * d, np.deg2rad(h), np.deg2rad(v)) for k, R, h, v in ((near, 40, 20.0, 15.0), (count - near, 90, 90.0, 70.0))]
        p0, p1 = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        vb = np.concatenate([parts[0][2], parts[1][2][1:] + parts[0][2][-1]]).astype(np.int32)
        flags = int(rng.choice([OCC, OCC | INFL, int(rng.integers(1, 8))]))
        box = (lo, dims) if rng.random() < 0.5 else None
        if not self.rich["views"]:  # (until one call had a non-trivial answer: rays that cross unknown space, counted everywhere)
            flags, box = flags & ~UNKNOWN or OCC, None
        shape = (dims[2], dims[1], dims[0])
        exclude = (rng.random(shape) < 0.1).astype(np.uint8) if box is not None and rng.random() < 0.5 else None
        mark = rng.integers(0, 4, size=shape).astype(np.uint8) if box is not None and rng.random() < 0.6 else None
        exp_t, exp_m = view_ref.views(p0, p1, vb, d, self.classes(), flags, box, exclude, None if mark is None else mark.copy())
        if box is None:  # which path a view takes: the bounding box of its start and end voxels against kViewLdsBits
            for k in range(count):
                ends = np.array([[q >> 10 for q in rw.lattice(p, d)] for p in np.concatenate([p0[vb[k]:vb[k + 1]], p1[vb[k]:vb[k + 1]]])])
                bits = int(np.prod(ends.max(0) - ends.min(0) + 1))
                self.lds_views += bits <= VIEW_LDS_BITS
                self.global_views += bits > VIEW_LDS_BITS
        try:
            view_ref.non_vacuous(exp_t)
            rich = True
        except AssertionError:
            rich = False
        self.count("views", rich)
        use_dev = self.dev()
        if self.gpu is None:
            return
        what = self.ctx(f"views {count} fans flags={flags} box={box} exclude={exclude is not None} mark={mark is not None} dev={use_dev}")
        if use_dev:
            a, c, v = self.to_dev(p0, p1, vb)
            dev = self.tensors({"table": ((count, view_ref.ROW), torch.int64)})
            ex = mk = None
            if exclude is not None:
                ex, = self.to_dev(exclude)
            if mark is not None:
                mk, = self.to_dev(mark)
            self.gpu.query_views_dev(a.data_ptr(), c.data_ptr(), v.data_ptr(), count, **kw3(flags), box=box, exclude=None if ex is None else ex.data_ptr(),
                                     mark=None if mk is None else mk.data_ptr(), table=dev["table"].data_ptr())
            got = self.fetch(dev)
            if mk is not None:
                got["mark"] = mk.cpu().numpy()
        else:
            got = self.gpu.query_views(p0, p1, vb, **kw3(flags), box=box, exclude=exclude, mark=False if mark is None else mark.copy())
        view_ref.assert_equal(got["table"], exp_t, got.get("mark"), exp_m, what)

    # ---- boxes ----------------------------------------------------------------------------------------------------------------
    def query_boxes(self, boxes, flags, mg, window, small, use_dev, what):
        boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 6)
        if use_dev:
            bd, = self.to_dev(boxes)
            got, took = self.host_took(len(boxes), lambda: self.gpu.query_boxes(bd, max_grow=mg, window=window, **kw3(flags)), False, what)
            self.gpu.sync()
            return {k: v.cpu().numpy() for k, v in got.items()}, took
        return self.host_took(len(boxes), lambda: self.gpu.query_boxes(boxes, max_grow=mg, window=window, **kw3(flags)), small, what)

    def boxes(self, lo, dims):
        rng, cl = self.rng, self.classes()
        glo, gd = grow(lo, dims, 3)
        v = grid(glo, gd)
        free = v[cl(v) == 0]
        seeds = free[rng.integers(0, len(free), 15)] if len(free) else v[rng.integers(0, len(v), 15)]
        a = np.array(lo) + np.stack([rng.integers(0, dims[x], 10) for x in range(3)], axis=1)
        ext = rng.integers(0, 5, size=(10, 3))
        ext[np.arange(10), rng.integers(0, 3, 10)] = 0  # thin
        far = np.array(lo) - self.n + np.stack([rng.integers(0, dims[x] + 2 * self.n, 14) for x in range(3)], axis=1)  # (across absent blocks past the map's edge)
        boxes = np.concatenate([np.concatenate([seeds, seeds], axis=1), np.concatenate([a, a + ext], axis=1),
                                np.concatenate([far, far + rng.integers(0, 4, size=(14, 3))], axis=1), [[3, 0, 0, 2, 0, 0]]]).astype(np.int32)
        boxes = past_the_mirror(boxes, [3, 0, 0, 2, 0, 0])
        for _ in range(1 if self.rich["boxes"] else 5):
            flags = int(rng.integers(0, 8))
            mg = [int(x) for x in rng.integers(0, 7, 6)] if rng.random() < 0.75 else None
            window = grow(lo, dims, 8) if rng.random() < 0.3 else None
            exp = box_ref.grow_all(boxes, flags, cl, mg, window)
            rich = ((exp["status"] == 1) & (exp["table"][:, 3] > 0) & (exp["closed"] != 0)).any()
            if rich:
                break
        for i in rng.permutation(40)[:5]:
            box_ref.check_properties(boxes[i], flags, cl, mg, window,
                                     (int(exp["status"][i]), tuple(int(x) for x in exp["box"][i]), int(exp["closed"][i]), tuple(int(x) for x in exp["table"][i])))
        self.count("boxes", rich)
        use_dev = self.dev()
        if self.gpu is None:
            return
        what = self.ctx(f"boxes {lo} {dims} flags={flags} max_grow={mg} window={window} dev={use_dev}")
        got, _ = self.query_boxes(boxes, flags, mg, window, False, use_dev, what)
        box_ref.assert_equal(got, exp, what)

    def op_boxes_small(self):
        v, c = self.around_an_obstacle()
        boxes = np.array([np.r_[v, v], np.r_[v + [1, 0, 0], v + [1, 0, 0]], np.r_[v - [0, 2, 1], v - [0, 1, 0]]], dtype=np.int32)
        exp = []
        for i in range(2):
            exp.append(box_ref.grow_all(boxes, OCC, self.classes(), 2))
            if self.gpu is not None:
                what = self.ctx(f"boxes_small {boxes.tolist()} batch {i}")
                got, took = self.query_boxes(boxes, OCC, 2, None, True, False, what)
                box_ref.assert_equal(got, exp[i], what)
            if i == 0:
                self.free_around(c)
        self.count_small("boxes", any(not np.array_equal(exp[0][k], exp[1][k]) for k in box_ref.OUTPUTS), 0 if self.gpu is None else took)

    # ---- nearest --------------------------------------------------------------------------------------------------------------
    def query_nearest(self, pts, C, flags, small, use_dev, what):
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        if use_dev:
            pd, = self.to_dev(pts)
            got, took = self.host_took(len(pts), lambda: self.gpu.query_nearest(pd, C, **kw3(flags)), False, what)
            self.gpu.sync()
            return {k: v.cpu().numpy() for k, v in got.items()}, took
        return self.host_took(len(pts), lambda: self.gpu.query_nearest(pts, C, **kw3(flags)), small, what)

    def aim(self):
        """the centre of a released block and the class bit of all its voxels, if the map holds one (frontier mode)"""
        rel = self.released() if self.cfg.use_exploration_frontiers else []
        if not len(rel):
            return None, 0
        v = rel[0] * self.n + self.n // 2
        return (v + 0.5) * self.d, int(self.classes()(v[None])[0]) & (OCC | UNKNOWN)

    def in_released(self, vox):
        """how many of the voxels [K, 3] lie in released blocks"""
        rel = self.released() if self.cfg.use_exploration_frontiers else []
        keys = set(map(tuple, np.asarray(rel).reshape(-1, 3).tolist()))
        return sum(tuple(g) in keys for g in np.floor_divide(np.asarray(vox, dtype=np.int64).reshape(-1, 3), self.n).tolist())

    def nearest(self, lo, dims):
        rng, d, n = self.rng, self.d, self.n
        wlo, whi = self.world(lo, dims)
        pts = np.concatenate([rng.uniform(wlo - 2 * d, whi + 2 * d, size=(40, 3)),
                              rw.centres(np.array(lo) + np.stack([rng.integers(0, dims[x], 20) for x in range(3)], axis=1), self.cfg)])
        target, bit = self.aim()
        if target is not None:
            pts[0] = target
        for _ in range(1 if self.rich["nearest"] else 5):
            C = int(rng.choice([1, n, n + 1, min(3 * n + 1, 24)]))
            flags = int(rng.integers(1, 8)) | bit  # (the class of the released block counts as an obstacle)
            if C > 16:  # (the reference reads (2C + 1)^3 voxels per point)
                pts = pts[:12]
            exp, _ = nearest_ref.nearest_all(pts, d, C, self.classes(), flags)
            rich = ((exp["status"] == 1) & (exp["sq"] > 0)).any() and (exp["status"] == 0).any()
            if rich:
                break
        self.released_hit += self.in_released(exp["voxel"][exp["status"] == 1])  # answers that are voxels of released blocks
        pts = past_the_mirror(pts, [np.nan] * 3)
        exp = {k: np.concatenate([v, nearest_ref.nearest_all(pts[len(v):], d, C, self.classes(), flags)[0][k]]) for k, v in exp.items()}
        self.count("nearest", rich)
        use_dev = self.dev()
        if self.gpu is None:
            return
        what = self.ctx(f"nearest {lo} {dims} C={C} flags={flags} dev={use_dev}")
        got, _ = self.query_nearest(pts, C, flags, False, use_dev, what)
        nearest_ref.assert_equal(got, exp, what)

    def op_nearest_small(self):
        v, c = self.around_an_obstacle()
        pts = c + self.rng.uniform(-2.0, 2.0, size=(5, 3)) * self.d
        exp = []
        for i in range(2):
            exp.append(nearest_ref.nearest_all(pts, self.d, 3, self.classes(), OCC)[0])
            if self.gpu is not None:
                what = self.ctx(f"nearest_small around {v.tolist()} batch {i}")
                got, took = self.query_nearest(pts, 3, OCC, True, False, what)
                nearest_ref.assert_equal(got, exp[i], what)
            if i == 0:
                self.free_around(c)
        self.count_small("nearest", any(not np.array_equal(exp[0][k], exp[1][k]) for k in ("status", "voxel", "sq")), 0 if self.gpu is None else took)

    # ---- sweeps ---------------------------------------------------------------------------------------------------------------
    def query_sweeps(self, p0, p1, r, flags, small, use_dev, what):
        p0, p1 = (np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3) for p in (p0, p1))
        if use_dev:
            a, c = self.to_dev(p0, p1)
            got, took = self.host_took(len(p0), lambda: self.gpu.query_sweeps(a, c, r, **kw3(flags)), False, what)
            self.gpu.sync()
            return {k: v.cpu().numpy() for k, v in got.items()}, took
        return self.host_took(len(p0), lambda: self.gpu.query_sweeps(p0, p1, r, **kw3(flags)), small, what)

    def edge_rays(self, occupied, r):
        """six rays of four steps past the blocks of the last op_import, which lie alone in unknown space.  o is an OCCUPIED voxel of
        the first voxel layer of those blocks on an axis a, the ray runs along another axis and ends at u = o - r on a, below all of
        them.  Its balls meet that layer alone, at distance r exactly: o, or another voxel of the layer on the way to it, stops the ray
        from the last block layer on a of the block box around the ball.  That layer starts a block, so past the cache's bound the
        box is kSweepNB + 1 blocks wide on a.  (A generator of its own: the sequence's draws stay what they are.)"""
        rng, n = np.random.default_rng([self.seed, self.calls["sweeps"]]), self.n
        far = occupied[(occupied[:, 0] < -20 * n) & (occupied[:, 1] < -20 * n)]
        if not len(far):
            return None
        far = far[(far[:, 0] < far[:, 0].min() + 2 * n) & (far[:, 1] < far[:, 1].min() + 2 * n)]  # (imports lie three blocks apart, two blocks wide)
        p0, p1 = [], []
        for a in (0, 1, 2):
            layer = far[far[:, a] == far[:, a].min()]
            for b in ((a + 1) % 3, (a + 2) % 3):
                u = layer[int(rng.integers(0, len(layer)))].copy()
                u[a] -= r
                start = u.copy()
                start[b] += 4 * int(rng.choice([-1, 1]))
                p0.append(start)
                p1.append(u)
        return rw.centres(np.array(p0), self.cfg), rw.centres(np.array(p1), self.cfg)

    def edge_stopped(self, exp, r, flags):
        """how many rays of a reference answer stop past their start voxel (in k_sweeps' cap, not in the start ball's search) on an
        OCCUPIED voxel in the first or the last block layer of the block box around the ball.  Past the cache's bound only where a
        slot cache of kSweepNB blocks per axis would answer otherwise: the box is kSweepNB + 1 blocks wide on that axis, and the voxel
        kSweepNB blocks further in, which shares the torus cell, is no obstacle under these flags."""
        n, cl, count = self.n, self.classes(), 0
        for i in np.flatnonzero((exp["status"] == 1) & (exp["n_steps"] >= 1)):
            u, o = exp["voxel"][i].astype(np.int64), exp["hit"][i].astype(np.int64)
            if not int(cl(o[None])[0]) & OCC:
                continue
            lo, hi, g = (u - r) // n, (u + r) // n, o // n
            for a in range(3):
                if g[a] != lo[a] and g[a] != hi[a]:
                    continue
                if r > self.r_c:
                    twin = o.copy()
                    twin[a] += SWEEP_NB * n * (1 if g[a] == lo[a] else -1)
                    if hi[a] - lo[a] != SWEEP_NB or int(cl(twin[None])[0]) & flags:
                        continue
                count += 1
                break
        return count

    def sweeps(self, lo, dims):
        rng, d = self.rng, self.d
        wlo, whi = self.world(lo, dims)
        a, c = rw.uniform_rays(rng, wlo - 2 * d, whi + 2 * d, 40)
        c = a + np.clip(c - a, -7.5 * d, 7.5 * d)  # (at most 8 voxels per axis: 25 path voxels)
        sa, sc = rw.special_rays(rng, wlo, whi, d, count=2)
        pick = rng.permutation(len(sa))[:10]
        p0, p1 = np.concatenate([a, sa[pick]]), np.concatenate([c, sc[pick]])
        occupied = self.occupied()
        if len(occupied):  # (five of the short rays end in OCCUPIED voxels in and around the box)
            close = occupied[((occupied >= np.array(lo) - 8) & (occupied < np.array(lo) + np.array(dims) + 8)).all(axis=1)]
            if len(close):
                p1[1:6] = rw.centres(close[rng.integers(0, len(close), 5)], self.cfg)
                p0[1:6] = p1[1:6] + rng.uniform(-7.5, 7.5, size=(5, 3)) * d
        target, bit = self.aim()
        if target is not None:
            p1[0] = target
            p0[0] = target + rng.uniform(-4.0, 4.0, 3) * d
        radii = [1, self.r_c, 0] + ([self.r_c + 1] if self.r_c < sweep_ref.MAX_RADIUS else [])
        r = radii[self.calls["sweeps"] % len(radii)]  # (every radius in turn: the two around the cache's bound are met often)
        edge = self.edge_rays(occupied, r) if r >= self.r_c and len(occupied) else None
        if edge is not None:  # (at the cache's bound and past it: six rays stopped from the outermost block layer of the ball's block box)
            p0[6:12], p1[6:12] = edge
        if r > 8:  # (the reference's time goes with r^3: twelve of the short rays, the five that end in obstacles among them, three special ones)
            keep = np.r_[0:12, 40:43]
            p0, p1 = p0[keep], p1[keep]
        for _ in range(1 if self.rich["sweeps"] or r != 1 else 4):  # (radius 1 until one call had a non-trivial answer: up to four draws of the flags)
            flags = int(rng.integers(1, 8)) | bit | (OCC if r > 1 else 0)  # (the released block's class; a large ball meets an OCCUPIED voxel: a stop at either side of the cache's bound)
            if r >= self.r_c:  # (a ball of this size holds unknown space wherever it starts, which would stop every ray at once)
                flags &= ~UNKNOWN
            exp =sweep_ref.sweep_all(p0, p1, d, r, self.classes(), (flags,))[0][flags]
            stop = exp["status"] == 1
            if (stop & (exp["hit_sq"] > 0)).any() and (exp["status"] == 0).any():
                break
        self.sweep_stops[r] = self.sweep_stops.get(r, 0) + bool(stop.any())
        self.edge_stops[r] = self.edge_stops.get(r, 0) + self.edge_stopped(exp, r, flags)
        self.released_hit += self.in_released(exp["hit"][stop]) + self.in_released(exp["voxel"][exp["status"] >= 0])  # obstacles in released blocks, rays that end in one
        p0, p1 = past_the_mirror(p0, [np.nan] * 3), past_the_mirror(p1, [np.nan] * 3)
        exp = {k: np.concatenate([v, sweep_ref.sweep_all(p0[len(v):], p1[len(v):], d, r, self.classes(), (flags,))[0][flags][k]]) for k, v in exp.items()}
        self.count("sweeps", (stop & (exp["hit_sq"][:len(stop)] > 0)).any() and (exp["status"][:len(stop)] == 0).any())
        use_dev = self.dev()
        if self.gpu is None:
            return
        what = self.ctx(f"sweeps {lo} {dims} r={r} flags={flags} dev={use_dev}")
        got, _ = self.query_sweeps(p0, p1, r, flags, False, use_dev, what)
        sweep_ref.assert_equal(got, exp, what)

    def op_sweeps_small(self):
        v, c = self.around_an_obstacle()
        p0 = c + self.rng.uniform(-3.0, 3.0, size=(5, 3)) * self.d
        p1 = 2 * c - p0  # (every ray passes the voxel)
        r = int(self.rng.choice([1, 2]))
        exp = []
        for i in range(2):
            exp.append(sweep_ref.sweep_all(p0, p1, self.d, r, self.classes(), (OCC,))[0][OCC])
            if self.gpu is not None:
                what = self.ctx(f"sweeps_small through {v.tolist()} r={r} batch {i}")
                got, took = self.query_sweeps(p0, p1, r, OCC, True, False, what)
                sweep_ref.assert_equal(got, exp[i], what)
            if i == 0:
                self.free_around(c)
        self.count_small("sweeps", any(not np.array_equal(exp[0][k], exp[1][k]) for k in ("status", "voxel", "hit", "hit_sq")), 0 if self.gpu is None else took)

    # ---- score ----------------------------------------------------------------------------------------------------------------
    def score_poses(self, pts, T, classes, box, field, cap, small, use_dev, what):
        if use_dev:
            pd, Td = self.to_dev(pts, T)
            fd = None if field is None else self.to_dev(field)[0]
            got, took = self.host_took(len(T), lambda: self.gpu.score_poses(pd, Td, classes, box, fd, cap), False, what)
            self.gpu.sync()
            return got["table"].cpu().numpy(), took
        got, took = self.host_took(len(T), lambda: self.gpu.score_poses(pts, T, classes, box, field, cap), small, what)
        return got["table"], took

    def score(self, lo, dims):
        from mlmapping_amd.mlmap import backproject, pose_grid

        rng, d, cfg = self.rng, self.d, self.cfg
        cloud = backproject(self.last[0], (cfg.cam_fx, cfg.cam_fy, cfg.cam_cx, cfg.cam_cy), step=4)
        if not self.rich["score"]:  # (until one call had a non-trivial answer: the box moves onto an inflated voxel, if the map has one)
            b = self.truth()[0]
            blk, cid = np.nonzero((b["infl"] == ord("o")) & (b["collapsed"] == 0)[:, None])
            if len(blk):
                i = int(rng.integers(0, len(blk)))
                v = b["keys"][blk[i]].astype(np.int64) * self.n + np.array([cid[i] % self.n, (cid[i] // self.n) % self.n, cid[i] // (self.n * self.n)])
                lo = [int(v[x]) - dims[x] // 2 for x in range(3)]
                self.note(lo, dims)
        # the candidates lie around the last frame's pose, moved so that one of the frame's points falls into the middle of the box
        T0 = self.T_last(1, 0.02)[0]
        w = score_ref.world(cloud, T0[None])[0]
        T0[9:] += (np.array(lo) + np.array(dims) / 2.0) * d - w[int(rng.integers(0, len(w)))]
        valid, vox = score_ref.voxels(score_ref.world(cloud, T0[None]), d)
        inside = valid[0] & ((vox[0] >= np.array(lo)) & (vox[0] < np.array(lo) + np.array(dims))).all(axis=1)
        first = rng.permutation(np.flatnonzero(inside))[:100]  # (up to half of the points fall into the box of the field ...
        bits = self.classes()(vox[0])
        other = [rng.permutation(np.flatnonzero(~inside & valid[0] & ((bits & f) != 0)))[:30] for f in (OCC, INFL)]  # ... some on surfaces and beside them)
        taken = np.concatenate([first] + other)
        rest = rng.permutation(np.setdiff1d(np.arange(len(cloud)), taken))[:200 - len(taken)]
        pts = np.ascontiguousarray(cloud[np.concatenate([taken, rest])])
        T = pose_grid(T0, d, half_xyz=(3, 2, 0), yaw_deg=(-1, 1))
        assert len(pts) == 200 and len(T) == 70, (len(pts), len(T))
        C, flags = 4, int(rng.integers(1, 8))
        field = esdf_ref.expected((self.bits(*grow(lo, dims, C)) & flags) != 0, C, False, d)["sqdist"]
        mode = int(rng.integers(0, 3))  # classes, a field, both
        classes, box, cap = mode != 1, (lo, dims) if mode else None, int(rng.choice([1, 64]))
        exp = score_ref.score(pts, T, d, self.classes() if classes else None, box, field if mode else None, cap)
        full = score_ref.score(pts, T, d, self.classes(), (lo, dims), field, C * C)  # match_pose's table
        try:
            score_ref.non_vacuous(full)
            rich = True
        except AssertionError:
            rich = False
        self.count("score", rich)
        use_dev = self.dev()
        if self.gpu is None:
            return
        what = self.ctx(f"score {lo} {dims} mode={mode} sq_cap={cap} flags={flags} dev={use_dev}")
        got, _ = self.score_poses(pts, T, classes, box, field if mode else None, cap, False, use_dev, what)
        score_ref.assert_equal(got, exp, what)
        m = self.gpu.match_pose(pts, T, lo, dims, max_dist=C, **kw3(flags), classes=True)
        score_ref.assert_equal(m["table"], full, "match_pose " + what)
        assert m["best"] == score_ref.best_row(full), what

    def op_score_small(self):
        v, c = self.around_an_obstacle()
        pts = self.rng.uniform(-1.5, 1.5, size=(50, 3)) * self.d
        T = np.tile(score_ref.IDENTITY, (8, 1))
        T[:, 9:] = c + self.rng.uniform(-1.0, 1.0, size=(8, 3)) * self.d
        T[0, 9:] = c
        exp = []
        for i in range(2):
            exp.append(score_ref.score(pts, T, self.d, self.classes()))
            if self.gpu is not None:
                what = self.ctx(f"score_small around {v.tolist()} batch {i}")
                got, took = self.score_poses(pts, T, True, None, None, 64, True, False, what)
                score_ref.assert_equal(got, exp[i], what)
            if i == 0:
                self.free_around(c)
        self.count_small("score", not np.array_equal(exp[0], exp[1]), 0 if self.gpu is None else took)

    def before_the_tail(self):
        """each small variant once"""
        for k in SMALL:
            self.log.append(k + "_small")
            getattr(self, f"op_{k}_small")()

    # ---- the conditions -------------------------------------------------------------------------------------------------------
    def counters(self):
        return {"calls": self.calls, "unsynced": self.unsynced, "in_async": self.in_async, "after_growth": self.after_growth, "rich": self.rich,
                "small_calls": self.small_calls, "small_shown": self.small_shown, "sweep_stops": self.sweep_stops, "edge_stops": self.edge_stops, "released_hit": self.released_hit,
                "lds_views": int(self.lds_views), "global_views": int(self.global_views), "unit_routes": self.unit_routes, "pinned": self.pinned,
                "straddle": self.straddle, "thin": self.thin, "absent": self.absent, "imports": self.imports, "stream_ops": self.stream_ops}

    def check_not_vacuous(self):
        super().check_not_vacuous()
        what = self.ctx(str(self.counters()))
        assert all(self.small_shown[k] >= 1 for k in SMALL), what
        assert self.lds_views >= 1 and self.global_views >= 1 and self.unit_routes >= 1, what
        if self.cfg.use_exploration_frontiers:
            assert self.released_hit >= 1, what
        if self.r_c < sweep_ref.MAX_RADIUS:
            assert self.sweep_stops.get(self.r_c, 0) >= 1 and self.sweep_stops.get(self.r_c + 1, 0) >= 1, what
            assert self.edge_stops.get(self.r_c, 0) >= 1 and self.edge_stops.get(self.r_c + 1, 0) >= 1, what


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


CASES = [(n, d, None) for n, d in GEOMETRIES] + [(GEOMETRIES[s % len(GEOMETRIES)] + (s,)) for s in EXTRA]  # (more seeds: MLM_STRESS_SEEDS)


@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("n,d,seed", CASES)
def test_random_query_sequences(mods, knobs, n, d, seed, explore):
    MLMap, OracleMap = mods
    fixed = seed is None
    seed = CASE_SEED.get((n, explore), SEED) if fixed else seed
    cfg = config(n, d, explore)
    knobs.set("pool_grow", 1)
    gpu, cpu = MLMap(cfg, max_blocks=MAX_BLOCKS, max_points=cfg.width * cfg.height, max_batch=4), OracleMap(cfg)
    s = QuerySequence(cfg, seed, gpu, cpu)
    s.run(STEPS)
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), s.ctx("the maps at the end"))
    st = gpu.frame_stats()
    assert st["n_pool_grows"] >= 1 and s.grew_in_flight >= 1, (st, s.grew_in_flight, s.ctx("pool growth"))
    if fixed:
        s.check_not_vacuous()
        assert all(s.host_items[k] > 0 for k in SMALL), s.ctx(f"answered on the host: {s.host_items}")
    gpu.close()
