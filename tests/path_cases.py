"""The fields and goals that tests/test_path_plan.py (CPU driver) and tests/test_gpu_paths.py (kernel, staged kernel, host branch) put
to mlm_query_paths, with their answers by tests/path_ref.py, computed once per session and shared.  Nothing here calls the code under test.

A case is a dict: name, group, parent (uint8 [z][y][x]), kind, lo, goals (n x 3 absolute), lookahead, max_moves, cap, fill (the
way3 buffer's content before the call, (n, cap, 3) int32)."""
import numpy as np

from mlmapping_amd.config import S1
from mlmapping_amd.mlmap import MLM_PATH_REACH, MLM_PATH_ROUTE, MLM_PATH_ROW
from tests import path_ref as ref
from tests import reach_ref, route_ref

assert (ref.REACH, ref.ROUTE, ref.ROW) == (MLM_PATH_REACH, MLM_PATH_ROUTE, MLM_PATH_ROW)  # the kinds the cases are written in are the binding's
D_SUB = S1.subbox_d_xyz  # 0.1: not a float32 value, so the contract's (double)(float) rounding shows; the GPU test's handle has it too
FILL = -123456789
_cases = None
_answers = {}
stats = {}   # per group: ties seen (set), [candidates, refused]


def case(name, group, parent, kind, lo, goals, lookahead, max_moves, cap=6, fill=FILL):
    g = np.ascontiguousarray(np.asarray(goals, dtype=np.int64).reshape(-1, 3).astype(np.int32))
    return {"name": name, "group": group, "parent": np.ascontiguousarray(parent, dtype=np.uint8), "kind": kind,
            "lo": np.asarray(lo, dtype=np.int32), "goals": g, "lookahead": int(lookahead), "max_moves": int(max_moves), "cap": int(cap),
            "fill": np.full((len(g), int(cap), 3), fill, dtype=np.int32)}


def reached_goals(parent, lo, every, M):
    v = np.argwhere(parent <= M)[::every, ::-1]
    return v + np.asarray(lo)


_random = None


def random_fields():
    global _random
    if _random is None:
        _random = _random_fields()
    return _random


def _random_fields():
    """[(name, parent, kind, lo)]: genuine fields over random masks, for the three connectivities with penalties, and reach fields"""
    out = []
    rng = np.random.default_rng(2024)
    for shape, density, lo in (((6, 20, 28), 0.12, (-7, 100, 3)), ((3, 17, 23), 0.08, (2 ** 31 - 1 - 23, -2 ** 31, -5))):
        for conn, costs, pen in ((6, (10, 14, 17), (7,)), (18, (10, 14, 17), (40, 15, 5)), (26, (10, 14, 17), (40, 15, 5)), (26, (3, 3, 3), ())):
            g = len(pen) + 1
            obs = rng.random(tuple(n + 2 * g for n in shape)) < density
            cls = route_ref.classes(obs, 0, len(pen))
            free = np.argwhere(cls != route_ref.BLOCKED)[:, ::-1]
            seeds = free[rng.integers(len(free), size=2)]
            f = route_ref.route(cls, seeds, conn, costs, pen)
            out.append((f"route{conn}-{'x'.join(map(str, shape))}-{len(pen)}", f["parent"], ref.ROUTE, lo))
        T = ~(rng.random(shape) < density)
        free = np.argwhere(T)[:, ::-1]
        out.append((f"reach-{'x'.join(map(str, shape))}", reach_ref.reach(T, free[rng.integers(len(free), size=2)])["parent"], ref.REACH, lo))
    return out


def corrupt(parent, rng, count):
    """a copy with `count` bytes replaced by arbitrary values (every byte value is legal input)"""
    p = parent.copy()
    at = rng.integers(p.size, size=count)
    p.reshape(-1)[at] = rng.integers(0, 256, size=count)
    return p


def maze():
    """(parent, far goal): the 26-connected route field of a serpentine maze of 3 x 41 x 41 from the corner (0, 0, 0)"""
    blocked = reach_ref.serpentine_slab(41, 41, 3)
    cls = np.where(blocked, route_ref.BLOCKED, 0).astype(np.uint8)
    f = route_ref.route(cls, [(0, 0, 0)], 26, (10, 14, 17), ())
    far = np.unravel_index(f["cost"].argmax(), cls.shape)[::-1]
    return f["parent"], tuple(int(v) for v in far)


def handmade():
    """[case]: fields no export call writes"""
    out = []
    S = route_ref.SEED
    code = {o: c for c, o in enumerate(ref.OFFSETS)}
    # a two-voxel cycle, a code pointing out of the box, one pointing at a 255, bytes 27 .. 254 as goals and as targets
    p = np.full((2, 3, 8), 255, dtype=np.uint8)
    p[0, 0, 0], p[0, 0, 1] = code[(1, 0, 0)], code[(-1, 0, 0)]          # cycle
    p[0, 1, 0] = code[(-1, 0, 0)]                                       # out of the box
    p[0, 1, 7] = code[(1, 1, 1)]                                        # out of the box through a corner
    p[0, 2, 3], p[0, 2, 2] = code[(-1, 0, 0)], 255                      # at a 255
    p[1, 0, 3], p[1, 0, 4] = code[(1, 0, 0)], 27                        # at a 27
    p[1, 1, 3], p[1, 1, 4] = code[(1, 0, 0)], 254
    p[1, 2, 0], p[1, 2, 1], p[1, 2, 2] = S, code[(-1, 0, 0)], code[(-1, 0, 0)]  # a sound path beside them
    p[1, 2, 5] = 100
    goals = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (7, 1, 0), (3, 2, 0), (3, 0, 1), (3, 1, 1), (2, 2, 1), (0, 2, 1), (5, 2, 1), (4, 0, 1),
             (-1, 0, 0), (8, 0, 0), (0, 3, 0), (0, 0, 2), (0, -1, 0), (2 ** 31 - 1, 0, 0), (-2 ** 31, -2 ** 31, -2 ** 31)]
    for mm in (1, 2, 5):
        out.append(case(f"hand-broken-mm{mm}", "hand", p, ref.ROUTE, (0, 0, 0), goals, 4, mm))
    lo = (10, -20, 30)
    out.append(case("hand-broken-lo", "hand", p, ref.ROUTE, lo, np.asarray(goals[:11]) + lo, 2, 7))
    # the same bytes read as a reach field: codes 6 .. 25 are moves no more (6 is the seed, the others closed)
    out.append(case("hand-as-reach", "hand", p, ref.REACH, (0, 0, 0), goals, 4, 5))
    # diagonals whose grazed voxel is closed: a 2-axis tie in a slab, a 3-axis tie in a cube; mlm_query_rays' own path between the
    # centres passes (it takes one of the tied axes first and never looks at the other voxels), vis must refuse.  The path runs
    # round the closed voxel, so only the shortening could cut the corner.
    q = np.full((1, 3, 3), 255, dtype=np.uint8)
    q[0, 0, 0] = S
    q[0, 1, 0], q[0, 2, 0], q[0, 2, 1], q[0, 2, 2] = code[(0, -1, 0)], code[(0, -1, 0)], code[(-1, 0, 0)], code[(-1, 0, 0)]
    q[0, 1, 1], q[0, 1, 2], q[0, 0, 1] = code[(-1, 0, 0)], code[(-1, 0, 0)], code[(-1, 0, 0)]  # (1, 1), (2, 1), (1, 0): open, off the path
    out.append(case("hand-tie2-open", "hand", q, ref.ROUTE, (0, 0, 0), [(2, 2, 0), (1, 2, 0)], 8, 16))
    q2 = q.copy()
    q2[0, 1, 2] = 255  # (2, 1) closed: the diagonal (2, 2) -> (0, 0) grazes it at its first tie
    out.append(case("hand-tie2-closed", "hand", q2, ref.ROUTE, (0, 0, 0), [(2, 2, 0), (1, 2, 0)], 8, 16))
    r = np.full((2, 2, 2), 255, dtype=np.uint8)
    r[0, 0, 0] = S
    r[0, 0, 1], r[0, 1, 1], r[1, 1, 1] = code[(-1, 0, 0)], code[(0, -1, 0)], code[(0, 0, -1)]
    out.append(case("hand-tie3-closed", "hand", r, ref.ROUTE, (0, 0, 0), [(1, 1, 1)], 8, 16))
    r2 = np.full((2, 2, 2), code[(-1, 0, 0)], dtype=np.uint8)
    r2[:, :, 0] = code[(0, -1, 0)]
    r2[:, 0, 0] = code[(0, 0, -1)]
    r2[0, 0, 0] = S
    out.append(case("hand-tie3-open", "hand", r2, ref.ROUTE, (0, 0, 0), [(1, 1, 1)], 8, 16))
    r3 = r2.copy()
    r3[1, 0, 1] = 255  # (1, 0, 1): one of the six grazed voxels closed, off the path
    out.append(case("hand-tie3-one-closed", "hand", r3, ref.ROUTE, (0, 0, 0), [(1, 1, 1)], 8, 16))
    return out


def build():
    global _cases
    if _cases is not None:
        return _cases
    out = []
    rng = np.random.default_rng(77)
    for name, parent, kind, lo in random_fields():
        M = ref.seed_code(kind)
        goals = reached_goals(parent, lo, 7, M)
        extra = np.concatenate([np.argwhere(parent > M)[:3, ::-1] + np.asarray(lo), np.asarray(lo)[None] + [[-1, 0, 0], [0, parent.shape[1], 0]]])
        for L in (1, 2, 16):
            out.append(case(f"{name}-L{L}", "random", parent, kind, lo, np.concatenate([goals, extra]), L, 4096))
        out.append(case(f"{name}-short", "random", parent, kind, lo, goals, 16, 6))
        out.append(case(f"{name}-corrupt", "random", corrupt(parent, rng, parent.size // 12), kind, lo, goals, 16, 64))
    mz, far = maze()
    others = np.argwhere(mz <= route_ref.SEED)[::397, ::-1]
    K = len(route_ref.walk(mz, far)) - 1
    for L in (63, 64, 65, 130):
        out.append(case(f"maze-L{L}", "maze", mz, ref.ROUTE, (5, 5, 5), np.concatenate([[far], others]) + 5, L, 4096))
    for mm in (K - 1, K, K + 1):
        out.append(case(f"maze-mm{mm - K:+d}", "maze", mz, ref.ROUTE, (0, 0, 0), [far], 64, mm))
    slab = route_ref.route(np.zeros((2, 70, 200), dtype=np.uint8), [(0, 0, 0)], 26, (10, 14, 17), ())["parent"]
    for L in (7, 64, 130, 4096):
        out.append(case(f"slab-L{L}", "slab", slab, ref.ROUTE, (0, 0, 0), [(199, 0, 0), (199, 69, 1), (150, 0, 1), (0, 69, 0), (64, 0, 0), (65, 0, 0)], L, 4096))
    out += handmade()
    # cap: 0, 1, W - 1, W, W + 1 on a goal of the first random field with W >= 3
    name, parent, kind, lo = random_fields()[2]
    goals = reached_goals(parent, lo, 7, ref.seed_code(kind))
    full = ref.query(parent, kind, lo, goals, 16, 4096, 0, D_SUB)
    i = int(np.argmax(full["table"][:, 1]))
    W = int(full["table"][i, 1])
    assert W >= 3
    for cap in (0, 1, W - 1, W, W + 1):
        out.append(case(f"cap{cap - W:+d}", "cap", parent, kind, lo, goals[[i, 0, i]], 16, 4096, cap=cap))
    _cases = out
    return out


def answer(c):
    """the reference's outputs of a case, computed once"""
    if c["name"] not in _answers:
        st = stats.setdefault(c["group"], {"ties": set(), "counts": [0, 0]})
        detail = []
        a = ref.query(c["parent"], c["kind"], c["lo"], c["goals"], c["lookahead"], c["max_moves"], c["cap"], D_SUB, way=c["fill"],
                      seen_ties=st["ties"], counts=st["counts"], detail=detail)
        a["detail"] = detail
        _answers[c["name"]] = a
    return _answers[c["name"]]


def assert_same(got, exp, what):
    """byte for byte: status, way, table, and length by its 64 bits"""
    for k in ("status", "way", "table"):
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k)
        bad = np.argwhere(got[k] != exp[k])
        assert len(bad) == 0, (what, k, bad[:5].tolist(), got[k][tuple(bad[0])], exp[k][tuple(bad[0])])
    assert np.array_equal(got["length"].view(np.uint64), exp["length"].view(np.uint64)), (what, "length")
