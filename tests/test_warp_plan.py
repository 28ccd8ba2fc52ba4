"""mlm_warp_blocks on the CPU: the rule of mlmapping_amd/csrc/mlm_warp.h — argument check, gather, live predicate, candidate rule,
emission order — run as the device phases run it (candidates, sort, count, scan, write) by tests/cpp/warp_driver.cpp, built with
g++ -fsanitize=address,undefined, and held byte for byte to the contract in numpy (tests/warp_ref.py), which is itself held to the
properties the contract states."""
import os
import subprocess

import numpy as np
import pytest

from tests import warp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlmapping_amd", "csrc")
NS = [2, 3, 4, 8]
NBS = [0, 1, 2, 63, 64, 65, 257]
D_SUB = 0.1
PLANES = ("keys", "log_odds", "occ", "infl")
GENERAL = ref.make_T(ref.rot(30.0, 7.0, -3.0), (0.23, -0.41, 0.17))  # yaw 30, pitch 7, roll -3 degrees; (2.3, -4.1, 1.7) voxels


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("warp")
    exe = d / "warp_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "warp_driver.cpp"), "-o", str(exe)])

    def run(blocks, n, T, key_lo=None, key_dims=None, flags=0, cap=None, want_out=True, d_sub=D_SUB):
        C = n ** 3
        nb = len(blocks["keys"])
        cap = nb * 64 + 64 if cap is None else cap
        lo3 = [0, 0, 0] if key_lo is None else [int(v) for v in key_lo]
        dims3 = [0, 0, 0] if key_dims is None else [int(v) for v in key_dims]
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([nb, n, flags, cap, T is not None, key_lo is not None, key_dims is not None, *lo3, *dims3, int(want_out), 0, 0],
                             dtype=np.int64).tobytes())
            f.write(np.array([d_sub, *(np.zeros(12) if T is None else np.asarray(T, dtype=np.float64).reshape(12))], dtype=np.float64).tobytes())
            for k, dt in (("keys", np.int32), ("log_odds", np.float32), ("occ", np.uint8), ("infl", np.uint8), ("collapsed", np.uint8)):
                f.write(np.ascontiguousarray(blocks[k], dtype=dt).tobytes())
        subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
        raw = open(d / "out.bin", "rb").read()
        head = np.frombuffer(raw[:80], dtype=np.int64)
        rows, at, out = int(head[5]), 80, {}
        for k, dt, cols in (("keys", np.int32, 3), ("log_odds", np.float32, C), ("occ", np.uint8, C), ("infl", np.uint8, C)):
            size = rows * cols * np.dtype(dt).itemsize
            out[k] = np.frombuffer(raw[at:at + size], dtype=dt).reshape(rows, cols)
            at += size
        assert at == len(raw)
        out.update(status=int(head[0]), code=int(head[1]), summary=head[2:].copy())
        return out

    return run


def cube_keys(rng, count, centre=(0, 0, 0)):
    """count distinct keys of a cube around `centre`: both sides of zero"""
    side = max(2, int(np.ceil((2.5 * count) ** (1 / 3))))
    flat = rng.choice(side ** 3, count, replace=False)
    keys = np.stack([flat % side, (flat // side) % side, flat // (side * side)], axis=1) - side // 2 + np.asarray(centre)
    return keys[rng.permutation(count)].astype(np.int32).reshape(count, 3)


def make_blocks(rng, keys, cells, released=0.3):
    """distinct log-odds per voxel, random classes, random released flags (as test_crop_plan.make_blocks)"""
    nb = len(keys)
    lo = (np.arange(nb * cells, dtype=np.float32).reshape(nb, cells) * np.float32(0.25) - np.float32(7.0))
    occ = rng.choice(np.frombuffer(b"ufo", dtype=np.uint8), size=(nb, cells))
    infl = rng.choice(np.frombuffer(b"uo", dtype=np.uint8), size=(nb, cells))
    return {"keys": np.asarray(keys, dtype=np.int32).reshape(nb, 3), "log_odds": lo, "occ": occ, "infl": infl,
            "collapsed": (rng.random(nb) < released).astype(np.uint8)}


def same(a, b, what=""):
    for k in PLANES:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {k}"


def same_counts(got, want, what=""):
    """summary [0], [2] .. [7]; [1] is an implementation count >= [2]"""
    g, w = np.asarray(got), np.asarray(want)
    assert g[0] == w[0] and g[2:].tolist() == w[2:].tolist() and g[1] >= g[2], (what, g, w)


def voxel_map(blocks, n):
    """{global voxel (x, y, z): (log_odds bits, occ, infl)} of every voxel of every block, released blocks expanded"""
    b = ref.sorted_blocks(blocks)
    cc = ref.cell_coords(n)
    out = {}
    for key, lo, occ, infl in zip(b["keys"].astype(np.int64), b["log_odds"].view(np.uint32), b["occ"], b["infl"]):
        v = key[None, :] * n + cc
        out.update(zip(map(tuple, v.tolist()), zip(lo.tolist(), occ.tolist(), infl.tolist())))
    return out


def blocks_from_voxels(vox, n):
    """the blocks that hold the voxels of `vox`, ascending keys, every other voxel 0.0f / 'u' / 'u'"""
    C = n ** 3
    keys = sorted({(x // n, y // n, z // n) for x, y, z in vox})
    row = {k: i for i, k in enumerate(keys)}
    lo = np.zeros((len(keys), C), dtype=np.uint32)
    occ = np.full((len(keys), C), ref.U, dtype=np.uint8)
    infl = np.full((len(keys), C), ref.U, dtype=np.uint8)
    for (x, y, z), (L, o, i) in vox.items():
        r, c = row[(x // n, y // n, z // n)], ((z % n) * n + (y % n)) * n + (x % n)
        lo[r, c], occ[r, c], infl[r, c] = L, o, i
    return {"keys": np.array(keys, dtype=np.int32).reshape(-1, 3), "log_odds": lo.view(np.float32), "occ": occ, "infl": infl}


@pytest.mark.parametrize("n", NS)
def test_identity_returns_the_sorted_blocks(driver, n):
    rng = np.random.default_rng(10 + n)
    for nb in NBS:
        blocks = make_blocks(rng, cube_keys(rng, nb), n ** 3)
        want = ref.warp(blocks, ref.make_T(), n, D_SUB)
        same(want, ref.sorted_blocks(blocks), f"identity n {n} nb {nb}")
        vox = (blocks["collapsed"] == 0)[:, None] & np.ones((1, n ** 3), bool)
        assert want["summary"][4] == nb * n ** 3 and want["summary"][2] == nb
        assert want["summary"][7] == int(((blocks["infl"] == ref.O) & vox).sum())
        got = driver(blocks, n, ref.make_T())
        assert got["status"] == 0
        same(got, want, f"driver identity n {n} nb {nb}")
        same_counts(got["summary"], want["summary"])


@pytest.mark.parametrize("n", NS)
def test_whole_voxel_translation_shifts_the_map(driver, n):
    """o = t voxels: destination voxel v holds source voxel v + t — t negative and no multiple of subbox_n, block keys crossing zero"""
    rng = np.random.default_rng(20 + n)
    for nb, t in ((1, (1, 0, 0)), (2, (-1, -2, -3)), (65, (n, -n, 2 * n)), (64, (n + 1, -1, -(2 * n + 1))), (257, (-5, 3, 7))):
        blocks = make_blocks(rng, cube_keys(rng, nb), n ** 3)
        T = ref.make_T(None, np.asarray(t, dtype=np.float64) * D_SUB)
        want = ref.warp(blocks, T, n, D_SUB)
        shifted = {(x - t[0], y - t[1], z - t[2]): val for (x, y, z), val in voxel_map(blocks, n).items()}
        same(want, blocks_from_voxels(shifted, n), f"shift {t} n {n} nb {nb}")
        assert want["summary"][4] == nb * n ** 3
        got = driver(blocks, n, T)
        same(got, want, f"driver shift {t} n {n} nb {nb}")
        same_counts(got["summary"], want["summary"])


@pytest.mark.parametrize("n", NS)
def test_quarter_turns_permute_the_voxels(driver, n):
    """90 degrees about each axis: an exact permutation of the voxels; four applications return the input"""
    rng = np.random.default_rng(30 + n)
    turns = {0: [[1, 0, 0], [0, 0, -1], [0, 1, 0]], 1: [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], 2: [[0, -1, 0], [1, 0, 0], [0, 0, 1]]}
    for nb in (1, 2, 65, 257 if n < 8 else 64):
        blocks = make_blocks(rng, cube_keys(rng, nb), n ** 3)
        for axis, R in turns.items():
            R = np.array(R, dtype=np.int64)
            T = ref.make_T(R.astype(np.float64))
            want = ref.warp(blocks, T, n, D_SUB)
            # source voxel of destination voxel v: the voxel of R (v + 1/2), i.e. R v with a negated row one lower
            turned = {}
            Rinv = R.T
            for s, val in voxel_map(blocks, n).items():
                v = Rinv @ (2 * np.array(s, dtype=np.int64) + 1)  # twice the centre, exactly
                turned[tuple(((v - 1) // 2).tolist())] = val
            same(want, blocks_from_voxels(turned, n), f"turn about {axis} n {n} nb {nb}")
            got = driver(blocks, n, T)
            same(got, want, f"driver turn about {axis} n {n} nb {nb}")
            same_counts(got["summary"], want["summary"])
            cur = dict(want, collapsed=np.zeros(len(want["keys"]), np.uint8))
            for _ in range(3):
                cur = ref.warp(cur, T, n, D_SUB)
            same(cur, ref.sorted_blocks(blocks), f"four turns about {axis} n {n} nb {nb}")


@pytest.mark.parametrize("n", NS)
def test_half_voxel_translation_is_decided_by_the_floor(driver, n):
    """centres land exactly on lattice boundaries: floor decides, and the driver agrees with the numpy rule"""
    rng = np.random.default_rng(40 + n)
    d = 0.125  # (a power of two: the centres are exact and so is the half-voxel step)
    for nb, o in ((2, (0.5, 0.0, 0.0)), (65, (0.5, -0.5, 0.5)), (257, (-1.5, 2.5, -0.5))):
        blocks = make_blocks(rng, cube_keys(rng, nb), n ** 3)
        T = ref.make_T(None, np.asarray(o) * d)
        valid, v = ref.source_voxels(T, blocks["keys"], n, d)
        want_v = blocks["keys"].astype(np.int64)[:, None, :] * n + ref.cell_coords(n)[None] + np.floor(np.asarray(o) + 0.5).astype(np.int64)
        assert valid.all() and np.array_equal(v, want_v)  # (v + 1/2 + o is an integer: the voxel it is the lower face of)
        want = ref.warp(blocks, T, n, d)
        got = driver(blocks, n, T, d_sub=d)
        same(got, want, f"half voxel {o} n {n} nb {nb}")
        same_counts(got["summary"], want["summary"])


@pytest.mark.parametrize("n", NS)
def test_seen_and_the_key_box_only_restrict(driver, n):
    rng = np.random.default_rng(50 + n)
    for nb in (1, 63, 257):
        blocks = make_blocks(rng, cube_keys(rng, nb), n ** 3)
        # a few blocks nothing has seen: MLM_WARP_SEEN must not emit what only they reach
        blank = rng.random(nb) < 0.3
        blocks["occ"][blank] = ref.U
        blocks["infl"][blank] = ref.U
        for T in (ref.make_T(), GENERAL):
            full = ref.warp(blocks, T, n, D_SUB)
            seen = ref.warp(blocks, T, n, D_SUB, seen=True)
            fk = {tuple(k): i for i, k in enumerate(full["keys"].tolist())}
            assert all(tuple(k) in fk for k in seen["keys"].tolist()) and len(seen["keys"]) <= len(full["keys"])
            if T is not GENERAL:  # (identity: a block nothing has seen — or a released one whose element 0 is unknown — is not emitted)
                b = ref.sorted_blocks(blocks)
                assert len(seen["keys"]) == int(((b["occ"] != ref.U) | (b["infl"] == ref.O)).any(axis=1).sum()) <= nb - int(blank.sum())
            rows = np.array([fk[tuple(k)] for k in seen["keys"].tolist()], dtype=np.int64)
            live = (full["occ"][rows] != ref.U) | (full["infl"][rows] == ref.O)
            for k in ("log_odds", "occ", "infl"):
                assert np.array_equal(seen[k][live].view(np.uint8), full[k][rows][live].view(np.uint8)), k
            assert not seen["log_odds"][~live].any() and np.all(seen["occ"][~live] == ref.U) and np.all(seen["infl"][~live] == ref.U)
            assert seen["summary"][4] == int(live.sum()) and live.any(axis=1).all()
            got = driver(blocks, n, T, flags=ref.SEEN)
            same(got, seen, f"driver seen n {n} nb {nb}")
            same_counts(got["summary"], seen["summary"])
            # key boxes: a slab, a single key, nothing, beyond the key range
            for lo, dims in (([0, -50, -50], [2, 100, 100]), ([-1, 0, 1], [1, 1, 1]), ([500, 500, 500], [3, 3, 3]),
                             ([ref.I32_MIN, ref.I32_MIN, 0], [ref.I32_MAX, ref.I32_MAX, 1]), ([ref.KEY_MAX + 1, 0, 0], [5, 5, 5])):
                boxed = ref.warp(blocks, T, n, D_SUB, lo, dims)
                k = full["keys"].astype(np.int64)
                inside = ((k >= np.array(lo, dtype=np.int64)) & (k < np.array(lo, dtype=np.int64) + np.array(dims, dtype=np.int64))).all(axis=1)
                same(boxed, {p: full[p][inside] for p in PLANES}, f"box {lo} {dims}")
                got = driver(blocks, n, T, lo, dims)
                same(got, boxed, f"driver box {lo} {dims} n {n} nb {nb}")
                same_counts(got["summary"], boxed["summary"])


@pytest.mark.parametrize("n", NS)
def test_general_rotation_puts_voxels_where_predicted(driver, n):
    """yaw 30, pitch 7, roll -3 degrees and a translation of a few non-integer voxels.  The gather is defined per destination voxel, so
    the prediction runs that way too: every destination voxel of the candidate region whose centre's image — evaluated apart from the
    rule, as a matrix product in extended precision — lies at least 0.01 voxel from every lattice plane holds exactly what the source
    map holds at the voxel of that image (0.0f / 'u' / 'u' where it holds nothing), and is in an emitted block if that is a live voxel.
    (A source voxel no destination centre falls into appears nowhere: nearest-voxel resampling under a rotation is no bijection.)"""
    rng = np.random.default_rng(60 + n)
    for nb in (1, 2, 64, 257):
        blocks = make_blocks(rng, cube_keys(rng, nb), n ** 3)
        want = ref.warp(blocks, GENERAL, n, D_SUB)
        got = driver(blocks, n, GENERAL)
        same(got, want, f"driver general n {n} nb {nb}")
        same_counts(got["summary"], want["summary"])
        src = voxel_map(blocks, n)
        emitted = {tuple(k): i for i, k in enumerate(want["keys"].tolist())}
        cand = ref.candidate_keys(blocks["keys"], GENERAL, n, D_SUB, margin=1)
        R, o = GENERAL[:9].reshape(3, 3).astype(np.longdouble), GENERAL[9:].astype(np.longdouble)
        d = np.longdouble(D_SUB)
        cc = ref.cell_coords(n)
        checked = hits = 0
        for g in cand:
            v = g[None, :] * n + cc
            w = ((v.astype(np.longdouble) + np.longdouble(0.5)) * d) @ R.T + o
            q = w / d
            sure = (np.abs(q - np.rint(q)) >= 0.01).all(axis=1)
            s = np.floor(q).astype(np.int64)
            row = emitted.get(tuple(g.tolist()))
            for c in np.flatnonzero(sure):
                val = src.get(tuple(s[c].tolist()))
                checked += 1
                if val is None:
                    assert row is None or (want["log_odds"][row, c] == 0 and want["occ"][row, c] == ref.U and want["infl"][row, c] == ref.U)
                else:
                    hits += 1
                    assert row is not None, "a block with a live voxel was not emitted"
                    assert (int(want["log_odds"].view(np.uint32)[row, c]), int(want["occ"][row, c]), int(want["infl"][row, c])) == val
        assert set(emitted) <= set(map(tuple, cand.tolist()))
        assert hits > (0.8 * nb * n ** 3 if nb * n ** 3 >= 500 else 0) and checked > hits


def test_keys_beyond_the_range_are_not_emitted(driver):
    """a map at the key bound shifted across it: destination blocks beyond the 21-bit range are not emitted, source blocks beyond it are absent"""
    rng = np.random.default_rng(7)
    n = 4
    keys = np.array([[ref.KEY_MAX, 0, 0], [ref.KEY_MAX - 1, 0, 0], [ref.KEY_MIN, 5, 5], [ref.KEY_MIN + 1, 5, 5], [0, ref.KEY_MAX, ref.KEY_MIN]], dtype=np.int32)
    blocks = make_blocks(rng, keys, n ** 3, released=0.0)
    lost = False
    for t in ((-n, 0, 0), (n, 0, 0), (-1, 0, 0), (0, -2, 3), (2 * n, 2 * n, -2 * n)):
        T = ref.make_T(None, np.asarray(t, dtype=np.float64) * D_SUB)
        want = ref.warp(blocks, T, n, D_SUB)
        shifted = {(x - t[0], y - t[1], z - t[2]): val for (x, y, z), val in voxel_map(blocks, n).items()}
        kept = {v: val for v, val in shifted.items() if all(ref.KEY_MIN <= c // n <= ref.KEY_MAX for c in v)}
        lost = lost or len(kept) < len(shifted)
        same(want, blocks_from_voxels(kept, n), f"shift {t} at the key bound")
        assert ((want["keys"] >= ref.KEY_MIN) & (want["keys"] <= ref.KEY_MAX)).all()
        got = driver(blocks, n, T)
        same(got, want, f"driver shift {t} at the key bound")
        same_counts(got["summary"], want["summary"])
    assert lost


def test_capacity_and_dry(driver):
    rng = np.random.default_rng(3)
    n = 3
    blocks = make_blocks(rng, cube_keys(rng, 65), n ** 3)
    want = ref.warp(blocks, GENERAL, n, D_SUB)
    E = int(want["summary"][2])
    assert E > 65
    for flags, cap, want_out, status, written in ((0, E - 1, True, ref.ERR_CAPACITY, 0), (0, 0, True, ref.ERR_CAPACITY, 0), (ref.DRY, E, True, ref.OK, 0),
                                                  (ref.DRY, 0, False, ref.OK, 0), (0, 0, False, ref.OK, 0), (0, E, True, ref.OK, E)):
        got = driver(blocks, n, GENERAL, flags=flags, cap=cap, want_out=want_out)
        assert got["status"] == status and len(got["keys"]) == written
        exp = want["summary"].copy()
        exp[3] = written
        same_counts(got["summary"], exp)


INVALID = [(dict(T=None), 1),
           (dict(T=ref.make_T(None, (np.nan, 0, 0))), 2), (dict(T=ref.make_T(None, (0, np.inf, 0))), 2), (dict(T=np.full(12, np.nan)), 2),
           (dict(T=ref.make_T(np.eye(3) * (1 + 1e-6))), 3), (dict(T=ref.make_T(np.eye(3) * 2.0)), 3), (dict(T=ref.make_T(np.zeros((3, 3)))), 3),
           (dict(T=ref.make_T([[1, 1e-3, 0], [0, 1, 0], [0, 0, 1]])), 3), (dict(T=ref.make_T(np.eye(3) * 1e200)), 3),
           (dict(key_lo=[0, 0, 0]), 4), (dict(key_dims=[1, 1, 1]), 4),
           (dict(key_lo=[0, 0, 0], key_dims=[1, 0, 1]), 5), (dict(key_lo=[0, 0, 0], key_dims=[1, 1, ref.I32_MIN]), 5),
           (dict(key_lo=[ref.I32_MAX, 0, 0], key_dims=[1, 1, 1]), 6), (dict(key_lo=[0, 2, 0], key_dims=[1, ref.I32_MAX - 1, 1]), 6),
           (dict(flags=8), 7), (dict(flags=-1), 7), (dict(flags=16 | ref.SEEN), 7),
           (dict(cap=-1), 8), (dict(cap=ref.I32_MIN), 8)]
VALID = [dict(), dict(T=GENERAL, flags=7, cap=5), dict(T=ref.make_T(np.eye(3) * (1 + 1e-10))), dict(T=ref.make_T(np.diag([1.0, -1.0, 1.0]))),
         dict(key_lo=[ref.I32_MIN] * 3, key_dims=[ref.I32_MAX] * 3), dict(key_lo=[ref.I32_MAX - 1, 0, 0], key_dims=[1, 1, 1]),
         dict(T=ref.make_T(ref.rot(123.0, -45.0, 200.0), (1e6, -1e6, 3.0)))]


def test_argument_check(driver):
    rng = np.random.default_rng(1)
    blocks = make_blocks(rng, cube_keys(rng, 2), 8)
    for case, code in INVALID + [(c, 0) for c in VALID]:
        a = dict(T=ref.make_T(), key_lo=None, key_dims=None, flags=0, cap=0)
        a.update(case)
        assert ref.check_args(a["T"], a["key_lo"], a["key_dims"], a["flags"], a["cap"]) == code, case
        got = driver(blocks, 2, a["T"], a["key_lo"], a["key_dims"], flags=a["flags"], cap=a["cap"], want_out=False)
        assert got["code"] == code and got["status"] == (ref.ERR_INVALID if code else ref.OK), (case, got["code"])
        if code:
            assert not got["summary"].any() and len(got["keys"]) == 0


def test_binding_names_the_call():
    from mlmapping_amd import mlmap

    assert "mlm_warp_blocks" in mlmap.ABI_SYMBOLS
    assert (mlmap.MLM_WARP_SEEN, mlmap.MLM_WARP_REPLACE, mlmap.MLM_WARP_DRY, mlmap.MLM_WARP_ROW) == (ref.SEEN, ref.REPLACE, ref.DRY, ref.ROW)
    assert hasattr(mlmap.MLMap, "warp_blocks") and hasattr(mlmap.MLMap, "reanchor")
    T = ref.make_T(ref.rot(30.0, 7.0, -3.0), (0.3, -1.2, 2.0))
    Ti = mlmap.invert_T(T)
    assert np.array_equal(Ti, ref.invert(T))
    R, o, Ri, oi = T[:9].reshape(3, 3), T[9:], Ti[:9].reshape(3, 3), Ti[9:]
    assert np.abs(Ri @ R - np.eye(3)).max() < 1e-15 and np.abs(Ri @ o + oi).max() < 1e-15
    header = open(os.path.join(ROOT, "include", "mlmap_hip.h")).read()
    assert "int mlm_warp_blocks(mlm_handle *h, const double T_sd[12], const int32_t key_lo[3], const int32_t key_dims[3]," in header
    assert "mlm_warp_blocks(h_, T_sd, key_lo, key_dims, flags, cap, keys, log_odds, occ, infl, summary)" in open(os.path.join(ROOT, "include", "mlmap_facade.hpp")).read()


def test_facade_member_compiles(tmp_path):
    """include/mlmap_facade.hpp's warpBlocks as a C++ client calls it (tests/cpp/warp_client.cpp)"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "cpp", "warp_client.cpp"),
                           "-o", str(tmp_path / "warp_client.o")])
