"""The accounting of mlm_query_views on the host (mlmapping_amd/csrc/mlm_views.h: bounding box, clipping, bit index, the rule for a
newly seen voxel and the plan, over the walk of mlm_raywalk.h — the code the kernels run too), built for the CPU with
-fsanitize=address,undefined and held to plain Python sets over the Python walk (tests/view_ref.py) on the oracle's block dump of a
room map: every table word and every mark byte, for every flag set, with and without a box, with exclude, on the LDS classes and on
the global path.  A build of the same driver that skips the de-duplication must fail the comparison."""
import os
import struct
import subprocess

import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests import raywalk_ref as rw
from tests import view_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BITS = (64 * 1024 - 64) * 8  # kViewLdsBits
GLOBAL, REFUSED = 5, -1


def compile_driver(out, *defines):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                           "-Wall", "-Werror", *defines, "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "view_driver.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return compile_driver(tmp_path_factory.mktemp("views") / "view_driver")


def run_driver(exe, tmp, cfg, b, p0, p1, vb, flags, box=None, exclude=None, mark=None, lds_bits=LDS_BITS):
    lo, dims = (box if box is not None else ([0, 0, 0], [0, 0, 0]))
    blob = struct.pack("<dq8i6i", cfg.subbox_d_xyz, lds_bits, cfg.subbox_n, b["keys"].shape[0], p0.shape[0], len(vb) - 1, flags, box is not None,
                       exclude is not None, mark is not None, *[int(x) for x in lo], *[int(x) for x in dims])
    blob += b["keys"].astype(np.int32).tobytes() + b["collapsed"].astype(np.uint8).tobytes()
    blob += b["occ"].astype(np.uint8).tobytes() + b["infl"].astype(np.uint8).tobytes()
    blob += np.ascontiguousarray(p0, dtype=np.float64).tobytes() + np.ascontiguousarray(p1, dtype=np.float64).tobytes()
    blob += np.asarray(vb, dtype=np.int32).tobytes()
    for arr in (exclude, mark):
        if arr is not None:
            blob += np.ascontiguousarray(arr, dtype=np.uint8).tobytes()
    (tmp / "views.bin").write_bytes(blob)
    subprocess.run([exe, str(tmp / "views.bin"), str(tmp / "views.out")], check=True)
    raw = (tmp / "views.out").read_bytes()
    nv = len(vb) - 1
    table = np.frombuffer(raw, dtype=np.int64, count=nv * 8).reshape(nv, 8).copy()
    cls = np.frombuffer(raw, dtype=np.int32, count=nv, offset=nv * 64).copy()
    mk = None
    if mark is not None:
        mk = np.frombuffer(raw, dtype=np.uint8, offset=nv * 68).reshape(np.shape(mark)).copy()
    return table, cls, mk


@pytest.fixture(scope="module")
def scene():
    """the room map, its views — six 64 x 48 fans of 4 m, four 16 x 16 fans of 8 m, an empty view, invalid rays only, the two
    32 768-voxel rays, ties and grazed corners, a refused view, an empty view — and their paths walked once"""
    from oracle.binding import OracleMap

    cfg = S1
    cpu = OracleMap(cfg)
    poses = []
    for img, (q, t) in syn.stream(cfg, "room_jitter", "smooth", 4):
        cpu.update_depth(img, q, t)
        poses.append(t)
    cpu.inflate_map(poses[-1])
    b = cpu.export_blocks()
    d, n = cfg.subbox_d_xyz, cfg.subbox_n
    rng = np.random.default_rng(17)
    big = vr.random_fans(rng, b, cfg, 6, 64, 48, 4.0)
    small = vr.random_fans(rng, b, cfg, 4, 16, 16, 8.0)
    lo_w, hi_w = b["keys"].min(0) * d * n - 0.5, (b["keys"].max(0) + 1) * d * n + 0.5
    w0, w1 = rw.weird_rays(d)
    bad = np.array([rw.valid(a, e, d) is None for a, e in zip(w0, w1)])
    assert bad.sum() >= 8 and (~bad).sum() == 2
    s0, s1 = rw.special_rays(rng, lo_w, hi_w, d, count=40)
    c = lambda *v: [(x + 0.5) * d for x in v]
    far0 = np.array([c(0, 0, 0), c(2000, 2000, 2000)])  # two short rays 2 000 voxels apart on every axis: a box of 8e9 voxels
    far1 = np.array([c(3, 1, 0), c(2002, 2001, 2000)])
    groups = [(big[0][i * 3072:(i + 1) * 3072], big[1][i * 3072:(i + 1) * 3072]) for i in range(6)]
    groups += [(small[0][i * 256:(i + 1) * 256], small[1][i * 256:(i + 1) * 256]) for i in range(4)]
    groups += [(w0[:0], w1[:0]), (w0[bad], w1[bad]), (w0[~bad], w1[~bad]), (s0, s1), (far0, far1), (w0[:0], w1[:0])]
    p0, p1 = np.concatenate([g[0] for g in groups]), np.concatenate([g[1] for g in groups])
    vb = np.concatenate([[0], np.cumsum([len(g[0]) for g in groups])]).astype(np.int32)
    walked = vr.walk(p0, p1, vb, d, rw.block_classes(b, n))
    full = (b["occ"] == ord("o")).any(axis=1)
    mid = (np.median(b["keys"][full], axis=0) * n).astype(int)
    box = ([int(mid[0]) - 12, int(mid[1]) - 14, int(mid[2]) - 6], [31, 29, 17])  # smaller than the fans
    return {"cfg": cfg, "b": b, "p0": p0, "p1": p1, "vb": vb, "walked": walked, "box": box}


def test_reference_is_not_vacuous(scene):
    t, _ = vr.account(scene["walked"][:6], rw.OCC)
    vr.non_vacuous(t)
    full, _ = vr.account(scene["walked"], rw.OCC)
    assert full[10].tolist() == [0] * 8 and full[15].tolist() == [0] * 8                      # the empty views
    assert full[11, 5] == scene["vb"][12] - scene["vb"][11] and full[11, [0, 3, 4, 6]].sum() == 0  # invalid rays only
    assert full[12, 6] >= 32768 and full[12, 0] + full[12, 3] >= 32768                          # the longest valid rays
    assert full[14].tolist() == [0, 0, 0, 0, 0, 0, 0, 1]                                        # refused
    # with exclude set from a winner's mark, some other view's gain drops but stays positive
    lo, dims = scene["box"]
    boxed, _ = vr.account(scene["walked"][:6], rw.OCC, box=scene["box"])
    win = int(np.argmax(boxed[:, 1]))
    _, mark = vr.account(scene["walked"][win:win + 1], rw.OCC, box=scene["box"], mark=np.zeros(dims[::-1], np.uint8))
    again, _ = vr.account(scene["walked"][:6], rw.OCC, box=scene["box"], exclude=mark)
    assert again[win, 1] == 0 and ((again[:, 1] < boxed[:, 1]) & (again[:, 1] > 0)).any(), (boxed[:, 1].tolist(), again[:, 1].tolist())


@pytest.mark.parametrize("flags", rw.FLAG_SETS)
def test_driver_equals_the_sets(exe, tmp_path, scene, flags):
    s = scene
    lo, dims = s["box"]
    shape = dims[::-1]
    rng = np.random.default_rng(flags)
    exclude = (rng.random(shape) < 0.3).astype(np.uint8) * rng.integers(1, 256, size=shape).astype(np.uint8)
    mark0 = rng.choice(np.array([0, 0, 1, 2, 4, 8, 128], dtype=np.uint8), size=shape)
    variants = [("no box", None, None, None), ("box", s["box"], None, None), ("box, mark", s["box"], None, mark0),
                ("box, exclude", s["box"], exclude, None), ("box, exclude, mark", s["box"], exclude, mark0)]
    for what, box, ex, mk in variants:
        exp_t, exp_m = vr.account(s["walked"], flags, box=box, exclude=ex, mark=None if mk is None else mk.copy())
        for lds_bits in (LDS_BITS, 0, 3000):
            t, cls, m = run_driver(exe, tmp_path, s["cfg"], s["b"], s["p0"], s["p1"], s["vb"], flags, box, ex, mk, lds_bits)
            vr.assert_equal(t, exp_t, m, exp_m, f"flags={flags} {what} lds_bits={lds_bits}")
            assert cls[14] == REFUSED or box is not None
            if lds_bits == 0 and box is None:  # everything with a bit to set is on the global path
                assert set(cls[:10].tolist()) == {GLOBAL}
            elif lds_bits == LDS_BITS and box is None:
                assert set(cls[:6].tolist()) <= {0, 1, 2, 3, 4} and GLOBAL in cls[6:10].tolist(), cls.tolist()
    if flags == rw.OCC:
        assert (exp_m != mark0).any() and ((exp_m & 1) != 0).any() and ((exp_m & 2) != 0).any()


def test_a_build_without_dedup_fails(tmp_path, scene):
    """MLM_VIEWS_NO_DEDUP counts every visit (what summing per-ray counts gives): the comparison that the real build passes fails"""
    s = scene
    exe = compile_driver(tmp_path / "view_driver_nodedup", "-DMLM_VIEWS_NO_DEDUP")
    t, _, _ = run_driver(exe, tmp_path, s["cfg"], s["b"], s["p0"], s["p1"], s["vb"], rw.OCC)
    exp, _ = vr.account(s["walked"], rw.OCC)
    assert np.array_equal(t[:, 4:], exp[:, 4:])                      # the per-ray words do not depend on the sets
    assert np.array_equal(t[:10, 0], exp[:10, 6]) and np.array_equal(t[:10, 3], exp[:10, 4])  # every visit counted
    assert (t[:10, 0] > exp[:10, 0]).all()
    with pytest.raises(AssertionError):
        vr.assert_equal(t, exp)


def test_fan_helpers():
    """pinhole_fan / fan_views (conveniences of the Python layer) build the fans of view_ref's generator"""
    from mlmapping_amd.mlmap import fan_views, pinhole_fan

    w, h, hf, vf = 16, 12, np.deg2rad(90.0), np.deg2rad(70.0)
    f = pinhole_fan(w, h, 0.5 * w / np.tan(0.5 * hf), 0.5 * h / np.tan(0.5 * vf), 0.5 * w, 0.5 * h, 4.0)
    ref = vr.fan(w, h, hf, vf, 4.0)
    assert f.shape == (w * h, 3) and np.allclose(f, ref, rtol=0, atol=1e-12) and np.allclose(np.linalg.norm(f, axis=1), 4.0)
    org = np.array([[0.5, -1.0, 1.0], [2.0, 0.0, 0.7]])
    R = np.stack([vr.rotation(0.3, 0.1), vr.rotation(-2.0, -0.4)])
    assert np.allclose(R[0] @ R[0].T, np.eye(3)) and np.isclose(np.linalg.det(R[0]), 1.0)
    p0, p1, vb = fan_views(org, R, f)
    assert vb.tolist() == [0, w * h, 2 * w * h] and vb.dtype == np.int32
    assert np.array_equal(p0[:w * h], np.repeat(org[:1], w * h, axis=0))
    assert np.allclose(p1[w * h:], org[1] + ref @ R[1].T, rtol=0, atol=1e-12)
