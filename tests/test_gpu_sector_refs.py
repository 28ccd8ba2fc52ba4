"""k_sector's reference pass, ray walk and miss passes (mlm_kernels_sector.h, mlm_sector_refs.h) on frames built for their cases, against
the oracle: hit sets, hit odds (float bits), miss sets and the map's log-odds (float bits), S1 map, record_awareness.  Dense frames of
8x8, 32x8, 40x16 and 64x64 pixels; every scene goes once as a lone synchronous frame (k_sector's 512-thread form, sixteen lanes per ray)
and once inside a batch of six (256 threads, four lanes per ray).

A camera with a focal length of 4 000 pixels sees 0.9 degrees with 64 pixels: the whole image lies in ONE azimuth column (yaw 10.5 degrees:
the middle of column 10) and one z cell, and a pixel's rho cell is its depth's.  So the image's depth pattern alone says which lanes of
an 8x8 pixel tile share a centre cell (one record per such group) and which rows of the tile a group fills:
  rows1 / rows2 / rows8   a group fills one row, two rows, all eight rows of its tile (asserted: frame_stats' n_groups is the count the pattern gives)
  corner                  only the last tile of the image holds points: every cell's first pixel lies outside the first tile column / row
  crowd, crowd_far        36 / 34 cells per tile: a column of more than 256 (40x16) and more than 512 (64x64) records — the second kept record (in the
                          batch: 256 threads), the re-read; ordered cells asserted, in crowd_far at 40x16 every record's own cell is one
  deep_crowd              eight cells per tile beyond 5.5 m: records with more than five targets, eight per tile
  deep                    centre cells at 5.8 and 5.9 m: seven targets per record (MLM_SEC_KEEP_MORE; asserted: more rho cells hit than five targets reach)
  flat / steep / tied     rays with z = zc (every level scene), with |z - zc| >= rho, and with exact half-integer steps (walls seen under a pitch;
                          asserted from the centre cell the scene gives, which the oracle must have hit)
  outer, half_outer       points beyond the map (6.5 m): ray starts only / next to hits
and one frame through the pixel list, one map in frontier mode.  Ordered cells (several kinds, order-dependent) are asserted from
frame_stats' n_multi_cells wherever the pattern makes them.  Reference: src/map_awareness.cpp:135-171, 243-274."""
import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests.util import compare_maps

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (32, 8), (40, 16), (64, 64)]  # (width, height), multiples of eight
YAW = np.radians(10.5)
POSE = syn.quat_from_rpy(0.0, 0.0, YAW), np.array([0.0, 0.0, 1.5])  # level: the cylinder is the sensor's, every point lies in z cell zc = 20


def _pitched(rho_m, dz_m):
    """the pose that looks at the point rho_m out and dz_m above or below the sensor, and that point's depth in millimetres"""
    return (syn.quat_from_rpy(0.0, -np.arctan2(dz_m, rho_m), YAW), np.array([0.0, 0.0, 1.5])), int(round(1000.0 * (np.hypot(rho_m, dz_m) - CAM_X)))


F = 4000.0
CAM_X = S1.T_B_S[3]  # the camera sits 0.12 m in front of the body's origin, on its x axis: range from the cylinder's axis = depth + 0.12
PHI = 10


def _cfg(w, h, **kw):
    return S1.with_(width=w, height=h, cam_cx=w / 2 - 0.5, cam_cy=h / 2 - 0.5, cam_fx=F, cam_fy=F, **kw)


def _scenes(w, h):
    """name -> (image, pose, expectations)"""
    yy, xx = np.mgrid[0:h, 0:w]
    tiles = (w // 8) * (h // 8)
    u16 = lambda a: a.astype(np.uint16)  # noqa: E731
    out = {}
    # (depths of 30 mm + a multiple of 100 mm: with the camera's 0.12 m the middle of a 0.1 m rho cell; 4 030 mm is cell 41)
    out["rows1"] = (u16(4030 + 100 * (yy % 8)), POSE, dict(groups=tiles * 8, multi=True, flat=(41, 0)))
    out["rows2"] = (u16(4030 + 100 * ((yy % 8) // 2)), POSE, dict(groups=tiles * 4, multi=True))
    # (two centre cells with one between them, which gets only their spreads: two weak kinds, ordered however many pixels there are)
    out["rows8"] = (u16(4030 + 200 * ((xx + yy) % 2)), POSE, dict(groups=tiles * 2, multi=True))
    corner = u16(4030 + 100 * (yy % 8))
    corner[(yy < h - 8) | (xx < w - 8)] = 0
    out["corner"] = (corner, POSE, dict(groups=8, multi=True, points=64))
    out["crowd"] = (u16(1030 + 100 * ((xx % 8) + 4 * (yy % 8))), POSE, dict(min_groups=tiles * 36, multi=True))
    # 34 centre cells per tile, rho 30 .. 63, where every centre spreads at least one cell: every cell gets a centre kind and spread kinds, and
    # at 40x16 (340 records, about twenty centre contributions of strength 1 per cell: short of MLM_SEC_STRONG_ENOUGH) EVERY record's own cell
    # needs its order — a wrong or missing reference of a thread's SECOND record (256 threads: the batch) would change that cell's odd
    out["crowd_far"] = (u16(2930 + 100 * ((xx % 8 + 8 * (yy % 8)) % 34)), POSE, dict(min_groups=tiles * 34, multi=True))
    out["deep"] = (u16(5830 + 100 * (yy % 2)), POSE, dict(groups=tiles * 2, multi=True, min_rho_cells=7))
    # eight centre cells per tile beyond 5.5 m, seven targets and more per record
    deep = u16(5630 + 100 * (xx % 8))
    deep[(yy >= 16) | (xx >= 40)] = 0  # (at most ten tiles: a cell with more than 2 047 references that needs its order sends the frame to the cell-table path)
    out["deep_crowd"] = (deep, POSE, dict(min_groups=min(tiles, 10) * 8, multi=True, min_rho_cells=9))
    # a wall seen under a pitch: one centre cell 15 z cells off the sensor's (the middle of the cell: 64 pixels span 27 mm at 3.4 m)
    pose, d = _pitched(1.05, 1.5)
    out["steep"] = (u16(np.full((h, w), d)), pose, dict(steep=(10, 15)))
    pose, d = _pitched(3.05, 1.5)
    out["tied"] = (u16(np.full((h, w), d)), pose, dict(tied=(30, 15)))
    out["outer"] = (u16(np.full((h, w), 9000)), POSE, dict(no_hits=True))
    half = u16(4030 + 100 * (yy % 8))
    half[:, : w // 2] = 9000 + 40 * (xx[:, : w // 2] % 8)
    out["half_outer"] = (half, POSE, dict(multi=True))
    return out


def _cells(cfg, cells):
    n_rho, n_phi = cfg.am_n_Rho, int(360 / cfg.am_d_Phi_deg)
    c = np.asarray(cells, dtype=np.int64)
    return c % n_rho, (c // n_rho) % n_phi, c // (n_rho * n_phi)


def _tied(rho, z, zc):
    """a step k of the ray from (rho, z) whose exact z is a half-integer: 2 k (z - zc) = rho (mod 2 rho)"""
    return any((2 * k * (z - zc)) % (2 * rho) == rho for k in range(1, rho))


def _check_frame(gpu, cpu, what):
    gc, go, _ = gpu.awareness_hits()
    cc, co = cpu.hit_cells_sorted()
    assert np.array_equal(gc, cc), f"{what}: hit cells differ"
    assert np.array_equal(go.view(np.uint32), co.view(np.uint32)), f"{what}: hit odds differ in bits"
    assert np.array_equal(gpu.awareness_misses(), np.sort(cpu.misses()).astype(np.int64)), f"{what}: miss cells differ"
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), what)
    return cc


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_reference_pass_ray_walk_and_miss_passes(w, h):
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    cfg = _cfg(w, h)
    zc = cfg.am_n_Z_below
    scenes = _scenes(w, h)
    seen = set()
    # ---- every scene as a lone synchronous frame
    gpu, cpu = MLMap(cfg, max_blocks=4096, max_points=w * h, record_awareness=True, max_batch=6), OracleMap(cfg)
    for name, (img, pose, exp) in scenes.items():
        what = f"{w}x{h} {name} (lone)"
        gpu.update_map(img, *pose)
        cpu.update_depth(img, *pose)
        cc = _check_frame(gpu, cpu, what)
        st = gpu.frame_stats()
        rho, phi, z = _cells(cfg, cc)
        print(what, {k: st[k] for k in ("n_points", "n_groups", "n_hit_cells", "n_miss_cells", "n_multi_cells", "n_rays")})
        if exp.get("no_hits"):
            assert len(cc) == 0 and len(cpu.misses()) > 0 and st["n_rays"] > 0, (what, st)
            seen.add("outer")
            continue
        # (one column holds the whole frame; under a pitch the image's azimuth span grows by range / rho: past a column's degree from 40 pixels on)
        if name in ("steep", "tied"):  # (... and the spread follows the ray's slope: a few rows around 15 off the sensor's)
            assert np.all(np.abs(phi - PHI) <= 1) and np.all(np.abs(np.abs(z - zc) - 15) <= 2), (what, np.unique(phi), np.unique(z))
        else:
            assert np.all(phi == PHI) and np.all(z == zc), (what, np.unique(phi), np.unique(z))
        if "groups" in exp:
            assert st["n_groups"] == exp["groups"], (what, st["n_groups"], exp["groups"])
        if "min_groups" in exp:
            assert st["n_groups"] >= exp["min_groups"], (what, st["n_groups"], exp["min_groups"])
            seen.update(k for k, n in (("records>256", 256), ("records>512", 512)) if st["n_groups"] > n)
        if "points" in exp:
            assert st["n_points"] == exp["points"], (what, st)
        if exp.get("multi"):
            assert st["n_multi_cells"] > 0, (what, st)
            seen.add({"rows1": "rows=1", "rows2": "rows=2", "rows8": "rows=8", "corner": "first pixel elsewhere", "deep": "targets>5",
                      "half_outer": "outer+hits"}.get(name, name))
        if "min_rho_cells" in exp:
            assert len(np.unique(rho)) >= exp["min_rho_cells"], (what, np.unique(rho))  # (two adjacent centres, five targets each: six)
        for kind in ("flat", "steep", "tied"):
            if kind in exp:
                r0, dz0 = exp[kind]  # (the centre cell the pattern gives: rho, |z - zc|)
                assert np.any((rho == r0) & (np.abs(z - zc) == dz0)), (what, kind, r0, dz0, rho, z)
                assert st["n_rays"] > 0, (what, st)
                ok = {"flat": dz0 == 0, "steep": dz0 >= r0, "tied": _tied(r0, zc + dz0, zc) and _tied(r0, zc - dz0, zc)}[kind]
                assert ok, (what, kind, r0, dz0)
                seen.add(kind)
    # ---- one frame through the pixel list (64 items per "row" of the reference pass)
    img, pose, _ = scenes["rows1"]
    pix = np.random.default_rng(w * 100 + h).permutation(w * h)[: max(48, (w * h * 3) // 4)].astype(np.int32)
    gpu.update_map(img, *pose, pixel_idx=pix)
    cpu.update_depth_indexed(img, pix, *pose)
    _check_frame(gpu, cpu, f"{w}x{h} pixel list")
    st = gpu.frame_stats()
    assert st["n_points"] == len(pix) and st["n_multi_cells"] > 0, st
    assert st["n_sector_fallbacks"] == 0, st
    gpu.close()
    want = {"rows=1", "rows=2", "rows=8", "targets>5", "outer", "outer+hits", "flat", "steep", "tied"}
    tiles = (w // 8) * (h // 8)
    if tiles > 1:
        want.add("first pixel elsewhere")  # (8x8: the image's only tile is its first)
    want |= {k for k, n in (("records>256", 256), ("records>512", 512)) if tiles * 34 > n}  # (40x16: 340 and 360 records, 64x64: 2 176 and 2 304)
    if (w, h) == (40, 16):  # the batch below runs these with 256 threads: second kept records, none re-read
        assert 256 < scenes["crowd_far"][0].size // 64 * 34 <= 512 and 256 < scenes["crowd"][0].size // 64 * 36 <= 512
    assert want <= seen, (w, h, sorted(want - seen))

    # ---- every scene inside a batch of six (the scenes in a different order: the maps differ from the lone run's)
    gpu, cpu = MLMap(cfg, max_blocks=4096, max_points=w * h, record_awareness=True, max_batch=6), OracleMap(cfg)
    names = sorted(scenes)
    names += names[: (-len(names)) % 6]
    for b in range(0, len(names), 6):
        part = [scenes[n] for n in names[b:b + 6]]
        gpu.update_map_batch(np.stack([p[0] for p in part]), np.stack([p[1][0] for p in part]), np.stack([p[1][1] for p in part]))
        for img, pose, _ in part:
            cpu.update_depth(img, *pose)
        _check_frame(gpu, cpu, f"{w}x{h} batch {names[b:b + 6]}")
    assert gpu.frame_stats()["n_sector_fallbacks"] == 0
    gpu.close()


def test_frontier_mode_frames():
    """frontier mode keeps a time per miss cell (the per-cell walk) and per-axis voxel tables: lone frames and a batch of six, 40x16"""
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    w, h = 40, 16
    cfg = _cfg(w, h, use_exploration_frontiers=True)
    scenes = _scenes(w, h)
    order = ["rows1", "tied", "crowd", "deep", "steep", "half_outer"]
    gpu, cpu = MLMap(cfg, max_blocks=4096, max_points=w * h, max_batch=6), OracleMap(cfg)
    for name in order:
        img, pose, _ = scenes[name]
        gpu.update_map(img, *pose)
        cpu.update_depth(img, *pose)
        compare_maps(gpu.export_blocks(), cpu.export_blocks(), f"frontier {name} (lone)")
        assert np.array_equal(gpu.export_frontier(), cpu.export_frontier()), name
    part = [scenes[n] for n in order]
    gpu.update_map_batch(np.stack([p[0] for p in part]), np.stack([p[1][0] for p in part]), np.stack([p[1][1] for p in part]))
    for img, pose, _ in part:
        cpu.update_depth(img, *pose)
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), "frontier batch")
    assert np.array_equal(gpu.export_frontier(), cpu.export_frontier())
    assert gpu.frame_stats()["n_sector_fallbacks"] == 0
    gpu.close()
