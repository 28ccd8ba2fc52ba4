"""k_sector books hit records by centre cell and spreads each centre once (mlm_kernels_sector.h, mlm_sector_book.h): frames built for the
cases of that pass, against the CPU oracle — the map's keys, classes and log-odds bits (tests.util.compare_maps) — and frame_stats'
n_hit_cells, n_multi_cells and n_contrib_slots against the values the library gave for the same inputs before centres were reduced
(PARENT, recorded once).  Every scene goes once as a lone synchronous frame (k_sector's 512-thread form) and once as an asynchronous
batch of 8 frames (the 256-thread form); S1 geometry with the image's size.

  shared_centre    24x16, 3 m everywhere, identity pose: a column's centre cells are fed by several 8x8 tiles (asserted)
  row_step         the same with a step of one dRho between the halves of every row: the two depths lie in different columns, no cell gets
                   two kinds (12 centres, 36 hit cells, as shared_centre)
  shared_targets   24x16 at 4 m, neighbouring pixels one dRho apart (a checkerboard: a step between the halves of a row would put the two
                   depths into different columns): a column's two centres spread into each other, cells get several kinds and need their
                   order (asserted: n_multi_cells) — references from records whose centres were merged
  beyond_kept      64x480 jittered wall: a column of more than 2 * 256 records (asserted), the reference pass re-reads records
  wraps            128x128 at 0.3 m, identity pose: the crowded cells in front of the sensor
  wraps_one_cell, wraps_one_cell_spread
                   128x144 through a lens of 16 000 pixels focal length at 0.3 m and at 4 m: the whole image is ONE centre cell, 2 304 mask
                   rows (asserted from n_groups): the reference count wraps on the centre (0.3 m: no spread) and on every target of its
                   spread (4 m: three hit cells); single-kind cells, so no frame may fall back
  frontier         shared_centre in frontier mode (the first point of a centre: s_p0)
  outer_mixed      shared_targets with every third row beyond the map's radius: columns hold ray-only records next to hit records (asserted)
  scatter_64x48    the 64x48 "scatter" scene of synthetic.stream: 280 records per column, about 260 hit cells — the small table holds them
  table_full       the same scene at 64x192: columns with more hit cells than the small table's 512 entries (asserted) go through the
                   large-table pass; no frame falls back"""
import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests.util import compare_maps

pytestmark = pytest.mark.gpu

IDENT = syn.static_pose()
YAWED = syn.quat_from_rpy(0.0, 0.0, np.radians(10.5)), np.array([0.0, 0.0, 1.5])  # (the middle of azimuth column 10)


def _cfg(w, h, f=None, **kw):
    if f is not None:
        kw.update(cam_fx=f, cam_fy=f)
    return S1.with_(width=w, height=h, cam_cx=w / 2 - 0.5, cam_cy=h / 2 - 0.5, **kw)


def _scene(name):
    """-> (cfg, [8 images], pose)"""
    u16 = lambda a: np.ascontiguousarray(a, dtype=np.uint16)  # noqa: E731
    if name in ("shared_centre", "frontier"):
        cfg = _cfg(24, 16, use_exploration_frontiers=name == "frontier")
        return cfg, [u16(np.full((16, 24), 3000))] * 8, IDENT
    if name == "row_step":
        cfg = _cfg(24, 16)
        img = np.full((16, 24), 3000)
        img[:, 12:] += 100
        return cfg, [u16(img)] * 8, IDENT
    if name in ("shared_targets", "outer_mixed"):
        cfg = _cfg(24, 16)
        yy, xx = np.mgrid[0:16, 0:24]
        img = 4030 + 100 * ((xx + yy) % 2)
        if name == "outer_mixed":
            img[::3, :] = 9000
        return cfg, [u16(img)] * 8, IDENT
    if name == "beyond_kept":
        cfg = _cfg(64, 480)
        base = np.full((480, 64), 3000, dtype=np.uint16)
        return cfg, [syn.jitter_depth(base, k, amp_mm=500) for k in range(8)], IDENT
    if name == "wraps":
        cfg = _cfg(128, 128)
        return cfg, [u16(np.full((128, 128), 300))] * 8, IDENT
    if name in ("wraps_one_cell", "wraps_one_cell_spread"):
        cfg = _cfg(128, 144, f=16000.0)
        return cfg, [u16(np.full((144, 128), 4030 if name.endswith("spread") else 300))] * 8, YAWED
    if name in ("scatter_64x48", "table_full"):
        cfg = _cfg(64, 48 if name == "scatter_64x48" else 192)
        return cfg, [img for img, _ in syn.stream(cfg, "scatter", "static", 8)], IDENT
    raise KeyError(name)


def _records(cfg, cpu, img, pose):
    """hit and ray-only records per azimuth column, and the most 8x8 tiles that feed one centre cell, from the oracle's back-projection
    (float arithmetic of this test: a point next to a cell boundary may land in the neighbour, the counts are asserted with room)"""
    h, w = img.shape
    p = cpu.project_dense(img)
    assert len(p) == w * h  # (every pixel valid)
    t_bs = np.asarray(cfg.T_B_S).reshape(4, 4)
    b = p @ t_bs[:3, :3].T + t_bs[:3, 3]
    qw, _, _, qz = pose[0]
    yaw = 2.0 * np.arctan2(qz, qw)
    rho = np.hypot(b[:, 0], b[:, 1])
    col = np.floor((np.degrees(np.arctan2(b[:, 1], b[:, 0]) + yaw) % 360.0) / cfg.am_d_Phi_deg).astype(np.int64)
    r = np.floor(rho / cfg.am_d_Rho).astype(np.int64)
    z = np.floor(b[:, 2] / cfg.am_d_Z + 0.5).astype(np.int64) + 100
    yy, xx = np.mgrid[0:h, 0:w]
    tile = ((yy // 8) * ((w + 7) // 8) + xx // 8).ravel()
    outer = r >= cfg.am_n_Rho
    rec = np.unique(np.stack([col, np.where(outer, -1, r), z, tile, outer.astype(np.int64)], axis=1), axis=0)
    n_phi = int(round(360 / cfg.am_d_Phi_deg))
    hit_per_col = np.bincount(rec[rec[:, 4] == 0, 0], minlength=n_phi)
    outer_per_col = np.bincount(rec[rec[:, 4] == 1, 0], minlength=n_phi)
    hits = rec[rec[:, 4] == 0]
    _, tiles_per_centre = np.unique(hits[:, :3], axis=0, return_counts=True) if len(hits) else (None, np.zeros(1, dtype=np.int64))
    return hit_per_col, outer_per_col, int(tiles_per_centre.max())


# (n_hit_cells, n_multi_cells, n_contrib_slots) of the last frame, as the library computed them record by record (the parent of the
# centre-wise booking), per scene: lone frame, batch of 8
PARENT = {
    "shared_centre": ((36, 0, 0), (36, 0, 0)),
    "row_step": ((36, 0, 0), (36, 0, 0)),
    "shared_targets": ((48, 20, 640), (48, 20, 640)),
    "beyond_kept": ((3183, 1473, 53600), (3189, 1472, 53520)),
    "wraps": ((14, 0, 0), (14, 0, 0)),
    "wraps_one_cell": ((1, 0, 0), (1, 0, 0)),
    "wraps_one_cell_spread": ((3, 0, 0), (3, 0, 0)),
    "frontier": ((36, 0, 0), (36, 0, 0)),
    "outer_mixed": ((48, 24, 576), (48, 24, 576)),
    "scatter_64x48": ((2623, 1425, 22800), (2633, 1445, 23120)),
    "table_full": ((9778, 5795, 92720), (9801, 5757, 92112)),
}
KEYS = ("n_hit_cells", "n_multi_cells", "n_contrib_slots")


def _check(gpu, cpu, cfg, what):
    compare_maps(gpu.export_blocks(), cpu.export_blocks(), what)
    if cfg.use_exploration_frontiers:
        assert np.array_equal(gpu.export_frontier(), cpu.export_frontier()), what


@pytest.mark.parametrize("name", list(PARENT))
def test_scene(name):
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    cfg, imgs, pose = _scene(name)
    h, w = imgs[0].shape
    got = []
    for mode in ("lone", "batch"):
        gpu, cpu = MLMap(cfg, max_blocks=8192, max_points=w * h, max_batch=8), OracleMap(cfg)
        if mode == "lone":
            gpu.update_map(imgs[0], *pose)
            cpu.update_depth(imgs[0], *pose)
        else:
            gpu.update_map_batch(np.stack(imgs), np.stack([pose[0]] * 8), np.stack([pose[1]] * 8))
            for img in imgs:
                cpu.update_depth(img, *pose)
        _check(gpu, cpu, cfg, f"{name} ({mode})")
        st = gpu.frame_stats()
        got.append(tuple(st[k] for k in KEYS))
        print(f"STATS {name} {mode} {got[-1]} groups {st['n_groups']} rays {st['n_rays']} fallbacks {st['n_sector_fallbacks']}")
        assert st["n_sector_fallbacks"] == 0, (name, mode, st)
        if mode == "lone":
            hit_rec, outer_rec, tiles = _records(cfg, cpu, imgs[0], pose)
            print(f"RECORDS {name} max hit records per column {hit_rec.max()}, most tiles per centre {tiles}, groups {st['n_groups']}")
            if name.startswith(("shared_centre", "frontier")):
                assert tiles >= 3, tiles
            if name == "shared_targets":
                assert st["n_multi_cells"] > 0, st
            if name == "beyond_kept":
                assert hit_rec.max() > 2 * 256 + 64, hit_rec.max()  # (with room for this test's float binning)
            if name.startswith("wraps_one_cell"):
                assert st["n_groups"] == (w // 8) * (h // 8) and (w // 8) * (h // 8) * 8 > 2047, st  # one record per tile, all on one centre: 2 304 rows
            if name == "outer_mixed":
                assert np.any((hit_rec > 0) & (outer_rec > 0)), (hit_rec.max(), outer_rec.max())
                assert st["n_multi_cells"] > 0, st
        if name == "table_full":
            # a column with more hit cells than the small table has entries (S1: 512) overflowed it; no frame fell back (above), so the
            # column went through the large-table pass (or through a table widened after it)
            cc, _ = cpu.hit_cells_sorted()
            per_col = np.bincount((cc // cfg.am_n_Rho) % int(round(360 / cfg.am_d_Phi_deg)))
            print(f"TABLE {name} {mode} most hit cells in a column {per_col.max()}")
            assert per_col.max() > 512, per_col.max()
        gpu.close()
    assert tuple(got) == PARENT[name], (name, got)
