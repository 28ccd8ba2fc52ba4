"""Query answers and the dense window read-out pinned to the CPU oracle BIT FOR BIT on crafted maps, imported into both
(mlm_import_blocks / mlo_import_blocks): log-odds distinct per voxel across [lo_min, lo_max] with both clamps and 0; plateaus of
log-odds a few float ulps apart, whose float odds tie or lie one ulp apart (getOddGrad's walk compares float odds with `<`, ties keep
the first direction: include/mlmap.h:237-295); random o/f/u classes; absent neighbours on every face, negative keys and keys at both
ends of the packed key range; released blocks in frontier mode.  Positions: voxel centres, voxel and block faces and 1, 2 ulps either
side (where the multiply-based quotient of mlm_voxel_of must hand over to the division), the id-0 quirk coordinates of get_subbox_id,
NaN, +-Inf, beyond the key range.  Every answer on both paths — the kernels (knob mirror = 0) and the host mirror — equals the
oracle's.  And the device's logit_inv (mlm_logit_inv) equals the host's on every hard case of tests/cpp/logit_inv_scan.cpp and on
dense samples of the whole log-odds range."""
import numpy as np
import pytest

from mlmapping_amd.config import S1
from tests.test_gpu_holes import quirk_coordinates
from tests.test_gpu_window import window_voxels
from tests.util import assert_same_bits, float_range, logit_inv_scan, voxel_centres

pytestmark = pytest.mark.gpu

KEY_LO, KEY_HI = -(1 << 20), (1 << 20) - 1  # block keys of the packed 21-bit key per axis (mlm_device.h: mlm_pack_key)
CLASSES = np.frombuffer(b"ofu", dtype=np.uint8)

CONFIGS = {
    "n10-d0.1": S1,
    "n10-d0.2": S1.with_(subbox_d_xyz=0.2),
    "n5-d0.05": S1.with_(subbox_n=5, subbox_d_xyz=0.05),
    "frontier-n5-d0.1": S1.with_(use_exploration_frontiers=True, subbox_n=5),
    "frontier-n10-d0.2": S1.with_(use_exploration_frontiers=True, subbox_d_xyz=0.2),
}


def _handles(cfg, max_blocks):
    """(kernel-path handle: knob mirror = 0; host-mirror handle: every batch on the host once the mirror is up to date)"""
    from mlmapping_amd import mlmap

    mlmap.debug_set("mirror", 0)
    ker = mlmap.MLMap(cfg, max_blocks=max_blocks)
    mlmap.debug_reset()
    mlmap.debug_set("mirror_max", 1 << 30)
    mir = mlmap.MLMap(cfg, max_blocks=max_blocks)
    mlmap.debug_reset()
    return ker, mir


def _ulps(base, k):
    """float32 base moved k ulps up (k < 0: down), never across 0"""
    b = np.int64(np.float32(base).view(np.int32))
    return (b + (k if base > 0 else -k)).astype(np.int32).view(np.float32)


def _quirk_near_origin(cfg):
    """(the id-0 quirk coordinate nearest to 0, all quirk coordinates within 40 m)"""
    qc = quirk_coordinates(cfg.subbox_d_xyz, cfg.subbox_n, lim=40.0)
    return float(qc[np.argmin(np.abs(qc))]), qc


def craft(cfg, seed):
    rng = np.random.default_rng(seed)
    C = cfg.cells_per_block
    lo_min, lo_max = np.float32(cfg.lm_log_odds_min), np.float32(cfg.lm_log_odds_max)
    box = np.stack(np.meshgrid(np.arange(-2, 2), np.arange(-2, 2), np.arange(-1, 2), indexing="ij"), -1).reshape(-1, 3)
    box = box[rng.random(box.shape[0]) < 0.7]  # holes: absent neighbours on every face
    ends = np.array([[KEY_HI, KEY_HI - 1, 0], [KEY_HI - 1, KEY_HI - 1, 0], [KEY_LO, KEY_LO, KEY_LO], [KEY_LO + 1, KEY_LO, KEY_LO],
                     [2, KEY_LO, KEY_HI]])
    kq = int(np.floor(_quirk_near_origin(cfg)[0] / (cfg.subbox_d_xyz * cfg.subbox_n)))
    quirk = np.stack(np.meshgrid(*[[kq - 1, kq]] * 3, indexing="ij"), -1).reshape(-1, 3)  # blocks around id-0 quirk coordinates
    keys = np.unique(np.concatenate([box, quirk, ends]), axis=0).astype(np.int32)
    nb = keys.shape[0]
    lo = rng.uniform(lo_min, lo_max, size=(nb, C)).astype(np.float32)
    flat = lo.reshape(-1)
    pick = rng.permutation(flat.size)[: 3 * (flat.size // 40)].reshape(3, -1)
    flat[pick[0]], flat[pick[1]], flat[pick[2]] = lo_min, lo_max, 0.0
    bases = [lo_max, np.float32(3.0), np.float32(2.5), np.float32(1.7), np.float32(-1.0), lo_min]
    for b in range(0, nb, 3):  # plateaus: odds that tie (high L) or lie an ulp apart
        base = bases[b // 3 % len(bases)]
        lo[b] = _ulps(base, rng.integers(0 if base == lo_min else -24, 1 if base == lo_max else 25, size=C))
    col = np.zeros(nb, dtype=np.uint8)
    if cfg.use_exploration_frontiers:
        col[rng.random(nb) < 0.3] = 1
    return {"keys": keys, "log_odds": lo, "occ": rng.choice(CLASSES, size=(nb, C)), "infl": rng.choice(CLASSES, size=(nb, C)),
            "collapsed": col}


def positions(cfg, keys, seed):
    rng = np.random.default_rng(seed)
    n, d = cfg.subbox_n, cfg.subbox_d_xyz
    dg = d * n
    held = voxel_centres({"keys": keys}, cfg)
    nbr = np.concatenate([keys + s for s in np.concatenate([np.eye(3, dtype=np.int32), -np.eye(3, dtype=np.int32)])])
    around = voxel_centres({"keys": nbr}, cfg, 6000, seed=seed)
    base = held[rng.integers(0, held.shape[0], 8000)]
    face = base.copy()  # voxel faces k*d (a quarter of them block faces) and 1, 2 ulps either side, on one to three axes
    for a in range(3):
        on = np.flatnonzero(rng.random(face.shape[0]) < 0.6)
        k = np.floor(base[on, a] / d) + rng.integers(0, 2, on.size)
        k[::4] = np.round(base[on[::4], a] / dg) * n
        x, step = k * d, rng.integers(-2, 3, on.size)
        for s in (1, 2):
            x[step >= s] = np.nextafter(x[step >= s], np.inf)
            x[step <= -s] = np.nextafter(x[step <= -s], -np.inf)
        face[on, a] = x
    x0, qc = _quirk_near_origin(cfg)  # coordinates where the two divisions of get_global_idx / get_subbox_id disagree: cell id 0
    kq = int(np.floor(x0 / dg))
    qb = np.stack(np.meshgrid(*[[kq - 1, kq]] * 3, indexing="ij"), -1).reshape(-1, 3)
    quirk = voxel_centres({"keys": qb}, cfg, 2000, seed=seed)
    qc = qc[np.abs(qc - x0) <= dg]
    for a in range(3):
        sel = rng.random(quirk.shape[0]) < 0.5
        quirk[sel, a] = rng.choice(qc, sel.sum())
    kf = np.concatenate([np.round(10.0 ** rng.uniform(3, 8, 300)), 1e9 / n + rng.integers(-3, 4, 100), 1e9 + rng.integers(-3, 4, 100)])
    far = rng.uniform(-1, 1, size=(kf.size, 3)) * dg  # |k| up to 1e8 voxels and around mlm_quot's 1e9 cut-off
    far[:, 0] = np.nextafter(rng.choice([-1, 1], kf.size) * kf * d, rng.choice([-np.inf, np.inf], kf.size))
    weird = np.array([[np.nan, 0.05, 0.05], [0.05, np.nan, 0.05], [np.inf, 0.05, 0.05], [-np.inf, -0.05, 0.05], [0.05, 0.05, np.inf],
                      [1e300, -1e300, 0.05], [(KEY_HI + 1) * dg + d / 2, 0.05, 0.05], [(KEY_LO - 1) * dg + d / 2, 0.05, 0.05],
                      [KEY_HI * dg + d / 2, (KEY_HI - 1) * dg + d / 2, d / 2], [2.2e9 * d, 0.05, 0.05], [0.05, -2.2e9 * d, 0.05]])
    return np.concatenate([held, around, face, quirk, far, weird])


def _kinds(d):
    kinds = [("getOccupancy", lambda m, p: m.getOccupancy(p)), ("getInflateOccupancy", lambda m, p: m.getInflateOccupancy(p)),
             ("getOdd", lambda m, p: m.getOdd(p))]
    kinds += [(f"getOccupancy(inflate={f:.3g})", (lambda f: lambda m, p: m.getOccupancy(p, inflate=f))(f)) for f in (0.0, d / 2, d, 0.15, 1.0, -0.15)]
    kinds += [(f"getOddGrad({it})", (lambda it: lambda m, p: m.getOddGrad(p, it))(it)) for it in (0, 1, 2, 5, 9)]
    return kinds


@pytest.fixture(scope="module", params=list(CONFIGS))
def crafted(request):
    from oracle.binding import OracleMap

    cfg = CONFIGS[request.param]
    b = craft(cfg, seed=len(request.param))
    ker, mir = _handles(cfg, 256)
    cpu = OracleMap(cfg)
    for m in (ker, mir, cpu):
        m.import_blocks(b["keys"], b["log_odds"], b["occ"], b["infl"], b["collapsed"])
    yield request.param, cfg, b, ker, mir, cpu
    ker.close()
    mir.close()


def test_crafted_map_has_ties_and_one_ulp_steps(crafted):
    """the plateaus do hold x-neighbours with different log-odds and equal float odds, and ones an ulp apart (else the walk's
    comparison is not tested)"""
    name, cfg, b, ker, mir, cpu = crafted
    n, C = cfg.subbox_n, cfg.cells_per_block
    keys = np.repeat(b["keys"], C, axis=0)
    cid = np.tile(np.arange(C, dtype=np.int32), b["keys"].shape[0])
    odd = cpu.getOddAt(keys, cid).reshape(-1, n)  # rows of n voxels along x (released blocks answer element 0: equal odds)
    lo = b["log_odds"].reshape(-1, n)
    live = np.repeat(b["collapsed"] == 0, C // n)
    diff_lo = (lo[:, 1:] != lo[:, :-1]) & live[:, None]
    du = np.abs(odd[:, 1:].view(np.int32).astype(np.int64) - odd[:, :-1].view(np.int32))
    assert (diff_lo & (du == 0)).sum() > 50 and (diff_lo & (du == 1)).sum() > 50
    assert (b["log_odds"] == np.float32(cfg.lm_log_odds_min)).any() and (b["log_odds"] == np.float32(cfg.lm_log_odds_max)).any()


def test_every_query_kind_on_both_paths(crafted):
    """every query kind at every position: the kernels' answers and the host mirror's (in one batch and one position per call) are
    the oracle's, bit for bit"""
    name, cfg, b, ker, mir, cpu = crafted
    pos = positions(cfg, b["keys"], seed=3)
    mir.getOdd(pos[:1])  # (the first query after the import refreshes the mirror; every later batch is answered on the host)
    h0, k0 = mir.frame_stats()["n_host_queries"], ker.frame_stats()["n_host_queries"]
    n_host = 0
    for what, fn in _kinds(cfg.subbox_d_xyz):
        want = fn(cpu, pos)
        assert_same_bits(fn(ker, pos), want, f"{name}: {what}, kernels")
        assert_same_bits(fn(mir, pos), want, f"{name}: {what}, host mirror")
        sel = np.random.default_rng(len(what)).choice(pos.shape[0], 60, replace=False)
        one = np.concatenate([fn(mir, pos[i:i + 1]) for i in sel])
        assert_same_bits(one, want[sel], f"{name}: {what}, host mirror one position per call")
        n_host += pos.shape[0] + sel.size
    assert mir.frame_stats()["n_host_queries"] - h0 == n_host, "the mirror handle should have answered everything on the host"
    assert ker.frame_stats()["n_host_queries"] == k0 == 0


def test_odds_at_on_both_paths(crafted):
    """getOdd(glb_id, subbox_id) at every voxel of the map, of its absent neighbours, and at keys beyond the packed key range"""
    name, cfg, b, ker, mir, cpu = crafted
    C = cfg.cells_per_block
    rng = np.random.default_rng(5)
    keys = np.concatenate([b["keys"], b["keys"] + [1, 0, 0], b["keys"] - [0, 0, 1]])
    glb = np.repeat(keys, C, axis=0)
    cid = np.tile(np.arange(C, dtype=np.int32), keys.shape[0])
    odd = np.array([[KEY_HI + 1, 0, 0], [KEY_LO - 1, 0, 0], [0, 1 << 21, 0], [0, 0, -(1 << 21)], [2 ** 31 - 1, 0, 0], [-2 ** 31, -2 ** 31, -2 ** 31],
                    [KEY_HI + (1 << 21), KEY_HI - 1, 0]], dtype=np.int64)
    glb = np.concatenate([glb, odd]).astype(np.int32)
    cid = np.concatenate([cid, rng.integers(0, C, odd.shape[0]).astype(np.int32)])
    want = cpu.getOddAt(glb, cid)
    mir.getOddAt(glb[:1], cid[:1])
    assert_same_bits(ker.getOddAt(glb, cid), want, f"{name}: getOddAt, kernels")
    assert_same_bits(mir.getOddAt(glb, cid), want, f"{name}: getOddAt, host mirror")
    sel = rng.choice(glb.shape[0], 200, replace=False)
    one = np.concatenate([mir.getOddAt(glb[i:i + 1], cid[i:i + 1]) for i in sel])
    assert_same_bits(one, want[sel], f"{name}: getOddAt one by one")


@pytest.mark.parametrize("max_iter", [5, 9])
def test_window_every_channel(crafted, max_iter):
    """export_window in every channel, into host and into device memory, over windows that straddle absent (and released) blocks
    around the origin and at the end of the key range: the oracle's answers at every voxel"""
    import torch

    name, cfg, b, ker, mir, cpu = crafted
    n = cfg.subbox_n
    for lo, dims in (([-3 * n + 1, -3 * n + 2, -2 * n + 3], [5 * n + 1, 5 * n - 3, 4 * n]),
                     ([(KEY_HI - 2) * n + 3, (KEY_HI - 2) * n - 2, -n + 1], [2 * n + 2, 3 * n + 1, 2 * n])):
        w = ker.export_window(lo, dims, odds=True, occ=True, infl=True, grad=True, max_iter=max_iter)
        keys, cid, cen = window_voxels(cfg, lo, dims)
        assert_same_bits(w["odds"].reshape(-1), cpu.getOddAt(keys, cid), f"{name}: window odds")
        assert_same_bits(w["occ"].reshape(-1).astype(np.int32), cpu.getOccupancy(cen), f"{name}: window occ")
        assert_same_bits(w["infl"].reshape(-1).astype(np.int32), cpu.getInflateOccupancy(cen), f"{name}: window infl")
        assert_same_bits(w["grad"].reshape(-1, 3), cpu.getOddGrad(cen, max_iter), f"{name}: window grad")
        shape = (dims[2], dims[1], dims[0])
        dev = {"odds": torch.full(shape, 7.0, dtype=torch.float32, device="cuda"), "occ": torch.full(shape, 7, dtype=torch.int8, device="cuda"),
               "infl": torch.full(shape, 7, dtype=torch.int8, device="cuda"), "grad": torch.full(shape + (3,), 7.0, dtype=torch.float64, device="cuda")}
        torch.cuda.synchronize()
        mir.export_window_dev(lo, dims, max_iter, **{k: v.data_ptr() for k, v in dev.items()})
        for k, v in dev.items():
            assert np.array_equal(v.cpu().numpy().view(np.uint8), w[k].view(np.uint8)), f"{name}: device-memory window {k}"


def test_device_logit_inv_equals_the_host(tmp_path_factory):
    """mlm_logit_inv on the device against glibc on the host: every hard case of the scan over [-2, 4.2] (the only floats where a
    device pow within 256 ulps could round to another odd), every float within 2^16 ulps of -2, 0 and 4.2, and every 256th float of
    the range — through the window's odds (device memory), getOddAt on the kernels and getOddAt on the host mirror"""
    import torch
    from oracle.binding import OracleMap

    cfg = S1
    s = logit_inv_scan(tmp_path_factory.mktemp("scan"), float(cfg.lm_log_odds_min), float(cfg.lm_log_odds_max))
    lo_min, lo_max = np.float32(cfg.lm_log_odds_min), np.float32(cfg.lm_log_odds_max)
    w16 = np.arange(-(1 << 16), (1 << 16) + 1)
    tiny = float(np.uint32(1 << 16).view(np.float32))  # 2^16 floats above 0
    near = [_ulps(lo_min, w16), float_range(-tiny, tiny), _ulps(lo_max, w16)]
    L = np.unique(np.concatenate([s["L"], *near, float_range(lo_min, lo_max, 256)]))
    L = L[(L >= lo_min) & (L <= lo_max)]
    C, side = cfg.cells_per_block, cfg.subbox_n
    nb = -(-L.size // C)
    g = int(np.ceil(np.sqrt(nb)))
    keys = np.stack([np.arange(nb) % g, np.arange(nb) // g, np.zeros(nb, dtype=np.int64)], axis=1).astype(np.int32)
    lo = np.zeros(nb * C, dtype=np.float32)
    lo[:L.size] = L
    lo = lo.reshape(nb, C)
    ker, mir = _handles(cfg, nb + 64)
    cpu = OracleMap(cfg)
    for m in (ker, mir, cpu):
        m.import_blocks(keys, lo)
    idx = np.arange(L.size)
    glb, cid = keys[idx // C], (idx % C).astype(np.int32)
    want = cpu.getOddAt(glb, cid)
    hard = np.searchsorted(L, s["L"])
    assert np.array_equal(want[hard].view(np.uint32), s["f"].view(np.uint32))
    mir.getOddAt(glb[:1], cid[:1])
    found = {}
    found["getOddAt, kernels"] = ker.getOddAt(glb, cid)
    found["getOddAt, host mirror"] = mir.getOddAt(glb, cid)
    dims = [g * side, -(-nb // g) * side, side]
    dev = torch.empty((dims[2], dims[1], dims[0]), dtype=torch.float32, device="cuda")
    ker.export_window_dev([0, 0, 0], dims, 0, odds=dev.data_ptr())
    wk, wc, _ = window_voxels(cfg, [0, 0, 0], dims)
    w = dev.cpu().numpy().reshape(-1)
    flat = (wk[:, 1] * g + wk[:, 0]).astype(np.int64) * C + wc  # (block, cell) of each window voxel -> index into L
    ok = (wk[:, 1] * g + wk[:, 0] < nb) & (flat < L.size)
    order = np.empty(L.size, dtype=np.int64)
    order[flat[ok]] = np.flatnonzero(ok)
    found["window odds, device memory"] = w[order]
    report = {k: int((v.view(np.uint32) != want.view(np.uint32)).sum()) for k, v in found.items()}
    report.update({k + " at hard cases": int((v[hard].view(np.uint32) != want[hard].view(np.uint32)).sum()) for k, v in found.items()})
    print(f"{L.size} log-odds, {s['L'].size} hard cases: mismatches {report}")
    assert not any(report.values()), report
    ker.close()
    mir.close()
