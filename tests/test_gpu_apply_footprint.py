"""k_apply_tiles' footprint: its voxel state in LDS (log-odds f32 + class u8, 0 = not fetched; the pool address of a voxel is
recomputed at write-back from a per-block table and the tile's integer coordinates, as k_tile composes it) and its 64-VGPR cap.

* The LDS layout (mlm_apply_lds, mlmapping_amd/csrc/mlm_host.h) built for the CPU: regions in order and apart, the block
  table large enough for every grid offset, 5 bytes per voxel plus the tables, and the shipped configurations inside the
  150 KB envelope mlm_create checks.
* Batched 64-frame streams of configs 2 and 3 whose poses spread over several grid heights in z (launch_apply_tiles cuts
  such a batch into several launches, and the launches that remain span up to two grid heights of layers), from a pool
  that has to grow (the frame that finds it full is replayed): the exported map must be bit-equal to the oracle's.  A
  write-back address that differed from the one k_tile put in the records would move voxels and fail here.
"""
import math
import os
import subprocess

import numpy as np
import pytest

from mlmapping_amd.config import S1, S3, SDEF, CONFIG2_YAML
from tests.util import compare_maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("al") / "apply_lds_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "mlmapping_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "apply_lds_driver.cpp"), "-o", str(exe)])

    def run(*args):
        out = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True).stdout
        return [tuple(int(x) for x in line.split()) for line in out.splitlines()]

    return run


def _geometry(cfg):
    """(edge, lv_nz, n) of a handle for batches of more than 8 frames (mlm_create's frame-local grid)."""
    lv_nz = math.ceil(cfg.n_z * cfg.am_d_Z / cfg.subbox_d_xyz) + 10
    sh = 3
    while sh > 0 and (lv_nz << (2 * sh)) > 4096:
        sh -= 1
    return 1 << sh, lv_nz, cfg.subbox_n


def test_apply_lds_layout(driver):
    rows = driver("sweep")
    assert len(rows) > 1000
    for edge, nz, n, occ, ztab, blk, total, bxy, bz in rows:
        nv = edge * edge * nz
        assert occ == 4 * nv                                  # log-odds
        assert ztab >= occ + nv and ztab % 4 == 0             # classes, then the layer table (the class clear writes whole words up to it)
        assert ztab - (occ + nv) < 4
        assert blk == ztab + 4 * nz
        assert total % 16 == 0 and total >= blk + 4 * bxy * bxy * bz  # every block a column may overlap has its entry
        cx, cz = (edge - 1) // n + 2, (nz - 1) // n + 2        # (the host's bound on the blocks an extent touches)
        assert total <= 5 * nv + 4 * nz + 4 * cx * cx * cz + 3 + 15


@pytest.mark.parametrize("cfg", [S1, S3, SDEF, CONFIG2_YAML], ids=["S1", "S3", "SDEF", "CONFIG2_YAML"])
def test_apply_lds_envelope(driver, cfg):
    edge, lv_nz, n = _geometry(cfg)
    (row,) = driver(edge, 2 * (lv_nz + 1), n)  # (mlm_create sizes for two grid heights; one layer of slack for the ceil)
    total, nv = row[-1], edge * edge * 2 * (lv_nz + 1)
    assert total <= 150 * 1024, (edge, lv_nz, n, total)
    assert total < 9 * nv + 16, (edge, lv_nz, n, total)


def _inputs(cfg, n_total, seed):
    """The bench's jittered room frames with random poses whose heights spread over about three grid heights."""
    from bench import make_inputs

    frames, q, t = make_inputs(cfg, 64, n_total, seed=seed)
    rng = np.random.default_rng(seed + 1)
    t = t.copy()
    t[:, 2] = rng.uniform(-6.0, 6.0, size=n_total)
    _, lv_nz, _ = _geometry(cfg)
    assert np.ptp(t[:64, 2]) > 2 * lv_nz * cfg.subbox_d_xyz  # (a batch's z origins lie further apart than one grid height)
    return frames, q, t


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,nb", [(S1, 2), (S3, 1)], ids=["cfg2", "cfg3"])
def test_batch64_wide_z_spread(cfg, nb):
    import torch

    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    B = 64
    frames, q, t = _inputs(cfg, B * nb, seed=7)
    d_frames = torch.from_numpy(frames.view(np.int16)).cuda()
    torch.cuda.synchronize()
    gpu = MLMap(cfg, max_blocks=64, max_points=cfg.width * cfg.height, max_batch=B)
    gpu.set_async(True)
    cpu = OracleMap(cfg)
    for j in range(nb):
        gpu.update_map_batch_dev(d_frames.data_ptr(), B, cfg.width, cfg.height, q[j * B:(j + 1) * B], t[j * B:(j + 1) * B])
        for k in range(j * B, (j + 1) * B):
            cpu.update_depth(frames[k % B], q[k], t[k])
        d = compare_maps(gpu.export_blocks(), cpu.export_blocks(), f"wide z spread, batch {j}")
        assert d["bit_mismatch"] == 0
    st = gpu.frame_stats()
    print("wide z spread", d, {k: st[k] for k in ("n_spec_replays", "n_sector_fallbacks", "n_pool_grows")})
    assert st["n_pool_grows"] >= 1
    # the grown map, one more batch with the heights in another order
    perm = np.random.default_rng(3).permutation(B)
    gpu.update_map_batch_dev(d_frames.data_ptr(), B, cfg.width, cfg.height, np.ascontiguousarray(q[perm]), np.ascontiguousarray(t[perm]))
    for k in range(B):
        cpu.update_depth(frames[k], q[perm[k]], t[perm[k]])
    assert compare_maps(gpu.export_blocks(), cpu.export_blocks(), "wide z spread, permuted batch")["bit_mismatch"] == 0
    gpu.close()
