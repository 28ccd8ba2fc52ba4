"""Kernel parameters fetched up front (k_bin_sectors stages its MlmDev / MlmFrame fields in registers at the kernel's start): what
can go wrong is a value taken too early or from the wrong slot, so every case changes parameters UNDER A LIVE HANDLE — slot sets that
come round again, lists and pool re-allocated between batches, two handles of different geometry fed alternately, handles with and
without the awareness read-back — and compares the map with the CPU oracle bit for bit.

Images are 96 x 64: 3 x 8 = 24 strips of 32 x 8 pixels, several strips per azimuth column and several columns per strip."""
import numpy as np
import pytest

from mlmapping_amd import synthetic as syn
from mlmapping_amd.config import S1
from tests.util import compare_maps

pytestmark = pytest.mark.gpu

W, H, B, N_BATCH = 96, 64, 2, 5
# S1's map behind a 96 x 64 camera (its vertical field of view narrowed so that most pixels stay inside the map's 4 m of height); noise
# at the edge of the odds table (3 sigma = 9.5 cells at the last rho), so that a speckle frame of 6 144 pixels leaves more unique hit
# cells (35 597 in the stream's fourth frame, by the oracle; a smooth frame leaves 20 000) than the 32 768 a need-sized list starts with; the stream needs 902 blocks
CFG_A = S1.with_(width=W, height=H, cam_cx=47.6, cam_cy=31.4, cam_fx=57.75, cam_fy=100.0, depth_noise_coe=0.0075)
# the 0.2 m / 5 degree map (config2.yaml's geometry, without its frontier mode)
CFG_B = S1.with_(width=W, height=H, cam_cx=47.6, cam_cy=31.4, cam_fx=57.75, cam_fy=57.75, am_d_Rho=0.2, am_d_Phi_deg=5.0, am_d_Z=0.2,
                 am_n_Rho=40, am_n_Z_below=20, am_n_Z_over=20, subbox_d_xyz=0.2)


def make_stream(cfg, n, seed):
    """n frames, each with a pose and a depth image of its own: speckle over the far half of the map's range; the first two frames and every
    third a smooth surface; a few holes"""
    rng = np.random.default_rng(seed)
    poses = syn.random_poses(n, seed=seed)
    far = int(1000 * cfg.am_n_Rho * cfg.am_d_Rho)
    out = []
    for k in range(n):
        if k < 2 or k % 3 == 2:  # (the first batch is smooth: the emulated hit container grows again in a later one)
            d = (0.55 * far + 0.1 * far * np.sin(np.arange(W) / 9.0 + k)[None, :] + 40.0 * np.arange(H)[:, None]).astype(np.uint16)
        else:
            d = rng.integers(int(far * 0.6), int(far * 0.95), size=(H, W)).astype(np.uint16)
        d[rng.random((H, W)) < 0.02] = 0
        out.append((d, poses[k][0], poses[k][1]))
    return out


@pytest.fixture(scope="module")
def mods():
    from mlmapping_amd.mlmap import MLMap
    from oracle.binding import OracleMap

    return MLMap, OracleMap


_ORACLE = {}


def oracle_map(OracleMap, cfg, frames, key):
    """the oracle's map after `frames` (computed once per stream, shared by the cases, never changed)"""
    if key not in _ORACLE:
        cpu = OracleMap(cfg)
        for img, q, t in frames:
            cpu.update_depth(img, q, t)
        _ORACLE[key] = cpu.export_blocks()
    return _ORACLE[key]


def feed(gpu, frames, k0):
    fr = frames[k0:k0 + B]
    gpu.update_map_batch(np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), np.stack([f[2] for f in fr]))


STREAM_A = make_stream(CFG_A, B * N_BATCH, 11)
STREAM_B = make_stream(CFG_B, B * N_BATCH, 12)


def test_slot_sets_come_round_again(mods, knobs):
    """asynchronous batches of 2 on a handle with three slot sets, five batches: every set is used, the first two twice; lists at their
    worst-case size (nothing is re-allocated on the way)"""
    MLMap, OracleMap = mods
    knobs.set("need_slots", 0)
    knobs.set("slot_sets", 3)
    gpu = MLMap(CFG_A, max_blocks=16384, max_points=W * H, max_batch=B)
    gpu.set_async(True)
    for k0 in range(0, B * N_BATCH, B):
        feed(gpu, STREAM_A, k0)
    compare_maps(gpu.export_blocks(), oracle_map(OracleMap, CFG_A, STREAM_A, "A"), "slot reuse")
    st = gpu.frame_stats()
    print({k: st[k] for k in ("n_slot_grows", "n_pool_grows", "n_spec_replays", "n_sector_fallbacks")})
    assert st["n_slot_grows"] == 0 and st["n_pool_grows"] == 0, st
    gpu.close()


@pytest.mark.parametrize("max_blocks", [16, 512])
def test_lists_and_pool_grow_between_batches(mods, knobs, max_blocks):
    """the same stream on a handle whose need-sized lists (32 768 unique hits) and block pool start too small: grow_slots and grow_pool
    re-allocate them between batches that are in flight — capacities and pointers change under the slot table — and the speckle frames of the second
    batch fill the emulated hit container past the bucket count the smooth first batch left (a rehash between batches)."""
    MLMap, OracleMap = mods
    knobs.set("slot_sets", 3)
    gpu = MLMap(CFG_A, max_blocks=max_blocks, max_points=W * H, max_batch=B)
    gpu.set_async(True)
    buckets1 = 0
    for k0 in range(0, B * N_BATCH, B):
        feed(gpu, STREAM_A, k0)
        if k0 == 0 and max_blocks == 512:  # (one case looks at the bucket count the smooth first batch leaves; the other never drains)
            gpu.sync()
            buckets1 = gpu.frame_stats()["hit_bucket_count"]
            assert buckets1 > 0
    compare_maps(gpu.export_blocks(), oracle_map(OracleMap, CFG_A, STREAM_A, "A"), f"growth, pool of {max_blocks}")
    st = gpu.frame_stats()
    print({k: st[k] for k in ("n_slot_grows", "n_pool_grows", "n_spec_replays", "n_sector_fallbacks", "hit_bucket_count", "block_capacity")}, buckets1)
    assert st["n_slot_grows"] >= 1 and st["n_pool_grows"] >= 1, st
    # the emulated hit container rehashed in a batch after the first: more buckets than the first batch left, and than 32 768 elements need
    assert st["hit_bucket_count"] > max(buckets1, 32768), (buckets1, st)
    gpu.close()


def test_two_handles_of_different_geometry_alternate(mods):
    """S1's map and the 0.2 m / 5 degree map on one GPU, their batches submitted alternately: each equals its own oracle"""
    MLMap, OracleMap = mods
    ga = MLMap(CFG_A, max_blocks=4096, max_points=W * H, max_batch=B)
    gb = MLMap(CFG_B, max_blocks=4096, max_points=W * H, max_batch=B)
    ga.set_async(True)
    gb.set_async(True)
    for k0 in range(0, B * N_BATCH, B):
        feed(ga, STREAM_A, k0)
        feed(gb, STREAM_B, k0)
    compare_maps(ga.export_blocks(), oracle_map(OracleMap, CFG_A, STREAM_A, "A"), "handle A (0.1 m / 1 degree)")
    compare_maps(gb.export_blocks(), oracle_map(OracleMap, CFG_B, STREAM_B, "B"), "handle B (0.2 m / 5 degrees)")
    ga.close()
    gb.close()


def test_handles_with_and_without_the_awareness_record_alternate(mods):
    """record_awareness is a limit of mlm_create (it sizes the miss-cell record: it cannot change on a live handle), so the two
    settings are two handles of one geometry, fed the same batches alternately: both maps equal the oracle's, and the recording
    handle's last frame reads back the oracle's hit and miss cells"""
    MLMap, OracleMap = mods
    rec = MLMap(CFG_A, max_blocks=4096, max_points=W * H, max_batch=B, record_awareness=True)
    plain = MLMap(CFG_A, max_blocks=4096, max_points=W * H, max_batch=B)
    cpu = OracleMap(CFG_A)
    for k0 in range(0, B * 2, B):
        feed(rec, STREAM_A, k0)
        feed(plain, STREAM_A, k0)
    for img, q, t in STREAM_A[:B * 2]:
        cpu.update_depth(img, q, t)
    want = cpu.export_blocks()
    compare_maps(rec.export_blocks(), want, "record_awareness on")
    compare_maps(plain.export_blocks(), want, "record_awareness off")
    gc, go, _ = rec.awareness_hits()
    cc, co = cpu.hit_cells_sorted()
    assert np.array_equal(gc, cc) and np.array_equal(go.view(np.uint32), co.view(np.uint32))
    assert np.array_equal(rec.awareness_misses(), np.sort(cpu.misses()).astype(np.int64))
    rec.close()
    plain.close()
